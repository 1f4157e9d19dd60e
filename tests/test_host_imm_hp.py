"""CPU: the host build of the IMM / MMAE arithmetic -- hc_imm_batch (tests/hostcheck/hostcheck.cpp: fk_imm.hpp, the per-track
arithmetic of imm_kernels.hip, and through its (9,4) instantiations the per-filter arithmetic of imm_lanes.hip, "same operations,
same order") -- against tests/imm_hp.py, the reference's IMMEstimator / MMAEFilterBank in longdouble, on stiff banks, held to the
bar of tests/test_gpu_imm_precision.py (imm_hp.check: 8 times the reference error of the float64 oracle, floor 1e-13).  The
four-lane kernel (imm_quad.hip) has no host build: only the GPU file measures it.  hc_imm_batch takes no mask: the banks with a
missing measurement are the GPU file's too.

Every row prints err/bar, the oracle's error, ref and the build's error; docs/MEASUREMENTS.md ("IMM precision") has the table."""
import ctypes

import numpy as np
import pytest

import imm_hp
from test_hostcheck_imm import _p, lib

# (kind, dim_x, dim_z, n_models): classes (2,1) (4,2) (6,3) of imm_kernels.hip; (9,3) x 4 and (8,4) x 4 padded into (9,4) x 4;
# (9,4) x 2 and x 8: the group widths G = 2 and G = 8 of imm_lanes.hip
HOST_BANKS = [("imm", 2, 1, 3), ("imm", 4, 2, 2), ("imm", 6, 3, 3), ("imm", 9, 3, 4), ("imm", 8, 4, 4), ("imm", 9, 4, 2), ("imm", 9, 4, 8),
              ("mmae", 6, 3, 2), ("mmae", 9, 3, 4)]
# every bank of tests/test_gpu_imm_precision.py: (kind, dim_x, dim_z, n_models, step 8 missing)
GPU_BANKS = [("imm", 2, 1, 3, False), ("imm", 4, 2, 2, False), ("imm", 6, 3, 3, False), ("mmae", 6, 3, 2, False), ("imm", 4, 2, 3, True),
             ("imm", 9, 4, 2, False), ("imm", 9, 3, 4, False), ("imm", 8, 4, 4, False), ("imm", 9, 4, 8, False), ("imm", 4, 2, 13, False),
             ("mmae", 9, 3, 4, False), ("imm", 9, 4, 8, True),
             ("imm", 12, 3, 2, False), ("imm", 14, 4, 3, False), ("imm", 16, 8, 2, False), ("mmae", 12, 3, 2, False), ("imm", 14, 4, 3, True)]
# benign, the control: one bank per kernel file (imm_kernels.hip, imm_lanes.hip, imm_quad.hip)
BENIGN = [("imm", 6, 3, 3, False), ("imm", 9, 4, 2, False), ("imm", 12, 3, 2, False)]


def host_run(t, fn=None):
    """the 16 checked tracks through the host build -> the nine arrays of imm_hp.OUTPUTS, [16]... each (None: MMAE's priors)"""
    B, mmae = t["model"], t["kind"] == "mmae"
    n, m, nm, T = B["n"], B["m"], B["nm"], B["T"]
    c = lambda a: np.ascontiguousarray(a, dtype=np.float64)  # noqa: E731
    fn = fn or lib().hc_imm_batch
    out = [[] for _ in imm_hp.OUTPUTS]
    for trk in B["tracks"]:
        xs, Ps, mu = c(B["xs0"][trk]).copy(), c(B["Ps0"][trk]).copy(), c(B["mu0"][trk]).copy()
        x, P, MU = np.zeros((T, n)), np.zeros((T, n, n)), np.zeros((T, nm))
        xp, Pp, L = np.zeros((T, n)), np.zeros((T, n, n)), np.zeros((T, nm))
        st = fn(n, m, nm, ctypes.c_long(T), _p(c(B["Fs"])), _p(c(B["Qs"])), _p(c(B["Hs"])), _p(c(B["Rs"])),
                _p(c(np.eye(nm)) if mmae else c(B["M"])), _p(c(B["zs"][:, trk])), _p(xs), _p(Ps), _p(mu), _p(x), _p(P), _p(MU),
                _p(xp), _p(Pp), _p(L), int(mmae))
        assert st == 0, (trk, st)
        for lst, a in zip(out, (x, P, MU, None if mmae else xp, None if mmae else Pp, L, xs, Ps, mu[None])):
            lst.append(a)
    return [None if v[0] is None else np.array(v) for v in out]


def hold(label, got, t):
    """print one row per output, then the bar -> the failures; the floor must have been kept"""
    eg, floor_ok = imm_hp.errors(got, t)
    B = t["model"]
    for name, eb, eo, ref, e in imm_hp.ratios(eg, t):
        print("%-5s %-4s %-20s (%d,%d)x%d %-8s err/bar %.3f  oracle %.2e  ref %.2e  build %.2e" % (
            label, t["kind"], B["family"], B["n"], B["m"], B["nm"], name, eb, eo, ref, e))
    assert floor_ok, "a likelihood whose truth is below 1e-330 is not DBL_MIN"
    return imm_hp.check(f"{label} {t['kind']} {B['family']} ({B['n']},{B['m']})x{B['nm']}", eg, t)


def test_longdouble_is_extended_precision():
    assert np.finfo(np.longdouble).eps < 2e-19


@pytest.mark.parametrize("kind,n,m,nm,masked", BENIGN + [("mmae", 6, 3, 2, False), ("imm", 4, 2, 3, True)])
def test_the_truth_is_a_truth(kind, n, m, nm, masked):
    """on the benign family the float64 oracle and the longdouble bank agree to 1e-12 on every output of every checked track
    (the likelihoods and mode probabilities pass through an exponential of a quadratic form of ~10: a few more ulps than the
    Kalman filter's 1e-13), a missing measurement included: x and P of that step are the priors, the likelihood the density of
    a zero residual"""
    t = imm_hp.truth(kind, "benign", n, m, nm, masked)
    imm_hp.measures_something(t)
    assert np.nanmax(t["eo"]) < 1e-12, np.nanmax(t["eo"], axis=1)
    if masked:
        s = imm_hp.ukf_hp.T_MISSING
        B = t["model"]
        assert not B["mask"][s] and B["mask"].sum() == B["T"] - 1
        # a zero residual under the S of step s - 1: the density's peak, so no smaller than that step's own likelihood
        assert np.all(t["raw"][:, s] >= t["raw"][:, s - 1]) and np.all(t["hp"][5][:, s] == t["raw"][:, s])


@pytest.mark.parametrize("kind,n,m,nm,masked", GPU_BANKS)
@pytest.mark.parametrize("family", imm_hp.STIFF)
def test_banks_measure_something(family, kind, n, m, nm, masked):
    """the condition of the precision tests, on the CPU for every bank the GPU file runs"""
    t = imm_hp.truth(kind, family, n, m, nm, masked)
    imm_hp.measures_something(t)
    print(family, kind, (n, m, nm), "missing" if masked else "", "left out %d of %d  worst best-model L %.1e  second mode > 1e-3: %.2f" % imm_hp.stats(t),
          "| oracle max %.1e ref max %.1e" % (np.nanmax(t["eo"]), np.nanmax(t["ref"])))
    assert imm_hp.not_the_neighbour(t["hp"][0], t) and imm_hp.not_the_neighbour(t["oracle"][0], t)


@pytest.mark.parametrize("kind,n,m,nm", HOST_BANKS)
@pytest.mark.parametrize("family", imm_hp.STIFF)
def test_host_build_meets_the_bar(family, kind, n, m, nm):
    t = imm_hp.truth(kind, family, n, m, nm)
    imm_hp.measures_something(t)
    got = host_run(t)
    bad = hold("host", got, t)
    assert not bad, bad
    assert imm_hp.not_the_neighbour(got[0], t)


@pytest.mark.parametrize("kind,n,m,nm", [b[:4] for b in BENIGN[:2]])
def test_host_build_meets_the_bar_on_the_benign_control(kind, n, m, nm):
    t = imm_hp.truth(kind, "benign", n, m, nm)
    imm_hp.measures_something(t)
    bad = hold("host", host_run(t), t)
    assert not bad, bad
