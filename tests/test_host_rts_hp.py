"""CPU: the host builds of the RTS smoother's one-lane arithmetic -- hc_rts (fk_math.hpp's rts_step: the full matrices of the
padded / rolled (16, 0) instantiation, and of the exact ones where FK_RTS_SYM = 0) and hc_rts_sym (fk_math_sym.hpp's
rts_step_sym: the packed upper triangles the exact instantiations of rts_kernels.hip run) -- against tests/rts_hp.py, the
reference's smoother in longdouble, on ill-conditioned models, held to the bar of tests/test_gpu_rts_precision.py (rts_hp.check:
MARGIN = 8 times the reference error of the float64 oracle, floor 1e-13).  The several-lane smoothers (rts_ml_9, rts_mlg.hip,
rts_mlx.hip) and the caller-supplied-inverse kernel have no host build: only the GPU file measures them.

Every condition the GPU file relies on is asserted here first, for every (family, dims, mode) it runs: the oracle finishes all 16
checked tracks within 1e-3 of the truth on all four outputs, and every one of the 150 tracks is further than 1e-3 from its
neighbour.  Each of those tests prints the oracle's and the reference's maxima; every host row prints err/bar, build/oracle and
ref/oracle.  docs/MEASUREMENTS.md ("RTS smoother precision") has the tables."""
import numpy as np
import pytest

import rts_hp
from test_hostcheck_math import hc_rts, hc_rts_sym

SYM_DIMS = [(2, 1), (4, 2), (6, 3), (8, 4), (9, 3)]
FULL_DIMS = SYM_DIMS + [(12, 3), (16, 8)]
# every (dims, mode) of tests/test_gpu_rts_precision.py
SHARED_DIMS = FULL_DIMS + [(13, 4), (14, 4)]
STEP_DIMS = [(4, 2), (9, 3), (12, 3)]
GIVEN_DIMS = [(6, 3), (12, 3)]
MODE_DIMS = [(n, m, "shared") for n, m in SHARED_DIMS] + [(n, m, mode) for n, m in STEP_DIMS for mode in ("class", "module")]
KEYS = [(f,) + k for f in rts_hp.FAMILIES for k in MODE_DIMS] + [("stiff", n, m, "given") for n, m in GIVEN_DIMS]


def host_run(fn, t):
    """the 16 checked tracks through one host build -> the four outputs, [16][12]... each"""
    out = [[] for _ in rts_hp.OUTPUTS]
    for trk in t["model"]["tracks"]:
        res = fn(t["Xs"][:, trk], t["Ps"][:, trk], t["F"], t["Q"])
        assert res[-1] == 0, (trk, res[-1])
        for lst, a in zip(out, res[:4]):
            lst.append(a)
    return [np.array(a) for a in out]


def test_longdouble_is_extended_precision():
    assert np.finfo(np.longdouble).eps < 2e-19


@pytest.mark.parametrize("n,m,mode", MODE_DIMS)
def test_the_truth_is_a_truth(n, m, mode):
    """on the benign family the float64 oracle and the longdouble smoother agree to 1e-13 on all four outputs of every checked
    track, with shared and with per-step models in either index convention; the last step is the filter's own, its gain zero"""
    t = rts_hp.truth("benign", n, m, mode)
    rts_hp.measures_something(t)
    assert t["eo"].max() < 1e-13, t["eo"].max(axis=1)
    trk = list(t["model"]["tracks"])
    assert not t["hp"][2][:, -1].any()
    assert np.array_equal(t["hp"][0][:, -1], t["Xs"][-1, trk]) and np.array_equal(t["hp"][1][:, -1], t["Ps"][-1, trk])
    assert np.array_equal(t["hp"][3][:, -1], t["Ps"][-1, trk])


def test_the_two_conventions_differ():
    """the per-step models change enough from step to step that taking Fs[k] for Fs[k+1] is seen: the class's and the module
    function's smoothed means are further apart than 1e-3 on every checked track"""
    for n, m in STEP_DIMS:
        a, b = rts_hp.truth("stiff", n, m, "class"), rts_hp.truth("stiff", n, m, "module")
        assert np.array_equal(a["Xs"], b["Xs"]) and np.array_equal(a["F"], b["F"])
        assert min(rts_hp.err(a["hp"][0][i], b["hp"][0][i]) for i in range(16)) > 1e-3


@pytest.mark.parametrize("family,n,m,mode", KEYS, ids=["%s-%d-%d-%s" % k for k in KEYS])
def test_models_measure_something(family, n, m, mode):
    """the condition of the precision tests, on the CPU for every model, dims and mode the GPU file uses: all 16 tracks finish in
    the oracle and in its perturbed runs, err(oracle, hp) < 1e-3 on all four outputs, and -- the lane condition, on ALL 150
    tracks -- every track's smoothed means are further than 1e-3 from its neighbour's"""
    t = rts_hp.truth(family, n, m, mode)
    rts_hp.measures_something(t)
    print(family, (n, m), mode, "oracle max", " ".join("%s %.1e" % (k, v) for k, v in zip(rts_hp.OUTPUTS, t["eo"].max(axis=1))),
          "| ref max", " ".join("%s %.1e" % (k, v) for k, v in zip(rts_hp.OUTPUTS, t["ref"].max(axis=1))))
    hp, N = t["hp_all"], t["model"]["N"]
    assert N == 150 == len(hp)
    apart = [rts_hp.err(hp[i], hp[(i + 1) % N]) for i in range(N)]
    assert min(apart) > 1e-3, (int(np.argmin(apart)), min(apart))
    own, other = rts_hp.lanes(hp, t)
    assert own == 0.0 and other == min(apart)


def test_supplied_inverses_are_the_rounded_truth():
    """mode "given": the inverses handed to everybody are float64, those of the longdouble Pp, and the truth's Pp is the plain
    recursion's (Pp[k] is a function of the inputs alone)"""
    for n, m in GIVEN_DIMS:
        g, s = rts_hp.truth("stiff", n, m, "given"), rts_hp.truth("stiff", n, m, "shared")
        assert g["invs"].dtype == np.float64 and g["invs"].shape == g["Ps"].shape and not g["invs"][-1].any()
        assert np.array_equal(g["hp"][3], s["hp"][3]) and np.array_equal(g["Xs"], s["Xs"])
        trk = g["model"]["tracks"][3]
        resid = rts_hp.ld(g["invs"][0, trk]) @ g["hp"][3][3][0] - np.eye(n)
        assert np.abs(resid).max() < 1e-6, np.abs(resid).max()              # cond(Pp) ~ 1e8 times the float64 rounding


def _hold(label, fn, family, n, m):
    t = rts_hp.truth(family, n, m)
    rts_hp.measures_something(t)
    eg = rts_hp.errors(host_run(fn, t), t["hp"])
    for name, eb, bo, ro in rts_hp.ratios(eg, t):
        print("%-6s %-20s (%d,%d) %-3s err/bar %.3f  build/oracle %6.2f  ref/oracle %6.2f" % (label, family, n, m, name, eb, bo, ro))
    return rts_hp.check(f"{label} {family} ({n},{m})", eg, t)


@pytest.mark.parametrize("n,m", FULL_DIMS)
@pytest.mark.parametrize("family", rts_hp.FAMILIES)
def test_full_host_build_meets_the_bar(family, n, m):
    bad = _hold("full", hc_rts, family, n, m)
    assert not bad, bad


@pytest.mark.parametrize("n,m", SYM_DIMS)
@pytest.mark.parametrize("family", rts_hp.FAMILIES)
def test_packed_symmetric_host_build_meets_the_bar(family, n, m):
    bad = _hold("packed", hc_rts_sym, family, n, m)
    assert not bad, bad
