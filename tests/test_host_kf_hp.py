"""CPU: the host builds of the Kalman filter kernels' templates -- hc_kf_batch (fk_math.hpp: the full arithmetic of kf_kernels.hip
and of kf_fast's SYM = 0 instantiations, exact, padded and (16,8)) and hc_kf_batch_sym (fk_math_sym.hpp: the packed-symmetric
arithmetic kf_fast runs where SYM = 1) -- against tests/kf_hp.py, the reference's algorithm in longdouble, on ill-conditioned
models, held to the bar of tests/test_gpu_kf_precision.py (kf_hp.check: MARGIN = 8 times the reference error of the float64
oracle, floor 1e-13).  The several-lane kernels (kf_ml.hip, kf_mlg.hip) have no host build: only the GPU file measures them.

Every row prints err/bar, build/oracle and ref/oracle; docs/MEASUREMENTS.md ("KF precision") has the table."""
import numpy as np
import pytest

import kf_hp
from test_hostcheck_math import hc_batch, hc_batch_sym

# every (dim_x, dim_z) the GPU file runs: exact (2,1) (4,2) (6,3) (9,3) (8,4), padded (5,4) in (6,6), (9,4) (12,3) (16,8) in (16,8)
DIMS = [(2, 1), (4, 2), (5, 4), (6, 3), (8, 4), (9, 3), (9, 4), (12, 3), (16, 8)]
SYM_DIMS = [(2, 1), (4, 2), (6, 3), (7, 4), (8, 4), (9, 3), (9, 4)]


def host_run(fn, t):
    """the 16 checked tracks through one host build -> the four forward outputs, [16][T]... each"""
    M = t["model"]
    out = [[] for _ in range(4)]
    for trk in M["tracks"]:
        res = fn(M["x0"][trk], M["P0"][trk], M["zs"][:, trk], M["F"], M["Q"], M["H"], M["R"], mask=M["mask"])
        assert res[-1] == 0, (trk, res[-1])
        for lst, a in zip(out, res[:4]):
            lst.append(a)
    return [np.array(a) for a in out]


def test_longdouble_is_extended_precision():
    assert np.finfo(np.longdouble).eps < 2e-19


@pytest.mark.parametrize("n,m", DIMS + [(7, 4)])
def test_the_truth_is_a_truth(n, m):
    """on the benign family the float64 oracle and the longdouble filter agree to 1e-13 on all eight outputs of every checked
    track, a missing measurement included (y = 0; K, S, SI keep their last values)"""
    t = kf_hp.truth("benign", n, m)
    kf_hp.measures_something(t)
    assert t["eo"][:7].max() < 1e-13, t["eo"].max(axis=1)
    M = t["model"]
    # y = z - H x is a difference: where the prediction is good it cancels (|y| << |z|), and its error relative to |y| says how
    # far it cancelled, not how wrong either filter is -- so y agrees to 1e-13 of its OPERANDS, max(|z|, |H x|) per step
    # (relative to |y| itself the worst benign track reaches 4e-13 at (2,1))
    for k, trk in enumerate(M["tracks"]):
        y, z = t["hp"][7][k], kf_hp.ld(M["zs"][:, trk]) * M["mask"][:, None]
        scale = np.maximum(np.abs(z).max(axis=1), np.abs(z - y).max(axis=1))
        assert np.all(np.abs(kf_hp.ld(t["oracle"][7][k]) - y).max(axis=1) <= 1e-13 * scale), (trk,)
    assert not M["mask"][kf_hp.ukf_hp.T_MISSING] and M["mask"].sum() == M["T"] - 1
    s = kf_hp.ukf_hp.T_MISSING
    assert not t["hp"][7][:, s].any() and np.array_equal(t["hp"][4][:, s], t["hp"][4][:, s - 1])
    assert np.array_equal(t["hp"][0][:, s], t["hp"][2][:, s]) and np.array_equal(t["hp"][1][:, s], t["hp"][3][:, s])


@pytest.mark.parametrize("n,m,masked", [(n, m, True) for n, m in DIMS + [(7, 4)]] + [(9, 3, False), (12, 3, False)])
@pytest.mark.parametrize("family", kf_hp.FAMILIES)
def test_models_measure_something(family, n, m, masked):
    """the condition of the precision tests, on the CPU for every model and dims they use, with the missing step and (for the
    four-lane histories) without: all 16 tracks finish in the oracle and in its perturbed runs, err(oracle, hp) < 1e-3 on all
    eight outputs (K, S, SI and y too), and the neighbour of every checked track is another track"""
    t = kf_hp.truth(family, n, m, masked)
    kf_hp.measures_something(t)
    print(family, (n, m), "oracle max", " ".join("%s %.1e" % (k, v) for k, v in zip(kf_hp.OUTPUTS, t["eo"].max(axis=1))),
          "| ref/oracle max %.1f" % (t["ref"].max(axis=1) / np.maximum(t["eo"].max(axis=1), 1e-300)).max())
    assert kf_hp.not_the_neighbour(t["hp"][0], t) and kf_hp.not_the_neighbour(t["oracle"][0], t)


def _hold(label, fn, family, n, m):
    t = kf_hp.truth(family, n, m)
    kf_hp.measures_something(t)
    eg = np.full((len(kf_hp.OUTPUTS), 16), np.nan)
    eg[kf_hp.FORWARD] = kf_hp.errors(host_run(fn, t), t["hp"][kf_hp.FORWARD])
    for name, eb, bo, ro in kf_hp.ratios(eg, t):
        print("%-6s %-20s (%d,%d) %-8s err/bar %.3f  build/oracle %6.2f  ref/oracle %6.2f" % (label, family, n, m, name, eb, bo, ro))
    return kf_hp.check(f"{label} {family} ({n},{m})", eg, t)


@pytest.mark.parametrize("n,m", DIMS)
@pytest.mark.parametrize("family", kf_hp.FAMILIES)
def test_full_host_build_meets_the_bar(family, n, m):
    bad = _hold("full", hc_batch, family, n, m)
    assert not bad, bad


@pytest.mark.parametrize("n,m", SYM_DIMS)
@pytest.mark.parametrize("family", kf_hp.FAMILIES)
def test_packed_symmetric_host_build_meets_the_bar(family, n, m):
    bad = _hold("packed", hc_batch_sym, family, n, m)
    assert not bad, bad
