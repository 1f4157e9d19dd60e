"""The information filter on the GPU (fk_info_*_f64, csrc/info_kernels.hip) against the goldens frozen from the live reference:
every case through InformationFilter and through InformationFilterBank in both layouts; banks with a tail workgroup against
tests/info_port.py; the fast kernels against the general one (forced in a child process); chained calls bit-identical to one;
the bank against KalmanFilterBank on the same model; a singular P_inv; the control input."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, golden, rel_err
import info_port as ip
from filterpy_amd.kalman import InformationFilter, InformationFilterBank, KalmanFilterBank

pytestmark = pytest.mark.gpu

G = golden("info")
NC = int(G["n_cases"])
TOL = 1e-10


def check_attrs(c, k, f, n, m, track=None):
    """x, P_inv, K and y of object f after call k of case c"""
    pick = (lambda a: np.asarray(a, dtype=float)) if track is None else (lambda a: np.asarray(a, dtype=float)[track])
    g = lambda a: ip.attr(G, c["p"], k, a)                                     # noqa: E731
    assert rel_err(np.ravel(pick(f.x)), np.ravel(g("x"))) <= TOL, (k, "x")
    assert rel_err(pick(f.P_inv), g("P_inv")) <= TOL, (k, "P_inv")
    if np.any(g("K") != 0):
        assert rel_err(pick(f.K), g("K")) <= TOL, (k, "K")
        assert rel_err(np.ravel(pick(f.y)), np.ravel(g("y"))) <= TOL, (k, "y")


@pytest.mark.parametrize("ci", range(NC))
def test_golden_cases_single_and_bank(ci):
    c = ip.case(G, ci)
    n, m = c["n"], c["m"]
    lik = ip.has_likelihood(n, m)
    f = ip.setup(InformationFilter(n, m, compute_log_likelihood=lik), c)
    for k, op in enumerate(c["ops"]):
        ip.run_op(f, c, k, op)
        check_attrs(c, k, f, n, m)
        for a in ip.ATTRS:
            if a in ("log_likelihood", "likelihood") and not lik:
                continue
            ref, mine = ip.attr(G, c["p"], k, a), np.asarray(getattr(f, a), dtype=float)
            assert mine.shape == ref.shape and rel_err(mine, ref) <= TOL, (k, a)
    Nt = 3
    for layout in ("soa", "aos"):
        b = InformationFilterBank(n, m, Nt, layout=layout)
        b.F, b.H, b.Q, b.R_inv, b.P_inv = c["F"], c["H"], c["Q"], c["Rinv"], c["Pinv0"]
        b.x = np.tile(c["x0"], (Nt, 1))
        if "B" in c:
            b.B = c["B"]
        for k, op in enumerate(c["ops"]):
            z = np.tile(c["zs"][k], (Nt, 1))
            if op == ip.PREDICT:
                b.predict()
            elif op == ip.PREDICT_U:
                b.predict(np.tile(c["us"][k], (Nt, 1)))
            elif op == ip.UPDATE:
                b.update(z)
            elif op == ip.UPDATE_RINV:
                b.update(z, R_inv=c["Rinv2"])
            elif op == ip.UPDATE_RINV_SCALAR:
                b.update(z, R_inv=ip.RINV_SCALAR)
            for i in range(Nt):
                check_attrs(c, k, b, n, m, track=i)


def test_reference_test_model():
    """the model of the reference's test_1d / test_against_kf: scalar measurements, update then predict"""
    f = InformationFilter(dim_x=2, dim_z=1)
    f.x = np.array([[2.], [0.]])
    f.F = np.array([[1., 1.], [0., 1.]])
    f.H = np.array([[1., 0.]])
    f.R_inv *= 1. / 5
    f.Q *= 0.0001
    for k in range(30):
        f.update(float(G["t_zs"][k]))
        for a in ip.ATTRS:
            assert rel_err(np.asarray(getattr(f, a), dtype=float), ip.attr(G, "t_", 2 * k, a)) <= TOL, (k, a)
        f.predict()
        for a in ("x", "P_inv", "x_prior", "P_inv_prior"):
            assert rel_err(np.asarray(getattr(f, a), dtype=float), ip.attr(G, "t_", 2 * k + 1, a)) <= TOL, (k, a)


def _bank(n, m, Nt, T, seed, layout):
    """a benign model (condition numbers of a few units), as tests/test_gpu_srkf.py's"""
    rs = np.random.RandomState(seed)
    A = rs.randn(n, n)
    b = InformationFilterBank(n, m, Nt, layout=layout)
    b.F, b.H = np.eye(n) + 0.1 * rs.randn(n, n) / np.sqrt(n), rs.randn(m, n)
    b.Q, b.R_inv = 0.01 * (A @ A.T + np.eye(n)), np.eye(m) * 1.25
    b.x = rs.randn(Nt, n)
    b.P_inv = np.eye(n)[None] / (1.0 + rs.rand(Nt, 1, 1))
    return b, rs.randn(T, Nt, m)


@pytest.mark.parametrize("update_first", [False, True])
@pytest.mark.parametrize("layout", ["soa", "aos"])
@pytest.mark.parametrize("dims", [(4, 2), (7, 3)])          # the fast kernel; the first shape that falls to the general one
def test_bank_with_tail_vs_port(layout, dims, update_first):
    n, m = dims
    Nt, T = 2 * 256 + 65, 8
    b, zs = _bank(n, m, Nt, T, 11, layout)
    mask = np.ones((T, Nt), dtype=bool)
    mask[3, 1::7] = False
    mask[3, [0, 63, 256, Nt - 1]] = False
    zs[5, [64, 255, Nt - 2]] = np.nan
    x0, P0 = b.x.copy(), b.P_inv.copy()
    out = b.batch_filter(zs, mask=mask, update_first=update_first)
    assert np.array_equal(b.x, x0) and np.array_equal(b.P_inv, P0)
    keep = mask & ~np.isnan(zs).any(axis=2)
    for i in (0, 63, 64, 255, 256, Nt - 2, Nt - 1):
        r = ip.batch(x0[i], P0[i], np.nan_to_num(zs[:, i]), b.F, b.Q, b.H, b.R_inv, mask=keep[:, i], update_first=update_first)
        for got, want in zip(out, r[:4]):
            assert rel_err(got[:, i], want) <= TOL, i
    want = ip.batch_tracks(x0, P0, np.nan_to_num(zs), b.F, b.Q, b.H, b.R_inv, mask=keep, update_first=update_first)
    for got, w in zip(out, want):
        assert rel_err(got, w) <= TOL                       # ... and every other track, against the vectorised port


FAST = [(a, c) for a in range(1, 5) for c in range(1, a + 1)] + [(a, c) for a in (5, 6) for c in (1, 2, 3)]

CHILD = r'''
import sys, numpy as np
sys.path.insert(0, %r); sys.path.insert(0, %r)
from test_gpu_info import _bank, FAST
out = {}
for n, m in FAST:
    for layout in ("soa", "aos"):
        b, zs = _bank(n, m, 300, 6, n * 10 + m, layout)
        zs[2, 5::11] = np.nan
        for uf in (False, True):
            r = b.batch_filter(zs, update_first=uf)
            for j, a in enumerate(r):
                out["%%d_%%d_%%s_%%d_%%d" %% (n, m, layout, uf, j)] = a
np.savez(sys.argv[1], **out)
'''


def test_fast_list_is_the_compiled_one():
    import re
    src = open(os.path.join(ROOT, "filterpy_amd", "csrc", "fk_dims_info.def")).read()
    assert sorted(FAST) == sorted((int(a), int(c)) for a, c in re.findall(r"^FK_INFO_INST\((\d+),\s*(\d+)\)", src, re.M))


def test_fast_and_general_kernels_agree(tmp_path):
    outs = {}
    for forced in ("0", "1"):
        env = dict(os.environ, FK_INFO_GENERAL=forced)
        path = str(tmp_path / ("o%s.npz" % forced))
        r = subprocess.run([sys.executable, "-c", CHILD % (ROOT, os.path.join(ROOT, "tests")), path], env=env,
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        outs[forced] = np.load(path)
    assert len(outs["0"].files) == len(FAST) * 2 * 2 * 4
    for k in outs["0"].files:
        assert rel_err(outs["0"][k], outs["1"][k]) <= 1e-12, k


@pytest.mark.parametrize("layout", ["soa", "aos"])
@pytest.mark.parametrize("dims", [(4, 2), (9, 3)])
def test_chained_calls_bit_identical(layout, dims):
    n, m = dims
    T, split = 12, 5
    b, zs = _bank(n, m, 333, T, 5, layout)
    mask = np.ones((T, 333), dtype=bool)
    mask[split - 1, ::3] = False                            # a missing measurement at the step before the split
    zs[split - 1, 1::3] = np.nan
    x0, P0 = b.x.copy(), b.P_inv.copy()
    one = b.batch_filter(zs, mask=mask)
    first = b.batch_filter(zs[:split], mask=mask[:split])
    b.x, b.P_inv = first[0][-1], first[1][-1]
    second = b.batch_filter(zs[split:], mask=mask[split:])
    for a, p, q in zip(one, first, second):
        assert np.array_equal(a, np.concatenate([p, q]))
    b.x, b.P_inv = x0, P0
    for t in range(T):                                      # predict / update steps: the same kernels, one phase each
        b.predict()
        assert rel_err(b.x, one[2][t]) <= 1e-13 and rel_err(b.P_inv, one[3][t]) <= 1e-13
        b.update(zs[t], mask=mask[t])
        assert rel_err(b.x, one[0][t]) <= 1e-13 and rel_err(b.P_inv, one[1][t]) <= 1e-13


@pytest.mark.parametrize("dims", [(4, 2), (6, 3)])
def test_bank_agrees_with_kalman_filter_bank(dims):
    n, m = dims
    Nt, T = 500, 20
    b, zs = _bank(n, m, Nt, T, 21, "soa")
    kf = KalmanFilterBank(n, m, Nt)
    kf.F, kf.H, kf.Q, kf.R, kf.x, kf.P = b.F, b.H, b.Q, np.linalg.inv(b.R_inv), b.x.copy(), np.linalg.inv(b.P_inv)
    mu, cov, mu_p, cov_p = kf.batch_filter(zs)[:4]
    imu, icov, imu_p, icov_p = b.batch_filter(zs)
    assert rel_err(imu, mu) <= 1e-9 and rel_err(imu_p, mu_p) <= 1e-9
    assert rel_err(np.linalg.inv(icov), cov) <= 1e-8 and rel_err(np.linalg.inv(icov_p), cov_p) <= 1e-8


def test_no_information_raises():
    """P_inv = 0: the status array says so (nothing faults), single filter and bank, fast and general shapes"""
    f = InformationFilter(2, 1)
    f.F, f.H = np.array([[1., 1.], [0., 1.]]), np.array([[1., 0.]])
    f.P_inv = np.zeros((2, 2))
    with pytest.raises(np.linalg.LinAlgError):
        f.predict()
    for n, m in ((4, 2), (7, 3)):
        for layout in ("soa", "aos"):
            b, zs = _bank(n, m, 70, 3, 2, layout)
            Pi = b.P_inv.copy()
            Pi[[3, 64, 69]] = 0.0
            b.P_inv = Pi
            with pytest.raises(np.linalg.LinAlgError):
                b.batch_filter(zs)
            with pytest.raises(np.linalg.LinAlgError):
                b.predict()
    b, zs = _bank(4, 2, 70, 3, 2, "soa")
    b.batch_filter(zs)                                      # the same bank with information: no error


@pytest.mark.parametrize("layout", ["soa", "aos"])
def test_control_input_both_forms(layout):
    rs = np.random.RandomState(2)
    n, m, Nt, T = 4, 2, 50, 8
    b, zs = _bank(n, m, Nt, T, 9, layout)
    for B, nu in ((rs.randn(n, 3), 3), (0.5, n)):           # a matrix B; the scalar B (b u, u of dim_x entries)
        b.B = B
        us = rs.randn(T, Nt, nu)
        out = b.batch_filter(zs, us=us)
        Bm = B if np.ndim(B) else np.eye(n) * B
        want = ip.batch_tracks(b.x, b.P_inv, zs, b.F, b.Q, b.H, b.R_inv, B=Bm, us=us)
        for got, w in zip(out, want):
            assert rel_err(got, w) <= TOL
    f = InformationFilter(n, m, compute_log_likelihood=False)
    f.F, f.H, f.Q, f.R_inv, f.B = b.F, b.H, b.Q, b.R_inv, rs.randn(n, 3)
    f.x = rs.randn(n)
    x0, u = f.x.copy(), rs.randn(3)
    f.predict(u)
    x, Pi = ip.predict(x0, np.eye(n), b.F, b.Q, f.B, u)
    assert rel_err(f.x, x) <= TOL and rel_err(f.P_inv, Pi) <= TOL
