"""The square-root Kalman filter on the GPU (fk_srkf_*_f64, csrc/srkf_kernels.hip) against the goldens frozen from the live
reference: every case through SquareRootKalmanFilter and through SquareRootKalmanFilterBank in both layouts; 70 001-track banks
against tests/srkf_port.py; the fast kernels against the general one (forced in a child process); chained calls bit-identical
to one; the bank against KalmanFilterBank on the same model."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, golden, rel_err
import srkf_port as sp
from filterpy_amd.kalman import KalmanFilterBank, SquareRootKalmanFilter, SquareRootKalmanFilterBank

pytestmark = pytest.mark.gpu

G = golden("srkf")
NC = int(G["n_cases"])
TOL = 1e-10


def check_attrs(c, k, f, track=None):
    """x, P1_2 (exact signs), K, y, S, SI and P of object f after call k of case c"""
    pick = (lambda a: np.asarray(a, dtype=float)) if track is None else (lambda a: np.asarray(a, dtype=float)[track])
    g = lambda a: sp.attr(G, c["p"], k, a)                                     # noqa: E731
    x, L = pick(f.x), pick(f._P1_2)
    assert rel_err(np.ravel(x), np.ravel(g("x"))) <= TOL, (k, "x")
    assert rel_err(L, g("_P1_2")) <= TOL, (k, "P1_2")
    assert np.array_equal(np.sign(np.diag(L)), np.sign(np.diag(g("_P1_2")))), (k, "signs of P1_2")
    assert rel_err(L @ L.T, g("_P1_2") @ g("_P1_2").T) <= TOL, (k, "P")
    if np.any(g("K") != 0):
        S12, SI12 = pick(f.S1_2), pick(f.SI1_2)
        assert rel_err(pick(f.K), g("K")) <= TOL, (k, "K")
        assert rel_err(np.ravel(pick(f.y)), np.ravel(g("y"))) <= TOL, (k, "y")
        assert rel_err(S12 @ S12.T, g("S1_2") @ g("S1_2").T) <= TOL, (k, "S")
        assert rel_err(SI12.T @ SI12, g("SI1_2").T @ g("SI1_2")) <= TOL, (k, "SI")
        assert np.array_equal(np.sign(np.diag(S12)), np.sign(np.diag(g("S1_2")))), (k, "signs of S1_2")


@pytest.mark.parametrize("ci", range(NC))
def test_golden_cases_single_and_bank(ci):
    c = sp.case(G, ci)
    n, m = c["n"], c["m"]
    f = sp.setup(SquareRootKalmanFilter(n, m), c)
    for k, op in enumerate(c["ops"]):
        sp.run_op(f, c, k, op)
        check_attrs(c, k, f)
        for a in ("x_prior", "x_post", "_P1_2_prior", "_P1_2_post", "M"):
            assert rel_err(np.asarray(getattr(f, a), dtype=float), sp.attr(G, c["p"], k, a)) <= TOL, (k, a)
    Nt = 3
    for layout in ("soa", "aos"):
        b = SquareRootKalmanFilterBank(n, m, Nt, layout=layout)
        b.F, b.H, b.Q, b.R, b.P = c["F"], c["H"], c["Q"], c["R"], c["P0"]
        b.x = np.tile(c["x0"], (Nt, 1))
        if "B" in c:
            b.B = c["B"]
        for k, op in enumerate(c["ops"]):
            z = np.tile(c["zs"][k], (Nt, 1))
            if op == sp.PREDICT:
                b.predict()
            elif op == sp.PREDICT_U:
                b.predict(np.tile(c["us"][k], (Nt, 1)))
            elif op == sp.UPDATE:
                b.update(z)
            elif op == sp.UPDATE_R2:
                b.update(z, R2=c["R2"])
            elif op == sp.UPDATE_R2_SCALAR:
                b.update(z, R2=sp.R2_SCALAR)
            for i in range(Nt):
                check_attrs(c, k, b, track=i)


def test_reference_test_model():
    """square_root.py's own test: exactly zero sub-columns in every update's QR (nothing reflected there)"""
    f = SquareRootKalmanFilter(dim_x=2, dim_z=2)
    f.x = np.array([[2.], [0.]])
    f.F = np.array([[1., 1.], [0., 1.]])
    f.H = np.array([[1., 0.], [0., 1.]])
    f.P = np.eye(2) * 1000.
    f.R *= 5
    f.Q *= 0.0001
    c = dict(p="t_")
    for k in range(30):
        f.update(G["t_zs"][k].reshape(2, 1))
        check_attrs(c, 2 * k, f)
        f.predict()
        check_attrs(c, 2 * k + 1, f)


def _bank(n, m, Nt, T, seed, layout):
    rs = np.random.RandomState(seed)
    A = rs.randn(n, n)
    b = SquareRootKalmanFilterBank(n, m, Nt, layout=layout)
    b.F, b.H = np.eye(n) + 0.1 * rs.randn(n, n) / np.sqrt(n), rs.randn(m, n)
    b.Q, b.R = 0.01 * (A @ A.T + np.eye(n)), np.eye(m) * 0.8
    b.x = rs.randn(Nt, n)
    b.P = np.eye(n)[None] * (1.0 + rs.rand(Nt, 1, 1))
    return b, rs.randn(T, Nt, m)


@pytest.mark.parametrize("layout", ["soa", "aos"])
@pytest.mark.parametrize("dims", [(4, 2), (6, 3)])
def test_large_bank_vs_port(layout, dims):
    n, m = dims
    Nt, T = 70001, 16
    b, zs = _bank(n, m, Nt, T, 11, layout)
    mask = np.ones((T, Nt), dtype=bool)
    mask[3, 1::7] = False
    out = b.batch_filter(zs, mask=mask)
    for i in (0, 1, 63, 64, 255, 256, 35000, Nt - 2, Nt - 1):
        r = sp.batch(b.x[i], b.P1_2[i], zs[:, i], b.F, b.Q1_2, b.H, b.R1_2, mask=mask[:, i])
        for got, want in zip(out, r[:4]):
            assert rel_err(got[:, i], want) <= TOL, i
            if got.ndim == 4:
                assert np.array_equal(np.sign(np.diagonal(got[:, i], axis1=1, axis2=2)),
                                      np.sign(np.diagonal(want, axis1=1, axis2=2))), i


CHILD = r'''
import sys, numpy as np
sys.path.insert(0, %r); sys.path.insert(0, %r)
from test_gpu_srkf import _bank
out = {}
for n, m in ((1, 1), (2, 1), (3, 3), (4, 2), (4, 4), (5, 3), (6, 3)):
    for layout in ("soa", "aos"):
        b, zs = _bank(n, m, 1000, 12, n * 10 + m, layout)
        for uf in (False, True):
            r = b.batch_filter(zs, update_first=uf)
            for j, a in enumerate(r):
                out["%%d_%%d_%%s_%%d_%%d" %% (n, m, layout, uf, j)] = a
np.savez(sys.argv[1], **out)
'''


def test_fast_and_general_kernels_agree(tmp_path):
    outs = {}
    for forced in ("0", "1"):
        env = dict(os.environ, FK_SRKF_GENERAL=forced)
        path = str(tmp_path / ("o%s.npz" % forced))
        r = subprocess.run([sys.executable, "-c", CHILD % (ROOT, os.path.join(ROOT, "tests")), path], env=env,
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        outs[forced] = np.load(path)
    for k in outs["0"].files:
        assert rel_err(outs["0"][k], outs["1"][k]) <= 1e-12, k


@pytest.mark.parametrize("layout", ["soa", "aos"])
@pytest.mark.parametrize("dims", [(4, 2), (9, 3)])
def test_chained_calls_bit_identical(layout, dims):
    n, m = dims
    b, zs = _bank(n, m, 777, 20, 5, layout)
    x0, L0 = b.x.copy(), b.P1_2.copy()
    one = b.batch_filter(zs)
    first = b.batch_filter(zs[:9])
    b.x, b.P1_2 = first[0][-1], first[1][-1]
    second = b.batch_filter(zs[9:])
    for a, p, q in zip(one, first, second):
        assert np.array_equal(a, np.concatenate([p, q]))
    b.x, b.P1_2 = x0, L0
    for t in range(3):                                      # predict / update steps: the same kernels, one phase each
        b.predict()
        b.update(zs[t])
    assert rel_err(b.x, one[0][2]) <= 1e-13 and rel_err(b.P1_2, one[1][2]) <= 1e-13


@pytest.mark.parametrize("dims", [(4, 2), (6, 3), (9, 3)])
def test_bank_agrees_with_kalman_filter_bank(dims):
    n, m = dims
    Nt, T = 2000, 30
    b, zs = _bank(n, m, Nt, T, 21, "soa")
    kf = KalmanFilterBank(n, m, Nt)
    kf.F, kf.H, kf.Q, kf.R, kf.x, kf.P = b.F, b.H, b.Q, b.R, b.x.copy(), b.P.copy()
    mu, cov, mu_p, cov_p = kf.batch_filter(zs)[:4]
    smu, scov, smu_p, scov_p = b.batch_filter(zs)
    assert rel_err(smu, mu) <= 1e-9 and rel_err(smu_p, mu_p) <= 1e-9
    assert rel_err(scov @ np.swapaxes(scov, -1, -2), cov) <= 1e-9
    assert rel_err(scov_p @ np.swapaxes(scov_p, -1, -2), cov_p) <= 1e-9


def test_singular_S_raises_and_control_input():
    b = SquareRootKalmanFilterBank(3, 2, 10, layout="aos")
    b.H = np.array([[1., 0, 0], [1., 0, 0]])
    with pytest.raises(np.linalg.LinAlgError):
        b.update(np.ones((10, 2)), R2=0.0)
    rs = np.random.RandomState(2)
    b = SquareRootKalmanFilterBank(4, 2, 50)
    b.H, b.B = rs.randn(2, 4), rs.randn(4, 3)
    us, zs = rs.randn(8, 50, 3), rs.randn(8, 50, 2)
    out = b.batch_filter(zs, us=us)
    for i in (0, 49):
        r = sp.batch(b.x[i], b.P1_2[i], zs[:, i], b.F, b.Q1_2, b.H, b.R1_2, B=b.B, us=us[:, i])
        for got, want in zip(out, r[:4]):
            assert rel_err(got[:, i], want) <= TOL
