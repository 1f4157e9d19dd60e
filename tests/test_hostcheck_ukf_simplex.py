"""The step functions of the fused simplex UKF kernels (filterpy_amd/csrc/fk_ukf_simplex.hpp: ukf_simplex_step,
ukf_simplex_rts_gain -- the very text ukf_simplex.hip instantiates) compiled for the host and held against the live-reference
goldens without a GPU.  The harness (tests/hostcheck/hostcheck_simplex.cpp) is built here, into pytest's temporary directory,
with the flags tests/conftest.py uses for libhostcheck.so.  Bar: the project's 1e-10 (max |d| / max |ref| per array)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import simplex_port as sp

HERE = os.path.dirname(os.path.abspath(__file__))
TOL = 1e-10
ST_NOT_PD = 1


@pytest.fixture(scope="module")
def hc(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("hostcheck_simplex") / "libhostcheck_simplex.so")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=on", "-w", "-o", so,
                           os.path.join(HERE, "hostcheck", "hostcheck_simplex.cpp")])
    return ctypes.CDLL(so)


@pytest.fixture(scope="module")
def gold():
    return sp.Golden()


def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def _c(a, dtype=np.float64):
    return np.ascontiguousarray(a, dtype=dtype)


def run_fwd(hc, F, H, Q, R, Wm, Wc, x0, P0, zl, cls=(0, 0)):
    """-> status, means, covs, x, P (the state the call leaves in place)"""
    n, m, T = F.shape[0], H.shape[0], len(zl)
    zs = _c([np.zeros(m) if z is None else np.reshape(z, m) for z in zl])
    mask = _c([z is not None for z in zl], np.uint8)
    x, P, mu, cov = _c(x0).copy(), _c(P0).copy(), np.zeros((T, n)), np.zeros((T, n, n))
    st = hc.hc_ukf_simplex(n, m, cls[0], cls[1], ctypes.c_long(T), _p(_c(F)), _p(_c(H)), _p(_c(Q)), _p(_c(R)), _p(_c(Wm)), _p(_c(Wc)),
                           _p(zs), _p(mask) if not mask.all() else None, _p(x), _p(P), _p(mu), _p(cov))
    return st, mu, cov, x, P


def run_rts(hc, F, Q, Wm, Wc, Xs, Ps, cls=0):
    T, n = Xs.shape
    xs, ps, Ks = np.zeros((T, n)), np.zeros((T, n, n)), np.full((T, n, n), np.nan)
    st = hc.hc_ukf_simplex_rts(n, cls, ctypes.c_long(T), _p(_c(F)), _p(_c(Q)), _p(_c(Wm)), _p(_c(Wc)), _p(_c(Xs)), _p(_c(Ps)),
                               _p(xs), _p(ps), _p(Ks))
    return st, xs, ps, Ks


def close(a, b, what):
    err = sp.rel(a, b)
    assert err < TOL, (what, err)


def test_table_is_the_point_matrix(hc, gold):
    """the dispatcher's (a_r, b_r): row r of the golden's I holds a_r in the columns 0..r and b_r in column r + 1 -- bit for bit"""
    for n in range(1, 10):
        ab = np.zeros(18)
        hc.hc_simplex_table(n, _p(ab))
        I = gold.I(n)
        for r in range(n):
            assert np.all(I[r, :r + 1] == ab[r]) and I[r, r + 1] == ab[9 + r] and not I[r, r + 2:].any(), (n, r)
        assert not ab[n:9].any() and not ab[9 + n:].any()
    ab = np.ones(18)
    hc.hc_simplex_table(10, _p(ab))
    assert not ab.any()


@pytest.mark.parametrize("n,m", sp.FUSED)
def test_step_functions_against_golden(hc, gold, n, m):
    """forward and smoother in the class the dispatcher picks -- (1,1), (2,1), (3,1), (5,3), (7,4) run padded --; (4,2) has the
    missing measurement"""
    c = gold.case(n, m)
    W = c["Wm"]
    st, mu, cov, x, P = run_fwd(hc, c["F"], c["H"], c["Q"], c["R"], W, W, c["x0"], c["P0"], c["zl"])
    assert st == 0
    close(mu, c["mu"], "mu"), close(cov, c["cov"], "cov")
    assert np.array_equal(x, mu[-1]) and np.array_equal(P, cov[-1])
    assert np.array_equal(cov, np.swapaxes(cov, 1, 2))
    st, xs, ps, Ks = run_rts(hc, c["F"], c["Q"], W, W, c["mu"], c["cov"])
    assert st == 0
    close(xs, c["rts_x"], "rts_x"), close(ps, c["rts_P"], "rts_P"), close(Ks, c["rts_K"], "rts_K")
    assert np.array_equal(xs[-1], c["mu"][-1]) and np.array_equal(ps[-1], c["cov"][-1]) and not Ks[-1].any()
    if (n, m) == (4, 2):
        t = gold.missing[1]
        assert c["zl"][t] is None and not np.array_equal(mu[t], mu[t - 1])


@pytest.mark.parametrize("n,m,cls", [(3, 1, (4, 2)), (3, 1, (6, 3)), (5, 2, (6, 3)), (7, 4, (8, 4)), (7, 3, (9, 3)), (2, 2, (9, 4)),
                                     (1, 1, (2, 2)), (8, 4, (9, 4))])
def test_padded_classes(hc, gold, n, m, cls):
    """a dim_x below its class: a_r = b_r = 0 from row n on, weight 0 behind point n, the padded block of P the identity"""
    if (n, m) in gold.cases:
        c = gold.case(n, m)
        F, H, Q, R, x0, P0, zl = c["F"], c["H"], c["Q"], c["R"], c["x0"], c["P0"], c["zl"]
    else:
        rs = np.random.RandomState(40 + 10 * n + m)
        A, B = rs.randn(n, n), rs.randn(m, m)
        F, H = np.eye(n) + 0.05 * rs.randn(n, n), rs.randn(m, n)
        Q, R, P0, x0 = 0.01 * (A @ A.T / n + np.eye(n)), B @ B.T / m + np.eye(m), 3.0 * (A.T @ A / n + np.eye(n)), rs.randn(n)
        zl = [None if t == 4 else rs.randn(m) for t in range(12)]
    W = sp.weights(n)
    want_mu, want_cov = sp.batch_filter(x0, P0, zl, F, H, Q, R)
    st, mu, cov, _, _ = run_fwd(hc, F, H, Q, R, W, W, x0, P0, zl, cls)
    assert st == 0
    close(mu, want_mu, "mu"), close(cov, want_cov, "cov")
    st, xs, ps, Ks = run_rts(hc, F, Q, W, W, want_mu, want_cov, cls[0])
    assert st == 0
    for got, want, key in zip((xs, ps, Ks), sp.rts_smoother(want_mu, want_cov, F, Q), "xPK"):
        close(got, want, "rts " + key)
    assert hc.hc_ukf_simplex(cls[0] + 1, m, cls[0], cls[1], ctypes.c_long(1), *[None] * 12) == -1      # not this class's


def test_a_track_that_is_not_positive_definite(hc, gold):
    """its status carries FK_STATUS_NOT_PD; the tracks run before and after it are exact (no state is shared)"""
    c = gold.case(6, 3)
    W = c["Wm"]
    bad = c["P0"].copy()
    bad[2, 2] = -1.0
    res = [run_fwd(hc, c["F"], c["H"], c["Q"], c["R"], W, W, c["x0"], P0, c["zl"]) for P0 in (c["P0"], bad, c["P0"])]
    assert res[1][0] & ST_NOT_PD
    for k in (0, 2):
        assert res[k][0] == 0 and np.isfinite(res[k][1]).all() and np.isfinite(res[k][2]).all()
        close(res[k][1], c["mu"], "mu"), close(res[k][2], c["cov"], "cov")
    Ps = c["cov"].copy()
    Ps[3] = bad
    assert run_rts(hc, c["F"], c["Q"], W, W, c["mu"], Ps)[0] & ST_NOT_PD
    st, xs, _, _ = run_rts(hc, c["F"], c["Q"], W, W, c["mu"], c["cov"])
    assert st == 0 and np.isfinite(xs).all()


@pytest.mark.parametrize("n,m", [(2, 2), (4, 2), (6, 3), (8, 4), (9, 3), (5, 3)])
def test_unequal_weights_are_used_as_given(hc, gold, n, m):
    """Wm != Wc, neither constant, Wm not summing to 1: point by point, against the port"""
    c = gold.case(n, m)
    rs = np.random.RandomState(70 + n)
    Wm = rs.uniform(0.5, 1.5, n + 1)
    Wm *= 1.02 / Wm.sum()
    # (no Wc above 1 / (n + 1): then sum_j Wc_j d_j d_j' <= P for the regenerated points, and P - K S K' stays positive definite)
    Wc = rs.uniform(0.7, 1.0, n + 1) / (n + 1)
    want_mu, want_cov = sp.batch_filter(c["x0"], c["P0"], c["zl"], c["F"], c["H"], c["Q"], c["R"], Wm, Wc)
    assert sp.rel(want_mu, c["mu"]) > 1e-3                                   # the weights matter
    st, mu, cov, _, _ = run_fwd(hc, c["F"], c["H"], c["Q"], c["R"], Wm, Wc, c["x0"], c["P0"], c["zl"])
    assert st == 0
    close(mu, want_mu, "mu"), close(cov, want_cov, "cov")
    st, xs, ps, Ks = run_rts(hc, c["F"], c["Q"], Wm, Wc, want_mu, want_cov)
    assert st == 0
    for got, want, key in zip((xs, ps, Ks), sp.rts_smoother(want_mu, want_cov, c["F"], c["Q"], Wm, Wc), "xPK"):
        close(got, want, "rts " + key)
