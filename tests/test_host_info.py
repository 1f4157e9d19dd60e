"""The information filter on the CPU: tests/info_port.py against the goldens frozen from the live reference (and against the
live reference where the checkout exists), tests/info_hp.py, the per-track step of filterpy_amd/csrc/fk_info.hpp compiled for
the host against the goldens and the port (its singularity flag and the factor of the precision bar included), the drop-in
layer (InformationFilter / InformationFilterBank) on a stand-in engine, and the ISA of the fast kernels."""
import ctypes
import glob
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, golden, rel_err
import info_models
import info_port as ip
from filterpy_amd.kalman import InformationFilter, InformationFilterBank

REF = os.environ.get("FILTERPY_REFERENCE", "/root/reference")
G = golden("info")
NC = int(G["n_cases"])
TOL = 1e-12


# ---- the port -------------------------------------------------------------------------------------------------------------
def check_case_against_golden(make, ci, tol):
    c = ip.case(G, ci)
    f = make(c)
    for k, op in enumerate(c["ops"]):
        ip.run_op(f, c, k, op)
        for a, mine in (("x", f.x), ("P_inv", f.Pi)):
            assert rel_err(np.ravel(mine), np.ravel(ip.attr(G, c["p"], k, a))) <= tol, (ci, k, a)
        if f.K is not None:
            for a, mine in (("K", f.K), ("y", f.y), ("S", f.Pi if op >= ip.UPDATE and op != ip.UPDATE_NONE else None)):
                if mine is not None:
                    assert rel_err(np.ravel(mine), np.ravel(ip.attr(G, c["p"], k, a))) <= tol, (ci, k, a)


@pytest.mark.parametrize("ci", range(NC))
def test_port_matches_golden(ci):
    check_case_against_golden(lambda c: ip.Port(c["n"], c["m"]).set(c), ci, 1e-13)


def test_goldens_cover_what_they_should():
    assert [tuple(d) for d in G["dims"]] == [(1, 1), (2, 1), (2, 2), (3, 2), (4, 2), (5, 3), (6, 3), (8, 4), (9, 3), (12, 4), (16, 8)]
    seen = set()
    for ci in range(NC):
        c = ip.case(G, ci)
        seen |= {("op", o) for o in c["ops"]} | {("order", c["order"]), ("nd", c["nd"]), ("ctrl", c["ctrl"])}
    assert seen >= {("op", o) for o in range(6)} | {("order", 0), ("order", 1), ("nd", 1), ("nd", 2), ("ctrl", 1), ("ctrl", 2)}
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "info.npz")) <= os.path.getsize(
        os.path.join(ROOT, "tests", "golden", "srkf.npz"))


def test_port_matches_golden_reference_test_model():
    """the model of the reference's test_1d / test_against_kf: update then predict, scalar measurements"""
    x, Pi = np.array([2., 0.]), np.eye(2)
    F, H, Q, Ri = np.array([[1., 1.], [0., 1.]]), np.array([[1., 0.]]), np.eye(2) * 0.0001, np.eye(1) / 5
    for k in range(30):
        x, Pi, y, K = ip.update(x, Pi, G["t_zs"][k:k + 1], H, Ri)
        assert rel_err(Pi, ip.attr(G, "t_", 2 * k, "P_inv")) <= 1e-13 and rel_err(K, ip.attr(G, "t_", 2 * k, "K")) <= 1e-13
        assert rel_err(x, np.ravel(ip.attr(G, "t_", 2 * k, "x"))) <= 1e-13
        x, Pi = ip.predict(x, Pi, F, Q)
        assert rel_err(x, np.ravel(ip.attr(G, "t_", 2 * k + 1, "x"))) <= 1e-13
        assert rel_err(Pi, ip.attr(G, "t_", 2 * k + 1, "P_inv")) <= 1e-13


def _model(n, m, rs):
    A = rs.randn(n, n)
    return dict(F=np.eye(n) + 0.1 * rs.randn(n, n) / np.sqrt(n), H=rs.randn(m, n), Q=0.01 * (A @ A.T + np.eye(n)),
                Rinv=np.eye(m) * 1.25)


def test_port_matches_live_reference_on_random_cases():
    if not os.path.isdir(os.path.join(REF, "filterpy")):
        pytest.skip("no reference checkout here")
    sys.path.insert(0, REF)
    try:
        from filterpy.kalman import InformationFilter as RefIF
    finally:
        sys.path.remove(REF)
    rs = np.random.RandomState(9)
    for n, m in ((4, 2), (6, 3), (9, 3), (3, 3), (16, 8)):
        d = _model(n, m, rs)
        f = RefIF(n, m, compute_log_likelihood=False)
        f.F, f.H, f.Q, f.R_inv, f.P_inv = d["F"], d["H"], d["Q"], d["Rinv"], np.eye(n) / 3
        f.x = rs.randn(n)
        x, Pi = f.x.copy(), f.P_inv.copy()
        for _ in range(20):
            z = rs.randn(m)
            f.predict()
            f.update(z)
            x, Pi = ip.predict(x, Pi, d["F"], d["Q"])
            x, Pi, y, K = ip.update(x, Pi, z, d["H"], d["Rinv"])
            assert rel_err(x, f.x) <= 1e-13 and rel_err(Pi, f.P_inv) <= 1e-13 and rel_err(K, f.K) <= 1e-13


def test_port_vectorised_over_tracks_matches_one_track():
    rs = np.random.RandomState(12)
    n, m, N, T = 4, 2, 5, 7
    d = _model(n, m, rs)
    x0, Pi0, zs = rs.randn(N, n), np.eye(n)[None] * (0.5 + rs.rand(N, 1, 1)), rs.randn(T, N, m)
    B, us = rs.randn(n, 2), rs.randn(T, N, 2)
    mask = rs.rand(T, N) > 0.3
    for uf in (False, True):
        out = ip.batch_tracks(x0, Pi0, zs, d["F"], d["Q"], d["H"], d["Rinv"], B, us, mask, uf)
        for i in range(N):
            r = ip.batch(x0[i], Pi0[i], zs[:, i], d["F"], d["Q"], d["H"], d["Rinv"], B, us[:, i], mask[:, i], uf)
            for a, b in zip(out, r[:4]):
                assert rel_err(a[:, i], b) <= 1e-13


# ---- tests/info_hp.py, the extended-precision truth of tests/test_gpu_info_precision.py --------------------------------------
def test_hp_is_extended_precision_and_agrees_with_the_port():
    import info_hp
    assert np.finfo(info_hp.LD).eps < 1e-18
    A = np.random.RandomState(1).randn(7, 7) + 3 * np.eye(7)
    AI = info_hp.inv(A)
    assert AI.dtype == info_hp.LD
    assert float(np.max(np.abs(AI @ info_hp.ld(A) - np.eye(7)))) <= 1e-17
    assert np.max(np.abs(AI.astype(float) - np.linalg.inv(A))) <= 1e-14
    assert float(np.max(np.abs(info_hp.inv(np.array([[0., 1.], [1., 0.]])) - np.array([[0., 1.], [1., 0.]])))) == 0   # it pivots
    n, m, T = 4, 2, 12
    rs = np.random.RandomState(4)
    d = _model(n, m, rs)
    zs, x0, Pi0 = rs.randn(T, m), rs.randn(n), np.eye(n) * 0.5
    hp = info_hp.batch(x0, Pi0, zs, d["F"], d["Q"], d["H"], d["Rinv"])
    port = ip.batch(x0, Pi0, zs, d["F"], d["Q"], d["H"], d["Rinv"])
    for a, b in zip(hp, port[:4]):
        assert rel_err(a.astype(float), b) <= 1e-13
        assert a.dtype == info_hp.LD


# ---- fk_info.hpp compiled for the host --------------------------------------------------------------------------------------
HC_SRC = r'''
#include "fk_info.hpp"
using namespace fk;
#ifndef HC_NX
#define HC_NX 16
#define HC_NZ 8
#endif
constexpr int NX = HC_NX, NZ = HC_NZ;
// the model padded as the general kernel pads it (identity in F, zeros in Q, H, G and HtRi); G and HtRi as the kernel computes them
static void model(InfoRegModel<NX, NZ> &M, int n, int m, const double *F, const double *Q, const double *H, const double *Ri)
{
    const bool meas = H && Ri;
    for (int i = 0; i < NX; ++i) for (int j = 0; j < NX; ++j) {
        M.F[i * NX + j] = (F && i < n && j < n) ? F[i * n + j] : (i == j);
        M.Q[i * NX + j] = (Q && i < n && j < n) ? Q[i * n + j] : 0.0;
    }
    for (int i = 0; i < NZ; ++i)
        for (int j = 0; j < NX; ++j) M.H[i * NX + j] = (H && i < m && j < n) ? H[i * n + j] : 0.0;
    for (int i = 0; i < NX; ++i)
        for (int c = 0; c < NZ; ++c) M.HtRi[i * NZ + c] = (meas && i < n && c < m) ? info_htri_entry(H, Ri, n, m, i, c) : 0.0;
    for (int i = 0; i < NX; ++i) for (int j = 0; j < NX; ++j) {
        const int hi = i > j ? i : j, lo = i > j ? j : i;
        M.G[i * NX + j] = (meas && hi < n) ? info_g_entry(M.HtRi + hi * NZ, H, n, m, lo) : 0.0;
    }
}
static void load(int n, const double *x0, const double *P0, double (&x)[NX], double (&Pi)[NX * NX])
{
    for (int i = 0; i < NX; ++i) x[i] = i < n ? x0[i] : 0.0;
    for (int i = 0; i < NX; ++i) for (int j = 0; j < NX; ++j) {
        const int hi = i > j ? i : j, lo = i > j ? j : i;
        Pi[i * NX + j] = (hi < n) ? P0[hi * n + lo] : (i == j);
    }
}
static void save(int n, const double (&x)[NX], const double (&Pi)[NX * NX], double *x0, double *P0)
{
    for (int i = 0; i < n; ++i) x0[i] = x[i];
    for (int i = 0; i < n; ++i) for (int j = 0; j < n; ++j) P0[i * n + j] = Pi[i * NX + j];
}
extern "C" int hc_predict(int n, const double *F, const double *Q, int nu, const double *B, const double *u, double *x0, double *P0)
{
    if (n > NX) return -1;
    InfoRegModel<NX, NZ> M;
    model(M, n, 1, F, Q, nullptr, nullptr);
    double x[NX], Pi[NX * NX], P[NX * NX] = {}, bu[NX] = {};
    load(n, x0, P0, x, Pi);
    for (int i = 0; i < n; ++i) for (int j = 0; j < nu; ++j) bu[i] = j == 0 ? B[i * nu] * u[0] : fma(B[i * nu + j], u[j], bu[i]);
    const int st = info_predict<NX>(x, Pi, P, false, M, bu, nu > 0, n);
    save(n, x, Pi, x0, P0);
    return st;
}
extern "C" int hc_update(int n, int m, const double *H, const double *Ri, const double *z0, double *x0, double *P0,
                         double *y0, double *K0)
{
    if (n > NX || m > NZ) return -1;
    InfoRegModel<NX, NZ> M;
    model(M, n, m, nullptr, nullptr, H, Ri);
    double x[NX], Pi[NX * NX], P[NX * NX] = {}, z[NZ] = {}, y[NZ], K[NX * NZ];
    load(n, x0, P0, x, Pi);
    for (int i = 0; i < m; ++i) z[i] = z0[i];
    const int st = info_update<NX, NZ>(x, Pi, P, z, M, n, y, K, true);
    save(n, x, Pi, x0, P0);
    for (int i = 0; i < m; ++i) y0[i] = y[i];
    for (int i = 0; i < n; ++i) for (int j = 0; j < m; ++j) K0[i * m + j] = K[i * NZ + j];
    return st;
}
// T steps, predict first, as the kernel's time loop runs them (the update's inverse reused by the next predict); the four
// histories out.  mask: 0 = no measurement at that step, or NULL.
extern "C" int hc_batch(int n, int m, int T, const double *F, const double *Q, const double *H, const double *Ri,
                        const double *zs, const unsigned char *mask, double *x0, double *P0, double *mu, double *cov,
                        double *mu_p, double *cov_p)
{
    if (n > NX || m > NZ) return -1;
    InfoRegModel<NX, NZ> M;
    model(M, n, m, F, Q, H, Ri);
    double x[NX], Pi[NX * NX], P[NX * NX] = {}, bu[NX] = {};
    load(n, x0, P0, x, Pi);
    int st = 0;
    bool have_P = false;
    for (int t = 0; t < T; ++t) {
        st |= info_predict<NX>(x, Pi, P, have_P, M, bu, false, n);
        have_P = false;
        save(n, x, Pi, mu_p + t * n, cov_p + t * n * n);
        if (!mask || mask[t]) {
            double z[NZ] = {}, y[NZ], K[NX * NZ];
            for (int i = 0; i < m; ++i) z[i] = zs[t * m + i];
            st |= info_update<NX, NZ>(x, Pi, P, z, M, n, y, K, false);
            have_P = true;
        }
        save(n, x, Pi, mu + t * n, cov + t * n * n);
    }
    save(n, x, Pi, x0, P0);
    return st;
}
'''
EXACT = [(2, 1), (4, 2), (6, 3)]


def _hc_cmd(src, so, dims=None):
    d = [] if dims is None else ["-DHC_NX=%d" % dims[0], "-DHC_NZ=%d" % dims[1]]
    return ["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=on", "-w", *d,
            "-I", os.path.join(ROOT, "filterpy_amd", "csrc"), str(src), "-o", str(so)]


@pytest.fixture(scope="module")
def hc(tmp_path_factory):
    """the padded (16, 8) build (what the general kernel runs) and exact builds of a few fast shapes"""
    d = tmp_path_factory.mktemp("hc_info")
    src = d / "hc_info.cpp"
    src.write_text(HC_SRC)
    libs = {}
    for dims in [None] + EXACT:
        so = d / ("libhc_info%s.so" % ("" if dims is None else "_%d_%d" % dims))
        subprocess.check_call(_hc_cmd(src, so, dims))
        libs[dims] = ctypes.CDLL(str(so))
    return libs


def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def _cc(a):
    return np.ascontiguousarray(a, dtype=float)


class HostFilter(ip.Port):
    """the port's interface, computed by one hc_info build"""

    def __init__(self, lib, n, m):
        super().__init__(n, m)
        self.lib = lib
        self.st = 0

    def predict(self, u=None):
        B = uu = None
        nu = 0
        if u is not None:
            uu = _cc(np.ravel(u))
            B = _cc(self.B if np.ndim(self.B) else np.eye(self.n) * self.B)
            nu = B.shape[1]
        x, Pi = _cc(self.x).copy(), _cc(self.Pi).copy()
        self.st = self.lib.hc_predict(self.n, _p(_cc(self.F)), _p(_cc(self.Q)), nu, _p(B), _p(uu), _p(x), _p(Pi))
        self.x, self.Pi = x, Pi

    def update(self, z, R_inv=None):
        if z is None:
            return
        n, m = self.n, self.m
        Ri = self.Rinv if R_inv is None else (np.eye(m) * R_inv if np.isscalar(R_inv) else R_inv)
        x, Pi = _cc(self.x).copy(), _cc(self.Pi).copy()
        y, K = np.zeros(m), np.zeros((n, m))
        self.st = self.lib.hc_update(n, m, _p(_cc(self.H)), _p(_cc(Ri)), _p(_cc(np.ravel(z))), _p(x), _p(Pi), _p(y), _p(K))
        self.x, self.Pi, self.y, self.K = x, Pi, y, K


def host_batch(lib, n, m, x0, Pi0, zs, F, Q, H, Ri, mask=None):
    T = len(zs)
    out = [np.zeros((T, n)), np.zeros((T, n, n)), np.zeros((T, n)), np.zeros((T, n, n))]
    x, Pi = _cc(x0).copy(), _cc(Pi0).copy()
    mk = None if mask is None else np.ascontiguousarray(mask, dtype=np.uint8)
    st = lib.hc_batch(n, m, T, _p(_cc(F)), _p(_cc(Q)), _p(_cc(H)), _p(_cc(Ri)), _p(_cc(zs)), _p(mk), _p(x), _p(Pi),
                      *(_p(o) for o in out))
    return out, st, x, Pi


@pytest.mark.parametrize("ci", range(NC))
def test_host_step_matches_golden(hc, ci):
    c = ip.case(G, ci)
    check_case_against_golden(lambda c: HostFilter(hc[None], c["n"], c["m"]).set(c), ci, TOL)
    if (c["n"], c["m"]) in EXACT:
        check_case_against_golden(lambda c: HostFilter(hc[(c["n"], c["m"])], c["n"], c["m"]).set(c), ci, TOL)


@pytest.mark.parametrize("dims", EXACT + [(3, 2), (7, 3), (9, 3)])
def test_host_batch_matches_port_and_padding_is_exact(hc, dims):
    n, m = dims
    rs = np.random.RandomState(n * 10 + m)
    d = _model(n, m, rs)
    T = 9
    zs, x0, Pi0 = rs.randn(T, m), rs.randn(n), np.eye(n) * 0.5 + 0.1 * np.ones((n, n))
    mask = np.ones(T, dtype=bool)
    mask[4] = False
    want = ip.batch(x0, Pi0, zs, d["F"], d["Q"], d["H"], d["Rinv"], mask=mask)
    got, st, x, Pi = host_batch(hc[None], n, m, x0, Pi0, zs, d["F"], d["Q"], d["H"], d["Rinv"], mask)
    assert st == 0
    for a, b in zip(got, want[:4]):
        assert rel_err(a, b) <= TOL
    assert np.array_equal(x, got[0][-1]) and np.array_equal(Pi, got[1][-1])
    assert np.array_equal(got[1], np.swapaxes(got[1], -1, -2))                 # P_inv leaves exactly symmetric
    if dims in EXACT:
        exact = host_batch(hc[dims], n, m, x0, Pi0, zs, d["F"], d["Q"], d["H"], d["Rinv"], mask)[0]
        for a, b in zip(got, exact):
            assert np.array_equal(a, b)                                         # the padded block adds exact zeros only
    # chained calls reproduce one call bit for bit, with the missing measurement right before the split
    first, _, x1, P1 = host_batch(hc[None], n, m, x0, Pi0, zs[:5], d["F"], d["Q"], d["H"], d["Rinv"], mask[:5])
    second = host_batch(hc[None], n, m, x1, P1, zs[5:], d["F"], d["Q"], d["H"], d["Rinv"], mask[5:])[0]
    for a, p, q in zip(got, first, second):
        assert np.array_equal(a, np.concatenate([p, q]))
    first, _, x1, P1 = host_batch(hc[None], n, m, x0, Pi0, zs[:3], d["F"], d["Q"], d["H"], d["Rinv"], mask[:3])
    second = host_batch(hc[None], n, m, x1, P1, zs[3:], d["F"], d["Q"], d["H"], d["Rinv"], mask[3:])[0]
    for a, p, q in zip(got, first, second):
        assert np.array_equal(a, np.concatenate([p, q]))                        # ... and right after an update


@pytest.mark.parametrize("dims", [None, (4, 2)])
def test_host_step_flags_singular_information(hc, dims):
    n, m = 4, 2
    rs = np.random.RandomState(3)
    d = _model(n, m, rs)
    h = HostFilter(hc[dims], n, m)
    h.F, h.H, h.Q, h.Rinv, h.x = d["F"], d["H"], d["Q"], d["Rinv"], np.ones(n)
    h.Pi = np.zeros((n, n))
    with np.errstate(all="ignore"):
        h.predict()
    assert h.st & 1                                         # P_inv = 0: no information
    A = rs.randn(n, n)
    Pi = A @ A.T + np.eye(n)
    Pi[2, :] = 0.0
    Pi[:, 2] = 0.0                                          # rank n - 1, an exactly zero row and column
    h.Pi, h.x = Pi, np.ones(n)
    with np.errstate(all="ignore"):
        h.predict()
    assert h.st & 1
    h.Pi, h.x = A @ A.T + np.eye(n), np.ones(n)
    h.predict()
    assert h.st == 0
    g = HostFilter(hc[dims], n, m)
    g.F, g.H, g.Q, g.Rinv, g.x = d["F"], np.zeros((m, n)), d["Q"], d["Rinv"], np.ones(n)
    g.Pi = np.zeros((n, n))
    with np.errstate(all="ignore"):
        g.update(np.ones(m))
    assert g.st & 1                                         # the update's own factorisation is tested too


def test_host_step_precision_ratio_fixes_the_bar(hc):
    """the factor of tests/test_gpu_info_precision.py's bar: the host-compiled step against the port on exactly its models,
    worst per-output ratio of the worst-track errors and of the medians; K_BAR is twice that, rounded up to a power of two"""
    worst = 0.0
    for dims in info_models.DIMS:
        n, m = dims
        d = info_models.model(dims)
        lib = hc[dims] if dims in hc else hc[None]
        out = [np.zeros((info_models.T, info_models.NT) + s) for s in ((n,), (n, n), (n,), (n, n))]
        for i in range(info_models.NT):
            r, st, _, _ = host_batch(lib, n, m, d["x0"][i], d["Pinv0"][i], d["zs"][:, i], d["F"], d["Q"], d["H"], d["Rinv"])
            assert st == 0
            for j in range(4):
                out[j][:, i] = r[j]
        eg, ep = info_models.errors(out, dims), info_models.truth(dims)[1]
        for j, name in enumerate(info_models.OUTPUTS):
            r_max, r_med = eg[j].max() / max(ep[j].max(), 1e-12), np.median(eg[j]) / max(np.median(ep[j]), 1e-12)
            print(dims, name, "host/port worst %.2f medians %.2f; port worst %.1e" % (r_max, r_med, ep[j].max()))
            worst = max(worst, r_max, r_med)
    print("worst ratio %.2f" % worst)
    assert 2 * worst <= info_models.K_BAR               # (measured: 3.75, the P_inv outputs of (12, 4); hence K_BAR = 8)
    assert info_models.K_BAR <= 32                          # a host build that needs more has worse arithmetic, not another order


# ---- the drop-in layer on a stand-in engine -----------------------------------------------------------------------------
@pytest.fixture
def fake(monkeypatch):
    import fake_info_engine
    return fake_info_engine.install(monkeypatch)


def check_dropin_attrs(f, p, k, n, m, tol=1e-10):
    for a in ip.ATTRS:
        if a in ("log_likelihood", "likelihood") and not ip.has_likelihood(n, m):
            continue
        ref, mine = ip.attr(G, p, k, a), np.asarray(getattr(f, a), dtype=float)
        assert mine.shape == ref.shape, (k, a, mine.shape, ref.shape)
        assert rel_err(mine, ref) <= tol, (k, a)
    assert rel_err(f.P, np.linalg.inv(ip.attr(G, p, k, "P_inv"))) <= 1e-9


@pytest.mark.parametrize("ci", range(NC))
def test_dropin_sequences_attributes(fake, ci):
    c = ip.case(G, ci)
    n, m = c["n"], c["m"]
    f = ip.setup(InformationFilter(n, m, compute_log_likelihood=ip.has_likelihood(n, m)), c)
    for k, op in enumerate(c["ops"]):
        ip.run_op(f, c, k, op)
        check_dropin_attrs(f, c["p"], k, n, m)
        if op == ip.UPDATE_NONE:
            assert f.z is None
        elif op >= ip.UPDATE:
            assert np.array_equal(np.ravel(f.z), c["zs"][k]) and np.array_equal(f.S, f.P_inv)
    assert len(fake) == sum(op != ip.UPDATE_NONE for op in c["ops"])     # one launch per call, none for update(None)


def test_dropin_reference_test_model(fake):
    f = InformationFilter(dim_x=2, dim_z=1)
    str(f)                                                   # before F is set, as the reference's test does
    f.x = np.array([[2.], [0.]])
    f.F = np.array([[1., 1.], [0., 1.]])
    f.H = np.array([[1., 0.]])
    f.R_inv *= 1. / 5
    f.Q *= 0.0001
    for k in range(30):
        f.update(float(G["t_zs"][k]))
        check_dropin_attrs(f, "t_", 2 * k, 2, 1)
        f.predict()
        check_dropin_attrs(f, "t_", 2 * k + 1, 2, 1)
    assert "InformationFilter object" in repr(f) and "_F_inv" in repr(f)


def test_dropin_defaults_and_quirks(fake):
    f = InformationFilter(3, 2)
    assert f.x.shape == (3, 1) and np.array_equal(f.P_inv, np.eye(3)) and np.array_equal(f.Q, np.eye(3))
    assert f.B == 0. and f.F == 0. and f._F_inv == 0. and f.K == 0. and f.S == 0. and f.inv is np.linalg.inv
    assert f.H.shape == (2, 3) and np.array_equal(f.R_inv, np.eye(2)) and f.y.shape == (2, 1) and f.z.shape == (2, 1)
    assert f.log_likelihood == math.log(sys.float_info.min) and f.likelihood == sys.float_info.min
    assert f._no_information is False and f.compute_log_likelihood is True
    for a in ("x_prior", "x_post", "P_inv_prior", "P_inv_post"):
        assert np.array_equal(getattr(f, a), f.x if a[0] == "x" else f.P_inv)
    F = np.array([[1., 1, 0], [0, 1, 1], [0, 0, 1]])
    f.F = F
    assert np.allclose(f._F_inv, np.linalg.inv(F)) and f.F is F
    f.H = np.array([[1., 0, 0], [0, 1, 0]])
    f.predict()
    f.update(np.ones((2, 1)))
    assert np.allclose(f.P, np.linalg.inv(f.P_inv)) and np.array_equal(f.S, f.P_inv_post)
    with pytest.raises(ValueError):
        f.log_likelihood                                    # 1 < dim_z < dim_x: the reference's logpdf(y, cov=S) cannot broadcast
    with pytest.raises(NotImplementedError):
        f.batch_filter([np.ones((2, 1))])
    g = InformationFilter(2, 1, compute_log_likelihood=False)
    g.F, g.H = np.eye(2), np.array([[1., 0.]])
    g.update(1.0)
    assert g.log_likelihood == math.log(sys.float_info.min) and g.y.shape == (1, 1)
    g.update(None)
    assert g.z is None and np.array_equal(g.x_post, g.x)


def test_dropin_errors(fake):
    with pytest.raises(ValueError):
        InformationFilter(0, 1)
    with pytest.raises(ValueError):
        InformationFilter(2, 0)
    with pytest.raises(ValueError):
        InformationFilter(2, 1, dim_u=-1)
    f = InformationFilter(3, 2)
    f.F = np.eye(3)
    with pytest.raises(ValueError):
        f.update(np.zeros(2))                             # column x, (m,) z with m > 1: y would be (m, m)
    with pytest.raises(ValueError):
        f.update(np.zeros((2, 1)), R_inv=np.ones((3, 3)))
    with pytest.raises(ValueError):
        f.predict(np.ones(3))                             # scalar B: b u in x's orientation (column)
    f.B = np.ones((3, 2))
    with pytest.raises(ValueError):
        f.predict(np.ones((3, 1)))                        # B has 2 columns
    with pytest.raises(ValueError):
        f.predict(2.0)                                    # nonzero scalar u with a matrix B
    for name in ("P_inv", "Q"):
        g = InformationFilter(3, 2)
        g.F = np.eye(3)
        setattr(g, name, 0.5)                             # the reference adds a scalar P_inv to every entry of H' R_inv H
        with pytest.raises(ValueError):
            g.predict()
    g = InformationFilter(3, 2)
    g.R_inv = 2.0
    with pytest.raises(ValueError):
        g.update(np.zeros((2, 1)))
    g = InformationFilter(3, 2)
    g.P_inv = 1e-21
    with pytest.raises(ValueError):
        g.update(np.zeros((2, 1)))
    f.x = np.zeros(3)
    with pytest.raises(ValueError):
        f.update(np.zeros((2, 1)))                        # 1-D x, column z
    f.x = np.zeros((1, 3))
    with pytest.raises(ValueError):
        f.predict()
    h = InformationFilter(2, 1)
    h.F = np.eye(2)
    h.inv = np.linalg.pinv
    with pytest.raises(NotImplementedError):
        h.predict()
    with pytest.raises(NotImplementedError):
        h.update(1.0)
    assert not fake                                       # nothing reached the engine
    g = InformationFilter(2, 1)
    g.F, g.H = np.eye(2), np.array([[1., 0.]])
    g.predict(0)                                          # u = 0 with the scalar B: no control input
    g.B = 0.5
    g.predict(2.0)                                        # scalar u, scalar B: b u on every entry, as numpy does
    assert np.allclose(g.x, 1.0)


def test_dropin_singular_information_raises(fake):
    f = InformationFilter(3, 2)
    f.F = np.eye(3)
    f.P_inv = np.zeros((3, 3))
    with pytest.raises(np.linalg.LinAlgError):
        f.predict()
    with pytest.raises(np.linalg.LinAlgError):
        f.update(np.ones((2, 1)))                         # H = 0: P_inv + H' R_inv H is still 0
    b = InformationFilterBank(3, 2, 4)
    b.P_inv = np.zeros((3, 3))
    with pytest.raises(np.linalg.LinAlgError):
        b.predict()
    with pytest.raises(np.linalg.LinAlgError):
        b.batch_filter(np.ones((2, 4, 2)))


def _bank_model(n, m, Nt, T, seed):
    rs = np.random.RandomState(seed)
    d = _model(n, m, rs)
    d.update(x0=rs.randn(Nt, n), Pinv0=np.eye(n)[None] * (0.5 + rs.rand(Nt, 1, 1)), zs=rs.randn(T, Nt, m))
    return d


@pytest.mark.parametrize("layout", ["soa", "aos"])
@pytest.mark.parametrize("update_first", [False, True])
def test_dropin_bank_on_stand_in(fake, layout, update_first):
    n, m, Nt, T = 3, 2, 5, 7
    d = _bank_model(n, m, Nt, T, 3)
    b = InformationFilterBank(n, m, Nt, layout=layout)
    b.F, b.H, b.Q, b.R_inv, b.x, b.P_inv = d["F"], d["H"], d["Q"], d["Rinv"], d["x0"], d["Pinv0"]
    zs = d["zs"].copy()
    zs[2, 1] = np.nan                                     # a missing measurement
    mask = np.ones((T, Nt), dtype=bool)
    mask[4, 3] = False
    x_before, P_before = b.x.copy(), b.P_inv.copy()
    mu, cov, mu_p, cov_p = b.batch_filter(zs, mask=mask, update_first=update_first)
    assert mu.shape == (T, Nt, n) and cov.shape == (T, Nt, n, n)
    assert np.array_equal(b.x, x_before) and np.array_equal(b.P_inv, P_before)
    keep = ~np.isnan(zs).any(axis=2) & mask
    want = ip.batch_tracks(d["x0"], d["Pinv0"], np.nan_to_num(zs), d["F"], d["Q"], d["H"], d["Rinv"], mask=keep,
                           update_first=update_first)
    for got, w in zip((mu, cov, mu_p, cov_p), want):
        assert rel_err(got, w) <= 1e-12
    assert rel_err(b.P, np.linalg.inv(d["Pinv0"])) <= 1e-12
    # the step methods: predict / update on the bank = the same run (predict first)
    if not update_first:
        for t in range(T):
            b.predict()
            b.update(zs[t], mask=mask[t])
            assert rel_err(b.x, mu[t]) <= 1e-12 and rel_err(b.P_inv, cov[t]) <= 1e-12
        assert b.y.shape == (Nt, m) and b.K.shape == (Nt, n, m)
        b.update(zs[0], R_inv=2.0)
        b.update(zs[0], R_inv=np.eye(m) * 2.0)
    e = b.batch_filter(zs[:0])
    assert e[0].shape == (0, Nt, n) and e[1].shape == (0, Nt, n, n)
    with pytest.raises(ValueError):
        b.batch_filter(zs[:, :, :1])
    with pytest.raises(ValueError):
        b.batch_filter(zs, us=np.ones((T, Nt, 2)))        # us without B
    b.B = np.ones((n, 2))
    us = np.ones((T, Nt, 2))
    b.x, b.P_inv = x_before, P_before
    got = b.batch_filter(np.nan_to_num(zs), us=us, update_first=update_first)
    want = ip.batch_tracks(d["x0"], d["Pinv0"], np.nan_to_num(zs), d["F"], d["Q"], d["H"], d["Rinv"], B=b.B, us=us,
                           update_first=update_first)
    for g_, w in zip(got, want):
        assert rel_err(g_, w) <= 1e-12


# ---- the fast kernels' ISA ------------------------------------------------------------------------------------------------
def test_fast_kernels_have_no_scratch_and_fit_the_instruction_cache():
    objs = sorted(glob.glob(os.path.join(ROOT, "filterpy_amd", "csrc", "build", "inst_info_*.o")))
    if not objs:
        pytest.skip("library not built here")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import isa_lint
    finally:
        sys.path.remove(os.path.join(ROOT, "tools"))
    import re
    import tempfile
    want = set(re.findall(r"^FK_INFO_INST\((\d+),\s*(\d+)\)", open(os.path.join(ROOT, "filterpy_amd", "csrc",
                                                                                "fk_dims_info.def")).read(), re.M))
    assert {(str(a), str(b)) for a in range(1, 5) for b in range(1, a + 1)} <= want and ("6", "3") in want
    assert len(objs) == len(want)
    seen = 0
    with tempfile.TemporaryDirectory() as tmp:
        for o in objs:
            for name, k in isa_lint.kernels(isa_lint.device_elf(o, tmp)).items():
                if "info_fast_kernel" not in name:
                    continue
                seen += 1
                assert int(k["scratch"]) == 0, (name, k)
                assert int(k["code"]) <= 65536, (name, k)
    assert seen == 2 * len(objs)
