"""The cubature Kalman filter on the CPU: tests/ckf_port.py against the goldens frozen from the live reference (and against the
live reference where the checkout exists), tests/ckf_hp.py, the per-track arithmetic of filterpy_amd/csrc/fk_ckf.hpp compiled
for the host against the goldens and the port (its NOT_PD flag and the factor of the precision bar included), the drop-in layer
(CubatureKalmanFilter in its four modes) on a stand-in engine, and the ISA of the fast kernels."""
import ctypes
import json
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, golden, rel_err
import ckf_models
import ckf_port as cp
from filterpy_amd.kalman import CubatureKalmanFilter, ckf_transform, spherical_radial_sigmas

REF = os.environ.get("FILTERPY_REFERENCE", "/root/reference")
G = golden("ckf")
SPECS = cp.specs()
TOL = 1e-12
STATE = ("x", "P", "x_prior", "P_prior", "x_post", "P_post", "K", "y", "S", "SI", "sigmas_f", "sigmas_h")


# ---- the port -------------------------------------------------------------------------------------------------------------
def check_case_against_golden(make, spec, tol, attrs=STATE):
    d = cp.inputs(*spec[:4])
    f = make(spec, d)
    p = f"c{spec[0]}_"
    for k in range(cp.n_ops(spec)):
        cp.run_op(f, spec, d, k)
        for a in attrs:
            ref, mine = cp.attr(G, p, k, a), np.asarray(getattr(f, a), dtype=float)
            if ref is None:
                continue
            assert mine.shape == ref.shape, (spec, k, a, mine.shape, ref.shape)
            assert rel_err(mine, ref) <= tol, (spec, k, a)
    return f


@pytest.mark.parametrize("spec", SPECS)
def test_port_matches_golden(spec):
    check_case_against_golden(lambda s, d: cp.make(cp.Port, s, d), spec, 1e-13)


def test_goldens_cover_what_they_should():
    assert [tuple(d) for d in G["dims"]] == [(1, 1), (2, 1), (2, 2), (4, 2), (6, 3), (9, 4), (12, 4), (16, 8)]
    assert int(G["n_cases"]) == len(SPECS) == 16
    seen = set()
    for spec in SPECS:
        ops = cp.SEQ[spec[4]][:cp.n_ops(spec)]
        seen |= {("op", o) for o in ops} | {("kind", spec[3]), ("custom", spec[5]), ("first", ops[0])}
        seen |= {("twice", a == b == cp.UPDATE) for a, b in zip(ops, ops[1:])}
        assert np.array_equal(G[f"c{spec[0]}_spec"], np.array(spec))
    assert seen >= {("op", o) for o in range(6)} | {("kind", 0), ("kind", 1), ("custom", 0), ("custom", 1),
                                                    ("first", cp.PREDICT), ("first", cp.UPDATE), ("twice", True)}
    assert cp.attr(G, "c0_", 0, "x").shape == (1, 1) and cp.attr(G, "c6_", 0, "x").shape == (4, 1)   # a column after predict()
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "ckf.npz")) <= os.path.getsize(
        os.path.join(ROOT, "tests", "golden", "info.npz"))


def test_custom_residual_matters_in_the_goldens():
    """at least one golden update wraps a bearing: without residual_wrap the port leaves the golden"""
    hit = 0
    for spec in SPECS:
        if not spec[5]:
            continue
        d = cp.inputs(*spec[:4])
        f, g = cp.make(cp.Port, spec, d), cp.make(cp.Port, spec, d)
        g.residual_z = np.subtract
        for k in range(cp.n_ops(spec)):
            cp.run_op(f, spec, d, k)
            cp.run_op(g, spec, d, k)
        hit += not np.allclose(f.x, g.x, rtol=1e-9, atol=0)
    assert hit >= 1


def test_port_matches_golden_reference_test_model():
    """the model of the reference's test_1d: Q H' = 0 and H Q H' = 0, where the cubature filter IS the linear Kalman filter"""
    F, H = np.array([[1., 1], [0, 1.1]]), np.array([[1., 0.]])
    f = cp.Port(2, 1, 0.1, lambda x: x[0:1], lambda x, dt: F @ x)
    f.x, f.P, f.R, f.Q = np.array([[1.], [2.]]), np.array([[1, 1.1], [1.1, 3]]), np.eye(1) * .05, np.array([[0., 0], [0., .001]])
    x, P = f.x.copy(), f.P.copy()
    for k in range(50):
        f.predict()
        assert rel_err(f.P, cp.attr(G, "t_", 2 * k, "P")) <= 1e-13 and rel_err(f.x, cp.attr(G, "t_", 2 * k, "x")) <= 1e-13
        f.update(np.array([[G["t_zs"][k]]]))
        assert rel_err(f.P, cp.attr(G, "t_", 2 * k + 1, "P")) <= 1e-13 and rel_err(f.x, cp.attr(G, "t_", 2 * k + 1, "x")) <= 1e-13
        assert rel_err(f.K, cp.attr(G, "t_", 2 * k + 1, "K")) <= 1e-13
        # ... and the linear Kalman filter's equations give the same numbers on this model (and on this model only)
        x, P = F @ x, F @ P @ F.T + f.Q
        S = H @ P @ H.T + f.R
        K = P @ H.T / S
        x, P = x + K * (G["t_zs"][k] - H @ x), P - K @ S @ K.T
        assert rel_err(x, f.x) <= 1e-9 and rel_err(P, f.P) <= 1e-9


def _model(n, m, rs):
    return dict(F=np.eye(n) + 0.1 * rs.randn(n, n) / np.sqrt(n), H=rs.randn(m, n), Q=cp.spd(rs, n, 0.02), R=cp.spd(rs, m, 0.5))


def _ref_class():
    if not os.path.isdir(os.path.join(REF, "filterpy")):
        pytest.skip("no reference checkout here")
    sys.path.insert(0, REF)
    try:
        from filterpy.kalman import CubatureKalmanFilter as RefCKF
    finally:
        sys.path.remove(REF)
    return RefCKF


def test_port_matches_live_reference_on_random_cases():
    RefCKF = _ref_class()
    rs = np.random.RandomState(9)
    for n, m in ((4, 2), (6, 3), (9, 4), (3, 3), (16, 8)):
        d = _model(n, m, rs)
        fs = [cls(n, m, 1.0, lambda s: d["H"] @ s, lambda s, dt: d["F"] @ s) for cls in (RefCKF, cp.Port)]
        x0, P0 = rs.randn(n), cp.spd(rs, n, 0.7)
        for f in fs:
            f.x, f.P, f.Q, f.R = x0.copy(), P0.copy(), d["Q"], d["R"]
        for _ in range(20):
            z = rs.randn(m, 1)
            for f in fs:
                f.predict()
                f.update(z)
            for a in ("x", "P", "K", "S", "SI", "y", "sigmas_f", "sigmas_h"):
                assert rel_err(getattr(fs[1], a), getattr(fs[0], a)) <= 1e-13, a


def test_cubature_filter_is_not_the_kalman_filter_with_a_general_q():
    """update() reuses the points of predict(): Q never reaches Pxz or H P H'.  With Q H' != 0 the port leaves the linear
    Kalman filter's equations at the 1e-2 level and beyond -- the truth of every other test is the reference, never KalmanFilter"""
    rs = np.random.RandomState(5)
    n, m = 4, 2
    d = _model(n, m, rs)
    x0, P0, zs = rs.randn(n), cp.spd(rs, n, 0.7), rs.randn(30, m)
    mu = cp.batch(x0, P0, zs, d["F"], d["Q"] * 50, d["H"], d["R"])[0]
    x, P = x0.copy(), P0.copy()
    for t in range(30):
        x, P = d["F"] @ x, d["F"] @ P @ d["F"].T + d["Q"] * 50
        S = d["H"] @ P @ d["H"].T + d["R"]
        K = P @ d["H"].T @ np.linalg.inv(S)
        x, P = x + K @ (zs[t] - d["H"] @ x), P - K @ S @ K.T
    assert rel_err(mu[-1], x) > 1e-3


# ---- tests/ckf_hp.py, the extended-precision truth ----------------------------------------------------------------------------
def test_hp_is_extended_precision_and_agrees_with_the_port():
    import ckf_hp
    assert np.finfo(ckf_hp.LD).eps < 1e-18
    A = cp.spd(np.random.RandomState(1), 7, 2.0)
    U = ckf_hp.chol_upper(A)
    assert U.dtype == ckf_hp.LD and float(np.max(np.abs(U.T @ U - ckf_hp.ld(A)))) <= 1e-17
    assert np.max(np.abs(U.astype(float) - np.linalg.cholesky(A).T)) <= 1e-14 and np.array_equal(U, np.triu(U))
    n, m, T = 4, 2, 12
    rs = np.random.RandomState(4)
    d = _model(n, m, rs)
    zs, x0, P0 = rs.randn(T, m), rs.randn(n), cp.spd(rs, n, 0.7)
    hp = ckf_hp.batch(x0, P0, zs, d["F"], d["Q"], d["H"], d["R"])
    port = cp.batch(x0, P0, zs, d["F"], d["Q"], d["H"], d["R"])
    for a, b in zip(hp, port[:4]):
        assert rel_err(a.astype(float), b) <= 1e-13
        assert a.dtype == ckf_hp.LD


def test_precision_models_are_hard_and_the_port_stays_sound_on_them():
    """condition 1e8, means 1e3 spreads out, and still the float64 port keeps 1e-6 on P over the 30 steps"""
    for dims in ckf_models.DIMS:
        d = ckf_models.model(dims)
        assert ckf_models.T == 30 and 1e7 < np.linalg.cond(d["P0"][0]) < 1e9
        assert np.max(np.abs(d["x0"]) / np.sqrt(np.einsum("nii->ni", d["P0"]))) > 900
        ep = ckf_models.truth(dims)[1]
        assert ep[1].max() < 1e-6 and ep[3].max() < 1e-6, (dims, ep.max(axis=1))


# ---- fk_ckf.hpp compiled for the host -----------------------------------------------------------------------------------------
HC_SRC = r'''
#include "fk_ckf.hpp"
using namespace fk;
#ifndef HC_NX
#define HC_NX 16
#define HC_NZ 8
#endif
constexpr int NX = HC_NX, NZ = HC_NZ;
// the model padded as the kernels pad it (identity in F and R, zeros in Q and H)
static void model(RegModel<NX, NZ> &M, int n, int m, const double *F, const double *Q, const double *H, const double *R)
{
    for (int i = 0; i < NX; ++i) for (int j = 0; j < NX; ++j) {
        M.F[i * NX + j] = (F && i < n && j < n) ? F[i * n + j] : (i == j);
        M.Q[i * NX + j] = (Q && i < n && j < n) ? Q[i * n + j] : 0.0;
    }
    for (int i = 0; i < NZ; ++i) {
        for (int j = 0; j < NX; ++j) M.H[i * NX + j] = (H && i < m && j < n) ? H[i * n + j] : 0.0;
        for (int j = 0; j < NZ; ++j) M.R[i * NZ + j] = (R && i < m && j < m) ? R[i * m + j] : (i == j);
    }
}
// x, P (its upper triangle mirrored, as the kernel's lane does) and the points record c | E
static void load(int n, const double *x0, const double *P0, const double *pts, double (&x)[NX], double (&P)[NX * NX],
                 double (&c)[NX], double (&E)[NX * NX])
{
    for (int i = 0; i < NX; ++i) { x[i] = i < n ? x0[i] : 0.0; c[i] = (pts && i < n) ? pts[i] : 0.0; }
    for (int i = 0; i < NX; ++i) for (int j = 0; j < NX; ++j) {
        const int lo = i < j ? i : j, hi = i < j ? j : i;
        P[i * NX + j] = (hi < n) ? P0[lo * n + hi] : (i == j);
        E[i * NX + j] = (pts && i < n && j < n) ? pts[n + i * n + j] : (i == j);
    }
}
static void save(int n, const double (&x)[NX], const double (&P)[NX * NX], double *x0, double *P0)
{
    for (int i = 0; i < n; ++i) x0[i] = x[i];
    for (int i = 0; i < n; ++i) for (int j = 0; j < n; ++j) P0[i * n + j] = P[i * NX + j];
}
static void save_pts(int n, const double (&c)[NX], const double (&E)[NX * NX], double *pts)
{
    for (int i = 0; i < n; ++i) pts[i] = c[i];
    for (int i = 0; i < n; ++i) for (int j = 0; j < n; ++j) pts[n + i * n + j] = E[i * NX + j];
}
static void save_m(int r, int c, int C, const double *A, double *out)
{
    for (int i = 0; i < r; ++i) for (int j = 0; j < c; ++j) out[i * c + j] = A[i * C + j];
}
extern "C" int hc_predict(int n, const double *F, const double *Q, double *x0, double *P0, double *pts)
{
    if (n > NX) return -1;
    RegModel<NX, NZ> M;
    model(M, n, 1, F, Q, nullptr, nullptr);
    double x[NX], P[NX * NX], c[NX], E[NX * NX];
    load(n, x0, P0, pts, x, P, c, E);
    const int st = ckf_linear_predict<NX>(x, P, c, E, M);
    save(n, x, P, x0, P0);
    save_pts(n, c, E, pts);
    return st;
}
extern "C" int hc_update(int n, int m, const double *H, const double *R, const double *z0, double *x0, double *P0,
                         const double *pts, double *y0, double *K0, double *S0, double *SI0)
{
    if (n > NX || m > NZ) return -1;
    RegModel<NX, NZ> M;
    model(M, n, m, nullptr, nullptr, H, R);
    double x[NX], P[NX * NX], c[NX], E[NX * NX], z[NZ] = {}, y[NZ], K[NX * NZ], S[NZ * NZ], Lf[NZ * NZ], dinv[NZ], SI[NZ * NZ];
    load(n, x0, P0, pts, x, P, c, E);
    for (int i = 0; i < m; ++i) z[i] = z0[i];
    const int st = ckf_linear_update<NX, NZ>(x, P, c, E, z, M, y, K, S, Lf, dinv);
    inv_from_ldlt<NZ>(Lf, dinv, SI);
    save(n, x, P, x0, P0);
    save_m(m, 1, 1, y, y0); save_m(n, m, NZ, K, K0); save_m(m, m, NZ, S, S0); save_m(m, m, NZ, SI, SI0);
    return st;
}
// T steps as the kernel's time loop runs them; the four histories out.  mask: 0 = no measurement at that step, or NULL.
extern "C" int hc_batch(int n, int m, int T, const double *F, const double *Q, const double *H, const double *R,
                        const double *zs, const unsigned char *mask, double *x0, double *P0, double *pts, double *mu,
                        double *cov, double *mu_p, double *cov_p)
{
    if (n > NX || m > NZ) return -1;
    RegModel<NX, NZ> M;
    model(M, n, m, F, Q, H, R);
    double x[NX], P[NX * NX], c[NX], E[NX * NX];
    load(n, x0, P0, pts, x, P, c, E);
    int st = 0;
    for (int t = 0; t < T; ++t) {
        st |= ckf_linear_predict<NX>(x, P, c, E, M);
        save(n, x, P, mu_p + t * n, cov_p + t * n * n);
        if (!mask || mask[t]) {
            double z[NZ] = {}, y[NZ], K[NX * NZ], S[NZ * NZ], Lf[NZ * NZ], dinv[NZ];
            for (int i = 0; i < m; ++i) z[i] = zs[t * m + i];
            st |= ckf_linear_update<NX, NZ>(x, P, c, E, z, M, y, K, S, Lf, dinv);
        }
        save(n, x, P, mu + t * n, cov + t * n * n);
    }
    save(n, x, P, x0, P0);
    save_pts(n, c, E, pts);
    return st;
}
// the building blocks
extern "C" int hc_points(int n, const double *x0, const double *P0, double *sig)
{
    if (n > NX) return -1;
    double x[NX], P[NX * NX], c[NX], E[NX * NX];
    load(n, x0, P0, nullptr, x, P, c, E);
    return ckf_points<NX>(n, x, P, [&](int p, int i, double v) { sig[p * n + i] = v; }) ? 0 : ST_NOT_PD;
}
extern "C" void hc_transform(int d, int k, const double *sig, const double *noise, double *xo, double *Po)
{
    double x[NX], P[NX * NX];
    ckf_transform<NX>(d, k, [&](int p, int i) { return sig[p * d + i]; }, noise, x, P);
    save(d, x, P, xo, Po);
}
extern "C" int hc_block_update(int n, int m, const double *sf, const double *sh, const double *R, const double *z0, int z_is_y,
                               double *x0, double *P0, double *zp0, double *S0, double *SI0, double *K0, double *y0,
                               double *Pxz0)
{
    if (n > NX || m > NZ) return -1;
    double x[NX], P[NX * NX], c[NX], E[NX * NX], z[NZ] = {}, zp[NZ], S[NZ * NZ], Pxz[NX * NZ], K[NX * NZ], y[NZ], Lf[NZ * NZ],
        dinv[NZ], SI[NZ * NZ];
    load(n, x0, P0, nullptr, x, P, c, E);
    for (int i = 0; i < m; ++i) z[i] = z0[i];
    const int st = ckf_update<NX, NZ>(n, m, [&](int p, int i) { return sf[p * n + i]; }, [&](int p, int r) { return sh[p * m + r]; },
                                      R, z, z_is_y != 0, x, P, zp, S, Pxz, K, y, Lf, dinv);
    inv_from_ldlt<NZ>(Lf, dinv, SI);
    save(n, x, P, x0, P0);
    save_m(m, 1, 1, zp, zp0); save_m(m, m, NZ, S, S0); save_m(m, m, NZ, SI, SI0); save_m(n, m, NZ, K, K0); save_m(m, 1, 1, y, y0);
    save_m(n, m, NZ, Pxz, Pxz0);
    return st;
}
'''
EXACT = [(2, 1), (4, 2), (6, 3)]


def _hc_cmd(src, so, dims=None, extra=()):
    d = [] if dims is None else ["-DHC_NX=%d" % dims[0], "-DHC_NZ=%d" % dims[1]]
    return ["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=on", "-w", *d, *extra,
            "-I", os.path.join(ROOT, "filterpy_amd", "csrc"), str(src), "-o", str(so)]


@pytest.fixture(scope="module")
def hc(tmp_path_factory):
    """the padded (16, 8) build (what the general kernel and the building blocks run) and exact builds of a few fast shapes"""
    d = tmp_path_factory.mktemp("hc_ckf")
    src = d / "hc_ckf.cpp"
    src.write_text(HC_SRC)
    libs = {}
    for dims in [None] + EXACT:
        so = d / ("libhc_ckf%s.so" % ("" if dims is None else "_%d_%d" % dims))
        subprocess.check_call(_hc_cmd(src, so, dims))
        libs[dims] = ctypes.CDLL(str(so))
    return libs


def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def _cc(a):
    return np.ascontiguousarray(a, dtype=float)


class HostFilter(cp.Port):
    """the port's interface, computed by one hc_ckf build: the matrix-model step where fx / hx are ckf_port's linear callables
    (their arguments are F and H), the building blocks around the Python callables otherwise"""

    def __init__(self, lib, *a, **kw):
        super().__init__(*a, **kw)
        self.lib, self.st, self.pts = lib, 0, np.zeros(self.dim_x + self.dim_x ** 2)

    def predict(self, dt=None, fx_args=()):
        n = self.dim_x
        dt = self._dt if dt is None else dt
        x, P = _cc(np.ravel(self.x)).copy(), _cc(self.P).copy()
        if self.fx is cp.fx_lin:
            self.st = self.lib.hc_predict(n, _p(_cc(fx_args[0])), _p(_cc(self.Q)), _p(x), _p(P), _p(self.pts))
            c, Eh = self.pts[None, :n], self.pts[n:].reshape(n, n) * math.sqrt(n)
            self.sigmas_f = np.concatenate([c + Eh, c - Eh])
        else:
            sig = np.zeros((2 * n, n))
            self.st = self.lib.hc_points(n, _p(x), _p(P), _p(sig))
            self.sigmas_f = _cc([self.fx(s, dt, *fx_args) for s in sig])
            self.lib.hc_transform(n, 2 * n, _p(self.sigmas_f), _p(_cc(self.Q)), _p(x), _p(P))
        self.x, self.P = x.reshape(n, 1), P
        self.x_prior, self.P_prior = self.x.copy(), self.P.copy()

    def update(self, z, R=None, hx_args=()):
        if z is None:
            self.x_post, self.P_post = self.x.copy(), self.P.copy()
            return
        n, m = self.dim_x, self.dim_z
        R = _cc(self.R if R is None else (np.eye(m) * R if np.isscalar(R) else R))
        x, P = _cc(np.ravel(self.x)).copy(), _cc(self.P).copy()
        y, K, S, SI, zp = np.zeros(m), np.zeros((n, m)), np.zeros((m, m)), np.zeros((m, m)), np.zeros(m)
        if self.hx is cp.hx_lin:
            H = _cc(hx_args[0])
            self.st = self.lib.hc_update(n, m, _p(H), _p(R), _p(_cc(np.ravel(z))), _p(x), _p(P), _p(self.pts), _p(y), _p(K),
                                         _p(S), _p(SI))
            self.sigmas_h = self.sigmas_f @ H.T
        else:
            sf = _cc(self.sigmas_f)
            self.sigmas_h = _cc([np.ravel(self.hx(s, *hx_args)) for s in sf])
            zin, z_is_y = _cc(np.ravel(z)), 0
            if self.residual_z is not np.subtract:
                zp0, S0 = np.zeros(m), np.zeros((m, m))
                self.lib.hc_transform(m, 2 * n, _p(self.sigmas_h), _p(R), _p(zp0), _p(S0))
                zin, z_is_y = _cc(np.ravel(self.residual_z(np.reshape(z, (m, 1)), zp0.reshape(m, 1)))), 1
            self.Pxz, self.zp, x_in = np.zeros((n, m)), zp, x.copy()
            self.st = self.lib.hc_block_update(n, m, _p(sf), _p(self.sigmas_h), _p(R), _p(zin), z_is_y, _p(x), _p(P), _p(zp),
                                               _p(S), _p(SI), _p(K), _p(y), _p(self.Pxz))
            # Pxz and zp as CubatureKalmanFilter.py:366-373 forms them, in the reference's order
            want_zp = sum(self.sigmas_h, 0) / (2 * n)
            self.Pxz_port = cp.outer_product_sum(sf - x_in, self.sigmas_h - want_zp) / (2 * n)
            self.zp_port = want_zp
        self.x, self.P, self.y, self.K, self.S, self.SI = x.reshape(n, 1), P, y.reshape(m, 1), K, S, SI
        self.x_post, self.P_post = self.x.copy(), self.P.copy()


def host_batch(lib, n, m, x0, P0, zs, F, Q, H, R, mask=None, pts=None):
    T = len(zs)
    out = [np.zeros((T, n)), np.zeros((T, n, n)), np.zeros((T, n)), np.zeros((T, n, n))]
    x, P = _cc(x0).copy(), _cc(P0).copy()
    pts = np.zeros(n + n * n) if pts is None else _cc(pts).copy()
    mk = None if mask is None else np.ascontiguousarray(mask, dtype=np.uint8)
    st = lib.hc_batch(n, m, T, _p(_cc(F)), _p(_cc(Q)), _p(_cc(H)), _p(_cc(R)), _p(_cc(zs)), _p(mk), _p(x), _p(P), _p(pts),
                      *(_p(o) for o in out))
    return out, st, x, P, pts


def _host_make(lib):
    return lambda s, d: cp.make(lambda *a, **kw: HostFilter(lib, *a, **kw), s, d)


@pytest.mark.parametrize("spec", SPECS)
def test_host_step_matches_golden(hc, spec):
    """the matrix-model step on the linear cases, the building blocks on the nonlinear ones; every attribute after every call"""
    check_case_against_golden(_host_make(hc[None]), spec, TOL)
    if (spec[1], spec[2]) in EXACT:
        check_case_against_golden(_host_make(hc[(spec[1], spec[2])]), spec, TOL)


@pytest.mark.parametrize("spec", [s for s in SPECS if s[3] == cp.NONLINEAR])
def test_host_update_block_cross_variance_and_mean_match_port(hc, spec):
    """the Pxz and zp outputs of the one-launch update, which no attribute of the reference's object shows"""
    d = cp.inputs(*spec[:4])
    f = _host_make(hc[None])(spec, d)
    seen = 0
    for k in range(cp.n_ops(spec)):
        op = cp.run_op(f, spec, d, k)
        if op >= cp.UPDATE and op != cp.UPDATE_NONE:
            seen += 1
            assert f.Pxz.shape == (spec[1], spec[2]) and rel_err(f.Pxz, f.Pxz_port) <= TOL, (spec, k)
            assert rel_err(f.zp, f.zp_port) <= TOL, (spec, k)
    assert seen >= 3


@pytest.mark.parametrize("dims", EXACT + [(3, 2), (5, 4), (9, 4)])
def test_host_batch_matches_port_and_padding_is_exact(hc, dims):
    n, m = dims
    rs = np.random.RandomState(n * 10 + m)
    d = _model(n, m, rs)
    T = 9
    zs, x0, P0 = rs.randn(T, m), rs.randn(n), cp.spd(rs, n, 0.7)
    mask = np.ones(T, dtype=bool)
    mask[4] = False
    want = cp.batch(x0, P0, zs, d["F"], d["Q"], d["H"], d["R"], mask=mask)
    got, st, x, P, pts = host_batch(hc[None], n, m, x0, P0, zs, d["F"], d["Q"], d["H"], d["R"], mask)
    assert st == 0
    for a, b in zip(got, want[:4]):
        assert rel_err(a, b) <= TOL
    assert np.array_equal(x, got[0][-1]) and np.array_equal(P, got[1][-1])
    assert np.array_equal(got[1], np.swapaxes(got[1], -1, -2)) and np.array_equal(got[3], np.swapaxes(got[3], -1, -2))
    c, Eh = pts[None, :n], pts[n:].reshape(n, n) * math.sqrt(n)
    assert rel_err(np.concatenate([c + Eh, c - Eh]), want[4].sigmas_f) <= TOL          # the points record IS sigmas_f
    if dims in EXACT:
        exact = host_batch(hc[dims], n, m, x0, P0, zs, d["F"], d["Q"], d["H"], d["R"], mask)[0]
        for a, b in zip(got, exact):
            assert np.array_equal(a, b)                                         # the padded block adds exact zeros only
    # chained calls reproduce one call bit for bit: the state is x, P and the points
    for cut in (5, 3, 1):
        first, _, x1, P1, pts1 = host_batch(hc[None], n, m, x0, P0, zs[:cut], d["F"], d["Q"], d["H"], d["R"], mask[:cut])
        second = host_batch(hc[None], n, m, x1, P1, zs[cut:], d["F"], d["Q"], d["H"], d["R"], mask[cut:], pts1)[0]
        for a, p, q in zip(got, first, second):
            assert np.array_equal(a, np.concatenate([p, q]))


@pytest.mark.parametrize("dims", [None, (4, 2)])
def test_host_step_flags_a_p_that_is_not_positive_definite(hc, dims):
    n, m = 4, 2
    rs = np.random.RandomState(3)
    d = _model(n, m, rs)
    A = np.linalg.qr(rs.randn(n, n))[0]
    bad = A @ np.diag([2.0, 1.0, 0.5, -0.1]) @ A.T               # one negative eigenvalue
    bad = (bad + bad.T) / 2
    x, P, pts = np.ones(n), bad.copy(), np.zeros(n + n * n)
    with np.errstate(all="ignore"):
        assert hc[dims].hc_predict(n, _p(_cc(d["F"])), _p(_cc(d["Q"])), _p(x), _p(P), _p(pts)) & 1
        sig = np.zeros((2 * n, n))
        assert hc[None].hc_points(n, _p(np.ones(n)), _p(bad.copy()), _p(sig)) & 1
    x, P = np.ones(n), A @ np.diag([2.0, 1.0, 0.5, 0.1]) @ A.T
    assert hc[dims].hc_predict(n, _p(_cc(d["F"])), _p(_cc(d["Q"])), _p(x), _p(_cc(P).copy()), _p(pts)) == 0
    # ... and an S that is not: R negative definite, no points
    y, K, S, SI = np.zeros(m), np.zeros((n, m)), np.zeros((m, m)), np.zeros((m, m))
    with np.errstate(all="ignore"):
        assert hc[dims].hc_update(n, m, _p(_cc(d["H"])), _p(_cc(-np.eye(m))), _p(np.ones(m)), _p(np.ones(n)), _p(np.eye(n)),
                                  _p(np.zeros(n + n * n)), _p(y), _p(K), _p(S), _p(SI)) & 1


def test_host_step_precision_ratio_fixes_the_bar(hc):
    """the factor of tests/test_gpu_ckf_precision.py's bar: the host-compiled step against the port on exactly its models, worst
    per-output ratio of the worst-track errors and of the medians; K_BAR is twice that, rounded up to a power of two"""
    worst = 0.0
    for dims in ckf_models.DIMS:
        n, m = dims
        d = ckf_models.model(dims)
        lib = hc[dims] if dims in hc else hc[None]
        out = [np.zeros((ckf_models.T, ckf_models.NT) + s) for s in ((n,), (n, n), (n,), (n, n))]
        for i in range(ckf_models.NT):
            r, st, *_ = host_batch(lib, n, m, d["x0"][i], d["P0"][i], d["zs"][:, i], d["F"], d["Q"], d["H"], d["R"])
            assert st == 0
            for j in range(4):
                out[j][:, i] = r[j]
        eg, ep = ckf_models.errors(out, dims), ckf_models.truth(dims)[1]
        for j, name in enumerate(ckf_models.OUTPUTS):
            r_max, r_med = eg[j].max() / max(ep[j].max(), 1e-12), np.median(eg[j]) / max(np.median(ep[j]), 1e-12)
            print(dims, name, "host/port worst %.5f medians %.5f; port worst %.1e host worst %.1e" % (r_max, r_med, ep[j].max(),
                                                                                                  eg[j].max()))
            worst = max(worst, r_max, r_med)
    print("worst ratio %.5f" % worst)
    assert 2 * worst <= ckf_models.K_BAR               # (measured: see ckf_models.K_BAR)
    assert ckf_models.K_BAR <= 32                          # a host build that needs more has worse arithmetic, not another order


# ---- the drop-in layer on a stand-in engine -----------------------------------------------------------------------------
@pytest.fixture
def fake(monkeypatch):
    import fake_ckf_engine
    return fake_ckf_engine.install(monkeypatch)


ALL_ATTRS = STATE + ("log_likelihood", "likelihood", "mahalanobis")


@pytest.mark.parametrize("spec", SPECS)
def test_dropin_sequences_attributes(fake, spec):
    """every attribute of the object, shapes included, after every call of the golden sequences (callables, one per point)"""
    f = check_case_against_golden(lambda s, d: cp.make(CubatureKalmanFilter, s, d), spec, 1e-10, ALL_ATTRS)
    ops = cp.SEQ[spec[4]][:cp.n_ops(spec)]
    assert f.z is not None and f.x.shape == (spec[1], 1) and f.y.shape == (spec[2], 1)
    kinds = [c[0] for c in fake]
    assert kinds.count("points") == sum(o in (cp.PREDICT, cp.PREDICT_DT) for o in ops)
    assert kinds.count("update") == sum(o >= cp.UPDATE and o != cp.UPDATE_NONE for o in ops)     # ONE launch per update


@pytest.mark.parametrize("spec", [s for s in SPECS if s[3] == cp.LINEAR])
def test_dropin_matrix_mode_matches_golden(fake, spec):
    """fx = F, hx = H as arrays: the fused single steps, sigmas_f / sigmas_h materialised from the points record"""
    def make(s, d):
        return cp.setup(CubatureKalmanFilter(s[1], s[2], cp.DT, d["H"], d["F"]), s, d)
    f = check_case_against_golden(make, spec, 1e-10, ALL_ATTRS)
    assert {c[0] for c in fake} <= {"lin_predict", "lin_update"}
    assert f.sigmas_f.shape == (2 * spec[1], spec[1]) and f.sigmas_h.shape == (2 * spec[1], spec[2])


def test_dropin_side_by_side_with_the_live_reference(fake):
    RefCKF = _ref_class()
    import warnings
    for spec in SPECS[:10]:
        d = cp.inputs(*spec[:4])
        fs = [cp.make(cls, spec, d) for cls in (RefCKF, CubatureKalmanFilter)]
        for k in range(cp.n_ops(spec)):
            for f in fs:
                cp.run_op(f, spec, d, k)
            for a in ALL_ATTRS:
                try:
                    with warnings.catch_warnings():
                        warnings.simplefilter("ignore")
                        ref = np.array(getattr(fs[0], a), dtype=float)
                except AttributeError:
                    continue
                mine = np.asarray(getattr(fs[1], a), dtype=float)
                assert mine.shape == ref.shape and rel_err(mine, ref) <= 1e-10, (spec, k, a)
            assert np.array_equal(np.asarray(fs[0].z), np.asarray(fs[1].z))


def test_dropin_defaults_and_quirks(fake):
    def hx(x):
        return x[:2]

    def fx(x, dt):
        return x
    f = CubatureKalmanFilter(3, 2, 0.1, hx, fx, x_mean_fn=1, z_mean_fn=2, residual_x=3)
    assert f.x.shape == (3,) and np.array_equal(f.P, np.eye(3)) and np.array_equal(f.Q, np.eye(3)) and np.array_equal(f.R, np.eye(2))
    assert f.K == 0 and f.y == 0 and f.z.shape == (2, 1) and f.z[0, 0] is None and f._dt == 0.1 and f._num_sigmas == 6
    assert f.S.shape == f.SI.shape == (2, 2) and f.sigmas_f.shape == (6, 3) and f.sigmas_h.shape == (6, 2)
    assert (f.x_mean, f.z_mean, f.residual_x) == (1, 2, 3) and f.residual_z is np.subtract      # stored, never called
    assert f.log_likelihood == math.log(sys.float_info.min) and f.likelihood == sys.float_info.min
    for a in ("x_prior", "x_post", "P_prior", "P_post"):
        assert np.array_equal(getattr(f, a), f.x if a[0] == "x" else f.P)
    f.predict()
    assert f.x.shape == (3, 1) and f.x_prior.shape == (3, 1)                     # a column from the first predict on
    f.update(np.ones((2, 1)))
    assert f.y.shape == (2, 1) and f.K.shape == (3, 2) and f.x.shape == (3, 1) and f.mahalanobis >= 0
    x, P = f.x.copy(), f.P.copy()
    f.update(None)
    assert f.z.shape == (2, 1) and f.z[0, 0] is None and np.array_equal(f.x, x) and np.array_equal(f.P_post, P)
    assert "CubatureKalmanFilter object" in repr(f) and "mahalanobis" in repr(f)
    g = CubatureKalmanFilter(1, 1, 1.0, lambda x: x, lambda x, dt: x)
    g.update(2.0)                                             # a scalar measurement, a 1-D x of one entry
    assert g.x.shape == (1, 1) and g.y.shape == (1, 1)


def test_dropin_measurement_shapes_agree(fake):
    rs = np.random.RandomState(2)
    n, m = 4, 2
    d = _model(n, m, rs)
    fs = [CubatureKalmanFilter(n, m, 1.0, d["H"], d["F"]) for _ in range(2)]
    for z in rs.randn(4, m):
        for f, zz in zip(fs, (z, z.reshape(m, 1))):
            f.predict()
            f.update(zz)
        for a in STATE:
            assert np.array_equal(getattr(fs[0], a), getattr(fs[1], a)), a


def test_dropin_errors(fake):
    def hx(x):
        return x[:2]

    def fx(x, dt):
        return x
    with pytest.raises(ValueError):
        CubatureKalmanFilter(0, 1, 1.0, hx, fx)
    with pytest.raises(ValueError):
        CubatureKalmanFilter(2, 1, 1.0, hx, fx, device_callables=True)          # needs a bank
    with pytest.raises(ValueError):
        CubatureKalmanFilter(2, 1, 1.0, hx, fx, layout="rows")
    f = CubatureKalmanFilter(3, 2, 1.0, hx, fx)
    with pytest.raises(ValueError):
        f.update(np.ones((2, 1)))                              # 1-D x before any predict: the reference makes x (3, 3)
    f.predict()
    for z in (np.ones(3), np.ones((1, 2)), 1.0):
        with pytest.raises(ValueError):
            f.update(z)
    with pytest.raises(ValueError):
        f.update(np.ones(2), R=np.ones((3, 3)))
    f.Q = 0.5
    with pytest.raises(ValueError):
        f.predict()
    f.Q, f.x = np.eye(3), np.zeros((1, 3))
    with pytest.raises(ValueError):
        f.predict()
    f.x, f.P = np.zeros(3), np.eye(2)
    with pytest.raises(ValueError):
        f.predict()
    assert [c for c in fake if c[0] != "points" and c[0] != "transform"] == []
    g = CubatureKalmanFilter(3, 2, 1.0, np.eye(2), np.eye(3))   # hx of the wrong shape
    with pytest.raises(ValueError):
        g.predict()
        g.update(np.ones(2))
    b = CubatureKalmanFilter(3, 2, 1.0, np.eye(2, 3), np.eye(3), n_tracks=4)
    with pytest.raises(ValueError):
        b.batch_filter(np.ones((5, 3, 2)))
    with pytest.raises(ValueError):
        b.batch_filter(np.ones((5, 4, 2)), Rs=[1.0])


def test_dropin_not_positive_definite_raises(fake):
    f = CubatureKalmanFilter(3, 2, 1.0, np.eye(2, 3), np.eye(3))
    f.P = np.diag([1.0, -1.0, 1.0])
    with pytest.raises(np.linalg.LinAlgError):
        f.predict()
    g = CubatureKalmanFilter(3, 2, 1.0, lambda x: x[:2], lambda x, dt: x, n_tracks=3)
    g.P = np.diag([1.0, -1.0, 1.0])
    with pytest.raises(np.linalg.LinAlgError):
        g.predict()
    with pytest.raises(np.linalg.LinAlgError):
        f.batch_filter(np.ones((2, 2)))
    with pytest.raises(np.linalg.LinAlgError):
        spherical_radial_sigmas(np.zeros(3), np.diag([1.0, -1.0, 1.0]))


def test_dropin_matrix_mode_refuses_points_that_are_no_pairs(fake):
    rs = np.random.RandomState(4)
    d = _model(3, 2, rs)
    f = CubatureKalmanFilter(3, 2, 1.0, d["H"], d["F"])
    f.x = np.zeros((3, 1))
    f.predict()
    s = np.array(f.sigmas_f)
    f.sigmas_f = s.copy()                                     # +- pairs as predict() left them: read back as a record
    f.update(np.ones(2))
    s[1] += 0.5                                               # one point moved: no centre and half-differences any more
    f.sigmas_f = s
    with pytest.raises(ValueError):
        f.update(np.ones(2))


def test_dropin_step_loop_keeps_the_status_of_an_early_step(fake, monkeypatch):
    """a NOT_PD flag at the first step of the resident loop raises although every later launch reports 0"""
    from filterpy_amd import _engine as E
    rs = np.random.RandomState(4)
    d = _model(3, 2, rs)
    b = CubatureKalmanFilter(3, 2, 1.0, lambda s: s @ d["H"].T, lambda s, dt: s @ d["F"].T, vectorized=True, n_tracks=4)
    real, calls = E.ckf_sigma_points, []

    def flagged(n, N, layout, x, P, sigmas, status=None):
        real(n, N, layout, x, P, sigmas, status)
        calls.append(1)
        if len(calls) == 1:
            status[2] = 1                                     # the first step only; the state stays finite
    monkeypatch.setattr(E, "ckf_sigma_points", flagged)
    with pytest.raises(np.linalg.LinAlgError):
        b.batch_filter(rs.randn(3, 4, 2))
    assert len(calls) == 3


def _bank(mode, n, m, N, d, layout):
    kw = dict(n_tracks=N, layout=layout)
    if mode == "matrix":
        return CubatureKalmanFilter(n, m, 1.0, d["H"], d["F"], **kw)
    if mode == "loop":
        return CubatureKalmanFilter(n, m, 1.0, lambda s: d["H"] @ s, lambda s, dt: d["F"] @ s, **kw)
    if mode == "vec":
        return CubatureKalmanFilter(n, m, 1.0, lambda s: s @ d["H"].T, lambda s, dt: s @ d["F"].T, vectorized=True, **kw)
    import torch
    Ft, Ht = torch.as_tensor(d["F"]), torch.as_tensor(d["H"])
    return CubatureKalmanFilter(n, m, 1.0, lambda s: s @ Ht.T, lambda s, dt: s @ Ft.T, device_callables=True, **kw)


@pytest.mark.parametrize("layout", ["soa", "aos"])
def test_dropin_four_modes_agree_and_batch_filter_is_the_step_loop(fake, layout):
    n, m, N, T = 4, 2, 5, 7
    rs = np.random.RandomState(3)
    d = _model(n, m, rs)
    x0, P0, zs = rs.randn(N, n), np.array([cp.spd(rs, n, 0.7) for _ in range(N)]), rs.randn(T, N, m)
    zl = list(zs)
    zl[3] = None                                              # a step without a measurement
    mask = np.ones((T, N), dtype=bool)
    mask[3] = False
    want = cp.batch_tracks(x0, P0, zs, d["F"], d["Q"], d["H"], d["R"], mask)
    for mode in ("matrix", "loop", "vec", "torch"):
        b = _bank(mode, n, m, N, d, layout)
        b.x, b.P, b.Q, b.R = x0.copy(), P0.copy(), d["Q"], d["R"]
        del fake[:]
        got = b.batch_filter(zl)
        assert [c[0] for c in fake] == ["lin_batch"] if mode == "matrix" else "lin_batch" not in [c[0] for c in fake]
        for g_, w in zip(got, want):
            assert g_.shape == w.shape and rel_err(g_, w) <= 1e-12, mode
        assert rel_err(b.x, want[0][-1]) <= 1e-12 and rel_err(b.P, want[1][-1]) <= 1e-12 and b.x.shape == (N, n)
        assert rel_err(b.x_prior, want[2][-1]) <= 1e-12 and b.sigmas_f.shape == (N, 2 * n, n) and np.array_equal(b.z, zs[-1])
        # the step loop on a fresh object: the same histories, and every by-product a bank's shape
        s = _bank(mode, n, m, N, d, layout)
        s.x, s.P, s.Q, s.R = x0.copy(), P0.copy(), d["Q"], d["R"]
        for t in range(T):
            s.predict()
            assert rel_err(s.x, want[2][t]) <= 1e-12 and rel_err(s.P, want[3][t]) <= 1e-12
            s.update(zl[t])
            assert rel_err(s.x, want[0][t]) <= 1e-12 and rel_err(s.P, want[1][t]) <= 1e-12
        assert s.K.shape == (N, n, m) and s.y.shape == (N, m) and s.S.shape == s.SI.shape == (N, m, m)
        assert s.sigmas_h.shape == (N, 2 * n, m) and rel_err(s.sigmas_f, b.sigmas_f) <= 1e-12
        assert s.log_likelihood.shape == (N,) and s.mahalanobis.shape == (N,)
        # Rs forces the step loop; device_outputs hands over the records
        r = _bank(mode, n, m, N, d, layout)
        r.x, r.P, r.Q, r.R = x0.copy(), P0.copy(), d["Q"], np.eye(m)
        del fake[:]
        dev = r.batch_filter(zl, Rs=[d["R"]] * T, device_outputs=True)
        assert "lin_batch" not in [c[0] for c in fake]
        assert tuple(dev[1].shape) == ((T, N, n * n) if layout == "aos" else (T, n * n, N))
        from filterpy_amd import _engine as E
        assert rel_err(E.from_records(dev[0], layout, 1, (n,)), want[0]) <= 1e-12
    e = _bank("matrix", n, m, N, d, layout).batch_filter(zs[:0])
    assert e[0].shape == (0, N, n) and e[1].shape == (0, N, n, n)


def test_dropin_single_filter_batch_filter_and_saver(fake):
    n, m, T = 4, 2, 6
    rs = np.random.RandomState(8)
    d = _model(n, m, rs)
    x0, P0, zs = rs.randn(n), cp.spd(rs, n, 0.7), rs.randn(T, m)
    want = cp.batch(x0, P0, zs, d["F"], d["Q"], d["H"], d["R"])

    class Saver(object):
        n = 0

        def save(self):
            Saver.n += 1
    for saver in (None, Saver()):
        f = CubatureKalmanFilter(n, m, 1.0, d["H"], d["F"])
        f.x, f.P, f.Q, f.R = x0.copy(), P0.copy(), d["Q"], d["R"]
        got = f.batch_filter(zs, saver=saver)
        for g_, w in zip(got, want[:4]):
            assert g_.shape == w.shape and rel_err(g_, w) <= 1e-12
        assert f.x.shape == (n, 1) and rel_err(f.x[:, 0], want[0][-1]) <= 1e-12 and rel_err(f.sigmas_f, want[4].sigmas_f) <= 1e-12
    assert Saver.n == T


def test_module_functions(fake):
    rs = np.random.RandomState(6)
    x, P = rs.randn(5), cp.spd(rs, 5, 0.7)
    s = spherical_radial_sigmas(x, P)
    assert s.shape == (10, 5) and rel_err(s, cp.spherical_radial_sigmas(x, P)) <= 1e-13
    xm, Pm = ckf_transform(s, np.eye(5) * 0.1)
    wx, wP = cp.ckf_transform(s, np.eye(5) * 0.1)
    assert xm.shape == (5, 1) and rel_err(xm, wx) <= 1e-13 and rel_err(Pm, wP) <= 1e-13


# ---- the fast kernels' ISA ------------------------------------------------------------------------------------------------
def test_fast_kernels_have_no_scratch_and_fit_the_instruction_cache():
    rows = json.load(open(os.path.join(ROOT, "profiles", "ckf", "isa.json")))["rows"]
    want = set(re.findall(r"^FK_CKF_SHAPE\((\d+),\s*(\d+)\)", open(os.path.join(ROOT, "filterpy_amd", "csrc",
                                                                                "fk_dims_ckf.def")).read(), re.M))
    assert {("2", "1"), ("4", "2"), ("6", "3")} <= want
    fast = [r for r in rows if "ckf_fast_kernel" in r["kernel"]]
    assert {r["object"] for r in fast} == {"ckf_fast_%s_%s.o" % d for d in want} and len(fast) == 2 * len(want)
    for r in fast:
        assert r["scratch"] == 0 and r["code"] <= 65536 and r["lds"] <= 160 * 1024, r
    assert any("ckf_general_kernel" in r["kernel"] for r in rows)
