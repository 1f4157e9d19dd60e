"""The square-root Kalman filter on the CPU: tests/srkf_port.py (its Householder QR against scipy.linalg.qr, signs included, and
the whole filter against the goldens frozen from the live reference -- and against the live reference where the checkout
exists), the per-track step of filterpy_amd/csrc/fk_srkf.hpp compiled for the host against the port, the drop-in layer
(SquareRootKalmanFilter / SquareRootKalmanFilterBank) on a stand-in engine, and the ISA of the fast kernels."""
import ctypes
import glob
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, golden, rel_err
import srkf_port as sp
from filterpy_amd.kalman import SquareRootKalmanFilter, SquareRootKalmanFilterBank

REF = os.environ.get("FILTERPY_REFERENCE", "/root/reference")
G = golden("srkf")
NC = int(G["n_cases"])
TOL = 1e-12


# ---- the port -------------------------------------------------------------------------------------------------------------
def test_port_qr_matches_scipy_with_signs():
    from scipy.linalg import qr
    rs = np.random.RandomState(5)
    for M, N in ((2, 1), (4, 2), (8, 4), (6, 6), (9, 9), (24, 24), (32, 16)):
        A = rs.randn(M, N)
        R, Rs = sp.qr_r(A), qr(A)[1]
        assert np.max(np.abs(R - Rs)) <= 1e-13 * np.max(np.abs(Rs))
        assert np.array_equal(np.sign(np.diag(R)), np.sign(np.diag(Rs)))
    # an exactly zero sub-column (column 1) and the last column of a square matrix: nothing reflected, alpha keeps its sign
    A = np.array([[2., 0, 0, 0], [0, -3, 0, 0], [1, 0, 4, 0], [0, 0, 0, 5.]])
    R, Rs = sp.qr_r(A), qr(A)[1]
    assert np.allclose(R, Rs, rtol=0, atol=1e-15) and R[1, 1] == -3 and R[3, 3] == 5 and R[0, 0] < 0
    assert np.array_equal(np.sign(np.diag(R)), np.sign(np.diag(Rs)))


def check_case_against_golden(make, ci, tol):
    c = sp.case(G, ci)
    f = make(c)
    for k, op in enumerate(c["ops"]):
        sp.run_op(f, c, k, op)
        for a, mine in (("x", f.x), ("_P1_2", f.L if isinstance(f, sp.Port) else f._P1_2)):
            ref = sp.attr(G, c["p"], k, a)
            assert rel_err(np.ravel(mine), np.ravel(ref)) <= tol, (ci, k, a)
        if isinstance(f, sp.Port) and f.K is not None:
            for a, mine in (("K", f.K), ("y", f.y), ("S1_2", f.S12), ("SI1_2", f.SI12)):
                assert rel_err(np.ravel(mine), np.ravel(sp.attr(G, c["p"], k, a))) <= tol, (ci, k, a)


@pytest.mark.parametrize("ci", range(NC))
def test_port_matches_golden(ci):
    check_case_against_golden(lambda c: sp.Port(c["n"], c["m"]).set(c), ci, 1e-12)


def test_port_matches_golden_reference_test_model():
    """square_root.py's own test model: exactly zero sub-columns in every update's QR"""
    p = sp.Port(2, 2)
    p.F, p.H = np.array([[1., 1.], [0., 1.]]), np.eye(2)
    p.Q12, p.R12, p.L = np.eye(2) * 0.01, np.eye(2) * np.sqrt(5.), np.eye(2) * np.sqrt(1000.)
    p.x = np.array([2., 0.])
    for k in range(30):
        p.update(G["t_zs"][k])
        assert rel_err(p.L, sp.attr(G, "t_", 2 * k, "_P1_2")) <= 1e-13
        assert rel_err(p.S12, sp.attr(G, "t_", 2 * k, "S1_2")) <= 1e-13
        p.predict()
        assert rel_err(p.x, np.ravel(sp.attr(G, "t_", 2 * k + 1, "x"))) <= 1e-12
        assert rel_err(p.L, sp.attr(G, "t_", 2 * k + 1, "_P1_2")) <= 1e-13


def test_port_matches_live_reference_on_random_cases():
    if not os.path.isdir(os.path.join(REF, "filterpy")):
        pytest.skip("no reference checkout here")
    sys.path.insert(0, REF)
    try:
        from filterpy.kalman import SquareRootKalmanFilter as RefSRKF
    finally:
        sys.path.remove(REF)
    rs = np.random.RandomState(9)
    for n, m in ((4, 2), (6, 3), (9, 3), (3, 3), (16, 8)):
        A = rs.randn(n, n)
        f = RefSRKF(n, m)
        f.F, f.H = np.eye(n) + 0.1 * rs.randn(n, n) / np.sqrt(n), rs.randn(m, n)
        f.Q, f.R, f.P = 0.01 * (A @ A.T + np.eye(n)), np.eye(m) * 0.7, np.eye(n) * 3
        f.x = rs.randn(n)
        p = sp.Port(n, m)
        p.F, p.H, p.Q12, p.R12, p.L, p.x = f.F, f.H, f._Q1_2, f._R1_2, f._P1_2.copy(), f.x.copy()
        for _ in range(20):
            z = rs.randn(m)
            f.predict()
            p.predict()
            f.update(z)
            p.update(z)
            assert rel_err(p.x, f.x) <= 1e-12 and rel_err(p.L, f._P1_2) <= 1e-12 and rel_err(p.K, f.K) <= 1e-12


# ---- fk_srkf.hpp compiled for the host ------------------------------------------------------------------------------------
HC_SRC = r'''
#include "fk_srkf.hpp"
using namespace fk;
#ifndef HC_NX
#define HC_NX 16
#define HC_NZ 8
#endif
constexpr int NX = HC_NX, NZ = HC_NZ;
// the model padded as the general kernel pads it (identity in F and R1_2, zeros in Q1_2 and H)
static void model(RegModel<NX, NZ> &M, int n, int m, const double *F, const double *Q12, const double *H, const double *R12)
{
    for (int i = 0; i < NX; ++i) for (int j = 0; j < NX; ++j) {
        M.F[i * NX + j] = (F && i < n && j < n) ? F[i * n + j] : (i == j);
        M.Q[i * NX + j] = (Q12 && i < n && j < n) ? Q12[i * n + j] : 0.0;
    }
    for (int i = 0; i < NZ; ++i) {
        for (int j = 0; j < NX; ++j) M.H[i * NX + j] = (H && i < m && j < n) ? H[i * n + j] : 0.0;
        for (int j = 0; j < NZ; ++j) M.R[i * NZ + j] = (R12 && i < m && j < m) ? R12[i * m + j] : (i == j);
    }
}
static void load(int n, const double *x0, const double *L0, double (&x)[NX], double (&L)[NX * NX])
{
    for (int i = 0; i < NX; ++i) x[i] = i < n ? x0[i] : 0.0;
    for (int i = 0; i < NX; ++i) for (int j = 0; j < NX; ++j) L[i * NX + j] = (i < n && j < n) ? (j <= i ? L0[i * n + j] : 0.0) : (i == j);
}
static void save(int n, const double (&x)[NX], const double (&L)[NX * NX], double *x0, double *L0)
{
    for (int i = 0; i < n; ++i) x0[i] = x[i];
    for (int i = 0; i < n; ++i) for (int j = 0; j < n; ++j) L0[i * n + j] = L[i * NX + j];
}
extern "C" int hc_predict(int n, const double *F, const double *Q12, int nu, const double *B, const double *u, double *x0, double *L0)
{
    if (n > NX) return -1;
    RegModel<NX, NZ> M;
    model(M, n, 1, F, Q12, nullptr, nullptr);
    double x[NX], L[NX * NX], bu[NX] = {};
    load(n, x0, L0, x, L);
    for (int i = 0; i < n; ++i) for (int j = 0; j < nu; ++j) bu[i] = j == 0 ? B[i * nu] * u[0] : fma(B[i * nu + j], u[j], bu[i]);
    srkf_predict<NX>(x, L, M, bu, nu > 0);
    save(n, x, L, x0, L0);
    return 0;
}
extern "C" int hc_update(int n, int m, const double *H, const double *R12, const double *z0, double *x0, double *L0,
                         double *y0, double *K0, double *S0, double *SI0)
{
    if (n > NX || m > NZ) return -1;
    RegModel<NX, NZ> M;
    model(M, n, m, nullptr, nullptr, H, R12);
    double x[NX], L[NX * NX], z[NZ] = {}, y[NZ], K[NX * NZ], S[NZ * NZ], SI[NZ * NZ];
    load(n, x0, L0, x, L);
    for (int i = 0; i < m; ++i) z[i] = z0[i];
    const int st = srkf_update<NX, NZ>(x, L, z, M, m, y, K, S, SI);
    save(n, x, L, x0, L0);
    for (int i = 0; i < m; ++i) y0[i] = y[i];
    for (int i = 0; i < n; ++i) for (int j = 0; j < m; ++j) K0[i * m + j] = K[i * NZ + j];
    for (int i = 0; i < m; ++i) for (int j = 0; j < m; ++j) { S0[i * m + j] = S[i * NZ + j]; SI0[i * m + j] = SI[i * NZ + j]; }
    return st;
}
'''
EXACT = [(2, 2), (4, 2), (6, 3)]


def _hc_cmd(src, so, dims=None):
    d = [] if dims is None else ["-DHC_NX=%d" % dims[0], "-DHC_NZ=%d" % dims[1]]
    return ["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=on", "-w", *d,
            "-I", os.path.join(ROOT, "filterpy_amd", "csrc"), str(src), "-o", str(so)]


@pytest.fixture(scope="module")
def hc(tmp_path_factory):
    """the padded (16, 8) build (what the general kernel runs) and exact builds of a few fast shapes"""
    d = tmp_path_factory.mktemp("hc_srkf")
    src = d / "hc_srkf.cpp"
    src.write_text(HC_SRC)
    libs = {}
    for dims in [None] + EXACT:
        so = d / ("libhc_srkf%s.so" % ("" if dims is None else "_%d_%d" % dims))
        subprocess.check_call(_hc_cmd(src, so, dims))
        libs[dims] = ctypes.CDLL(str(so))
    return libs


def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


class HostFilter(sp.Port):
    """the port's interface, computed by one hc_srkf build"""

    def __init__(self, lib, n, m):
        super().__init__(n, m)
        self.lib = lib

    def predict(self, u=None):
        cc = lambda a: np.ascontiguousarray(a, dtype=float)      # noqa: E731
        B = uu = None
        nu = 0
        if u is not None:
            uu = cc(np.ravel(u))
            B = cc(self.B if np.ndim(self.B) else np.eye(self.n) * self.B)
            nu = B.shape[1]
        x, L = cc(self.x).copy(), cc(self.L).copy()
        assert self.lib.hc_predict(self.n, _p(cc(self.F)), _p(cc(self.Q12)), nu, _p(B), _p(uu), _p(x), _p(L)) == 0
        self.x, self.L = x, L

    def update(self, z, R2=None):
        if z is None:
            return
        cc = lambda a: np.ascontiguousarray(a, dtype=float)      # noqa: E731
        n, m = self.n, self.m
        R12 = self.R12 if R2 is None else (np.eye(m) * R2 if np.isscalar(R2) else R2)
        x, L = cc(self.x).copy(), cc(self.L).copy()
        y, K, S, SI = np.zeros(m), np.zeros((n, m)), np.zeros((m, m)), np.zeros((m, m))
        self.st = self.lib.hc_update(n, m, _p(cc(self.H)), _p(cc(R12)), _p(cc(np.ravel(z))), _p(x), _p(L), _p(y), _p(K), _p(S),
                                     _p(SI))
        self.x, self.L, self.y, self.K, self.S12, self.SI12 = x, L, y, K, S, SI


@pytest.mark.parametrize("ci", range(NC))
def test_host_step_matches_golden(hc, ci):
    c = sp.case(G, ci)
    check_case_against_golden(lambda c: HostFilter(hc[None], c["n"], c["m"]).set(c), ci, 1e-12)
    if (c["n"], c["m"]) in EXACT:
        check_case_against_golden(lambda c: HostFilter(hc[(c["n"], c["m"])], c["n"], c["m"]).set(c), ci, 1e-12)


@pytest.mark.parametrize("dims", [None] + EXACT)
def test_host_step_vs_port_with_both_no_reflection_cases(hc, dims):
    """structured models where LAPACK reflects nothing: exactly zero sub-columns (diagonal P1_2, H = I) and the last column of
    the square M; the host step must keep alpha with its own sign exactly where the port (= scipy's qr) does"""
    n, m = (2, 2) if dims is None else dims
    rs = np.random.RandomState(n * 10 + m)
    for variant in range(3):
        h, p = HostFilter(hc[dims], n, m), sp.Port(n, m)
        F = np.eye(n) + (np.diag(np.ones(n - 1), 1) if variant == 0 else 0.1 * rs.randn(n, n))
        H = np.eye(m, n) if variant < 2 else rs.randn(m, n)
        L0 = np.diag(rs.rand(n) + 0.5) if variant < 2 else np.tril(rs.randn(n, n)) + 3 * np.eye(n)
        for o in (h, p):
            o.F, o.H, o.Q12, o.R12, o.L, o.x = F, H, np.eye(n) * 0.01, np.eye(m) * 2.0, L0.copy(), rs.randn(n) * 0 + 1.0
        for k in range(6):
            z = rs.randn(m)
            for o in (h, p):
                o.update(z)
            assert h.st == 0
            assert np.array_equal(np.sign(np.diag(h.L)), np.sign(np.diag(p.L))), (variant, k, np.diag(h.L), np.diag(p.L))
            assert np.array_equal(np.sign(np.diag(h.S12)), np.sign(np.diag(p.S12)))
            for a in ("x", "L", "K", "y", "S12", "SI12"):
                assert rel_err(getattr(h, a), getattr(p, a)) <= TOL, (variant, k, a)
            for o in (h, p):
                o.predict()
            assert np.array_equal(np.sign(np.diag(h.L)), np.sign(np.diag(p.L)))
            assert rel_err(h.L, p.L) <= TOL and rel_err(h.x, p.x) <= TOL


def test_host_step_flags_a_singular_S(hc):
    h = HostFilter(hc[None], 3, 2)
    h.F, h.H, h.Q12, h.R12, h.L, h.x = np.eye(3), np.array([[1., 0, 0], [1., 0, 0]]), np.eye(3), np.zeros((2, 2)), np.eye(3), np.ones(3)
    h.update(np.ones(2))
    assert h.st == 1                                        # two identical rows of H, R = 0: S1_2 has a zero pivot


# ---- the drop-in layer on a stand-in engine -----------------------------------------------------------------------------
@pytest.fixture
def fake(monkeypatch):
    import fake_srkf_engine
    return fake_srkf_engine.install(monkeypatch)


def check_dropin_case(c, f):
    for k, op in enumerate(c["ops"]):
        sp.run_op(f, c, k, op)
        for a in sp.ATTRS:
            ref, mine = sp.attr(G, c["p"], k, a), np.asarray(getattr(f, a), dtype=float)
            assert mine.shape == ref.shape, (k, a, mine.shape, ref.shape)
            assert rel_err(mine, ref) <= 1e-10, (k, a)
        P1_2, P1_2_prior = sp.attr(G, c["p"], k, "_P1_2"), sp.attr(G, c["p"], k, "_P1_2_prior")
        assert rel_err(f.P, P1_2 @ P1_2.T) <= 1e-10
        assert rel_err(f.P_prior, P1_2_prior @ P1_2_prior.T) <= 1e-10
        assert rel_err(f.P_post, P1_2_prior @ P1_2_prior.T) <= 1e-10          # the reference's quirk: the prior's product
        S12, SI12 = sp.attr(G, c["p"], k, "S1_2"), sp.attr(G, c["p"], k, "SI1_2")
        assert rel_err(f.S, S12 @ S12.T) <= 1e-10 and rel_err(f.SI, SI12.T @ SI12) <= 1e-10
        if op == sp.UPDATE_NONE:
            assert f.z.shape == (c["m"], 1) and all(v is None for v in f.z.ravel())


@pytest.mark.parametrize("ci", range(NC))
def test_dropin_sequences_attributes(fake, ci):
    c = sp.case(G, ci)
    f = sp.setup(SquareRootKalmanFilter(c["n"], c["m"]), c)
    check_dropin_case(c, f)
    assert len(fake) == sum(op != sp.UPDATE_NONE for op in c["ops"])     # one launch per call, none for update(None)


def test_dropin_reference_test_model(fake):
    f = SquareRootKalmanFilter(dim_x=2, dim_z=2)
    f.x = np.array([[2.], [0.]])
    f.F = np.array([[1., 1.], [0., 1.]])
    f.H = np.array([[1., 0.], [0., 1.]])
    f.P = np.eye(2) * 1000.
    f.R *= 5
    f.Q *= 0.0001
    str(f)
    for k in range(30):
        f.update(G["t_zs"][k].reshape(2, 1))
        for a in sp.ATTRS:
            assert rel_err(np.asarray(getattr(f, a), dtype=float), sp.attr(G, "t_", 2 * k, a)) <= 1e-10, a
        f.predict()
        assert rel_err(f.x, sp.attr(G, "t_", 2 * k + 1, "x")) <= 1e-10


def test_dropin_properties_and_quirks(fake):
    f = SquareRootKalmanFilter(3, 2)
    A = np.array([[4., 1, 0], [1, 3, 0.5], [0, 0.5, 2]])
    f.P = A
    assert f._P is A and np.allclose(f.P1_2 @ f.P1_2.T, A) and np.all(np.triu(f.P1_2, 1) == 0)
    f.Q = A * 0.1
    f.R = np.eye(2) * 4.
    assert np.allclose(f.Q1_2, np.linalg.cholesky(A * 0.1)) and np.allclose(f.R1_2, 2 * np.eye(2))
    assert f.residual_of(np.ones((2, 1))).shape == (2, 1) and f.measurement_of_state(np.ones((3, 1))).shape == (2, 1)
    assert "SquareRootKalmanFilter object" in repr(f)
    f.H = np.array([[1., 0, 0], [0, 1, 0]])
    f.predict()
    f.update(np.ones((2, 1)))
    assert np.array_equal(f.P_post, f.P_prior) and not np.allclose(f.P_post, f.P)


def test_dropin_errors(fake):
    with pytest.raises(ValueError):
        SquareRootKalmanFilter(0, 1)
    with pytest.raises(ValueError):
        SquareRootKalmanFilter(2, 0)
    with pytest.raises(ValueError):
        SquareRootKalmanFilter(2, 1, dim_u=-1)
    f = SquareRootKalmanFilter(3, 2)
    with pytest.raises(ValueError):
        f.update(np.zeros(2))                             # column x, (m,) z with m > 1: y would be (m, m)
    with pytest.raises(ValueError):
        f.update(np.zeros((2, 1)), R2=np.ones((2, 2)))    # an R2 with an upper triangle
    with pytest.raises(ValueError):
        f.predict(np.ones(3))                             # scalar B: b u in x's orientation (column)
    f.B = np.ones((3, 2))
    with pytest.raises(ValueError):
        f.predict(np.ones((3, 1)))                        # B has 2 columns
    with pytest.raises(ValueError):
        f.predict(2.0)                                    # nonzero scalar u with a matrix B
    f.x = np.zeros(3)
    with pytest.raises(ValueError):
        f.update(np.zeros((2, 1)))                        # 1-D x, column z
    f.x = np.zeros((1, 3))
    with pytest.raises(ValueError):
        f.predict()
    assert not fake                                       # nothing reached the engine
    g = SquareRootKalmanFilter(2, 1)
    g.H = np.array([[1., 0.]])
    g.predict(0)                                          # u = 0 with the scalar B: no control input
    g.B = 0.5
    g.predict(2.0)                                        # scalar u, scalar B: b u on every entry, as numpy does
    assert np.allclose(g.x, 1.0)


def test_dropin_singular_S_raises(fake):
    f = SquareRootKalmanFilter(3, 2)
    f.H = np.array([[1., 0, 0], [1., 0, 0]])
    f.R = np.eye(2)
    with pytest.raises(np.linalg.LinAlgError):
        f.update(np.ones((2, 1)), R2=0.0)


def _bank_model(n, m, Nt, T, seed):
    rs = np.random.RandomState(seed)
    A = rs.randn(n, n)
    return dict(F=np.eye(n) + 0.1 * rs.randn(n, n) / np.sqrt(n), Q=0.01 * (A @ A.T + np.eye(n)), H=rs.randn(m, n),
                R=np.eye(m) * 0.8, x0=rs.randn(Nt, n), P0=np.eye(n)[None] * (1.0 + rs.rand(Nt, 1, 1)), zs=rs.randn(T, Nt, m))


@pytest.mark.parametrize("layout", ["soa", "aos"])
@pytest.mark.parametrize("update_first", [False, True])
def test_dropin_bank_on_stand_in(fake, layout, update_first):
    n, m, Nt, T = 3, 2, 5, 7
    d = _bank_model(n, m, Nt, T, 3)
    b = SquareRootKalmanFilterBank(n, m, Nt, layout=layout)
    b.F, b.H, b.Q, b.R, b.x, b.P = d["F"], d["H"], d["Q"], d["R"], d["x0"], d["P0"]
    zs = d["zs"].copy()
    zs[2, 1] = np.nan                                     # a missing measurement
    mask = np.ones((T, Nt), dtype=bool)
    mask[4, 3] = False
    x_before = b.x.copy()
    mu, cov, mu_p, cov_p = b.batch_filter(zs, mask=mask, update_first=update_first)
    assert mu.shape == (T, Nt, n) and cov.shape == (T, Nt, n, n) and np.array_equal(b.x, x_before)
    for i in range(Nt):
        keep = ~np.isnan(zs[:, i]).any(axis=1) & mask[:, i]
        r = sp.batch(d["x0"][i], np.linalg.cholesky(d["P0"][i]), np.nan_to_num(zs[:, i]), d["F"], b.Q1_2, d["H"], b.R1_2,
                     mask=keep, update_first=update_first)
        for got, want in zip((mu, cov, mu_p, cov_p), r[:4]):
            assert rel_err(got[:, i], want) <= 1e-12
    # the step methods: predict / update on the bank = the same run (predict first)
    if not update_first:
        for t in range(T):
            b.predict()
            b.update(zs[t], mask=mask[t])
            assert rel_err(b.x, mu[t]) <= 1e-12 and rel_err(b.P1_2, cov[t]) <= 1e-12
    with pytest.raises(ValueError):
        b.batch_filter(zs[:, :, :1])
    with pytest.raises(ValueError):
        b.batch_filter(zs, us=np.ones((T, Nt, 2)))        # us without B


# ---- the fast kernels' ISA ------------------------------------------------------------------------------------------------
def test_fast_kernels_have_no_scratch_and_fit_the_instruction_cache():
    objs = sorted(glob.glob(os.path.join(ROOT, "filterpy_amd", "csrc", "build", "inst_srkf_*.o")))
    if not objs:
        pytest.skip("library not built here")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import isa_lint
    finally:
        sys.path.remove(os.path.join(ROOT, "tools"))
    import re
    import tempfile
    want = set(re.findall(r"^FK_SRKF_INST\((\d+),\s*(\d+)\)", open(os.path.join(ROOT, "filterpy_amd", "csrc",
                                                                                "fk_dims_srkf.def")).read(), re.M))
    assert {(str(a), str(b)) for a in range(1, 5) for b in range(1, a + 1)} <= want and ("6", "3") in want
    assert len(objs) == len(want)
    seen = 0
    with tempfile.TemporaryDirectory() as tmp:
        for o in objs:
            for name, k in isa_lint.kernels(isa_lint.device_elf(o, tmp)).items():
                if "srkf_fast_kernel" not in name:
                    continue
                seen += 1
                assert int(k["scratch"]) == 0, (name, k)
                assert int(k["code"]) <= 65536, (name, k)
    assert seen == 2 * len(objs)


# ---- tests/srkf_hp.py, the extended-precision truth of tests/test_gpu_srkf_precision.py -------------------------------------
def test_hp_is_extended_precision_and_agrees_with_the_port():
    import srkf_hp
    assert np.finfo(srkf_hp.LD).eps < 1e-18
    A = np.random.RandomState(1).randn(9, 5)
    assert np.max(np.abs(srkf_hp.qr_r(A).astype(float) - sp.qr_r(A))) <= 1e-14
    n, m, T = 4, 2, 12
    rs = np.random.RandomState(4)
    F, H = np.eye(n) + 0.1 * rs.randn(n, n), rs.randn(m, n)
    Q12, R12, L0 = np.eye(n) * 0.1, np.eye(m) * 0.5, np.linalg.cholesky(np.eye(n) * 2)
    zs, x0 = rs.randn(T, m), rs.randn(n)
    hp, port = srkf_hp.batch(x0, L0, zs, F, Q12, H, R12), sp.batch(x0, L0, zs, F, Q12, H, R12)
    for a, b in zip(hp, port[:4]):
        assert rel_err(a.astype(float), b) <= 1e-13
        assert a.dtype == srkf_hp.LD
