"""The fixed-lag smoother on the CPU: tests/fls_port.py against the goldens frozen from the live reference (and against the live
reference where the checkout exists), the per-track step of filterpy_amd/csrc/fk_fls.hpp compiled for the host, the drop-in layer
(FixedLagSmoother / FixedLagSmootherBank) on a stand-in engine, and the ISA of the fast kernels."""
import ctypes
import glob
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, golden, rel_err, rel_err_rows
import fls_hp
import fls_port
from filterpy_amd.kalman import FixedLagSmoother, FixedLagSmootherBank

REF = os.environ.get("FILTERPY_REFERENCE", "/root/reference")
G = golden("fls")
NC = int(G["n_cases"])


def case(ci):
    p = f"c{ci}_"
    n, m, lag, nd, ctrl, scal, zsc = (int(v) for v in G[p + "spec"])
    d = dict(n=n, m=m, lag=lag, nd=nd, ctrl=ctrl, scal=scal, zsc=zsc)
    for k in ("F", "Q", "H", "R", "P0", "x0", "zs", "xs", "xhat", "us", "B"):
        if p + k in G.files:
            d[k] = G[p + k]
    for k in ("Q", "R", "B"):
        if k in d and d[k].ndim == 0:
            d[k] = float(d[k])
    return d


def ref_inputs(c):
    """the case's inputs in the shapes the reference was given"""
    n, m, T = c["n"], c["m"], c["zs"].shape[0]
    x0 = c["x0"].copy() if c["nd"] == 1 else c["x0"].reshape(n, 1).copy()
    zs = c["zs"][:, 0] if c["zsc"] else (c["zs"] if c["nd"] == 1 else c["zs"].reshape(T, m, 1))
    us = None
    if "us" in c:
        us = c["us"] if c["nd"] == 1 else c["us"].reshape(T, -1, 1)
    B = c.get("B", 0.)
    return x0, zs, us, B


@pytest.mark.parametrize("ci", range(NC))
def test_port_matches_golden(ci):
    c = case(ci)
    x0, zs, us, B = ref_inputs(c)
    xs, xhat = fls_port.smooth_batch(x0, c["P0"], zs, c["lag"], c["F"], c["Q"], c["H"], c["R"], B=B, us=us)
    assert xs.shape == c["xs"].shape
    assert rel_err_rows(xs, c["xs"]) <= 1e-13
    assert rel_err_rows(xhat, c["xhat"]) <= 1e-13


def test_port_smooth_sequence_matches_golden():
    for si, (n, m, lag, nd, ctrl) in enumerate(G["seqs"]):
        p = f"s{si}_"
        x0 = G[p + "x0"] if nd == 1 else G[p + "x0"].reshape(n, 1)
        B = G[p + "B"] if p + "B" in G.files else 0.
        sp = fls_port.SmoothPort(x0, G[p + "P0"], int(lag), G[p + "F"], G[p + "Q"], G[p + "H"], G[p + "R"], B=B)
        for k in range(G[p + "zs"].shape[0]):
            z = G[p + "zs"][k] if nd == 1 else G[p + "zs"][k].reshape(m, 1)
            u = None
            if p + "us" in G.files:
                u = G[p + "us"][k] if nd == 1 else G[p + "us"][k].reshape(-1, 1)
            sp.smooth(z, u)
            q = f"{p}k{k}_"
            assert rel_err_rows(np.array(sp.xSmooth), G[q + "xSmooth"]) <= 1e-13
            assert rel_err_rows(sp.x[None], G[q + "x"][None]) <= 1e-13


def test_port_matches_live_reference_on_random_cases():
    if not os.path.isdir(os.path.join(REF, "filterpy")):
        pytest.skip("no reference checkout here")
    sys.path.insert(0, REF)
    try:
        from filterpy.kalman import FixedLagSmoother as RefFLS
    finally:
        sys.path.remove(REF)
    rs = np.random.RandomState(7)
    for n, m, lag, T in ((4, 2, 8, 40), (6, 3, 16, 50), (9, 3, 3, 30), (2, 1, 0, 10), (3, 3, 25, 20)):
        F = np.eye(n) + 0.1 * rs.randn(n, n) / np.sqrt(n)
        A = rs.randn(n, n)
        f = RefFLS(n, m)
        f.F, f.H, f.Q, f.R, f.P = F, rs.randn(m, n), 0.01 * (A @ A.T + np.eye(n)), np.eye(m) * 0.7, np.eye(n) * 3
        f.x = rs.randn(n)
        zs = rs.randn(T, m)
        a = f.smooth_batch(zs, lag)
        b = fls_port.smooth_batch(f.x, f.P, zs, lag, f.F, f.Q, f.H, f.R)
        assert rel_err_rows(a[0], b[0]) <= 1e-13 and rel_err_rows(a[1], b[1]) <= 1e-13


# ---- fk_fls.hpp compiled for the host -----------------------------------------------------------------------------------
HC_SRC = r'''
#include "fk_fls.hpp"
using namespace fk;
// the register shapes: -DHC_NX/-DHC_NZ/-DHC_LMAX builds one entry of fk_dims_fls.def at its exact dims; the default is a padded
// (16, 8) model that serves every golden case
#ifndef HC_NX
#define HC_NX 16
#define HC_NZ 8
#define HC_LMAX 24
#endif
constexpr int NX = HC_NX, NZ = HC_NZ, LMAX = HC_LMAX;
// one track through fls_step, the shift register's rows written out as the kernel does.  Pout, yout, Sout (NULL: not
// wanted) receive the final P and the last step's y and S.
extern "C" int hc_fls(int n, int m, int lag, long T, const double *F, const double *Q, const double *H, const double *R,
                      int nu, const double *B, const double *us, const double *zs, int rj, double *x0, double *P0,
                      double *xs, double *xhat, double *Pout, double *yout, double *Sout)
{
    if (n > NX || m > NZ) return -1;
    RegModel<NX, NZ> M;
    for (int i = 0; i < NX; ++i) for (int j = 0; j < NX; ++j) {
        M.F[i * NX + j] = (i < n && j < n) ? F[i * n + j] : (i == j);
        M.Q[i * NX + j] = (i < n && j < n) ? Q[i * n + j] : 0.0;
    }
    for (int i = 0; i < NZ; ++i) {
        for (int j = 0; j < NX; ++j) M.H[i * NX + j] = (i < m && j < n) ? H[i * n + j] : 0.0;
        for (int j = 0; j < NZ; ++j) M.R[i * NZ + j] = (i < m && j < m) ? R[i * m + j] : (i == j);
    }
    double x[NX] = {}, P[NX * NX] = {}, pend[LMAX * NX] = {}, y[NZ], S[NZ * NZ];
    for (int i = 0; i < NX; ++i) for (int j = 0; j < NX; ++j) P[i * NX + j] = (i < n && j < n) ? P0[i * n + j] : (i == j);
    for (int i = 0; i < n; ++i) x[i] = x0[i];
    const int Lf = lag > 1 ? lag : 1;
    if (Lf > LMAX) return -1;
    int st = 0;
    for (long k = 0; k < T; ++k) {
        double z[NZ] = {}, bu[NX] = {};
        for (int i = 0; i < m; ++i) z[i] = zs[k * m + i];
        for (int i = 0; i < n; ++i) for (int j = 0; j < nu; ++j) bu[i] = (j == 0) ? B[i * nu] * us[k * nu] : fma(B[i * nu + j], us[k * nu + j], bu[i]);
        st |= fls_step<NX, NZ, LMAX>(x, P, z, M, bu, nu > 0, rj != 0, k, lag, pend, y, S);
        for (int i = 0; i < n; ++i) xhat[k * n + i] = x[i];
        const long j = k - Lf + 1;
        if (j >= 0) for (int i = 0; i < n; ++i) xs[j * n + i] = pend[(Lf - 1) * NX + i];
    }
    const long W = Lf - 1 < T ? Lf - 1 : T;
    for (long r = 0; r < W; ++r) for (int i = 0; i < n; ++i) xs[(T - 1 - r) * n + i] = pend[r * NX + i];
    for (int i = 0; i < n; ++i) x0[i] = x[i];
    if (Pout) for (int i = 0; i < n; ++i) for (int j = 0; j < n; ++j) Pout[i * n + j] = P[i * NX + j];
    if (yout) for (int i = 0; i < m; ++i) yout[i] = y[i];
    if (Sout) for (int i = 0; i < m; ++i) for (int j = 0; j < m; ++j) Sout[i * m + j] = S[i * NZ + j];
    return st;
}
'''


def _hc_cmd(src, so, dims=None):
    d = [] if dims is None else ["-DHC_NX=%d" % dims[0], "-DHC_NZ=%d" % dims[1], "-DHC_LMAX=%d" % dims[2]]
    return ["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=on", "-w", *d,
            "-I", os.path.join(ROOT, "filterpy_amd", "csrc"), str(src), "-o", str(so)]


@pytest.fixture(scope="module")
def hc(tmp_path_factory):
    d = tmp_path_factory.mktemp("hc_fls")
    src, so = d / "hc_fls.cpp", d / "libhc_fls.so"
    src.write_text(HC_SRC)
    subprocess.check_call(_hc_cmd(src, so))
    return ctypes.CDLL(str(so))


def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def matrices(c):
    """the golden case's attributes as the engine takes them (Python layer's scalar rules)"""
    n, m = c["n"], c["m"]
    Q = np.full((n, n), c["Q"]) if np.ndim(c["Q"]) == 0 else c["Q"]
    R = np.full((m, m), c["R"]) if np.ndim(c["R"]) == 0 else c["R"]
    rj = int(np.ndim(c["R"]) == 0 and m > 1)
    B = us = None
    if "us" in c:
        B = c["B"] if np.ndim(c["B"]) else np.eye(n) * c["B"]
        us = c["us"]
    return Q, R, rj, B, us


@pytest.mark.parametrize("ci", range(NC))
def test_host_step_matches_golden(hc, ci):
    c = case(ci)
    n, m, lag, T = c["n"], c["m"], c["lag"], c["zs"].shape[0]
    Q, R, rj, B, us = matrices(c)
    cc = lambda a: np.ascontiguousarray(a, dtype=float)      # noqa: E731
    x0, xs, xhat = cc(c["x0"]).copy(), np.zeros((T, n)), np.zeros((T, n))
    nu = 0 if B is None else B.shape[1]
    st = hc.hc_fls(n, m, lag, ctypes.c_long(T), _p(cc(c["F"])), _p(cc(Q)), _p(cc(c["H"])), _p(cc(R)), nu,
                   _p(None if B is None else cc(B)), _p(None if us is None else cc(us)), _p(cc(c["zs"])), rj,
                   _p(x0), _p(cc(c["P0"])), _p(xs), _p(xhat), None, None, None)
    assert st == 0
    assert rel_err_rows(xs, c["xs"].reshape(T, n)) <= 1e-12
    assert rel_err_rows(xhat, c["xhat"].reshape(T, n)) <= 1e-12


# ---- tests/fls_hp.py, the extended-precision truth ------------------------------------------------------------------------
def test_hp_is_extended_precision():
    assert fls_hp.LD is np.longdouble and np.finfo(fls_hp.LD).eps < 1e-18
    one = fls_hp.ld(1.0)
    assert one + fls_hp.ld(2.0 ** -60) != one
    S = fls_hp.ld([[[0.0, 2.0, 1.0], [1.0, 1e-3, 0.0], [3.0, 1.0, 7.0]]])     # a zero pivot: needs the row exchange
    E = fls_hp.inv(S) @ S - np.eye(3, dtype=fls_hp.LD)
    assert fls_hp.inv(S).dtype == fls_hp.LD and float(np.max(np.abs(E))) < 1e-17


@pytest.mark.parametrize("ci", range(NC))
def test_hp_matches_golden(ci):
    c = case(ci)
    n, m, T = c["n"], c["m"], c["zs"].shape[0]
    B, us = c.get("B"), None
    if "us" in c:
        us = c["us"].reshape(T, 1, -1)
    h = fls_hp.smooth_batch(c["x0"].reshape(1, n), c["P0"][None], c["zs"].reshape(T, 1, m), c["lag"], c["F"], c["Q"], c["H"],
                            c["R"], B=B, us=us)
    # normwise over the run: a row that cancels (case 17: 0.09 after rows of 27) carries the golden's float64 error, 2e-12 of it
    assert rel_err(h["xs"][:, 0].astype(float), c["xs"].reshape(T, n)) <= 1e-12
    assert rel_err(h["xhat"][:, 0].astype(float), c["xhat"].reshape(T, n)) <= 1e-12


def _mp_smooth(x0, P0, zs, lag, F, Q, H, R, B=None, us=None):
    """the reference's smooth_batch once more, in mpmath at 40 digits (scalar R: numpy's rule)"""
    import mpmath as mp
    M = lambda a: mp.matrix([[mp.mpf(float(v)) for v in row] for row in np.atleast_2d(a)])     # noqa: E731
    col = lambda v: mp.matrix([mp.mpf(float(e)) for e in np.ravel(v)])                          # noqa: E731
    n, m = len(x0), zs.shape[1]
    F, Q, H = M(F), M(Q), M(H)
    Rm = mp.matrix(m, m) + mp.mpf(float(R)) if np.ndim(R) == 0 else M(R)
    KR_scalar = np.ndim(R) == 0
    if KR_scalar:
        Rm = mp.matrix([[mp.mpf(float(R))] * m for _ in range(m)])
    x, P, I = col(x0), M(P0), mp.eye(n)
    rows, xhat = [], []
    for k in range(zs.shape[0]):
        x_pre = F * x
        if us is not None:
            x_pre = x_pre + (mp.mpf(float(B)) * col(us[k]) if np.ndim(B) == 0 else M(B) * col(us[k]))
        P = F * P * F.T + Q
        y = col(zs[k]) - H * x_pre
        S = H * P * H.T + Rm
        SI = mp.inverse(S)
        K = P * H.T * SI
        x = x_pre + K * y
        IKH = I - K * H
        P = IKH * P * IKH.T + (mp.mpf(float(R)) * K * K.T if KR_scalar else K * Rm * K.T)
        xhat.append(x)
        rows.append(x_pre)
        if k >= lag:
            PS, FLH = P, (F - K * H).T
            for i in range(lag):
                rows[k - i] = rows[k - i] + PS * H.T * SI * y
                PS = PS * FLH
        else:
            rows[k] = x
    to = lambda vs: np.array([[float(e) for e in v] for v in vs])        # noqa: E731
    exact = lambda vs: [[e for e in v] for v in vs]                       # noqa: E731
    return exact(rows), exact(xhat), to(rows)


def _mpf_ld(v):
    """a longdouble exactly: its 64-bit significand is the sum of two doubles"""
    import mpmath as mp
    hi = float(v)
    return mp.mpf(hi) + mp.mpf(float(v - fls_hp.ld(hi)))


@pytest.mark.parametrize("n,m,lag,T,ctrl,scalar_R", [(1, 1, 2, 8, 0, 0), (2, 1, 3, 8, 1, 0), (3, 2, 2, 7, 0, 1),
                                                     (3, 3, 8, 6, 1, 0), (2, 2, 0, 5, 0, 0), (3, 1, -1, 4, 1, 1)])
def test_hp_matches_mpmath(n, m, lag, T, ctrl, scalar_R):
    import mpmath as mp
    mp.mp.dps = 40
    d = fls_hp.random_model(n, m, 1, T, 100 * n + 10 * m + lag, nu=2 if ctrl else 0, scalar_R=bool(scalar_R))
    if ctrl and n == 3 and m == 1:
        d["B"] = 0.5                                        # a scalar B: b u
        d["us"] = np.random.RandomState(1).randn(T, 1, n)
    us = None if d["us"] is None else d["us"][:, 0]
    rows, xhat, _ = _mp_smooth(d["x0"][0], d["P0"][0], d["zs"][:, 0], lag, d["F"], d["Q"], d["H"], d["R"], d["B"], us)
    h = fls_hp.smooth_batch(d["x0"], d["P0"], d["zs"], lag, d["F"], d["Q"], d["H"], d["R"], B=d["B"], us=d["us"])
    for name, ref in (("xs", rows), ("xhat", xhat)):
        for k in range(T):
            scale = max(abs(e) for e in ref[k])
            err = max(abs(_mpf_ld(h[name][k, 0, i]) - ref[k][i]) for i in range(n)) / scale
            assert err <= 1e-17, (name, k, float(err))


# ---- fk_fls.hpp at the exact shapes of fk_dims_fls.def, against tests/fls_hp.py ----------------------------------------------
ENTRIES = fls_hp.fast_entries()
_EXERCISED = set()


@pytest.fixture(scope="module")
def hc_exact(tmp_path_factory):
    """one host build of hc_fls per FK_FLS_INST entry (compiled side by side)"""
    from concurrent.futures import ThreadPoolExecutor
    d = tmp_path_factory.mktemp("hc_fls_exact")
    src = d / "hc_fls.cpp"
    src.write_text(HC_SRC)
    sos = {e: d / ("libhc_fls_%d_%d_%d.so" % e) for e in ENTRIES}
    with ThreadPoolExecutor(max(1, min(8, len(os.sched_getaffinity(0))))) as ex:
        list(ex.map(lambda e: subprocess.check_call(_hc_cmd(src, sos[e], e)), ENTRIES))
    return {e: ctypes.CDLL(str(so)) for e, so in sos.items()}


def _hc_run(lib, d, lag, T):
    """track 0 of model d, first T steps, through one hc_fls build -> the outputs as fls_port / fls_hp name them"""
    cc = lambda a: np.ascontiguousarray(a, dtype=float)      # noqa: E731
    n, m = d["F"].shape[0], d["H"].shape[0]
    scalar_R = np.ndim(d["R"]) == 0
    R = np.full((m, m), d["R"]) if scalar_R else d["R"]
    nu = 0 if d["B"] is None else d["B"].shape[1]
    x, P0 = cc(d["x0"][0]).copy(), cc(d["P0"][0])
    o = dict(xs=np.zeros((T, n)), xhat=np.zeros((T, n)), P=np.zeros((n, n)), y=np.zeros(m), S=np.zeros((m, m)))
    st = lib.hc_fls(n, m, lag, ctypes.c_long(T), _p(cc(d["F"])), _p(cc(d["Q"])), _p(cc(d["H"])), _p(cc(R)), nu,
                    _p(None if nu == 0 else cc(d["B"])), _p(None if nu == 0 else cc(d["us"][:T, 0])), _p(cc(d["zs"][:T, 0])),
                    int(scalar_R and m > 1), _p(x), _p(P0), _p(o["xs"]), _p(o["xhat"]), _p(o["P"]), _p(o["y"]), _p(o["S"]))
    o["x"] = x
    return st, o


def check_exact_entry(lib, e):
    nx, nz, L = e
    for variant in ("plain", "control", "scalar_R"):
        seed = 1000 * nx + 100 * nz + L + {"plain": 0, "control": 1, "scalar_R": 2}[variant]
        d = fls_hp.random_model(nx, nz, 1, 2 * L + 3, seed, nu=2 if variant == "control" else 0,
                                scalar_R=variant == "scalar_R")
        for lag in (-2, 0, 1, 2, L - 1, L):
            for T in (1, L - 1, 2 * L + 3):
                st, got = _hc_run(lib, d, lag, T)
                assert st == 0
                us = None if d["us"] is None else d["us"][:T]
                port = dict(zip(("xs", "xhat", "x", "P", "y", "S"),
                                fls_port.smooth_batch_state(d["x0"][0], d["P0"][0], d["zs"][:T, 0], lag, d["F"], d["Q"],
                                                            d["H"], d["R"], d["B"], None if us is None else us[:, 0])))
                hp = fls_hp.smooth_batch(d["x0"], d["P0"], d["zs"][:T], lag, d["F"], d["Q"], d["H"], d["R"], B=d["B"], us=us)
                fls_hp.compare_track(f"host {e} {variant} lag {lag} T {T}", got, port, hp, family="host exact shapes")
    _EXERCISED.add(e)


@pytest.mark.parametrize("e", ENTRIES, ids=lambda e: "%d_%d_%d" % e)
def test_host_step_exact_shape_vs_hp(hc_exact, e):
    check_exact_entry(hc_exact[e], e)


def test_host_every_def_entry_exercised(hc_exact):
    assert len(ENTRIES) >= 16 and len(set(ENTRIES)) == len(ENTRIES)
    for e in ENTRIES:                          # (run alone, or under a -k that skipped some: exercise the rest here)
        if e not in _EXERCISED:
            check_exact_entry(hc_exact[e], e)
    assert _EXERCISED == set(ENTRIES)


# ---- the drop-in layer on a stand-in engine -----------------------------------------------------------------------------
@pytest.fixture
def fake(monkeypatch):
    import fake_fls_engine
    return fake_fls_engine.install(monkeypatch)


def make_fls(c, N=None):
    x0, zs, us, B = ref_inputs(c)
    f = FixedLagSmoother(c["n"], c["m"], N=N)
    f.F, f.H, f.P, f.Q, f.R, f.x, f.B = c["F"], c["H"], c["P0"], c["Q"], c["R"], x0, B
    return f, zs, us


@pytest.mark.parametrize("ci", range(0, NC, 7))
def test_dropin_smooth_batch_shapes_and_values(fake, ci):
    c = case(ci)
    f, zs, us = make_fls(c)
    x_before, P_before = np.array(f.x), np.array(f.P)
    xs, xhat = f.smooth_batch(zs, c["lag"], us=us)
    assert xs.shape == c["xs"].shape and xhat.shape == c["xhat"].shape
    assert rel_err_rows(xs, c["xs"]) <= 1e-12 and rel_err_rows(xhat, c["xhat"]) <= 1e-12
    assert np.array_equal(f.x, x_before) and np.array_equal(f.P, P_before)      # smooth_batch leaves x and P alone
    assert fake and fake[-1][1] == 0                                            # one launch, k0 = 0


def test_dropin_smooth_sequence_attributes(fake):
    for si, (n, m, lag, nd, ctrl) in enumerate(G["seqs"]):
        p = f"s{si}_"
        f = FixedLagSmoother(int(n), int(m), N=int(lag))
        f.F, f.Q, f.H, f.R, f.P = G[p + "F"], G[p + "Q"], G[p + "H"], G[p + "R"], G[p + "P0"]
        f.x = G[p + "x0"].copy() if nd == 1 else G[p + "x0"].reshape(n, 1).copy()
        if p + "B" in G.files:
            f.B = G[p + "B"] if G[p + "B"].ndim else float(G[p + "B"])
        K0, xs0 = f.K.copy(), f.x_s.copy()
        for k in range(G[p + "zs"].shape[0]):
            z = G[p + "zs"][k] if nd == 1 else G[p + "zs"][k].reshape(m, 1)
            u = None
            if p + "us" in G.files:
                u = G[p + "us"][k] if nd == 1 else G[p + "us"][k].reshape(-1, 1)
            f.smooth(z, u)
            q = f"{p}k{k}_"
            assert f.count == int(G[q + "count"]) == k + 1
            assert len(f.xSmooth) == k + 1
            assert np.array(f.xSmooth).shape == G[q + "xSmooth"].shape
            assert rel_err_rows(np.array(f.xSmooth), G[q + "xSmooth"]) <= 1e-12
            for a in ("x", "P", "y", "S"):
                assert np.shape(getattr(f, a)) == G[q + a].shape, (a, np.shape(getattr(f, a)), G[q + a].shape)
                assert rel_err_rows(np.atleast_2d(getattr(f, a)), np.atleast_2d(G[q + a])) <= 1e-12, a
        assert np.array_equal(f.K, K0) and np.array_equal(f.x_s, xs0)
        assert fake[-1] == (int(lag), G[p + "zs"].shape[0] - 1, 1)            # T = 1 launches with k0 = count


def test_dropin_errors(fake):
    f = FixedLagSmoother(3, 2)
    with pytest.raises(AttributeError):
        f.smooth(np.zeros((2, 1)))                      # built without N (the reference: no xSmooth)
    with pytest.raises(ValueError):
        f.smooth_batch(np.zeros((5, 2)), 2)             # column x, (T, m) zs with m > 1: y would be (m, m)
    f.x = np.zeros(3)
    with pytest.raises(ValueError):
        f.smooth_batch(np.zeros((5, 2, 1)), 2)          # 1-D x, column zs
    with pytest.raises(ValueError):
        f.smooth_batch(np.zeros((5, 2)), 2, us=np.ones((5, 2)))     # scalar B: u must have dim_x entries
    f.B = np.ones((3, 2))
    with pytest.raises(ValueError):
        f.smooth_batch(np.zeros((5, 2)), 2, us=np.ones((5, 3)))     # B has 2 columns
    f.x = np.zeros((3, 1))
    with pytest.raises(ValueError):
        f.smooth_batch(np.zeros((5, 2, 1)), 2, us=np.ones((5, 2)))          # column x, 1-D u: x_pre would be (3, 3)
    f.x = np.zeros(3)
    with pytest.raises(ValueError):
        f.smooth_batch(np.zeros((5, 2)), 2, us=np.ones((5, 2, 1)))          # 1-D x, column u
    f.B, f.N, f.xSmooth = 0.5, 2, []
    with pytest.raises(ValueError):
        f.smooth(np.zeros(2), u=np.ones((3, 1)))                            # scalar B: b u in x's orientation
    f.B = np.ones((3, 2))
    f.x = np.zeros((1, 3))
    with pytest.raises(ValueError):
        f.smooth_batch(np.zeros((5, 2)), 2)
    assert not fake                                     # nothing reached the engine
    assert "FixedLagSmoother object" in repr(FixedLagSmoother(2, 1, N=3))


def test_dropin_bank_on_stand_in(fake):
    rs = np.random.RandomState(3)
    n, m, Nt, T, lag = 3, 2, 5, 9, 3
    b = FixedLagSmootherBank(n, m, Nt, N=lag, layout="aos")
    b.F = np.eye(n) + 0.1 * rs.randn(n, n)
    b.H = rs.randn(m, n)
    b.x = rs.randn(Nt, n)
    zs = rs.randn(T, Nt, m)
    xs, xhat = b.smooth_batch(zs, lag)
    assert xs.shape == (T, Nt, n) and xhat.shape == (T, Nt, n)
    for i in range(Nt):
        a = fls_port.smooth_batch(b.x[i], np.eye(n), zs[:, i], lag, b.F, b.Q, b.H, b.R)
        assert rel_err_rows(xs[:, i], a[0]) <= 1e-12
    for t in range(T):
        b.smooth(zs[t])
    assert np.array_equal(b.xSmooth, xs) and b.count == T
    with pytest.raises(AttributeError):
        FixedLagSmootherBank(n, m, Nt).smooth(zs[0])
    with pytest.raises(ValueError):
        b.smooth_batch(zs[:, :, :1], lag)


# ---- the fast kernels' ISA ------------------------------------------------------------------------------------------------
def test_fast_kernels_have_no_scratch_and_fit_the_instruction_cache():
    objs = sorted(glob.glob(os.path.join(ROOT, "filterpy_amd", "csrc", "build", "inst_fls_*.o")))
    if not objs:
        pytest.skip("library not built here")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import isa_lint
    finally:
        sys.path.remove(os.path.join(ROOT, "tools"))
    import tempfile
    seen = 0
    with tempfile.TemporaryDirectory() as tmp:
        for o in objs:
            for name, k in isa_lint.kernels(isa_lint.device_elf(o, tmp)).items():
                if "fls_fast_kernel" not in name:
                    continue
                seen += 1
                assert int(k["scratch"]) == 0, (name, k)
                assert int(k["code"]) <= 65536, (name, k)
    assert seen == 2 * len(objs)
