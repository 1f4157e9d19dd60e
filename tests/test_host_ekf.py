"""The extended Kalman filter on the CPU: tests/ekf_port.py against the goldens frozen from the live reference (and against the
live reference where the checkout exists), the class on a stand-in engine side by side with the port / the reference, the
per-track arithmetic of filterpy_amd/csrc/fk_ekf.hpp compiled for the host (one build per listed shape and the padded general
one) against the port and tests/ekf_hp.py -- the factor of the precision bar included --, the same step code as a stand-alone
program under AddressSanitizer and UBSan, the ISA facts of the fast kernels and the refusals of the three entry points."""
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
import ekf_hp
import ekf_models as em
import ekf_port as ep
from filterpy_amd.kalman import ExtendedKalmanFilter

REF = os.environ.get("FILTERPY_REFERENCE", "/root/reference")
G = golden("ekf")
TOL = 1e-12
CSRC = os.path.join(ROOT, "filterpy_amd", "csrc")
SHAPES = [tuple(int(v) for v in s) for s in re.findall(r"^FK_EKF_SHAPE\((\d+),\s*(\d+)\)", open(os.path.join(CSRC, "fk_dims_ekf.def")).read(),
                                                       re.M)]


def _ref_class():
    if not os.path.isdir(os.path.join(REF, "filterpy")):
        return None
    sys.path.insert(0, REF)
    try:
        from filterpy.kalman import ExtendedKalmanFilter as R
        return R
    except ImportError:                                 # the reference needs scipy / matplotlib; anything else is a failure
        return None
    finally:
        sys.path.remove(REF)


def attr(f, a):
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return np.array(getattr(f, a), dtype=float)


def same_attrs(f, g, tol, where):
    for a in em.ATTRS:
        mine, ref = attr(f, a), attr(g, a)
        assert mine.shape == ref.shape, (where, a, mine.shape, ref.shape)
        assert rel_err(mine, ref) <= tol, (where, a, mine, ref)


# ---- the port -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sorted(em.CASES))
def test_port_matches_golden(case):
    f, d = em.make(ep.Port, case)
    for k in range(len(em.OPS)):
        em.run_op(f, case, d, k)
        for a in em.ATTRS:
            ref, mine = G[f"{case}_k{k}_{a}"], attr(f, a)
            assert mine.shape == ref.shape, (case, k, a, mine.shape, ref.shape)
            assert rel_err(mine, ref) <= TOL, (case, k, a)


def test_goldens_cover_what_they_should():
    assert int(G["n_ops"]) == len(em.OPS) and {"predict", "update", "predict_update", "update_none", "update_scalar_R"} == set(em.OPS)
    assert G["radar_k0_x"].shape == (3,) and G["rb_k0_x"].shape == (4, 1) and G["rb_k1_y"].shape == (2, 1)
    # the angle-wrapping residual matters: some update of the range-bearing case sees a bearing difference beyond pi
    f, d = em.make(ep.Port, "rb")
    wrapped = 0
    for k in range(len(em.OPS)):
        if em.OPS[k].startswith("update") and em.OPS[k] != "update_none":
            raw = np.subtract(d["zs"][k], em.rb_hx(f.x))
            wrapped += abs(raw[1, 0]) > math.pi
        em.run_op(f, "rb", d, k)
    assert wrapped >= 1
    # predict_update stores the PRE-predict state as the prior (EKF.py:229-230)
    k = em.OPS.index("predict_update")
    assert np.array_equal(G[f"radar_k{k}_x_prior"], G[f"radar_k{k - 1}_x"])


def test_port_matches_live_reference():
    R = _ref_class()
    if R is None:
        pytest.skip("no reference checkout here (the goldens pin the port)")
    for case in sorted(em.CASES):
        f, d = em.make(ep.Port, case)
        g, _ = em.make(R, case)
        for k in range(len(em.OPS)):
            em.run_op(f, case, d, k)
            em.run_op(g, case, d, k)
            same_attrs(f, g, TOL, (case, k))


def test_hp_is_extended_precision_and_agrees_with_the_port():
    assert np.finfo(ekf_hp.LD).eps < 2e-19
    d = em.model((4, 2))
    a = (d["x0"][0], d["P0"][0], d["zs"][:, 0], d["F"], d["Q"], d["R"], lambda x: em.jac(x, 2), lambda x: em.hx(x, 2))
    hp, port = ekf_hp.batch(*a), ep.batch(*a)
    assert all(h.dtype == ekf_hp.LD for h in hp)
    for j in range(4):
        assert 0 < em.err(port[j], hp[j]) < 1e-9


def test_precision_models_are_hard_and_the_port_stays_sound_on_them():
    """condition 1e8, and the float64 port alone stays finite and below 1e-6 on P for all 30 steps of every model"""
    for dims in em.DIMS:
        d = em.model(dims)
        assert min(np.linalg.cond(P) for P in d["P0"]) > 1e7
        hps, epo = em.truth(dims)
        assert np.isfinite(epo).all() and all(np.isfinite(np.asarray(h, dtype=float)).all() for hp in hps for h in hp)
        assert epo[1].max() < 1e-6 and epo[3].max() < 1e-6, (dims, epo[1].max(), epo[3].max())


def test_precision_callables_are_plus_and_times_only():
    """NumPy and torch agree bit for bit on the CPU too (the GPU test asserts the same on the device)"""
    import torch
    d = em.model((6, 3))
    x = d["x0"]
    assert np.array_equal(em.jac(x, 3), em.jac(torch.as_tensor(x), 3).numpy())
    assert np.array_equal(em.hx(x, 3), em.hx(torch.as_tensor(x), 3).numpy())
    # and the Jacobian is the derivative of hx
    h = 1e-6 * np.abs(x[0]) + 1e-12
    for k in range(6):
        e = np.zeros(6)
        e[k] = h[k]
        fd = (em.hx(x[0] + e, 3) - em.hx(x[0] - e, 3)) / (2 * h[k])
        assert np.allclose(fd, em.jac(x[0], 3)[:, k], rtol=1e-6, atol=1e-9)


# ---- fk_ekf.hpp compiled for the host ---------------------------------------------------------------------------------------
HC_SRC = r'''
#include <string.h>
#include <stdio.h>
#include "fk_ekf.hpp"
#ifndef HC_NX
#define HC_NX 16
#define HC_NZ 8
#endif
using namespace fk;
constexpr int NX = HC_NX, NZ = HC_NZ;

static void pad(int r, int c, int R, int C, const double *src, double *dst, double diag)
{
    for (int i = 0; i < R; ++i)
        for (int j = 0; j < C; ++j) dst[i * C + j] = (src && i < r && j < c) ? src[i * c + j] : (i == j ? diag : 0.0);
}
static void unpad(int r, int c, int C, const double *src, double *dst)
{
    if (!dst) return;
    for (int i = 0; i < r; ++i)
        for (int j = 0; j < c; ++j) dst[i * c + j] = src[i * C + j];
}

struct State {
    double x[NX], P[NX * NX], H[NZ * NX], y[NZ], bu[NX], K[NX * NZ], S[NZ * NZ], Lf[NZ * NZ], dinv[NZ];
    RegModel<NX, NZ> M;
};

static void load(State &s, int n, int m, const double *F, const double *Q, const double *R, const double *H, const double *y,
                 const double *bu, const double *x, const double *P)
{
    pad(n, n, NX, NX, F, s.M.F, 1.0);
    pad(n, n, NX, NX, Q, s.M.Q, 0.0);
    pad(m, m, NZ, NZ, R, s.M.R, 1.0);
    pad(m, n, NZ, NX, nullptr, s.M.H, 0.0);
    pad(m, n, NZ, NX, H, s.H, 0.0);
    pad(m, 1, NZ, 1, y, s.y, 0.0);
    pad(n, 1, NX, 1, bu, s.bu, 0.0);
    pad(n, 1, NX, 1, x, s.x, 0.0);
    pad(n, n, NX, NX, P, s.P, 1.0);
}

static void by_products(State &s, int n, int m, double *K, double *S, double *SI, double *ll, double *maha)
{
    double si[NZ * NZ], l, q;
    inv_from_ldlt<NZ>(s.Lf, s.dinv, si);
    ekf_likelihood<NZ>(s.y, s.Lf, s.dinv, m, l, q);
    unpad(n, m, NZ, s.K, K);
    unpad(m, m, NZ, s.S, S);
    unpad(m, m, NZ, si, SI);
    if (ll) *ll = l;
    if (maha) *maha = q;
}

extern "C" int hc_dims(int which) { return which ? NZ : NX; }

extern "C" int hc_predict(int n, const double *F, const double *Q, const double *bu, double *x, double *P)
{
    static State s;
    load(s, n, 1, F, Q, nullptr, nullptr, nullptr, bu, x, P);
    const int st = ekf_predict<NX>(s.x, s.P, s.bu, s.M);
    unpad(n, 1, 1, s.x, x);
    unpad(n, n, NX, s.P, P);
    return st;
}

extern "C" int hc_update(int n, int m, const double *H, const double *R, const double *y, int rj_diag, double *x, double *P,
                         double *K, double *S, double *SI, double *ll, double *maha)
{
    static State s;
    load(s, n, m, nullptr, nullptr, R, H, y, nullptr, x, P);
    const int st = ekf_update<NX, NZ>(s.x, s.P, s.H, s.y, s.M, s.K, s.S, s.Lf, s.dinv, rj_diag != 0);
    unpad(n, 1, 1, s.x, x);
    unpad(n, n, NX, s.P, P);
    by_products(s, n, m, K, S, SI, ll, maha);
    return st;
}

// update (unless masked), then predict; x_post / P_post receive the posterior
extern "C" int hc_step(int n, int m, const double *H, const double *R, const double *y, int rj_diag, int do_update,
                       const double *F, const double *Q, const double *bu, double *x, double *P, double *x_post, double *P_post,
                       double *K, double *S, double *SI, double *ll, double *maha)
{
    static State s;
    load(s, n, m, F, Q, R, H, y, bu, x, P);
    const int st = ekf_step<NX, NZ>(s.x, s.P, s.H, s.y, s.bu, s.M, s.K, s.S, s.Lf, s.dinv, rj_diag != 0, do_update != 0, true,
                                    [&](const double (&xp)[NX], const double (&Pp)[NX * NX], bool) {
                                        unpad(n, 1, 1, xp, x_post);
                                        unpad(n, n, NX, Pp, P_post);
                                    });
    unpad(n, 1, 1, s.x, x);
    unpad(n, n, NX, s.P, P);
    if (do_update) by_products(s, n, m, K, S, SI, ll, maha);
    return st;
}

#ifdef HC_MAIN
// stand-alone: T steps of a small nonlinear model through hc_step, every output buffer exactly as large as it must be (heap
// blocks: the sanitizer sees a write past any of them), one indefinite S on the way.  Prints a checksum.
#include <stdlib.h>
#include <vector>
int main()
{
    const int dims[3][2] = {{1, 1}, {NX < 4 ? NX : 4, NZ < 2 ? NZ : 2}, {NX, NZ}};
    double sum = 0.0;
    int flagged = 0;
    for (const auto &d : dims) {
        const int n = d[0], m = d[1];
        std::vector<double> F(n * n), Q(n * n), R(m * m), H(m * n), y(m), bu(n), x(n), P(n * n), xp(n), Pp(n * n), K(n * m), S(m * m),
            SI(m * m);
        double ll, maha;
        for (int i = 0; i < n; ++i)
            for (int j = 0; j < n; ++j) {
                F[i * n + j] = (i == j) + 0.01 * ((i * 7 + j * 3) % 5 - 2);
                Q[i * n + j] = (i == j) * 0.01;
                P[i * n + j] = (i == j) * (1.0 + i);
            }
        for (int i = 0; i < m; ++i)
            for (int j = 0; j < m; ++j) R[i * m + j] = (i == j) * 0.5;
        for (int i = 0; i < n; ++i) { x[i] = 0.5 * (i + 1); bu[i] = 0.001 * i; }
        for (int t = 0; t < 6; ++t) {
            for (int r = 0; r < m; ++r) {
                for (int j = 0; j < n; ++j) H[r * n + j] = 0.0;
                H[r * n + r] = 1.0 + 0.01 * x[(r + 1) % n];
                H[r * n + (r + 1) % n] += 0.01 * x[r];
                y[r] = 0.1 * ((t + r) % 3 - 1);
            }
            if (t == 3) R[0] = -1e6;                       // an indefinite S: the status says so, nothing else happens
            const int st = hc_step(n, m, H.data(), R.data(), y.data(), 0, t != 2, F.data(), Q.data(), bu.data(), x.data(), P.data(),
                                   xp.data(), Pp.data(), K.data(), S.data(), SI.data(), &ll, &maha);
            if (t == 3) { R[0] = 0.5; flagged += (st & 1); for (int i = 0; i < n * n; ++i) P[i] = (i % (n + 1) == 0) * 1.0; }
            else if (st) return 3;
            hc_predict(n, F.data(), Q.data(), nullptr, xp.data(), Pp.data());
            hc_update(n, m, H.data(), R.data(), y.data(), m > 1, xp.data(), Pp.data(), nullptr, nullptr, nullptr, nullptr, nullptr);
            for (int i = 0; i < n; ++i) sum += x[i] + xp[i];
        }
    }
    printf("HC_MAIN ok %d %.17g\n", flagged, sum);
    return flagged == 3 ? 0 : 4;
}
#endif
'''


def _hc_cmd(src, out, dims=None, extra=("-shared",)):
    d = [] if dims is None else ["-DHC_NX=%d" % dims[0], "-DHC_NZ=%d" % dims[1]]
    return ["g++", "-O1", "-std=c++17", "-fPIC", "-ffp-contract=on", "-w", *d, *extra, "-I", CSRC, str(src), "-o", str(out)]


@pytest.fixture(scope="module")
def hc(tmp_path_factory):
    """one host build of fk_ekf.hpp per listed shape, and the padded (16, 8) one (what the general kernel runs), side by side"""
    d = tmp_path_factory.mktemp("hc_ekf")
    src = d / "hc_ekf.cpp"
    src.write_text(HC_SRC)
    procs = {}
    for dims in [None] + SHAPES:
        so = d / ("libhc_ekf%s.so" % ("" if dims is None else "_%d_%d" % dims))
        procs[dims] = (so, subprocess.Popen(_hc_cmd(src, so, dims)))
    libs = {}
    for dims, (so, p) in procs.items():
        assert p.wait() == 0, dims
        libs[dims] = ctypes.CDLL(str(so))
    return libs


def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def _cc(a):
    return np.ascontiguousarray(a, dtype=float)


def host_update(lib, x, P, H, R, y, rj=0):
    n, m = len(x), len(y)
    x, P = _cc(x).copy(), _cc(P).copy()
    K, S, SI = np.zeros((n, m)), np.zeros((m, m)), np.zeros((m, m))
    ll, maha = ctypes.c_double(), ctypes.c_double()
    st = lib.hc_update(n, m, _p(_cc(H)), _p(_cc(R)), _p(_cc(y)), rj, _p(x), _p(P), _p(K), _p(S), _p(SI), ctypes.byref(ll),
                       ctypes.byref(maha))
    return st, x, P, K, S, SI, ll.value, maha.value


def host_predict(lib, x, P, F, Q, bu=None):
    x, P = _cc(x).copy(), _cc(P).copy()
    st = lib.hc_predict(len(x), _p(_cc(F)), _p(_cc(Q)), _p(None if bu is None else _cc(bu)), _p(x), _p(P))
    return st, x, P


def host_step(lib, x, P, H, R, y, F, Q, bu=None, rj=0, do_update=1):
    n, m = len(x), len(y)
    x, P = _cc(x).copy(), _cc(P).copy()
    xp, Pp, K, S, SI = np.zeros(n), np.zeros((n, n)), np.zeros((n, m)), np.zeros((m, m)), np.zeros((m, m))
    ll, maha = ctypes.c_double(), ctypes.c_double()
    st = lib.hc_step(n, m, _p(_cc(H)), _p(_cc(R)), _p(_cc(y)), rj, do_update, _p(_cc(F)), _p(_cc(Q)),
                     _p(None if bu is None else _cc(bu)), _p(x), _p(P), _p(xp), _p(Pp), _p(K), _p(S), _p(SI), ctypes.byref(ll),
                     ctypes.byref(maha))
    return st, x, P, xp, Pp, K, S, SI, ll.value, maha.value


def _case(n, m, seed):
    rs = np.random.RandomState(seed)
    A = rs.randn(n, n)
    P = A @ A.T / n + np.eye(n)
    F = np.eye(n) + 0.1 * rs.randn(n, n)
    B = rs.randn(m, m)
    return dict(x=rs.randn(n), P=P, F=F, Q=np.diag(rs.uniform(0.01, 0.1, n)), R=B @ B.T / m + 0.5 * np.eye(m), H=rs.randn(m, n),
                y=rs.randn(m), bu=0.1 * rs.randn(n))


@pytest.mark.parametrize("dims", SHAPES + [(5, 4), (9, 4), (16, 8), (3, 3)])
def test_host_step_matches_port_and_padding_is_exact(hc, dims):
    """predict, update and step of every listed shape's own build and of the padded build against the port, every output and
    by-product; the padded build gives the exact build's bits"""
    n, m = dims
    c = _case(n, m, 100 * n + m)
    libs = [hc[None]] + ([hc[dims]] if dims in hc else [])
    got = []
    for lib in libs:
        assert (lib.hc_dims(0), lib.hc_dims(1)) == ((16, 8) if lib is hc[None] else dims)
        st, x1, P1 = host_predict(lib, c["x"], c["P"], c["F"], c["Q"], c["bu"])
        xr, Pr = ep.predict(c["x"], c["P"], c["F"], c["Q"], np.eye(n), c["bu"])
        assert st == 0 and rel_err(x1, xr) < 1e-13 and rel_err(P1, Pr) < 1e-13
        st, x2, P2, K, S, SI, ll, maha = host_update(lib, c["x"], c["P"], c["H"], c["R"], c["y"])
        xr, Pr, Kr, Sr, SIr = ep.update(c["x"], c["P"], c["H"], c["y"], c["R"])
        assert st == 0
        for a, b in ((x2, xr), (P2, Pr), (K, Kr), (S, Sr), (SI, SIr)):
            assert rel_err(a, b) < 1e-12
        assert abs(ll - ep.loglik(c["y"], Sr)) < 1e-12 * abs(ll) and abs(maha - ep.maha(c["y"], SIr)) < 1e-12 * maha
        # step = update, then predict: the same bits as the two calls, the posterior on the way
        s = host_step(lib, c["x"], c["P"], c["H"], c["R"], c["y"], c["F"], c["Q"], c["bu"])
        st, x3, P3 = host_predict(lib, x2, P2, c["F"], c["Q"], c["bu"])
        assert s[0] == 0 and np.array_equal(s[1], x3) and np.array_equal(s[2], P3)
        assert np.array_equal(s[3], x2) and np.array_equal(s[4], P2) and np.array_equal(s[5], K) and s[8] == ll and s[9] == maha
        # a track without a measurement: the posterior is the state as it was, the predict still runs
        s0 = host_step(lib, c["x"], c["P"], c["H"], c["R"], c["y"], c["F"], c["Q"], c["bu"], do_update=0)
        assert np.array_equal(s0[3], c["x"]) and np.array_equal(s0[4], c["P"]) and np.array_equal(s0[1], x1) and np.array_equal(s0[2], P1)
        got.append((x1, P1, x2, P2, K, S, SI, ll, maha))
    if len(got) == 2:
        for a, b in zip(*got):
            assert np.array_equal(a, b)


@pytest.mark.parametrize("dims", [(3, 2), (4, 4), (9, 4)])
def test_host_update_scalar_r_attribute(hc, dims):
    """FK_KF_FLAG_R_JOSEPH_DIAG: R arrives as r * ones, S gets r on every element, the Joseph term is r K K'"""
    n, m = dims
    c = _case(n, m, 7 * n + m)
    lib = hc[dims] if dims in hc else hc[None]
    st, x, P, K, S, SI, *_ = host_update(lib, c["x"], c["P"], c["H"], np.full((m, m), 0.3), c["y"], rj=1)
    xr, Pr, Kr, Sr, SIr = ep.update(c["x"], c["P"], c["H"], c["y"], None, scalar_r=0.3)
    for a, b in ((x, xr), (P, Pr), (K, Kr), (S, Sr), (SI, SIr)):
        assert rel_err(a, b) < 1e-11


@pytest.mark.parametrize("dims", [(1, 1), (4, 2), (9, 4)])
def test_host_update_flags_an_indefinite_s_and_a_nonfinite_state(hc, dims):
    n, m = dims
    c = _case(n, m, 11 * n + m)
    lib = hc[dims] if dims in hc else hc[None]
    R = c["R"].copy()
    R[m - 1, m - 1] = -1e3 * np.trace(c["H"] @ c["P"] @ c["H"].T)             # the last pivot of S goes negative
    assert host_update(lib, c["x"], c["P"], c["H"], R, c["y"])[0] & 1
    assert host_update(lib, c["x"], c["P"], c["H"], c["R"], c["y"])[0] == 0
    x = c["x"].copy()
    x[0] = np.inf
    assert host_update(lib, x, c["P"], c["H"], c["R"], c["y"])[0] == 2
    assert host_predict(lib, x, c["P"], c["F"], c["Q"])[0] == 2


def host_batch(lib, d, i):
    """ekf_port.batch's histories of track i of a precision model through the host build (predict first)"""
    n, m, T = d["n"], d["m"], em.T
    out = [np.zeros((T, n)), np.zeros((T, n, n)), np.zeros((T, n)), np.zeros((T, n, n))]
    st, x, P = host_predict(lib, d["x0"][i], d["P0"][i], d["F"], d["Q"])
    assert st == 0
    for t in range(T):
        out[2][t], out[3][t] = x, P
        H, y = em.jac(x, m), d["zs"][t, i] - em.hx(x, m)
        if t < T - 1:
            st, x, P, out[0][t], out[1][t], *_ = host_step(lib, x, P, H, d["R"], y, d["F"], d["Q"])
        else:
            st, x, P, *_ = host_update(lib, x, P, H, d["R"], y)
            out[0][t], out[1][t] = x, P
        assert st == 0
    return out


def test_host_step_precision_ratio_fixes_the_bar(hc):
    """the factor of tests/test_gpu_ekf_precision.py's bar: the host-compiled step against the port on exactly its models, worst
    per-output ratio of the worst-track errors and of the medians; K_BAR is twice that, rounded up to a power of two"""
    worst = 0.0
    for dims in em.DIMS:
        n, m = dims
        d = em.model(dims)
        lib = hc[dims] if dims in hc else hc[None]
        out = [np.zeros((em.T, em.NT) + s) for s in ((n,), (n, n), (n,), (n, n))]
        for i in range(em.NT):
            r = host_batch(lib, d, i)
            for j in range(4):
                out[j][:, i] = r[j]
        eg, epo = em.errors(out, dims), em.truth(dims)[1]
        for j, name in enumerate(em.OUTPUTS):
            r_max, r_med = eg[j].max() / epo[j].max(), np.median(eg[j]) / np.median(epo[j])
            print(dims, name, "host/port worst %.5f medians %.5f; port worst %.1e host worst %.1e" % (r_max, r_med, epo[j].max(),
                                                                                                  eg[j].max()))
            worst = max(worst, r_max, r_med)
    print("worst ratio %.5f" % worst)
    assert abs(worst - em.RATIO) <= 0.1 * em.RATIO, (worst, em.RATIO)          # the number written next to K_BAR is this one
    assert 2 * worst <= em.K_BAR
    assert em.K_BAR <= 32                                  # a host build that needs more has worse arithmetic, not another order
    assert em.K_BAR == 2.0 ** math.ceil(math.log2(2 * em.RATIO))


def test_step_code_stand_alone_under_address_and_ub_sanitizers(tmp_path):
    """the same step code as a program of its own (HC_MAIN), built with -fsanitize=address,undefined and run directly: the
    padded (16, 8) build and an exact one.  Nothing is loaded into Python."""
    src = tmp_path / "hc_ekf.cpp"
    src.write_text(HC_SRC)
    for dims in (None, (4, 2)):
        exe = tmp_path / ("hc_ekf_main%s" % ("" if dims is None else "_%d_%d" % dims))
        r = subprocess.run(_hc_cmd(src, exe, dims, extra=("-DHC_MAIN=1", "-g", "-fsanitize=address,undefined",
                                                          "-fno-sanitize-recover=all")), capture_output=True, text=True)
        if r.returncode != 0:
            if re.search(r"cannot find.*(asan|ubsan)|libasan|libubsan", r.stderr):
                pytest.skip("the compiler's sanitizer runtime is not installed here")
            raise AssertionError(r.stderr[-2000:])
        r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and "HC_MAIN ok 3" in r.stdout, (r.returncode, r.stdout[-500:], r.stderr[-2000:])


# ---- the fast kernels' ISA ------------------------------------------------------------------------------------------------
def test_fast_kernels_have_no_scratch_and_fit_the_instruction_cache():
    rows = json.load(open(os.path.join(ROOT, "profiles", "ekf", "isa.json")))["rows"]
    want = set(SHAPES)
    assert {(2, 1), (4, 2), (6, 3)} <= want and (8, 4) not in want
    fast = [r for r in rows if "ekf_fast_kernel" in r["kernel"]]
    # four kernels per object: two record orders x shared / per-track model
    assert {r["object"] for r in fast} == {"ekf_fast_%d_%d.o" % d for d in want} and len(fast) == 4 * len(want)
    for r in fast:
        assert r["scratch"] == 0 and r["code"] <= 65536 and r["lds"] <= 160 * 1024 and r["vgpr"] <= 512, r
    assert sum("ekf_general_kernel" in r["kernel"] for r in rows) == 4


def test_isa_facts_describe_the_built_objects():
    """where the objects are built (every checkout that ran build()): every kernel of the committed facts is there, without scratch"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_lint
    import tempfile
    objs = [os.path.join(CSRC, "build", "ekf_fast_%d_%d.o" % d) for d in SHAPES]
    if not all(os.path.exists(o) for o in objs) or not os.path.exists(f"{isa_lint.LLVM}/llvm-readelf"):
        pytest.skip("no built objects here")
    rows = {(r["object"], r["kernel"]): r for r in json.load(open(os.path.join(ROOT, "profiles", "ekf", "isa.json")))["rows"]}
    with tempfile.TemporaryDirectory() as tmp:
        for o in objs:
            for name, k in isa_lint.kernels(isa_lint.device_elf(o, tmp)).items():
                if "ekf_" in name:
                    r = rows[(os.path.basename(o), isa_lint.short(name))]
                    assert int(k["scratch"]) == 0 == r["scratch"] and int(k["vgpr"]) <= 512, (o, name, k, r)


# ---- the entry points' refusals (no device is touched) ----------------------------------------------------------------------
REFUSALS = r'''
import ctypes, sys
sys.path.insert(0, %r)
from filterpy_amd import _abi
lib = _abi.lib()
BAD, UNS = _abi.FK_ERR_BAD_ARG, _abi.FK_ERR_UNSUPPORTED


def desc(**kw):
    d = dict(n=4, m=2, nu=0, model_mode=0, N=8, T=1, layout=1, update_first=0, alpha_sq=1.0, flags=0)
    d.update(kw)
    return _abi.fk_kf_desc(**d)


def calls(d, ptr):
    return [lib.fk_ekf_predict_f64(ctypes.byref(d), *([ptr] * 8)), lib.fk_ekf_update_f64(ctypes.byref(d), *([ptr] * 13)),
            lib.fk_ekf_step_f64(ctypes.byref(d), *([ptr] * 19))]


buf = (ctypes.c_double * 4096)()
some = ctypes.addressof(buf)
# what the descriptor says is refused whatever the pointers are
for ptr in (None, some):
    for mode in (_abi.FK_MODEL_PER_TRACK_STEP, _abi.FK_MODEL_PER_STEP, 7):
        assert calls(desc(model_mode=mode), ptr) == [UNS] * 3, mode
        assert b"FK_MODEL_SHARED or FK_MODEL_PER_TRACK" in lib.fk_last_error()
    for kw in (dict(n=17), dict(m=9), dict(n=17, m=9), dict(alpha_sq=1.01), dict(update_first=1), dict(flags=2), dict(flags=4)):
        assert calls(desc(**kw), ptr) == [UNS] * 3, kw
    for kw in (dict(n=0), dict(m=0), dict(nu=-1), dict(N=-1), dict(layout=2)):
        assert calls(desc(**kw), ptr) == [BAD] * 3, kw
    # one step's record block is addressed with 32-bit offsets: the control record, and the track's own B [n * nu]
    assert calls(desc(nu=64, N=1 << 23), ptr) == [UNS] * 3
    assert calls(desc(n=16, nu=64, N=1 << 19, model_mode=1), ptr) == [UNS] * 3
    assert lib.fk_ekf_predict_f64(None, *([ptr] * 8)) == BAD
# ... and x, P, H, y of the widest shape
assert calls(desc(n=16, m=8, N=1 << 22), some) == [UNS] * 3
# NULL where data is required; the by-products, the mask and the status may be NULL
for mode in (0, 1):
    assert calls(desc(model_mode=mode), None) == [BAD] * 3
assert lib.fk_ekf_predict_f64(ctypes.byref(desc(nu=1)), some, some, None, None, some, some, None, None) == BAD       # B, u
assert b"dim_u > 0 needs B and u" in lib.fk_last_error()
assert lib.fk_ekf_update_f64(ctypes.byref(desc()), some, some, None, None, some, some, *([None] * 7)) == BAD            # y
assert lib.fk_ekf_step_f64(ctypes.byref(desc()), some, some, some, None, None, some, *([some] * 13)) == BAD            # F
# nothing to do
assert calls(desc(N=0), None) == [0] * 3
assert calls(desc(N=0, model_mode=1, flags=1), None) == [0] * 3
print("REFUSALS_DONE")
'''


def test_entry_points_refuse_what_they_do_not_serve():
    """per-step model modes, sizes above (16, 8), nonsense descriptors, NULL where data is required: FK_ERR_UNSUPPORTED /
    FK_ERR_BAD_ARG before anything is launched.  In a child process that sees no device at all."""
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="", CUDA_VISIBLE_DEVICES="")
    r = subprocess.run([sys.executable, "-c", REFUSALS % ROOT], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and "REFUSALS_DONE" in r.stdout, (r.returncode, r.stdout[-400:], r.stderr[-1500:])


def test_engine_wrappers_hand_every_operand_to_the_parameter_of_its_name(monkeypatch):
    """ekf_predict / ekf_update / ekf_step of filterpy_amd/_engine.py: a distinct tensor per operand, a recording stand-in for the
    library; every pointer must sit at the position of the header parameter that carries the operand's name"""
    import inspect
    import torch
    from filterpy_amd import _abi, _engine as E
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "filterhip.h")).read(), flags=re.S)
    protos = {n: [p.strip().split()[-1].lstrip("*") for p in ps.replace("\n", " ").split(",")]
              for n, ps in re.findall(r"^\s*int\s*(fk_ekf_[a-z0-9_]+)\s*\(([^;{]*?)\)\s*;", src, flags=re.M | re.S)}
    assert set(protos) == {"fk_ekf_predict_f64", "fk_ekf_update_f64", "fk_ekf_step_f64"}
    calls = []

    class Lib:
        def __getattr__(self, name):
            return lambda *a: calls.append((name, a)) or 0
    monkeypatch.setattr(_abi, "lib", lambda: Lib())
    monkeypatch.setattr(E, "_stream", lambda: 4321)
    desc_kw = dict(n=3, m=2, nu=1, model_mode=1, N=5, T=1, layout=1, update_first=0, alpha_sq=1.0, flags=1)
    for wname in ("ekf_predict", "ekf_update", "ekf_step"):
        fn, cname = getattr(E, wname), "fk_" + wname + "_f64"
        tensors = {p: torch.zeros(3, dtype=torch.uint8 if p == "mask" else torch.float64)
                   for p in inspect.signature(fn).parameters if p != "desc_kw"}
        del calls[:]
        fn(desc_kw=dict(desc_kw), **tensors)
        (name, args), cparams = calls[0], protos[cname]
        assert name == cname and len(calls) == 1 and len(args) == len(cparams)
        for pname, t in tensors.items():
            assert args[cparams.index(pname)] == t.data_ptr(), (wname, pname)
        assert args[cparams.index("stream")] == 4321
        d = args[cparams.index("desc")]
        assert all(getattr(d, k) == v for k, v in desc_kw.items())


# ---- the class on a stand-in engine -----------------------------------------------------------------------------------------
@pytest.fixture
def fake(monkeypatch):
    import fake_ekf_engine
    return fake_ekf_engine.install(monkeypatch)


@pytest.mark.parametrize("case", sorted(em.CASES))
def test_dropin_matches_golden_after_every_call(fake, case):
    f, d = em.make(ExtendedKalmanFilter, case)
    for k in range(len(em.OPS)):
        em.run_op(f, case, d, k)
        for a in em.ATTRS:
            ref, mine = G[f"{case}_k{k}_{a}"], attr(f, a)
            assert mine.shape == ref.shape, (case, k, a, mine.shape, ref.shape)
            assert rel_err(mine, ref) <= TOL, (case, k, a)
    kinds = [c[0] for c in fake]
    assert kinds.count("predict") == em.OPS.count("predict") + em.OPS.count("predict_update") and "step" not in kinds


@pytest.mark.parametrize("case", sorted(em.CASES))
def test_dropin_side_by_side_with_the_reference_object(fake, case):
    """the live reference where the checkout exists, its port otherwise: every attribute after every call"""
    R = _ref_class() or ep.Port
    f, d = em.make(ExtendedKalmanFilter, case)
    g, _ = em.make(R, case)
    for k in range(len(em.OPS)):
        em.run_op(f, case, d, k)
        em.run_op(g, case, d, k)
        same_attrs(f, g, TOL, (case, k))
        assert np.array_equal(np.asarray(f.z, dtype=object), np.asarray(g.z, dtype=object))


def test_dropin_defaults_and_quirks(fake):
    R = _ref_class() or ep.Port
    f, g = ExtendedKalmanFilter(3, 2, dim_u=1), R(3, 2, dim_u=1)
    for a in ("dim_x", "dim_z", "dim_u", "x", "P", "B", "F", "R", "Q", "y", "K", "S", "SI", "x_prior", "P_prior", "x_post", "P_post"):
        assert np.array_equal(np.asarray(getattr(f, a)), np.asarray(getattr(g, a))), a
    assert f.z.shape == (2, 1) and f.z[0, 0] is None
    assert f.log_likelihood == g.log_likelihood and f.likelihood == g.likelihood and f.mahalanobis == 0.0
    assert "ExtendedKalmanFilter object" in repr(f) and "log-likelihood" in repr(f)
    # predict_update(None): TypeError before any state is touched
    f.x = np.array([[1.0], [2.0], [3.0]])
    before = {a: np.copy(getattr(f, a)) for a in ("x", "P", "K", "S", "SI", "y", "x_prior")}
    with pytest.raises(TypeError):
        f.predict_update(None, lambda x: np.eye(2, 3), lambda x: x[:2])
    assert all(np.array_equal(before[a], getattr(f, a)) for a in before) and not fake
    # update(None) only copies the posts
    f.update(None, None, None)
    assert np.array_equal(f.x_post, f.x) and f.z.shape == (2, 1) and not fake
    # args / hx_args that are no tuples; a control input through B
    f.B = np.array([[1.0], [0.0], [2.0]])
    g.x, g.B = f.x.copy(), f.B.copy()
    jac, hx = (lambda x, s: s * np.eye(2, 3)), (lambda x, o: x[:2] + o)
    for o in (f, g):
        o.predict(u=np.array([[0.5]]))
        o.update(np.array([[1.0], [2.5]]), jac, hx, args=2.0, hx_args=0.25)
        o.predict_update(np.array([[1.5], [2.0]]), jac, hx, args=(2.0,), hx_args=(0.25,), u=np.array([[0.1]]))
    same_attrs(f, g, TOL, "control")
    assert ("predict", 0, 1) in fake
    # a scalar z with dim_z == 1, a scalar R attribute with dim_z > 1
    f1, g1 = ExtendedKalmanFilter(2, 1), R(2, 1)
    for o in (f1, g1):
        o.x = np.array([0.5, -0.25])          # (1-D: with a column x the reference's x + dot(K, y) broadcasts to (n, n) here)
        o.update(0.7, lambda x: np.array([[1.0, 0.5]]), lambda x: x[0] + 0.5 * x[1])
        o.predict_update(0.9, lambda x: np.array([[1.0, 0.5]]), lambda x: x[0] + 0.5 * x[1])
    same_attrs(f1, g1, TOL, "scalar z")
    for o in (f, g):
        o.R = 0.3
        o.update(np.array([[1.0], [2.0]]), jac, hx, args=2.0, hx_args=0.25)
    same_attrs(f, g, TOL, "scalar R attribute")
    assert fake[-1] == ("update", 0, 1)


def test_dropin_predict_x_override(fake):
    R = _ref_class() or ep.Port

    def mk(base):
        class Own(base):
            def predict_x(self, u=0):
                self.x = self.x * 1.01 + 0.5
        return Own
    f, d = em.make(mk(ExtendedKalmanFilter), "radar")
    g, _ = em.make(mk(R), "radar")
    for k in range(4):
        em.run_op(f, "radar", d, k)
        em.run_op(g, "radar", d, k)
        same_attrs(f, g, TOL, ("override", k))


def test_dropin_errors(fake):
    with pytest.raises(ValueError):
        ExtendedKalmanFilter(2, 1, device_callables=True)
    with pytest.raises(ValueError):
        ExtendedKalmanFilter(2, 1, vectorized=True)
    with pytest.raises(ValueError):
        ExtendedKalmanFilter(0, 1)
    with pytest.raises(ValueError):
        ExtendedKalmanFilter(2, 1, layout="x")
    f = ExtendedKalmanFilter(2, 1)
    with pytest.raises(ValueError):
        f.update(1.0, lambda x: np.eye(2), lambda x: x[0])                       # a Jacobian of the wrong shape
    with pytest.raises(ValueError):
        f.update(1.0, lambda x: np.array([[1.0, 0.0]]), lambda x: x, mask=[True])        # mask on a single filter
    with pytest.raises(ValueError):
        f.batch_filter(np.zeros((2, 1, 1)), None, None)
    f.P = -np.eye(2)
    with pytest.raises(np.linalg.LinAlgError):
        f.update(1.0, lambda x: np.array([[1.0, 0.0]]), lambda x: x[0], R=0.5)   # S = -0.5


def _bank(mode, dims, N, layout, per_track):
    n, m = dims
    rs = np.random.RandomState(17 * n + m)
    b = ExtendedKalmanFilter(n, m, n_tracks=N, layout=layout, vectorized=mode == "vec", device_callables=mode == "torch")
    A = rs.randn(N, n, n)
    b.x, b.P = rs.randn(N, n), A @ np.swapaxes(A, 1, 2) / n + np.eye(n)
    b.F = np.eye(n) + 0.05 * rs.randn(*((N,) if per_track else ()), n, n)
    b.Q = 0.01 * np.eye(n) * (1 + np.arange(N)[:, None, None] if per_track else 1)
    b.R = 0.2 * np.eye(m) * (1 + np.arange(N)[:, None, None] if per_track else 1)
    b.B = rs.randn(*((N,) if per_track else ()), n, 2)
    return b, rs.randn(5, N, m), 0.1 * rs.randn(5, N, 2)


def _callables(mode, m):
    if mode == "loop":
        return (lambda x: em.jac(x[:, 0], m)), (lambda x: em.hx(x[:, 0], m))
    return (lambda x: em.jac(x, m)), (lambda x: em.hx(x, m))


@pytest.mark.parametrize("per_track", [False, True])
@pytest.mark.parametrize("layout", ["soa", "aos"])
def test_dropin_bank_modes_agree_with_single_filters_and_batch_filter_is_the_step_loop(fake, layout, per_track):
    import torch
    dims, N = (4, 2), 5
    n, m = dims
    res = {}
    for mode in ("loop", "vec", "torch"):
        b, zs, us = _bank(mode, dims, N, layout, per_track)
        jac, hx = _callables(mode, m)
        b2, _, _ = _bank(mode, dims, N, layout, per_track)
        del fake[:]
        out = b.batch_filter(zs, jac, hx, us=us)
        kinds = [c[0] for c in fake]
        if mode == "torch":
            assert kinds == ["predict"] + ["step"] * 4 + ["update"]
        else:
            assert kinds == ["predict", "update"] * 5
        assert all(c[1] == int(per_track) for c in fake)
        means, covs, means_p, covs_p = ([], [], [], [])
        for t in range(5):
            b2.predict(us[t])
            means_p.append(b2.x.copy())
            covs_p.append(b2.P.copy())
            b2.update(zs[t], jac, hx)
            means.append(b2.x.copy())
            covs.append(b2.P.copy())
        for a, c in zip(out, (means, covs, means_p, covs_p)):
            assert np.array_equal(np.asarray(a), np.asarray(c))
        same_attrs(b, b2, 0.0, mode)
        res[mode] = out
        if mode == "torch":
            dev = b2.batch_filter(torch.as_tensor(zs), jac, hx, us=us, device_outputs=True)
            assert all(isinstance(t, torch.Tensor) for t in dev)
            assert tuple(dev[1].shape) == ((5, N, n * n) if layout == "aos" else (5, n * n, N))
    for mode in ("vec", "torch"):
        for a, c in zip(res["loop"], res[mode]):
            assert np.array_equal(a, c)
    # ... and every track is the single filter (the port) on its own model
    b, zs, us = _bank("loop", dims, N, layout, per_track)
    for i in range(N):
        g = ep.Port(n, m)
        g.x, g.P = b.x[i].reshape(n, 1).copy(), b.P[i].copy()
        g.F, g.Q, g.R, g.B = (np.asarray(M)[i] if np.ndim(M) == 3 else M for M in (b.F, b.Q, b.R, b.B))
        for t in range(5):
            g.predict(us[t, i].reshape(2, 1))
            assert rel_err(res["loop"][2][t, i], g.x[:, 0]) < TOL and rel_err(res["loop"][3][t, i], g.P) < TOL
            g.update(zs[t, i].reshape(m, 1), lambda x: em.jac(x[:, 0], m), lambda x: em.hx(x[:, 0], m).reshape(m, 1))
            assert rel_err(res["loop"][0][t, i], g.x[:, 0]) < TOL and rel_err(res["loop"][1][t, i], g.P) < TOL


def test_dropin_fused_batch_filter_uploads_the_model_once(fake, monkeypatch):
    """with device callables the uploads of a batch_filter call do not grow with T: F, Q, R, B, the measurements and the controls
    go to the device before the loop"""
    from filterpy_amd import _engine as E
    counts = []
    for T in (2, 5):
        b, zs, us = _bank("torch", (4, 2), 5, "soa", True)
        jac, hx = _callables("torch", 2)
        n_up = [0]
        real = E.dev
        monkeypatch.setattr(E, "dev", lambda a, device=None: (n_up.__setitem__(0, n_up[0] + 1), real(a, device))[1])
        b.batch_filter(zs[:T], jac, hx, us=us[:T])
        monkeypatch.setattr(E, "dev", real)
        counts.append(n_up[0])
        assert b._resident is None
    assert counts[0] == counts[1], counts


def test_dropin_bank_mask_predict_update_and_saver(fake):
    from filterpy_amd.common.helpers import Saver
    dims, N = (3, 2), 4
    n, m = dims
    b, zs, us = _bank("vec", dims, N, "soa", False)
    jac, hx = _callables("vec", m)
    b.predict()
    b.update(zs[0], jac, hx)
    keep = {a: np.copy(getattr(b, a)) for a in ("x", "P", "K", "S", "SI", "y", "log_likelihood", "mahalanobis")}
    b2, _, _ = _bank("vec", dims, N, "soa", False)
    b2.predict()
    b2.update(zs[0], jac, hx)
    mask = np.array([False, True, True, False])
    b.update(zs[1], jac, hx, mask=mask)
    b2.update(zs[1], jac, hx)
    for a in keep:
        got, full = np.asarray(getattr(b, a)), np.asarray(getattr(b2, a))
        assert np.array_equal(got[~mask], keep[a][~mask]) and np.array_equal(got[mask], full[mask]), a
    # predict_update on a bank: H at the state before the predict, Hx at the predicted one, the prior is the pre-predict state
    x_pre = b.x.copy()
    b.predict_update(zs[2], jac, hx, u=us[2])
    assert np.array_equal(b.x_prior, x_pre)
    for i in range(N):
        g = ep.Port(n, m)
        g.x, g.P, g.F, g.Q, g.R, g.B = x_pre[i].reshape(n, 1), b.P_prior[i], b.F, b.Q, b.R, b.B
        g.predict_update(zs[2, i].reshape(m, 1), lambda x: em.jac(x[:, 0], m), lambda x: em.hx(x[:, 0], m).reshape(m, 1),
                         u=us[2, i].reshape(2, 1))
        assert rel_err(b.x[i], g.x[:, 0]) < TOL and rel_err(b.P[i], g.P) < TOL and rel_err(b.K[i], g.K) < TOL
        assert abs(b.log_likelihood[i] - g.log_likelihood) < 1e-10 * abs(g.log_likelihood)
    s = Saver(b)
    b.batch_filter(zs[3:], jac, hx, saver=s)
    assert len(s.x) == 2 and np.array_equal(s.x[-1], b.x)
    with pytest.raises(ValueError):
        b.update(zs[0], jac, hx, mask=[True])
    with pytest.raises(ValueError):
        b.update(zs[0][:2], jac, hx)
