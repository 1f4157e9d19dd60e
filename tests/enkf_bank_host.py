"""fk_enkf.hpp compiled for the host and driven as the two routes of enkf_bank.hip drive it -- one wave per ensemble (N <= 64),
one 256-lane workgroup per ensemble above --: the pivots, the lanes' member order, the group's tree into ONE slab, that slab
through enkf_run_sum / enkf_total with nslabs = 1 (0.0 + slab, then fifteen + 0.0), the finalize entry by entry with
enkf_spd_inverse_in on caller-held work arrays, the dense and the padded gain, the apply (the one-wave route keeps its member
and its h from the first phase) and the new mean.  The driver restates what enkf_bank.hip does around fk_enkf.hpp and changes
with it; tests/test_host_enkf_bank.py holds it bit for bit to the single-ensemble driver of tests/enkf_host.py."""
import ctypes
import os
import subprocess

import numpy as np

from conftest import ROOT
from enkf_host import EXACT, _p, _cc

HB_SRC = r'''
#include <vector>
#include "fk_enkf.hpp"
using namespace fk;
#ifndef HC_NX
#define HC_NX 16
#define HC_NZ 8
#endif
constexpr int NX = HC_NX, NZ = HC_NZ;

static void pad(double *dst, int ROWS, int COLS, const double *src, int r, int c, double diag)
{
    for (int a = 0; a < ROWS; ++a)
        for (int b = 0; b < COLS; ++b) dst[a * COLS + b] = (src && a < r && b < c) ? src[a * c + b] : (a == b ? diag : 0.0);
}
template <int D> static void load(double (&v)[D], const double *base, long i, int d) { for (int e = 0; e < D; ++e) v[e] = e < d ? base[i * d + e] : 0.0; }
template <int D> static void store(const double (&v)[D], double *base, long i, int d) { for (int e = 0; e < d; ++e) base[i * d + e] = v[e]; }

static double waves_sum(double w0, double w1, double w2, double w3) { return ((w0 + w1) + w2) + w3; }
// the butterfly over the 64 lanes of wave `wave` of lanes[G][A], element e: every lane ends with the wave's sum
template <int A> static double butterfly(std::vector<double> &lanes, int wave, int e)
{
    double t[64];
    for (int off = 32; off >= 1; off >>= 1) {
        for (int l = 0; l < 64; ++l) t[l] = lanes[(wave * 64 + l) * A + e] + lanes[(wave * 64 + (l ^ off)) * A + e];
        for (int l = 0; l < 64; ++l) lanes[(wave * 64 + l) * A + e] = t[l];
    }
    return lanes[(wave * 64) * A + e];
}
// the group's tree into its one slab: a wave alone stands as wave 0 of a workgroup whose other waves are absent (0.0)
template <int A> static void group_sum(std::vector<double> &lanes, int G, double *slab)
{
    for (int e = 0; e < A; ++e) {
        if (G == 64) slab[e] = waves_sum(butterfly<A>(lanes, 0, e), 0.0, 0.0, 0.0);
        else {
            double w[4];
            for (int wave = 0; wave < 4; ++wave) w[wave] = butterfly<A>(lanes, wave, e);
            slab[e] = waves_sum(w[0], w[1], w[2], w[3]);
        }
    }
}
// the total over that one slab, as the single path's finalize forms it
static double one_slab_total(const double *slab, int e)
{
    double runs[ENKF_GROUPS];
    for (int g = 0; g < ENKF_GROUPS; ++g) runs[g] = enkf_run_sum(slab, 1, e, g);
    return enkf_total(runs, 1, 0);
}
// one phase: member(i, acc of the lane that owns member i) in the route's order, then the tree and the totals
template <int A, class Member> static void phase(long N, int G, double *tot, Member member)
{
    std::vector<double> lanes((size_t)G * A, 0.0);
    const int per = G == 64 ? 1 : ENKF_PER_LANE;
    for (int l = 0; l < G; ++l)
        for (int j = 0; j < per; ++j) {
            const long i = (long)j * G + l;
            if (i < N) member(i, *reinterpret_cast<double (*)[A]>(&lanes[(size_t)l * A]));
        }
    double slab[A];
    group_sum<A>(lanes, G, slab);
    for (int e = 0; e < A; ++e) tot[e] = one_slab_total(slab, e);
}
static int route(long N) { return N <= 64 ? 64 : ENKF_BLOCK; }

// the tree and the totals alone, every lane of the group carrying v in its one accumulator (v = -0.0: the sum of -0.0 that the
// added zeros turn into +0.0)
extern "C" double hb_tree(double v, int G)
{
    std::vector<double> lanes((size_t)G, v);
    double slab[1];
    group_sum<1>(lanes, G, slab);
    return one_slab_total(slab, 0);
}

extern "C" int hb_predict(int n, long N, const double *F, const double *noise, const double *factor, double *sig, double *x, double *P)
{
    if (n > NX || N > ENKF_CHUNK) return -1;
    using Acc = EnkfPredictAcc<NX>;
    double Fp[NX * NX], fp[NX * NX], piv[NX], xs[NX];
    pad(Fp, NX, NX, F, n, n, 1.0);
    pad(fp, NX, NX, factor, n, n, 0.0);
    for (int j = 0; j < NX; ++j) xs[j] = j < n ? x[j] : 0.0;
    for (int i = 0; i < NX; ++i) {
        double p = xs[i];
        if (F) { p = Fp[i * NX] * xs[0]; for (int j = 1; j < NX; ++j) p = fma(Fp[i * NX + j], xs[j], p); }
        piv[i] = p;
    }
    double tot[Acc::SIZE];
    phase<Acc::SIZE>(N, route(N), tot, [&](long i, double (&acc)[Acc::SIZE]) {
        double s[NX], w[NX], e[NX];
        load<NX>(s, sig, i, n); load<NX>(w, noise, i, n);
        enkf_draw<NX>(w, factor ? fp : nullptr, e);
        enkf_predict_member<NX>(s, e, F ? Fp : nullptr, piv, acc);
        store<NX>(s, sig, i, n);
    });
    for (int i = 0; i < n; ++i) x[i] = enkf_mean(piv[i], tot[i], N);
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j) {
            const int hi = i > j ? i : j, lo = i > j ? j : i;
            P[i * n + j] = enkf_cov(tot[Acc::OFF_DD + enkf_tri(hi, lo)], tot[hi], tot[lo], N);
        }
    return 0;
}

extern "C" int hb_update(int n, int m, long N, const double *H, const double *sigmas_h, const double *R, const double *z,
                         const double *noise, const double *factor, double *sig, double *x, double *P, double *S, double *SI,
                         double *K)
{
    if (n > NX || m > NZ || N > ENKF_CHUNK) return -1;
    using Acc = EnkfStatsAcc<NX, NZ>;
    const int G = route(N);
    double Hp[NZ * NX], fp[NZ * NZ], px[NX], ph[NZ], zp[NZ];
    pad(Hp, NZ, NX, H, m, n, 0.0);
    pad(fp, NZ, NZ, factor, m, m, 0.0);
    for (int i = 0; i < NX; ++i) px[i] = i < n ? x[i] : 0.0;
    for (int c = 0; c < NZ; ++c) {
        zp[c] = c < m ? z[c] : 0.0;
        double p = 0.0;
        if (H) { p = Hp[c * NX] * px[0]; for (int j = 1; j < NX; ++j) p = fma(Hp[c * NX + j], px[j], p); }
        else if (c < m) p = sigmas_h[c];
        ph[c] = p;
    }
    auto h_of = [&](const double (&s)[NX], long i, double (&h)[NZ]) {
        if (H) enkf_matvec<NZ, NX>(Hp, s, h); else load<NZ>(h, sigmas_h, i, m);
    };
    // the one-wave route keeps member and h of its lane
    std::vector<double> keep_s((size_t)64 * NX), keep_h((size_t)64 * NZ);
    double tot[Acc::SIZE], pxz[NX * NZ], Kd[NX * NZ], Kp[NX * NZ];
    phase<Acc::SIZE>(N, G, tot, [&](long i, double (&acc)[Acc::SIZE]) {
        double s[NX], h[NZ];
        load<NX>(s, sig, i, n);
        h_of(s, i, h);
        enkf_stats_member<NX, NZ>(s, h, px, ph, acc);
        if (G == 64) {
            for (int e = 0; e < NX; ++e) keep_s[i * NX + e] = s[e];
            for (int e = 0; e < NZ; ++e) keep_h[i * NZ + e] = h[e];
        }
    });
    double Sd[ENKF_MAXZ * ENKF_MAXZ], SId[ENKF_MAXZ * ENKF_MAXZ];
    for (int r = 0; r < m; ++r)
        for (int c = 0; c < m; ++c) {
            const int hi = r > c ? r : c, lo = r > c ? c : r;
            Sd[r * m + c] = enkf_cov(tot[Acc::OFF_HH + enkf_tri(hi, lo)], tot[Acc::OFF_H + hi], tot[Acc::OFF_H + lo], N) + R[hi * m + lo];
        }
    for (int i = 0; i < n; ++i)
        for (int c = 0; c < m; ++c) pxz[i * m + c] = enkf_cov(tot[Acc::OFF_SH + i * NZ + c], tot[i], tot[Acc::OFF_H + c], N);
    double wL[ENKF_MAXZ * ENKF_MAXZ], wX[ENKF_MAXZ * ENKF_MAXZ], wd[ENKF_MAXZ], wdinv[ENKF_MAXZ];
    const int st = enkf_spd_inverse_in(Sd, m, SId, wL, wd, wdinv, wX);
    for (int t = 0; t < m * m; ++t) { S[t] = Sd[t]; SI[t] = SId[t]; }
    for (int t = 0; t < NX * NZ; ++t) Kp[t] = 0.0;
    for (int t = 0; t < n * m; ++t) {
        const double v = enkf_gain_entry(pxz, SId, m, t / m, t % m);
        Kd[t] = v;
        Kp[(t / m) * NZ + t % m] = v;
        K[t] = v;
    }
    for (int t = 0; t < n * n; ++t) P[t] = P[t] - enkf_ksk_entry(Kd, Sd, m, t / n, t % n);
    double tot2[NX];
    phase<NX>(N, G, tot2, [&](long i, double (&acc)[NX]) {
        double s[NX], h[NZ], w[NZ], e[NZ];
        if (G == 64) {
            for (int k = 0; k < NX; ++k) s[k] = keep_s[i * NX + k];
            for (int k = 0; k < NZ; ++k) h[k] = keep_h[i * NZ + k];
        } else {
            load<NX>(s, sig, i, n);
            h_of(s, i, h);
        }
        load<NZ>(w, noise, i, m);
        enkf_draw<NZ>(w, factor ? fp : nullptr, e);
        enkf_apply_member<NX, NZ>(s, h, e, zp, Kp, px, acc);
        store<NX>(s, sig, i, n);
    });
    for (int i = 0; i < n; ++i) x[i] = enkf_mean(px[i], tot2[i], N);
    return st;
}
'''
_libs = {}


def libs(tmp_path_factory):
    """{None: the padded (16, 8) build, (n, m): the exact build}: compiled once per session, side by side"""
    if _libs:
        return _libs
    d = tmp_path_factory.mktemp("hb_enkf")
    src = d / "hb_enkf.cpp"
    src.write_text(HB_SRC)
    jobs = []
    for dims in [None] + EXACT:
        so = d / ("libhb_enkf%s.so" % ("" if dims is None else "_%d_%d" % dims))
        defs = [] if dims is None else ["-DHC_NX=%d" % dims[0], "-DHC_NZ=%d" % dims[1]]
        jobs.append((dims, so, subprocess.Popen(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=on", "-w", *defs,
                                                 "-I", os.path.join(ROOT, "filterpy_amd", "csrc"), str(src), "-o", str(so)])))
    for dims, so, p in jobs:
        assert p.wait() == 0, dims
    for dims, so, p in jobs:
        lib = ctypes.CDLL(str(so))
        lib.hb_tree.restype = ctypes.c_double
        lib.hb_tree.argtypes = [ctypes.c_double, ctypes.c_int]
        _libs[dims] = lib
    return _libs


def hb_predict(lib, sig, x, e, F=None, factor=None):
    N, n = sig.shape
    sig, x, P = _cc(sig).copy(), _cc(x).copy(), np.zeros((n, n))
    F, e, factor = _cc(F), _cc(e), _cc(factor)
    assert lib.hb_predict(n, ctypes.c_long(N), _p(F), _p(e), _p(factor), _p(sig), _p(x), _p(P)) == 0
    return sig, x, P


def hb_update(lib, sig, x, P, z, R, e, H=None, sigmas_h=None, factor=None):
    N, n = sig.shape
    m = len(z)
    sig, x, P = _cc(sig).copy(), _cc(x).copy(), _cc(P).copy()
    S, SI, K = np.zeros((m, m)), np.zeros((m, m)), np.zeros((n, m))
    H, sigmas_h, R, z, e, factor = _cc(H), _cc(sigmas_h), _cc(R), _cc(z), _cc(e), _cc(factor)
    st = lib.hb_update(n, m, ctypes.c_long(N), _p(H), _p(sigmas_h), _p(R), _p(z), _p(e), _p(factor), _p(sig), _p(x), _p(P), _p(S),
                       _p(SI), _p(K))
    return sig, x, P, K, S, SI, st
