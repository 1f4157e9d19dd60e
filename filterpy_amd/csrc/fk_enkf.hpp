// fk_enkf.hpp -- the arithmetic of the ensemble Kalman filter (filterpy/kalman/ensemble_kalman_filter.py:218-290) as the
// kernels of enkf_kernels.hip run it: what one lane does with one member, how the partial sums of the workgroups are added up,
// and the small dense algebra of the finalize.  __host__ __device__: tests/test_host_enkf.py compiles this text with g++ and
// drives it chunk by chunk in the kernels' order.
//
// The scheme.  The ensemble is cut into chunks of ENKF_CHUNK members, one workgroup each; lane l of a chunk takes members
// l, l + 256, ... in that order.  A pass kernel leaves one SLAB of ENKF_SLAB partial sums per chunk in the workspace; the
// finalize (one workgroup) adds the slabs in a fixed order -- ENKF_GROUPS contiguous runs of slabs, each in index order, then
// the runs in index order -- and does the dense algebra once.  Nothing depends on which workgroup finishes first.
//
// Centring.  Every second moment is a ONE-pass sum of products of data shifted by a pivot that is known before the pass,
// corrected by the shifted mean in the finalize:
//     sum (a - mean a)(b - mean b)' = sum da db' - (sum da)(sum db)' / N,     da = a - pa, db = b - pb.
// The pivots are the incoming x (update), F x or x (predict) and H x or member 0's h: as close to the mean as the spread of
// the ensemble -- member 0 as close as ONE member is -- so the correction term is of the size of the result and costs no
// digits (the uncentred sum s s' - N x x' loses |x|^2 / var of them).  A pivot d spreads from the mean costs eps d^2: with
// member 0 at d = 30, S, SI, K and P are 100-210 x less accurate than the two-pass form and still 0.05 of the precision bar
// (tests/test_host_enkf_hp.py, tests/test_gpu_enkf_precision.py: the pivot contract).  The update's centre of the members IS self.x, as in the reference (:256-257), so there the
// member pivot is not a device but the definition.
//
// Accumulators per lane (NX, NZ the register shapes):
//   predict  [ sum d (NX) | sum d d' lower triangle, row-major (NX (NX + 1) / 2) ]
//   stats    [ sum ds (NX) | sum dh (NZ) | sum dh dh' lower triangle (NZ (NZ + 1) / 2) | sum ds dh' (NX x NZ) ]
//   apply    [ sum (s_new - x) (NX) ]
#pragma once

#include <stdint.h>

#include "fk_math.hpp"
#include "fk_ukf.hpp"

namespace fk {

constexpr int ENKF_BLOCK = 256;                            // lanes of a pass workgroup
constexpr int ENKF_PER_LANE = 8;                           // members a lane takes
constexpr int ENKF_CHUNK = ENKF_BLOCK * ENKF_PER_LANE;     // members of a chunk (= of a slab)
constexpr int ENKF_GROUPS = 16;                            // runs of slabs the finalize adds side by side
constexpr int ENKF_MAXX = 16, ENKF_MAXZ = 8;
constexpr int ENKF_SLAB = ENKF_MAXX + ENKF_MAXZ + ENKF_MAXZ * (ENKF_MAXZ + 1) / 2 + ENKF_MAXX * ENKF_MAXZ;   // 188 doubles
// the workspace, in doubles: the pivots of the pass in flight, the gain for the apply pass, then the slabs
constexpr int ENKF_WS_PIVX = 0, ENKF_WS_PIVH = ENKF_MAXX, ENKF_WS_K = ENKF_MAXX + ENKF_MAXZ;
constexpr int ENKF_WS_SLABS = ENKF_WS_K + ENKF_MAXX * ENKF_MAXZ;

static_assert(ENKF_MAXX + ENKF_MAXX * (ENKF_MAXX + 1) / 2 <= ENKF_SLAB, "the predict sums fit a slab");

FK_HD long enkf_slabs(long N) { return N > 0 ? (N + ENKF_CHUNK - 1) / ENKF_CHUNK : 1; }
FK_HD long enkf_workspace_doubles(long N) { return ENKF_WS_SLABS + enkf_slabs(N) * ENKF_SLAB; }

template <int NX> struct EnkfPredictAcc { static constexpr int OFF_DD = NX, SIZE = NX + NX * (NX + 1) / 2; };
template <int NX, int NZ>
struct EnkfStatsAcc {
    static constexpr int OFF_H = NX, OFF_HH = NX + NZ, OFF_SH = OFF_HH + NZ * (NZ + 1) / 2, SIZE = OFF_SH + NX * NZ;
};
FK_HD int enkf_tri(int i, int j) { return i * (i + 1) / 2 + j; }          // i >= j

// ---- one member ------------------------------------------------------------------------------------------------------------

// r = M v for a ROWS x COLS matrix M (row-major, padded); the first product, then fused multiply-adds in column order
template <int ROWS, int COLS>
FK_HD void enkf_matvec(const double *M, const double (&v)[COLS], double (&r)[ROWS])
{
    FK_UNROLL for (int i = 0; i < ROWS; ++i) {
        double t = M[i * COLS] * v[0];
        FK_UNROLL for (int j = 1; j < COLS; ++j) t = fma(M[i * COLS + j], v[j], t);
        r[i] = t;
    }
}

// The draw of one member: e = w as it is (fac NULL), or e = A' w, e[j] = sum_k A[k][j] w[k], with the D x D factor A of the
// covariance (numpy.random.multivariate_normal's sqrt(s)[:, None] * v of the SVD; padded with zeros).
template <int D>
FK_HD void enkf_draw(const double (&w)[D], const double *fac, double (&e)[D])
{
    if (fac == nullptr) {
        FK_UNROLL for (int j = 0; j < D; ++j) e[j] = w[j];
        return;
    }
    FK_UNROLL for (int j = 0; j < D; ++j) {
        double t = fac[j] * w[0];
        FK_UNROLL for (int k = 1; k < D; ++k) t = fma(fac[k * D + j], w[k], t);
        e[j] = t;
    }
}

// predict (:278-286): s <- F s (F NULL: s) + e; the sums take d = s - piv
template <int NX>
FK_HD void enkf_predict_member(double (&s)[NX], const double (&e)[NX], const double *F, const double *piv,
                               double (&acc)[EnkfPredictAcc<NX>::SIZE])
{
    using A = EnkfPredictAcc<NX>;
    if (F != nullptr) {
        double fs[NX];
        enkf_matvec<NX, NX>(F, s, fs);
        FK_UNROLL for (int i = 0; i < NX; ++i) s[i] = fs[i];
    }
    double d[NX];
    FK_UNROLL for (int i = 0; i < NX; ++i) {
        s[i] += e[i];
        d[i] = s[i] - piv[i];
        acc[i] += d[i];
    }
    FK_UNROLL for (int i = 0; i < NX; ++i)
        FK_UNROLL for (int j = 0; j <= i; ++j) acc[A::OFF_DD + enkf_tri(i, j)] = fma(d[i], d[j], acc[A::OFF_DD + enkf_tri(i, j)]);
}

// update, first pass (:250-257): the sums of ds = s - x and dh = h - ph
template <int NX, int NZ>
FK_HD void enkf_stats_member(const double (&s)[NX], const double (&h)[NZ], const double *px, const double *ph,
                             double (&acc)[EnkfStatsAcc<NX, NZ>::SIZE])
{
    using A = EnkfStatsAcc<NX, NZ>;
    double ds[NX], dh[NZ];
    FK_UNROLL for (int i = 0; i < NX; ++i) {
        ds[i] = s[i] - px[i];
        acc[i] += ds[i];
    }
    FK_UNROLL for (int c = 0; c < NZ; ++c) {
        dh[c] = h[c] - ph[c];
        acc[A::OFF_H + c] += dh[c];
    }
    FK_UNROLL for (int a = 0; a < NZ; ++a)
        FK_UNROLL for (int b = 0; b <= a; ++b) acc[A::OFF_HH + enkf_tri(a, b)] = fma(dh[a], dh[b], acc[A::OFF_HH + enkf_tri(a, b)]);
    FK_UNROLL for (int i = 0; i < NX; ++i)
        FK_UNROLL for (int c = 0; c < NZ; ++c) acc[A::OFF_SH + i * NZ + c] = fma(ds[i], dh[c], acc[A::OFF_SH + i * NZ + c]);
}

// update, second pass (:263-265): s += K ((z + e) - h); the sum takes s - px (px: the centre the update started from)
template <int NX, int NZ>
FK_HD void enkf_apply_member(double (&s)[NX], const double (&h)[NZ], const double (&e)[NZ], const double *z, const double *K,
                             const double *px, double (&acc)[NX])
{
    double v[NZ], kv[NX];
    FK_UNROLL for (int c = 0; c < NZ; ++c) v[c] = (z[c] + e[c]) - h[c];
    enkf_matvec<NX, NZ>(K, v, kv);
    FK_UNROLL for (int i = 0; i < NX; ++i) {
        s[i] += kv[i];
        acc[i] += s[i] - px[i];
    }
}

// ---- the slabs -------------------------------------------------------------------------------------------------------------

// element e of run g: slabs [g per, (g + 1) per) in index order, per = ceil(nslabs / ENKF_GROUPS)
FK_HD double enkf_run_sum(const double *slabs, long nslabs, int e, int g)
{
    const long per = (nslabs + ENKF_GROUPS - 1) / ENKF_GROUPS;
    const long k0 = g * per, k1 = (k0 + per < nslabs) ? k0 + per : nslabs;
    double t = 0.0;
    for (long k = k0; k < k1; ++k) t += slabs[k * ENKF_SLAB + e];
    return t;
}

// ... and the runs in index order (runs: [ENKF_GROUPS][stride])
FK_HD double enkf_total(const double *runs, int stride, int e)
{
    double t = runs[e];
    for (int g = 1; g < ENKF_GROUPS; ++g) t += runs[g * stride + e];
    return t;
}

// ---- the finalize, entry by entry (tot: the totals of the pass, in the accumulators' order) --------------------------------

// the mean of a shifted sum put back on its pivot
FK_HD double enkf_mean(double piv, double sum, long N) { return piv + sum / (double)N; }

// sum (a - mean a)(b - mean b) / (N - 1) from sum da db, sum da and sum db
FK_HD double enkf_cov(double sab, double sa, double sb, long N)
{
    return fma(-sa, sb / (double)N, sab) / (double)(N - 1);
}

// SI = S^-1 for the m x m S (row-major, stride m; its lower triangle is read) by the refined-pivot L D L' of fk_ukf.hpp,
// padded to 8 x 8 with the identity.  Returns ST_NOT_PD when a pivot is at or below m eps max|diag S| (or is not a number).
// L, d, dinv, X: the work arrays, wherever the caller keeps them (the bank kernels of enkf_bank.hip: in LDS, so that the one
// lane that runs this holds none of the 144 doubles in scratch memory).
FK_HD int enkf_spd_inverse_in(const double *S, int m, double *SI, double (&L)[ENKF_MAXZ * ENKF_MAXZ], double (&d)[ENKF_MAXZ],
                              double (&dinv)[ENKF_MAXZ], double (&X)[ENKF_MAXZ * ENKF_MAXZ])
{
    constexpr int M = ENKF_MAXZ;
    double dmax = 0.0;
    for (int a = 0; a < M; ++a)
        for (int b = 0; b < M; ++b) {
            const int hi = a > b ? a : b, lo = a > b ? b : a;
            L[a * M + b] = (hi < m) ? S[hi * m + lo] : (a == b ? 1.0 : 0.0);
            X[a * M + b] = (a == b) ? 1.0 : 0.0;
        }
    for (int a = 0; a < m; ++a) dmax = fmax(dmax, fabs(S[a * m + a]));
    ldlt2_rs<M>(L, d, dinv);
    const double cut = (double)m * 2.220446049250313e-16 * dmax;
    int st = 0;
    for (int a = 0; a < m; ++a)
        if (!(d[a] > cut)) st = ST_NOT_PD;
    solve_rows_ldlt<M, M>(L, dinv, X);
    // S^-1 is symmetric: the lower triangle of the solve, mirrored
    for (int a = 0; a < m; ++a)
        for (int b = 0; b <= a; ++b) SI[a * m + b] = SI[b * m + a] = X[a * M + b];
    return st;
}

FK_HD int enkf_spd_inverse(const double *S, int m, double *SI)
{
    constexpr int M = ENKF_MAXZ;
    double L[M * M], d[M], dinv[M], X[M * M];
    return enkf_spd_inverse_in(S, m, SI, L, d, dinv, X);
}

// K[i][c] = sum_a Pxz[i][a] SI[a][c]   (dot(P_xz, SI), :261)
FK_HD double enkf_gain_entry(const double *Pxz, const double *SI, int m, int i, int c)
{
    double t = Pxz[i * m] * SI[c];
    for (int a = 1; a < m; ++a) t = fma(Pxz[i * m + a], SI[a * m + c], t);
    return t;
}

// (K S K')[i][j] as dot(dot(K, S), K.T) forms it (:268)
FK_HD double enkf_ksk_entry(const double *K, const double *S, int m, int i, int j)
{
    double t = 0.0;
    for (int b = 0; b < m; ++b) {
        double ks = K[i * m] * S[b];
        for (int a = 1; a < m; ++a) ks = fma(K[i * m + a], S[a * m + b], ks);
        t = (b == 0) ? ks * K[j * m] : fma(ks, K[j * m + b], t);
    }
    return t;
}

enum : int { ENKF_PREDICT = 0, ENKF_STATS = 1, ENKF_APPLY = 2, ENKF_FIN_PREDICT = 3, ENKF_FIN_UPDATE = 4, ENKF_FIN_APPLY = 5 };

// What every kernel of the family takes.  ax, az: the shapes the pass kernel's accumulators were laid out for ((n, m) for an
// exact kernel, (16, 8) for the general one): the finalize reads the slabs by them.
struct EnkfArgs {
    const double *F, *H, *sigmas_h, *R, *z, *noise, *factor;
    double *sigmas, *x, *P, *S, *SI, *K, *ws;
    int32_t *status;
    long N;
    int n, m, phase, ax, az;
};

// What the bank kernels (enkf_bank.hip) take: B ensembles of N <= ENKF_CHUNK members each, one contiguous block per ensemble
// ([B][d][N] or [B][N][d]); x [B][n], P [B][n*n], K [B][n*m], S, SI [B][m*m], z [B][m], mask, status [B]; F, H, R and the
// factor once (per_track 0) or once per ensemble.
struct EnkfBankArgs {
    const double *F, *H, *sigmas_h, *R, *z, *noise, *factor;
    const uint8_t *mask;
    double *sigmas, *x, *P, *S, *SI, *K;
    int32_t *status;
    long B, N;
    int n, m, per_track, update;
};

}  // namespace fk
