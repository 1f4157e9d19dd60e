// fls_kernels.hip -- the fixed-lag smoother (filterpy/kalman/fixed_lag_smoother.py:133-311) for a bank of tracks (gfx950).
//
// One track per lane, the whole time loop inside the kernel, the model shared by every track and staged once in LDS.  The
// step is fk_fls.hpp's: predict, the Joseph-form update of kf_update, w = H' S^-1 y, G = F - K H, then the lag loop
// row(k-i) += P u_i, u_{i+1} = G' u_i (the reference's PS_i H'SI y reassociated -- see fk_fls.hpp).
//
// Two kernels:
//   fls_fast_kernel<NX, NZ, LMAX>   exact (dim_x, dim_z), lags with max(lag, 1) <= LMAX: x, P and the pending rows in VGPRs.
//       The pending rows are a SHIFT REGISTER over the compile-time capacity LMAX (every index a constant: no scratch; a
//       runtime-indexed array would live in scratch memory).  The uniform runtime lag cuts the lag loop short.  At step k
//       row k - max(lag, 1) + 1 is final and leaves for HBM -- every output row is written once: the rows still pending at
//       the end of the launch go out after the time loop.  Compiled once per -DFK_NX/-DFK_NZ/-DFK_LMAX (fk_dims_fls.def).
//   fls_general_kernel              everything else (dim_x <= 16, dim_z <= 8, any lag): ONE padded (16, 8) instantiation
//       with rolled loops (arrays in scratch), the pending rows read-modify-written in place in `xs`.  An escape path in the
//       style of kf_given_inv.hip, not a throughput path: its speed is documented, not tuned.
//       Compiled with -DFK_FLS_GENERAL=1.
// Which one runs depends on (n, m, lag, layout) only (fls_dispatch.cpp): chained calls are bit-identical to one call.
#if defined(FK_FLS_GENERAL) && FK_FLS_GENERAL
#define FK_ROLLED 1
#endif
#include "fk_bank.hpp"
#include "fk_fls.hpp"

namespace fk {

// the model is F | Q | H | R as given, B u of step t (x = F x + B u, fixed_lag_smoother.py:270-272) is bank_control (fk_bank.hpp)
template <int NX, int NZ>
__device__ __forceinline__ void fls_fill_model(double *s_model, const FlsArgs &a)
{
    bank_fill_model<NX, NZ>(s_model, a.F, a.Q, a.H, a.R, a.n, a.m);
}

#if !(defined(FK_FLS_GENERAL) && FK_FLS_GENERAL)

template <int NX, int NZ, int LMAX, int LAYOUT>
__global__ void __launch_bounds__(BLOCK)
fls_fast_kernel(const FlsArgs a)
{
    using SM = LdsModel<NX, NZ>;
    __shared__ double s_model[SM::SIZE];
    fls_fill_model<NX, NZ>(s_model, a);          // (the only barrier: lanes past N may leave after it)
    const long N = a.N;
    const long blk0 = (long)blockIdx.x * BLOCK;
    if (blk0 + threadIdx.x >= N) return;
    const Lane ln{blk0, threadIdx.x, N};
    const SM sm{s_model};
    const int lag = a.lag, Lf = lag > 1 ? lag : 1;
    const long W = a.W, k0 = a.k0, T = a.T;
    const long row0 = k0 - W;                    // the global step of xs's first row

    double x[NX], P[NX * NX];
    load_rec<NX, 1, LAYOUT, true>(x, a.x, ln, NX, 1, 0.0);
    load_rec<NX, NX, LAYOUT, true>(P, a.P, ln, NX, NX, 1.0);
    // pend[i]: row k-1-i before step k (the pending window of the previous call: rows k0-1 .. k0-W)
    double pend[LMAX * NX];
    FK_UNROLL for (int i = 0; i < LMAX; ++i) {
        double r[NX];
        if (i < W) load_rec<NX, 1, LAYOUT, true>(r, a.xs + (W - 1 - i) * N * NX, ln, NX, 1, 0.0);
        else FK_UNROLL for (int j = 0; j < NX; ++j) r[j] = 0.0;
        FK_UNROLL for (int j = 0; j < NX; ++j) pend[i * NX + j] = r[j];
    }
    int st = 0;
    double y[NZ], S[NZ * NZ];
    for (long t = 0; t < T; ++t) {
        const long k = k0 + t;
        double z[NZ], bu[NX];
        load_rec<NZ, 1, LAYOUT, true>(z, a.z + t * N * NZ, ln, NZ, 1, 0.0);
        bank_control<NX, LAYOUT>(a, ln, a.u, t, bu);
        st |= fls_step<NX, NZ, LMAX>(x, P, z, sm, bu, a.nu > 0, a.rj_diag != 0, k, lag, pend, y, S);
        store_rec<NX, 1, LAYOUT, true>(x, a.xhat + t * N * NX, ln, NX, 1);
        const long j = k - Lf + 1;               // final now
        if (j >= 0) {
            double *dst = a.xs + (j - row0) * N * NX;
            FK_UNROLL for (int i = 0; i < LMAX; ++i) {
                if (i == Lf - 1) {               // uniform: one branch taken, no register indexing
                    double r[NX];
                    FK_UNROLL for (int e = 0; e < NX; ++e) r[e] = pend[i * NX + e];
                    store_rec<NX, 1, LAYOUT, true>(r, dst, ln, NX, 1);
                }
            }
        }
    }
    // the window that stays pending: rows k0+T-1-i, i < min(Lf-1, k0+T)
    const long Wout = (long)(Lf - 1) < k0 + T ? (long)(Lf - 1) : k0 + T;
    FK_UNROLL for (int i = 0; i < LMAX; ++i) {
        if (i < Wout) {
            double r[NX];
            FK_UNROLL for (int e = 0; e < NX; ++e) r[e] = pend[i * NX + e];
            store_rec<NX, 1, LAYOUT, true>(r, a.xs + (W + T - 1 - i) * N * NX, ln, NX, 1);
        }
    }
    store_rec<NX, 1, LAYOUT, true>(x, a.x, ln, NX, 1);
    store_rec<NX, NX, LAYOUT, true>(P, a.P, ln, NX, NX);
    if (a.y) store_rec<NZ, 1, LAYOUT, true>(y, a.y, ln, NZ, 1);
    if (a.S) store_rec<NZ, NZ, LAYOUT, true>(S, a.S, ln, NZ, NZ);
    if (a.status) {
        if (!all_finite<NX>(x) || !all_finite<NX * NX>(P)) st |= ST_NONFINITE;
        a.status[ln.blk0 + ln.tid] = st;
    }
}

#define FK_CAT_(a, b, c, d) a##b##_##c##_##d
#define FK_CAT(a, b, c, d) FK_CAT_(a, b, c, d)

int FK_CAT(launch_fls_fast_, FK_NX, FK_NZ, FK_LMAX)(const FlsArgs &a, int layout, hipStream_t stream)
{
    return bank_launch(fls_fast_kernel<FK_NX, FK_NZ, FK_LMAX, LAYOUT_SOA>, fls_fast_kernel<FK_NX, FK_NZ, FK_LMAX, LAYOUT_AOS>,
                       "fls_fast_kernel", a, layout, stream);
}

#else  // FK_FLS_GENERAL

constexpr int GX = 16, GZ = 8;

// element e of the lane's record of row `row` in xs ([rows][N][n] AOS / [rows][n][N] SOA): plain loads and stores, so that a
// row written at one step and read back at the next needs no thought about ordering
template <int LAYOUT>
__device__ __forceinline__ double *fls_row(const FlsArgs &a, long row, long track)
{
    double *blk = a.xs + row * a.N * a.n;
    return LAYOUT == LAYOUT_AOS ? blk + track * a.n : blk + track;
}

template <int LAYOUT>
__global__ void __launch_bounds__(BLOCK)
fls_general_kernel(const FlsArgs a)
{
    using SM = LdsModel<GX, GZ>;
    __shared__ double s_model[SM::SIZE];
    fls_fill_model<GX, GZ>(s_model, a);
    const long N = a.N;
    const long blk0 = (long)blockIdx.x * BLOCK;
    if (blk0 + threadIdx.x >= N) return;
    const Lane ln{blk0, threadIdx.x, N};
    const long track = blk0 + threadIdx.x;
    const SM sm{s_model};
    const int n = a.n, m = a.m, lag = a.lag;
    const long es = LAYOUT == LAYOUT_AOS ? 1 : N;          // element stride of a row record
    const long row0 = a.k0 - a.W;

    double x[GX], P[GX * GX];
    load_rec<GX, 1, LAYOUT, false>(x, a.x, ln, n, 1, 0.0);
    load_rec<GX, GX, LAYOUT, false>(P, a.P, ln, n, n, 1.0);
    int st = 0;
    double y[GZ], S[GZ * GZ];
    for (long t = 0; t < a.T; ++t) {
        const long k = a.k0 + t;
        double z[GZ], bu[GX], xpre[GX], w[GX], G[GX * GX];
        load_rec<GZ, 1, LAYOUT, false>(z, a.z + t * N * m, ln, m, 1, 0.0);
        bank_control<GX, LAYOUT>(a, ln, a.u, t, bu);
        st |= fls_filter_step<GX, GZ>(x, P, z, sm, bu, a.nu > 0, a.rj_diag != 0, xpre, w, G, y, S);
        store_rec<GX, 1, LAYOUT, false>(x, a.xhat + t * N * n, ln, n, 1);
        const bool smooth = k >= (long)lag;
        double *rk = fls_row<LAYOUT>(a, k - row0, track);
        FK_UNROLL for (int e = 0; e < GX; ++e)
            if (e < n) rk[e * es] = smooth ? xpre[e] : x[e];
        if (!smooth) continue;
        for (int i = 0; i < lag; ++i) {
            double r[GX];
            double *ri = fls_row<LAYOUT>(a, k - i - row0, track);
            FK_UNROLL for (int e = 0; e < GX; ++e) r[e] = e < n ? ri[e * es] : 0.0;
            fls_lag_step<GX>(P, G, w, r, i + 1 < lag);
            FK_UNROLL for (int e = 0; e < GX; ++e)
                if (e < n) ri[e * es] = r[e];
        }
    }
    store_rec<GX, 1, LAYOUT, false>(x, a.x, ln, n, 1);
    store_rec<GX, GX, LAYOUT, false>(P, a.P, ln, n, n);
    if (a.y) store_rec<GZ, 1, LAYOUT, false>(y, a.y, ln, m, 1);
    if (a.S) store_rec<GZ, GZ, LAYOUT, false>(S, a.S, ln, m, m);
    if (a.status) {
        if (!all_finite<GX>(x) || !all_finite<GX * GX>(P)) st |= ST_NONFINITE;
        a.status[ln.blk0 + ln.tid] = st;
    }
}

int launch_fls_general(const FlsArgs &a, int layout, hipStream_t stream)
{
    return bank_launch(fls_general_kernel<LAYOUT_SOA>, fls_general_kernel<LAYOUT_AOS>, "fls_general_kernel", a, layout, stream);
}

#endif

}  // namespace fk
