// ckf_kernels.hip -- the cubature Kalman filter (filterpy/kalman/CubatureKalmanFilter.py:32-98, 292-390) for a bank of tracks
// (gfx950).  One track per lane throughout.
//
// The matrix model (fx = F, hx = H shared by every track; fk_ckf.hpp): the whole time loop inside the kernel, the model in
// LDS.  The state is x, P and the points predict left, held as the centre c = F x and the n half-differences E[k] = F U[k]
// (record [n + n*n]: c, then E row by row): an update without a predict and the first update of a chained call see them.
//   ckf_fast_kernel<NX, NZ>    exact (dim_x, dim_z): x, P, c and E in VGPRs, every loop unrolled; in NumPy order the four
//       histories leave through an LDS transpose (wave_store_aos), as info_kernels.hip's do, where its tiles fit.  Compiled once per
//       -DFK_NX/-DFK_NZ (fk_dims_ckf.def).
//   ckf_general_kernel         everything else (dim_x <= 16, dim_z <= 8): ONE padded (16, 8) instantiation with rolled loops
//       (arrays in scratch).  A correctness path.  Compiled with -DFK_CKF_GENERAL=1.
// Which one runs depends on (n, m, layout) only (ckf_dispatch.cpp): chained calls are bit-identical to one call.
//
// The building blocks for arbitrary fx / hx (compiled with the general kernel, padded (16, 8), rolled):
//   ckf_points_kernel      <- spherical_radial_sigmas (:32-61)
//   ckf_transform_kernel   <- ckf_transform (:64-98)
//   ckf_update_kernel      <- update (:357-379): zp, S, SI, Pxz, K, y, x and P in ONE launch -- the reference has no hook
//                             between them (fk_ut_transform_f64 / fk_ut_cross_variance_f64 / fk_ukf_correct_f64 are three)
#if defined(FK_CKF_GENERAL) && FK_CKF_GENERAL
#define FK_ROLLED 1
#endif
#include "fk_bank.hpp"
#include "fk_ckf.hpp"

namespace fk {

// the points record of the lane's track: c [n], then E [n][n]
template <int NX, int LAYOUT, bool EXACT>
__device__ __forceinline__ void ckf_load_pts(double (&c)[NX], double (&E)[NX * NX], const double *pts, const Lane &ln, int n)
{
    const RecView<LAYOUT> v(pts, ln, EXACT ? NX + NX * NX : n + n * n);
    FK_UNROLL for (int i = 0; i < NX; ++i) c[i] = (EXACT || i < n) ? v.load(i) : 0.0;
    FK_UNROLL for (int k = 0; k < NX; ++k)
        FK_UNROLL for (int i = 0; i < NX; ++i)
            E[k * NX + i] = (EXACT || (k < n && i < n)) ? v.load(EXACT ? NX + k * NX + i : n + k * n + i) : (k == i ? 1.0 : 0.0);
}

template <int NX, int LAYOUT, bool EXACT>
__device__ __forceinline__ void ckf_store_pts(const double (&c)[NX], const double (&E)[NX * NX], double *pts, const Lane &ln,
                                              int n)
{
    const RecView<LAYOUT> v(pts, ln, EXACT ? NX + NX * NX : n + n * n);
    FK_UNROLL for (int i = 0; i < NX; ++i)
        if (EXACT || i < n) v.store(i, c[i]);
    FK_UNROLL for (int k = 0; k < NX; ++k)
        FK_UNROLL for (int i = 0; i < NX; ++i)
            if (EXACT || (k < n && i < n)) v.store(EXACT ? NX + k * NX + i : n + k * n + i, E[k * NX + i]);
}

// The whole launch for one lane: NX, NZ the register shapes (the real n, m when EXACT).  last_row: the block's last real
// track; lanes past it (WAVE only) run a copy of that track.
template <int NX, int NZ, int LAYOUT, bool EXACT, bool WAVE>
__device__ __forceinline__ void ckf_lane(const CkfArgs &a, const double *s_model, double *tile, unsigned last_row)
{
    const long N = a.N;
    const long blk0 = (long)blockIdx.x * BLOCK;
    const unsigned tid = threadIdx.x < last_row ? threadIdx.x : last_row;
    const Lane ln{blk0, tid, N};
    const long track = blk0 + tid;
    const LdsModel<NX, NZ> sm{s_model};
    const int n = EXACT ? NX : a.n, m = EXACT ? NZ : a.m;

    double x[NX], P[NX * NX], c[NX], E[NX * NX];
    load_rec<NX, 1, LAYOUT, EXACT>(x, a.x, ln, n, 1, 0.0);
    load_rec<NX, NX, LAYOUT, EXACT>(P, a.P, ln, n, n, 1.0);
    // P is symmetric: cholesky reads the upper triangle, and carrying the lower one as a copy of it lets the compiler keep
    // one register per pair across the time loop
    FK_UNROLL for (int r = 0; r < NX; ++r)
        FK_UNROLL for (int q = r + 1; q < NX; ++q) P[q * NX + r] = P[r * NX + q];
    ckf_load_pts<NX, LAYOUT, EXACT>(c, E, a.pts, ln, n);
    int st = 0;
    const bool do_predict = a.phase != CKF_UPDATE, do_update = a.phase != CKF_PREDICT;
    for (long t = 0; t < a.T; ++t) {
        if (do_predict) {
            st |= ckf_linear_predict<NX>(x, P, c, E, sm);
            if (a.means_p) bank_put<NX, 1, LAYOUT, EXACT, WAVE>(x, a.means_p, t, ln, n, 1, tile, last_row);
            if (a.covs_p) bank_put<NX, NX, LAYOUT, EXACT, WAVE>(P, a.covs_p, t, ln, n, n, tile, last_row);
        }
        if (do_update) {
            const bool upd = a.mask == nullptr || a.mask[t * N + track] != 0;
            if (upd) {
                double z[NZ], y[NZ], K[NX * NZ], S[NZ * NZ], Lf[NZ * NZ], dinv[NZ];
                load_rec<NZ, 1, LAYOUT, EXACT>(z, a.z + t * N * m, ln, m, 1, 0.0);
                st |= ckf_linear_update<NX, NZ>(x, P, c, E, z, sm, y, K, S, Lf, dinv);
                // the by-products of the last update (single steps; written by every step that updates)
                if (a.y) store_rec<NZ, 1, LAYOUT, EXACT>(y, a.y, ln, m, 1);
                if (a.K) store_rec<NX, NZ, LAYOUT, EXACT>(K, a.K, ln, n, m);
                if (a.S) store_rec<NZ, NZ, LAYOUT, EXACT>(S, a.S, ln, m, m);
                if (a.SI) {
                    double SI[NZ * NZ];
                    inv_from_ldlt<NZ>(Lf, dinv, SI);
                    store_rec<NZ, NZ, LAYOUT, EXACT>(SI, a.SI, ln, m, m);
                }
            }
            if (a.means) bank_put<NX, 1, LAYOUT, EXACT, WAVE>(x, a.means, t, ln, n, 1, tile, last_row);
            if (a.covs) bank_put<NX, NX, LAYOUT, EXACT, WAVE>(P, a.covs, t, ln, n, n, tile, last_row);
        }
    }
    store_rec<NX, 1, LAYOUT, EXACT>(x, a.x, ln, n, 1);
    store_rec<NX, NX, LAYOUT, EXACT>(P, a.P, ln, n, n);
    if (do_predict) ckf_store_pts<NX, LAYOUT, EXACT>(c, E, a.pts, ln, n);
    if (a.status) {
        if (!all_finite<NX>(x) || !all_finite<NX * NX>(P)) st |= ST_NONFINITE;
        a.status[track] = st;
    }
}

#if !(defined(FK_CKF_GENERAL) && FK_CKF_GENERAL)

template <int NX, int NZ, int LAYOUT>
__global__ void __launch_bounds__(BLOCK)
ckf_fast_kernel(const CkfArgs a)
{
    constexpr int TILE = 64 * ((NX * NX) | 1);    // wave_store_aos's tile: 64 records of the longest history, odd row stride
    // (at dim_x 9 four such tiles are 162 KB, more than the 160 KB of LDS: NumPy order then stores lane by lane)
    constexpr bool WAVE = LAYOUT == LAYOUT_AOS && ((BLOCK / 64) * TILE + LdsModel<NX, NZ>::SIZE) * 8 <= 160 * 1024;
    __shared__ double s_model[LdsModel<NX, NZ>::SIZE];
    __shared__ double s_tile[WAVE ? (BLOCK / 64) * TILE : 1];
    bank_fill_model<NX, NZ>(s_model, a.F, a.Q, a.H, a.R, a.n, a.m);     // (the only barrier)
    const long left = a.N - (long)blockIdx.x * BLOCK;
    const unsigned last_row = (unsigned)(left < BLOCK ? left : BLOCK) - 1u;
    if (!WAVE && threadIdx.x > last_row) return;
    ckf_lane<NX, NZ, LAYOUT, true, WAVE>(a, s_model, s_tile + (WAVE ? (threadIdx.x >> 6) * TILE : 0), last_row);
}

#define FK_CAT_(a, b, c) a##b##_##c
#define FK_CAT(a, b, c) FK_CAT_(a, b, c)

int FK_CAT(launch_ckf_fast_, FK_NX, FK_NZ)(const CkfArgs &a, int layout, hipStream_t stream)
{
    return bank_launch(ckf_fast_kernel<FK_NX, FK_NZ, LAYOUT_SOA>, ckf_fast_kernel<FK_NX, FK_NZ, LAYOUT_AOS>,
                       "ckf_fast_kernel", a, layout, stream);
}

#else  // FK_CKF_GENERAL

constexpr int GX = 16, GZ = 8;

template <int LAYOUT>
__global__ void __launch_bounds__(BLOCK)
ckf_general_kernel(const CkfArgs a)
{
    __shared__ double s_model[LdsModel<GX, GZ>::SIZE];
    bank_fill_model<GX, GZ>(s_model, a.F, a.Q, a.H, a.R, a.n, a.m);
    const long left = a.N - (long)blockIdx.x * BLOCK;
    const unsigned last_row = (unsigned)(left < BLOCK ? left : BLOCK) - 1u;
    if (threadIdx.x > last_row) return;
    ckf_lane<GX, GZ, LAYOUT, false, false>(a, s_model, nullptr, last_row);
}

int launch_ckf_general(const CkfArgs &a, int layout, hipStream_t stream)
{
    return bank_launch(ckf_general_kernel<LAYOUT_SOA>, ckf_general_kernel<LAYOUT_AOS>, "ckf_general_kernel", a, layout, stream);
}

// ------------------------------------------------------------------------------------------------ the building blocks --

struct CkfBlockArgs {
    const double *x_in, *P_in, *sig_f, *sig_h, *noise, *z;
    double *sig_out, *x, *P, *zp, *S, *SI, *Pxz, *K, *y;
    int32_t *status;
    long N;
    int n, m, k;
};

template <int LAYOUT>
__global__ void __launch_bounds__(BLOCK)
ckf_points_kernel(const CkfBlockArgs a)
{
    const long blk0 = (long)blockIdx.x * BLOCK;
    const Lane ln{blk0, threadIdx.x, a.N};
    if (blk0 + ln.tid >= a.N) return;
    const int n = a.n;
    double x[GX], P[GX * GX];
    load_rec<GX, 1, LAYOUT, false>(x, a.x_in, ln, n, 1, 0.0);
    load_rec<GX, GX, LAYOUT, false>(P, a.P_in, ln, n, n, 1.0);
    const RecView<LAYOUT> out(a.sig_out, ln, 2 * n * n);
    const bool pd = ckf_points<GX>(n, x, P, [&](int p, int i, double v) { out.store(p * n + i, v); });
    if (a.status) a.status[blk0 + ln.tid] = pd ? 0 : ST_NOT_PD;
}

// d = a.n (the points' dimension: dim_x or dim_z), k = a.k points; noise [d*d] shared or NULL
template <int LAYOUT>
__global__ void __launch_bounds__(BLOCK)
ckf_transform_kernel(const CkfBlockArgs a)
{
    const long blk0 = (long)blockIdx.x * BLOCK;
    const Lane ln{blk0, threadIdx.x, a.N};
    if (blk0 + ln.tid >= a.N) return;
    const int d = a.n;
    const RecView<LAYOUT> sv(a.sig_f, ln, a.k * d);
    double xo[GX], Po[GX * GX];
    ckf_transform<GX>(d, a.k, [&](int p, int i) { return sv.load(p * d + i); }, a.noise, xo, Po);
    store_rec<GX, 1, LAYOUT, false>(xo, a.x, ln, d, 1);
    store_rec<GX, GX, LAYOUT, false>(Po, a.P, ln, d, d);
}

template <int LAYOUT>
__global__ void __launch_bounds__(BLOCK)
ckf_update_kernel(const CkfBlockArgs a)
{
    const long blk0 = (long)blockIdx.x * BLOCK;
    const Lane ln{blk0, threadIdx.x, a.N};
    if (blk0 + ln.tid >= a.N) return;
    const int n = a.n, m = a.m;
    const RecView<LAYOUT> fv(a.sig_f, ln, 2 * n * n), hv(a.sig_h, ln, 2 * n * m);
    double x[GX], P[GX * GX], z[GZ], zp[GZ], S[GZ * GZ], Pxz[GX * GZ], K[GX * GZ], y[GZ], Lf[GZ * GZ], dinv[GZ];
    load_rec<GX, 1, LAYOUT, false>(x, a.x, ln, n, 1, 0.0);
    load_rec<GX, GX, LAYOUT, false>(P, a.P, ln, n, n, 1.0);
    load_rec<GZ, 1, LAYOUT, false>(z, a.z, ln, m, 1, 0.0);
    int st = ckf_update<GX, GZ>(n, m, [&](int p, int i) { return fv.load(p * n + i); },
                                [&](int p, int r) { return hv.load(p * m + r); }, a.noise, z, a.zp == nullptr, x, P, zp, S,
                                Pxz, K, y, Lf, dinv);
    store_rec<GX, 1, LAYOUT, false>(x, a.x, ln, n, 1);
    store_rec<GX, GX, LAYOUT, false>(P, a.P, ln, n, n);
    if (a.zp) store_rec<GZ, 1, LAYOUT, false>(zp, a.zp, ln, m, 1);
    if (a.S) store_rec<GZ, GZ, LAYOUT, false>(S, a.S, ln, m, m);
    if (a.SI) {
        double SI[GZ * GZ];
        inv_from_ldlt<GZ>(Lf, dinv, SI);
        store_rec<GZ, GZ, LAYOUT, false>(SI, a.SI, ln, m, m);
    }
    if (a.Pxz) store_rec<GX, GZ, LAYOUT, false>(Pxz, a.Pxz, ln, n, m);
    if (a.K) store_rec<GX, GZ, LAYOUT, false>(K, a.K, ln, n, m);
    if (a.y) store_rec<GZ, 1, LAYOUT, false>(y, a.y, ln, m, 1);
    if (a.status) {
        if (!all_finite<GX>(x) || !all_finite<GX * GX>(P)) st |= ST_NONFINITE;
        a.status[blk0 + ln.tid] = st;
    }
}

int launch_ckf_points(int n, long N, int layout, const double *x, const double *P, double *sigmas, int32_t *status,
                      hipStream_t stream)
{
    CkfBlockArgs a{};
    a.x_in = x; a.P_in = P; a.sig_out = sigmas; a.status = status; a.N = N; a.n = n;
    return bank_launch(ckf_points_kernel<LAYOUT_SOA>, ckf_points_kernel<LAYOUT_AOS>, "ckf_points_kernel", a, layout, stream);
}

int launch_ckf_transform(int d, int k, long N, int layout, const double *sigmas, const double *noise, double *x_out,
                         double *P_out, hipStream_t stream)
{
    CkfBlockArgs a{};
    a.sig_f = sigmas; a.noise = noise; a.x = x_out; a.P = P_out; a.N = N; a.n = d; a.k = k;
    return bank_launch(ckf_transform_kernel<LAYOUT_SOA>, ckf_transform_kernel<LAYOUT_AOS>, "ckf_transform_kernel", a, layout,
                       stream);
}

int launch_ckf_update(int n, int m, long N, int layout, const double *sigmas_f, const double *sigmas_h, const double *R,
                      const double *z, double *x, double *P, double *zp, double *S, double *SI, double *Pxz, double *K,
                      double *y, int32_t *status, hipStream_t stream)
{
    CkfBlockArgs a{};
    a.sig_f = sigmas_f; a.sig_h = sigmas_h; a.noise = R; a.z = z; a.x = x; a.P = P; a.zp = zp; a.S = S; a.SI = SI;
    a.Pxz = Pxz; a.K = K; a.y = y; a.status = status; a.N = N; a.n = n; a.m = m;
    return bank_launch(ckf_update_kernel<LAYOUT_SOA>, ckf_update_kernel<LAYOUT_AOS>, "ckf_update_kernel", a, layout, stream);
}

#endif

}  // namespace fk
