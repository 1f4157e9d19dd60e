// info_kernels.hip -- the information filter (filterpy/kalman/information_filter.py:178-289) for a bank of tracks (gfx950).
//
// One track per lane, the whole time loop inside the kernel.  The state is x and P_inv; the model (F, Q, H, R_inv) is shared
// by every track.  G = H' R_inv H and HtRi = H' R_inv are computed once per launch by the workgroup and staged in LDS next to
// F, Q and H.  The step is fk_info.hpp's: two L D L' factorisations of n x n matrices per step -- P = inv(P_inv) after the
// update (reused by the predict that follows), P_inv = inv(F P F' + Q) in the predict -- where the reference inverts three.
//
// Two kernels:
//   info_fast_kernel<NX, NZ>   exact (dim_x, dim_z): x, P_inv and P in VGPRs, every loop unrolled; in NumPy order the four
//       histories leave through an LDS transpose (wave_store_aos), as srkf_kernels.hip's do.  Compiled once per
//       -DFK_NX/-DFK_NZ (fk_dims_info.def).
//   info_general_kernel        everything else (dim_x <= 16, dim_z <= 8): ONE padded (16, 8) instantiation with rolled loops
//       (arrays in scratch).  The padding (identity in F and P_inv, zeros in Q, H, G and HtRi) keeps the padded block exactly
//       the identity and adds exact zeros only, so the real block comes out as the exact kernel's.  A correctness path, not a
//       throughput path.  Compiled with -DFK_INFO_GENERAL=1.
// Which one runs depends on (n, m, layout) only (info_dispatch.cpp): chained calls are bit-identical to one call.
#if defined(FK_INFO_GENERAL) && FK_INFO_GENERAL
#define FK_ROLLED 1
#endif
#include "fk_bank.hpp"
#include "fk_info.hpp"

namespace fk {

// The shared model in LDS, padded to NX / NZ: F | Q | H | G | HtRi, broadcast-read one row at a time.
template <int NX, int NZ>
struct InfoLdsModel {
    static constexpr int OFF_F = 0, OFF_Q = NX * NX, OFF_H = 2 * NX * NX, OFF_G = OFF_H + NZ * NX, OFF_HR = OFF_G + NX * NX;
    static constexpr int SIZE = OFF_HR + NX * NZ;
    const double *s;
    template <int LEN>
    __device__ __forceinline__ void row(int off, double (&r)[LEN]) const
    {
        FK_UNROLL for (int j = 0; j < LEN; ++j) r[j] = s[off + j];
    }
    __device__ __forceinline__ void rowF(int i, double (&r)[NX]) const { row<NX>(OFF_F + i * NX, r); }
    __device__ __forceinline__ void rowQ(int i, double (&r)[NX]) const { row<NX>(OFF_Q + i * NX, r); }
    __device__ __forceinline__ void rowH(int i, double (&r)[NX]) const { row<NX>(OFF_H + i * NX, r); }
    __device__ __forceinline__ void rowG(int i, double (&r)[NX]) const { row<NX>(OFF_G + i * NX, r); }
    __device__ __forceinline__ void rowHtRi(int i, double (&r)[NZ]) const { row<NZ>(OFF_HR + i * NZ, r); }
};

// F, Q, H as given (NULL in the phase that does not read them: pure padding); HtRi = H' R_inv, then G = HtRi H on the lower
// triangle, mirrored.  Two barriers, both before any lane leaves.
template <int NX, int NZ>
__device__ __forceinline__ void info_fill_model(double *s_model, const InfoArgs &a)
{
    using SM = InfoLdsModel<NX, NZ>;
    lds_fill<NX, NX>(s_model + SM::OFF_F, a.F, a.n, a.n, 1.0, threadIdx.x);
    lds_fill<NX, NX>(s_model + SM::OFF_Q, a.Q, a.n, a.n, 0.0, threadIdx.x);
    lds_fill<NZ, NX>(s_model + SM::OFF_H, a.H, a.m, a.n, 0.0, threadIdx.x);
    const bool meas = a.H != nullptr && a.Rinv != nullptr;
    for (unsigned k = threadIdx.x; k < (unsigned)(NX * NZ); k += BLOCK) {
        const int i = (int)k / NZ, c = (int)k % NZ;
        s_model[SM::OFF_HR + k] = (meas && i < a.n && c < a.m) ? info_htri_entry(a.H, a.Rinv, a.n, a.m, i, c) : 0.0;
    }
    __syncthreads();
    for (unsigned k = threadIdx.x; k < (unsigned)(NX * NX); k += BLOCK) {
        const int i = (int)k / NX, j = (int)k % NX;
        const int hi = i > j ? i : j, lo = i > j ? j : i;
        s_model[SM::OFF_G + k] = (meas && hi < a.n) ? info_g_entry(s_model + SM::OFF_HR + hi * NZ, a.H, a.n, a.m, lo) : 0.0;
    }
    __syncthreads();
}

// The whole launch for one lane: NX, NZ the register shapes (the real n, m when EXACT).  last_row: the block's last real
// track; lanes past it (WAVE only) run a copy of that track.
template <int NX, int NZ, int LAYOUT, bool EXACT, bool WAVE>
__device__ __forceinline__ void info_lane(const InfoArgs &a, const double *s_model, double *tile, unsigned last_row)
{
    const long N = a.N;
    const long blk0 = (long)blockIdx.x * BLOCK;
    const unsigned tid = threadIdx.x < last_row ? threadIdx.x : last_row;
    const Lane ln{blk0, tid, N};
    const long track = blk0 + tid;
    const InfoLdsModel<NX, NZ> sm{s_model};
    const int n = EXACT ? NX : a.n, m = EXACT ? NZ : a.m;

    double x[NX], Pi[NX * NX], P[NX * NX];
    load_rec<NX, 1, LAYOUT, EXACT>(x, a.x, ln, n, 1, 0.0);
    load_rec<NX, NX, LAYOUT, EXACT>(Pi, a.Pinv, ln, n, n, 1.0);
    // P_inv is symmetric: the lower triangle is what the step reads, and carrying the upper one as a copy of it lets the
    // compiler keep one register per pair across the time loop
    FK_UNROLL for (int r = 0; r < NX; ++r)
        FK_UNROLL for (int c = r + 1; c < NX; ++c) Pi[r * NX + c] = Pi[c * NX + r];
    FK_UNROLL for (int e = 0; e < NX * NX; ++e) P[e] = 0.0;
    int st = 0;
    bool have_P = false;                            // P == info_spd_inv(Pi) of the Pi held now (set by an update only)
    const bool do_predict = a.phase != INFO_UPDATE, do_update = a.phase != INFO_PREDICT;
    const bool uf = a.update_first != 0 && a.phase == INFO_STEPS;
    for (long t = 0; t < a.T; ++t) {
        if (do_predict && !uf) {
            double bu[NX];
            bank_control<NX, LAYOUT>(a, ln, a.nu > 0 ? a.u + t * N * a.nu : nullptr, 0, bu);
            st |= info_predict<NX>(x, Pi, P, have_P, sm, bu, a.nu > 0, n);
            have_P = false;
            if (a.means_p) bank_put<NX, 1, LAYOUT, EXACT, WAVE>(x, a.means_p, t, ln, n, 1, tile, last_row);
            if (a.covs_p) bank_put<NX, NX, LAYOUT, EXACT, WAVE>(Pi, a.covs_p, t, ln, n, n, tile, last_row);
        }
        if (do_update) {
            const bool upd = a.mask == nullptr || a.mask[t * N + track] != 0;
            if (upd) {
                double z[NZ], y[NZ], K[NX * NZ];
                load_rec<NZ, 1, LAYOUT, EXACT>(z, a.z + t * N * m, ln, m, 1, 0.0);
                st |= info_update<NX, NZ>(x, Pi, P, z, sm, n, y, K, a.K != nullptr);
                have_P = true;
                // the by-products of the last update (single steps; written by every step that updates)
                if (a.y) store_rec<NZ, 1, LAYOUT, EXACT>(y, a.y, ln, m, 1);
                if (a.K) store_rec<NX, NZ, LAYOUT, EXACT>(K, a.K, ln, n, m);
            }
            if (a.means) bank_put<NX, 1, LAYOUT, EXACT, WAVE>(x, a.means, t, ln, n, 1, tile, last_row);
            if (a.covs) bank_put<NX, NX, LAYOUT, EXACT, WAVE>(Pi, a.covs, t, ln, n, n, tile, last_row);
        }
        if (do_predict && uf) {
            double bu[NX];
            bank_control<NX, LAYOUT>(a, ln, a.nu > 0 ? a.u + t * N * a.nu : nullptr, 0, bu);
            st |= info_predict<NX>(x, Pi, P, have_P, sm, bu, a.nu > 0, n);
            have_P = false;
            if (a.means_p) bank_put<NX, 1, LAYOUT, EXACT, WAVE>(x, a.means_p, t, ln, n, 1, tile, last_row);
            if (a.covs_p) bank_put<NX, NX, LAYOUT, EXACT, WAVE>(Pi, a.covs_p, t, ln, n, n, tile, last_row);
        }
    }
    store_rec<NX, 1, LAYOUT, EXACT>(x, a.x, ln, n, 1);
    store_rec<NX, NX, LAYOUT, EXACT>(Pi, a.Pinv, ln, n, n);
    if (a.status) {
        if (!all_finite<NX>(x) || !all_finite<NX * NX>(Pi)) st |= ST_NONFINITE;
        a.status[track] = st;
    }
}

#if !(defined(FK_INFO_GENERAL) && FK_INFO_GENERAL)

template <int NX, int NZ, int LAYOUT>
__global__ void __launch_bounds__(BLOCK)
info_fast_kernel(const InfoArgs a)
{
    constexpr bool WAVE = LAYOUT == LAYOUT_AOS;
    constexpr int TILE = 64 * ((NX * NX) | 1);    // wave_store_aos's tile: 64 records of the longest history, odd row stride
    __shared__ double s_model[InfoLdsModel<NX, NZ>::SIZE];
    __shared__ double s_tile[WAVE ? (BLOCK / 64) * TILE : 1];
    info_fill_model<NX, NZ>(s_model, a);          // (the only barriers: lanes past N may leave after them unless WAVE)
    const long left = a.N - (long)blockIdx.x * BLOCK;
    const unsigned last_row = (unsigned)(left < BLOCK ? left : BLOCK) - 1u;
    if (!WAVE && threadIdx.x > last_row) return;
    info_lane<NX, NZ, LAYOUT, true, WAVE>(a, s_model, s_tile + (WAVE ? (threadIdx.x >> 6) * TILE : 0), last_row);
}

#define FK_CAT_(a, b, c) a##b##_##c
#define FK_CAT(a, b, c) FK_CAT_(a, b, c)

int FK_CAT(launch_info_fast_, FK_NX, FK_NZ)(const InfoArgs &a, int layout, hipStream_t stream)
{
    return bank_launch(info_fast_kernel<FK_NX, FK_NZ, LAYOUT_SOA>, info_fast_kernel<FK_NX, FK_NZ, LAYOUT_AOS>,
                       "info_fast_kernel", a, layout, stream);
}

#else  // FK_INFO_GENERAL

constexpr int GX = 16, GZ = 8;

template <int LAYOUT>
__global__ void __launch_bounds__(BLOCK)
info_general_kernel(const InfoArgs a)
{
    __shared__ double s_model[InfoLdsModel<GX, GZ>::SIZE];
    info_fill_model<GX, GZ>(s_model, a);
    const long left = a.N - (long)blockIdx.x * BLOCK;
    const unsigned last_row = (unsigned)(left < BLOCK ? left : BLOCK) - 1u;
    if (threadIdx.x > last_row) return;
    info_lane<GX, GZ, LAYOUT, false, false>(a, s_model, nullptr, last_row);
}

int launch_info_general(const InfoArgs &a, int layout, hipStream_t stream)
{
    return bank_launch(info_general_kernel<LAYOUT_SOA>, info_general_kernel<LAYOUT_AOS>, "info_general_kernel", a, layout, stream);
}

#endif

}  // namespace fk
