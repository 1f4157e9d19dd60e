// srkf_kernels.hip -- the square-root Kalman filter (filterpy/kalman/square_root.py:172-248) for a bank of tracks (gfx950).
//
// One track per lane, the whole time loop inside the kernel, the model (F, Q1_2, H, R1_2) shared by every track and staged once
// in LDS.  The step is fk_srkf.hpp's: two Householder QR factorisations per step (predict, update) in LAPACK's sign convention
// and one triangular inverse; P is carried as its factor P1_2 and never formed.
//
// Two kernels:
//   srkf_fast_kernel<NX, NZ>   exact (dim_x, dim_z): x, P1_2 and the QR blocks in VGPRs, every loop unrolled; in NumPy order the
//       four histories leave through an LDS transpose (wave_store_aos), as kf_fast.hip's do.  Compiled once per -DFK_NX/-DFK_NZ
//       (fk_dims_srkf.def).
//   srkf_general_kernel        everything else (dim_x <= 16, dim_z <= 8): ONE padded (16, 8) instantiation with rolled loops
//       (arrays in scratch).  The padding (identity in F, P1_2 and R1_2, zeros in Q1_2 and H) adds exact zeros only, and every
//       padded column has an all-zero sub-column (nothing reflected), so the real block comes out as the exact kernel's.
//       A correctness path, not a throughput path.  Compiled with -DFK_SRKF_GENERAL=1.
// Which one runs depends on (n, m, layout) only (srkf_dispatch.cpp): chained calls are bit-identical to one call.
#if defined(FK_SRKF_GENERAL) && FK_SRKF_GENERAL
#define FK_ROLLED 1
#endif
#include "fk_bank.hpp"
#include "fk_srkf.hpp"

namespace fk {

// the lower triangle of a loaded factor (its upper triangle is not read: zeros)
template <int NX>
__device__ __forceinline__ void srkf_lower(double (&L)[NX * NX])
{
    FK_UNROLL for (int r = 0; r < NX; ++r)
        FK_UNROLL for (int c = r + 1; c < NX; ++c) L[r * NX + c] = 0.0;
}

// The whole launch for one lane: NX, NZ the register shapes (the real n, m when EXACT).  last_row: the block's last real
// track; lanes past it (WAVE only) run a copy of that track.
template <int NX, int NZ, int LAYOUT, bool EXACT, bool WAVE>
__device__ __forceinline__ void srkf_lane(const SrkfArgs &a, const double *s_model, double *tile, unsigned last_row)
{
    const long N = a.N;
    const long blk0 = (long)blockIdx.x * BLOCK;
    const unsigned tid = threadIdx.x < last_row ? threadIdx.x : last_row;
    const Lane ln{blk0, tid, N};
    const long track = blk0 + tid;
    const LdsModel<NX, NZ> sm{s_model};
    const int n = EXACT ? NX : a.n, m = EXACT ? NZ : a.m;

    double x[NX], L[NX * NX];
    load_rec<NX, 1, LAYOUT, EXACT>(x, a.x, ln, n, 1, 0.0);
    load_rec<NX, NX, LAYOUT, EXACT>(L, a.P12, ln, n, n, 1.0);
    srkf_lower<NX>(L);
    int st = 0;
    const bool do_predict = a.phase != SRKF_UPDATE, do_update = a.phase != SRKF_PREDICT;
    const bool uf = a.update_first != 0 && a.phase == SRKF_STEPS;
    for (long t = 0; t < a.T; ++t) {
        if (do_predict && !uf) {
            double bu[NX];
            bank_control<NX, LAYOUT>(a, ln, a.nu > 0 ? a.u + t * N * a.nu : nullptr, 0, bu);
            srkf_predict<NX>(x, L, sm, bu, a.nu > 0);
            if (a.means_p) bank_put<NX, 1, LAYOUT, EXACT, WAVE>(x, a.means_p, t, ln, n, 1, tile, last_row);
            if (a.covs_p) bank_put<NX, NX, LAYOUT, EXACT, WAVE>(L, a.covs_p, t, ln, n, n, tile, last_row);
        }
        if (do_update) {
            const bool upd = a.mask == nullptr || a.mask[t * N + track] != 0;
            if (upd) {
                double z[NZ], y[NZ], K[NX * NZ], S[NZ * NZ], SI[NZ * NZ];
                load_rec<NZ, 1, LAYOUT, EXACT>(z, a.z + t * N * m, ln, m, 1, 0.0);
                st |= srkf_update<NX, NZ>(x, L, z, sm, m, y, K, S, SI);
                // the by-products of the last update (single steps; written by every step that updates)
                if (a.y) store_rec<NZ, 1, LAYOUT, EXACT>(y, a.y, ln, m, 1);
                if (a.K) store_rec<NX, NZ, LAYOUT, EXACT>(K, a.K, ln, n, m);
                if (a.S12) store_rec<NZ, NZ, LAYOUT, EXACT>(S, a.S12, ln, m, m);
                if (a.SI12) store_rec<NZ, NZ, LAYOUT, EXACT>(SI, a.SI12, ln, m, m);
            }
            if (a.means) bank_put<NX, 1, LAYOUT, EXACT, WAVE>(x, a.means, t, ln, n, 1, tile, last_row);
            if (a.covs) bank_put<NX, NX, LAYOUT, EXACT, WAVE>(L, a.covs, t, ln, n, n, tile, last_row);
        }
        if (do_predict && uf) {
            double bu[NX];
            bank_control<NX, LAYOUT>(a, ln, a.nu > 0 ? a.u + t * N * a.nu : nullptr, 0, bu);
            srkf_predict<NX>(x, L, sm, bu, a.nu > 0);
            if (a.means_p) bank_put<NX, 1, LAYOUT, EXACT, WAVE>(x, a.means_p, t, ln, n, 1, tile, last_row);
            if (a.covs_p) bank_put<NX, NX, LAYOUT, EXACT, WAVE>(L, a.covs_p, t, ln, n, n, tile, last_row);
        }
    }
    store_rec<NX, 1, LAYOUT, EXACT>(x, a.x, ln, n, 1);
    store_rec<NX, NX, LAYOUT, EXACT>(L, a.P12, ln, n, n);
    if (a.status) {
        if (!all_finite<NX>(x) || !all_finite<NX * NX>(L)) st |= ST_NONFINITE;
        a.status[track] = st;
    }
}

#if !(defined(FK_SRKF_GENERAL) && FK_SRKF_GENERAL)

template <int NX, int NZ, int LAYOUT>
__global__ void __launch_bounds__(BLOCK)
srkf_fast_kernel(const SrkfArgs a)
{
    constexpr bool WAVE = LAYOUT == LAYOUT_AOS;
    constexpr int TILE = 64 * ((NX * NX) | 1);    // wave_store_aos's tile: 64 records of the longest history, odd row stride
    __shared__ double s_model[LdsModel<NX, NZ>::SIZE];
    __shared__ double s_tile[WAVE ? (BLOCK / 64) * TILE : 1];
    // (the only barrier: lanes past N may leave after it unless WAVE)
    bank_fill_model<NX, NZ>(s_model, a.F, a.Q12, a.H, a.R12, a.n, a.m);
    const long left = a.N - (long)blockIdx.x * BLOCK;
    const unsigned last_row = (unsigned)(left < BLOCK ? left : BLOCK) - 1u;
    if (!WAVE && threadIdx.x > last_row) return;
    srkf_lane<NX, NZ, LAYOUT, true, WAVE>(a, s_model, s_tile + (WAVE ? (threadIdx.x >> 6) * TILE : 0), last_row);
}

#define FK_CAT_(a, b, c) a##b##_##c
#define FK_CAT(a, b, c) FK_CAT_(a, b, c)

int FK_CAT(launch_srkf_fast_, FK_NX, FK_NZ)(const SrkfArgs &a, int layout, hipStream_t stream)
{
    return bank_launch(srkf_fast_kernel<FK_NX, FK_NZ, LAYOUT_SOA>, srkf_fast_kernel<FK_NX, FK_NZ, LAYOUT_AOS>,
                       "srkf_fast_kernel", a, layout, stream);
}

#else  // FK_SRKF_GENERAL

constexpr int GX = 16, GZ = 8;

template <int LAYOUT>
__global__ void __launch_bounds__(BLOCK)
srkf_general_kernel(const SrkfArgs a)
{
    __shared__ double s_model[LdsModel<GX, GZ>::SIZE];
    bank_fill_model<GX, GZ>(s_model, a.F, a.Q12, a.H, a.R12, a.n, a.m);
    const long left = a.N - (long)blockIdx.x * BLOCK;
    const unsigned last_row = (unsigned)(left < BLOCK ? left : BLOCK) - 1u;
    if (threadIdx.x > last_row) return;
    srkf_lane<GX, GZ, LAYOUT, false, false>(a, s_model, nullptr, last_row);
}

int launch_srkf_general(const SrkfArgs &a, int layout, hipStream_t stream)
{
    return bank_launch(srkf_general_kernel<LAYOUT_SOA>, srkf_general_kernel<LAYOUT_AOS>, "srkf_general_kernel", a, layout, stream);
}

#endif

}  // namespace fk
