// ukf_simplex.hip -- fused linear-model unscented Kalman filter on the SIMPLEX sigma-point set (n + 1 points,
// filterpy/kalman/sigma_points.py:386-534) for gfx950 (MI355X).
//
//   ukf_simplex_kernel      <- UnscentedKalmanFilter(points=SimplexSigmaPoints(n)).batch_filter (filterpy/kalman/UKF.py:524-632)
//                              with fx(x, dt) = F x, hx(x) = H x: the predict / update loop in registers over the time steps
//   ukf_simplex_rts_kernel  <- .rts_smoother (UKF.py:634-739), likewise
// Reached through fk_ukf_linear_batch_f64 / fk_ukf_linear_rts_f64 with FK_UKF_FLAG_SIMPLEX (ukf_dispatch.cpp); the arithmetic of
// a step is fk_ukf_simplex.hpp (held against the live-reference goldens on the host by tests/test_hostcheck_ukf_simplex.py).
// One track per lane, the time loop inside the launch, and the kernel around the step built by the rules of ukf_kernels.hip
// (see there for the why of each): EXACT instantiations without element guards and padded ones for every smaller size; the
// next step's measurement and mask byte requested in front of this step's stores; no store in the loop predicated -- lanes
// past the bank's last track duplicate the block's last track, optional outputs get a descriptor of zero records; NumPy order
// at the exact even dims leaves (and, in the smoother, arrives) through a wave-private LDS tile, 1 KiB contiguous per
// instruction.  Not taken over: the 16-byte element-major stores, the persistent ticket grid, the smoother's LDS-DMA fetch and
// chunked calls -- nobody has measured this kernel yet (docs/KERNEL_NOTES.md).
// FK_SIMPLEX_PART: the Makefile compiles this file four times (parallel build) -- 1: forward dim_x <= 6, 2: forward 7..9,
// 3: smoother dim_x <= 6, 4: smoother 7..9.
#include <stdlib.h>

#ifndef FK_SIMPLEX_PART
#define FK_SIMPLEX_PART 0
#endif
#define FK_SIMPLEX_HAS(p) (FK_SIMPLEX_PART == 0 || FK_SIMPLEX_PART == (p))
// (parts 91 / 92: the forward / smoother kernel templates alone, for one-off instantiations)
#define FK_SIMPLEX_FWD (FK_SIMPLEX_HAS(1) || FK_SIMPLEX_HAS(2) || FK_SIMPLEX_PART == 91)
#define FK_SIMPLEX_RTS (FK_SIMPLEX_HAS(3) || FK_SIMPLEX_HAS(4) || FK_SIMPLEX_PART == 92)

#include "../../include/filterhip.h"
#include "fk_device.hpp"
#include "fk_kernel_args.hpp"
#include "fk_launchers.hpp"
#include "fk_math_sym.hpp"
#include "fk_ukf_simplex.hpp"

namespace fk {

// The shared operands of both kernels in LDS: the padded model, then Wm | Wc (NX + 1 each, weight 0 behind point n), then
// the table a | b (NX each, 0 from row n on).
template <int NX, int NZ>
struct SimplexShared {
    using Model = LdsModel<NX, NZ>;
    static constexpr int KS = NX + 1;
    static constexpr int OFF_WM = Model::SIZE, OFF_WC = OFF_WM + KS, OFF_SA = OFF_WC + KS, OFF_SB = OFF_SA + NX;
    static constexpr int SIZE = OFF_SB + NX;
    struct View { Model sm; const double *Wm, *Wc, *Sa, *Sb; };
    __device__ static __forceinline__ void fill_points(double *s, const double *pWm, const double *pWc, const SimplexTable &tab, int n)
    {
        for (unsigned q = threadIdx.x; q < (unsigned)(2 * KS); q += BLOCK) {
            const int which = q / KS, j = q % KS;
            const double *W = which ? pWc : pWm;
            s[OFF_WM + q] = j <= n ? W[j] : 0.0;
        }
        for (unsigned q = threadIdx.x; q < (unsigned)NX; q += BLOCK) {
            s[OFF_SA + q] = (int)q < n ? tab.a[q] : 0.0;
            s[OFF_SB + q] = (int)q < n ? tab.b[q] : 0.0;
        }
    }
    // a view the optimiser cannot relate to the previous one (an opaque OFFSET: the LDS address space is kept), ordered
    // behind the arithmetic that produced `after`: see ukf_kernels.hip
    __device__ static __forceinline__ View view(const double *s, double after)
    {
        int off = 0;
        asm volatile("" : "+v"(off) : "v"(after));
        const double *mb = s + off;
        return View{Model{mb}, mb + OFF_WM, mb + OFF_WC, mb + OFF_SA, mb + OFF_SB};
    }
};

#if FK_SIMPLEX_FWD
template <int NX, int NZ, int LAYOUT, bool EXACT>
__global__ void __launch_bounds__(BLOCK, (NX <= 2 ? 4 : NX <= 6 ? 2 : 1))
ukf_simplex_kernel(const UkfArgs a, const SimplexTable tab, const double *__restrict__ pF, const double *__restrict__ pH,
                   const double *__restrict__ pQ, const double *__restrict__ pR, const double *__restrict__ pWm,
                   const double *__restrict__ pWc, const double *__restrict__ pz, const uint8_t *__restrict__ pmask)
{
    constexpr int PL = NX * (NX + 1) / 2;
    using Shared = SimplexShared<NX, NZ>;
    using SharedModel = typename Shared::Model;
    __shared__ double s_model[Shared::SIZE];
    // NumPy order at the exact even dims: the per-step outputs leave through a wave-private LDS tile (wave_store_aos_flat)
    constexpr bool COOP = EXACT && LAYOUT == LAYOUT_AOS && NX <= 8 && NX % 2 == 0;
    constexpr int TILE = 64 * NX * NX;
    __shared__ double s_tile[COOP ? (BLOCK / 64) * TILE : 1];
    const long N = a.N;
    const int n = EXACT ? NX : a.n, m = EXACT ? NZ : a.m;
    double *tile = s_tile + (COOP ? (threadIdx.x >> 6) * TILE : 0);
    const unsigned lane = threadIdx.x & 63u, wave_row0 = (threadIdx.x >> 6) * 64u;

    lds_fill<NX, NX>(s_model + SharedModel::OFF_F, pF, n, n, 1.0, threadIdx.x);
    lds_fill<NX, NX>(s_model + SharedModel::OFF_Q, pQ, n, n, 1.0, threadIdx.x);   // padded block of P stays I
    lds_fill<NZ, NX>(s_model + SharedModel::OFF_H, pH, m, n, 0.0, threadIdx.x);
    lds_fill<NZ, NZ>(s_model + SharedModel::OFF_R, pR, m, m, 1.0, threadIdx.x);
    Shared::fill_points(s_model, pWm, pWc, tab, n);
    __syncthreads();
    auto fresh = [&](double after = 0.0) { return Shared::view(s_model, after); };

    const long blk0 = a.i0 + (long)blockIdx.x * BLOCK;
    const long left = a.i0 + a.cnt - blk0;
    const unsigned last_row = (unsigned)(left < BLOCK ? left : BLOCK) - 1u;
    const bool live = threadIdx.x <= last_row;
    const Lane ln{blk0, live ? threadIdx.x : last_row, N};      // lanes past the last track duplicate it
    double x[NX], P[PL];
    load_rec<NX, 1, LAYOUT, EXACT>(x, a.x, ln, n, 1, 0.0);
    {
        const RecView<LAYOUT> pv(a.P, ln, n * n);
        FK_UNROLL for (int i = 0; i < NX; ++i)
            FK_UNROLL for (int j = 0; j < NX; ++j)
                if (j >= i) P[sym_idx<NX>(i, j)] = (EXACT || (i < n && j < n)) ? pv.load(i * n + j) : (i == j ? 1.0 : 0.0);
    }
    // without a mask the byte comes from a valid dummy address (the measurements) and is selected away: no branch
    const uint8_t *mk0 = (pmask ? pmask : reinterpret_cast<const uint8_t *>(pz)) + blk0;
    unsigned hc = __builtin_amdgcn_raw_buffer_load_b8(make_rsrc(mk0), ln.tid, 0, 0);
    // z is carried from step to step: z[t+1] is requested at the end of step t in front of that step's stores
    double zc[NZ];
    load_rec<NZ, 1, LAYOUT, EXACT>(zc, pz, ln, m, 1, 0.0);
    // the prologue's loads are landed before the loop
    FK_UNROLL for (int c = 0; c < NX; ++c) asm volatile("" ::"v"(x[c]));
    FK_UNROLL for (int e = 0; e < PL; ++e) asm volatile("" ::"v"(P[e]));
    FK_UNROLL for (int c = 0; c < NZ; ++c) asm volatile("" ::"v"(zc[c]));
    asm volatile("" ::"v"(hc));
    const bool st_m = a.means != nullptr, st_c = a.covs != nullptr;
    int st = 0;

    _Pragma("nounroll") for (long t = 0; t < a.T; ++t) {
        const bool has_z = pmask ? hc != 0u : true;
        auto load_z = [&](double (&z)[NZ]) { FK_UNROLL for (int c = 0; c < NZ; ++c) z[c] = zc[c]; };
        st |= ukf_simplex_step<NX, NZ>(x, P, load_z, has_z, fresh);
        FK_STAGE();
        // step t+1's measurement and mask byte (clamped index, no branch), in front of this step's stores
        {
            long tn = t + 1 < a.T ? t + 1 : t;
            asm volatile("" : "+s"(tn));
            hc = __builtin_amdgcn_raw_buffer_load_b8(make_rsrc(mk0 + tn * N), ln.tid, 0, 0);
            load_rec<NZ, 1, LAYOUT, EXACT>(zc, pz + tn * N * m, ln, m, 1, 0.0);
        }
        FK_STAGE();
        double Pf[NX * NX];
        FK_UNROLL for (int i = 0; i < NX; ++i)
            FK_UNROLL for (int j = 0; j < NX; ++j) Pf[i * NX + j] = P[sym_idx<NX>(i, j)];
        if constexpr (COOP) {
            wave_store_aos_flat<NX>(x, a.means + t * N * NX + blk0 * NX, wave_row0, tile, lane, last_row, st_m);
            wave_store_aos_flat<NX * NX>(Pf, a.covs + t * N * (NX * NX) + blk0 * (NX * NX), wave_row0, tile, lane, last_row, st_c);
        } else {
            store_rec<NX, 1, LAYOUT, EXACT>(x, a.means + t * N * n, ln, n, 1, st_m);
            store_rec<NX, NX, LAYOUT, EXACT>(Pf, a.covs + t * N * n * n, ln, n, n, st_c);
        }
    }
    // the in-place store of the final state is predicated and behind a barrier: a duplicate must have consumed x0 / P0 before
    // its owner overwrites them
    __syncthreads();
    if (live) {
        store_rec<NX, 1, LAYOUT, EXACT>(x, a.x, ln, n, 1);
        double Pf[NX * NX];
        FK_UNROLL for (int i = 0; i < NX; ++i)
            FK_UNROLL for (int j = 0; j < NX; ++j) Pf[i * NX + j] = P[sym_idx<NX>(i, j)];
        store_rec<NX, NX, LAYOUT, EXACT>(Pf, a.P, ln, n, n);
        if (a.status) {
            if (!all_finite<NX>(x) || !all_finite<PL>(P)) st |= ST_NONFINITE;
            a.status[ln.blk0 + ln.tid] = a.status_or ? (a.status[ln.blk0 + ln.tid] | st) : st;
        }
    }
}

// One class: the exact instantiation where the dims are the class's own, the padded one otherwise.  PADDED = false: a class
// that only ever serves its own dims -- (9,4): dim_x 9 with dim_z 4 and nothing else -- has no padded instantiation.
template <int NXV, int NZV, bool PADDED = true>
static void simplex_fwd_go(const UkfArgs &a, const SimplexTable &tab, int layout, hipStream_t s)
{
    const dim3 grid((unsigned)((a.cnt + BLOCK - 1) / BLOCK)), block(BLOCK);
    const bool ex = !PADDED || (a.n == NXV && a.m == NZV);
#define FK_SIMPLEX_LAUNCH(LAY, EX) hipLaunchKernelGGL((ukf_simplex_kernel<NXV, NZV, LAY, EX>), grid, block, 0, s, a, tab, a.F, a.H, a.Q, a.R, a.Wm, a.Wc, a.z, a.mask)
    if (layout == FK_LAYOUT_SOA) {
        if (ex) FK_SIMPLEX_LAUNCH(LAYOUT_SOA, true);
        else if constexpr (PADDED) FK_SIMPLEX_LAUNCH(LAYOUT_SOA, false);
    } else {
        if (ex) FK_SIMPLEX_LAUNCH(LAYOUT_AOS, true);
        else if constexpr (PADDED) FK_SIMPLEX_LAUNCH(LAYOUT_AOS, false);
    }
#undef FK_SIMPLEX_LAUNCH
}
#if FK_SIMPLEX_HAS(1)
int ukf_simplex_fwd_launch_small(const UkfArgs &a, const SimplexTable &tab, int layout, hipStream_t s)
{
    if (a.n <= 2 && a.m <= 2) simplex_fwd_go<2, 2>(a, tab, layout, s);
    else if (a.n <= 4 && a.m <= 2) simplex_fwd_go<4, 2>(a, tab, layout, s);
    else simplex_fwd_go<6, 3>(a, tab, layout, s);
    return check_launch("ukf_simplex_kernel");
}
#endif
#if FK_SIMPLEX_HAS(2)
int ukf_simplex_fwd_launch_big(const UkfArgs &a, const SimplexTable &tab, int layout, hipStream_t s)
{
    if (a.n <= 8) simplex_fwd_go<8, 4>(a, tab, layout, s);
    else if (a.m <= 3) simplex_fwd_go<9, 3>(a, tab, layout, s);
    else simplex_fwd_go<9, 4, false>(a, tab, layout, s);
    return check_launch("ukf_simplex_kernel");
}
#endif
#endif

#if FK_SIMPLEX_RTS
// The whole backward loop in one launch, the smoothed step k+1 carried in registers -- or, from dim_x 7 on and wherever the
// LDS holds it, parked in LDS between its birth and its one use (PARK: ukf_kernels.hip).  Reads Xs[k], Ps[k]; writes xs[k],
// ps[k], Ks[k].  The K of the last step is zero; the reference's Qs argument is never read (UKF.py:717-719): the filter's Q.
template <int NX, int LAYOUT, bool EXACT>
__global__ void __launch_bounds__(BLOCK, (NX <= 2 ? 4 : NX <= 4 ? 2 : 1))
ukf_simplex_rts_kernel(const UkfRtsArgs a, const SimplexTable tab, const double *__restrict__ pF, const double *__restrict__ pQ,
                       const double *__restrict__ pWm, const double *__restrict__ pWc)
{
    constexpr int PL = NX * (NX + 1) / 2;
    constexpr int NN = NX * NX;
    constexpr bool COOP = EXACT && LAYOUT == LAYOUT_AOS && NX % 2 == 0 && NX <= 8;
    using Shared = SimplexShared<NX, 1>;
    using SharedModel = typename Shared::Model;
    __shared__ double s_model[Shared::SIZE];
    __shared__ double s_tile[COOP ? (BLOCK / 64) * 64 * NN : 1];
    constexpr bool PARK = NX >= 7 && ((COOP ? (BLOCK / 64) * 64 * NN : 1) + (BLOCK / 64) * 64 * (NX + PL)) * 8 + 4096 <= 160 * 1024;
    __shared__ double s_park[PARK ? (BLOCK / 64) * 64 * (NX + PL) : 1];
    double *park = s_park + (PARK ? (threadIdx.x >> 6) * 64 * (NX + PL) + (threadIdx.x & 63u) : 0);
    const long N = a.N;
    const long blk0 = a.i0 + (long)blockIdx.x * BLOCK;
    const long left = a.i0 + a.cnt - blk0;
    const unsigned last_row = (unsigned)(left < BLOCK ? left : BLOCK) - 1u;
    const bool live = threadIdx.x <= last_row;
    const Lane ln{blk0, live ? threadIdx.x : last_row, N};
    const int n = EXACT ? NX : a.n;
    double *tile = s_tile + (COOP ? (threadIdx.x >> 6) * 64 * NN : 0);
    const unsigned lane = threadIdx.x & 63u, wave_row0 = (threadIdx.x >> 6) * 64u;
    lds_fill<NX, NX>(s_model + SharedModel::OFF_F, pF, n, n, 1.0, threadIdx.x);
    lds_fill<NX, NX>(s_model + SharedModel::OFF_Q, pQ, n, n, 1.0, threadIdx.x);
    Shared::fill_points(s_model, pWm, pWc, tab, n);
    __syncthreads();
    auto fresh = [&](double after = 0.0) { return Shared::view(s_model, after); };
    int st = 0;

    // the filtered state of step t: element-major (and the padded classes) into the lane's own registers; cooperative: the
    // wave's slab as register quads, then through the tile
    auto fetch = [&](const double *srcx, const double *srcP, long t, double (&x)[NX], double (&Pf)[NN]) {
        if constexpr (COOP) {
            WaveAosFetch<NX> fx;
            WaveAosFetch<NN> fP;
            fx.issue(srcx + t * N * NX + blk0 * NX, wave_row0, lane, last_row);
            fP.issue(srcP + t * N * NN + blk0 * NN, wave_row0, lane, last_row);
            fx.to_tile(tile, lane);
            FK_UNROLL for (int c = 0; c < NX; ++c) x[c] = tile[lane * NX + c];
            fP.to_tile(tile, lane);
            FK_UNROLL for (int e = 0; e < NN; ++e) Pf[e] = tile[lane * NN + e];
            wave_lds_fence();
        } else {
            load_rec<NX, 1, LAYOUT, EXACT>(x, srcx + t * N * n, ln, n, 1, 0.0);
            load_rec<NX, NX, LAYOUT, EXACT>(Pf, srcP + t * N * n * n, ln, n, n, 1.0);
        }
    };
    auto pack = [&](const double (&Pf)[NN], double (&P)[PL]) {
        FK_UNROLL for (int i = 0; i < NX; ++i)
            FK_UNROLL for (int j = 0; j < NX; ++j)
                if (j >= i) P[sym_idx<NX>(i, j)] = Pf[i * NX + j];
    };
    auto store_x = [&](long t, const double (&x)[NX]) {
        if constexpr (COOP) wave_store_aos_flat<NX>(x, a.xs + t * N * NX + blk0 * NX, wave_row0, tile, lane, last_row);
        else store_rec<NX, 1, LAYOUT, EXACT>(x, a.xs + t * N * n, ln, n, 1);
    };
    auto store_full = [&](double *arr, long t, const double (&M)[NN]) {
        if constexpr (COOP) wave_store_aos_flat<NN>(M, arr + t * N * NN + blk0 * NN, wave_row0, tile, lane, last_row);
        else store_rec<NX, NX, LAYOUT, EXACT>(M, arr + t * N * n * n, ln, n, n);
    };

    // the last step is the filter's own output, copied as it is (both triangles: xs, ps = Xs.copy(), Ps.copy())
    double xn[NX], Pn[PL];
    {
        double Pf[NN];
        fetch(a.Xs, a.Ps, a.T - 1, xn, Pf);
        pack(Pf, Pn);
        store_x(a.T - 1, xn);
        store_full(a.ps, a.T - 1, Pf);
        if (a.Ks) {
            double Z[NN];
            FK_UNROLL for (int e = 0; e < NN; ++e) Z[e] = 0.0;
            store_full(a.Ks, a.T - 1, Z);
        }
    }
    FK_UNROLL for (int c = 0; c < NX; ++c) asm volatile("" ::"v"(xn[c]));
    FK_UNROLL for (int e = 0; e < PL; ++e) asm volatile("" ::"v"(Pn[e]));
    if constexpr (PARK) {
        FK_UNROLL for (int c = 0; c < NX; ++c) park[c * 64] = xn[c];
        FK_UNROLL for (int e = 0; e < PL; ++e) park[(NX + e) * 64] = Pn[e];
    }
    _Pragma("nounroll") for (long t = a.T - 2; t >= 0; --t) {
        double x[NX], P[PL], K[NN];
        {
            double Pf[NN];
            fetch(a.Xs, a.Ps, t, x, Pf);
            pack(Pf, P);
        }
        {
            double xb[NX], Pb[PL];
            st |= ukf_simplex_rts_gain<NX>(x, P, xb, Pb, K, fresh);
            if constexpr (PARK) {
                double xq[NX], Pq[PL];
                FK_UNROLL for (int c = 0; c < NX; ++c) xq[c] = park[c * 64];
                FK_UNROLL for (int e = 0; e < PL; ++e) Pq[e] = park[(NX + e) * 64];
                ukf_linear_rts_correct<NX>(x, P, xq, Pq, xb, Pb, K);
                FK_UNROLL for (int c = 0; c < NX; ++c) park[c * 64] = x[c];
                FK_UNROLL for (int e = 0; e < PL; ++e) park[(NX + e) * 64] = P[e];
            } else {
                ukf_linear_rts_correct<NX>(x, P, xn, Pn, xb, Pb, K);
                FK_UNROLL for (int c = 0; c < NX; ++c) xn[c] = x[c];
                FK_UNROLL for (int e = 0; e < PL; ++e) Pn[e] = P[e];
            }
        }
        store_x(t, x);
        {
            double Pf[NN];
            FK_UNROLL for (int i = 0; i < NX; ++i)
                FK_UNROLL for (int j = 0; j < NX; ++j) Pf[i * NX + j] = P[sym_idx<NX>(i, j)];
            store_full(a.ps, t, Pf);
        }
        if (a.Ks) store_full(a.Ks, t, K);
    }
    if constexpr (PARK) {
        FK_UNROLL for (int c = 0; c < NX; ++c) xn[c] = park[c * 64];
        FK_UNROLL for (int e = 0; e < PL; ++e) Pn[e] = park[(NX + e) * 64];
    }
    if (live && a.status) {
        if (!all_finite<NX>(xn) || !all_finite<PL>(Pn)) st |= ST_NONFINITE;
        a.status[ln.blk0 + ln.tid] = a.status_or ? (a.status[ln.blk0 + ln.tid] | st) : st;
    }
}

// (PADDED = false: the class 9 serves dim_x 9 alone)
template <int NXV, bool PADDED = true>
static void simplex_rts_go(const UkfRtsArgs &a, const SimplexTable &tab, const double *F, const double *Q, const double *Wm, const double *Wc, int layout, hipStream_t s)
{
    const dim3 grid((unsigned)((a.cnt + BLOCK - 1) / BLOCK)), block(BLOCK);
    const bool ex = !PADDED || a.n == NXV;
#define FK_SIMPLEX_LAUNCH(LAY, EX) hipLaunchKernelGGL((ukf_simplex_rts_kernel<NXV, LAY, EX>), grid, block, 0, s, a, tab, F, Q, Wm, Wc)
    if (layout == FK_LAYOUT_SOA) {
        if (ex) FK_SIMPLEX_LAUNCH(LAYOUT_SOA, true);
        else if constexpr (PADDED) FK_SIMPLEX_LAUNCH(LAYOUT_SOA, false);
    } else {
        if (ex) FK_SIMPLEX_LAUNCH(LAYOUT_AOS, true);
        else if constexpr (PADDED) FK_SIMPLEX_LAUNCH(LAYOUT_AOS, false);
    }
#undef FK_SIMPLEX_LAUNCH
}
#if FK_SIMPLEX_HAS(3)
int ukf_simplex_rts_launch_small(const UkfRtsArgs &a, const SimplexTable &tab, const double *F, const double *Q, const double *Wm, const double *Wc, int layout, hipStream_t s)
{
    if (a.n <= 2) simplex_rts_go<2>(a, tab, F, Q, Wm, Wc, layout, s);
    else if (a.n <= 4) simplex_rts_go<4>(a, tab, F, Q, Wm, Wc, layout, s);
    else simplex_rts_go<6>(a, tab, F, Q, Wm, Wc, layout, s);
    return check_launch("ukf_simplex_rts_kernel");
}
#endif
#if FK_SIMPLEX_HAS(4)
int ukf_simplex_rts_launch_big(const UkfRtsArgs &a, const SimplexTable &tab, const double *F, const double *Q, const double *Wm, const double *Wc, int layout, hipStream_t s)
{
    if (a.n <= 8) simplex_rts_go<8>(a, tab, F, Q, Wm, Wc, layout, s);
    else simplex_rts_go<9, false>(a, tab, F, Q, Wm, Wc, layout, s);
    return check_launch("ukf_simplex_rts_kernel");
}
#endif
#endif

}  // namespace fk
