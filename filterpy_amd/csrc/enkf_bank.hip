// enkf_bank.hip -- the ensemble Kalman filter (filterpy/kalman/ensemble_kalman_filter.py:218-290) for a BANK of B ensembles of
// N <= ENKF_CHUNK members each (gfx950): a whole predict() is ONE launch for all ensembles, and so is a whole update().
//
// enkf_kernels.hip spreads one ensemble over the grid and needs the launch boundary between its pass kernels and the
// one-workgroup finalize.  An ensemble that fits one chunk fits one workgroup: nothing waits for another workgroup, so the
// sums, S^-1, the gain, the members and the new mean follow each other inside one kernel, separated by barriers of the lanes
// that hold the ensemble.  The arithmetic is fk_enkf.hpp's and the tree is fk_enkf_dev.hpp's, in the single-ensemble kernels'
// order: the result for ensemble b is bit-identical to fk_enkf_predict_f64 / fk_enkf_update_f64 on slice b
// (tests/test_gpu_enkf_bank.py).  What the single path does for its one slab is kept step by step: the slab goes to LDS and
// enkf_run_sum / enkf_total add it up with nslabs = 1 -- 0.0 + slab, then fifteen + 0.0 -- which also turns a sum of -0.0
// into +0.0 as there.
//
// Two routes, chosen by N in the launcher:
//   one wave per ensemble (N <= 64)       four ensembles per 256-lane workgroup, each wave on its own part of LDS.  No
//       workgroup barrier, only the wave's own order (wave_lds_fence).  A lane holds at most one member: it stays in registers
//       between the sums and the apply, so an update reads the ensemble and the noise once and writes the ensemble once.  A wave
//       past the last ensemble, or one whose ensemble is masked, leaves at once.
//   one workgroup per ensemble (64 < N <= 2048)   lane l takes members l, l + 256, ... as enkf_kernels.hip does.  The apply
//       phase READS THE MEMBERS AGAIN from global memory -- in practice from L2: the ensemble is at most 2048 x 16 doubles
//       (256 KiB) and was read by the same workgroup microseconds before.  Keeping them in LDS instead would need up to
//       2048 x (dim_x + dim_z) doubles (208 KiB at (9, 4), beyond the 160 KiB of a CU, and one workgroup per CU long before
//       that); keeping them in registers needs 8 x (dim_x + dim_z) doubles per lane next to the 58 sums at (9, 4).  The second
//       read costs no HBM traffic as long as the ensemble stays in L2; neither alternative has been measured.
// enkf_spd_inverse runs on one lane, as in the single path's finalize, with its work arrays in LDS (enkf_spd_inverse_in):
// the exact kernels use no scratch memory (profiles/enkf/bank_isa.json).
//
// No atomics on global memory, no waiting between workgroups, no state between launches: there is no workspace.
// Builds: exact (dim_x, dim_z) of fk_dims_enkf.def (-DFK_NX/-DFK_NZ) and ONE padded rolled instantiation up to (16, 8)
// (-DFK_ENKF_GENERAL=1), as enkf_kernels.hip.
#if defined(FK_ENKF_GENERAL) && FK_ENKF_GENERAL
#define FK_ROLLED 1
#endif
#include "fk_device.hpp"
#include "fk_enkf.hpp"
#include "fk_enkf_dev.hpp"

namespace fk {

constexpr int ENKF_WAVE = 64;

// the G lanes that hold one ensemble: a wave (G = 64; four groups per workgroup) or the workgroup (G = 256)
template <int G>
struct EnkfGroup {
    static_assert(G == ENKF_WAVE || G == ENKF_BLOCK, "a wave or the workgroup");
    static constexpr int PER_BLOCK = ENKF_BLOCK / G;
    static constexpr int PER_LANE = G == ENKF_WAVE ? 1 : ENKF_PER_LANE;
    static __device__ __forceinline__ unsigned lid() { return G == ENKF_WAVE ? (threadIdx.x & 63u) : threadIdx.x; }
    static __device__ __forceinline__ unsigned sub() { return G == ENKF_WAVE ? wave_index() : 0u; }
    static __device__ __forceinline__ void sync()
    {
        if (G == ENKF_WAVE) wave_lds_fence();
        else __syncthreads();
    }
};

// a ROWS x COLS matrix in LDS from an r x c one in global memory (NULL: padding only); the caller synchronises
template <int ROWS, int COLS, int G>
__device__ __forceinline__ void enkf_group_fill(double *dst, const double *__restrict__ src, int r, int c, double diag_pad)
{
    for (unsigned k = EnkfGroup<G>::lid(); k < (unsigned)(ROWS * COLS); k += G) {
        const int a = (int)k / COLS, b = (int)k % COLS;
        dst[k] = (src != nullptr && a < r && b < c) ? src[a * c + b] : ((a == b) ? diag_pad : 0.0);
    }
}

// the group's sums into its ONE slab (LDS), by the tree of fk_enkf_dev.hpp; the caller synchronises
template <int A, int G>
__device__ __forceinline__ void enkf_group_sum(double (&acc)[A], double *red, double *slab)
{
    if constexpr (G == ENKF_WAVE) enkf_wave_sum<A>(acc, slab);
    else enkf_block_sum<A>(acc, red, slab);
}

// element e of the total over that one slab, as the finalize of enkf_kernels.hip forms it: run 0 is 0.0 + slab, the other
// fifteen runs are empty, and enkf_total adds them in index order
__device__ __forceinline__ double enkf_one_slab_total(const double *slab, int e)
{
    double runs[ENKF_GROUPS];
    FK_UNROLL for (int g = 0; g < ENKF_GROUPS; ++g) runs[g] = enkf_run_sum(slab, 1, e, g);
    return enkf_total(runs, 1, 0);
}

__device__ __forceinline__ bool enkf_finite(double v) { return fabs(v) <= 1.79769313486231570815e+308; }

// ---- predict -----------------------------------------------------------------------------------------------------------
template <int NX, int G>
struct EnkfBankPredictLds {
    using Acc = EnkfPredictAcc<NX>;
    double F[NX * NX], fac[NX * NX], x[NX], piv[NX], slab[Acc::SIZE], tot[Acc::SIZE];
    double red[G == ENKF_WAVE ? 1 : 4 * Acc::SIZE];
    int st;
};

template <int NX, int LAYOUT, bool EXACT, int G>
__device__ __forceinline__ void enkf_bank_predict_body(const EnkfBankArgs &a)
{
    using Grp = EnkfGroup<G>;
    using Acc = EnkfPredictAcc<NX>;
    __shared__ EnkfBankPredictLds<NX, G> s_all[Grp::PER_BLOCK];
    const long b = (long)blockIdx.x * Grp::PER_BLOCK + Grp::sub();
    if (b >= a.B) return;                                     // (a whole wave of the one-wave route; never the other route)
    EnkfBankPredictLds<NX, G> &L = s_all[Grp::sub()];
    const int lid = (int)Grp::lid();
    const int n = EXACT ? NX : a.n;
    const long N = a.N, tk = a.per_track ? b : 0;
    const double *gF = a.F != nullptr ? a.F + tk * n * n : nullptr, *gfac = a.factor != nullptr ? a.factor + tk * n * n : nullptr;
    double *gx = a.x + b * n, *gP = a.P + b * n * n, *sig = a.sigmas + b * n * N;
    const double *noise = a.noise + b * n * N;

    enkf_group_fill<NX, NX, G>(L.F, gF, n, n, 1.0);
    enkf_group_fill<NX, NX, G>(L.fac, gfac, n, n, 0.0);
    if (lid < NX) L.x[lid] = lid < n ? gx[lid] : 0.0;
    if (lid == 0) L.st = 0;
    Grp::sync();
    // the pivot: F x, or x
    if (lid < NX) {
        double p = L.x[lid];
        if (gF != nullptr) {
            p = L.F[lid * NX] * L.x[0];
            for (int j = 1; j < NX; ++j) p = fma(L.F[lid * NX + j], L.x[j], p);
        }
        L.piv[lid] = p;
    }
    Grp::sync();
    const double *F = gF != nullptr ? L.F : nullptr, *fac = gfac != nullptr ? L.fac : nullptr;
    double acc[Acc::SIZE];
    FK_UNROLL for (int e = 0; e < Acc::SIZE; ++e) acc[e] = 0.0;
    for (int j = 0; j < Grp::PER_LANE; ++j) {
        const long i = (long)j * G + lid;
        if (i < N) {
            double s[NX], w[NX], e[NX];
            enkf_load<NX, LAYOUT, EXACT>(s, sig, i, N, n);
            enkf_load<NX, LAYOUT, EXACT>(w, noise, i, N, n);
            enkf_draw<NX>(w, fac, e);
            enkf_predict_member<NX>(s, e, F, L.piv, acc);
            enkf_store<NX, LAYOUT, EXACT>(s, sig, i, N, n);
        }
    }
    enkf_group_sum<Acc::SIZE, G>(acc, L.red, L.slab);
    Grp::sync();
    for (int e = lid; e < Acc::SIZE; e += G) L.tot[e] = enkf_one_slab_total(L.slab, e);
    Grp::sync();
    // x = pivot + mean d;  P = sum (d - mean d)(d - mean d)' / (N - 1)   (:285-286)
    bool finite = true;
    for (int t = lid; t < n; t += G) {
        const double v = enkf_mean(L.piv[t], L.tot[t], N);
        gx[t] = v;
        finite = finite && enkf_finite(v);
    }
    for (int t = lid; t < n * n; t += G) {
        const int i = t / n, j = t % n, hi = i > j ? i : j, lo = i > j ? j : i;
        const double v = enkf_cov(L.tot[Acc::OFF_DD + enkf_tri(hi, lo)], L.tot[hi], L.tot[lo], N);
        gP[t] = v;
        finite = finite && enkf_finite(v);
    }
    if (!finite) atomicOr(&L.st, (int)ST_NONFINITE);
    Grp::sync();
    if (lid == 0 && a.status != nullptr) a.status[b] = L.st;
}

// ---- update ------------------------------------------------------------------------------------------------------------
template <int NX, int NZ, int G>
struct EnkfBankUpdateLds {
    using Acc = EnkfStatsAcc<NX, NZ>;
    double H[NZ * NX], K[NX * NZ], Kd[NX * NZ], fac[NZ * NZ], px[NX], ph[NZ], z[NZ];
    double slab[Acc::SIZE], tot[Acc::SIZE], S[ENKF_MAXZ * ENKF_MAXZ], SI[ENKF_MAXZ * ENKF_MAXZ], pxz[NX * NZ];
    double wL[ENKF_MAXZ * ENKF_MAXZ], wX[ENKF_MAXZ * ENKF_MAXZ], wd[ENKF_MAXZ], wdinv[ENKF_MAXZ];     // enkf_spd_inverse_in
    double red[G == ENKF_WAVE ? 1 : 4 * Acc::SIZE];
    int st;
};

template <int NX, int NZ, int LAYOUT, bool EXACT, int G>
__device__ __forceinline__ void enkf_bank_update_body(const EnkfBankArgs &a)
{
    using Grp = EnkfGroup<G>;
    using Acc = EnkfStatsAcc<NX, NZ>;
    __shared__ EnkfBankUpdateLds<NX, NZ, G> s_all[Grp::PER_BLOCK];
    const long b = (long)blockIdx.x * Grp::PER_BLOCK + Grp::sub();
    if (b >= a.B) return;
    const int lid = (int)Grp::lid();
    // a masked ensemble: nothing is touched (uniform over the group: the whole wave, or the whole workgroup, leaves)
    if (a.mask != nullptr && a.mask[b] == 0) {
        if (lid == 0 && a.status != nullptr) a.status[b] = 0;
        return;
    }
    EnkfBankUpdateLds<NX, NZ, G> &L = s_all[Grp::sub()];
    const int n = EXACT ? NX : a.n, m = EXACT ? NZ : a.m;
    const long N = a.N, tk = a.per_track ? b : 0;
    const double *gH = a.H != nullptr ? a.H + tk * m * n : nullptr, *gR = a.R + tk * m * m;
    const double *gfac = a.factor != nullptr ? a.factor + tk * m * m : nullptr, *gz = a.z + b * m;
    const double *sh = a.sigmas_h != nullptr ? a.sigmas_h + b * m * N : nullptr, *noise = a.noise + b * m * N;
    double *gx = a.x + b * n, *gP = a.P + b * n * n, *sig = a.sigmas + b * n * N;

    enkf_group_fill<NZ, NX, G>(L.H, gH, m, n, 0.0);
    enkf_group_fill<NZ, NZ, G>(L.fac, gfac, m, m, 0.0);
    enkf_group_fill<NX, NZ, G>(L.K, nullptr, 0, 0, 0.0);
    if (lid < NX) L.px[lid] = lid < n ? gx[lid] : 0.0;
    if (lid < NZ) L.z[lid] = lid < m ? gz[lid] : 0.0;
    Grp::sync();
    // the pivot of h: H x, or member 0's h
    if (lid < NZ) {
        double p = 0.0;
        if (gH != nullptr) {
            p = L.H[lid * NX] * L.px[0];
            for (int j = 1; j < NX; ++j) p = fma(L.H[lid * NX + j], L.px[j], p);
        } else if (lid < m) {
            p = sh[enkf_at<LAYOUT>(0, lid, N, m)];
        }
        L.ph[lid] = p;
    }
    Grp::sync();
    // h of member i: H s in-lane, or the record of sigmas_h
    auto h_of = [&](const double (&s)[NX], long i, double (&h)[NZ]) {
        if (gH != nullptr) enkf_matvec<NZ, NX>(L.H, s, h);
        else enkf_load<NZ, LAYOUT, EXACT>(h, sh, i, N, m);
    };
    // the sums of s - x and h - pivot; the one-wave route keeps its member (s1, h1) for the apply
    double s1[NX], h1[NZ];
    {
        double acc[Acc::SIZE];
        FK_UNROLL for (int e = 0; e < Acc::SIZE; ++e) acc[e] = 0.0;
        if constexpr (G == ENKF_WAVE) {
            if (lid < N) {
                enkf_load<NX, LAYOUT, EXACT>(s1, sig, lid, N, n);
                h_of(s1, lid, h1);
                enkf_stats_member<NX, NZ>(s1, h1, L.px, L.ph, acc);
            }
        } else {
            for (int j = 0; j < Grp::PER_LANE; ++j) {
                const long i = (long)j * G + lid;
                if (i < N) {
                    double s[NX], h[NZ];
                    enkf_load<NX, LAYOUT, EXACT>(s, sig, i, N, n);
                    h_of(s, i, h);
                    enkf_stats_member<NX, NZ>(s, h, L.px, L.ph, acc);
                }
            }
        }
        enkf_group_sum<Acc::SIZE, G>(acc, L.red, L.slab);
    }
    Grp::sync();
    for (int e = lid; e < Acc::SIZE; e += G) L.tot[e] = enkf_one_slab_total(L.slab, e);
    Grp::sync();
    // S = sum (h - z_mean)(h - z_mean)' / (N - 1) + R;  P_xz = sum (s - x)(h - z_mean)' / (N - 1)   (:253-259)
    double *oS = a.S != nullptr ? a.S + b * m * m : nullptr, *oSI = a.SI != nullptr ? a.SI + b * m * m : nullptr;
    double *oK = a.K != nullptr ? a.K + b * n * m : nullptr;
    for (int t = lid; t < m * m; t += G) {
        const int r = t / m, c = t % m, hi = r > c ? r : c, lo = r > c ? c : r;
        const double v = enkf_cov(L.tot[Acc::OFF_HH + enkf_tri(hi, lo)], L.tot[Acc::OFF_H + hi], L.tot[Acc::OFF_H + lo], N) + gR[hi * m + lo];
        L.S[t] = v;
        if (oS) oS[t] = v;
    }
    for (int t = lid; t < n * m; t += G) {
        const int i = t / m, c = t % m;
        L.pxz[t] = enkf_cov(L.tot[Acc::OFF_SH + i * NZ + c], L.tot[i], L.tot[Acc::OFF_H + c], N);
    }
    Grp::sync();
    if (lid == 0) L.st = enkf_spd_inverse_in(L.S, m, L.SI, L.wL, L.wd, L.wdinv, L.wX);
    Grp::sync();
    bool finite = true;
    for (int t = lid; t < m * m; t += G)
        if (oSI) oSI[t] = L.SI[t];
    // K = P_xz SI: dense (stride m) for K S K' and the caller, padded (stride NZ) for the members
    for (int t = lid; t < n * m; t += G) {
        const double v = enkf_gain_entry(L.pxz, L.SI, m, t / m, t % m);
        L.Kd[t] = v;
        L.K[(t / m) * NZ + t % m] = v;
        if (oK) oK[t] = v;
        finite = finite && enkf_finite(v);
    }
    Grp::sync();
    // P -= K S K'   (:268: the stored P)
    for (int t = lid; t < n * n; t += G) {
        const double v = gP[t] - enkf_ksk_entry(L.Kd, L.S, m, t / n, t % n);
        gP[t] = v;
        finite = finite && enkf_finite(v);
    }
    // the members: s += K (z + e - h); the sums of s - x
    const double *fac = gfac != nullptr ? L.fac : nullptr;
    {
        double acc[NX];
        FK_UNROLL for (int e = 0; e < NX; ++e) acc[e] = 0.0;
        if constexpr (G == ENKF_WAVE) {
            if (lid < N) {
                double w[NZ], e[NZ];
                enkf_load<NZ, LAYOUT, EXACT>(w, noise, lid, N, m);
                enkf_draw<NZ>(w, fac, e);
                enkf_apply_member<NX, NZ>(s1, h1, e, L.z, L.K, L.px, acc);
                enkf_store<NX, LAYOUT, EXACT>(s1, sig, lid, N, n);
            }
        } else {
            for (int j = 0; j < Grp::PER_LANE; ++j) {
                const long i = (long)j * G + lid;
                if (i < N) {
                    double s[NX], h[NZ], w[NZ], e[NZ];
                    enkf_load<NX, LAYOUT, EXACT>(s, sig, i, N, n);
                    h_of(s, i, h);
                    enkf_load<NZ, LAYOUT, EXACT>(w, noise, i, N, m);
                    enkf_draw<NZ>(w, fac, e);
                    enkf_apply_member<NX, NZ>(s, h, e, L.z, L.K, L.px, acc);
                    enkf_store<NX, LAYOUT, EXACT>(s, sig, i, N, n);
                }
            }
        }
        enkf_group_sum<NX, G>(acc, L.red, L.slab);
    }
    Grp::sync();
    for (int e = lid; e < NX; e += G) L.tot[e] = enkf_one_slab_total(L.slab, e);
    Grp::sync();
    // x = x + mean (s - x)   (:267)
    for (int t = lid; t < n; t += G) {
        const double v = enkf_mean(L.px[t], L.tot[t], N);
        gx[t] = v;
        finite = finite && enkf_finite(v);
    }
    if (!finite) atomicOr(&L.st, (int)ST_NONFINITE);
    Grp::sync();
    if (lid == 0 && a.status != nullptr) a.status[b] = L.st;
}

template <int NX, int NZ, int LAYOUT, bool EXACT, int G>
__global__ void __launch_bounds__(ENKF_BLOCK) enkf_bank_predict_kernel(const EnkfBankArgs a)
{
    enkf_bank_predict_body<NX, LAYOUT, EXACT, G>(a);
}
template <int NX, int NZ, int LAYOUT, bool EXACT, int G>
__global__ void __launch_bounds__(ENKF_BLOCK) enkf_bank_update_kernel(const EnkfBankArgs a)
{
    enkf_bank_update_body<NX, NZ, LAYOUT, EXACT, G>(a);
}

// the route by N, the kernel by the call and the record layout
template <int NX, int NZ, bool EXACT>
static int enkf_bank_launch(const EnkfBankArgs &a, int layout, hipStream_t stream)
{
    const bool soa = layout == LAYOUT_SOA, wave = a.N <= ENKF_WAVE;
    const long per = wave ? ENKF_BLOCK / ENKF_WAVE : 1;
    const dim3 grid((unsigned)((a.B + per - 1) / per)), block(ENKF_BLOCK);
    void (*k)(const EnkfBankArgs) = nullptr;
    if (!a.update) {
        if (wave) k = soa ? enkf_bank_predict_kernel<NX, NZ, LAYOUT_SOA, EXACT, ENKF_WAVE> : enkf_bank_predict_kernel<NX, NZ, LAYOUT_AOS, EXACT, ENKF_WAVE>;
        else k = soa ? enkf_bank_predict_kernel<NX, NZ, LAYOUT_SOA, EXACT, ENKF_BLOCK> : enkf_bank_predict_kernel<NX, NZ, LAYOUT_AOS, EXACT, ENKF_BLOCK>;
    } else {
        if (wave) k = soa ? enkf_bank_update_kernel<NX, NZ, LAYOUT_SOA, EXACT, ENKF_WAVE> : enkf_bank_update_kernel<NX, NZ, LAYOUT_AOS, EXACT, ENKF_WAVE>;
        else k = soa ? enkf_bank_update_kernel<NX, NZ, LAYOUT_SOA, EXACT, ENKF_BLOCK> : enkf_bank_update_kernel<NX, NZ, LAYOUT_AOS, EXACT, ENKF_BLOCK>;
    }
    hipLaunchKernelGGL(k, grid, block, 0, stream, a);
    return check_launch(a.update ? "enkf_bank_update_kernel" : "enkf_bank_predict_kernel");
}

#if !(defined(FK_ENKF_GENERAL) && FK_ENKF_GENERAL)

#define FK_CAT_(a, b, c) a##b##_##c
#define FK_CAT(a, b, c) FK_CAT_(a, b, c)

int FK_CAT(launch_enkf_bank_fast_, FK_NX, FK_NZ)(const EnkfBankArgs &a, int layout, hipStream_t stream)
{
    return enkf_bank_launch<FK_NX, FK_NZ, true>(a, layout, stream);
}

#else  // FK_ENKF_GENERAL

int launch_enkf_bank_general(const EnkfBankArgs &a, int layout, hipStream_t stream)
{
    return enkf_bank_launch<ENKF_MAXX, ENKF_MAXZ, false>(a, layout, stream);
}

#endif

}  // namespace fk
