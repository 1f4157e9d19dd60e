// enkf_kernels.hip -- the ensemble Kalman filter (filterpy/kalman/ensemble_kalman_filter.py:218-290) for ONE ensemble of N
// members (gfx950).
//
// Unlike every other family of the library the parallelism is over the MEMBERS of one filter, and the result is a reduction
// over all of them.  A pass kernel streams the ensemble: workgroup c owns members [c ENKF_CHUNK, (c + 1) ENKF_CHUNK), lane l
// members l, l + 256, ... of them (element-major records: 512 contiguous bytes per wave and load).  Each lane keeps its sums
// in registers, the workgroup adds its 256 lanes in a fixed tree (butterfly inside a wave, the four waves in order through
// LDS) and writes ONE slab of partial sums to the workspace with plain stores.  enkf_finalize_kernel -- one workgroup, the
// next launch -- adds the slabs in a fixed order and does the dense algebra (fk_enkf.hpp).  No atomics, no arrival order, no
// waiting inside a launch: the launch boundary is the synchronisation, and the same call gives the same bytes.
//
//   predict      enkf_predict_kernel  (s <- F s + e, sums of s - pivot)        -> finalize: x, P
//   update       enkf_stats_kernel    (sums of s - x, h - pivot)               -> finalize: S, SI, K, P -= K S K'
//                enkf_apply_kernel    (s += K (z + e - h), sums of s - x)      -> finalize: x
// The fused linear update reads the ensemble twice (h = H s is formed in-lane both times), the noise once, and writes the
// ensemble once; the fused linear predict is one read of members and noise and one write.
//
// Two builds of the pass kernels:
//   fast      exact (dim_x, dim_z), every loop unrolled, the sums in VGPRs (fk_dims_enkf.def; -DFK_NX/-DFK_NZ)
//   general   everything else up to (16, 8): ONE padded instantiation with rolled loops, the sums in scratch memory
//             (-DFK_ENKF_GENERAL=1).  A correctness path.  The padding (zeros in members, draws, pivots, H, K and the factor,
//             identity in F) adds exact zeros only.  The finalize kernel is built with it and serves both.
#if defined(FK_ENKF_GENERAL) && FK_ENKF_GENERAL
#define FK_ROLLED 1
#endif
#include "fk_device.hpp"
#include "fk_enkf.hpp"
#include "fk_enkf_dev.hpp"

namespace fk {

static_assert(ENKF_BLOCK == BLOCK, "four waves per workgroup");

// a ROWS x COLS matrix in LDS from an r x c one in global memory (NULL: padding only); the caller synchronises
template <int ROWS, int COLS>
__device__ __forceinline__ void enkf_fill(double *dst, const double *__restrict__ src, int r, int c, double diag_pad)
{
    for (unsigned k = threadIdx.x; k < (unsigned)(ROWS * COLS); k += ENKF_BLOCK) {
        const int a = (int)k / COLS, b = (int)k % COLS;
        dst[k] = (src != nullptr && a < r && b < c) ? src[a * c + b] : ((a == b) ? diag_pad : 0.0);
    }
}

// ---- predict -----------------------------------------------------------------------------------------------------------
template <int NX, int LAYOUT, bool EXACT>
__device__ __forceinline__ void enkf_predict_body(const EnkfArgs &a)
{
    using Acc = EnkfPredictAcc<NX>;
    __shared__ double s_F[NX * NX], s_fac[NX * NX], s_x[NX], s_piv[NX], s_red[4 * Acc::SIZE];
    const int n = EXACT ? NX : a.n;
    enkf_fill<NX, NX>(s_F, a.F, n, n, 1.0);
    enkf_fill<NX, NX>(s_fac, a.factor, n, n, 0.0);
    if (threadIdx.x < NX) s_x[threadIdx.x] = (int)threadIdx.x < n ? a.x[threadIdx.x] : 0.0;
    __syncthreads();
    // the pivot: F x, or x
    if (threadIdx.x < NX) {
        double p = s_x[threadIdx.x];
        if (a.F != nullptr) {
            p = s_F[threadIdx.x * NX] * s_x[0];
            for (int j = 1; j < NX; ++j) p = fma(s_F[threadIdx.x * NX + j], s_x[j], p);
        }
        s_piv[threadIdx.x] = p;
        if (blockIdx.x == 0) a.ws[ENKF_WS_PIVX + threadIdx.x] = p;
    }
    __syncthreads();
    const double *F = a.F != nullptr ? s_F : nullptr, *fac = a.factor != nullptr ? s_fac : nullptr;
    double acc[Acc::SIZE];
    FK_UNROLL for (int e = 0; e < Acc::SIZE; ++e) acc[e] = 0.0;
    const long c0 = (long)blockIdx.x * ENKF_CHUNK;
    for (int j = 0; j < ENKF_PER_LANE; ++j) {
        const long i = c0 + (long)j * ENKF_BLOCK + threadIdx.x;
        if (i < a.N) {
            double s[NX], w[NX], e[NX];
            enkf_load<NX, LAYOUT, EXACT>(s, a.sigmas, i, a.N, n);
            enkf_load<NX, LAYOUT, EXACT>(w, a.noise, i, a.N, n);
            enkf_draw<NX>(w, fac, e);
            enkf_predict_member<NX>(s, e, F, s_piv, acc);
            enkf_store<NX, LAYOUT, EXACT>(s, a.sigmas, i, a.N, n);
        }
    }
    enkf_block_sum<Acc::SIZE>(acc, s_red, a.ws + ENKF_WS_SLABS + (long)blockIdx.x * ENKF_SLAB);
}

// ---- update: the sums ------------------------------------------------------------------------------------------------------
// h of member i: H s in-lane, or the record of sigmas_h
template <int NX, int NZ, int LAYOUT, bool EXACT>
__device__ __forceinline__ void enkf_h(const EnkfArgs &a, const double *s_H, const double (&s)[NX], long i, int m, double (&h)[NZ])
{
    if (a.H != nullptr) enkf_matvec<NZ, NX>(s_H, s, h);
    else enkf_load<NZ, LAYOUT, EXACT>(h, a.sigmas_h, i, a.N, m);
}

template <int NX, int NZ, int LAYOUT, bool EXACT>
__device__ __forceinline__ void enkf_stats_body(const EnkfArgs &a)
{
    using Acc = EnkfStatsAcc<NX, NZ>;
    __shared__ double s_H[NZ * NX], s_px[NX], s_ph[NZ], s_red[4 * Acc::SIZE];
    const int n = EXACT ? NX : a.n, m = EXACT ? NZ : a.m;
    enkf_fill<NZ, NX>(s_H, a.H, m, n, 0.0);
    if (threadIdx.x < NX) {
        const double p = (int)threadIdx.x < n ? a.x[threadIdx.x] : 0.0;
        s_px[threadIdx.x] = p;
        if (blockIdx.x == 0) a.ws[ENKF_WS_PIVX + threadIdx.x] = p;
    }
    __syncthreads();
    // the pivot of h: H x, or member 0's h
    if (threadIdx.x < NZ) {
        double p = 0.0;
        if (a.H != nullptr) {
            p = s_H[threadIdx.x * NX] * s_px[0];
            for (int j = 1; j < NX; ++j) p = fma(s_H[threadIdx.x * NX + j], s_px[j], p);
        } else if ((int)threadIdx.x < m) {
            p = a.sigmas_h[enkf_at<LAYOUT>(0, (int)threadIdx.x, a.N, m)];
        }
        s_ph[threadIdx.x] = p;
        if (blockIdx.x == 0) a.ws[ENKF_WS_PIVH + threadIdx.x] = p;
    }
    __syncthreads();
    double acc[Acc::SIZE];
    FK_UNROLL for (int e = 0; e < Acc::SIZE; ++e) acc[e] = 0.0;
    const long c0 = (long)blockIdx.x * ENKF_CHUNK;
    for (int j = 0; j < ENKF_PER_LANE; ++j) {
        const long i = c0 + (long)j * ENKF_BLOCK + threadIdx.x;
        if (i < a.N) {
            double s[NX], h[NZ];
            enkf_load<NX, LAYOUT, EXACT>(s, a.sigmas, i, a.N, n);
            enkf_h<NX, NZ, LAYOUT, EXACT>(a, s_H, s, i, m, h);
            enkf_stats_member<NX, NZ>(s, h, s_px, s_ph, acc);
        }
    }
    enkf_block_sum<Acc::SIZE>(acc, s_red, a.ws + ENKF_WS_SLABS + (long)blockIdx.x * ENKF_SLAB);
}

// ---- update: the members -----------------------------------------------------------------------------------------------------
template <int NX, int NZ, int LAYOUT, bool EXACT>
__device__ __forceinline__ void enkf_apply_body(const EnkfArgs &a)
{
    __shared__ double s_H[NZ * NX], s_K[NX * NZ], s_fac[NZ * NZ], s_px[NX], s_z[NZ], s_red[4 * NX];
    const int n = EXACT ? NX : a.n, m = EXACT ? NZ : a.m;
    enkf_fill<NZ, NX>(s_H, a.H, m, n, 0.0);
    enkf_fill<NX, NZ>(s_K, a.ws + ENKF_WS_K, n, m, 0.0);
    enkf_fill<NZ, NZ>(s_fac, a.factor, m, m, 0.0);
    if (threadIdx.x < NX) s_px[threadIdx.x] = (int)threadIdx.x < n ? a.ws[ENKF_WS_PIVX + threadIdx.x] : 0.0;
    if (threadIdx.x < NZ) s_z[threadIdx.x] = (int)threadIdx.x < m ? a.z[threadIdx.x] : 0.0;
    __syncthreads();
    const double *fac = a.factor != nullptr ? s_fac : nullptr;
    double acc[NX];
    FK_UNROLL for (int e = 0; e < NX; ++e) acc[e] = 0.0;
    const long c0 = (long)blockIdx.x * ENKF_CHUNK;
    for (int j = 0; j < ENKF_PER_LANE; ++j) {
        const long i = c0 + (long)j * ENKF_BLOCK + threadIdx.x;
        if (i < a.N) {
            double s[NX], h[NZ], w[NZ], e[NZ];
            enkf_load<NX, LAYOUT, EXACT>(s, a.sigmas, i, a.N, n);
            enkf_h<NX, NZ, LAYOUT, EXACT>(a, s_H, s, i, m, h);
            enkf_load<NZ, LAYOUT, EXACT>(w, a.noise, i, a.N, m);
            enkf_draw<NZ>(w, fac, e);
            enkf_apply_member<NX, NZ>(s, h, e, s_z, s_K, s_px, acc);
            enkf_store<NX, LAYOUT, EXACT>(s, a.sigmas, i, a.N, n);
        }
    }
    enkf_block_sum<NX>(acc, s_red, a.ws + ENKF_WS_SLABS + (long)blockIdx.x * ENKF_SLAB);
}

template <int NX, int NZ, int LAYOUT, bool EXACT>
__global__ void __launch_bounds__(ENKF_BLOCK) enkf_predict_kernel(const EnkfArgs a) { enkf_predict_body<NX, LAYOUT, EXACT>(a); }
template <int NX, int NZ, int LAYOUT, bool EXACT>
__global__ void __launch_bounds__(ENKF_BLOCK) enkf_stats_kernel(const EnkfArgs a) { enkf_stats_body<NX, NZ, LAYOUT, EXACT>(a); }
template <int NX, int NZ, int LAYOUT, bool EXACT>
__global__ void __launch_bounds__(ENKF_BLOCK) enkf_apply_kernel(const EnkfArgs a) { enkf_apply_body<NX, NZ, LAYOUT, EXACT>(a); }

// one workgroup per chunk; the phase and the record layout pick the kernel
template <int NX, int NZ, bool EXACT>
static int enkf_launch_pass(const EnkfArgs &a, int layout, hipStream_t stream)
{
    const dim3 grid((unsigned)enkf_slabs(a.N)), block(ENKF_BLOCK);
    const bool soa = layout == LAYOUT_SOA;
    void (*k)(const EnkfArgs) = nullptr;
    const char *name = "enkf_predict_kernel";
    if (a.phase == ENKF_PREDICT) {
        k = soa ? enkf_predict_kernel<NX, NZ, LAYOUT_SOA, EXACT> : enkf_predict_kernel<NX, NZ, LAYOUT_AOS, EXACT>;
    } else if (a.phase == ENKF_STATS) {
        k = soa ? enkf_stats_kernel<NX, NZ, LAYOUT_SOA, EXACT> : enkf_stats_kernel<NX, NZ, LAYOUT_AOS, EXACT>;
        name = "enkf_stats_kernel";
    } else {
        k = soa ? enkf_apply_kernel<NX, NZ, LAYOUT_SOA, EXACT> : enkf_apply_kernel<NX, NZ, LAYOUT_AOS, EXACT>;
        name = "enkf_apply_kernel";
    }
    EnkfArgs b = a;
    b.ax = NX; b.az = NZ;
    hipLaunchKernelGGL(k, grid, block, 0, stream, b);
    return check_launch(name);
}

#if !(defined(FK_ENKF_GENERAL) && FK_ENKF_GENERAL)

#define FK_CAT_(a, b, c) a##b##_##c
#define FK_CAT(a, b, c) FK_CAT_(a, b, c)

int FK_CAT(launch_enkf_fast_, FK_NX, FK_NZ)(const EnkfArgs &a, int layout, hipStream_t stream)
{
    return enkf_launch_pass<FK_NX, FK_NZ, true>(a, layout, stream);
}

#else  // FK_ENKF_GENERAL

int launch_enkf_general(const EnkfArgs &a, int layout, hipStream_t stream)
{
    return enkf_launch_pass<ENKF_MAXX, ENKF_MAXZ, false>(a, layout, stream);
}

// ---- the finalize ------------------------------------------------------------------------------------------------------
constexpr int ENKF_FIN_BLOCK = 64 * ENKF_GROUPS;           // run g on wave g, 64 elements side by side

__global__ void __launch_bounds__(ENKF_FIN_BLOCK) enkf_finalize_kernel(const EnkfArgs a)
{
    __shared__ double s_runs[ENKF_GROUPS * ENKF_SLAB], s_tot[ENKF_SLAB];
    __shared__ double s_S[ENKF_MAXZ * ENKF_MAXZ], s_SI[ENKF_MAXZ * ENKF_MAXZ], s_K[ENKF_MAXX * ENKF_MAXZ];
    __shared__ double s_pxz[ENKF_MAXX * ENKF_MAXZ];
    __shared__ int s_st;
    const int n = a.n, m = a.m, ax = a.ax, az = a.az;
    const int tid = (int)threadIdx.x;
    const long N = a.N, nslabs = enkf_slabs(N);
    const int A = a.phase == ENKF_FIN_PREDICT ? ax + ax * (ax + 1) / 2
                : a.phase == ENKF_FIN_UPDATE ? ax + az + az * (az + 1) / 2 + ax * az : ax;
    const double *slabs = a.ws + ENKF_WS_SLABS;
    for (int e = tid & 63; e < A; e += 64) s_runs[(tid >> 6) * ENKF_SLAB + e] = enkf_run_sum(slabs, nslabs, e, tid >> 6);
    __syncthreads();
    for (int e = tid; e < A; e += ENKF_FIN_BLOCK) s_tot[e] = enkf_total(s_runs, ENKF_SLAB, e);
    if (tid == 0) s_st = 0;
    __syncthreads();
    const double *piv = a.ws + ENKF_WS_PIVX;
    bool finite = true;
    if (a.phase == ENKF_FIN_PREDICT) {
        // x = pivot + mean d;  P = sum (d - mean d)(d - mean d)' / (N - 1)   (:285-286)
        if (tid < n) {
            const double v = enkf_mean(piv[tid], s_tot[tid], N);
            a.x[tid] = v;
            finite = fabs(v) <= 1.79769313486231570815e+308;
        }
        if (tid < n * n) {
            const int i = tid / n, j = tid % n, hi = i > j ? i : j, lo = i > j ? j : i;
            const double v = enkf_cov(s_tot[ax + enkf_tri(hi, lo)], s_tot[hi], s_tot[lo], N);
            a.P[tid] = v;
            finite = finite && fabs(v) <= 1.79769313486231570815e+308;
        }
    } else if (a.phase == ENKF_FIN_UPDATE) {
        const int off_h = ax, off_hh = ax + az, off_sh = off_hh + az * (az + 1) / 2;
        // S = sum (h - z_mean)(h - z_mean)' / (N - 1) + R;  P_xz = sum (s - x)(h - z_mean)' / (N - 1)   (:253-259)
        if (tid < m * m) {
            const int r = tid / m, c = tid % m, hi = r > c ? r : c, lo = r > c ? c : r;
            const double v = enkf_cov(s_tot[off_hh + enkf_tri(hi, lo)], s_tot[off_h + hi], s_tot[off_h + lo], N) + a.R[hi * m + lo];
            s_S[tid] = v;
            if (a.S) a.S[tid] = v;
        }
        if (tid < n * m) {
            const int i = tid / m, c = tid % m;
            s_pxz[tid] = enkf_cov(s_tot[off_sh + i * az + c], s_tot[i], s_tot[off_h + c], N);
        }
        __syncthreads();
        if (tid == 0) s_st = enkf_spd_inverse(s_S, m, s_SI);
        __syncthreads();
        if (tid < m * m && a.SI) a.SI[tid] = s_SI[tid];
        if (tid < n * m) {
            const double v = enkf_gain_entry(s_pxz, s_SI, m, tid / m, tid % m);
            s_K[tid] = v;
            a.ws[ENKF_WS_K + tid] = v;
            if (a.K) a.K[tid] = v;
            finite = fabs(v) <= 1.79769313486231570815e+308;
        }
        __syncthreads();
        // P -= K S K'   (:268: the stored P)
        if (tid < n * n) {
            const double v = a.P[tid] - enkf_ksk_entry(s_K, s_S, m, tid / n, tid % n);
            a.P[tid] = v;
            finite = finite && fabs(v) <= 1.79769313486231570815e+308;
        }
    } else {
        // x = x + mean (s - x)   (:267)
        if (tid < n) {
            const double v = enkf_mean(piv[tid], s_tot[tid], N);
            a.x[tid] = v;
            finite = fabs(v) <= 1.79769313486231570815e+308;
        }
    }
    if (!finite) atomicOr(&s_st, (int)ST_NONFINITE);
    __syncthreads();
    // one status word: the update's two finalizes share it (the second adds to what the first left)
    if (tid == 0 && a.status) *a.status = (a.phase == ENKF_FIN_APPLY ? *a.status : 0) | s_st;
}

int launch_enkf_finalize(const EnkfArgs &a, hipStream_t stream)
{
    hipLaunchKernelGGL(enkf_finalize_kernel, dim3(1), dim3(ENKF_FIN_BLOCK), 0, stream, a);
    return check_launch("enkf_finalize_kernel");
}

#endif

}  // namespace fk
