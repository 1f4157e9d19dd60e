// fk_enkf_dev.hpp -- what the two kernel files of the ensemble Kalman filter share on the device: how a member's record is
// addressed, loaded and stored, and the fixed tree by which the lanes of a workgroup (enkf_kernels.hip, the 256-lane route of
// enkf_bank.hip) or of one wave (the one-wave route of enkf_bank.hip) add their partial sums into ONE slab.  The tree is stated
// here once: the bank is bit-identical to the single-ensemble kernels because both run this text.
#pragma once

#include "fk_device.hpp"
#include "fk_enkf.hpp"

namespace fk {

// element e of member i's record: [d][N] element-major, [N][d] NumPy order (64-bit indices: no 4 GiB limit on the ensemble)
template <int LAYOUT>
__device__ __forceinline__ long enkf_at(long i, int e, long N, int d)
{
    return LAYOUT == LAYOUT_SOA ? (long)e * N + i : i * d + e;
}

template <int D, int LAYOUT, bool EXACT>
__device__ __forceinline__ void enkf_load(double (&v)[D], const double *__restrict__ base, long i, long N, int d)
{
    FK_UNROLL for (int e = 0; e < D; ++e) v[e] = (EXACT || e < d) ? base[enkf_at<LAYOUT>(i, e, N, EXACT ? D : d)] : 0.0;
}

template <int D, int LAYOUT, bool EXACT>
__device__ __forceinline__ void enkf_store(const double (&v)[D], double *__restrict__ base, long i, long N, int d)
{
    FK_UNROLL for (int e = 0; e < D; ++e)
        if (EXACT || e < d) base[enkf_at<LAYOUT>(i, e, N, EXACT ? D : d)] = v[e];
}

// the four waves of a workgroup in index order; a wave that is not there is 0.0
__device__ __forceinline__ double enkf_waves_sum(double w0, double w1, double w2, double w3) { return ((w0 + w1) + w2) + w3; }

// The workgroup's sum of every accumulator, in a fixed tree, into its slab: a butterfly over the 64 lanes of a wave (every
// lane ends with the wave's sum), then the four waves in index order.  red: [4][A] doubles of LDS.
template <int A>
__device__ __forceinline__ void enkf_block_sum(double (&acc)[A], double *red, double *__restrict__ slab)
{
    const unsigned lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    FK_UNROLL for (int e = 0; e < A; ++e) {
        double v = acc[e];
        FK_UNROLL for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
        if (lane == 0) red[wave * A + e] = v;
    }
    __syncthreads();
    for (unsigned e = threadIdx.x; e < (unsigned)A; e += ENKF_BLOCK)
        slab[e] = enkf_waves_sum(red[e], red[A + e], red[2 * A + e], red[3 * A + e]);
}

// ... the same tree for an ensemble that ONE wave holds (N <= 64, a lane without a member carries zeros): the butterfly, then
// the wave as wave 0 of a workgroup whose other three waves are absent.  No workgroup barrier; the caller fences the wave.
template <int A>
__device__ __forceinline__ void enkf_wave_sum(double (&acc)[A], double *slab)
{
    const unsigned lane = threadIdx.x & 63u;
    FK_UNROLL for (int e = 0; e < A; ++e) {
        double v = acc[e];
        FK_UNROLL for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
        if (lane == 0) slab[e] = enkf_waves_sum(v, 0.0, 0.0, 0.0);
    }
}

}  // namespace fk
