// poly_kernels.hip -- the fixed-gain polynomial filters (g-h / g-h-k, fading memory, least squares) for a bank of N tracks:
// fk_poly_run.  Seven kernels, one per (order, form) of fk_poly.hpp.  Built with -ffp-contract=off (csrc/Makefile): every line
// of the step functions is single IEEE operations, the results are the reference's bits.
//
// Shape: one track per lane, the state (order + 1 doubles) in registers, the T loop inside the launch, a grid-stride loop over
// the tracks.  The job is pure streaming -- 8 bytes in and 8 (order + 1) bytes out per track-step against half a dozen
// operations -- so the kernel is built around its memory operations:
//   - ONE track per lane: a wave's load or store of one element row is 512 contiguous bytes (soa).  The project's own
//     store-width measurement has 512-byte wave stores at 0.81 of peak and 1 KiB ones at 0.78, so two
//     tracks per lane buy nothing, and they would ask 16-byte alignment of every array where the ABI promises 8.
//   - z of the coming POLY_DEPTH steps is loaded ahead of use (a ring of registers, refilled the moment an entry is consumed):
//     a wave always has POLY_DEPTH loads outstanding behind its stores, and the recurrence never waits for the load it
//     just issued.
//   - all offsets in 64 bits: T * N * 3 passes 2^31 at ordinary sizes.
//   - no LDS, no cross-lane traffic, no atomics; layout is two run-time strides (fk_poly.hpp PolyArgs), not a template
//     argument, and absent outputs are wave-uniform branches.
// One long filter (N = 1, T large) is latency-bound and stays so: evaluating the recurrence in parallel over time would
// change the bits.
#include <hip/hip_runtime.h>

#include "../../include/filterhip.h"
#include "fk_device.hpp"
#include "fk_poly.hpp"

namespace fk {

constexpr int POLY_DEPTH = 4;            // steps of z in flight per lane
constexpr int POLY_MAX_BLOCKS = 2048;    // 256 CUs x 8 workgroups of 4 waves: every wave slot at these kernels' register counts

template <int ORDER, int FORM>
__global__ __launch_bounds__(BLOCK) void poly_kernel(const PolyArgs a, const double *__restrict__ gains, const double *__restrict__ zs)
{
    constexpr int C = ORDER + 1;
    const long N = a.N, T = a.T;
    const long hist = (long)C * N;                     // doubles per history step
    const long stride = (long)gridDim.x * BLOCK;
    // wave-uniform: which outputs exist, and whether the gains come from the table
    const bool has_xs = a.xs != nullptr, has_pred = a.pred != nullptr, has_y = a.y != nullptr, has_table = gains != nullptr;
    // NumPy order at order 1: a track's history record is the pair (x, dx), 16 bytes.  Where xs is 16-byte aligned it leaves as
    // ONE store (a wave then writes 1 KiB contiguous per instruction instead of two interleaved halves); the ABI promises 8
    // bytes only, so the 8-byte form stays for every other pointer.
    const bool pair_store = ORDER == 1 && a.es == 1 && (reinterpret_cast<unsigned long long>(a.xs) & 15ull) == 0;
    for (long i = (long)blockIdx.x * BLOCK + threadIdx.x; i < N; i += stride) {
        double s[C];
        FK_UNROLL for (int e = 0; e < C; ++e) s[e] = a.x[e * a.es + i * a.ts];
        double g[3] = {a.g[0], a.g[1], a.g[2]};
        double pred, y;
        // The ring of fetched measurements.  Every fetch is UNCONDITIONAL: past the last step the pointer stands still and the
        // lane reads z[T - 1] again (a cache hit, never used).  A fetch under `if (t + POLY_DEPTH < T)` merges a loaded and
        // a kept value in one register, and the compiler then waits for the load where it was issued.
        const double *zp = zs + i;                     // z[t][i], t = min(the next step to fetch, T - 1)
        double zb[POLY_DEPTH];
        FK_UNROLL for (int j = 0; j < POLY_DEPTH; ++j) {
            zb[j] = *zp;
            zp += (j + 1 < T) ? N : 0;
        }
        long xo = i * a.ts, so = i;                    // where the lane's next history record / pred and y go
        auto step = [&](double z, long t) {
            if (has_table) {
                FK_UNROLL for (int e = 0; e < C; ++e) g[e] = gains[t * C + e];
            }
            poly_step<ORDER, FORM>(s, z, a.k, g, pred, y);
        };
        auto store = [&]() {
            if (has_xs) {
                bool done = false;
                if constexpr (ORDER == 1) {
                    if (pair_store) {                  // (xo = 2 (t N + i): even, the record is aligned with the array)
                        *reinterpret_cast<double2 *>(a.xs + xo) = make_double2(s[0], s[1]);
                        done = true;
                    }
                }
                if (!done) {
                    FK_UNROLL for (int e = 0; e < C; ++e) a.xs[xo + e * a.es] = s[e];
                }
                xo += hist;
            }
            if (has_pred) a.pred[so] = pred;
            if (has_y) a.y[so] = y;
            so += N;
        };
        // whole rounds of the ring: no exit inside, every slot is refilled (after the step has consumed it, so that the load
        // lands in the very register) POLY_DEPTH steps ahead of its use
        long t = 0;
        for (; t + POLY_DEPTH <= T; t += POLY_DEPTH) {
            FK_UNROLL for (int j = 0; j < POLY_DEPTH; ++j) {
                step(zb[j], t + j);
                zb[j] = *zp;
                zp += (t + j + POLY_DEPTH + 1 < T) ? N : 0;
                store();
            }
        }
        // the last T % POLY_DEPTH steps: their measurements are in the ring already
        FK_UNROLL for (int j = 0; j < POLY_DEPTH - 1; ++j) {
            if (t + j < T) {
                step(zb[j], t + j);
                store();
            }
        }
        FK_UNROLL for (int e = 0; e < C; ++e) a.x[e * a.es + i * a.ts] = s[e];
    }
}

template <int ORDER, int FORM>
static int launch(const PolyArgs &a, hipStream_t stream)
{
    long blocks = (a.N + BLOCK - 1) / BLOCK;
    if (blocks > POLY_MAX_BLOCKS) blocks = POLY_MAX_BLOCKS;
    hipLaunchKernelGGL((poly_kernel<ORDER, FORM>), dim3((unsigned)blocks), dim3(BLOCK), 0, stream, a, a.gains, a.z);
    return check_launch("fk_poly_run");
}

// (order, form) is one of the seven: poly_dispatch.cpp has refused everything else
int launch_poly(int order, int form, const PolyArgs &a, hipStream_t stream)
{
    switch (form * 3 + order) {
    case POLY_FORM_A * 3 + 0: return launch<0, POLY_FORM_A>(a, stream);
    case POLY_FORM_A * 3 + 1: return launch<1, POLY_FORM_A>(a, stream);
    case POLY_FORM_A * 3 + 2: return launch<2, POLY_FORM_A>(a, stream);
    case POLY_FORM_B * 3 + 1: return launch<1, POLY_FORM_B>(a, stream);
    case POLY_FORM_B * 3 + 2: return launch<2, POLY_FORM_B>(a, stream);
    case POLY_FORM_C * 3 + 1: return launch<1, POLY_FORM_C>(a, stream);
    case POLY_FORM_C * 3 + 2: return launch<2, POLY_FORM_C>(a, stream);
    }
    set_last_error("fk_poly_run: no kernel for this (order, form)");
    return FK_ERR_UNSUPPORTED;
}

}  // namespace fk
