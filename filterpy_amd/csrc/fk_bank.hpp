// fk_bank.hpp -- the scaffold of the kernels that run ONE track per lane, the whole time loop inside the kernel, on a model
// shared by every track and staged once in LDS (gfx950): the square-root filter (srkf_kernels.hip), the information filter
// (info_kernels.hip) and the fixed-lag smoother (fls_kernels.hip).
//
// Held here, once: B u of a step, the store of a history record (wave transpose or lane store), the F | Q | H | R model
// fill and the layout-switching launcher.  Everything on the device side is __forceinline__ and every shape, layout and path
// choice a template parameter: all 102 kernels of the three families disassemble to what they were when each file carried
// its own copy of this text (docs/MEASUREMENTS.md).
//
// Not held here: the lane's time loop of the two predict / update filters (srkf_lane, info_lane) and the kernel bodies.  A
// driver generic over a per-filter policy (state, predict, update, by-products) was built and compiled to other code in every
// form tried -- the state as members of the policy or as arrays passed by reference, the time update as a function or
// written out, the by-products declared in the policy or in the driver: between 2 and 35 VGPRs more or fewer on 16 to 34 of
// the 34 kernels of a family (docs/MEASUREMENTS.md).  The register allocation of these fully unrolled kernels follows the
// order in which the inlined code declares its arrays; the bar for this file is the parent's ISA, so the loops stay where
// they were until a kernel change re-measures them anyway.
#pragma once

#include "fk_device.hpp"

namespace fk {

// B u of one step: B [n][nu] shared, u the lane's record in record block t of `u` ([N][nu] each; nothing is read when
// nu == 0).  The filters pass the step's own block and t = 0, the smoother its whole array and the step: where the block's
// address is formed is where each kernel's code always formed it, and moving it costs registers in some instantiation.
template <int NX, int LAYOUT, class Args>
__device__ __forceinline__ void bank_control(const Args &a, const Lane &ln, const double *u, long t, double (&bu)[NX])
{
    FK_UNROLL for (int r = 0; r < NX; ++r) bu[r] = 0.0;
    if (a.nu <= 0) return;
    const RecView<LAYOUT> uv(u + t * a.N * a.nu, ln, a.nu);
    for (int j = 0; j < a.nu; ++j) {
        const double uj = uv.load(j);
        FK_UNROLL for (int r = 0; r < NX; ++r) {
            if (r < a.n) {
                const double b = a.B[r * a.nu + j];
                bu[r] = (j == 0) ? b * uj : fma(b, uj, bu[r]);
            }
        }
    }
}

// F | Q | H | R into an LdsModel, padded to NX / NZ (identity in F and R, zeros in Q and H); one barrier
template <int NX, int NZ>
__device__ __forceinline__ void bank_fill_model(double *s_model, const double *F, const double *Q, const double *H,
                                                const double *R, int n, int m)
{
    using SM = LdsModel<NX, NZ>;
    lds_fill<NX, NX>(s_model + SM::OFF_F, F, n, n, 1.0, threadIdx.x);
    lds_fill<NX, NX>(s_model + SM::OFF_Q, Q, n, n, 0.0, threadIdx.x);
    lds_fill<NZ, NX>(s_model + SM::OFF_H, H, m, n, 0.0, threadIdx.x);
    lds_fill<NZ, NZ>(s_model + SM::OFF_R, R, m, m, 1.0, threadIdx.x);
    __syncthreads();
}

// One record per lane of the step's history block (block t of `base`, [N][E]).  WAVE (the fast kernel in NumPy order): the
// wave's 64 records leave through an LDS transpose as contiguous 16-byte stores (wave_store_aos, fk_device.hpp; every lane of
// the wave takes part -- tail lanes carry a copy of the last track and the descriptor drops their rows); otherwise lane stores.
template <int R, int C, int LAYOUT, bool EXACT, bool WAVE>
__device__ __forceinline__ void bank_put(const double (&v)[R * C], double *base, long t, const Lane &ln, int r, int c,
                                         double *tile, unsigned last_row)
{
    if constexpr (WAVE) {
        const unsigned lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
        wave_store_aos<R * C>(v, base + (t * ln.N + ln.blk0) * (R * C), wave * 64u, tile, lane, last_row);
    } else {
        store_rec<R, C, LAYOUT, EXACT>(v, base + t * ln.N * r * c, ln, r, c);
    }
}

// One workgroup per BLOCK tracks; the record layout picks the instantiation.
template <class Args>
int bank_launch(void (*soa)(Args), void (*aos)(Args), const char *name, const Args &a, int layout, hipStream_t stream)
{
    const dim3 grid((unsigned)((a.N + BLOCK - 1) / BLOCK)), block(BLOCK);
    hipLaunchKernelGGL(layout == LAYOUT_SOA ? soa : aos, grid, block, 0, stream, a);
    return check_launch(name);
}

}  // namespace fk
