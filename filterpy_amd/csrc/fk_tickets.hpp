// fk_tickets.hpp -- the persistent "ticket" grid of kf_ml_kernel, rts_ml_kernel (kf_ml.hip) and ukf_linear_kernel (ukf_kernels.hip):
// the plan, the host side and the device protocol, each stated once.  A call is cut into G track groups x H time chunks; the
// resident workgroups draw (group, chunk) TICKETS from an atomic counter, chunk-major.  Chunk c of a group needs chunk c - 1 of that
// group: a ticket G draws older, i.e. held by a workgroup that runs or is done -- no deadlock whatever is resident.  The state travels
// through a hand-over block of the call's scratch (agent-scope accesses), announced by the completion word ctl[1 + g] (ctl[0]: tickets).
// Same arithmetic per track: bit-identical to one launch.  Part 1 is plain C++17 and runs on the host (tests/test_hostcheck_tickets.py).
#pragma once
#include <stddef.h>
#include <stdlib.h>
#include "fk_math.hpp"

namespace fk {
// ------------------------------------------------------------------------------------------------------- 1. the plan --
enum TicketSwitch { TICKETS_UNLESS_0, TICKETS_IF_NONZERO, TICKETS_IF_1 };      // how the switch's integer value is read
// TICKET_H_THREE: three chunks from 48 steps on, T / 16 below (>= 16 steps each; at BASELINE configs[2] 3: 3.10 ms, 4: 3.15, 6: 3.22, 10: 3.29,
// one launch 3.39).  TICKET_H_FULLEST: the count in [4, T / 6] whose last round of tickets is fullest; a larger count must add 0.02 of fill.
enum TicketChunks { TICKET_H_THREE, TICKET_H_FULLEST };
struct TicketPolicy {
    const char *env;                  // the switch, read per call ...
    TicketSwitch on;                  // ... and when it says yes
    const char *env_h;                // overrides the chunk count, before the refusals
    long group;                       // tracks per group: a workgroup's
    TicketChunks chunks;
    bool cnt0_is_bank, whole_bank;    // cnt == 0 means the whole bank (RtsArgs); takes whole-bank calls only
    long min_T;
    bool more_than_cus, two_steps, h_within_T;   // refuses G <= CUs (else G <= slots = 2 x CUs); T / H < 2; H > T.  Always: G > 2^24, H < 2
    bool grid_to_tickets;             // the grid is min(G H, slots), else slots
    long ws_doubles;                  // hand-over doubles per track of the bank (N, not cnt)
};
// kf_ml_kernel (9,3): ON unless FK_ML_PERSIST=0, serves BASELINE configs[2]; hand-over [9 + 81][N].  rts_ml_kernel (9) and
// ukf_linear_kernel (6,3; hand-over [6 + 21][N]) measured no faster (docs/KERNEL_NOTES.md): off unless asked for.
constexpr TicketPolicy KF_TICKETS = {"FK_ML_PERSIST", TICKETS_UNLESS_0, "FK_ML_PERSIST_H", 64, TICKET_H_THREE, false, false, 0, false, false, false, false, 90};
constexpr TicketPolicy RTS_TICKETS = {"FK_RTS_PERSIST", TICKETS_IF_NONZERO, "FK_RTS_PERSIST_H", 64, TICKET_H_THREE, true, false, 0, false, true, false, false, 90};
constexpr TicketPolicy UKF_TICKETS = {"FK_UKF_PERSIST", TICKETS_IF_1, "FK_UKF_PERSIST_H", 256, TICKET_H_FULLEST, false, true, 32, true, false, true, true, 27};

inline bool kf_tickets_serve(bool outs, bool aos)      // the forward kernel's instantiations: outputs; element-major only with slab stores
{
    const char *sv = getenv("FK_ML_SLAB");
    return outs && (aos || !(sv && atoi(sv) == 0));
}

// take == false: not a call the grid takes (all else 0).  The scratch: [tickets | G completion words] rounded to 256 bytes, hand-over.
struct TicketPlan { bool take; int G, H; unsigned grid; size_t ctl_bytes, ws_bytes; };
// The plan of a call over tracks [i0, i0 + cnt) of a bank of N, T steps.  n_cu() is asked only once the switch, `served` (what
// the family's instantiations need beyond the policy) and the call's shape have passed.
template <class NCu> inline TicketPlan ticket_plan(const TicketPolicy &p, long i0, long cnt, long N, long T, NCu &&n_cu, bool served = true)
{
    const char *pv = getenv(p.env);
    const int v = pv ? atoi(pv) : 0;
    if (!(p.on == TICKETS_UNLESS_0 ? !(pv && v == 0) : p.on == TICKETS_IF_NONZERO ? (pv && v != 0) : (pv && v == 1)) || !served) return {};
    if (p.cnt0_is_bank && cnt == 0) i0 = 0, cnt = N;
    if ((p.whole_bank && (i0 != 0 || cnt != N)) || T < p.min_T) return {};
    const long cus = n_cu(), slots = 2 * cus, G = (cnt + p.group - 1) / p.group;
    if (G <= (p.more_than_cus ? cus : slots) || G > (1L << 24)) return {};
    long H = T >= 48 ? 3 : T / 16;
    if (p.chunks == TICKET_H_FULLEST) {
        double best = 0.0;
        H = 0;
        for (long h = 4; h <= T / 6; ++h) {
            const double rounds = (double)(G * h) / (double)slots, fill = rounds / (double)((G * h + slots - 1) / slots);
            if (fill > best + 0.02) { best = fill; H = h; }
        }
    }
    if (const char *hv = getenv(p.env_h)) H = atol(hv);
    if (H < 2 || (p.two_steps && T / H < 2) || (p.h_within_T && H > T)) return {};
    return {true, (int)G, (int)H, (unsigned)(p.grid_to_tickets && G * H < slots ? G * H : slots),
            ((size_t)(1 + G) * sizeof(int) + 255) & ~(size_t)255, (size_t)p.ws_doubles * (size_t)N * sizeof(double)};
}

// Ticket `task` of G groups x H chunks over T steps: group g, the chunk's number in DRAWING order (it waits for ctl[1 + g] >= chunk --
// the ticket task - G -- and publishes chunk + 1) and its steps [t0, t1).  Forward, chunk c is the c-th window of the time axis; backward
// the c-th from its END, continuing (cont, c > 0) from the step above its window, which chunk c - 1 smoothed: t1 - t0 + 1 steps.
struct TicketWindow { int g, chunk; long t0, t1; bool cont; };
FK_HD TicketWindow ticket_window(int task, int G, int H, long T, bool backward)
{
    const int c = task / G, g = task - c * G;
    const long h0 = backward ? H - 1 - c : c, h1 = backward ? h0 + 1 : c + 1;      // (no branch: the kernels' code as it was)
    return {g, c, T * h0 / H, T * h1 / H, backward && c > 0};
}

}  // namespace fk

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
namespace fk {
// ------------------------------------------------------------------------------------------------- 2. the host side --
// compute units of the device that is current (256 where it cannot be asked), cached per device index
inline int cu_count()
{
    static int cus[16];
    int dev = 0;
    hipDeviceProp_t prop;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 16) return 256;
    if (!cus[dev]) cus[dev] = (hipGetDeviceProperties(&prop, dev) == hipSuccess && prop.multiProcessorCount > 0) ? prop.multiProcessorCount : 256;
    return cus[dev];
}

// The scratch of one ticket-grid call: stream-ordered and this call's alone (nothing shared between concurrent calls; capturable), the
// control block zeroed, freed on the same stream when the launcher returns.  False: the plan does not take the call, or no memory was to be
// had (the error is cleared) -- the launcher returns 1.
struct TicketScratch {
    int *ctl = nullptr;
    double *ws = nullptr;
    const hipStream_t s;
    TicketScratch(const TicketPlan &p, hipStream_t stream) : s(stream)
    {
        if (!p.take) return;
        if (hipMallocAsync((void **)&ctl, p.ctl_bytes + p.ws_bytes, s) != hipSuccess || !ctl) ctl = nullptr;
        else if (hipMemsetAsync(ctl, 0, p.ctl_bytes, s) != hipSuccess) { (void)hipFreeAsync(ctl, s); ctl = nullptr; }
        if (ctl) ws = reinterpret_cast<double *>(reinterpret_cast<char *>(ctl) + p.ctl_bytes);
        else (void)hipGetLastError();
    }
    TicketScratch(const TicketScratch &) = delete;
    ~TicketScratch() { if (ctl) (void)hipFreeAsync(ctl, s); }
    explicit operator bool() const { return ctl != nullptr; }
};

// --------------------------------------------------------------------- 3. the device protocol (all forced inline) --
// the next ticket, uniform over the workgroup (s_task: one LDS word of the kernel's)
__device__ __forceinline__ int ticket_draw(int *ctl, int &s_task)
{
    __syncthreads();                                         // the previous ticket's LDS traffic is over, s_task is free
    if (threadIdx.x == 0) s_task = atomicAdd(ctl, 1);
    __syncthreads();
    return __builtin_amdgcn_readfirstlane(s_task);
}

// until `need` chunks of group g are done.  (The state is then read with agent-scope loads: no acquire fence, no L2 invalidation.)
__device__ __forceinline__ void ticket_wait(int *ctl, int g, int need)
{
    if (need <= 0) return;
    if (threadIdx.x == 0)
        while (__hip_atomic_load(&ctl[1 + g], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < need) __builtin_amdgcn_s_sleep(8);
    __syncthreads();
}

// This chunk's state (and status) is in place -- written with agent-scope stores, which are coherent across the XCDs by themselves
// (a release FENCE here writes back the whole L2 the kernel is streaming 14 GB of outputs through: measured 0.55 ms per chunk).
// They are COMPLETE only once every wave's vmcnt has drained: a workgroup barrier does not wait for VMEM on gfx950 (the compiler
// emits `s_waitcnt vmcnt(63)` -- nothing -- in front of s_barrier; ADVICE r4: with status == NULL no other wait stood between the
// hand-over stores and the flag), so every wave drains explicitly -- inline asm, invisible to the pass that drops "redundant"
// waits -- then the barrier, then the chunk is published (value: the chunks of group g that are done).
__device__ __forceinline__ void ticket_publish(int *ctl, int g, int value)
{
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0) __hip_atomic_store(&ctl[1 + g], value, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// a track's status word, shared by the chunks of its group: agent-scope like the hand-over (status_or: OR into what is there)
__device__ __forceinline__ void status_merge_agent(int *status, long idx, int status_or, int s)
{
    const int old = status_or ? __hip_atomic_load(&status[idx], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0;
    __hip_atomic_store(&status[idx], old | s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

}  // namespace fk
#endif   // __HIPCC__
