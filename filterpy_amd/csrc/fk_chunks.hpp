// fk_chunks.hpp -- tail filling for the several-lanes-per-track kernels: the HIP side.  fk_chunk_plan.hpp decides how a call
// is cut and drives the pieces; here are the streams it drives them on.  The helper streams fork from and join the caller's
// stream with events (capturable into a HIP graph); they and the events are created once per device.
#pragma once
#include <hip/hip_runtime.h>

#include <mutex>

#include "fk_chunk_plan.hpp"

namespace fk {

struct MlStreams {
    static constexpr int MAXG = CHUNK_MAXG;
    hipStream_t st[MAXG] = {};
    hipEvent_t fork = nullptr, done[MAXG] = {};
    bool ok = false;
    std::mutex mu;      // one chunked call enqueues at a time: a stream wait binds to the event's LATEST record
    void create()       // on the device that is current: streams and events belong to a device
    {
        ok = hipEventCreateWithFlags(&fork, hipEventDisableTiming) == hipSuccess;
        for (int g = 1; g < MAXG && ok; ++g)
            ok = hipStreamCreateWithFlags(&st[g], hipStreamNonBlocking) == hipSuccess &&
                 hipEventCreateWithFlags(&done[g], hipEventDisableTiming) == hipSuccess;
    }
};

// one set of helper streams per device, created on first use with that device current (a process that drives several
// GPUs must not launch one device's pieces on another device's streams); nullptr: no chunking
inline MlStreams *ml_streams()
{
    static constexpr int MAXDEV = 16;
    static MlStreams sets[MAXDEV];
    static bool made[MAXDEV] = {};
    static std::mutex mk;
    int dev = -1;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= MAXDEV) return nullptr;
    std::lock_guard<std::mutex> lock(mk);
    if (!made[dev]) {
        sets[dev].create();
        made[dev] = true;
    }
    return sets[dev].ok ? &sets[dev] : nullptr;
}

// the lanes of one chunked call on the caller's stream s (chunked_call, fk_chunk_plan.hpp): the current device's helper
// streams, held from the fork until the call has enqueued its last piece and its joins
struct MlLanes {
    hipStream_t s;
    MlStreams *ms = nullptr;
    std::unique_lock<std::mutex> lock;
    hipStream_t stream(int g) const { return g == 0 ? s : ms->st[g]; }
    bool fork()
    {
        if (!(ms = ml_streams())) return false;
        lock = std::unique_lock<std::mutex>(ms->mu);
        return hipEventRecord(ms->fork, s) == hipSuccess;
    }
    bool wait(int g) { return hipStreamWaitEvent(ms->st[g], ms->fork, 0) == hipSuccess; }
    bool join(int g)
    {
        if (hipEventRecord(ms->done[g], ms->st[g]) == hipSuccess && hipStreamWaitEvent(s, ms->done[g], 0) == hipSuccess) return true;
        (void)hipStreamSynchronize(ms->st[g]);          // last resort: the join must not be skipped
        return false;
    }
};

// The five families' calls (fk_chunk_plan.hpp: kf_chunked ...) on these lanes.  `one(args, stream)` launches one piece.
template <class Args, class One>
int kf_chunked_call(const Args &a, int n, int m, long slots, One &&one, hipStream_t s, int tracks_per_wave = 16, long group_quantum = 64)
{
    return kf_chunked(a, n, m, slots, tracks_per_wave, group_quantum, MlLanes{s}, one);
}

template <class Args, class One>
int rts_chunked_call(const Args &a, int n, long slots, One &&one, hipStream_t s)
{
    return rts_chunked(a, n, slots, MlLanes{s}, one);
}

template <class Args, class One>
int imm_chunked_call(const Args &a, int n, int m, int nm, long slots, One &&one, hipStream_t s)
{
    return imm_chunked(a, n, m, nm, slots, MlLanes{s}, one);
}

template <class Args, class One>
int ukf_rts_chunked_call(const Args &a, int n, long slots, One &&one, hipStream_t s)
{
    return ukf_rts_chunked(a, n, slots, MlLanes{s}, one);
}

template <class Args, class One>
int ukf_chunked_call(const Args &a, int n, int m, One &&one, hipStream_t s)
{
    return ukf_chunked(a, n, m, MlLanes{s}, one);
}

}  // namespace fk
