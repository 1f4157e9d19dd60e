// fk_chunk_plan.hpp -- tail filling for the several-lanes-per-track kernels: the plan and the driver (no HIP in here).
//
// Their step is bound by arithmetic and latency, every wave runs the same T steps, so a bank of W waves on S wave slots
// takes ceil(W / S) rounds: BASELINE config 3 (1e5 tracks = 6250 waves on 2048 slots) pays 4 rounds for 3.05 rounds of
// work.  A chunked call cuts the bank into G track groups (multiples of a quantum of tracks) and the steps into H time chunks
// and launches the pieces on G streams -- group g's chunks in order on stream g, the state handed from chunk to chunk through
// memory (kernel boundaries of one stream: no protocol), different groups concurrently: while one group's piece tails
// off, the other groups' pieces fill the slots, and what is left at the very end is the tail of a piece 1/H as long.
// Group g's chunk boundaries are shifted by g / G of a chunk, else all groups would tail off at the same moments.
// Same arithmetic per track: results are bit-identical to the single launch (tests/test_gpu_kf.py).
//
// This header is plain C++17: tests/hostcheck compiles it for the host and runs chunked_call on recording lanes
// (tests/test_hostcheck_chunks.py: the pieces of every family against the goldens, the failure path).  The streams and
// events behind the lanes are fk_chunks.hpp's.
#pragma once
#include <stdio.h>
#include <stdlib.h>

// default decomposition of a chunked call: track groups x time chunks
#ifndef FK_ML_CHUNK_G
#define FK_ML_CHUNK_G 3
#endif
#ifndef FK_ML_CHUNK_H
#define FK_ML_CHUNK_H 4
#endif
#ifndef FK_ML_CHUNK_STAGGER
#define FK_ML_CHUNK_STAGGER 1
#endif

namespace fk {

constexpr int CHUNK_MAXG = 4;       // streams of a chunked call: the caller's and three helpers

// When a family's calls are cut.  "G,H" in the environment variable forces a decomposition ("1,1" or unparsable: one launch;
// read per call).  Else the default G x H applies where the call's waves are more than `lo` rounds of the wave slots and at
// most `hi` (0: no upper end: at 15 rounds a partial last one is 2 % of the call and the pieces' overheads are not -- the UKF
// smoother at 1e6 tracks x 20 steps measured 3.06 ms in one launch, 3.63 ms cut up), there are 16 steps or more and the
// last round is not empty and less than fill_tenths / 10 full.
struct ChunkPolicy {
    const char *env;
    bool has_default;               // false: cut only on request
    long lo, hi;
    int fill_tenths;
    long tracks_per_wave, quantum;  // quantum: the groups are multiples of it (a workgroup's tracks)
};
// KF / RTS several-lane kernels (kf_fast's caller passes 64 tracks per wave in groups of 256): last round under 40 %
constexpr ChunkPolicy KF_CHUNKS = {"FK_ML_CHUNKS", true, 2, 0, 4, 16, 64};
constexpr ChunkPolicy RTS_CHUNKS = KF_CHUNKS;
// IMM / MMAE banks: one to four rounds, last one under 60 % (the one-wave-per-SIMD classes lose up to a quarter to it: 2e5
// banks of (6,3) x 2 took 4.25 ms where 196 608 -- three full rounds -- took 3.28)
constexpr ChunkPolicy IMM_CHUNKS = {"FK_IMM_CHUNKS", true, 1, 4, 6, 64, 256};
// fused UKF smoother: one to three rounds, last one under 60 % (BASELINE configs[3]: 1563 waves on 1024 slots)
constexpr ChunkPolicy UKF_RTS_CHUNKS = {"FK_UKF_RTS_CHUNKS", true, 1, 3, 6, 64, 256};
// fused UKF: measured no faster (profiles/r03/ukf_chunking.jsonl)
constexpr ChunkPolicy UKF_CHUNKS = {"FK_UKF_CHUNKS", false, 0, 0, 0, 64, 256};

// G x H decomposition of a call over `tracks` tracks and `steps` steps; false: one launch
inline bool chunk_policy(const ChunkPolicy &p, long tracks, long steps, long slots, int &G, int &H)
{
    G = H = 1;
    const long waves = (tracks + p.tracks_per_wave - 1) / p.tracks_per_wave;
    if (const char *cv = getenv(p.env)) {
        if (sscanf(cv, "%d,%d", &G, &H) != 2) G = H = 1;
    } else if (p.has_default && waves > p.lo * slots && (p.hi == 0 || waves <= p.hi * slots) && steps >= 16) {
        const long rem = waves % slots;
        if (rem != 0 && rem * 10 < slots * p.fill_tenths) { G = FK_ML_CHUNK_G; H = FK_ML_CHUNK_H; }
    }
    if (G > CHUNK_MAXG) G = CHUNK_MAXG;
    if (H > 64) H = 64;
    if (H > steps) H = (int)steps;
    return G >= 1 && H >= 1 && !(G == 1 && H == 1) && tracks >= p.quantum * G;
}

// Window h (0..H; there is one more window than chunks because of the stagger) of track group g over L steps: [w0, w1).
// Group g's boundaries are shifted down by g / G of a chunk; false: empty window.  The H + 1 windows of a group tile
// [0, L) in order (tests/test_host_logic.py checks this through fk_chunk_plan for every L <= 128, G <= 4, H <= L).
inline bool chunk_window(long L, int G, int H, int g, int h, long &w0, long &w1)
{
    const long shift = (FK_ML_CHUNK_STAGGER && !getenv("FK_ML_NO_STAGGER")) ? (L * g) / ((long)H * G) : 0;
    w0 = L * h / H - shift;
    w1 = L * (h + 1) / H - shift;
    if (w0 < 0) w0 = 0;
    if (h == H) w1 = L;
    if (w1 > L) w1 = L;
    return w1 > w0;
}

// one launch of a chunked call: tracks [i0, i0 + cnt) x steps [t0, t1) on stream g
struct ChunkPiece {
    int g;
    long i0, cnt, t0, t1;
    bool first;                     // the first piece on its stream
};

// The pieces of tracks [i0, i0 + cnt) x L steps cut G x H, in launch order: f(piece) for group after group (multiples of
// the quantum, the last one takes the remainder), a group's non-empty windows from the first to the last -- backward: from
// the last to the first --; f's first nonzero return ends the walk and is returned.
template <class F>
int chunk_pieces(long i0, long cnt, long L, int G, int H, long quantum, bool backward, F &&f)
{
    const long blocks = (cnt + quantum - 1) / quantum, per = (blocks + G - 1) / G * quantum;
    for (int g = 0; g < G; ++g) {
        ChunkPiece p = {g, i0 + g * per, per, 0, 0, true};
        if (p.i0 + per > i0 + cnt) p.cnt = i0 + cnt - p.i0;
        if (p.cnt <= 0) break;
        for (int k = 0; k <= H; ++k) {
            if (!chunk_window(L, G, H, g, backward ? H - k : k, p.t0, p.t1)) continue;
            if (const int rc = f(p)) return rc;
            p.first = false;
        }
    }
    return 0;
}

// The driver.  `one(args, stream)` launches one piece, `slice(a, piece)` writes its arguments from the call's; the call
// covers tracks [i0, i0 + cnt) x `steps` steps.  The lanes are the streams: stream(0) the caller's, fork() marks the point
// of the caller's stream that the helpers start from (false: no helpers, one launch), wait(g) makes helper g wait for it,
// join(g) makes the caller's stream wait for what helper g was given.  Every helper that waited is joined -- also when a
// later piece failed to launch: the caller may free or reuse the buffers as soon as its own stream is done.
template <class Args, class Lanes, class Slice, class One>
int chunked_call(const ChunkPolicy &p, const Args &a, long i0, long cnt, long steps, long slots, bool backward, Lanes &&lanes,
                 Slice &&slice, One &&one)
{
    int G, H;
    if (!chunk_policy(p, cnt, steps, slots, G, H) || !lanes.fork()) return one(a, lanes.stream(0));
    bool forked[CHUNK_MAXG] = {};
    int rc = chunk_pieces(i0, cnt, steps, G, H, p.quantum, backward, [&](const ChunkPiece &pc) -> int {
        if (pc.first && pc.g > 0) {
            if (!lanes.wait(pc.g)) return -1;
            forked[pc.g] = true;
        }
        return one(slice(a, pc), lanes.stream(pc.g));
    });
    for (int g = 1; g < CHUNK_MAXG; ++g)
        if (forked[g] && !lanes.join(g) && rc == 0) rc = -1;
    return rc;
}

// optional output / input arrays: a NULL stays NULL in every piece
template <class Ptr>
inline Ptr ml_off(Ptr p, long d)
{
    return p ? p + d : nullptr;
}

// What the pieces of every family share: the track window, and the status bits are ORed into what an earlier piece left.
template <class Args>
inline Args chunk_slice(const Args &a, const ChunkPiece &p)
{
    Args b = a;
    b.i0 = p.i0;
    b.cnt = p.cnt;
    b.status_or = p.first ? a.status_or : 1;
    return b;
}

// The families.  (KfArgs ... UkfArgs are template parameters only to keep this header free of the kernel headers.)

// Forward filter: T steps from the pointers in the piece's arguments; the state is handed from chunk to chunk through x / P
// in place.
template <class Args, class Lanes, class One>
int kf_chunked(const Args &a, int n, int m, long slots, int tracks_per_wave, long group_quantum, Lanes &&lanes, One &&one)
{
    ChunkPolicy pol = KF_CHUNKS;
    pol.tracks_per_wave = tracks_per_wave;
    pol.quantum = group_quantum;
    return chunked_call(pol, a, a.i0, a.cnt, a.T, slots, false, lanes, [n, m](const Args &a, const ChunkPiece &p) {
        const long t0 = p.t0, nn = (long)n * n;
        Args b = chunk_slice(a, p);
        b.T = p.t1 - t0;
        b.z = a.z + t0 * a.N * m;
        b.mask = ml_off(a.mask, t0 * a.N);
        b.means = ml_off(a.means, t0 * a.N * n);
        b.means_p = ml_off(a.means_p, t0 * a.N * n);
        b.covs = ml_off(a.covs, t0 * a.cov_step);              // (cov_step = N n^2, or 2 N n^2: FK_KF_FLAG_COV_INTERLEAVED)
        b.covs_p = ml_off(a.covs_p, t0 * a.cov_step);
        if (a.model_t) {                                   // one model per step, shared by the bank (VAR instantiations)
            b.F = a.F + t0 * nn;
            b.Q = a.Q + t0 * nn;
            b.H = a.H + t0 * (long)m * n;
            b.R = a.R + t0 * (long)m * m;
            if (a.nu > 0) b.B = ml_off(a.B, t0 * (long)n * a.nu);
        }
        if (a.nu > 0) b.u = ml_off(a.u, t0 * a.N * a.nu);
        if (a.extras_per_step) {                           // the by-product histories advance with the time window too
            b.y_out = ml_off(a.y_out, t0 * a.N * m);
            b.K_out = ml_off(a.K_out, t0 * a.N * (long)n * m);
            b.S_out = ml_off(a.S_out, t0 * a.N * (long)m * m);
            b.SI_out = ml_off(a.SI_out, t0 * a.N * (long)m * m);
            b.ll_out = ml_off(a.ll_out, t0 * a.N);
            b.maha_out = ml_off(a.maha_out, t0 * a.N);
        }
        return b;
    }, one);
}

// The smoother runs backwards over the T - 1 steps T-2 .. 0: group g's chunks go from the last time window to the first on
// stream g; a chunk's window [k0, k1] shares its top step k1 with the chunk before it (which smoothed it): RtsArgs::cont.
// (the call may itself be a track window of a larger bank: cnt != 0 -- kf_dispatch.cpp; N stays the array stride)
template <class Args, class Lanes, class One>
int rts_chunked(const Args &a, int n, long slots, Lanes &&lanes, One &&one)
{
    return chunked_call(RTS_CHUNKS, a, a.cnt ? a.i0 : 0, a.cnt ? a.cnt : a.N, a.T - 1, slots, true, lanes,
                        [n](const Args &a, const ChunkPiece &p) {
        const long k0 = p.t0, nn = (long)n * n;
        Args b = chunk_slice(a, p);
        b.T = p.t1 - k0 + 1;                                   // steps k0 .. k1 of the arrays; k1 is the window's "T-1"
        b.cont = p.first ? 0 : 1;
        b.Xs = a.Xs + k0 * a.N * n;
        b.Ps = a.Ps + k0 * a.N * nn;
        b.xs = a.xs + k0 * a.N * n;
        b.Ps_out = a.Ps_out + k0 * a.N * nn;
        b.K = ml_off(a.K, k0 * a.N * nn);
        b.Pp = ml_off(a.Pp, k0 * a.N * nn);
        return b;
    }, one);
}

// The IMM / MMAE banks (imm_kernels.hip, ImmArgs; whole steps only): forward time chunks, the state handed from chunk to
// chunk through xs / Ps / mu (and ll0) in place.
template <class Args, class Lanes, class One>
int imm_chunked(const Args &a, int n, int m, int nm, long slots, Lanes &&lanes, One &&one)
{
    // A masked call carries, per filter, the log-density of a zero residual under the LAST S (what update(None) leaves,
    // kalman_filter.py:515-520 + IMM.py:176-177) from step to step: in registers inside one launch, through ll0 between
    // launches.  Without ll0 a later time chunk would restart them at -inf: such a call is one launch.
    if (a.mask && !a.ll0) return one(a, lanes.stream(0));
    return chunked_call(IMM_CHUNKS, a, a.i0, a.cnt, a.T, slots, false, lanes, [n, m, nm](const Args &a, const ChunkPiece &p) {
        const long t0 = p.t0, nn = (long)n * n;
        Args b = chunk_slice(a, p);
        b.T = p.t1 - t0;
        b.z = a.z + t0 * a.N * m;
        b.mask = ml_off(a.mask, t0 * a.N);
        if (a.nu > 0) b.u = ml_off(a.u, t0 * a.N * a.nu);
        b.x_out = ml_off(a.x_out, t0 * a.N * n);
        b.P_out = ml_off(a.P_out, t0 * a.N * nn);
        b.mu_out = ml_off(a.mu_out, t0 * a.N * nm);
        b.xp_out = ml_off(a.xp_out, t0 * a.N * n);
        b.Pp_out = ml_off(a.Pp_out, t0 * a.N * nn);
        b.L_out = ml_off(a.L_out, t0 * a.N * nm);
        return b;
    }, one);
}

// The fused linear UKF smoother (ukf_kernels.hip, UkfRtsArgs): backward windows like rts_chunked; the call itself may be a
// continuation (a.cont).
template <class Args, class Lanes, class One>
int ukf_rts_chunked(const Args &a, int n, long slots, Lanes &&lanes, One &&one)
{
    return chunked_call(UKF_RTS_CHUNKS, a, a.i0, a.cnt, a.T - 1, slots, true, lanes, [n](const Args &a, const ChunkPiece &p) {
        const long k0 = p.t0, nn = (long)n * n;
        Args b = chunk_slice(a, p);
        b.T = p.t1 - k0 + 1;
        b.cont = p.first ? a.cont : 1;
        b.Xs = a.Xs + k0 * a.N * n;
        b.Ps = a.Ps + k0 * a.N * nn;
        b.xs = a.xs + k0 * a.N * n;
        b.ps = a.ps + k0 * a.N * nn;
        b.Ks = ml_off(a.Ks, k0 * a.N * nn);
        return b;
    }, one);
}

// The fused linear UKF (ukf_kernels.hip, UkfArgs): only on request, same hand-over through x / P.
template <class Args, class Lanes, class One>
int ukf_chunked(const Args &a, int n, int m, Lanes &&lanes, One &&one)
{
    return chunked_call(UKF_CHUNKS, a, a.i0, a.cnt, a.T, 0, false, lanes, [n, m](const Args &a, const ChunkPiece &p) {
        const long t0 = p.t0, nn = (long)n * n;
        Args b = chunk_slice(a, p);
        b.T = p.t1 - t0;
        b.z = a.z + t0 * a.N * m;
        b.mask = ml_off(a.mask, t0 * a.N);
        b.means = ml_off(a.means, t0 * a.N * n);
        b.covs = ml_off(a.covs, t0 * a.N * nn);
        return b;
    }, one);
}

}  // namespace fk
