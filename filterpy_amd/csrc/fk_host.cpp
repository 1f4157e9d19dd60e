// fk_host.cpp -- host-side plumbing of libfilterhip: error capture and ABI utilities.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <string.h>

#include "../../include/filterhip.h"
#include "fk_device.hpp"
#include "fk_chunk_plan.hpp"

namespace fk {

static thread_local char g_err[512] = "";

void set_last_error(const char *msg)
{
    strncpy(g_err, msg ? msg : "", sizeof(g_err) - 1);
    g_err[sizeof(g_err) - 1] = 0;
}

int check_launch(const char *what)
{
    const hipError_t e = hipGetLastError();
    if (e == hipSuccess) return FK_OK;
    char buf[512];
    snprintf(buf, sizeof(buf), "%s: %s", what, hipGetErrorString(e));
    set_last_error(buf);
    return FK_ERR_LAUNCH;
}

}  // namespace fk

extern "C" {

int fk_abi_version(void) { return FK_ABI_VERSION; }
const char *fk_build_arch(void) { return "gfx950"; }
const char *fk_last_error(void) { return fk::g_err; }

// what a chunked call would do (fk_chunk_plan.hpp): host arithmetic only, no GPU work
int fk_chunk_plan(int64_t n_tracks, int64_t n_steps, int32_t tracks_per_wave, int64_t wave_slots, int32_t group,
                  int64_t *windows, int32_t *n_groups, int32_t *n_chunks)
{
    if (n_tracks < 0 || n_steps < 1 || tracks_per_wave < 1 || wave_slots < 1 || !windows) return -1;
    fk::ChunkPolicy pol = fk::KF_CHUNKS;
    pol.tracks_per_wave = tracks_per_wave;
    pol.quantum = 0;                                    // (the waves alone decide here, however few the tracks)
    int G, H;
    if (!fk::chunk_policy(pol, n_tracks, n_steps, wave_slots, G, H)) G = H = 1;
    if (n_groups) *n_groups = G;
    if (n_chunks) *n_chunks = H;
    if (group < 0 || group >= G) return -1;
    int nw = 0;
    // the step windows do not depend on the tracks: G groups of one track each
    fk::chunk_pieces(0, G, n_steps, G, H, 1, false, [&](const fk::ChunkPiece &p) {
        if (p.g == group) {
            windows[2 * nw] = p.t0;
            windows[2 * nw + 1] = p.t1;
            ++nw;
        }
        return 0;
    });
    return nw;
}

}  // extern "C"
