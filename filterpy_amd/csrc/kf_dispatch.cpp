// kf_dispatch.cpp -- C-ABI entry points of the linear Kalman filter path and the
// (dim_x, dim_z) -> kernel instantiation dispatch.
//
// fk_kf_batch_filter_f64 <- KalmanFilter.batch_filter  (filterpy/kalman/kalman_filter.py:826-993)
// fk_kf_predict_f64      <- KalmanFilter.predict       (:437-482)
// fk_kf_update_f64       <- KalmanFilter.update        (:485-561)
// fk_kf_rts_f64          <- KalmanFilter.rts_smoother  (:995-1074), module rts_smoother (:1792-1858)
// fk_kf_steadystate_f64       <- KalmanFilter.predict_steadystate / update_steadystate (:563-668), T steps in one launch
// fk_kf_update_correlated_f64 <- KalmanFilter.update_correlated (:670-752)
#include "fk_dispatch.hpp"
#include "fk_kernel_args.hpp"
#include "fk_chunks.hpp"
#include "fk_launchers.hpp"

namespace fk {

// One entry type per launcher signature: the general filter kernels (layout, one model for the bank), the specialised filter
// kernels (layout, outputs stored, model mode) and the smoothers.
struct KfEntry {
    int nx, nz, exact;
    int (*fn)(const KfArgs &, int, bool, hipStream_t);
};
struct KfModeEntry {
    int nx, nz, variant;
    int (*fn)(const KfArgs &, int, bool, int, hipStream_t);
};
struct RtsEntry {
    static constexpr int nz = 0;
    int nx, exact;
    int (*fn)(const RtsArgs &, int, bool, hipStream_t);
};

#define FK_KF_INST(NX, NZ, EX) int launch_kf_##NX##_##NZ##_##EX(const KfArgs &, int, bool, hipStream_t);
#include "fk_dims.def"
#undef FK_KF_INST
#define FK_FAST_INST(NX, NZ, V, W, S, WA, ZD) int launch_kf_fast_##NX##_##NZ##_v##V(const KfArgs &, int, bool, int, hipStream_t);
#include "fk_dims_fast.def"
#undef FK_FAST_INST
#define FK_RTS_INST(NX, EX) int launch_rts_##NX##_##EX(const RtsArgs &, int, bool, hipStream_t);
#include "fk_dims_rts.def"
#undef FK_RTS_INST
#define FK_MLG_INST(NX, NZ) int launch_kf_mlg_##NX##_##NZ(const KfArgs &, int, bool, int, hipStream_t);
#define FK_RMLG_INST(NX) int launch_rts_mlg_##NX(const RtsArgs &, int, bool, hipStream_t);
#define FK_RMLX_INST(NX) int launch_rts_mlx_##NX(const RtsArgs &, int, bool, hipStream_t);
#include "fk_dims_mlg.def"
#undef FK_MLG_INST
#undef FK_RMLG_INST
#undef FK_RMLX_INST

int launch_kf_given(const KfArgs &, int, bool, int, hipStream_t);     // kf_given_inv.hip: update() / rts_smoother() around a
int launch_rts_given(const RtsArgs &, int, bool, int, hipStream_t);   // caller-supplied inverse
int launch_kf_ml_9_3(const KfArgs &, int, bool, int, hipStream_t);   // kf_ml.hip: three lanes per track
int launch_rts_ml_9(const RtsArgs &, int, bool, hipStream_t);

static const KfEntry kf_table[] = {
#define FK_KF_INST(NX, NZ, EX) {NX, NZ, EX, launch_kf_##NX##_##NZ##_##EX},
#include "fk_dims.def"
#undef FK_KF_INST
};
static const KfModeEntry fast_table[] = {
#define FK_FAST_INST(NX, NZ, V, W, S, WA, ZD) {NX, NZ, V, launch_kf_fast_##NX##_##NZ##_v##V},
#include "fk_dims_fast.def"
#undef FK_FAST_INST
};
static const RtsEntry rts_table[] = {
#define FK_RTS_INST(NX, EX) {NX, EX, launch_rts_##NX##_##EX},
#include "fk_dims_rts.def"
#undef FK_RTS_INST
};
// kf_mlg.hip / rts_mlg.hip: four lanes per track, dim_x = 10..16; rts_mlx.hip: eight (the list gives an empty meaning to
// whichever of its three macros the includer leaves out)
#define FK_MLG_INST(NX, NZ) {NX, NZ, 0, launch_kf_mlg_##NX##_##NZ},
static const KfModeEntry mlg_table[] = {
#include "fk_dims_mlg.def"
};
#undef FK_MLG_INST
#undef FK_RMLG_INST
#undef FK_RMLX_INST
#define FK_RMLG_INST(NX) {NX, 1, launch_rts_mlg_##NX},
static const RtsEntry rmlg_table[] = {
#include "fk_dims_mlg.def"
};
#undef FK_MLG_INST
#undef FK_RMLG_INST
#undef FK_RMLX_INST
#define FK_RMLX_INST(NX) {NX, 1, launch_rts_mlx_##NX},
static const RtsEntry rmlx_table[] = {
#include "fk_dims_mlg.def"
};
#undef FK_MLG_INST
#undef FK_RMLG_INST
#undef FK_RMLX_INST

static const KfModeEntry *pick_fast_variant(int n, int m)
{
    // FK_FAST_VARIANT selects a tuning variant (A/B measurements); default 0
    const char *ev = getenv("FK_FAST_VARIANT");
    const int want = ev ? atoi(ev) : 0;
    const KfModeEntry *dflt = nullptr;
    for (const KfModeEntry &e : fast_table) {
        if (e.nx != n || e.nz != m) continue;
        if (e.variant == want) return &e;
        if (!dflt || e.variant < dflt->variant) dflt = &e;     // variant 0 if compiled, else the lean one
    }
    return dflt;
}

// The general kernel of a size: the exact instantiation if there is one, else the padded one that holds it at the smallest
// NX^3 + NX^2*NZ cost (the smoothers' tables hold nz = 0: the smallest NX).
template <class Entry, size_t K>
static const Entry *pick_general(const Entry (&table)[K], int n, int m = 0)
{
    const Entry *best = nullptr;
    long best_cost = 0;
    for (const Entry &e : table) {
        if (e.exact) {
            if (e.nx == n && e.nz == m) return &e;
            continue;
        }
        if (e.nx < n || e.nz < m) continue;
        const long cost = (long)e.nx * e.nx * e.nx + (long)e.nx * e.nx * e.nz;
        if (!best || cost < best_cost) {
            best = &e;
            best_cost = cost;
        }
    }
    return best;
}

static const char *const RANGE = "dim_x/dim_z outside the compiled range (dim_x <= 16, dim_z <= 8)";

static int check_kf_desc(const fk_kf_desc *d)
{
    if (!d) return fail(FK_ERR_BAD_ARG, "desc is NULL");
    if (d->n < 1 || d->m < 1 || d->nu < 0) return fail(FK_ERR_BAD_ARG, "dim_x, dim_z must be >= 1, dim_u >= 0");
    if (d->N < 0 || d->T < 0) return fail(FK_ERR_BAD_ARG, "N and T must be >= 0");
    if (d->layout != FK_LAYOUT_AOS && d->layout != FK_LAYOUT_SOA) return fail(FK_ERR_BAD_ARG, "bad layout");
    if (d->model_mode < 0 || d->model_mode > 3) return fail(FK_ERR_BAD_ARG, "bad model_mode");
    if (d->flags & ~(FK_KF_FLAG_R_JOSEPH_DIAG | FK_KF_FLAG_COV_INTERLEAVED | FK_KF_FLAG_S_ONLY | FK_KF_FLAG_SI_GIVEN |
                     FK_KF_FLAG_PP_ONLY | FK_KF_FLAG_PPINV_GIVEN))
        return fail(FK_ERR_BAD_ARG, "unknown desc flag");
    // NumPy order: the entry points cut a larger bank into track windows themselves (walk_windows below); element-major:
    // element e of a step sits e * N * 8 bytes into it whatever the window, so there the caller has to split the bank
    // (32 bytes short of 4 GiB: the by-product histories' copy-out drops stores by an offset just below it, fk_ml.hpp)
    if (d->layout != FK_LAYOUT_SOA) return FK_OK;
    return check_record_block((double)d->N, (double)d->n * (d->n > d->m ? d->n : d->m), FK_4GIB - 32.0,
                              "element-major layout: N * dim^2 * 8 bytes must stay below 4 GiB (use FK_LAYOUT_AOS, which is split automatically, or split the bank)");
}

// What desc says about the models, for the arguments and for the launchers.
static bool uniform_model(const fk_kf_desc *d) { return d->model_mode == FK_MODEL_SHARED || d->model_mode == FK_MODEL_PER_STEP; }
static int model_per_step(const fk_kf_desc *d) { return (d->model_mode == FK_MODEL_PER_TRACK_STEP || d->model_mode == FK_MODEL_PER_STEP) ? 1 : 0; }

// The fields of the argument block that come from desc, for a launch over tracks [0, cnt) of the pointers in a.
static void fill(KfArgs &a, const fk_kf_desc *d, long cnt)
{
    a.N = d->N; a.n = d->n; a.m = d->m; a.nu = d->nu;
    a.model_t = model_per_step(d);
    a.update_first = d->update_first;
    a.alpha_sq = d->alpha_sq;
    a.rj_diag = (d->flags & FK_KF_FLAG_R_JOSEPH_DIAG) ? 1 : 0;      // served by the generic kernels only
    a.i0 = 0; a.cnt = cnt;
    a.cov_step = d->N * (long)d->n * d->n;
    a.cov_pitch = d->n * d->n;
}

// Largest track window whose per-step record block stays below 4 GiB (a multiple of the workgroup's 256 tracks).  In NumPy
// order every record array is [..][N][E], so advancing each pointer by i0 records leaves the step stride N * E alone and the
// window's tracks count from 0: banks beyond one window are walked, not refused.
static long kf_window_tracks(const fk_kf_desc *d)
{
    const long E = (long)d->n * (d->n > d->m ? d->n : d->m);
    long w = (long)(4294967295.0 / ((double)E * 8.0));
    if (const char *wv = getenv("FK_KF_WINDOW")) {              // tests: force the windowing on a small bank
        const long f = atol(wv);
        if (f > 0 && f < w) w = f;
    }
    w = w / 256 * 256;
    return w < 256 ? 256 : w;
}

// The arguments of the window that starts at track i0 (optional arrays stay NULL: ml_off, fk_chunks.hpp).
static KfArgs window_of(const fk_kf_desc *d, const KfArgs &a, long i0)
{
    KfArgs b = a;
    const long n = d->n, m = d->m, nu = d->nu;
    if (!uniform_model(d)) {
        b.F = ml_off(a.F, i0 * n * n); b.Q = ml_off(a.Q, i0 * n * n); b.H = ml_off(a.H, i0 * m * n); b.R = ml_off(a.R, i0 * m * m);
        b.B = ml_off(a.B, i0 * n * nu);
    }
    b.u = ml_off(a.u, i0 * nu); b.z = ml_off(a.z, i0 * m); b.mask = ml_off(a.mask, i0);
    b.x = ml_off(a.x, i0 * n); b.P = ml_off(a.P, i0 * n * n);
    b.means = ml_off(a.means, i0 * n); b.means_p = ml_off(a.means_p, i0 * n);
    const long pitch = (d->flags & FK_KF_FLAG_COV_INTERLEAVED) ? 2 * n * n : n * n;
    b.covs = ml_off(a.covs, i0 * pitch); b.covs_p = ml_off(a.covs_p, i0 * pitch);
    b.y_out = ml_off(a.y_out, i0 * m); b.K_out = ml_off(a.K_out, i0 * n * m); b.S_out = ml_off(a.S_out, i0 * m * m);
    b.SI_out = ml_off(a.SI_out, i0 * m * m); b.ll_out = ml_off(a.ll_out, i0); b.maha_out = ml_off(a.maha_out, i0);
    b.status = ml_off(a.status, i0);
    return b;
}

static RtsArgs window_of(const fk_kf_desc *d, const RtsArgs &a, long i0)
{
    RtsArgs b = a;
    const long n = d->n, nn = n * n;
    if (!uniform_model(d)) { b.F = ml_off(a.F, i0 * nn); b.Q = ml_off(a.Q, i0 * nn); }
    b.Xs = ml_off(a.Xs, i0 * n); b.xs = ml_off(a.xs, i0 * n);
    b.Ps = ml_off(a.Ps, i0 * nn); b.Ps_out = ml_off(a.Ps_out, i0 * nn); b.K = ml_off(a.K, i0 * nn); b.Pp = ml_off(a.Pp, i0 * nn);
    b.status = ml_off(a.status, i0);
    return b;
}

// The filter and the smoother over a bank: one call of run(args, tracks) -- `whole` tracks -- where the bank fits a window or
// is element-major, else the windows in turn on the caller's stream (each is millions of tracks).
template <class Args, class Run>
static int walk_windows(const fk_kf_desc *d, Args &a, long whole, Run &&run)
{
    const long w = kf_window_tracks(d);
    if (d->layout != FK_LAYOUT_AOS || d->N <= w) return run(a, whole);
    for (long i0 = 0; i0 < d->N; i0 += w) {
        Args b = window_of(d, a, i0);
        if (int rc = run(b, d->N - i0 < w ? d->N - i0 : w)) return rc;
    }
    return FK_OK;
}

// FK_KF_FLAG_COV_INTERLEAVED: covs / covs_p are the two halves of one array (fk_kernel_args.hpp)
static int check_interleaved(const fk_kf_desc *d, KfArgs &a)
{
    const long nn = (long)d->n * d->n;
    if (!a.means || !a.covs || !a.means_p || !a.covs_p || !a.do_predict || !a.do_update)
        return fail(FK_ERR_BAD_ARG, "FK_KF_FLAG_COV_INTERLEAVED: batch_filter with all four outputs");
    const long half = d->layout == FK_LAYOUT_AOS ? nn : nn * d->N;
    if (a.covs_p != a.covs + half) return fail(FK_ERR_BAD_ARG, "FK_KF_FLAG_COV_INTERLEAVED: covs_p must be covs + n*n (AOS) / covs + n*n*N (SOA)");
    if (int rc = check_record_block((double)a.cnt, 2.0 * (double)nn, FK_4GIB, "FK_KF_FLAG_COV_INTERLEAVED: 2 * N * dim_x^2 * 8 bytes must stay below 4 GiB"))
        return rc;
    a.cov_step = 2 * d->N * nn;
    if (d->layout == FK_LAYOUT_AOS) a.cov_pitch = (int)(2 * nn);
    return FK_OK;
}

// The switches of the two routes below (A/B measurements, tests): read per call -- tests set them in-process -- and each only
// by the candidate that asks.
static bool env_set(const char *name) { return getenv(name) != nullptr; }
static int env_int(const char *name, int dflt) { const char *v = getenv(name); return v ? atoi(v) : dflt; }
static bool no_fast() { return env_set("FK_NO_FAST"); }             // the general kernel instead of the specialised ones
static bool no_fast_ex() { return env_set("FK_NO_FAST_EX"); }       // ... for the calls with by-product histories
static bool no_ml() { return env_set("FK_NO_ML"); }                 // no three-lane kernels (kf_ml.hip)
static bool no_mlg() { return env_set("FK_NO_MLG"); }               // no four- / eight-lane kernels (kf_mlg.hip, rts_mlg.hip, rts_mlx.hip)
static bool no_mlg_ex() { return env_set("FK_NO_MLG_EX"); }         // ... for the calls with by-product histories
// FK_ML9 = g / m: dim_x = 9 (and the smoother's 8) on the four-lane kernels / on the three- and one-lane ones; 0: unset
static char ml9() { const char *v = getenv("FK_ML9"); return v ? v[0] : '\0'; }
static int fast_xcd() { return env_int("FK_FAST_XCD", 0); }
static int rts_lanes(int dflt) { return env_int("FK_RTS_LANES", dflt); }    // 8 / 4 forces one organisation of the smoother

// The filter kernel of a call: the candidates in order, each a condition and a launcher; the first that does not answer
// NOT_SERVED has the call, the general kernel takes what is left.
static int route_kf(const fk_kf_desc *d, KfArgs &a, const KfEntry *general, hipStream_t s)
{
    const int n = d->n, m = d->m, layout = d->layout, mode = d->model_mode;
    const bool inter = (d->flags & FK_KF_FLAG_COV_INTERLEAVED) != 0;
    // The specialised kernels serve the common batch_filter call: predict->update, all four outputs stored or none ...
    const bool all_out = a.means && a.covs && a.means_p && a.covs_p;
    const bool no_out = !a.means && !a.covs && !a.means_p && !a.covs_p;
    // ... and the same call with the update's by-products as per-step histories (batch_filter_ex): shared constant model,
    // all four outputs, no control input
    const bool want_ex = a.y_out || a.K_out || a.S_out || a.SI_out || a.ll_out || a.maha_out;
    const bool plain_ex = want_ex && a.extras_per_step && all_out && mode == FK_MODEL_SHARED && d->nu == 0 && !d->update_first &&
                          !no_fast_ex();
    const auto four_lanes = [&] {
        const KfModeEntry *g = find_entry(mlg_table, n, m);
        return g ? g->fn(a, layout, all_out, mode, s) : NOT_SERVED;
    };
    int rc;
    // the histories from the four-lane kernels' EX instantiations (dim_x >= 10, and (9,3)): the plain call without a mask
    const bool four_lanes_ex = plain_ex && !a.mask && !inter && n >= 9 && !no_mlg_ex() && !no_mlg();
    if (a.do_predict && a.do_update && (all_out || no_out) && (!want_ex || plain_ex) && !a.rj_diag && !no_fast()) {
        if (four_lanes_ex && (rc = four_lanes()) != NOT_SERVED) return rc;
        const char g9 = ml9();          // 'g': dim_x = 9 on the four-lane kernels (A/B against kf_ml / rts_ml)
        // (9,3): three lanes per track (kf_ml.hip)
        if (!want_ex && n == 9 && m == 3 && !no_ml() && g9 != 'g') {
            if (inter) return fail(FK_ERR_UNSUPPORTED, "FK_KF_FLAG_COV_INTERLEAVED: (9,3) runs on the three-lane kernel, which takes two arrays");
            if ((rc = launch_kf_ml_9_3(a, layout, all_out, mode, s)) != NOT_SERVED) return rc;
        }
        // dim_x >= 10: four lanes per track (kf_mlg.hip)
        // (dim_x = 7, 8 were tried on the four-lane kernel too: 0.30 against kf_fast's 0.50 -- two rows per lane leave
        // the replicated S / x work dominant; profiles/r02/dims_7_8_ml_vs_fast.txt)
        // (9,1), (9,2), (9,4) too -- the one-lane kernel holds 9 x 9 at 0.18-0.26 of HBM (profiles/r05/dims/); FK_ML9=m keeps it
        const bool nine_g = n == 9 && (m != 3 ? g9 != 'm' : g9 == 'g');
        if (!want_ex && (n >= 10 || nine_g) && !no_mlg()) {
            if (inter) return fail(FK_ERR_UNSUPPORTED, "FK_KF_FLAG_COV_INTERLEAVED: dim_x >= 9 runs on the several-lane kernels, which take two arrays");
            if ((rc = four_lanes()) != NOT_SERVED) return rc;
        }
        // exact (dim_x, dim_z) up to 9: one lane per track (kf_fast.hip; every model mode at dim_x <= 6, shared constant model
        // above -- NOT_SERVED: this instantiation does not carry the model mode)
        if (const KfModeEntry *f = pick_fast_variant(n, m)) {
            a.xcd_swizzle = fast_xcd();
            if (n >= 7 && all_out && !want_ex && mode == FK_MODEL_SHARED && d->nu == 0 && !d->update_first) {
                // the one-wave-per-SIMD instantiations (dim_x 7..9) are bound by arithmetic, not HBM: tail filling
                // (fk_chunks.hpp) where the last round of waves would be mostly idle -- e.g. 2e5 tracks = 3125 waves
                // of 64 on 1024 slots
                rc = kf_chunked_call(a, n, m, 1024,
                                     [f, layout, mode](const KfArgs &b, hipStream_t sb) { return f->fn(b, layout, true, mode, sb); },
                                     s, 64, 256);
            } else {
                rc = f->fn(a, layout, all_out, mode, s);
            }
            if (rc != NOT_SERVED) return rc;
        }
    }
    if (inter) return fail(FK_ERR_UNSUPPORTED, "FK_KF_FLAG_COV_INTERLEAVED: not a call the specialised kernel serves");
    return general->fn(a, layout, uniform_model(d), s);
}

// One track window of a filter call: the arguments, the interleaved flag, the route.
static int run_kf_window(const fk_kf_desc *d, KfArgs &a, long cnt, void *stream)
{
    const KfEntry *general = pick_general(kf_table, d->n, d->m);
    if (!general) return fail(FK_ERR_UNSUPPORTED, RANGE);
    fill(a, d, cnt);
    if (d->flags & FK_KF_FLAG_COV_INTERLEAVED)
        if (int rc = check_interleaved(d, a)) return rc;
    return route_kf(d, a, general, (hipStream_t)stream);
}

static int run_kf(const fk_kf_desc *d, KfArgs &a, void *stream)
{
    if (d->N == 0 || a.T == 0) return FK_OK;
    return walk_windows(d, a, d->N, [&](KfArgs &b, long cnt) { return run_kf_window(d, b, cnt, stream); });
}

// The smoother kernel of a call, as route_kf.
static int route_rts(const fk_kf_desc *d, const RtsArgs &a, const RtsEntry *general, hipStream_t s)
{
    const int n = d->n, layout = d->layout;
    const bool uniform = uniform_model(d);
    const auto from = [&](const RtsEntry *g) { return g ? g->fn(a, layout, uniform, s) : NOT_SERVED; };
    int rc;
    // dim_x = 9: the three-lane smoother (rts_ml_kernel) in the element-major layout, the four-lane one (rts_mlg_kernel<9>)
    // in NumPy order -- its row blocks leave through an LDS slab as 1 KiB stores: 0.51 of HBM against 0.35 for
    // rts_ml's 16-byte-per-lane AOS path (profiles/r02/c3_ml_vs_mlg.jsonl).
    const char g9 = ml9();
    const bool rts9_generic = g9 ? g9 == 'g' : layout == FK_LAYOUT_AOS;
    if (n == 9 && !no_ml() && !rts9_generic && (rc = launch_rts_ml_9(a, layout, uniform, s)) != NOT_SERVED) return rc;
    // dim_x = 8 in NumPy order: the one-lane smoother's per-lane 16-byte accesses reach 0.34, the four-lane kernel's
    // slab 0.51 (element-major: 0.63 vs 0.58, stays); FK_ML9=m keeps the one-lane kernel
    const bool rts8_generic = n == 8 && layout == FK_LAYOUT_AOS && g9 != 'm';
    if ((n >= 10 || (n == 9 && rts9_generic) || rts8_generic) && !no_mlg()) {
        // eight lanes per track + LDS exchange where the four-lane kernel's unrolled step outgrows the instruction
        // cache (dim_x >= 15; n = 14 AOS: 76 KB of code)
        const int lanes = rts_lanes((n >= 15 || (n == 14 && layout == FK_LAYOUT_AOS)) ? 8 : 4);
        if (lanes == 8 && (rc = from(find_entry(rmlx_table, n))) != NOT_SERVED) return rc;
        if ((rc = from(find_entry(rmlg_table, n))) != NOT_SERVED) return rc;
    }
    return general->fn(a, layout, uniform, s);
}

// The two caller-supplied-inverse calls (kf_given_inv.hip: update() with FK_KF_FLAG_S_ONLY / _SI_GIVEN, rts_smoother() with
// _PP_ONLY / _PPINV_GIVEN; one padded instantiation for every size): the kernel's mode -- 1: the by-product only, 2: the
// inverse given -- or the refusal.  A bank beyond one track window is refused, not walked.
static int check_given(const fk_kf_desc *d, int only, int given, const char *both, bool only_ok, const char *only_needs,
                       bool given_ok, const char *given_needs, bool in_range)
{
    const int gm = d->flags & (only | given);
    if (gm == (only | given)) return fail(FK_ERR_BAD_ARG, both);
    if (gm == only && !only_ok) return fail(FK_ERR_BAD_ARG, only_needs);
    if (gm == given && !given_ok) return fail(FK_ERR_BAD_ARG, given_needs);
    if (!in_range) return fail(FK_ERR_UNSUPPORTED, RANGE);
    if (d->N > kf_window_tracks(d)) return fail(FK_ERR_UNSUPPORTED, "caller-supplied inverse: N * dim^2 * 8 bytes must stay below 4 GiB (split the bank)");
    return gm == only ? 1 : 2;
}

}  // namespace fk

using namespace fk;

extern "C" {

int fk_kf_batch_filter_f64(const fk_kf_desc *desc, const double *F, const double *Q, const double *H,
                           const double *R, const double *B, const double *u, const double *z,
                           const uint8_t *mask, double *x, double *P, double *means, double *covs,
                           double *means_p, double *covs_p, int32_t *status, void *stream)
{
    return fk_kf_batch_filter_ex_f64(desc, F, Q, H, R, B, u, z, mask, x, P, means, covs, means_p, covs_p, nullptr, status, stream);
}

int fk_kf_batch_filter_ex_f64(const fk_kf_desc *desc, const double *F, const double *Q, const double *H,
                              const double *R, const double *B, const double *u, const double *z,
                              const uint8_t *mask, double *x, double *P, double *means, double *covs,
                              double *means_p, double *covs_p, const fk_kf_extras *ex, int32_t *status,
                              void *stream)
{
    if (int rc = check_kf_desc(desc)) return rc;
    if (desc->N == 0 || desc->T == 0) return FK_OK;                 // an empty bank / an empty run: nothing to read, nothing to touch
    if (!F || !Q || !H || !R || !z || !x || !P) return fail(FK_ERR_BAD_ARG, "F,Q,H,R,z,x,P must not be NULL");
    if (int rc = check_control(desc, B, u)) return rc;
    KfArgs a{};
    a.F = F; a.Q = Q; a.H = H; a.R = R; a.B = B; a.u = u; a.z = z; a.mask = mask;
    a.x = x; a.P = P; a.means = means; a.covs = covs; a.means_p = means_p; a.covs_p = covs_p;
    a.status = status;
    a.T = desc->T;
    a.do_predict = 1;
    a.do_update = 1;
    if (ex) {
        a.y_out = ex->y; a.K_out = ex->K; a.S_out = ex->S; a.SI_out = ex->SI;
        a.ll_out = ex->log_likelihood; a.maha_out = ex->mahalanobis;
        a.extras_per_step = 1;
    }
    return run_kf(desc, a, stream);
}

int fk_kf_predict_f64(const fk_kf_desc *desc, const double *F, const double *Q, const double *B,
                      const double *u, double *x, double *P, int32_t *status, void *stream)
{
    if (int rc = check_kf_desc(desc)) return rc;
    if (desc->N == 0) return FK_OK;                 // an empty bank: nothing to read, nothing to touch
    if (!F || !Q || !x || !P) return fail(FK_ERR_BAD_ARG, "F,Q,x,P must not be NULL");
    if (int rc = check_control(desc, B, u)) return rc;
    KfArgs a{};
    a.F = F; a.Q = Q; a.B = B; a.u = u; a.x = x; a.P = P; a.status = status;
    a.T = 1;
    a.do_predict = 1;
    a.do_update = 0;
    return run_kf(desc, a, stream);
}

int fk_kf_update_f64(const fk_kf_desc *desc, const double *H, const double *R, const double *z,
                     const uint8_t *mask, double *x, double *P, double *y, double *K, double *S,
                     double *SI, int32_t *status, void *stream)
{
    if (int rc = check_kf_desc(desc)) return rc;
    if (desc->N == 0) return FK_OK;                 // an empty bank: nothing to read, nothing to touch
    if (!H || !R || !z || !x || !P) return fail(FK_ERR_BAD_ARG, "H,R,z,x,P must not be NULL");
    KfArgs a{};
    a.H = H; a.R = R; a.z = z; a.mask = mask; a.x = x; a.P = P;
    a.y_out = y; a.K_out = K; a.S_out = S; a.SI_out = SI; a.status = status;
    a.T = 1;
    a.do_predict = 0;
    a.do_update = 1;
    fk_kf_desc d = *desc;
    d.nu = 0;
    if (d.flags & (FK_KF_FLAG_S_ONLY | FK_KF_FLAG_SI_GIVEN)) {
        const int gm = check_given(&d, FK_KF_FLAG_S_ONLY, FK_KF_FLAG_SI_GIVEN, "FK_KF_FLAG_S_ONLY and FK_KF_FLAG_SI_GIVEN exclude each other",
                                   y && S, "FK_KF_FLAG_S_ONLY: y and S must not be NULL", SI, "FK_KF_FLAG_SI_GIVEN: SI (the input) must not be NULL",
                                   d.n <= 16 && d.m <= 8);
        if (gm < 0) return gm;
        fill(a, &d, d.N);
        return launch_kf_given(a, d.layout, uniform_model(&d), gm, (hipStream_t)stream);
    }
    return run_kf(&d, a, stream);
}

int fk_kf_rts_f64(const fk_kf_desc *desc, const double *F, const double *Q, const double *Xs,
                  const double *Ps, double *xs, double *Ps_out, double *K, double *Pp,
                  int32_t index_convention, int32_t *status, void *stream)
{
    if (int rc = check_kf_desc(desc)) return rc;
    if (desc->N == 0 || desc->T == 0) return FK_OK;                 // an empty bank / an empty run: nothing to read, nothing to touch
    if (!F || !Q || !Xs || !Ps || !xs || !Ps_out) return fail(FK_ERR_BAD_ARG, "F,Q,Xs,Ps,xs,Ps_out must not be NULL");
    if (index_convention != 0 && index_convention != 1) return fail(FK_ERR_BAD_ARG, "index_convention must be 0 or 1");
    const RtsEntry *general = pick_general(rts_table, desc->n);
    if (!general) return fail(FK_ERR_UNSUPPORTED, "dim_x outside the compiled range (<= 16)");
    RtsArgs a{};
    a.F = F; a.Q = Q; a.Xs = Xs; a.Ps = Ps; a.xs = xs; a.Ps_out = Ps_out; a.K = K; a.Pp = Pp;
    a.status = status;
    a.N = desc->N; a.T = desc->T; a.n = desc->n;
    a.model_t = model_per_step(desc);
    a.conv_off = index_convention == 0 ? 1 : 0;                     // (i0 = cnt = 0: all N)
    if (desc->flags & (FK_KF_FLAG_PP_ONLY | FK_KF_FLAG_PPINV_GIVEN)) {
        const int gm = check_given(desc, FK_KF_FLAG_PP_ONLY, FK_KF_FLAG_PPINV_GIVEN, "FK_KF_FLAG_PP_ONLY and FK_KF_FLAG_PPINV_GIVEN exclude each other",
                                   Pp, "FK_KF_FLAG_PP_ONLY: Pp must not be NULL", K, "FK_KF_FLAG_PPINV_GIVEN: K (inverses in, gains out) must not be NULL",
                                   true);     // (dim_x: refused above; dim_z is not read)
        if (gm < 0) return gm;
        a.cnt = desc->N;
        return launch_rts_given(a, desc->layout, uniform_model(desc), gm, (hipStream_t)stream);
    }
    return walk_windows(desc, a, 0, [&](RtsArgs &b, long cnt) {
        b.cnt = cnt;
        return route_rts(desc, b, general, (hipStream_t)stream);
    });
}

// The two variants (kf_variants.hip) keep rules and words of their own: sizes below 1 are FK_ERR_UNSUPPORTED, K / M is shared
// or per track, the record block may reach 4 GiB exactly, and an empty bank is FK_OK only after the pointers are there.

int fk_kf_steadystate_f64(const fk_kf_desc *d, const double *F, const double *H, const double *K, const double *B,
                          const double *u, const double *z, const uint8_t *mask, double *x, double *means, double *means_p,
                          double *y_out, void *stream)
{
    if (!d) return fail(FK_ERR_BAD_ARG, "desc is NULL");
    if (d->n < 1 || d->n > 16 || d->m < 1 || d->m > 8 || d->nu < 0 || d->nu > 4)
        return fail(FK_ERR_UNSUPPORTED, "steady state: dim_x 1..16, dim_z 1..8, dim_u 0..4");
    if (d->layout != FK_LAYOUT_AOS && d->layout != FK_LAYOUT_SOA) return fail(FK_ERR_BAD_ARG, "steady state: bad layout");
    if (d->model_mode != FK_MODEL_SHARED && d->model_mode != FK_MODEL_PER_TRACK)
        return fail(FK_ERR_UNSUPPORTED, "steady state: K is shared or per track");
    if (d->N < 0 || d->T < 0 || !x || (!F && !z) || (z && (!H || !K)) || (d->nu > 0 && F && (!B || !u)))
        return fail(FK_ERR_BAD_ARG, "steady state: bad argument");
    if (int rc = check_record_block((double)d->N, (double)d->n * d->m, FK_4GIB, "steady state: record block >= 4 GiB")) return rc;
    if (d->N == 0 || d->T == 0) return FK_OK;
    SteadyArgs a{};
    a.F = F; a.H = H; a.K = K; a.B = (d->nu > 0 && F) ? B : nullptr; a.u = u; a.z = z; a.mask = mask;
    a.x = x; a.means = means; a.means_p = means_p; a.y_out = y_out; a.N = d->N; a.T = d->T;
    a.n = d->n; a.m = d->m; a.nu = d->nu; a.k_per_track = d->model_mode == FK_MODEL_PER_TRACK && K != nullptr;
    return launch_steady(a, d->layout, (hipStream_t)stream);
}

int fk_kf_update_correlated_f64(const fk_kf_desc *d, const double *H, const double *R, const double *M, const double *z,
                                const uint8_t *mask, double *x, double *P, double *y, double *K, double *S, double *SI,
                                int32_t *status, void *stream)
{
    if (!d) return fail(FK_ERR_BAD_ARG, "desc is NULL");
    if (d->n < 1 || d->n > 16 || d->m < 1 || d->m > 8) return fail(FK_ERR_UNSUPPORTED, "update_correlated: dim_x 1..16, dim_z 1..8");
    if (d->layout != FK_LAYOUT_AOS && d->layout != FK_LAYOUT_SOA) return fail(FK_ERR_BAD_ARG, "update_correlated: bad layout");
    if (d->model_mode != FK_MODEL_SHARED && d->model_mode != FK_MODEL_PER_TRACK)
        return fail(FK_ERR_UNSUPPORTED, "update_correlated: M is shared or per track");
    if (d->N < 0 || !H || !R || !M || !z || !x || !P) return fail(FK_ERR_BAD_ARG, "update_correlated: bad argument");
    if (int rc = check_record_block((double)d->N, (double)d->n * d->n, FK_4GIB, "update_correlated: record block >= 4 GiB")) return rc;
    if (d->N == 0) return FK_OK;
    return launch_corr_update(d->n, d->m, (long)d->N, d->layout, H, R, M, d->model_mode == FK_MODEL_PER_TRACK, z, mask, x, P, y, K,
                              S, SI, status, (hipStream_t)stream);
}

}  // extern "C"
