// ukf_dispatch.cpp -- C-ABI entry points of the unscented Kalman filter and their choice of launcher.
//
// fk_ukf_linear_batch_f64 / _rts_f64 <- UnscentedKalmanFilter.batch_filter / rts_smoother with fx = F, hx = H (ukf_kernels.hip,
//                                        ukf_mlg.hip); fk_ukf_linear_supported: which sizes they take (the host side asks first)
// fk_ut_*_f64, fk_ukf_correct_f64     <- the building blocks of a filter with arbitrary fx / hx (ut_kernels.hip)
// fk_ukf_rts_correct_f64              <- the gain / correction of rts_smoother (kf_variants.hip)
// FK_UKF_FLAG_SIMPLEX: the same two calls on the n + 1 points of SimplexSigmaPoints (ukf_simplex.hip), a route of its own below.
// These calls keep rules and words of their own (no check_desc): tests/test_host_refusals.py pins each branch and its place.
#include "fk_dispatch.hpp"
#include "fk_chunks.hpp"
#include "fk_launchers.hpp"
#include "fk_ukf_simplex.hpp"

namespace fk {

// ukf_mlg.hip: four / eight lanes per track, one object per dim_x of fk_dims_ukf.def (NOT_SERVED: not this object's call)
struct UmlgEntry {
    static constexpr int nz = 0;
    int nx;
    int (*fwd)(const UkfArgs &, int, hipStream_t);
    int (*rts)(const UkfRtsArgs &, const double *, const double *, const double *, const double *, int, hipStream_t);
};
#define FK_UKF_MLG_DIM(NX)                                        \
    int launch_ukf_mlg_##NX(const UkfArgs &, int, hipStream_t); \
    int launch_ukf_mlg_rts_##NX(const UkfRtsArgs &, const double *, const double *, const double *, const double *, int, hipStream_t);
#include "fk_dims_ukf.def"
#undef FK_UKF_MLG_DIM
static const UmlgEntry umlg_table[] = {
#define FK_UKF_MLG_DIM(NX) {NX, launch_ukf_mlg_##NX, launch_ukf_mlg_rts_##NX},
#include "fk_dims_ukf.def"
#undef FK_UKF_MLG_DIM
};

// Which calls the several-lane kernels serve, decided by measurement (profiles/r05/ukf_mlg/):
//   filter:   dim_x 10..16 (no one-lane kernel exists there); at 7..9 the one-lane classes are faster (8: 1.9 vs 2.8 ms, 9: 2.2
//             vs 4.4 ms at N = 1e5, T = 100) and keep the call;
//   smoother: dim_x 10..16, and 7..9 too for pair-weight callers (8: 5.1 / 8.2 -> 4.4 / 4.1 ms, 9: 10.3 / 13.8 -> 7.8 / 7.4 ms
//             element-major / NumPy order): the one-lane smoother classes run one wave per SIMD with 0.4-1.3 KB of scratch.
// A/B knobs, ONE snapshot per process (fk_ukf_linear_supported and the two calls must agree): FK_UKF_MLG=0 takes
// the several-lane kernels out altogether (dim_x >= 10 then answers FK_ERR_UNSUPPORTED and the host takes the building
// blocks); FK_UKF_MLG_MIN_NX / FK_UKF_MLG_RTS_MIN_NX = 7..10 move the filter's / the smoother's lower bound.
struct UkfMlgRoute { int fwd_min, rts_min; };
static UkfMlgRoute ukf_mlg_route()
{
    static const UkfMlgRoute v = [] {
        const char *on = getenv("FK_UKF_MLG");
        if (on && on[0] == '0') return UkfMlgRoute{99, 99};
        auto knob = [](const char *name, int dflt) {
            const char *mn = getenv(name);
            const int m = mn ? atoi(mn) : dflt;
            return m >= 7 && m <= 10 ? m : dflt;
        };
        return UkfMlgRoute{knob("FK_UKF_MLG_MIN_NX", 10), knob("FK_UKF_MLG_RTS_MIN_NX", 7)};
    }();
    return v;
}

// FK_UKF_PADDED=1: the padded instantiations also at the exact dims (A/B, and the parity tests of the padded path)
static bool ukf_exact()
{
    static const bool padded = [] { const char *v = getenv("FK_UKF_PADDED"); return v && v[0] == '1'; }();
    return !padded;
}

// The pair-regrouped kernels run when the caller asserts weights equal within every +- pair (FK_UKF_FLAG_PAIR_WEIGHTS);
// FK_UKF_PAIRED=0 keeps the index-order sums for every call (A/B, and the parity tests of that path).
static bool ukf_paired(const fk_ukf_desc *d)
{
    static const bool off = [] { const char *v = getenv("FK_UKF_PAIRED"); return v && v[0] == '0'; }();
    return !off && (d->flags & FK_UKF_FLAG_PAIR_WEIGHTS) != 0;
}

// FK_UKF_FLAG_SIMPLEX: the sizes the one-lane simplex kernels (ukf_simplex.hip) take -- the one-lane table of the other point
// sets; nothing at dim_x 10..16, no switch
static bool simplex_sizes(int n, int m, bool smoother)
{
    if (smoother) return n >= 1 && n <= 9;
    return (n >= 1 && n <= 6 && m >= 1 && m <= 3) || (n >= 7 && n <= 9 && m >= 1 && m <= 4);
}

// The two fused calls with FK_UKF_FLAG_SIMPLEX: refusals in the order of the other route (size, bad argument, the 4 GiB guard,
// nothing to do), then ONE launch.  Wm / Wc hold n + 1 weights, desc.scale is not read, FK_UKF_FLAG_PAIR_WEIGHTS is ignored.
static int ukf_simplex_batch(const fk_ukf_desc *d, const double *F, const double *H, const double *Q, const double *R,
                             const double *Wm, const double *Wc, const double *z, const uint8_t *mask, double *x, double *P,
                             double *means, double *covs, int32_t *status, void *stream)
{
    if (!simplex_sizes(d->n, d->m, false))
        return fail(FK_ERR_UNSUPPORTED, "fused linear UKF with FK_UKF_FLAG_SIMPLEX: dim_x 1..6 with dim_z 1..3, dim_x 7..9 with dim_z 1..4");
    if (d->N < 0 || d->T < 0 || !F || !H || !Q || !R || !Wm || !Wc || !z || !x || !P)
        return fail(FK_ERR_BAD_ARG, "fused linear UKF: bad argument");
    if (int rc = check_record_block((double)d->N, (double)d->n * d->n, FK_4GIB - 32.0, "fused linear UKF: record block >= 4 GiB, split the batch"))
        return rc;
    if (d->N == 0 || d->T == 0) return FK_OK;
    UkfArgs a{};
    a.F = F; a.H = H; a.Q = Q; a.R = R; a.Wm = Wm; a.Wc = Wc; a.z = z; a.mask = mask;
    a.x = x; a.P = P; a.means = means; a.covs = covs; a.status = status;
    a.N = d->N; a.T = d->T; a.n = d->n; a.m = d->m; a.scale = 1.0;
    a.i0 = 0; a.cnt = d->N; a.status_or = 0; a.soa_pairs = 0;
    const SimplexTable tab = simplex_table(d->n);
    return (a.n <= 6 && a.m <= 3) ? ukf_simplex_fwd_launch_small(a, tab, d->layout, (hipStream_t)stream)
                                  : ukf_simplex_fwd_launch_big(a, tab, d->layout, (hipStream_t)stream);
}

static int ukf_simplex_rts(const fk_ukf_desc *d, const double *F, const double *Q, const double *Wm, const double *Wc,
                           const double *Xs, const double *Ps, double *xs, double *Ps_out, double *K, int32_t *status, void *stream)
{
    if (!simplex_sizes(d->n, 1, true))
        return fail(FK_ERR_UNSUPPORTED, "fused linear UKF smoother with FK_UKF_FLAG_SIMPLEX: dim_x 1..9");
    if (d->N < 0 || d->T < 0 || !F || !Q || !Wm || !Wc || !Xs || !Ps || !xs || !Ps_out)
        return fail(FK_ERR_BAD_ARG, "fused linear UKF smoother: bad argument");
    if (int rc = check_record_block((double)d->N, (double)d->n * d->n, FK_4GIB, "fused linear UKF smoother: record block >= 4 GiB, split the batch"))
        return rc;
    if (d->N == 0 || d->T == 0) return FK_OK;
    UkfRtsArgs a{};
    a.Xs = Xs; a.Ps = Ps; a.xs = xs; a.ps = Ps_out; a.Ks = K; a.status = status;
    a.N = d->N; a.T = d->T; a.n = d->n; a.scale = 1.0;
    a.i0 = 0; a.cnt = d->N; a.cont = 0; a.status_or = 0;
    const SimplexTable tab = simplex_table(d->n);
    return a.n <= 6 ? ukf_simplex_rts_launch_small(a, tab, F, Q, Wm, Wc, d->layout, (hipStream_t)stream)
                    : ukf_simplex_rts_launch_big(a, tab, F, Q, Wm, Wc, d->layout, (hipStream_t)stream);
}

}  // namespace fk

using namespace fk;

extern "C" {

int fk_ukf_linear_supported(int32_t n, int32_t m, int32_t flags, int32_t smoother)
{
    if (flags & FK_UKF_FLAG_SIMPLEX) return simplex_sizes(n, m, smoother != 0);
    const bool pairw = (flags & FK_UKF_FLAG_PAIR_WEIGHTS) != 0;
    if (smoother) {
        if (n >= 10 && n <= 16) return pairw && ukf_mlg_route().rts_min <= 10;
        return n >= 1 && n <= 9;
    }
    if (n >= 10 && n <= 16) return m >= 1 && m <= 8 && pairw && ukf_mlg_route().fwd_min <= 10;
    return (n >= 1 && n <= 6 && m >= 1 && m <= 3) || (n >= 7 && n <= 9 && m >= 1 && m <= 4);
}

int fk_ukf_linear_batch_f64(const fk_ukf_desc *d, const double *F, const double *H, const double *Q, const double *R,
                            const double *Wm, const double *Wc, const double *z, const uint8_t *mask, double *x, double *P,
                            double *means, double *covs, int32_t *status, void *stream)
{
    if (!d) return fail(FK_ERR_BAD_ARG, "desc is NULL");
    if (d->flags & FK_UKF_FLAG_SIMPLEX) return ukf_simplex_batch(d, F, H, Q, R, Wm, Wc, z, mask, x, P, means, covs, status, stream);
    // dim_x 10..16 (dim_z 1..8): four / eight lanes per track (ukf_mlg.hip), the pair-regrouped sums only
    const int fwd_min = ukf_mlg_route().fwd_min;
    const bool big = d->n >= 10 && d->n <= 16 && d->m >= 1 && d->m <= 8;
    const bool quad = big || (d->n >= fwd_min && d->n <= 9 && d->m >= 1 && d->m <= 4 && (d->flags & FK_UKF_FLAG_PAIR_WEIGHTS) && ukf_paired(d));
    if (big) {
        if (fwd_min > 10 || !(d->flags & FK_UKF_FLAG_PAIR_WEIGHTS))
            return fail(FK_ERR_UNSUPPORTED, "fused linear UKF at dim_x 10..16: needs weights equal within every +- pair (FK_UKF_FLAG_PAIR_WEIGHTS; and FK_UKF_MLG != 0)");
    } else if (d->n < 1 || d->n > 9 || d->m < 1 || d->m > 4 || (d->n <= 6 && d->m > 3))
        return fail(FK_ERR_UNSUPPORTED, "fused linear UKF: dim_x 1..6 with dim_z 1..3, dim_x 7..9 with dim_z 1..4, dim_x 10..16 with dim_z 1..8");
    if (d->N < 0 || d->T < 0 || !F || !H || !Q || !R || !Wm || !Wc || !z || !x || !P)
        return fail(FK_ERR_BAD_ARG, "fused linear UKF: bad argument");
    if (int rc = check_record_block((double)d->N, (double)d->n * d->n, FK_4GIB - 32.0, "fused linear UKF: record block >= 4 GiB, split the batch"))
        return rc;
    if (d->N == 0 || d->T == 0) return FK_OK;
    UkfArgs a0{};
    a0.F = F; a0.H = H; a0.Q = Q; a0.R = R; a0.Wm = Wm; a0.Wc = Wc; a0.z = z; a0.mask = mask;
    a0.x = x; a0.P = P; a0.means = means; a0.covs = covs; a0.status = status;
    a0.N = d->N; a0.T = d->T; a0.n = d->n; a0.m = d->m; a0.scale = d->scale;
    a0.i0 = 0; a0.cnt = d->N; a0.status_or = 0;
    {   // FK_UKF_SOA_PAIRS=0: the element-major outputs as 8-byte stores everywhere (A/B; read per call)
        const char *pv = getenv("FK_UKF_SOA_PAIRS");
        a0.soa_pairs = !(pv && pv[0] == '0');
    }
    const int layout = d->layout;
    const bool exact = ukf_exact(), paired = ukf_paired(d);
    // one piece: tracks [a.i0, a.i0 + a.cnt), a.T steps from the pointers in a.  Classes (2,2), (4,2), (6,3), (8,4), (9,3),
    // (9,4): the exact instantiation where the dims are the class's own, the padded one otherwise.
    auto one = [&](const UkfArgs &a, hipStream_t s) -> int {
        if (quad) {
            const UmlgEntry *e = find_entry(umlg_table, a.n);
            const int rc = e ? e->fwd(a, layout, s) : NOT_SERVED;
            return rc == NOT_SERVED ? fail(FK_ERR_UNSUPPORTED, "fused linear UKF: no four-lane instantiation for these dims") : rc;
        }
        if (paired) return (a.n <= 6 && a.m <= 3) ? ukf_fwd_launch_small_paired(a, layout, exact, s) : ukf_fwd_launch_big_paired(a, layout, exact, s);
        return (a.n <= 6 && a.m <= 3) ? ukf_fwd_launch_small(a, layout, exact, s) : ukf_fwd_launch_big(a, layout, exact, s);
    };
    // one launch unless FK_UKF_CHUNKS="G,H" asks for track groups x time chunks (fk_chunks.hpp; measured no faster:
    // profiles/r03/ukf_chunking.jsonl)
    return ukf_chunked_call(a0, a0.n, a0.m, one, (hipStream_t)stream);
}

int fk_ukf_linear_rts_f64(const fk_ukf_desc *d, const double *F, const double *Q, const double *Wm, const double *Wc,
                          const double *Xs, const double *Ps, double *xs, double *Ps_out, double *K, int32_t *status,
                          void *stream)
{
    const char *const guard = "fused linear UKF smoother: record block >= 4 GiB, split the batch";
    if (!d) return fail(FK_ERR_BAD_ARG, "desc is NULL");
    if (d->flags & FK_UKF_FLAG_SIMPLEX) return ukf_simplex_rts(d, F, Q, Wm, Wc, Xs, Ps, xs, Ps_out, K, status, stream);
    // dim_x 10..16 -- and 7..9 for pair-weight callers (ukf_mlg_route) --: four / eight lanes per track (ukf_mlg.hip), pair-regrouped sums only
    const int rts_min = ukf_mlg_route().rts_min;
    const bool big = d->n >= 10 && d->n <= 16;
    const bool quad = big || (d->n >= rts_min && d->n <= 9 && (d->flags & FK_UKF_FLAG_PAIR_WEIGHTS) && ukf_paired(d));
    if (big) {
        if (rts_min > 10 || !(d->flags & FK_UKF_FLAG_PAIR_WEIGHTS))
            return fail(FK_ERR_UNSUPPORTED, "fused linear UKF smoother at dim_x 10..16: needs weights equal within every +- pair (FK_UKF_FLAG_PAIR_WEIGHTS; and FK_UKF_MLG != 0)");
    } else if (d->n < 1 || d->n > 9) return fail(FK_ERR_UNSUPPORTED, "fused linear UKF smoother: dim_x 1..9, 10..16");
    // (as found: the several-lane route's limit is 32 bytes short of 4 GiB and in front of the pointer checks, the other's not)
    if (quad)
        if (int rc = check_record_block((double)d->N, (double)d->n * d->n, FK_4GIB - 32.0, guard)) return rc;
    if (d->N < 0 || d->T < 0 || !F || !Q || !Wm || !Wc || !Xs || !Ps || !xs || !Ps_out)
        return fail(FK_ERR_BAD_ARG, "fused linear UKF smoother: bad argument");
    if (int rc = check_record_block((double)d->N, (double)d->n * d->n, FK_4GIB, guard)) return rc;
    if (d->N == 0 || d->T == 0) return FK_OK;
    UkfRtsArgs a0{};
    a0.Xs = Xs; a0.Ps = Ps; a0.xs = xs; a0.ps = Ps_out; a0.Ks = K; a0.status = status;
    a0.N = d->N; a0.T = d->T; a0.n = d->n; a0.scale = d->scale;
    a0.i0 = 0; a0.cnt = d->N; a0.cont = 0; a0.status_or = 0;
    const int layout = d->layout;
    if (quad) {
        const UmlgEntry *e = find_entry(umlg_table, a0.n);
        const int rc = e ? e->rts(a0, F, Q, Wm, Wc, layout, (hipStream_t)stream) : NOT_SERVED;
        return rc == NOT_SERVED ? fail(FK_ERR_UNSUPPORTED, "fused linear UKF smoother: no four-lane instantiation for this dim_x") : rc;
    }
    const bool exact = ukf_exact(), paired = ukf_paired(d);
    auto one = [&](const UkfRtsArgs &a, hipStream_t s) -> int {
        if (paired) return a.n <= 6 ? ukf_rts_launch_small_paired(a, F, Q, Wm, Wc, layout, exact, s) : ukf_rts_launch_big_paired(a, F, Q, Wm, Wc, layout, exact, s);
        return a.n <= 6 ? ukf_rts_launch_small(a, F, Q, Wm, Wc, layout, exact, s) : ukf_rts_launch_big(a, F, Q, Wm, Wc, layout, exact, s);
    };
    // Tail filling (fk_chunks.hpp): the classes of dim_x >= 5 run one wave per SIMD, so BASELINE configs[3]'s 1563 waves are
    // two rounds for 1.53 rounds of work; cut into track groups x backward time windows they fill each other's tails.
    const long slots = 1024L * (d->n <= 2 ? 4 : d->n <= 4 ? 2 : 1);
    return ukf_rts_chunked_call(a0, a0.n, slots, one, (hipStream_t)stream);
}

// The building blocks.  None but fk_ukf_rts_correct_f64 looks at layout: whatever is not FK_LAYOUT_SOA runs the NumPy-order
// kernel.  Their record blocks may reach 4 GiB exactly.

int fk_ut_sigma_points_f64(int32_t n, int64_t N, int32_t layout, double scale, const double *x, const double *P, double *sigmas,
                           int32_t *status, void *stream)
{
    if (n < 1 || n > 16) return fail(FK_ERR_UNSUPPORTED, "sigma points: dim_x must be 1..16");
    if (N < 0 || !x || !P || !sigmas) return fail(FK_ERR_BAD_ARG, "sigma points: bad argument");
    if (int rc = check_record_block((double)N, (2.0 * n + 1) * n, FK_4GIB, "sigma points: record block >= 4 GiB, split the batch")) return rc;
    if (N == 0) return FK_OK;
    return launch_ut_points(n, (long)N, layout, scale, x, P, sigmas, status, (hipStream_t)stream);
}

int fk_ut_transform_f64(int32_t n, int32_t k, int64_t N, int32_t layout, const double *sigmas, const double *Wm, const double *Wc,
                        const double *noise_cov, double *x_out, double *P_out, void *stream)
{
    if (n < 1 || n > 16 || k < 1) return fail(FK_ERR_UNSUPPORTED, "unscented transform: dim must be 1..16");
    if (N < 0 || !sigmas || !Wm || !Wc || !x_out || !P_out) return fail(FK_ERR_BAD_ARG, "unscented transform: bad argument");
    if (int rc = check_record_block((double)N, (double)k * n, FK_4GIB, "unscented transform: record block >= 4 GiB, split the batch")) return rc;
    if (N == 0) return FK_OK;
    return launch_ut_transform(n, k, (long)N, layout, sigmas, Wm, Wc, noise_cov, x_out, P_out, (hipStream_t)stream);
}

int fk_ut_cross_variance_f64(int32_t n, int32_t m, int32_t k, int64_t N, int32_t layout, const double *x, const double *z,
                             const double *sigmas_f, const double *sigmas_h, const double *Wc, double *Pxz, void *stream)
{
    if (n < 1 || n > 16 || m < 1 || k < 1) return fail(FK_ERR_UNSUPPORTED, "cross variance: dim_x must be 1..16");
    // (x / z NULL: the caller applied its own residuals, sigmas_f / sigmas_h hold the differences)
    if (N < 0 || !sigmas_f || !sigmas_h || !Wc || !Pxz) return fail(FK_ERR_BAD_ARG, "cross variance: bad argument");
    if (int rc = check_record_block((double)N, (double)k * (n > m ? n : m), FK_4GIB, "cross variance: record block >= 4 GiB, split the batch")) return rc;
    if (N == 0) return FK_OK;
    return launch_ut_cross(n, m, k, (long)N, layout, x, z, sigmas_f, sigmas_h, Wc, Pxz, (hipStream_t)stream);
}

int fk_ut_linear_map_f64(int32_t n_in, int32_t n_out, int32_t k, int64_t N, int32_t layout, const double *M, const double *in,
                         double *out, void *stream)
{
    if (n_in < 1 || n_in > 16 || n_out < 1 || n_out > 16 || k < 1) return fail(FK_ERR_UNSUPPORTED, "linear map: dims must be 1..16");
    if (N < 0 || !M || !in || !out) return fail(FK_ERR_BAD_ARG, "linear map: bad argument");
    if (int rc = check_record_block((double)N, (double)k * (n_in > n_out ? n_in : n_out), FK_4GIB, "linear map: record block >= 4 GiB, split the batch")) return rc;
    if (N == 0) return FK_OK;
    return launch_ut_linear_map(n_in, n_out, k, (long)N, layout, M, in, out, (hipStream_t)stream);
}

int fk_ukf_correct_f64(int32_t n, int32_t m, int64_t N, int32_t layout, const double *Pxz, const double *zp, const double *S,
                       const double *z, double *x, double *P, double *K, int32_t *status, void *stream)
{
    if (n < 1 || n > 16 || m < 1 || m > 8) return fail(FK_ERR_UNSUPPORTED, "ukf correct: dim_x 1..16, dim_z 1..8");
    if (N < 0 || !Pxz || !S || !z || !x || !P) return fail(FK_ERR_BAD_ARG, "ukf correct: bad argument");
    if (int rc = check_record_block((double)N, (double)n * n, FK_4GIB, "ukf correct: record block >= 4 GiB, split the batch")) return rc;
    if (N == 0) return FK_OK;
    return launch_ukf_correct(n, m, (long)N, layout, Pxz, zp, S, z, x, P, K, status, (hipStream_t)stream);
}

int fk_ukf_rts_correct_f64(int32_t n, int64_t N, int32_t layout, const double *Pxb, const double *xb, const double *Pb,
                           const double *xn, const double *Pn, double *x, double *P, double *K, int32_t *status, void *stream)
{
    if (n < 1 || n > 16) return fail(FK_ERR_UNSUPPORTED, "ukf rts: dim_x 1..16");
    if (layout != FK_LAYOUT_AOS && layout != FK_LAYOUT_SOA) return fail(FK_ERR_BAD_ARG, "ukf rts: bad layout");
    if (N < 0 || !Pxb || !Pb || !xn || !Pn || !x || !P) return fail(FK_ERR_BAD_ARG, "ukf rts: bad argument");
    if (int rc = check_record_block((double)N, (double)n * n, FK_4GIB, "ukf rts: record block >= 4 GiB")) return rc;
    if (N == 0) return FK_OK;
    return launch_ukf_rts_correct(n, (long)N, layout, Pxb, xb, Pb, xn, Pn, x, P, K, status, (hipStream_t)stream);
}

}  // extern "C"
