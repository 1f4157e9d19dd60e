// imm_dispatch.cpp -- C ABI entry of the batched IMM estimator: argument checks and the choice of
// the (dim_x, dim_z, n_models) instantiation of imm_kernels.hip.
#include "fk_dispatch.hpp"
#include "fk_chunks.hpp"
#include "fk_kernel_args.hpp"

using namespace fk;

// imm_kernels.hip: register-resident instantiations for the small banks (fk_dims_imm.def: 2 / 3 filters, dim_x <= 6, dim_z <= 3),
// each with the waves per SIMD its compiled output sets are tuned for
#define FK_IMM_INST(NX, NZ, NM, W) void launch_imm_##NX##_##NZ##_##NM(const ImmArgs &, int, int, hipStream_t);
#include "fk_dims_imm.def"
#undef FK_IMM_INST
struct ImmSmallEntry {
    int nx, nz, nm, waves;
    void (*fn)(const ImmArgs &, int, int, hipStream_t);
};
static const ImmSmallEntry small_table[] = {
#define FK_IMM_INST(NX, NZ, NM, W) {NX, NZ, NM, W, launch_imm_##NX##_##NZ##_##NM},
#include "fk_dims_imm.def"
#undef FK_IMM_INST
};

// the smallest class that holds the filters of a bank of exactly n_models, or nullptr
static const ImmSmallEntry *pick_small(int n, int m, int n_models)
{
    const ImmSmallEntry *best = nullptr;
    for (const ImmSmallEntry &e : small_table)
        if (e.nm == n_models && e.nx >= n && e.nz >= m && (!best || e.nx < best->nx)) best = &e;
    return best;
}

// imm_lanes.hip: one lane per filter of a bank (round 6), classes (4, 2), (6, 3), (9, 4); imm_quad.hip: four lanes per filter,
// classes (12, 4) and (16, 8).  Every bank size 2..16 each: one object per lanes-per-bank step g2 / g4 / g8 / g16 (a bank of
// n_models runs on the smallest that holds it) and per call kind -- x0: the plain call; x1: the instantiation that also
// carries MMAE, missing measurements, the control input and the single-phase calls.
using ImmBankFn = int (*)(const ImmArgs &, int, int, hipStream_t);
struct ImmBankClass {
    int nx, nz;
    ImmBankFn fn[4][2];     // [bank-size step][extended]
};
#define FK_IMM_BANK_DECL(FAM, NX, NZ, G)                                                                               \
    int launch_imm_##FAM##_##NX##_##NZ##_g##G##_x0(const ImmArgs &, int, int, hipStream_t);                             \
    int launch_imm_##FAM##_##NX##_##NZ##_g##G##_x1(const ImmArgs &, int, int, hipStream_t);
#define FK_IMM_BANK_PAIR(FAM, NX, NZ, G) {launch_imm_##FAM##_##NX##_##NZ##_g##G##_x0, launch_imm_##FAM##_##NX##_##NZ##_g##G##_x1}
#define FK_IMM_BANK_CLASS(FAM, NX, NZ)                                                                                 \
    FK_IMM_BANK_DECL(FAM, NX, NZ, 2) FK_IMM_BANK_DECL(FAM, NX, NZ, 4) FK_IMM_BANK_DECL(FAM, NX, NZ, 8) FK_IMM_BANK_DECL(FAM, NX, NZ, 16) \
    static const ImmBankClass FAM##_##NX##_##NZ{NX, NZ, {FK_IMM_BANK_PAIR(FAM, NX, NZ, 2), FK_IMM_BANK_PAIR(FAM, NX, NZ, 4),          \
                                                        FK_IMM_BANK_PAIR(FAM, NX, NZ, 8), FK_IMM_BANK_PAIR(FAM, NX, NZ, 16)}};
FK_IMM_BANK_CLASS(lanes, 4, 2)
FK_IMM_BANK_CLASS(lanes, 6, 3)
FK_IMM_BANK_CLASS(lanes, 9, 4)
FK_IMM_BANK_CLASS(quad, 12, 4)
FK_IMM_BANK_CLASS(quad, 16, 8)
// the same unit built with EIGHT lanes per filter (FK_IQ_LPF=8): the class (16, 8), banks of two filters -- where it is the faster one
// (x, P, mu out: 7.2 -> 6.4 ms per 1e6 bank-steps; banks of four: the same, of eight: slower; docs/KERNEL_NOTES.md)
FK_IMM_BANK_DECL(oct, 16, 8, 2)
static const ImmBankFn oct_16_8[2] = FK_IMM_BANK_PAIR(oct, 16, 8, 2);
#undef FK_IMM_BANK_CLASS
#undef FK_IMM_BANK_PAIR
#undef FK_IMM_BANK_DECL
static const ImmBankClass *const lanes_classes[] = {&lanes_4_2, &lanes_6_3, &lanes_9_4};       // smallest first
static const ImmBankClass *const quad_classes[] = {&quad_12_4, &quad_16_8};

// what only the x1 instantiations carry
static bool extended(const ImmArgs &a) { return a.mmae || a.mask || a.ll0 || a.nu > 0 || a.phase != FK_IMM_STEP; }
// lanes-per-bank step of a bank: 2, 4, 8 or 16 = 2 << step (a wave holds 64 >> (step + 1) banks)
static int bank_step(int n_models) { return n_models <= 2 ? 0 : n_models <= 4 ? 1 : n_models <= 8 ? 2 : 3; }

// the launcher of the smallest class that holds the filters (the last one where none does: its launcher answers NOT_SERVED)
template <size_t K>
static ImmBankFn pick_bank(const ImmBankClass *const (&classes)[K], const ImmArgs &a, int n_models)
{
    const ImmBankClass *c = classes[K - 1];
    for (size_t i = K; i-- > 0;)
        if (a.n <= classes[i]->nx && a.m <= classes[i]->nz) c = classes[i];
    return c->fn[bank_step(n_models)][extended(a)];
}

extern "C" int fk_imm_batch_f64(const fk_imm_desc *d, const double *F, const double *Q, const double *H,
                                const double *R, const double *M, const double *z, double *xs, double *Ps,
                                double *mu, double *x_out, double *P_out, double *mu_out, double *x_prior_out,
                                double *P_prior_out, double *likelihood_out, int32_t *status, void *stream)
{
    return fk_imm_batch_ex_f64(d, F, Q, H, R, M, z, nullptr, nullptr, 0, nullptr, nullptr, xs, Ps, mu, x_out, P_out, mu_out, x_prior_out,
                                   P_prior_out, likelihood_out, status, stream);
}

extern "C" int fk_imm_batch_ex_f64(const fk_imm_desc *d, const double *F, const double *Q, const double *H,
                                       const double *R, const double *M, const double *z, const uint8_t *zmask,
                                       double *ll0, int32_t nu, const double *B, const double *u, double *xs, double *Ps,
                                       double *mu, double *x_out, double *P_out,
                                       double *mu_out, double *x_prior_out, double *P_prior_out, double *likelihood_out,
                                       int32_t *status, void *stream)
{
    if (!d) return fail(FK_ERR_BAD_ARG, "desc is NULL");
    if (d->n < 1 || d->n > 16 || d->m < 1 || d->m > 8 || d->n_models < 2 || d->n_models > 16)
        return fail(FK_ERR_UNSUPPORTED, "IMM: dim_x 1..16, dim_z 1..8, 2..16 models");
    if (d->layout != FK_LAYOUT_AOS && d->layout != FK_LAYOUT_SOA) return fail(FK_ERR_BAD_ARG, "IMM: bad layout");
    if (d->phase < FK_IMM_STEP || d->phase > FK_IMM_UPDATE) return fail(FK_ERR_BAD_ARG, "IMM: bad phase");
    const bool needs_z = (d->phase == FK_IMM_STEP && d->T > 0) || d->phase == FK_IMM_UPDATE;
    if (d->N < 0 || d->T < 0 || !F || !Q || !H || !R || (!M && !(d->flags & FK_IMM_FLAG_MMAE)) || !xs || !Ps || !mu || (needs_z && !z))
        return fail(FK_ERR_BAD_ARG, "IMM: bad argument");
    if (int rc = check_record_block((double)d->N * d->n_models, (double)d->n * d->n, FK_4GIB, "IMM: record block >= 4 GiB, split the batch"))
        return rc;
    if (d->N == 0) return FK_OK;
    ImmArgs a{};
    a.F = F; a.Q = Q; a.H = H; a.R = R; a.Mt = M;
    a.z = z ? z : xs;   // predict-only: the measurement is read but never used
    a.xs = xs; a.Ps = Ps; a.mu = mu;
    a.x_out = x_out; a.P_out = P_out; a.mu_out = mu_out; a.xp_out = x_prior_out; a.Pp_out = P_prior_out;
    a.L_out = likelihood_out; a.status = status; a.N = d->N; a.T = d->phase == FK_IMM_STEP ? d->T : 1;
    a.n = d->n; a.m = d->m; a.phase = d->phase; a.mmae = (d->flags & FK_IMM_FLAG_MMAE) ? 1 : 0;
    a.mask = zmask; a.ll0 = ll0;
    if (nu < 0 || nu > 4 || (nu > 0 && (!B || !u))) return fail(FK_ERR_BAD_ARG, "IMM: control input needs 1 <= dim_u <= 4, B and u");
    a.nu = nu; a.B = B; a.u = u;
    if (a.mmae && (x_prior_out || P_prior_out)) return fail(FK_ERR_BAD_ARG, "MMAE: prior outputs are not defined");
    // which compiled output set (if any) the given pointers form; the single-phase calls use the
    // run-time-tested kernel (one step, launch-bound anyway)
    const int post = (x_out && P_out && mu_out) ? 1 : ((x_out || P_out || mu_out) ? -1 : 0);
    const int prior = (x_prior_out && P_prior_out) ? 2 : ((x_prior_out || P_prior_out) ? -1 : 0);
    int mask = (post < 0 || prior < 0) ? -1 : (post | prior | (likelihood_out ? 4 : 0));
    if (mask != 0 && mask != 1 && mask != 7) mask = -1;
    if (extended(a)) mask = -1;     // the general kernel also carries the MMAE arithmetic, the missing-measurement bookkeeping and the control input
    a.i0 = 0; a.cnt = d->N; a.status_or = 0;
    const int layout = d->layout, n_models = d->n_models;
    const ImmSmallEntry *small = pick_small(d->n, d->m, n_models);
    // Every other bank, 2..16 filters, IMM or MMAE, missing measurements, control input and the single-phase calls included: one lane per
    // FILTER up to dim_x 9 / dim_z 4 (imm_lanes.hip), FOUR lanes per filter above (imm_quad.hip).  FK_IMM_LANES=2: the small banks on
    // imm_lanes.hip too (the A/B of tests/test_gpu_imm.py).
    static const int lanes_mode = [] { const char *v = getenv("FK_IMM_LANES"); return v ? atoi(v) : 1; }();
    const bool quad = !(d->n <= 9 && d->m <= 4);
    const bool lanes = (lanes_mode > 1 || !small) && !quad;
    auto one = [&](const ImmArgs &b, hipStream_t s) -> int {
        if (lanes && pick_bank(lanes_classes, b, n_models)(b, n_models, layout, s) == 0) return check_launch("imm_lanes_kernel");
        if (quad) {
            // (the class (16, 8) with two filters: eight lanes per filter; FK_IMM_OCT=0: four, the A/B)
            static const int oct_mode = [] { const char *v = getenv("FK_IMM_OCT"); return v ? atoi(v) : 1; }();
            const bool oct = !(b.n <= 12 && b.m <= 4) && oct_mode > 0 && n_models <= 2;
            const ImmBankFn fn = oct ? oct_16_8[extended(b)] : pick_bank(quad_classes, b, n_models);
            if (fn(b, n_models, layout, s) == 0) return check_launch("imm_quad_kernel");
        }
        if (!small) return fail(FK_ERR_UNSUPPORTED, "IMM: no kernel holds this bank");      // (not reached: the three families cover dim_x <= 16, dim_z <= 8, 2..16 filters)
        small->fn(b, layout, mask, s);
        return check_launch("imm_kernel");
    };
    hipStream_t s = (hipStream_t)stream;
    if (d->phase != FK_IMM_STEP || a.T < 2) return one(a, s);
    // tail filling (fk_chunks.hpp, imm_chunked_call): wave slots of the instantiation the call runs on -- the compiled output
    // sets of the small banks at their FK_IMM_WAVES per SIMD (fk_dims_imm.def), everything else at one
    // (the lanes kernel: a wave holds 64 / G banks, G = the bank size rounded up to a power of two)
    const int lanes_g = 2 << bank_step(n_models);
    const long slots = quad ? 256L / lanes_g : lanes ? 1024L / lanes_g : 1024L * ((small && mask >= 0) ? small->waves : 1);
    return imm_chunked_call(a, d->n, d->m, n_models, slots, one, s);
}
