// fls_dispatch.cpp -- C-ABI entry point of the fixed-lag smoother and its choice of kernel.
//
// fk_fls_batch_f64 <- FixedLagSmoother.smooth_batch / smooth  (filterpy/kalman/fixed_lag_smoother.py:133-311)
#include <hip/hip_runtime.h>
#include <stdlib.h>

#include "../../include/filterhip.h"
#include "fk_device.hpp"
#include "fk_fls.hpp"

namespace fk {

#define FK_FLS_INST(NX, NZ, L) int launch_fls_fast_##NX##_##NZ##_##L(const FlsArgs &, int, hipStream_t);
#include "fk_dims_fls.def"
#undef FK_FLS_INST
int launch_fls_general(const FlsArgs &, int, hipStream_t);

struct FlsEntry {
    int nx, nz, lmax;
    int (*fn)(const FlsArgs &, int, hipStream_t);
};
static const FlsEntry fls_table[] = {
#define FK_FLS_INST(NX, NZ, L) {NX, NZ, L, launch_fls_fast_##NX##_##NZ##_##L},
#include "fk_dims_fls.def"
#undef FK_FLS_INST
};

static int fail(int code, const char *msg)
{
    set_last_error(msg);
    return code;
}

// The fast kernel serves exact (n, m) with max(lag, 1) <= LMAX; FK_FLS_GENERAL=1 in the environment forces the general
// kernel (A/B and tests).  Nothing else enters the choice: chained calls run the kernel one call would.
static const FlsEntry *pick_fls(int n, int m, int lag)
{
    const char *ev = getenv("FK_FLS_GENERAL");
    if (ev && atoi(ev) != 0) return nullptr;
    const int Lf = lag > 1 ? lag : 1;
    for (const FlsEntry &e : fls_table)
        if (e.nx == n && e.nz == m && Lf <= e.lmax) return &e;
    return nullptr;
}

}  // namespace fk

using namespace fk;

extern "C" int fk_fls_batch_f64(const fk_kf_desc *desc, int32_t lag, int64_t k0,
                                const double *F, const double *Q, const double *H, const double *R,
                                const double *B, const double *u, const double *z,
                                double *x, double *P, double *xs, double *xhat,
                                double *y, double *S, int32_t *status, void *stream)
{
    if (!desc) return fail(FK_ERR_BAD_ARG, "desc is NULL");
    const fk_kf_desc *d = desc;
    if (d->n < 1 || d->m < 1 || d->nu < 0) return fail(FK_ERR_BAD_ARG, "dim_x, dim_z must be >= 1, dim_u >= 0");
    if (d->N < 0 || d->T < 0 || k0 < 0) return fail(FK_ERR_BAD_ARG, "N, T and k0 must be >= 0");
    if (d->layout != FK_LAYOUT_AOS && d->layout != FK_LAYOUT_SOA) return fail(FK_ERR_BAD_ARG, "bad layout");
    if (d->n > 16 || d->m > 8) return fail(FK_ERR_UNSUPPORTED, "dim_x/dim_z outside the compiled range (dim_x <= 16, dim_z <= 8)");
    if (d->model_mode != FK_MODEL_SHARED) return fail(FK_ERR_UNSUPPORTED, "fixed-lag smoother: FK_MODEL_SHARED only");
    if (d->update_first != 0 || d->alpha_sq != 1.0) return fail(FK_ERR_UNSUPPORTED, "fixed-lag smoother: update_first 0 and alpha_sq 1 only");
    if (d->flags & ~FK_KF_FLAG_R_JOSEPH_DIAG) return fail(FK_ERR_UNSUPPORTED, "fixed-lag smoother: flags 0 or FK_KF_FLAG_R_JOSEPH_DIAG only");
    if (d->N == 0 || d->T == 0) return FK_OK;                 // nothing to read, nothing to touch
    if (!F || !Q || !H || !R || !z || !x || !P || !xs || !xhat) return fail(FK_ERR_BAD_ARG, "F,Q,H,R,z,x,P,xs,xhat must not be NULL");
    if (d->nu > 0 && (!B || !u)) return fail(FK_ERR_BAD_ARG, "dim_u > 0 needs B and u");
    // one step's record block is addressed with 32-bit byte offsets (fk_device.hpp)
    long E = (long)d->n * (d->n > d->m ? d->n : d->m);
    if (d->nu > E) E = d->nu;
    if ((double)d->N * (double)E * 8.0 >= 4294967264.0) return fail(FK_ERR_UNSUPPORTED, "N * dim^2 * 8 bytes must stay below 4 GiB (split the bank)");
    FlsArgs a{};
    a.F = F; a.Q = Q; a.H = H; a.R = R; a.B = d->nu > 0 ? B : nullptr; a.u = d->nu > 0 ? u : nullptr; a.z = z;
    a.x = x; a.P = P; a.xs = xs; a.xhat = xhat; a.y = y; a.S = S; a.status = status;
    a.N = d->N; a.T = d->T; a.k0 = k0;
    const long Lf = lag > 1 ? lag : 1;
    a.W = Lf - 1 < k0 ? Lf - 1 : k0;
    a.n = d->n; a.m = d->m; a.nu = d->nu; a.lag = lag;
    a.rj_diag = (d->flags & FK_KF_FLAG_R_JOSEPH_DIAG) ? 1 : 0;
    const FlsEntry *e = pick_fls(d->n, d->m, lag);
    return e ? e->fn(a, d->layout, (hipStream_t)stream) : launch_fls_general(a, d->layout, (hipStream_t)stream);
}
