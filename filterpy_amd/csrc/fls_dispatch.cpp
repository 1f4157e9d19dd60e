// fls_dispatch.cpp -- C-ABI entry point of the fixed-lag smoother and its choice of kernel.
//
// fk_fls_batch_f64 <- FixedLagSmoother.smooth_batch / smooth  (filterpy/kalman/fixed_lag_smoother.py:133-311)
#include "fk_dispatch.hpp"
#include "fk_fls.hpp"

namespace fk {

#define FK_FLS_INST(NX, NZ, L) int launch_fls_fast_##NX##_##NZ##_##L(const FlsArgs &, int, hipStream_t);
#include "fk_dims_fls.def"
#undef FK_FLS_INST
int launch_fls_general(const FlsArgs &, int, hipStream_t);

static const FastEntry<FlsArgs> fls_table[] = {
#define FK_FLS_INST(NX, NZ, L) {NX, NZ, L, launch_fls_fast_##NX##_##NZ##_##L},
#include "fk_dims_fls.def"
#undef FK_FLS_INST
};

static const Family FLS{"fixed-lag smoother", /*update_first*/ false, /*flags*/ FK_KF_FLAG_R_JOSEPH_DIAG, /*k0*/ true};

}  // namespace fk

using namespace fk;

extern "C" int fk_fls_batch_f64(const fk_kf_desc *desc, int32_t lag, int64_t k0,
                                const double *F, const double *Q, const double *H, const double *R,
                                const double *B, const double *u, const double *z,
                                double *x, double *P, double *xs, double *xhat,
                                double *y, double *S, int32_t *status, void *stream)
{
    int rc = check_desc(desc, FLS, true, k0);
    if (rc != FK_OK) return rc;
    const fk_kf_desc *d = desc;
    if (d->N == 0 || d->T == 0) return FK_OK;                 // nothing to read, nothing to touch
    if (!F || !Q || !H || !R || !z || !x || !P || !xs || !xhat) return fail(FK_ERR_BAD_ARG, "F,Q,H,R,z,x,P,xs,xhat must not be NULL");
    if ((rc = check_control(d, B, u)) != FK_OK) return rc;
    // the widest record is P (n x n) or K (n x m): narrower than the filters' max(n, m)^2
    if ((rc = check_record_block(d, (long)d->n * (d->n > d->m ? d->n : d->m))) != FK_OK) return rc;
    FlsArgs a{};
    a.F = F; a.Q = Q; a.H = H; a.R = R; a.B = d->nu > 0 ? B : nullptr; a.u = d->nu > 0 ? u : nullptr; a.z = z;
    a.x = x; a.P = P; a.xs = xs; a.xhat = xhat; a.y = y; a.S = S; a.status = status;
    a.N = d->N; a.T = d->T; a.k0 = k0;
    const long Lf = lag > 1 ? lag : 1;
    a.W = Lf - 1 < k0 ? Lf - 1 : k0;
    a.n = d->n; a.m = d->m; a.nu = d->nu; a.lag = lag;
    a.rj_diag = (d->flags & FK_KF_FLAG_R_JOSEPH_DIAG) ? 1 : 0;
    // the fast kernel serves exact (n, m) with max(lag, 1) <= LMAX
    const FastEntry<FlsArgs> *e = pick_fast(fls_table, "FK_FLS_GENERAL", d->n, d->m, (int)Lf);
    return e ? e->fn(a, d->layout, (hipStream_t)stream) : launch_fls_general(a, d->layout, (hipStream_t)stream);
}
