// srkf_dispatch.cpp -- C-ABI entry points of the square-root Kalman filter and their choice of kernel.
//
// fk_srkf_batch_f64    <- SquareRootKalmanFilterBank.batch_filter  (predict / update of filterpy/kalman/square_root.py:172-248,
//                         T steps in one launch)
// fk_srkf_predict_f64  <- SquareRootKalmanFilter.predict           (square_root.py:226-248)
// fk_srkf_update_f64   <- SquareRootKalmanFilter.update            (square_root.py:172-224)
#include <hip/hip_runtime.h>
#include <stdlib.h>

#include "../../include/filterhip.h"
#include "fk_device.hpp"
#include "fk_srkf.hpp"

namespace fk {

#define FK_SRKF_INST(NX, NZ) int launch_srkf_fast_##NX##_##NZ(const SrkfArgs &, int, hipStream_t);
#include "fk_dims_srkf.def"
#undef FK_SRKF_INST
int launch_srkf_general(const SrkfArgs &, int, hipStream_t);

struct SrkfEntry {
    int nx, nz;
    int (*fn)(const SrkfArgs &, int, hipStream_t);
};
static const SrkfEntry srkf_table[] = {
#define FK_SRKF_INST(NX, NZ) {NX, NZ, launch_srkf_fast_##NX##_##NZ},
#include "fk_dims_srkf.def"
#undef FK_SRKF_INST
};

static int fail(int code, const char *msg)
{
    set_last_error(msg);
    return code;
}

// The fast kernel serves exact (n, m); FK_SRKF_GENERAL=1 in the environment forces the general kernel (A/B and tests).  Nothing
// else enters the choice: chained calls run the kernel one call would.
static const SrkfEntry *pick_srkf(int n, int m)
{
    const char *ev = getenv("FK_SRKF_GENERAL");
    if (ev && atoi(ev) != 0) return nullptr;
    for (const SrkfEntry &e : srkf_table)
        if (e.nx == n && e.nz == m) return &e;
    return nullptr;
}

// Everything about desc that does not need a pointer; T is ignored for the single steps (treated as 1).
static int check_desc(const fk_kf_desc *d, bool steps)
{
    if (!d) return fail(FK_ERR_BAD_ARG, "desc is NULL");
    if (d->n < 1 || d->m < 1 || d->nu < 0) return fail(FK_ERR_BAD_ARG, "dim_x, dim_z must be >= 1, dim_u >= 0");
    if (d->N < 0 || (steps && d->T < 0)) return fail(FK_ERR_BAD_ARG, "N and T must be >= 0");
    if (d->layout != FK_LAYOUT_AOS && d->layout != FK_LAYOUT_SOA) return fail(FK_ERR_BAD_ARG, "bad layout");
    if (d->n > 16 || d->m > 8) return fail(FK_ERR_UNSUPPORTED, "dim_x/dim_z outside the compiled range (dim_x <= 16, dim_z <= 8)");
    if (d->model_mode != FK_MODEL_SHARED) return fail(FK_ERR_UNSUPPORTED, "square-root filter: FK_MODEL_SHARED only");
    if (d->alpha_sq != 1.0 || d->flags != 0) return fail(FK_ERR_UNSUPPORTED, "square-root filter: alpha_sq 1 and flags 0 only");
    return FK_OK;
}

static int launch(const fk_kf_desc *d, SrkfArgs &a, void *stream)
{
    // one step's record block is addressed with 32-bit byte offsets (fk_device.hpp)
    const long mx = d->n > d->m ? d->n : d->m;
    long E = mx * mx;
    if (d->nu > E) E = d->nu;
    if ((double)d->N * (double)E * 8.0 >= 4294967264.0) return fail(FK_ERR_UNSUPPORTED, "N * dim^2 * 8 bytes must stay below 4 GiB (split the bank)");
    a.N = d->N;
    a.n = d->n; a.m = d->m; a.nu = d->nu;
    const SrkfEntry *e = pick_srkf(d->n, d->m);
    return e ? e->fn(a, d->layout, (hipStream_t)stream) : launch_srkf_general(a, d->layout, (hipStream_t)stream);
}

}  // namespace fk

using namespace fk;

extern "C" int fk_srkf_batch_f64(const fk_kf_desc *desc, const double *F, const double *Q1_2, const double *H,
                                 const double *R1_2, const double *B, const double *u, const double *z, const uint8_t *mask,
                                 double *x, double *P1_2, double *means, double *sqrt_covs, double *means_p,
                                 double *sqrt_covs_p, double *y, double *K, double *S1_2, double *SI1_2,
                                 int32_t *status, void *stream)
{
    const int rc = check_desc(desc, true);
    if (rc != FK_OK) return rc;
    const fk_kf_desc *d = desc;
    if (d->N == 0 || d->T == 0) return FK_OK;                 // nothing to read, nothing to touch
    if (!F || !Q1_2 || !H || !R1_2 || !z || !x || !P1_2) return fail(FK_ERR_BAD_ARG, "F,Q1_2,H,R1_2,z,x,P1_2 must not be NULL");
    if (d->nu > 0 && (!B || !u)) return fail(FK_ERR_BAD_ARG, "dim_u > 0 needs B and u");
    SrkfArgs a{};
    a.F = F; a.Q12 = Q1_2; a.H = H; a.R12 = R1_2; a.B = d->nu > 0 ? B : nullptr; a.u = d->nu > 0 ? u : nullptr; a.z = z;
    a.mask = mask; a.x = x; a.P12 = P1_2;
    a.means = means; a.covs = sqrt_covs; a.means_p = means_p; a.covs_p = sqrt_covs_p;
    a.y = y; a.K = K; a.S12 = S1_2; a.SI12 = SI1_2; a.status = status;
    a.T = d->T; a.update_first = d->update_first != 0; a.phase = SRKF_STEPS;
    return launch(d, a, stream);
}

extern "C" int fk_srkf_predict_f64(const fk_kf_desc *desc, const double *F, const double *Q1_2, const double *B,
                                   const double *u, double *x, double *P1_2, int32_t *status, void *stream)
{
    const int rc = check_desc(desc, false);
    if (rc != FK_OK) return rc;
    const fk_kf_desc *d = desc;
    if (d->N == 0) return FK_OK;
    if (!F || !Q1_2 || !x || !P1_2) return fail(FK_ERR_BAD_ARG, "F,Q1_2,x,P1_2 must not be NULL");
    if (d->nu > 0 && (!B || !u)) return fail(FK_ERR_BAD_ARG, "dim_u > 0 needs B and u");
    SrkfArgs a{};
    a.F = F; a.Q12 = Q1_2; a.B = d->nu > 0 ? B : nullptr; a.u = d->nu > 0 ? u : nullptr;
    a.x = x; a.P12 = P1_2; a.status = status;
    a.T = 1; a.phase = SRKF_PREDICT;
    return launch(d, a, stream);
}

extern "C" int fk_srkf_update_f64(const fk_kf_desc *desc, const double *H, const double *R1_2, const double *z,
                                  const uint8_t *mask, double *x, double *P1_2, double *y, double *K, double *S1_2,
                                  double *SI1_2, int32_t *status, void *stream)
{
    const int rc = check_desc(desc, false);
    if (rc != FK_OK) return rc;
    const fk_kf_desc *d = desc;
    if (d->N == 0) return FK_OK;
    if (!H || !R1_2 || !z || !x || !P1_2) return fail(FK_ERR_BAD_ARG, "H,R1_2,z,x,P1_2 must not be NULL");
    SrkfArgs a{};
    a.H = H; a.R12 = R1_2; a.z = z; a.mask = mask; a.x = x; a.P12 = P1_2;
    a.y = y; a.K = K; a.S12 = S1_2; a.SI12 = SI1_2; a.status = status;
    a.T = 1; a.phase = SRKF_UPDATE;
    return launch(d, a, stream);
}
