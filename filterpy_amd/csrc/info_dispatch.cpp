// info_dispatch.cpp -- C-ABI entry points of the information filter and their choice of kernel.
//
// fk_info_batch_f64    <- InformationFilterBank.batch_filter  (predict / update of filterpy/kalman/information_filter.py:178-289,
//                         T steps in one launch; the reference's own batch_filter raises NotImplementedError, :291-326)
// fk_info_predict_f64  <- InformationFilter.predict           (information_filter.py:245-289, invertible branch)
// fk_info_update_f64   <- InformationFilter.update            (information_filter.py:178-243)
#include <hip/hip_runtime.h>
#include <stdlib.h>

#include "../../include/filterhip.h"
#include "fk_device.hpp"
#include "fk_info.hpp"

namespace fk {

#define FK_INFO_INST(NX, NZ) int launch_info_fast_##NX##_##NZ(const InfoArgs &, int, hipStream_t);
#include "fk_dims_info.def"
#undef FK_INFO_INST
int launch_info_general(const InfoArgs &, int, hipStream_t);

struct InfoEntry {
    int nx, nz;
    int (*fn)(const InfoArgs &, int, hipStream_t);
};
static const InfoEntry info_table[] = {
#define FK_INFO_INST(NX, NZ) {NX, NZ, launch_info_fast_##NX##_##NZ},
#include "fk_dims_info.def"
#undef FK_INFO_INST
};

static int fail(int code, const char *msg)
{
    set_last_error(msg);
    return code;
}

// The fast kernel serves exact (n, m); FK_INFO_GENERAL=1 in the environment forces the general kernel (A/B and tests).  Nothing
// else enters the choice: chained calls run the kernel one call would.
static const InfoEntry *pick_info(int n, int m)
{
    const char *ev = getenv("FK_INFO_GENERAL");
    if (ev && atoi(ev) != 0) return nullptr;
    for (const InfoEntry &e : info_table)
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
    if (d->model_mode != FK_MODEL_SHARED) return fail(FK_ERR_UNSUPPORTED, "information filter: FK_MODEL_SHARED only");
    if (d->alpha_sq != 1.0 || d->flags != 0) return fail(FK_ERR_UNSUPPORTED, "information filter: alpha_sq 1 and flags 0 only");
    return FK_OK;
}

static int launch(const fk_kf_desc *d, InfoArgs &a, void *stream)
{
    // one step's record block is addressed with 32-bit byte offsets (fk_device.hpp)
    const long mx = d->n > d->m ? d->n : d->m;
    long E = mx * mx;
    if (d->nu > E) E = d->nu;
    if ((double)d->N * (double)E * 8.0 >= 4294967264.0) return fail(FK_ERR_UNSUPPORTED, "N * dim^2 * 8 bytes must stay below 4 GiB (split the bank)");
    a.N = d->N;
    a.n = d->n; a.m = d->m; a.nu = d->nu;
    const InfoEntry *e = pick_info(d->n, d->m);
    return e ? e->fn(a, d->layout, (hipStream_t)stream) : launch_info_general(a, d->layout, (hipStream_t)stream);
}

}  // namespace fk

using namespace fk;

extern "C" int fk_info_batch_f64(const fk_kf_desc *desc, const double *F, const double *Q, const double *H,
                                 const double *R_inv, const double *B, const double *u, const double *z, const uint8_t *mask,
                                 double *x, double *P_inv, double *means, double *covs, double *means_p, double *covs_p,
                                 int32_t *status, void *stream)
{
    const int rc = check_desc(desc, true);
    if (rc != FK_OK) return rc;
    const fk_kf_desc *d = desc;
    if (d->N == 0 || d->T == 0) return FK_OK;                 // nothing to read, nothing to touch
    if (!F || !Q || !H || !R_inv || !z || !x || !P_inv) return fail(FK_ERR_BAD_ARG, "F,Q,H,R_inv,z,x,P_inv must not be NULL");
    if (d->nu > 0 && (!B || !u)) return fail(FK_ERR_BAD_ARG, "dim_u > 0 needs B and u");
    InfoArgs a{};
    a.F = F; a.Q = Q; a.H = H; a.Rinv = R_inv; a.B = d->nu > 0 ? B : nullptr; a.u = d->nu > 0 ? u : nullptr; a.z = z;
    a.mask = mask; a.x = x; a.Pinv = P_inv;
    a.means = means; a.covs = covs; a.means_p = means_p; a.covs_p = covs_p; a.status = status;
    a.T = d->T; a.update_first = d->update_first != 0; a.phase = INFO_STEPS;
    return launch(d, a, stream);
}

extern "C" int fk_info_predict_f64(const fk_kf_desc *desc, const double *F, const double *Q, const double *B,
                                   const double *u, double *x, double *P_inv, int32_t *status, void *stream)
{
    const int rc = check_desc(desc, false);
    if (rc != FK_OK) return rc;
    const fk_kf_desc *d = desc;
    if (d->N == 0) return FK_OK;
    if (!F || !Q || !x || !P_inv) return fail(FK_ERR_BAD_ARG, "F,Q,x,P_inv must not be NULL");
    if (d->nu > 0 && (!B || !u)) return fail(FK_ERR_BAD_ARG, "dim_u > 0 needs B and u");
    InfoArgs a{};
    a.F = F; a.Q = Q; a.B = d->nu > 0 ? B : nullptr; a.u = d->nu > 0 ? u : nullptr;
    a.x = x; a.Pinv = P_inv; a.status = status;
    a.T = 1; a.phase = INFO_PREDICT;
    return launch(d, a, stream);
}

extern "C" int fk_info_update_f64(const fk_kf_desc *desc, const double *H, const double *R_inv, const double *z,
                                  const uint8_t *mask, double *x, double *P_inv, double *y, double *K,
                                  int32_t *status, void *stream)
{
    const int rc = check_desc(desc, false);
    if (rc != FK_OK) return rc;
    const fk_kf_desc *d = desc;
    if (d->N == 0) return FK_OK;
    if (!H || !R_inv || !z || !x || !P_inv) return fail(FK_ERR_BAD_ARG, "H,R_inv,z,x,P_inv must not be NULL");
    InfoArgs a{};
    a.H = H; a.Rinv = R_inv; a.z = z; a.mask = mask; a.x = x; a.Pinv = P_inv;
    a.y = y; a.K = K; a.status = status;
    a.T = 1; a.phase = INFO_UPDATE;
    return launch(d, a, stream);
}
