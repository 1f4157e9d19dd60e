// info_dispatch.cpp -- C-ABI entry points of the information filter and their choice of kernel.
//
// fk_info_batch_f64    <- InformationFilterBank.batch_filter  (predict / update of filterpy/kalman/information_filter.py:178-289,
//                         T steps in one launch; the reference's own batch_filter raises NotImplementedError, :291-326)
// fk_info_predict_f64  <- InformationFilter.predict           (information_filter.py:245-289, invertible branch)
// fk_info_update_f64   <- InformationFilter.update            (information_filter.py:178-243)
#include "fk_dispatch.hpp"
#include "fk_info.hpp"

namespace fk {

#define FK_INFO_INST(NX, NZ) int launch_info_fast_##NX##_##NZ(const InfoArgs &, int, hipStream_t);
#include "fk_dims_info.def"
#undef FK_INFO_INST
int launch_info_general(const InfoArgs &, int, hipStream_t);

static const FastEntry<InfoArgs> info_table[] = {
#define FK_INFO_INST(NX, NZ) {NX, NZ, 0, launch_info_fast_##NX##_##NZ},
#include "fk_dims_info.def"
#undef FK_INFO_INST
};

static const Family INFO{"information filter", /*update_first*/ true, /*flags*/ 0, /*k0*/ false};

static int launch(const fk_kf_desc *d, InfoArgs &a, void *stream)
{
    return launch_filter(d, a, stream, info_table, "FK_INFO_GENERAL", launch_info_general);
}

}  // namespace fk

using namespace fk;

extern "C" int fk_info_batch_f64(const fk_kf_desc *desc, const double *F, const double *Q, const double *H,
                                 const double *R_inv, const double *B, const double *u, const double *z, const uint8_t *mask,
                                 double *x, double *P_inv, double *means, double *covs, double *means_p, double *covs_p,
                                 int32_t *status, void *stream)
{
    int rc = check_desc(desc, INFO, true);
    if (rc != FK_OK) return rc;
    const fk_kf_desc *d = desc;
    if (d->N == 0 || d->T == 0) return FK_OK;                 // nothing to read, nothing to touch
    if (!F || !Q || !H || !R_inv || !z || !x || !P_inv) return fail(FK_ERR_BAD_ARG, "F,Q,H,R_inv,z,x,P_inv must not be NULL");
    if ((rc = check_control(d, B, u)) != FK_OK) return rc;
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
    int rc = check_desc(desc, INFO, false);
    if (rc != FK_OK) return rc;
    const fk_kf_desc *d = desc;
    if (d->N == 0) return FK_OK;
    if (!F || !Q || !x || !P_inv) return fail(FK_ERR_BAD_ARG, "F,Q,x,P_inv must not be NULL");
    if ((rc = check_control(d, B, u)) != FK_OK) return rc;
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
    int rc = check_desc(desc, INFO, false);
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
