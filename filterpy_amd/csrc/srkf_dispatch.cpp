// srkf_dispatch.cpp -- C-ABI entry points of the square-root Kalman filter and their choice of kernel.
//
// fk_srkf_batch_f64    <- SquareRootKalmanFilterBank.batch_filter  (predict / update of filterpy/kalman/square_root.py:172-248,
//                         T steps in one launch)
// fk_srkf_predict_f64  <- SquareRootKalmanFilter.predict           (square_root.py:226-248)
// fk_srkf_update_f64   <- SquareRootKalmanFilter.update            (square_root.py:172-224)
#include "fk_dispatch.hpp"
#include "fk_srkf.hpp"

namespace fk {

#define FK_SRKF_INST(NX, NZ) int launch_srkf_fast_##NX##_##NZ(const SrkfArgs &, int, hipStream_t);
#include "fk_dims_srkf.def"
#undef FK_SRKF_INST
int launch_srkf_general(const SrkfArgs &, int, hipStream_t);

static const FastEntry<SrkfArgs> srkf_table[] = {
#define FK_SRKF_INST(NX, NZ) {NX, NZ, 0, launch_srkf_fast_##NX##_##NZ},
#include "fk_dims_srkf.def"
#undef FK_SRKF_INST
};

static const Family SRKF{"square-root filter", /*update_first*/ true, /*flags*/ 0, /*k0*/ false};

static int launch(const fk_kf_desc *d, SrkfArgs &a, void *stream)
{
    return launch_filter(d, a, stream, srkf_table, "FK_SRKF_GENERAL", launch_srkf_general);
}

}  // namespace fk

using namespace fk;

extern "C" int fk_srkf_batch_f64(const fk_kf_desc *desc, const double *F, const double *Q1_2, const double *H,
                                 const double *R1_2, const double *B, const double *u, const double *z, const uint8_t *mask,
                                 double *x, double *P1_2, double *means, double *sqrt_covs, double *means_p,
                                 double *sqrt_covs_p, double *y, double *K, double *S1_2, double *SI1_2,
                                 int32_t *status, void *stream)
{
    int rc = check_desc(desc, SRKF, true);
    if (rc != FK_OK) return rc;
    const fk_kf_desc *d = desc;
    if (d->N == 0 || d->T == 0) return FK_OK;                 // nothing to read, nothing to touch
    if (!F || !Q1_2 || !H || !R1_2 || !z || !x || !P1_2) return fail(FK_ERR_BAD_ARG, "F,Q1_2,H,R1_2,z,x,P1_2 must not be NULL");
    if ((rc = check_control(d, B, u)) != FK_OK) return rc;
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
    int rc = check_desc(desc, SRKF, false);
    if (rc != FK_OK) return rc;
    const fk_kf_desc *d = desc;
    if (d->N == 0) return FK_OK;
    if (!F || !Q1_2 || !x || !P1_2) return fail(FK_ERR_BAD_ARG, "F,Q1_2,x,P1_2 must not be NULL");
    if ((rc = check_control(d, B, u)) != FK_OK) return rc;
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
    int rc = check_desc(desc, SRKF, false);
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
