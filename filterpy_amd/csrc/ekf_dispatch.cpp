// ekf_dispatch.cpp -- C-ABI entry points of the extended Kalman filter and their choice of kernel.
//
// fk_ekf_predict_f64  <- ExtendedKalmanFilter.predict_x / predict                  (filterpy/kalman/EKF.py:351, 367)
// fk_ekf_update_f64   <- ExtendedKalmanFilter.update, H and y given                (EKF.py:319-332; by-products :380, :409)
// fk_ekf_step_f64     <- that update, then the predict of the next step, in ONE launch (the reference has no such call;
//                        predict_update, :222-242, is the other order)
#include "fk_dispatch.hpp"
#include "fk_ekf.hpp"

namespace fk {

#define FK_EKF_SHAPE(NX, NZ) int launch_ekf_fast_##NX##_##NZ(const EkfArgs &, int, hipStream_t);
#include "fk_dims_ekf.def"
#undef FK_EKF_SHAPE
int launch_ekf_general(const EkfArgs &, int, hipStream_t);

static const FastEntry<EkfArgs> ekf_table[] = {
#define FK_EKF_SHAPE(NX, NZ) {NX, NZ, 0, launch_ekf_fast_##NX##_##NZ},
#include "fk_dims_ekf.def"
#undef FK_EKF_SHAPE
};

static const Family EKF{"extended Kalman filter", /*update_first*/ false, /*flags*/ FK_KF_FLAG_R_JOSEPH_DIAG, /*k0*/ false};

// desc, for all three entry points (T is ignored): the scaffold's refusals with the model mode taken out, then the family's
// own rule for it -- F, Q, R, B shared or records of the track; a model per step has no meaning in a one-step call.
static int check_ekf_desc(const fk_kf_desc *d)
{
    if (!d) return fail(FK_ERR_BAD_ARG, "desc is NULL");
    fk_kf_desc c = *d;
    c.model_mode = FK_MODEL_SHARED;
    const int rc = check_desc(&c, EKF, false);
    if (rc != FK_OK) return rc;
    if (d->model_mode != FK_MODEL_SHARED && d->model_mode != FK_MODEL_PER_TRACK)
        return fail(FK_ERR_UNSUPPORTED, "extended Kalman filter: FK_MODEL_SHARED or FK_MODEL_PER_TRACK only");
    // the widest record beyond launch_filter's max(n, m)^2: the track's own B [n*nu]
    return check_record_block(d, d->model_mode == FK_MODEL_PER_TRACK ? (long)d->n * d->nu : 0L);
}

static int launch(const fk_kf_desc *d, EkfArgs &a, void *stream)
{
    a.per_track = d->model_mode == FK_MODEL_PER_TRACK;
    a.rj_diag = (d->flags & FK_KF_FLAG_R_JOSEPH_DIAG) != 0;
    return launch_filter(d, a, stream, ekf_table, "FK_EKF_GENERAL", launch_ekf_general);
}

}  // namespace fk

using namespace fk;

extern "C" int fk_ekf_predict_f64(const fk_kf_desc *desc, const double *F, const double *Q, const double *B, const double *u,
                                  double *x, double *P, int32_t *status, void *stream)
{
    int rc = check_ekf_desc(desc);
    if (rc != FK_OK) return rc;
    const fk_kf_desc *d = desc;
    if (d->N == 0) return FK_OK;
    if (!F || !Q || !x || !P) return fail(FK_ERR_BAD_ARG, "F,Q,x,P must not be NULL");
    rc = check_control(d, B, u);
    if (rc != FK_OK) return rc;
    EkfArgs a{};
    a.F = F; a.Q = Q; a.B = B; a.u = u; a.x = x; a.P = P; a.status = status;
    a.phase = EKF_PREDICT;
    return launch(d, a, stream);
}

extern "C" int fk_ekf_update_f64(const fk_kf_desc *desc, const double *H, const double *R, const double *y, const uint8_t *mask,
                                 double *x, double *P, double *K, double *S, double *SI, double *log_likelihood,
                                 double *mahalanobis, int32_t *status, void *stream)
{
    const int rc = check_ekf_desc(desc);
    if (rc != FK_OK) return rc;
    const fk_kf_desc *d = desc;
    if (d->N == 0) return FK_OK;
    if (!H || !R || !y || !x || !P) return fail(FK_ERR_BAD_ARG, "H,R,y,x,P must not be NULL");
    EkfArgs a{};
    a.H = H; a.R = R; a.y = y; a.mask = mask; a.x = x; a.P = P; a.K = K; a.S = S; a.SI = SI;
    a.ll = log_likelihood; a.maha = mahalanobis; a.status = status;
    a.phase = EKF_UPDATE;
    // (nu plays no part in an update: the control record is not read)
    fk_kf_desc c = *d;
    c.nu = 0;
    return launch(&c, a, stream);
}

extern "C" int fk_ekf_step_f64(const fk_kf_desc *desc, const double *H, const double *R, const double *y, const uint8_t *mask,
                               const double *F, const double *Q, const double *B, const double *u, double *x, double *P,
                               double *x_post, double *P_post, double *K, double *S, double *SI, double *log_likelihood,
                               double *mahalanobis, int32_t *status, void *stream)
{
    int rc = check_ekf_desc(desc);
    if (rc != FK_OK) return rc;
    const fk_kf_desc *d = desc;
    if (d->N == 0) return FK_OK;
    if (!H || !R || !y || !F || !Q || !x || !P) return fail(FK_ERR_BAD_ARG, "H,R,y,F,Q,x,P must not be NULL");
    rc = check_control(d, B, u);
    if (rc != FK_OK) return rc;
    EkfArgs a{};
    a.H = H; a.R = R; a.y = y; a.mask = mask; a.F = F; a.Q = Q; a.B = B; a.u = u; a.x = x; a.P = P;
    a.x_post = x_post; a.P_post = P_post; a.K = K; a.S = S; a.SI = SI; a.ll = log_likelihood; a.maha = mahalanobis;
    a.status = status;
    a.phase = EKF_STEP;
    return launch(d, a, stream);
}
