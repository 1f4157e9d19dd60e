// ckf_dispatch.cpp -- C-ABI entry points of the cubature Kalman filter and their choice of kernel.
//
// fk_ckf_sigma_points_f64    <- spherical_radial_sigmas            (filterpy/kalman/CubatureKalmanFilter.py:32-61)
// fk_ckf_transform_f64       <- ckf_transform                      (CubatureKalmanFilter.py:64-98)
// fk_ckf_update_f64          <- CubatureKalmanFilter.update        (CubatureKalmanFilter.py:357-379), arbitrary hx
// fk_ckf_linear_batch_f64    <- CubatureKalmanFilter.batch_filter with fx = F, hx = H (predict :292-327 and update :329-390,
//                               T steps in one launch; the reference has no batch_filter)
// fk_ckf_linear_predict_f64  <- CubatureKalmanFilter.predict with fx = F
// fk_ckf_linear_update_f64   <- CubatureKalmanFilter.update with hx = H
#include "fk_dispatch.hpp"
#include "fk_ckf.hpp"

namespace fk {

#define FK_CKF_SHAPE(NX, NZ) int launch_ckf_fast_##NX##_##NZ(const CkfArgs &, int, hipStream_t);
#include "fk_dims_ckf.def"
#undef FK_CKF_SHAPE
int launch_ckf_general(const CkfArgs &, int, hipStream_t);
int launch_ckf_points(int, long, int, const double *, const double *, double *, int32_t *, hipStream_t);
int launch_ckf_transform(int, int, long, int, const double *, const double *, double *, double *, hipStream_t);
int launch_ckf_update(int, int, long, int, const double *, const double *, const double *, const double *, double *, double *,
                      double *, double *, double *, double *, double *, double *, int32_t *, hipStream_t);

static const FastEntry<CkfArgs> ckf_table[] = {
#define FK_CKF_SHAPE(NX, NZ) {NX, NZ, 0, launch_ckf_fast_##NX##_##NZ},
#include "fk_dims_ckf.def"
#undef FK_CKF_SHAPE
};

static const Family CKF{"cubature Kalman filter", /*update_first*/ false, /*flags*/ 0, /*k0*/ false};

static int check_ckf_desc(const fk_kf_desc *d, bool steps)
{
    if (d && (d->flags != 0 || d->nu != 0 || d->update_first != 0))
        return fail(FK_ERR_UNSUPPORTED, "cubature Kalman filter: flags 0, dim_u 0 and update_first 0 only");
    int rc = check_desc(d, CKF, steps);
    if (rc != FK_OK) return rc;
    // the widest record is the points' [n + n*n]
    return check_record_block(d, (long)d->n * d->n + d->n);
}

static int launch(const fk_kf_desc *d, CkfArgs &a, void *stream)
{
    return launch_filter(d, a, stream, ckf_table, "FK_CKF_GENERAL", launch_ckf_general);
}

// the building blocks: dimensions, layout and the 32-bit record offsets (E: the widest record in doubles)
static int check_block(int n, int m, int64_t N, int layout, long E)
{
    if (n < 1 || m < 1) return fail(FK_ERR_BAD_ARG, "dim_x, dim_z must be >= 1");
    if (N < 0) return fail(FK_ERR_BAD_ARG, "N must be >= 0");
    if (layout != FK_LAYOUT_AOS && layout != FK_LAYOUT_SOA) return fail(FK_ERR_BAD_ARG, "bad layout");
    if (n > 16 || m > 8) return fail(FK_ERR_UNSUPPORTED, "dim_x/dim_z outside the compiled range (dim_x <= 16, dim_z <= 8)");
    return check_record_block((double)N, (double)E, FK_4GIB - 32.0, "N * record * 8 bytes must stay below 4 GiB (split the bank)");
}

}  // namespace fk

using namespace fk;

extern "C" int fk_ckf_sigma_points_f64(int32_t n, int64_t N, int32_t layout, const double *x, const double *P, double *sigmas,
                                       int32_t *status, void *stream)
{
    const int rc = check_block(n, 1, N, layout, 2L * n * n);
    if (rc != FK_OK) return rc;
    if (N == 0) return FK_OK;
    if (!x || !P || !sigmas) return fail(FK_ERR_BAD_ARG, "x,P,sigmas must not be NULL");
    return launch_ckf_points(n, N, layout, x, P, sigmas, status, (hipStream_t)stream);
}

extern "C" int fk_ckf_transform_f64(int32_t d, int32_t k, int64_t N, int32_t layout, const double *sigmas,
                                    const double *noise_cov, double *x_out, double *P_out, void *stream)
{
    if (k < 1 || k > 32) return fail(FK_ERR_UNSUPPORTED, "cubature transform: 1 <= k <= 32 points");
    const int rc = check_block(d, 1, N, layout, (long)k * d > (long)d * d ? (long)k * d : (long)d * d);
    if (rc != FK_OK) return rc;
    if (N == 0) return FK_OK;
    if (!sigmas || !x_out || !P_out) return fail(FK_ERR_BAD_ARG, "sigmas,x_out,P_out must not be NULL");
    return launch_ckf_transform(d, k, N, layout, sigmas, noise_cov, x_out, P_out, (hipStream_t)stream);
}

extern "C" int fk_ckf_update_f64(int32_t n, int32_t m, int64_t N, int32_t layout, const double *sigmas_f,
                                 const double *sigmas_h, const double *R, const double *z, double *x, double *P, double *zp,
                                 double *S, double *SI, double *Pxz, double *K, double *y, int32_t *status, void *stream)
{
    // the widest record: sigmas_f [2n*n], sigmas_h [2n*m], S / SI [m*m] or Pxz / K [n*m]
    long E = 2L * n * n;
    if (2L * n * m > E) E = 2L * n * m;
    if ((long)m * m > E) E = (long)m * m;
    const int rc = check_block(n, m, N, layout, E);
    if (rc != FK_OK) return rc;
    if (N == 0) return FK_OK;
    if (!sigmas_f || !sigmas_h || !R || !z || !x || !P)
        return fail(FK_ERR_BAD_ARG, "sigmas_f,sigmas_h,R,z,x,P must not be NULL");
    return launch_ckf_update(n, m, N, layout, sigmas_f, sigmas_h, R, z, x, P, zp, S, SI, Pxz, K, y, status, (hipStream_t)stream);
}

extern "C" int fk_ckf_linear_batch_f64(const fk_kf_desc *desc, const double *F, const double *Q, const double *H,
                                       const double *R, const double *z, const uint8_t *mask, double *x, double *P,
                                       double *points, double *means, double *covs, double *means_p, double *covs_p,
                                       int32_t *status, void *stream)
{
    int rc = check_ckf_desc(desc, true);
    if (rc != FK_OK) return rc;
    const fk_kf_desc *d = desc;
    if (d->N == 0 || d->T == 0) return FK_OK;                 // nothing to read, nothing to touch
    if (!F || !Q || !H || !R || !z || !x || !P || !points) return fail(FK_ERR_BAD_ARG, "F,Q,H,R,z,x,P,points must not be NULL");
    CkfArgs a{};
    a.F = F; a.Q = Q; a.H = H; a.R = R; a.z = z; a.mask = mask; a.x = x; a.P = P; a.pts = points;
    a.means = means; a.covs = covs; a.means_p = means_p; a.covs_p = covs_p; a.status = status;
    a.T = d->T; a.phase = CKF_STEPS;
    return launch(d, a, stream);
}

extern "C" int fk_ckf_linear_predict_f64(const fk_kf_desc *desc, const double *F, const double *Q, double *x, double *P,
                                         double *points, int32_t *status, void *stream)
{
    int rc = check_ckf_desc(desc, false);
    if (rc != FK_OK) return rc;
    const fk_kf_desc *d = desc;
    if (d->N == 0) return FK_OK;
    if (!F || !Q || !x || !P || !points) return fail(FK_ERR_BAD_ARG, "F,Q,x,P,points must not be NULL");
    CkfArgs a{};
    a.F = F; a.Q = Q; a.x = x; a.P = P; a.pts = points; a.status = status;
    a.T = 1; a.phase = CKF_PREDICT;
    return launch(d, a, stream);
}

extern "C" int fk_ckf_linear_update_f64(const fk_kf_desc *desc, const double *H, const double *R, const double *z,
                                        const uint8_t *mask, double *x, double *P, const double *points, double *y, double *K,
                                        double *S, double *SI, int32_t *status, void *stream)
{
    int rc = check_ckf_desc(desc, false);
    if (rc != FK_OK) return rc;
    const fk_kf_desc *d = desc;
    if (d->N == 0) return FK_OK;
    if (!H || !R || !z || !x || !P || !points) return fail(FK_ERR_BAD_ARG, "H,R,z,x,P,points must not be NULL");
    CkfArgs a{};
    a.H = H; a.R = R; a.z = z; a.mask = mask; a.x = x; a.P = P; a.pts = const_cast<double *>(points);
    a.y = y; a.K = K; a.S = S; a.SI = SI; a.status = status;
    a.T = 1; a.phase = CKF_UPDATE;
    return launch(d, a, stream);
}
