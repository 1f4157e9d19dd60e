// enkf_dispatch.cpp -- C-ABI entry points of the ensemble Kalman filter and their choice of kernel.
//
// fk_enkf_workspace_bytes                                        (the slabs of partial sums, the pivots and the gain)
// fk_enkf_predict_f64  <- EnsembleKalmanFilter.predict / initialize  (filterpy/kalman/ensemble_kalman_filter.py:275-290; two launches)
// fk_enkf_update_f64   <- EnsembleKalmanFilter.update                (ensemble_kalman_filter.py:218-273; four launches)
// fk_enkf_bank_predict_f64 / fk_enkf_bank_update_f64 <- EnsembleKalmanFilterBank: B ensembles of N <= 2048 members, ONE launch each
#include "fk_dispatch.hpp"
#include "fk_enkf.hpp"

namespace fk {

#define FK_ENKF_INST(NX, NZ) int launch_enkf_fast_##NX##_##NZ(const EnkfArgs &, int, hipStream_t);
#include "fk_dims_enkf.def"
#undef FK_ENKF_INST
int launch_enkf_general(const EnkfArgs &, int, hipStream_t);
int launch_enkf_finalize(const EnkfArgs &, hipStream_t);

static const FastEntry<EnkfArgs> enkf_table[] = {
#define FK_ENKF_INST(NX, NZ) {NX, NZ, 0, launch_enkf_fast_##NX##_##NZ},
#include "fk_dims_enkf.def"
#undef FK_ENKF_INST
};

#define FK_ENKF_INST(NX, NZ) int launch_enkf_bank_fast_##NX##_##NZ(const EnkfBankArgs &, int, hipStream_t);
#include "fk_dims_enkf.def"
#undef FK_ENKF_INST
int launch_enkf_bank_general(const EnkfBankArgs &, int, hipStream_t);

static const FastEntry<EnkfBankArgs> enkf_bank_table[] = {
#define FK_ENKF_INST(NX, NZ) {NX, NZ, 0, launch_enkf_bank_fast_##NX##_##NZ},
#include "fk_dims_enkf.def"
#undef FK_ENKF_INST
};

static const Family ENKF{"ensemble Kalman filter", /*update_first*/ true, /*flags*/ 0, /*k0*/ false};

// desc, the ensemble size and the workspace: what both entry points check before they look at their own pointers
static int check_call(const fk_kf_desc *d, const void *workspace, size_t workspace_bytes, bool pointers)
{
    const int rc = check_desc(d, ENKF, false);
    if (rc != FK_OK) return rc;
    if (d->N < 2) return fail(FK_ERR_BAD_ARG, "ensemble Kalman filter: N (the ensemble size) must be >= 2");
    if (!pointers || !workspace) return fail(FK_ERR_BAD_ARG, "sigmas, noise, x, P, workspace (and R, z for the update) must not be NULL");
    if (workspace_bytes < fk_enkf_workspace_bytes(d->n, d->m, d->N))
        return fail(FK_ERR_WORKSPACE, "workspace smaller than fk_enkf_workspace_bytes(n, m, N)");
    return FK_OK;
}

// one pass over the ensemble (the fast kernel serves exact (n, m), the general kernel the rest), then its finalize
static int pass(const fk_kf_desc *d, EnkfArgs &a, int phase, int fin, hipStream_t stream)
{
    const FastEntry<EnkfArgs> *e = pick_fast(enkf_table, "FK_ENKF_GENERAL", d->n, d->m);
    a.phase = phase;
    a.ax = e ? d->n : ENKF_MAXX;
    a.az = e ? d->m : ENKF_MAXZ;
    int rc = e ? e->fn(a, d->layout, stream) : launch_enkf_general(a, d->layout, stream);
    if (rc != FK_OK) return rc;
    a.phase = fin;
    return launch_enkf_finalize(a, stream);
}

// desc, the ensemble size and the number of ensembles of a bank call.  The models are shared or one per ensemble.
static int check_bank_call(const fk_kf_desc *d, int64_t n_ensembles, bool pointers)
{
    if (!d) return fail(FK_ERR_BAD_ARG, "desc is NULL");
    fk_kf_desc shared = *d;
    if (d->model_mode == FK_MODEL_PER_TRACK) shared.model_mode = FK_MODEL_SHARED;
    const int rc = check_desc(&shared, ENKF, false);
    if (rc != FK_OK) return rc;
    if (d->N < 2) return fail(FK_ERR_BAD_ARG, "ensemble Kalman filter: N (the ensemble size) must be >= 2");
    if (d->N > ENKF_CHUNK)
        return fail(FK_ERR_UNSUPPORTED, "ensemble Kalman filter bank: N (the ensemble size) must be <= 2048 (larger ensembles: fk_enkf_predict_f64 / fk_enkf_update_f64, one at a time)");
    if (n_ensembles < 1 || n_ensembles > 2147483647)
        return fail(FK_ERR_BAD_ARG, "ensemble Kalman filter bank: the number of ensembles must be >= 1 (and below 2^31)");
    if (!pointers) return fail(FK_ERR_BAD_ARG, "sigmas, noise, x, P (and R, z for the update) must not be NULL");
    return FK_OK;
}

// the one launch: the fast kernel serves exact (n, m), the general kernel the rest; the route by N is the launcher's
static int bank_launch(const fk_kf_desc *d, EnkfBankArgs &a, int64_t n_ensembles, hipStream_t stream)
{
    a.B = n_ensembles; a.N = d->N; a.n = d->n; a.m = d->m;
    a.per_track = d->model_mode == FK_MODEL_PER_TRACK;
    const FastEntry<EnkfBankArgs> *e = pick_fast(enkf_bank_table, "FK_ENKF_GENERAL", d->n, d->m);
    return e ? e->fn(a, d->layout, stream) : launch_enkf_bank_general(a, d->layout, stream);
}

}  // namespace fk

using namespace fk;

extern "C" size_t fk_enkf_workspace_bytes(int32_t n, int32_t m, int64_t N)
{
    if (n < 1 || n > ENKF_MAXX || m < 1 || m > ENKF_MAXZ || N < 0) return 0;
    return (size_t)enkf_workspace_doubles(N) * sizeof(double);
}

extern "C" int fk_enkf_predict_f64(const fk_kf_desc *desc, const double *F, const double *noise, const double *factor,
                                   double *sigmas, double *x, double *P, void *workspace, size_t workspace_bytes,
                                   int32_t *status, void *stream)
{
    const int rc = check_call(desc, workspace, workspace_bytes, noise && sigmas && x && P);
    if (rc != FK_OK) return rc;
    EnkfArgs a{};
    a.F = F; a.noise = noise; a.factor = factor; a.sigmas = sigmas; a.x = x; a.P = P;
    a.ws = (double *)workspace; a.status = status;
    a.N = desc->N; a.n = desc->n; a.m = desc->m;
    return pass(desc, a, ENKF_PREDICT, ENKF_FIN_PREDICT, (hipStream_t)stream);
}

extern "C" int fk_enkf_update_f64(const fk_kf_desc *desc, const double *H, const double *sigmas_h, const double *R,
                                  const double *z, const double *noise, const double *factor, double *sigmas, double *x,
                                  double *P, double *S, double *SI, double *K, void *workspace, size_t workspace_bytes,
                                  int32_t *status, void *stream)
{
    int rc = check_call(desc, workspace, workspace_bytes, R && z && noise && sigmas && x && P);
    if (rc != FK_OK) return rc;
    if (!H == !sigmas_h) return fail(FK_ERR_BAD_ARG, "exactly one of H and sigmas_h must be given");
    EnkfArgs a{};
    a.H = H; a.sigmas_h = sigmas_h; a.R = R; a.z = z; a.noise = noise; a.factor = factor;
    a.sigmas = sigmas; a.x = x; a.P = P; a.S = S; a.SI = SI; a.K = K;
    a.ws = (double *)workspace; a.status = status;
    a.N = desc->N; a.n = desc->n; a.m = desc->m;
    if ((rc = pass(desc, a, ENKF_STATS, ENKF_FIN_UPDATE, (hipStream_t)stream)) != FK_OK) return rc;
    return pass(desc, a, ENKF_APPLY, ENKF_FIN_APPLY, (hipStream_t)stream);
}

extern "C" int fk_enkf_bank_predict_f64(const fk_kf_desc *desc, int64_t n_ensembles, const double *F, const double *noise,
                                        const double *factor, double *sigmas, double *x, double *P, int32_t *status, void *stream)
{
    const int rc = check_bank_call(desc, n_ensembles, noise && sigmas && x && P);
    if (rc != FK_OK) return rc;
    EnkfBankArgs a{};
    a.F = F; a.noise = noise; a.factor = factor; a.sigmas = sigmas; a.x = x; a.P = P; a.status = status;
    a.update = 0;
    return bank_launch(desc, a, n_ensembles, (hipStream_t)stream);
}

extern "C" int fk_enkf_bank_update_f64(const fk_kf_desc *desc, int64_t n_ensembles, const double *H, const double *sigmas_h,
                                       const double *R, const double *z, const uint8_t *mask, const double *noise,
                                       const double *factor, double *sigmas, double *x, double *P, double *S, double *SI,
                                       double *K, int32_t *status, void *stream)
{
    const int rc = check_bank_call(desc, n_ensembles, R && z && noise && sigmas && x && P);
    if (rc != FK_OK) return rc;
    if (!H == !sigmas_h) return fail(FK_ERR_BAD_ARG, "exactly one of H and sigmas_h must be given");
    EnkfBankArgs a{};
    a.H = H; a.sigmas_h = sigmas_h; a.R = R; a.z = z; a.mask = mask; a.noise = noise; a.factor = factor;
    a.sigmas = sigmas; a.x = x; a.P = P; a.S = S; a.SI = SI; a.K = K; a.status = status;
    a.update = 1;
    return bank_launch(desc, a, n_ensembles, (hipStream_t)stream);
}
