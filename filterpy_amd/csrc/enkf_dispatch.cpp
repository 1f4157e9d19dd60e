// enkf_dispatch.cpp -- C-ABI entry points of the ensemble Kalman filter and their choice of kernel.
//
// fk_enkf_workspace_bytes                                        (the slabs of partial sums, the pivots and the gain)
// fk_enkf_predict_f64  <- EnsembleKalmanFilter.predict / initialize  (filterpy/kalman/ensemble_kalman_filter.py:275-290; two launches)
// fk_enkf_update_f64   <- EnsembleKalmanFilter.update                (ensemble_kalman_filter.py:218-273; four launches)
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
