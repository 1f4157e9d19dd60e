// fk_launchers.hpp -- what ukf_kernels.hip, ut_kernels.hip and kf_variants.hip share with their dispatchers (ukf_dispatch.cpp,
// kf_dispatch.cpp): the launchers, each of which picks the instantiation of a call that passed the checks, declared once for
// the unit that defines them and the dispatcher that calls them.  (ukf_mlg.hip's come from fk_dims_ukf.def.)
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fk_kernel_args.hpp"

namespace fk {

// ukf_kernels.hip, one lane per track: _small -- the forward classes (2,2), (4,2), (6,3), the smoother's 2, 4, 6 --, _big --
// (8,4), (9,3), (9,4) and 8, 9 --, index-order sums and their pair-regrouped twins (_paired)
#define FK_UKF_LAUNCHERS(SUFFIX)                                                                                               \
    int ukf_fwd_launch_small##SUFFIX(const UkfArgs &a, int layout, bool exact, hipStream_t s);                                  \
    int ukf_fwd_launch_big##SUFFIX(const UkfArgs &a, int layout, bool exact, hipStream_t s);                                    \
    int ukf_rts_launch_small##SUFFIX(const UkfRtsArgs &a, const double *F, const double *Q, const double *Wm, const double *Wc, int layout, bool exact, hipStream_t s); \
    int ukf_rts_launch_big##SUFFIX(const UkfRtsArgs &a, const double *F, const double *Q, const double *Wm, const double *Wc, int layout, bool exact, hipStream_t s);
FK_UKF_LAUNCHERS()
FK_UKF_LAUNCHERS(_paired)
#undef FK_UKF_LAUNCHERS

// ukf_simplex.hip, one lane per track on the simplex point set (FK_UKF_FLAG_SIMPLEX): the same classes; tab: the point matrix's
// (a_r, b_r) table, formed by the dispatcher (fk_ukf_simplex.hpp, simplex_table)
struct SimplexTable;
int ukf_simplex_fwd_launch_small(const UkfArgs &a, const SimplexTable &tab, int layout, hipStream_t s);
int ukf_simplex_fwd_launch_big(const UkfArgs &a, const SimplexTable &tab, int layout, hipStream_t s);
int ukf_simplex_rts_launch_small(const UkfRtsArgs &a, const SimplexTable &tab, const double *F, const double *Q, const double *Wm, const double *Wc, int layout, hipStream_t s);
int ukf_simplex_rts_launch_big(const UkfRtsArgs &a, const SimplexTable &tab, const double *F, const double *Q, const double *Wm, const double *Wc, int layout, hipStream_t s);

// ut_kernels.hip: the building blocks
int launch_ut_points(int n, long N, int layout, double scale, const double *x, const double *P, double *sigmas, int32_t *status,
                     hipStream_t stream);
int launch_ut_transform(int n, int k, long N, int layout, const double *sigmas, const double *Wm, const double *Wc,
                        const double *noise_cov, double *x_out, double *P_out, hipStream_t stream);
int launch_ut_cross(int n, int m, int k, long N, int layout, const double *x, const double *z, const double *sigmas_f,
                    const double *sigmas_h, const double *Wc, double *Pxz, hipStream_t stream);
int launch_ut_linear_map(int n_in, int n_out, int k, long N, int layout, const double *M, const double *in, double *out,
                         hipStream_t stream);
int launch_ukf_correct(int n, int m, long N, int layout, const double *Pxz, const double *zp, const double *S, const double *z,
                       double *x, double *P, double *K, int32_t *status, hipStream_t s);

// kf_variants.hip

struct SteadyArgs {
    const double *F, *H, *K, *B, *u, *z;
    const uint8_t *mask;
    double *x, *means, *means_p, *y_out;
    long N, T;
    int n, m, nu, k_per_track;
};

int launch_steady(const SteadyArgs &a, int layout, hipStream_t s);
int launch_corr_update(int n, int m, long N, int layout, const double *H, const double *R, const double *M, int per_track,
                       const double *z, const uint8_t *mask, double *x, double *P, double *y, double *K, double *S, double *SI,
                       int32_t *status, hipStream_t s);
int launch_ukf_rts_correct(int n, long N, int layout, const double *Pxb, const double *xb, const double *Pb, const double *xn,
                           const double *Pn, double *x, double *P, double *K, int32_t *status, hipStream_t s);

}  // namespace fk
