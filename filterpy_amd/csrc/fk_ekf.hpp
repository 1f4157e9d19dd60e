// fk_ekf.hpp -- the extended Kalman filter (filterpy/kalman/EKF.py:32-428), per track.
//
// Reference:
//   predict_x (:351)      x = F x + B u
//   predict (:367)        P = F P F' + Q
//   update (:319-332)     PHT = P H';  S = H PHT + R;  SI = inv(S);  K = PHT SI;  y = residual(z, Hx(x));  x += K y;
//                         I_KH = I - K H;  P = I_KH P I_KH' + K R K'
//   log_likelihood (:380) logpdf(y; 0, S);   mahalanobis (:409) sqrt(y' SI y)
//
// What is nonlinear in an EKF -- H = HJacobian(x) and y = residual(z, Hx(x)) -- is formed OUTSIDE and arrives as the track's
// own H (m x n) and y (m): nothing here forms z - H x.  The rest is the linear filter's arithmetic in the linear filter's
// operation order (fk_math.hpp: kf_predict with alpha_sq 1, kf_update's Joseph form), inv(S) through the in-lane L D L' and
// two triangular solves.
//
// Status: a pivot of the L D L' of S that is not > 0 sets ST_NOT_PD (dim_z 1: S itself; the reference's inv raises for an
// exactly singular S only), a non-finite x or P after the operation ST_NONFINITE.
// rj_diag (FK_KF_FLAG_R_JOSEPH_DIAG, as for fk_kf_update_f64): the reference with a scalar R attribute and dim_z > 1 -- :320 adds
// r to every element of S, :332 forms r K K': R arrives as r * ones and the Joseph term keeps only its diagonal.
//
// Padded instantiations (n < NX, m < NZ): identity in F, P and R, zeros in Q, H, y and B u -- every padded pivot is exactly 1,
// every coupling term an exact zero.
//
// Host-compilable like fk_ckf.hpp (tests/test_host_ekf.py builds it with g++ and runs it against tests/ekf_port.py).
#pragma once

#include <stdint.h>

#include "fk_math.hpp"

namespace fk {

template <int NX>
FK_HD int ekf_nonfinite(const double (&x)[NX], const double (&P)[NX * NX])
{
    bool ok = true;
    FK_UNROLL for (int i = 0; i < NX; ++i) ok = ok && (fabs(x[i]) <= 1.79769313486231570815e+308);
    FK_UNROLL for (int i = 0; i < NX * NX; ++i) ok = ok && (fabs(P[i]) <= 1.79769313486231570815e+308);
    return ok ? 0 : ST_NONFINITE;
}

// predict (:351, :367).  bu = B u of the step (zeros without a control input).  Model: rowF, rowQ.  Returns ST_NONFINITE or 0.
template <int NX, class Model>
FK_HD int ekf_predict(double (&x)[NX], double (&P)[NX * NX], const double (&bu)[NX], const Model &M)
{
    kf_predict<NX>(x, P, M, 1.0);
    FK_UNROLL for (int i = 0; i < NX; ++i) x[i] += bu[i];
    return ekf_nonfinite<NX>(x, P);
}

// update (:319-332) with the track's Jacobian H (m x n, row-major) and the innovation y given.  Model: rowR.
// Out: K (n x m), S, and the L D L' of S (Lf, dinv: for inv_from_ldlt and ekf_likelihood).  Returns status bits.
template <int NX, int NZ, class Model>
FK_HD int ekf_update(double (&x)[NX], double (&P)[NX * NX], const double (&H)[NZ * NX], const double (&y)[NZ], const Model &M,
                     double (&K)[NX * NZ], double (&S)[NZ * NZ], double (&Lf)[NZ * NZ], double (&dinv)[NZ], bool rj_diag = false)
{
    int st = 0;
    double PHT[NX * NZ];
    FK_UNROLL for (int r = 0; r < NZ; ++r) {
        FK_UNROLL for (int i = 0; i < NX; ++i) {
            double acc = P[i * NX] * H[r * NX];
            FK_UNROLL for (int k = 1; k < NX; ++k) acc = fma(P[i * NX + k], H[r * NX + k], acc);
            PHT[i * NZ + r] = acc;
        }
        FK_STAGE();
    }
    FK_UNROLL for (int r = 0; r < NZ; ++r) {
        double rr[NZ];
        M.rowR(r, rr);
        FK_UNROLL for (int c = 0; c < NZ; ++c) {
            double acc = H[r * NX] * PHT[c];
            FK_UNROLL for (int k = 1; k < NX; ++k) acc = fma(H[r * NX + k], PHT[k * NZ + c], acc);
            S[r * NZ + c] = acc + rr[c];
        }
        FK_STAGE();
    }
    FK_UNROLL for (int i = 0; i < NX * NZ; ++i) K[i] = PHT[i];
    if constexpr (NZ == 1) {
        const double si = 1.0 / S[0];
        if (!(S[0] > 0.0)) st |= ST_NOT_PD;
        dinv[0] = si;
        Lf[0] = S[0];
        FK_UNROLL for (int i = 0; i < NX; ++i) K[i] = PHT[i] * si;
    } else {
        double d[NZ];
        FK_UNROLL for (int i = 0; i < NZ * NZ; ++i) Lf[i] = S[i];
        if (!ldlt2<NZ>(Lf, d, dinv)) st |= ST_NOT_PD;
        solve_rows_ldlt<NX, NZ>(Lf, dinv, K);
    }
    FK_STAGE();

    FK_UNROLL for (int i = 0; i < NX; ++i) {
        double acc = x[i];
        FK_UNROLL for (int k = 0; k < NZ; ++k) acc = fma(K[i * NZ + k], y[k], acc);
        x[i] = acc;
    }

    double IKH[NX * NX];
    FK_UNROLL for (int i = 0; i < NX; ++i)
        FK_UNROLL for (int j = 0; j < NX; ++j) IKH[i * NX + j] = (i == j) ? 1.0 : 0.0;
    FK_UNROLL for (int r = 0; r < NZ; ++r) {
        FK_UNROLL for (int i = 0; i < NX; ++i)
            FK_UNROLL for (int j = 0; j < NX; ++j) IKH[i * NX + j] = fma(-K[i * NZ + r], H[r * NX + j], IKH[i * NX + j]);
        FK_STAGE();
    }
    // T1 = I_KH P   (P is dead afterwards and is overwritten by the result below)
    double T1[NX * NX];
    matmul<NX, NX, NX>(IKH, P, T1);
    FK_STAGE();
    double KR[NX * NZ];
    FK_UNROLL for (int i = 0; i < NX * NZ; ++i) KR[i] = 0.0;
    FK_UNROLL for (int r = 0; r < NZ; ++r) {
        double rr[NZ];
        M.rowR(r, rr);
        FK_UNROLL for (int c = 0; c < NZ; ++c) rr[c] = (rj_diag && c != r) ? 0.0 : rr[c];
        FK_UNROLL for (int i = 0; i < NX; ++i)
            FK_UNROLL for (int c = 0; c < NZ; ++c)
                KR[i * NZ + c] = (r == 0) ? K[i * NZ] * rr[c] : fma(K[i * NZ + r], rr[c], KR[i * NZ + c]);
    }
    FK_STAGE();
    FK_UNROLL for (int i = 0; i < NX; ++i) {
        FK_UNROLL for (int j = 0; j < NX; ++j) {
            double acc = T1[i * NX] * IKH[j * NX];
            FK_UNROLL for (int k = 1; k < NX; ++k) acc = fma(T1[i * NX + k], IKH[j * NX + k], acc);
            FK_UNROLL for (int k = 0; k < NZ; ++k) acc = fma(KR[i * NZ + k], K[j * NZ + k], acc);
            P[i * NX + j] = acc;
        }
        FK_STAGE();
    }
    return st | ekf_nonfinite<NX>(x, P);
}

// The by-products (:380, :409) from the factorisation ekf_update left: ll = log N(y; 0, S), maha = sqrt(y' S^-1 y).
// m: the run-time dim_z (padded instantiations).
template <int NZ>
FK_HD void ekf_likelihood(const double (&y)[NZ], const double (&Lf)[NZ * NZ], const double (&dinv)[NZ], int m, double &ll,
                          double &maha)
{
    double logdet, q = 0.0;
    if constexpr (NZ == 1) {
        logdet = log(Lf[0]);
        q = y[0] * y[0] * dinv[0];
    } else {
        double w[NZ];
        FK_UNROLL for (int i = 0; i < NZ; ++i) {
            double acc = y[i];
            FK_UNROLL for (int k = 0; k < NZ; ++k)
                if (k < i) acc = fma(-Lf[i * NZ + k], w[k], acc);
            w[i] = acc;
            if (i < m) q = fma(acc * acc, dinv[i], q);
        }
        logdet = logdet_from_dinv<NZ>(dinv, m);
    }
    ll = -0.5 * (m * 1.8378770664093453 + logdet + q);
    maha = sqrt(q);
}

// step: the update of step k, then the predict of step k + 1 -- the whole of a launch of ekf_kernels.hip, whose three phases
// are this one function with a half switched off (do_update: also false for a track without a measurement; do_predict).  One
// copy of each half in a code object is what makes a fused step the bits of an update followed by a predict.
// post(x, P, updated) runs between the halves, for everybody: the posterior and the by-products leave there (K, S, Lf, dinv are
// written only where `updated`), and bu -- needed from here on only -- may be filled there.
template <int NX, int NZ, class Model, class Post>
FK_HD int ekf_step(double (&x)[NX], double (&P)[NX * NX], const double (&H)[NZ * NX], const double (&y)[NZ], double (&bu)[NX],
                   const Model &M, double (&K)[NX * NZ], double (&S)[NZ * NZ], double (&Lf)[NZ * NZ], double (&dinv)[NZ],
                   bool rj_diag, bool do_update, bool do_predict, Post post)
{
    int st = 0;
    if (do_update) st |= ekf_update<NX, NZ>(x, P, H, y, M, K, S, Lf, dinv, rj_diag);
    post(x, P, do_update);
    if (do_predict) st |= ekf_predict<NX>(x, P, bu, M);
    return st;
}

// Kernel arguments of fk_ekf_predict_f64 / fk_ekf_update_f64 / fk_ekf_step_f64 (ekf_kernels.hip).
struct EkfArgs {
    const double *F, *Q, *B, *u, *H, *R, *y;
    const uint8_t *mask;
    double *x, *P, *x_post, *P_post, *K, *S, *SI, *ll, *maha;
    int32_t *status;
    long N;
    int n, m, nu;
    int phase;          // EKF_PREDICT / EKF_UPDATE: one of them, once; EKF_STEP: the update, then the predict
    int per_track;      // F, Q, R, B are records of the track ([N][n*n] ...), not shared matrices
    int rj_diag;
};
enum : int { EKF_PREDICT = 0, EKF_UPDATE = 1, EKF_STEP = 2 };

}  // namespace fk
