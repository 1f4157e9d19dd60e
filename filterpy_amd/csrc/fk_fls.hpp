// fk_fls.hpp -- one step of the fixed-lag smoother (filterpy/kalman/fixed_lag_smoother.py:133-311), per track.
//
// Reference, step k with lag L (smooth_batch :270-309):
//   x_pre = F x (+ B u);  P = F P F' + Q;  the Joseph-form update of kalman_filter.py (kf_update, fk_math.hpp);
//   xhat[k] = x;  xSmooth[k] = x_pre;
//   k >= L:  PS_0 = P (the posterior), for i < L:  xSmooth[k-i] += PS_i H' SI y,  PS_{i+1} = PS_i (F - K H)'
//   k <  L:  xSmooth[k] = x.
// The lag loop is REASSOCIATED, not copied: PS_i H'SI y = P ((F - K H)')^i w with w = H' (S^-1 y), so the step carries a
// vector u_0 = w, u_{i+1} = (F - K H)' u_i and adds P u_i to row k-i -- 2 n^2 FMAs per lag step instead of the reference's
// 2 n^3 + 2 n^2 m.  The rounding differs from the reference's order by a few ulps of the result (2e-13 normwise measured
// over dims (4,2) .. (16,8) and lags up to 32, against a 1e-10 bar).  S^-1 y comes from kf_update's L D L' factorisation.
//
// Host-compilable like fk_math.hpp (tests/test_host_fls.py builds it with g++ and runs it against the goldens).
#pragma once

#include <stdint.h>

#include "fk_math.hpp"

namespace fk {

// Predict (+ the control input bu, added iff has_u) and update of one step.  On return x, P are the posterior, xpre the prior
// mean, w = H' S^-1 y, G = F - K H (row-major), y and S the innovation and its covariance.  Returns status bits (ST_NOT_PD).
// (A/B, DESIGN.md section 4: forming G' u as F' u - H' (K' u) from the model rows and K -- n m doubles live instead of n^2 --
//  leaves the registers of every instantiation within a few of these: the Joseph update's temporaries set the peak, not G.
//  It costs 2 n m more FMAs per lag step and is not used.)
template <int NX, int NZ, class Model>
FK_HD int fls_filter_step(double (&x)[NX], double (&P)[NX * NX], const double (&z)[NZ], const Model &M,
                          const double (&bu)[NX], bool has_u, bool rj_diag,
                          double (&xpre)[NX], double (&w)[NX], double (&G)[NX * NX], double (&y)[NZ], double (&S)[NZ * NZ])
{
    kf_predict<NX>(x, P, M, 1.0);
    if (has_u) {
        FK_UNROLL for (int i = 0; i < NX; ++i) x[i] += bu[i];
    }
    FK_UNROLL for (int i = 0; i < NX; ++i) xpre[i] = x[i];
    double K[NX * NZ], Lf[NZ * NZ], dinv[NZ];
    const int st = kf_update<NX, NZ>(x, P, z, M, K, y, S, Lf, dinv, rj_diag);
    FK_STAGE();
    // v = S^-1 y (one row through the factorisation), w = H' v
    double v[NZ];
    FK_UNROLL for (int r = 0; r < NZ; ++r) v[r] = y[r];
    solve_rows_ldlt<1, NZ>(Lf, dinv, v);
    FK_UNROLL for (int j = 0; j < NX; ++j) w[j] = 0.0;
    // G = F - K H
    FK_UNROLL for (int i = 0; i < NX; ++i) {
        double f[NX];
        M.rowF(i, f);
        FK_UNROLL for (int j = 0; j < NX; ++j) G[i * NX + j] = f[j];
    }
    FK_UNROLL for (int r = 0; r < NZ; ++r) {
        double h[NX];
        M.rowH(r, h);
        FK_UNROLL for (int j = 0; j < NX; ++j) w[j] = fma(h[j], v[r], w[j]);
        FK_UNROLL for (int i = 0; i < NX; ++i)
            FK_UNROLL for (int j = 0; j < NX; ++j) G[i * NX + j] = fma(-K[i * NZ + r], h[j], G[i * NX + j]);
    }
    FK_STAGE();
    return st;
}

// One lag step: row += P u;  then (if `advance`) u = G' u.
template <int NX>
FK_HD void fls_lag_step(const double (&P)[NX * NX], const double (&G)[NX * NX], double (&u)[NX], double *row, bool advance)
{
    FK_UNROLL for (int i = 0; i < NX; ++i) {
        double acc = row[i];
        FK_UNROLL for (int l = 0; l < NX; ++l) acc = fma(P[i * NX + l], u[l], acc);
        row[i] = acc;
    }
    if (advance) {
        double un[NX];
        FK_UNROLL for (int j = 0; j < NX; ++j) {
            double acc = G[j] * u[0];
            FK_UNROLL for (int l = 1; l < NX; ++l) acc = fma(G[l * NX + j], u[l], acc);
            un[j] = acc;
        }
        FK_UNROLL for (int j = 0; j < NX; ++j) u[j] = un[j];
    }
}

// The whole step on a SHIFT REGISTER of pending rows: pend[i * NX ..] is row k-i after the call (row k = the new one).  The
// caller passes the global step k and the lag (uniform, max(lag, 1) <= LMAX); rows older than LMAX-1 fall off the end.  After
// the call row k - max(lag, 1) + 1 = pend[max(lag, 1) - 1] is final: the caller writes it out before the next step.
// Every index into pend is a compile-time constant: the register file holds it (no scratch).
template <int NX, int NZ, int LMAX, class Model>
FK_HD int fls_step(double (&x)[NX], double (&P)[NX * NX], const double (&z)[NZ], const Model &M,
                   const double (&bu)[NX], bool has_u, bool rj_diag, long k, int lag,
                   double (&pend)[LMAX * NX], double (&y)[NZ], double (&S)[NZ * NZ])
{
    double xpre[NX], w[NX], G[NX * NX];
    const int st = fls_filter_step<NX, NZ>(x, P, z, M, bu, has_u, rj_diag, xpre, w, G, y, S);
    FK_UNROLL for (int i = LMAX - 1; i > 0; --i)
        FK_UNROLL for (int j = 0; j < NX; ++j) pend[i * NX + j] = pend[(i - 1) * NX + j];
    const bool smooth = k >= (long)lag;
    FK_UNROLL for (int j = 0; j < NX; ++j) pend[j] = smooth ? xpre[j] : x[j];
    if (smooth) {
        FK_UNROLL for (int i = 0; i < LMAX; ++i) {
            if (i < lag) {
                double r[NX];
                FK_UNROLL for (int j = 0; j < NX; ++j) r[j] = pend[i * NX + j];
                fls_lag_step<NX>(P, G, w, r, i + 1 < lag);
                FK_UNROLL for (int j = 0; j < NX; ++j) pend[i * NX + j] = r[j];
            }
        }
    }
    return st;
}

// Kernel arguments of fk_fls_batch_f64 (fls_kernels.hip).
struct FlsArgs {
    const double *F, *Q, *H, *R, *B, *u, *z;
    double *x, *P, *xs, *xhat, *y, *S;
    int32_t *status;
    long N, T, k0, W;   // W: pending rows at the head of xs on entry
    int n, m, nu, lag;
    int rj_diag;
};

}  // namespace fk
