// fk_ckf.hpp -- the cubature Kalman filter (filterpy/kalman/CubatureKalmanFilter.py:32-98, 292-390), per track.
//
// Reference:
//   spherical_radial_sigmas (:32-61)   U = cholesky(P) * sqrt(n) (upper);  points x + U[k], x - U[k]: 2n points, no centre
//   ckf_transform (:64-98)             x = sum(Xs) / k;  P = sum_k (Xs[k] Xs[k]' - x x');  P *= 1 / k;  P += Q
//   predict (:292-327)                 sigmas_f[k] = fx(point k);  x, P = ckf_transform(sigmas_f, Q)
//   update (:329-390)                  sigmas_h[k] = hx(sigmas_f[k]) -- the points predict() LEFT, not new ones from P;
//                                      zp, S = ckf_transform(sigmas_h, R);  Pxz = sum (sigmas_f[k] - x)(sigmas_h[k] - zp)' / k
//                                      with x as it stands;  K = Pxz inv(S);  x += K (z - zp);  P -= K S K'
//
// Two forms of it here.
//
// The building blocks (ckf_points, ckf_transform, ckf_update) serve arbitrary fx / hx: padded NX x NX arrays, the points read
// through an accessor.  The second moments are summed CENTRED, sum (X - x)(X - x)' -- the reference's sum (X X' - x x') is the
// same number with the cancellation left in (FK_UKF_FLAG_PAIR_WEIGHTS and enkf_kernels.hip's pivot-shifted sums are the
// precedents); P -= K S K' is formed as K Pxz' (K S = Pxz inv(S) S), on the lower triangle and mirrored.
//
// The matrix model (fx = F, hx = H): point k of a +- pair is F x +- sqrt(n) F U[k], so the propagated points are the centre
// c = F x and the n half-differences.  The state carried between predict and update is (x, P, c, E) with
//   E[k] = F U[k]        (k = 0 .. n-1; sigmas_f[k] = c + sqrt(n) E[k], sigmas_f[n + k] = c - sqrt(n) E[k])
// and every sum over the 2n points collapses to one over the n pairs, the sqrt(n) against the 1 / (2n) of the transform:
//   predict   x = c;  P = sum_k E[k] E[k]' + Q
//   update    zp = H c;  G[k] = H E[k];  S = sum_k G[k] G[k]' + R;  Pxz = sum_k E[k] G[k]'   (the (c - x) terms of a pair cancel)
//             K = Pxz inv(S);  y = z - zp;  x += K y;  P -= K Pxz'
// One Cholesky factorisation (n square roots) and one L D L' of S per step; Q never reaches Pxz or S, as in the reference.
//
// Pivots: a pivot of cholesky(P) that is not > 0 sets ST_NOT_PD (chol_lower's rule, fk_math.hpp; the reference's cholesky
// raises); so does a pivot of the L D L' of S (the reference's inv(S) raises for an exactly singular S only).  Root and
// reciprocal of a pivot are fk_ukf.hpp's sqrt_rsqrt.  P and R are symmetric: cholesky reads P's upper triangle like LAPACK's
// dpotrf('U'), the lower triangle of R is read, P and S are written whole and exactly symmetric.
//
// Padded instantiations (n < NX): identity in F, P and R, zeros in Q, H, c and E -- every padded pivot is exactly 1, E's padded
// block the identity, every coupling term an exact zero.
//
// Host-compilable like fk_info.hpp (tests/test_host_ckf.py builds it with g++ and runs it against tests/ckf_port.py).
#pragma once

#include <stdint.h>

#include "fk_math.hpp"
#include "fk_ukf.hpp"

namespace fk {

// L with L L' = P, i.e. L = U' for scipy.linalg.cholesky's upper factor: U[k][j] = L[j * NX + k].  Only j >= k is written.
// Reads P's upper triangle.  Returns true iff every pivot is > 0.
template <int NX>
FK_HD bool ckf_chol(const double (&P)[NX * NX], double (&L)[NX * NX])
{
    bool pd = true;
    FK_UNROLL for (int j = 0; j < NX; ++j) {
        double d = P[j * NX + j];
        FK_UNROLL for (int k = 0; k < j; ++k) d = fma(-L[j * NX + k], L[j * NX + k], d);
        pd = pd && (d > 0.0);
        double ljj, inv;
        sqrt_rsqrt(d, ljj, inv);
        L[j * NX + j] = ljj;
        FK_UNROLL for (int i = j + 1; i < NX; ++i) {
            double s = P[j * NX + i];
            FK_UNROLL for (int k = 0; k < j; ++k) s = fma(-L[i * NX + k], L[j * NX + k], s);
            L[i * NX + j] = s * inv;
        }
    }
    return pd;
}

// ---------------------------------------------------------------------------------------------------- the matrix model --

// predict (:292-327) with fx = F.  x, P: in the posterior, out the prior; c, E: out (see the head of the file).
// Model: rowF, rowQ.  Returns ST_NOT_PD or 0.
template <int NX, class Model>
FK_HD int ckf_linear_predict(double (&x)[NX], double (&P)[NX * NX], double (&c)[NX], double (&E)[NX * NX], const Model &M)
{
    double L[NX * NX];
    const bool pd = ckf_chol<NX>(P, L);
    FK_STAGE();
    FK_UNROLL for (int i = 0; i < NX; ++i) {
        double f[NX];
        M.rowF(i, f);
        c[i] = dot<NX>(f, x);
        FK_UNROLL for (int k = 0; k < NX; ++k) {
            double acc = f[k] * L[k * NX + k];
            FK_UNROLL for (int j = k + 1; j < NX; ++j) acc = fma(f[j], L[j * NX + k], acc);
            E[k * NX + i] = acc;
        }
    }
    FK_UNROLL for (int i = 0; i < NX; ++i) x[i] = c[i];
    FK_STAGE();
    FK_UNROLL for (int i = 0; i < NX; ++i) {
        double q[NX];
        M.rowQ(i, q);
        FK_UNROLL for (int j = 0; j <= i; ++j) {
            double acc = q[j];
            FK_UNROLL for (int k = 0; k < NX; ++k) acc = fma(E[k * NX + i], E[k * NX + j], acc);
            P[i * NX + j] = acc;
            P[j * NX + i] = acc;
        }
    }
    return pd ? 0 : ST_NOT_PD;
}

// update (:329-390) with hx = H, on the points predict left (c, E).  Out: y, K (n x m), S, and the L D L' of S (Lf, dinv: for
// inv_from_ldlt when SI is asked for).  Model: rowH, rowR.  Returns ST_NOT_PD or 0.
template <int NX, int NZ, class Model>
FK_HD int ckf_linear_update(double (&x)[NX], double (&P)[NX * NX], const double (&c)[NX], const double (&E)[NX * NX],
                            const double (&z)[NZ], const Model &M, double (&y)[NZ], double (&K)[NX * NZ],
                            double (&S)[NZ * NZ], double (&Lf)[NZ * NZ], double (&dinv)[NZ])
{
    int st = 0;
    double G[NX * NZ];                                // G[k][r] = H[r] . E[k]
    FK_UNROLL for (int r = 0; r < NZ; ++r) {
        double h[NX];
        M.rowH(r, h);
        y[r] = z[r] - dot<NX>(h, c);
        FK_UNROLL for (int k = 0; k < NX; ++k) {
            double acc = h[0] * E[k * NX];
            FK_UNROLL for (int i = 1; i < NX; ++i) acc = fma(h[i], E[k * NX + i], acc);
            G[k * NZ + r] = acc;
        }
    }
    FK_STAGE();
    FK_UNROLL for (int r = 0; r < NZ; ++r) {
        double rr[NZ];
        M.rowR(r, rr);
        FK_UNROLL for (int s = 0; s <= r; ++s) {
            double acc = rr[s];
            FK_UNROLL for (int k = 0; k < NX; ++k) acc = fma(G[k * NZ + r], G[k * NZ + s], acc);
            S[r * NZ + s] = acc;
            S[s * NZ + r] = acc;
        }
    }
    double Pxz[NX * NZ];
    FK_UNROLL for (int i = 0; i < NX; ++i) {
        FK_UNROLL for (int r = 0; r < NZ; ++r) {
            double acc = E[i] * G[r];
            FK_UNROLL for (int k = 1; k < NX; ++k) acc = fma(E[k * NX + i], G[k * NZ + r], acc);
            Pxz[i * NZ + r] = acc;
            K[i * NZ + r] = acc;
        }
    }
    FK_STAGE();
    if constexpr (NZ == 1) {
        if (!(S[0] > 0.0)) st |= ST_NOT_PD;
        const double si = fk_rcp(S[0]);
        dinv[0] = si;
        Lf[0] = S[0];
        FK_UNROLL for (int i = 0; i < NX; ++i) K[i] = Pxz[i] * si;
    } else {
        double d[NZ];
        FK_UNROLL for (int i = 0; i < NZ * NZ; ++i) Lf[i] = S[i];
        if (!ldlt2<NZ, true>(Lf, d, dinv)) st |= ST_NOT_PD;
        solve_rows_ldlt<NX, NZ>(Lf, dinv, K);
    }
    FK_STAGE();
    FK_UNROLL for (int i = 0; i < NX; ++i) {
        double acc = x[i];
        FK_UNROLL for (int r = 0; r < NZ; ++r) acc = fma(K[i * NZ + r], y[r], acc);
        x[i] = acc;
    }
    FK_UNROLL for (int i = 0; i < NX; ++i) {
        FK_UNROLL for (int j = 0; j <= i; ++j) {
            double acc = P[i * NX + j];
            FK_UNROLL for (int r = 0; r < NZ; ++r) acc = fma(-K[i * NZ + r], Pxz[j * NZ + r], acc);
            P[i * NX + j] = acc;
            P[j * NX + i] = acc;
        }
    }
    return st;
}

// ------------------------------------------------------------------------------------------------ the building blocks --
// Padded NX / NZ arrays with the run-time n / m; loops over the real block only.

// spherical_radial_sigmas (:32-61): put(p, i, v) receives component i of point p (p = 0 .. 2n-1).  Returns true iff SPD.
template <int NX, class Put>
FK_HD bool ckf_points(int n, const double (&x)[NX], const double (&P)[NX * NX], Put put)
{
    double L[NX * NX];
    const bool pd = ckf_chol<NX>(P, L);
    const double rt = sqrt((double)n);
    for (int k = 0; k < n; ++k)
        for (int i = 0; i < n; ++i) {
            const double u = i >= k ? L[i * NX + k] * rt : 0.0;     // U[k][i] * sqrt(n)
            put(k, i, x[i] + u);
            put(n + k, i, x[i] - u);
        }
    return pd;
}

// ckf_transform (:64-98) of k points of dimension d: get(p, i); noise d x d row-major (lower triangle read) or NULL.
// xo, Po (row stride D, exactly symmetric): the real block is written.
template <int D, class Get>
FK_HD void ckf_transform(int d, int k, Get get, const double *noise, double (&xo)[D], double (&Po)[D * D])
{
    const double w = 1.0 / (double)k;
    for (int i = 0; i < d; ++i) {
        double acc = get(0, i);
        for (int p = 1; p < k; ++p) acc += get(p, i);
        xo[i] = acc / (double)k;
        for (int j = 0; j <= i; ++j) Po[i * D + j] = 0.0;
    }
    for (int p = 0; p < k; ++p) {
        double dx[D];
        for (int i = 0; i < d; ++i) dx[i] = get(p, i) - xo[i];
        for (int i = 0; i < d; ++i)
            for (int j = 0; j <= i; ++j) Po[i * D + j] = fma(dx[i], dx[j], Po[i * D + j]);
    }
    for (int i = 0; i < d; ++i)
        for (int j = 0; j <= i; ++j) {
            const double v = noise ? fma(Po[i * D + j], w, noise[i * d + j]) : Po[i * D + j] * w;
            Po[i * D + j] = v;
            Po[j * D + i] = v;
        }
}

// The whole update (:357-379) given both point sets: sf(p, i) = sigmas_f[p][i], sh(p, r) = sigmas_h[p][r], p = 0 .. 2n-1.
// R m x m row-major (lower triangle read).  z_is_y: z already holds residual_z(z, zp).  x, P in place (P's real block, whole
// and symmetric); zp, S, Pxz, K, y out; Lf, dinv: the L D L' of S (padded with the identity).  Returns ST_NOT_PD or 0.
template <int NX, int NZ, class GetF, class GetH>
FK_HD int ckf_update(int n, int m, GetF sf, GetH sh, const double *R, const double (&z)[NZ], bool z_is_y, double (&x)[NX],
                     double (&P)[NX * NX], double (&zp)[NZ], double (&S)[NZ * NZ], double (&Pxz)[NX * NZ],
                     double (&K)[NX * NZ], double (&y)[NZ], double (&Lf)[NZ * NZ], double (&dinv)[NZ])
{
    const int k = 2 * n;
    const double w = 1.0 / (double)k;
    for (int r = 0; r < NZ; ++r) {
        zp[r] = 0.0;
        for (int s = 0; s < NZ; ++s) S[r * NZ + s] = (r == s && r >= m) ? 1.0 : 0.0;
    }
    for (int i = 0; i < NX * NZ; ++i) Pxz[i] = 0.0;
    for (int r = 0; r < m; ++r) {
        double acc = sh(0, r);
        for (int p = 1; p < k; ++p) acc += sh(p, r);
        zp[r] = acc / (double)k;
    }
    for (int p = 0; p < k; ++p) {
        double dz[NZ];
        for (int r = 0; r < m; ++r) dz[r] = sh(p, r) - zp[r];
        for (int r = 0; r < m; ++r)
            for (int s = 0; s <= r; ++s) S[r * NZ + s] = fma(dz[r], dz[s], S[r * NZ + s]);
        for (int i = 0; i < n; ++i) {
            const double dx = sf(p, i) - x[i];
            for (int r = 0; r < m; ++r) Pxz[i * NZ + r] = fma(dx, dz[r], Pxz[i * NZ + r]);
        }
    }
    for (int r = 0; r < m; ++r)
        for (int s = 0; s <= r; ++s) {
            const double v = fma(S[r * NZ + s], w, R[r * m + s]);
            S[r * NZ + s] = v;
            S[s * NZ + r] = v;
        }
    for (int i = 0; i < NX * NZ; ++i) {
        Pxz[i] *= w;
        K[i] = Pxz[i];
    }
    int st = 0;
    double d[NZ];
    for (int i = 0; i < NZ * NZ; ++i) Lf[i] = S[i];
    if (!ldlt2<NZ, true>(Lf, d, dinv)) st |= ST_NOT_PD;
    solve_rows_ldlt<NX, NZ>(Lf, dinv, K);
    for (int r = 0; r < NZ; ++r) y[r] = r < m ? (z_is_y ? z[r] : z[r] - zp[r]) : 0.0;
    for (int i = 0; i < n; ++i) {
        double acc = x[i];
        for (int r = 0; r < m; ++r) acc = fma(K[i * NZ + r], y[r], acc);
        x[i] = acc;
    }
    for (int i = 0; i < n; ++i)
        for (int j = 0; j <= i; ++j) {
            double acc = P[i * NX + j];
            for (int r = 0; r < m; ++r) acc = fma(-K[i * NZ + r], Pxz[j * NZ + r], acc);
            P[i * NX + j] = acc;
            P[j * NX + i] = acc;
        }
    return st;
}

// Kernel arguments of fk_ckf_linear_batch_f64 / fk_ckf_linear_predict_f64 / fk_ckf_linear_update_f64 (ckf_kernels.hip).
struct CkfArgs {
    const double *F, *Q, *H, *R, *z;
    const uint8_t *mask;
    double *x, *P, *pts, *means, *covs, *means_p, *covs_p, *y, *K, *S, *SI;
    int32_t *status;
    long N, T;
    int n, m, nu;
    int phase;          // CKF_STEPS: T steps of predict and update; CKF_PREDICT / CKF_UPDATE: one of them, once
};
enum : int { CKF_STEPS = 0, CKF_PREDICT = 1, CKF_UPDATE = 2 };

}  // namespace fk
