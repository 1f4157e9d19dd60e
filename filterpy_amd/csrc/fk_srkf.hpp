// fk_srkf.hpp -- one step of the square-root Kalman filter (filterpy/kalman/square_root.py:172-248), per track.
//
// Reference (scipy.linalg.qr = LAPACK dgeqrf -> dgeqr2 -> dlarfg at these sizes):
//   predict (:226-248)  x = F x + B u;  R = qr([F P1_2, Q1_2]');  P1_2 = R[:n, :n]'
//   update  (:172-224)  M = [[R2', 0], [(H P1_2)', P1_2']] ((m+n) x (m+n));  r = qr(M);  S1_2 = r[:m, :m]';
//                       SI1_2 = pinv(S1_2);  K = r[:m, m:]' SI1_2;  y = z - H x;  x += K y;  P1_2 = r[m:, m:]'
// The factors are carried as they are: P = P1_2 P1_2' is never formed (forming and re-factoring it would lose what the
// square-root form is for).  Every Householder reflector is LAPACK's: the new diagonal entry of R is -sign(alpha) |column|,
// except that nothing is reflected (R keeps alpha, sign included) when the sub-column below alpha is exactly zero, or when the
// column is the last one of the square M (dlarfg with n = 1) -- so S1_2 and P1_2 carry the reference's signs.
//
// Structure used (the factors are lower triangular: Q1_2, R1_2 and P1_2 -- their upper triangles are never read):
//   predict  the stacked matrix is [(F P1_2)' ; Q1_2'] (2n x n): the bottom block is upper triangular and stays so, reflector j
//            touches the top rows j..n-1 and the bottom rows 0..j -- n+1 entries instead of 2n-j;
//   update   the top-left block R2' is upper triangular and its rows below j are untouched by reflector j, so the m measurement
//            reflectors touch one top row and the n bottom rows each; the top-right block starts as zeros (row j of it is -tau w
//            of reflector j alone); P1_2' below its diagonal is zero for the first reflector; then a plain QR of the n x n
//            bottom-right block, whose last column is not reflected.
// pinv(S1_2) of the reference is the triangular inverse here; a diagonal entry of S1_2 at or below m eps max|diag| sets
// ST_NOT_PD instead (pinv's cutoff would go on with a pseudo-inverse).
//
// Host-compilable like fk_math.hpp (tests/test_host_srkf.py builds it with g++ and runs it against tests/srkf_port.py).
#pragma once

#include <stdint.h>

#include "fk_math.hpp"

namespace fk {

FK_HD double srkf_rcp(double d)
{
    return fk_rcp(d);
}

// dlarfg on (alpha, sub-column with sum of squares ss): returns beta, the new diagonal entry of R; tau and scal (v = x scal,
// v[0] = 1 implied) out.  ss == 0 reflects nothing: tau = 0, beta = alpha, v = 0.
FK_HD double srkf_reflector(double alpha, double ss, double &tau, double &scal)
{
    const bool none = ss == 0.0;
    const double nrm = sqrt(fma(alpha, alpha, ss));
    const double beta = none ? alpha : -copysign(nrm, alpha);
    const double d = alpha - beta;
    scal = none ? 0.0 : srkf_rcp(d);
    tau = none ? 0.0 : -d * srkf_rcp(beta);      // (beta - alpha) / beta
    return beta;
}

// x = F x (+ bu), P1_2 = R[:n, :n]' of qr([F P1_2, Q1_2]').  L = P1_2, row-major, lower triangular (its upper triangle is
// written as zeros).  Model: rowF, rowQ (Q1_2's rows).
template <int NX, class Model>
FK_HD void srkf_predict(double (&x)[NX], double (&L)[NX * NX], const Model &M, const double (&bu)[NX], bool has_u)
{
    // A[r][c] = (F L)'[r][c] = sum_{k >= r} F[c][k] L[k][r]  (the top block);  Bq = Q1_2' (upper triangular)
    double A[NX * NX], Bq[NX * NX];
    {
        double xn[NX];
        FK_UNROLL for (int c = 0; c < NX; ++c) {
            double f[NX];
            M.rowF(c, f);
            xn[c] = dot<NX>(f, x);
            FK_UNROLL for (int r = 0; r < NX; ++r) {
                double acc = f[r] * L[r * NX + r];
                FK_UNROLL for (int k = r + 1; k < NX; ++k) acc = fma(f[k], L[k * NX + r], acc);
                A[r * NX + c] = acc;
            }
        }
        FK_UNROLL for (int i = 0; i < NX; ++i) x[i] = has_u ? xn[i] + bu[i] : xn[i];
    }
    FK_UNROLL for (int c = 0; c < NX; ++c) {
        double q[NX];
        M.rowQ(c, q);
        FK_UNROLL for (int r = 0; r < NX; ++r) Bq[r * NX + c] = r <= c ? q[r] : 0.0;
    }
    FK_STAGE();
    FK_UNROLL for (int j = 0; j < NX; ++j) {
        double ss = 0.0;
        FK_UNROLL for (int i = j + 1; i < NX; ++i) ss = fma(A[i * NX + j], A[i * NX + j], ss);
        FK_UNROLL for (int r = 0; r <= j; ++r) ss = fma(Bq[r * NX + j], Bq[r * NX + j], ss);
        double tau, scal;
        A[j * NX + j] = srkf_reflector(A[j * NX + j], ss, tau, scal);
        double v[NX], vb[NX];
        FK_UNROLL for (int i = j + 1; i < NX; ++i) v[i] = A[i * NX + j] * scal;
        FK_UNROLL for (int r = 0; r <= j; ++r) vb[r] = Bq[r * NX + j] * scal;
        FK_UNROLL for (int c = j + 1; c < NX; ++c) {
            double w = A[j * NX + c];
            FK_UNROLL for (int i = j + 1; i < NX; ++i) w = fma(v[i], A[i * NX + c], w);
            FK_UNROLL for (int r = 0; r <= j; ++r) w = fma(vb[r], Bq[r * NX + c], w);
            const double tw = -tau * w;
            A[j * NX + c] += tw;
            FK_UNROLL for (int i = j + 1; i < NX; ++i) A[i * NX + c] = fma(v[i], tw, A[i * NX + c]);
            FK_UNROLL for (int r = 0; r <= j; ++r) Bq[r * NX + c] = fma(vb[r], tw, Bq[r * NX + c]);
        }
    }
    FK_STAGE();
    FK_UNROLL for (int r = 0; r < NX; ++r)
        FK_UNROLL for (int c = 0; c < NX; ++c) L[r * NX + c] = c <= r ? A[c * NX + r] : 0.0;
}

// The update with z (all of it: the caller skips the call for a missing measurement).  L = P1_2 (prior in, posterior out);
// y, K (n x m), S = S1_2 and SI = SI1_2 (m x m, lower, upper triangles written as zeros) out.  Model: rowH, rowR (R1_2's rows).
// m: the real dim_z (padded instantiations), for the singularity test.  Returns ST_NOT_PD or 0.
template <int NX, int NZ, class Model>
FK_HD int srkf_update(double (&x)[NX], double (&L)[NX * NX], const double (&z)[NZ], const Model &M, int m,
                      double (&y)[NZ], double (&K)[NX * NZ], double (&S)[NZ * NZ], double (&SI)[NZ * NZ])
{
    // the four blocks of M: Zz = R2' (m x m, upper), Zx (m x n, zeros), Xz = (H L)' (n x m), Xx = L' (n x n, upper)
    double Zz[NZ * NZ], Zx[NZ * NX], Xz[NX * NZ], Xx[NX * NX];
    FK_UNROLL for (int c = 0; c < NZ; ++c) {
        double rr[NZ];
        M.rowR(c, rr);
        FK_UNROLL for (int j = 0; j < NZ; ++j) Zz[j * NZ + c] = j <= c ? rr[j] : 0.0;
    }
    FK_UNROLL for (int c = 0; c < NZ; ++c) {
        double h[NX];
        M.rowH(c, h);
        y[c] = z[c] - dot<NX>(h, x);
        FK_UNROLL for (int r = 0; r < NX; ++r) {
            double acc = h[r] * L[r * NX + r];
            FK_UNROLL for (int k = r + 1; k < NX; ++k) acc = fma(h[k], L[k * NX + r], acc);
            Xz[r * NZ + c] = acc;
        }
    }
    FK_UNROLL for (int r = 0; r < NX; ++r)
        FK_UNROLL for (int c = 0; c < NX; ++c) Xx[r * NX + c] = c >= r ? L[c * NX + r] : 0.0;
    FK_STAGE();
    // the m measurement columns: reflector j touches row j of the top block and the n rows of the bottom block
    FK_UNROLL for (int j = 0; j < NZ; ++j) {
        double ss = 0.0;
        FK_UNROLL for (int r = 0; r < NX; ++r) ss = fma(Xz[r * NZ + j], Xz[r * NZ + j], ss);
        double tau, scal;
        Zz[j * NZ + j] = srkf_reflector(Zz[j * NZ + j], ss, tau, scal);
        double v[NX];
        FK_UNROLL for (int r = 0; r < NX; ++r) v[r] = Xz[r * NZ + j] * scal;
        FK_UNROLL for (int c = j + 1; c < NZ; ++c) {
            double w = Zz[j * NZ + c];
            FK_UNROLL for (int r = 0; r < NX; ++r) w = fma(v[r], Xz[r * NZ + c], w);
            const double tw = -tau * w;
            Zz[j * NZ + c] += tw;
            FK_UNROLL for (int r = 0; r < NX; ++r) Xz[r * NZ + c] = fma(v[r], tw, Xz[r * NZ + c]);
        }
        FK_UNROLL for (int c = 0; c < NX; ++c) {
            double w = 0.0;                                   // Zx[j][c] before this reflector
            FK_UNROLL for (int r = 0; r < NX; ++r)
                if (j > 0 || r <= c) w = fma(v[r], Xx[r * NX + c], w);   // (L' is upper triangular until the first reflector)
            const double tw = -tau * w;
            Zx[j * NX + c] = tw;
            FK_UNROLL for (int r = 0; r < NX; ++r) Xx[r * NX + c] = fma(v[r], tw, Xx[r * NX + c]);
        }
    }
    FK_STAGE();
    // the n state columns: a QR of the bottom-right block; its last column is the last of the square M (not reflected)
    FK_UNROLL for (int k = 0; k + 1 < NX; ++k) {
        double ss = 0.0;
        FK_UNROLL for (int i = k + 1; i < NX; ++i) ss = fma(Xx[i * NX + k], Xx[i * NX + k], ss);
        double tau, scal;
        Xx[k * NX + k] = srkf_reflector(Xx[k * NX + k], ss, tau, scal);
        double v[NX];
        FK_UNROLL for (int i = k + 1; i < NX; ++i) v[i] = Xx[i * NX + k] * scal;
        FK_UNROLL for (int c = k + 1; c < NX; ++c) {
            double w = Xx[k * NX + c];
            FK_UNROLL for (int i = k + 1; i < NX; ++i) w = fma(v[i], Xx[i * NX + c], w);
            const double tw = -tau * w;
            Xx[k * NX + c] += tw;
            FK_UNROLL for (int i = k + 1; i < NX; ++i) Xx[i * NX + c] = fma(v[i], tw, Xx[i * NX + c]);
        }
    }
    FK_STAGE();
    // S1_2 = r[:m, :m]', its inverse, and the singularity test on its diagonal
    FK_UNROLL for (int r = 0; r < NZ; ++r)
        FK_UNROLL for (int c = 0; c < NZ; ++c) S[r * NZ + c] = c <= r ? Zz[c * NZ + r] : 0.0;
    double dmax = 0.0;
    FK_UNROLL for (int i = 0; i < NZ; ++i)
        if (i < m) dmax = fmax(dmax, fabs(S[i * NZ + i]));
    const double cut = (double)m * 2.220446049250313e-16 * dmax;
    bool bad = false;
    FK_UNROLL for (int i = 0; i < NZ; ++i)
        if (i < m) bad = bad || !(fabs(S[i * NZ + i]) > cut);
    FK_UNROLL for (int i = 0; i < NZ; ++i) {
        const double di = srkf_rcp(S[i * NZ + i]);
        FK_UNROLL for (int j = 0; j < i; ++j) {
            double acc = S[i * NZ + j] * SI[j * NZ + j];
            FK_UNROLL for (int k = j + 1; k < i; ++k) acc = fma(S[i * NZ + k], SI[k * NZ + j], acc);
            SI[i * NZ + j] = -acc * di;
        }
        SI[i * NZ + i] = di;
        FK_UNROLL for (int j = i + 1; j < NZ; ++j) SI[i * NZ + j] = 0.0;
    }
    // K = r[:m, m:]' SI1_2 (SI lower: K[i][c] = sum_{k >= c} r[k][m+i] SI[k][c]);  x += K y
    FK_UNROLL for (int i = 0; i < NX; ++i) {
        double acc = x[i];
        FK_UNROLL for (int c = 0; c < NZ; ++c) {
            double kc = Zx[c * NX + i] * SI[c * NZ + c];
            FK_UNROLL for (int k = c + 1; k < NZ; ++k) kc = fma(Zx[k * NX + i], SI[k * NZ + c], kc);
            K[i * NZ + c] = kc;
            acc = fma(kc, y[c], acc);
        }
        x[i] = acc;
    }
    // P1_2 = r[m:, m:]'
    FK_UNROLL for (int r = 0; r < NX; ++r)
        FK_UNROLL for (int c = 0; c < NX; ++c) L[r * NX + c] = c <= r ? Xx[c * NX + r] : 0.0;
    return bad ? ST_NOT_PD : 0;
}

// Kernel arguments of fk_srkf_batch_f64 / fk_srkf_predict_f64 / fk_srkf_update_f64 (srkf_kernels.hip).
struct SrkfArgs {
    const double *F, *Q12, *H, *R12, *B, *u, *z;
    const uint8_t *mask;
    double *x, *P12, *means, *covs, *means_p, *covs_p, *y, *K, *S12, *SI12;
    int32_t *status;
    long N, T;
    int n, m, nu, update_first;
    int phase;          // SRKF_STEPS: T steps of predict and update; SRKF_PREDICT / SRKF_UPDATE: one of them, once
};
enum : int { SRKF_STEPS = 0, SRKF_PREDICT = 1, SRKF_UPDATE = 2 };

}  // namespace fk
