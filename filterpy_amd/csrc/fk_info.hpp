// fk_info.hpp -- one step of the information filter (filterpy/kalman/information_filter.py:178-289, invertible branch), per track.
//
// Reference (three numpy.linalg.inv of n x n matrices per step, F^-1 precomputed by the F setter):
//   predict (:245-289)  A = F^-T P_inv F^-1;  AI = inv(A);  x = F x + B u;  P_inv = inv(AI + Q)
//   update  (:178-243)  y = z - H x;  S = P_inv + H' R_inv H;  K = inv(S) H' R_inv;  x += K y;  P_inv = S
// AI is F P F' with P = inv(P_inv), so the step here is two factorisations of symmetric positive definite n x n matrices and
// no F^-1:
//   predict  P = inv(P_inv);  Pp = F P F' + Q (lower triangle computed, mirrored);  P_inv = inv(Pp)
//   update   P_inv += G, G = H' R_inv H;  P = inv(P_inv);  x += P (HtRi y), HtRi = H' R_inv;  K = P HtRi only when asked for
// G and HtRi belong to the model: the caller computes them once (info_htri_entry / info_g_entry) and hands them over through
// the Model policy (rowG, rowHtRi) next to rowF, rowQ and rowH.
// inv(.) is info_spd_inv: L D L' of the lower triangle (pivot reciprocals from fk_rcp), the inverse of the unit triangle, and
// L^-T D^-1 L^-1 formed on the lower triangle and mirrored -- n^3 / 2 FMAs, exactly symmetric.
//
// Bit-identity: the state between steps is x and P_inv alone.  predict starts from info_spd_inv of the stored P_inv; directly
// after an update it may reuse that update's P (have_P), which IS info_spd_inv of the stored P_inv -- the same operations on
// the same bits.  After a predict P holds Pp and is never carried over.  Every multiply-add is an explicit fma and no product
// feeds a plain addition, so the compiler's contraction has nothing to decide differently at the two inline sites.
//
// Singularity: a pivot at or below n eps max|diag| of the matrix being factored sets ST_NOT_PD (fk_srkf.hpp's rule).  The
// reference's _no_information branch (an exactly singular A) is not ported.
//
// Padded instantiations (n < NX): identity in F and P_inv, zeros in Q, H, G and HtRi.  Every pivot of the padded block is
// exactly 1, every coupling term an exact zero appended to the real sums, so the real block is the exact instantiation's.
//
// Host-compilable like fk_math.hpp (tests/test_host_info.py builds it with g++ and runs it against tests/info_port.py).
#pragma once

#include <stdint.h>

#include "fk_math.hpp"

namespace fk {

// HtRi[i][c] = sum_k H[k][i] R_inv[k][c]  (H m x n, R_inv m x m, both C order)
FK_HD double info_htri_entry(const double *H, const double *Ri, int n, int m, int i, int c)
{
    double acc = H[i] * Ri[c];
    for (int k = 1; k < m; ++k) acc = fma(H[k * n + i], Ri[k * m + c], acc);
    return acc;
}

// G[i][j] = sum_c HtRi[i][c] H[c][j] from row i of HtRi.  Callers compute j <= i and mirror: G is exactly symmetric.
FK_HD double info_g_entry(const double *htri_row, const double *H, int n, int m, int j)
{
    double acc = htri_row[0] * H[j];
    for (int c = 1; c < m; ++c) acc = fma(htri_row[c], H[c * n + j], acc);
    return acc;
}

// The model held in plain arrays (the host harness; padded by the caller).
template <int NX, int NZ>
struct InfoRegModel {
    double F[NX * NX], Q[NX * NX], H[NZ * NX], G[NX * NX], HtRi[NX * NZ];
    FK_HD void rowF(int i, double (&r)[NX]) const { FK_UNROLL for (int j = 0; j < NX; ++j) r[j] = F[i * NX + j]; }
    FK_HD void rowQ(int i, double (&r)[NX]) const { FK_UNROLL for (int j = 0; j < NX; ++j) r[j] = Q[i * NX + j]; }
    FK_HD void rowH(int i, double (&r)[NX]) const { FK_UNROLL for (int j = 0; j < NX; ++j) r[j] = H[i * NX + j]; }
    FK_HD void rowG(int i, double (&r)[NX]) const { FK_UNROLL for (int j = 0; j < NX; ++j) r[j] = G[i * NX + j]; }
    FK_HD void rowHtRi(int i, double (&r)[NZ]) const { FK_UNROLL for (int j = 0; j < NZ; ++j) r[j] = HtRi[i * NZ + j]; }
};

// AI = A^-1 for a symmetric positive definite A; only A's lower triangle is read, AI is written whole and exactly symmetric.
// n: the real dimension (padded instantiations), for the singularity test.  Returns true when a pivot is at or below
// n eps max|diag A| (or is not a number).
template <int NX>
FK_HD bool info_spd_inv(const double (&A)[NX * NX], double (&AI)[NX * NX], int n)
{
    double L[NX * NX], M[NX * NX], dinv[NX];          // strict lower triangles: L of A = L D L', M = L^-1 and then D^-1 M
    double dmax = 0.0;
    FK_UNROLL for (int i = 0; i < NX; ++i)
        if (i < n) dmax = fmax(dmax, fabs(A[i * NX + i]));
    const double cut = (double)n * 2.220446049250313e-16 * dmax;
    bool bad = false;
    FK_UNROLL for (int j = 0; j < NX; ++j) {
        // v[k] = L[j][k] d[k] sits in M's row j until the row is taken for L^-1 below
        double dj = A[j * NX + j];
        FK_UNROLL for (int k = 0; k < j; ++k) dj = fma(-L[j * NX + k], M[j * NX + k], dj);
        if (j < n) bad = bad || !(dj > cut);
        const double di = fk_rcp(dj);
        dinv[j] = di;
        FK_UNROLL for (int i = j + 1; i < NX; ++i) {
            double s = A[i * NX + j];
            FK_UNROLL for (int k = 0; k < j; ++k) s = fma(-L[i * NX + k], M[j * NX + k], s);
            M[i * NX + j] = s;                        // L[i][j] d[j]
            L[i * NX + j] = s * di;
        }
    }
    FK_STAGE();
    // M = L^-1 (unit lower triangular): M[i][j] = -(L[i][j] + sum_{j < k < i} L[i][k] M[k][j])
    FK_UNROLL for (int i = 1; i < NX; ++i) {
        FK_UNROLL for (int j = 0; j < i; ++j) {
            double acc = L[i * NX + j];
            FK_UNROLL for (int k = j + 1; k < i; ++k) acc = fma(L[i * NX + k], M[k * NX + j], acc);
            M[i * NX + j] = -acc;
        }
    }
    FK_STAGE();
    // AI = M' D^-1 M on the lower triangle: AI[i][j] = sum_{k >= i} M[k][i] dinv[k] M[k][j], M[i][i] = 1.  L's triangle takes
    // W = D^-1 M.
    FK_UNROLL for (int k = 1; k < NX; ++k)
        FK_UNROLL for (int j = 0; j < k; ++j) L[k * NX + j] = dinv[k] * M[k * NX + j];
    FK_UNROLL for (int i = 0; i < NX; ++i) {
        FK_UNROLL for (int j = 0; j <= i; ++j) {
            double acc = (j < i) ? L[i * NX + j] : dinv[i];
            FK_UNROLL for (int k = i + 1; k < NX; ++k) acc = fma(M[k * NX + i], L[k * NX + j], acc);
            AI[i * NX + j] = acc;
            AI[j * NX + i] = acc;
        }
    }
    return bad;
}

// x = F x (+ bu);  P_inv = inv(F inv(P_inv) F' + Q).  Pi = P_inv (in: prior of the last step, out: predicted); P: scratch the
// caller keeps -- with have_P it holds info_spd_inv(Pi) from the update just before, on return it holds Pp (do not carry it).
// Model: rowF, rowQ.  Returns ST_NOT_PD or 0.
template <int NX, class Model>
FK_HD int info_predict(double (&x)[NX], double (&Pi)[NX * NX], double (&P)[NX * NX], bool have_P, const Model &M,
                       const double (&bu)[NX], bool has_u, int n)
{
    bool bad = false;
    if (!have_P) bad = info_spd_inv<NX>(Pi, P, n);
    FK_STAGE();
    double FP[NX * NX];
    {
        double xn[NX];
        FK_UNROLL for (int i = 0; i < NX; ++i) {
            double f[NX];
            M.rowF(i, f);
            xn[i] = dot<NX>(f, x);
            FK_UNROLL for (int j = 0; j < NX; ++j) {
                double acc = f[0] * P[j];
                FK_UNROLL for (int k = 1; k < NX; ++k) acc = fma(f[k], P[k * NX + j], acc);
                FP[i * NX + j] = acc;
            }
        }
        FK_UNROLL for (int i = 0; i < NX; ++i) x[i] = has_u ? xn[i] + bu[i] : xn[i];
    }
    FK_STAGE();
    // Pp = (F P) F' + Q on the lower triangle: column j needs row j of F
    FK_UNROLL for (int j = 0; j < NX; ++j) {
        double f[NX];
        M.rowF(j, f);
        FK_UNROLL for (int i = j; i < NX; ++i) {
            double acc = FP[i * NX] * f[0];
            FK_UNROLL for (int k = 1; k < NX; ++k) acc = fma(FP[i * NX + k], f[k], acc);
            P[i * NX + j] = acc;
        }
    }
    FK_UNROLL for (int i = 0; i < NX; ++i) {
        double q[NX];
        M.rowQ(i, q);
        FK_UNROLL for (int j = 0; j <= i; ++j) P[i * NX + j] += q[j];
    }
    FK_STAGE();
    bad = info_spd_inv<NX>(P, Pi, n) || bad;
    return bad ? ST_NOT_PD : 0;
}

// The update with z (the caller skips the call for a missing measurement).  Pi = P_inv (prior in, its lower triangle read;
// posterior = the reference's S out, whole and exactly symmetric); P = info_spd_inv(Pi) out (the next predict may reuse it); y out; K (n x m) only when want_K.  Model: rowH, rowG,
// rowHtRi.  Returns ST_NOT_PD or 0.
template <int NX, int NZ, class Model>
FK_HD int info_update(double (&x)[NX], double (&Pi)[NX * NX], double (&P)[NX * NX], const double (&z)[NZ], const Model &M,
                      int n, double (&y)[NZ], double (&K)[NX * NZ], bool want_K)
{
    FK_UNROLL for (int c = 0; c < NZ; ++c) {
        double h[NX];
        M.rowH(c, h);
        y[c] = z[c] - dot<NX>(h, x);
    }
    double w[NX];
    FK_UNROLL for (int i = 0; i < NX; ++i) {
        double r[NZ], g[NX];
        M.rowHtRi(i, r);
        w[i] = dot<NZ>(r, y);
        M.rowG(i, g);
        FK_UNROLL for (int j = 0; j <= i; ++j) {
            Pi[i * NX + j] += g[j];
            Pi[j * NX + i] = Pi[i * NX + j];
        }
    }
    FK_STAGE();
    const bool bad = info_spd_inv<NX>(Pi, P, n);
    FK_STAGE();
    FK_UNROLL for (int i = 0; i < NX; ++i) {
        double acc = x[i];
        FK_UNROLL for (int j = 0; j < NX; ++j) acc = fma(P[i * NX + j], w[j], acc);
        x[i] = acc;
    }
    if (want_K) {
        FK_UNROLL for (int j = 0; j < NX; ++j) {
            double r[NZ];
            M.rowHtRi(j, r);
            FK_UNROLL for (int i = 0; i < NX; ++i)
                FK_UNROLL for (int c = 0; c < NZ; ++c)
                    K[i * NZ + c] = (j == 0) ? P[i * NX] * r[c] : fma(P[i * NX + j], r[c], K[i * NZ + c]);
        }
    }
    return bad ? ST_NOT_PD : 0;
}

// Kernel arguments of fk_info_batch_f64 / fk_info_predict_f64 / fk_info_update_f64 (info_kernels.hip).
struct InfoArgs {
    const double *F, *Q, *H, *Rinv, *B, *u, *z;
    const uint8_t *mask;
    double *x, *Pinv, *means, *covs, *means_p, *covs_p, *y, *K;
    int32_t *status;
    long N, T;
    int n, m, nu, update_first;
    int phase;          // INFO_STEPS: T steps of predict and update; INFO_PREDICT / INFO_UPDATE: one of them, once
};
enum : int { INFO_STEPS = 0, INFO_PREDICT = 1, INFO_UPDATE = 2 };

}  // namespace fk
