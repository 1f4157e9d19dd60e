// fk_ukf_simplex.hpp -- one predict + update step of the fused linear-model UKF on the SIMPLEX point set (n + 1 points,
// filterpy/kalman/sigma_points.py:386-534) and one backward step of its smoother: the arithmetic of ukf_simplex.hip.
// __host__ __device__ like fk_ukf.hpp: the kernel runs it per lane, tests/hostcheck/hostcheck_simplex.cpp runs the very same
// text on the host against the live-reference goldens.
//
// The point set.  sigma_points.py:499-513 forms  sigmas = x + U' I  with U = cholesky(P) (upper; no scaling) and the constant
// n x (n + 1) matrix I = sqrt(n) Istar (:501-509).  Row r of I (0-based) holds ONE value a_r in the columns 0..r, one value
// b_r in column r + 1 and zeros behind it, so with L = U' (lower) the deviation of point j from the mean is
//     d_j = b_{j-1} L[:, j-1] + s_j ,    s_j = sum_{r >= j} a_r L[:, r]      (d_0 = s_0;  s_n = 0)
// a suffix sum over the columns of the factor.  simplex_deviations() forms all n + 1 of them in one backward sweep over the
// columns (the column r is read once: b_r times it is point r + 1's own term, a_r times it joins the running sum).
// For fx(x) = F x the images are F x + (the same sweep over the columns of F L) -- ukf_linear_step_v3's factor-image
// organisation: one pass over the rows of F gives F x and F L, no point is pushed through F on its own.  Likewise H.
// The weights Wm / Wc (n + 1 each) are applied as given, point by point in index order (unscented_transform.py:104-126,
// UKF.py:483-497): nothing here assumes them equal or summing to 1.  The offsets of the images from their weighted mean are
// formed as (F x - mean) + deviation, which keeps the digits of the deviation (see ukf_linear_step_v3).
//
// The table (a_r, b_r) comes from the HOST (simplex_table below: sqrt and the divisions in the reference's operation order,
// correctly rounded) and reaches the step through the view:
//   fresh() returns {sm, Wm, Wc, Sa, Sb}: the shared model (rowF / rowQ / rowH / rowR), the weights padded to NX + 1 points
//   (weight 0 behind point n) and the table padded to NX rows (a_r = b_r = 0 from row n on).  A padded instantiation then
//   computes on a factor whose padded block is the identity: every padded column is multiplied by 0, every padded point has
//   deviation 0 and weight 0.
#pragma once

#include <math.h>

#include "fk_ukf.hpp"

namespace fk {

constexpr int SIMPLEX_MAX_NX = 9;

// a_r, b_r of the n x (n + 1) matrix I = sqrt(n) Istar, by value (kernel argument); rows >= n are 0
struct SimplexTable {
    double a[SIMPLEX_MAX_NX], b[SIMPLEX_MAX_NX];
};

// sigma_points.py:501-509 in its operation order.  Row 1 is [-1/sqrt(2 lambda), +1/sqrt(2 lambda)] -- the general rule
// negated --, row d >= 2 is 1./sqrt(lambda d (d+1)) in the columns 0..d-1 and -d/sqrt(lambda d (d+1)) in column d; the whole
// matrix is then multiplied by sqrt(n).  Host only: the table is the same for every track, and the device's
// sqrt has not been held to the host's bits (its fp64 `/` has: docs/KERNEL_NOTES.md, "polynomial filters").
inline SimplexTable simplex_table(int n)
{
    SimplexTable t;
    for (int r = 0; r < SIMPLEX_MAX_NX; ++r) t.a[r] = t.b[r] = 0.0;
    if (n < 1 || n > SIMPLEX_MAX_NX) return t;
    const double lambda = (double)n / (double)(n + 1);
    const double sn = sqrt((double)n);
    t.a[0] = sn * (-1.0 / sqrt(2.0 * lambda));
    t.b[0] = sn * (1.0 / sqrt(2.0 * lambda));
    for (int d = 2; d <= n; ++d) {
        const double root = sqrt(lambda * d * (d + 1));      // (lambda_*d*(d + 1): left to right)
        t.a[d - 1] = sn * (1.0 * 1. / root);
        t.b[d - 1] = sn * (-(double)d / root);
    }
    return t;
}

// The deviations of the NX + 1 points in the image of an R-row linear map M: C[r][k] = (M L)[r][k] in, E0 / C out with
// E0[r] = deviation of point 0, C[r][k] = deviation of point k + 1 (in place: column k is spent when point k + 1 is formed).
template <int R, int NX>
FK_HD void simplex_deviations(double (&C)[R][NX], double (&E0)[R], const double *Sa, const double *Sb)
{
    FK_UNROLL for (int r = 0; r < R; ++r) E0[r] = 0.0;
    FK_UNROLL for (int k = NX - 1; k >= 0; --k) {
        const double ak = Sa[k], bk = Sb[k];
        FK_UNROLL for (int r = 0; r < R; ++r) {
            const double c = C[r][k];
            C[r][k] = fma(bk, c, E0[r]);
            E0[r] = fma(ak, c, E0[r]);
        }
    }
}

// The same sweep over the columns of the packed lower factor itself: D[i][j] = component i of the deviation of point j
// (j = 0..NX).  Column r of L is zero above its diagonal, so D[i][j] is an exact zero for j > i + 1: those entries are
// neither formed nor read (simplex_dev_nonzero).
constexpr bool simplex_dev_nonzero(int i, int j) { return j <= i + 1; }

template <int NX>
FK_HD void simplex_factor_deviations(const double (&L)[NX * (NX + 1) / 2], double (&D)[NX][NX + 1], const double *Sa, const double *Sb)
{
    FK_UNROLL for (int i = 0; i < NX; ++i) {
        double s = 0.0;
        FK_UNROLL for (int k = NX - 1; k >= 0; --k) {
            if (k > i) continue;                                   // L[i][k] = 0
            const double c = L[sym_idx<NX>(i, k)];
            D[i][k + 1] = fma(Sb[k], c, s);
            s = fma(Sa[k], c, s);
        }
        D[i][0] = s;
    }
}

// image of the state and of the factor under an R-row map whose rows come from row(r, buf): Mx = M x, ML = M L
template <int R, int NX, class Row>
FK_HD void simplex_map(Row &&row, const double (&x)[NX], const double (&L)[NX * (NX + 1) / 2], double (&Mx)[R], double (&ML)[R][NX])
{
    FK_UNROLL for (int r = 0; r < R; ++r) {
        double f[NX];
        row(r, f);
        Mx[r] = dot<NX>(f, x);
        FK_UNROLL for (int k = 0; k < NX; ++k) {
            double acc = f[k] * L[sym_idx<NX>(k, k)];
            FK_UNROLL for (int c = 0; c < NX; ++c)
                if (c > k) acc = fma(f[c], L[sym_idx<NX>(c, k)], acc);
            ML[r][k] = acc;
        }
        FK_STAGE();
    }
}

// mean = sum_j W_j (Mx + dev_j), index order; afterwards Mx holds Mx - mean (the centre's offset, made opaque so that the
// second sweep re-forms the offsets instead of holding all of them)
template <int R, int NX>
FK_HD void simplex_mean(const double *W, double (&Mx)[R], const double (&E0)[R], const double (&E)[R][NX], double (&mean)[R])
{
    FK_UNROLL for (int r = 0; r < R; ++r) mean[r] = W[0] * (Mx[r] + E0[r]);
    FK_UNROLL for (int k = 0; k < NX; ++k)
        FK_UNROLL for (int r = 0; r < R; ++r) mean[r] = fma(W[1 + k], Mx[r] + E[r][k], mean[r]);
    FK_UNROLL for (int r = 0; r < R; ++r) Mx[r] -= mean[r];
    FK_UNROLL for (int r = 0; r < R; ++r) FK_OPAQUE(Mx[r]);
}

// One predict + update step (UKF.py:400-411, 462-481) on the simplex set.
//   predict  L = chol(P) ; sf_j = F x + F d_j ; x- = sum Wm_j sf_j ; P- = sum Wc_j (sf_j - x-)(.)' + Q
//   update   L = chol(P-), the points regenerated (UKF.py:407) ; sh_j = H x- + H d_j ; zp = sum Wm_j sh_j ;
//            S = sum Wc_j (sh_j - zp)(.)' + R ; Pxz = sum Wc_j d_j (sh_j - zp)' ; K = Pxz S^-1 ; x = x- + K (z - zp) ; P = P- - K S K'
// (sigma_j - x- = d_j: the reference's (x + d) - x differs from d by one rounding of x, like in ukf_linear_step_v3).
template <int NX, int NZ, class LoadZ, class Fresh>
FK_HD int ukf_simplex_step(double (&x)[NX], double (&P)[NX * (NX + 1) / 2], LoadZ &&load_z, bool has_z, Fresh &&fresh)
{
    constexpr int PL = NX * (NX + 1) / 2;
    int st = 0;
    // ---------------- predict
    {
        double Fx[NX], E0[NX], E[NX][NX];
        {
            double L[PL];
            if (!chol_packed_rs<NX>(P, 1.0, L)) st |= ST_NOT_PD;
            const auto mv = fresh();
            simplex_map<NX, NX>([&](int r, double (&f)[NX]) { mv.sm.rowF(r, f); }, x, L, Fx, E);
            const auto tv = fresh(E[NX - 1][NX - 1]);
            simplex_deviations<NX, NX>(E, E0, tv.Sa, tv.Sb);
        }
        FK_STAGE();
        {
            const auto mv = fresh(E0[NX - 1]);
            simplex_mean<NX, NX>(mv.Wm, Fx, E0, E, x);
        }
        FK_STAGE();
        FK_UNROLL for (int j = 0; j < NX + 1; ++j) {
            const double wc = fresh(j ? P[PL - 1] : x[NX - 1]).Wc[j];
            double y[NX], wy[NX];
            FK_UNROLL for (int r = 0; r < NX; ++r) y[r] = Fx[r] + (j == 0 ? E0[r] : E[r][(j + NX - 1) % NX]);
            FK_UNROLL for (int r = 0; r < NX; ++r) wy[r] = wc * y[r];
            FK_UNROLL for (int a2 = 0; a2 < NX; ++a2)
                FK_UNROLL for (int b = 0; b < NX; ++b)
                    if (b >= a2) P[sym_idx<NX>(a2, b)] = (j == 0) ? y[a2] * wy[b] : fma(y[a2], wy[b], P[sym_idx<NX>(a2, b)]);
            FK_STAGE();
        }
        FK_UNROLL for (int e = 0; e < PL; ++e) FK_OPAQUE(P[e]);         // every sum complete before the rows of Q are read
        const auto mv = fresh(P[PL - 1]);
        FK_UNROLL for (int r = 0; r < NX; ++r) {
            double q[NX];
            mv.sm.rowQ(r, q);
            FK_UNROLL for (int b = 0; b < NX; ++b)
                if (b >= r) P[sym_idx<NX>(r, b)] += q[b];
        }
    }
    // ---------------- update, sigma points regenerated from the prior
    if (has_z) {
        double z[NZ];
        load_z(z);
        double D[NX][NX + 1];
        double Hx[NZ], G0[NZ], G[NZ][NX];
        {
            double L[PL];
            if (!chol_packed_rs<NX>(P, 1.0, L)) st |= ST_NOT_PD;
            const auto mv = fresh();
            simplex_map<NZ, NX>([&](int r, double (&h)[NX]) { mv.sm.rowH(r, h); }, x, L, Hx, G);
            const auto tv = fresh(G[NZ - 1][NX - 1]);
            simplex_deviations<NZ, NX>(G, G0, tv.Sa, tv.Sb);
            simplex_factor_deviations<NX>(L, D, tv.Sa, tv.Sb);
        }
        FK_STAGE();
        double zp[NZ];
        {
            const auto mv = fresh(G0[NZ - 1]);
            simplex_mean<NZ, NX>(mv.Wm, Hx, G0, G, zp);
        }
        double S[NZ * NZ], K[NX * NZ];
        FK_UNROLL for (int j = 0; j < NX + 1; ++j) {
            const double wc = fresh(j ? S[NZ * NZ - 1] : zp[NZ - 1]).Wc[j];
            double d[NZ], wd[NZ];
            FK_UNROLL for (int r = 0; r < NZ; ++r) d[r] = Hx[r] + (j == 0 ? G0[r] : G[r][(j + NX - 1) % NX]);
            FK_UNROLL for (int r = 0; r < NZ; ++r) wd[r] = wc * d[r];
            // upper triangle; the lower one is its mirror image (the reference's w * outer(d, d) is symmetric bit for bit)
            FK_UNROLL for (int r = 0; r < NZ; ++r)
                FK_UNROLL for (int c = 0; c < NZ; ++c)
                    if (c >= r) S[r * NZ + c] = (j == 0) ? d[r] * wd[c] : fma(d[r], wd[c], S[r * NZ + c]);
            // row i of Pxz receives its first term from point 0 (D[i][0] exists for every i)
            FK_UNROLL for (int i = 0; i < NX; ++i) {
                if (!simplex_dev_nonzero(i, j)) continue;
                FK_UNROLL for (int c = 0; c < NZ; ++c)
                    K[i * NZ + c] = (j == 0) ? D[i][j] * wd[c] : fma(D[i][j], wd[c], K[i * NZ + c]);
            }
            FK_STAGE();
        }
        FK_UNROLL for (int r = 0; r < NZ; ++r)
            FK_UNROLL for (int c = 0; c < NZ; ++c)
                if (c < r) S[r * NZ + c] = S[c * NZ + r];
        FK_UNROLL for (int e = 0; e < NZ * NZ; ++e) FK_OPAQUE(S[e]);
        FK_UNROLL for (int e = 0; e < NX * NZ; ++e) FK_OPAQUE(K[e]);
        {
            const auto mv = fresh(S[NZ * NZ - 1]);
            FK_UNROLL for (int r = 0; r < NZ; ++r) {
                double rr[NZ];
                mv.sm.rowR(r, rr);
                FK_UNROLL for (int c = 0; c < NZ; ++c) S[r * NZ + c] += rr[c];
            }
        }
        // K = Pxz S^-1
        double Lf[NZ * NZ], dd[NZ], dinv[NZ];
        FK_UNROLL for (int e = 0; e < NZ * NZ; ++e) Lf[e] = S[e];
        if (!ldlt2_rs<NZ>(Lf, dd, dinv)) st |= ST_NOT_PD;
        solve_rows_ldlt<NX, NZ>(Lf, dinv, K);
        // x += K (z - zp)
        FK_UNROLL for (int c = 0; c < NZ; ++c) z[c] -= zp[c];
        FK_UNROLL for (int r = 0; r < NX; ++r) {
            double acc = K[r * NZ] * z[0];
            FK_UNROLL for (int c = 1; c < NZ; ++c) acc = fma(K[r * NZ + c], z[c], acc);
            x[r] += acc;
        }
        // P -= K (S K'), upper triangle
        FK_UNROLL for (int c2 = 0; c2 < NX; ++c2) {
            double sk[NZ];                 // column c2 of S K'
            FK_UNROLL for (int q = 0; q < NZ; ++q) {
                double acc = S[q * NZ] * K[c2 * NZ];
                FK_UNROLL for (int w = 1; w < NZ; ++w) acc = fma(S[q * NZ + w], K[c2 * NZ + w], acc);
                sk[q] = acc;
            }
            FK_UNROLL for (int r = 0; r < NX; ++r)
                if (r <= c2) {
                    double acc = K[r * NZ] * sk[0];
                    FK_UNROLL for (int q = 1; q < NZ; ++q) acc = fma(K[r * NZ + q], sk[q], acc);
                    P[sym_idx<NX>(r, c2)] -= acc;
                }
            FK_STAGE();
        }
    }
    return st;
}

// The gain of one backward step of rts_smoother (UKF.py:714-732) on the simplex set; ukf_linear_rts_correct (fk_ukf.hpp)
// finishes the step.  (x, P): the filter's output of step k;  xb, Pb (packed), K (full n x n) out.
//   sf_j = F x + F d_j ; (xb, Pb) = UT(sf, Wm, Wc, Q) ; Pxb = sum Wc_j d_j (sf_j - xb)' ; K = Pxb inv(Pb)
template <int NX, class Fresh>
FK_HD int ukf_simplex_rts_gain(const double (&x)[NX], const double (&P)[NX * (NX + 1) / 2], double (&xb)[NX],
                               double (&Pb)[NX * (NX + 1) / 2], double (&K)[NX * NX], Fresh &&fresh)
{
    constexpr int PL = NX * (NX + 1) / 2;
    int st = 0;
    double D[NX][NX + 1];
    double Fx[NX], E0[NX], E[NX][NX];
    {
        double L[PL];
        if (!chol_packed_rs<NX>(P, 1.0, L)) st |= ST_NOT_PD;
        const auto mv = fresh();
        simplex_map<NX, NX>([&](int r, double (&f)[NX]) { mv.sm.rowF(r, f); }, x, L, Fx, E);
        const auto tv = fresh(E[NX - 1][NX - 1]);
        simplex_deviations<NX, NX>(E, E0, tv.Sa, tv.Sb);
        simplex_factor_deviations<NX>(L, D, tv.Sa, tv.Sb);
    }
    FK_STAGE();
    {
        const auto mv = fresh(E0[NX - 1]);
        simplex_mean<NX, NX>(mv.Wm, Fx, E0, E, xb);
    }
    FK_STAGE();
    FK_UNROLL for (int j = 0; j < NX + 1; ++j) {
        const double wc = fresh(j ? Pb[PL - 1] : xb[NX - 1]).Wc[j];
        double y[NX], wy[NX];
        FK_UNROLL for (int r = 0; r < NX; ++r) y[r] = Fx[r] + (j == 0 ? E0[r] : E[r][(j + NX - 1) % NX]);
        FK_UNROLL for (int r = 0; r < NX; ++r) wy[r] = wc * y[r];
        FK_UNROLL for (int a2 = 0; a2 < NX; ++a2)
            FK_UNROLL for (int b = 0; b < NX; ++b)
                if (b >= a2) Pb[sym_idx<NX>(a2, b)] = (j == 0) ? y[a2] * wy[b] : fma(y[a2], wy[b], Pb[sym_idx<NX>(a2, b)]);
        FK_UNROLL for (int i = 0; i < NX; ++i) {
            if (!simplex_dev_nonzero(i, j)) continue;
            FK_UNROLL for (int c = 0; c < NX; ++c)
                K[i * NX + c] = (j == 0) ? D[i][j] * wy[c] : fma(D[i][j], wy[c], K[i * NX + c]);
        }
        FK_STAGE();
    }
    FK_UNROLL for (int e = 0; e < PL; ++e) FK_OPAQUE(Pb[e]);
    {
        const auto mv = fresh(Pb[PL - 1]);
        FK_UNROLL for (int r = 0; r < NX; ++r) {
            double q[NX];
            mv.sm.rowQ(r, q);
            FK_UNROLL for (int b = 0; b < NX; ++b)
                if (b >= r) Pb[sym_idx<NX>(r, b)] += q[b];
        }
    }
    // K = Pxb inv(Pb)
    {
        double Lp[PL], d[NX], dinv[NX];
        FK_UNROLL for (int e = 0; e < PL; ++e) Lp[e] = Pb[e];
        if (!ldlt_packed_rs<NX>(Lp, d, dinv)) st |= ST_NOT_PD;
        FK_UNROLL for (int r = 0; r < NX; ++r) {
            double row[NX];
            FK_UNROLL for (int c = 0; c < NX; ++c) row[c] = K[r * NX + c];
            solve_row_packed<NX>(Lp, dinv, row);
            FK_UNROLL for (int c = 0; c < NX; ++c) K[r * NX + c] = row[c];
        }
    }
    FK_STAGE();
    return st;
}

}  // namespace fk
