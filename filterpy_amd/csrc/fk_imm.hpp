// fk_imm.hpp -- per-track arithmetic of the interacting-multiple-model estimator
// (filterpy/kalman/IMM.py:160-249) on a bank of NM linear Kalman filters whose covariances are
// held packed (upper triangle, fk_math_sym.hpp).  Host/device like fk_math.hpp so the test-only
// host harness can run it against the oracle; the product calls it from imm_kernels.hip, imm_lanes.hip and imm_quad.hip.
#pragma once

#include "fk_math.hpp"
#include "fk_math_sym.hpp"

namespace fk {

// mu-weighted moments of the bank (IMM.py:224-237)
template <int NX, int NM>
FK_HD void imm_estimate(const double (&xs)[NM][NX], const double (&Ps)[NM][NX * (NX + 1) / 2],
                                             const double (&mu)[NM], double (&x)[NX], double (&P)[NX * NX])
{
    FK_UNROLL for (int a = 0; a < NX; ++a) {
        double acc = 0.0;
        FK_UNROLL for (int j = 0; j < NM; ++j) acc = fma(xs[j][a], mu[j], acc);
        x[a] = acc;
    }
    FK_UNROLL for (int k = 0; k < NX * NX; ++k) P[k] = 0.0;
    FK_UNROLL for (int j = 0; j < NM; ++j) {
        double y[NX];
        FK_UNROLL for (int a = 0; a < NX; ++a) y[a] = xs[j][a] - x[a];
        FK_UNROLL for (int a = 0; a < NX; ++a)
            FK_UNROLL for (int b = a; b < NX; ++b)
                P[a * NX + b] = fma(mu[j], fma(y[a], y[b], Ps[j][sym_idx<NX>(a, b)]), P[a * NX + b]);
        FK_STAGE();
    }
    FK_UNROLL for (int a = 0; a < NX; ++a)
        FK_UNROLL for (int b = 0; b < a; ++b) P[a * NX + b] = P[b * NX + a];
}

// MMAEFilterBank's estimate (mmae.py:191-207): x as above; the covariance loop zips the components
// of x with the filters, i.e. filter k is centred on the SCALAR x[k] and only the first
// min(dim_x, n_models) filters contribute -- reproduced as the reference computes it.  n = runtime dim_x.
template <int NX, int NM>
FK_HD void mmae_estimate(const double (&xs)[NM][NX], const double (&Ps)[NM][NX * (NX + 1) / 2],
                         const double (&p)[NM], int n, double (&x)[NX], double (&P)[NX * NX])
{
    FK_UNROLL for (int a = 0; a < NX; ++a) {
        double acc = 0.0;
        FK_UNROLL for (int j = 0; j < NM; ++j) acc = fma(xs[j][a], p[j], acc);
        x[a] = acc;
    }
    FK_UNROLL for (int k = 0; k < NX * NX; ++k) P[k] = 0.0;
    FK_UNROLL for (int k = 0; k < NM; ++k) {
        if (k < NX && k < n) {
            double y[NX];
            FK_UNROLL for (int a = 0; a < NX; ++a) y[a] = xs[k][a] - x[k];
            FK_UNROLL for (int a = 0; a < NX; ++a)
                FK_UNROLL for (int b = 0; b < NX; ++b)
                    P[a * NX + b] = fma(p[k], fma(y[a], y[b], Ps[k][sym_idx<NX>(a, b)]), P[a * NX + b]);
        }
    }
}

// cbar = mu . M  (IMM.py:244); M row-major NM x NM
template <int NM>
FK_HD void imm_mixing_cbar(const double (&mu)[NM], const double *M, double (&cbar)[NM])
{
    FK_UNROLL for (int j = 0; j < NM; ++j) {
        double acc = 0.0;
        FK_UNROLL for (int i = 0; i < NM; ++i) acc = fma(mu[i], M[i * NM + j], acc);
        cbar[j] = acc;
    }
}

// IMMEstimator.predict (IMM.py:200-219): mixed initial conditions with
// omega[i][j] = M[i][j] mu[i] / cbar[j] (IMM.py:245-249), then every filter's own predict.
template <int NX, int NM, class Model>
FK_HD void imm_predict(double (&xs)[NM][NX], double (&Ps)[NM][NX * (NX + 1) / 2], const double (&mu)[NM],
                       const double (&cbar)[NM], const double *M, const Model (&mods)[NM])
{
    // Mixed covariances are formed ELEMENT BY ELEMENT, in place: element (r,c) of every mixed P_j
    // needs only element (r,c) of the old P_i and the spreads y_ij = x_i - x0_j, so the bank is never
    // held twice (same operations and order per element as the reference's loop over filters).
    double w[NM][NM], mx[NM][NX], y[NM][NM][NX];
    FK_UNROLL for (int j = 0; j < NM; ++j) {
        // one reciprocal per column, not NM divisions (a subnormal cbar is scaled first, like the sum in imm_update)
        const bool tiny = cbar[j] < 0x1p-500;
        const double rc = fk_rcp(tiny ? cbar[j] * 0x1p600 : cbar[j]);
        FK_UNROLL for (int i = 0; i < NM; ++i) {
            const double num = M[i * NM + j] * mu[i];
            w[i][j] = (tiny ? num * 0x1p600 : num) * rc;
        }
        FK_UNROLL for (int r = 0; r < NX; ++r) {
            double acc = 0.0;
            FK_UNROLL for (int i = 0; i < NM; ++i) acc = fma(xs[i][r], w[i][j], acc);
            mx[j][r] = acc;
        }
    }
    FK_UNROLL for (int j = 0; j < NM; ++j)
        FK_UNROLL for (int i = 0; i < NM; ++i)
            FK_UNROLL for (int r = 0; r < NX; ++r) y[i][j][r] = xs[i][r] - mx[j][r];
    FK_STAGE();
    FK_UNROLL for (int r = 0; r < NX; ++r) {
        FK_UNROLL for (int c = r; c < NX; ++c) {
            double acc[NM];
            FK_UNROLL for (int j = 0; j < NM; ++j) {
                acc[j] = 0.0;
                FK_UNROLL for (int i = 0; i < NM; ++i)
                    acc[j] = fma(w[i][j], fma(y[i][j][r], y[i][j][c], Ps[i][sym_idx<NX>(r, c)]), acc[j]);
            }
            FK_UNROLL for (int j = 0; j < NM; ++j) Ps[j][sym_idx<NX>(r, c)] = acc[j];
        }
        FK_STAGE();
    }
    FK_UNROLL for (int j = 0; j < NM; ++j) {
        FK_UNROLL for (int r = 0; r < NX; ++r) xs[j][r] = mx[j][r];
        kf_predict_sym<NX>(xs[j], Ps[j], mods[j], 1.0);
    }
}

// IMMEstimator.update (IMM.py:171-179): every filter's update with the same z, its likelihood
// exp(logpdf(y; 0, S)) floored at DBL_MIN (kalman_filter.py:1213-1226), then
// mu = cbar * likelihood, normalised.  m = runtime dim_z (<= NZ).  Returns status bits.
template <int NX, int NZ, int NM, class Model>
FK_HD int imm_update(double (&xs)[NM][NX], double (&Ps)[NM][NX * (NX + 1) / 2], double (&mu)[NM],
                     const double (&cbar)[NM], const double (&z)[NZ], int m, const Model (&mods)[NM],
                     double (&L)[NM], double *ll0 = nullptr)
{
    // ll0 (optional, NM entries): -(m ln 2 pi + ln |S_j|) / 2, the log-density of a ZERO residual under this update's
    // S_j -- what a later update(None) turns into that filter's likelihood (kalman_filter.py:511-520, :1203-1226)
    int st = 0;
    const double log2pi_m = m * 1.8378770664093453;
    // (2 pi)^(-m/2), m = 1..8
    const double cm = m == 1 ? 0.3989422804014327 : m == 2 ? 0.15915494309189535 : m == 3 ? 0.06349363593424097
                    : m == 4 ? 0.025330295910584444 : m == 5 ? 0.010105326013811644 : m == 6 ? 0.004031441804149937
                    : m == 7 ? 0.0016083125866532416 : m == 8 ? 0.000641623890917771 : 1.0;
    FK_UNROLL for (int j = 0; j < NM; ++j) {
        double K[NX * NZ], y[NZ], S[NZ * NZ], Lf[NZ * NZ], dinv[NZ];
        // (SYMM: both triangles of the Joseph form, fk_math_sym.hpp -- one triangle sat AT the bar of tests/imm_hp.py on stiff banks)
        st |= kf_update_sym<NX, NZ, true, true, true>(xs[j], Ps[j], z, mods[j], K, y, S, Lf, dinv);
        double q = 0.0;
        if constexpr (NZ == 1) {
            q = y[0] * y[0] * dinv[0];
        } else {
            double w[NZ];
            FK_UNROLL for (int i = 0; i < NZ; ++i) {
                double acc = y[i];
                FK_UNROLL for (int k2 = 0; k2 < NZ; ++k2)
                    if (k2 < i) acc = fma(-Lf[i * NZ + k2], w[k2], acc);
                w[i] = acc;
                if (i < m) q = fma(acc * acc, dinv[i], q);
            }
        }
        // The density exp(-(m ln 2 pi + ln |S| + q) / 2) as (2 pi)^(-m/2) |S|^(-1/2) exp(-q / 2): |S|^(-1/2) is the root of the
        // product of the reciprocal pivots the factorisation already holds (rsqrt_det_from_dinv: ~15 instructions), where the
        // literal form took a division and a double-precision logarithm PER PIVOT (~105 VALU instructions each: 440 of the
        // 1480 of a (4,2) x 2 bank-step).  No branch anywhere: a fall-back path inside the time loop splits its one basic
        // block and the allocator spills 0.5 KB.  ln |S| itself is only needed for ll0 (the masked instantiations): one
        // logarithm of the same product (logdet_from_dinv).
        // (the root's binary exponent rides inside the one exponential: the two factors would under- / overflow apart --
        //  exp(-q/2) is 0 beyond q ~ 1490 even where a tiny |S| brings the density back into range, and inf * 0 is NaN:
        //  ADVICE r3; same VALU count, no branch)
        int e2;
        const double g = rsqrt_det_parts<NZ>(dinv, m, e2);
        double lj = (cm * g) * exp(fma((double)e2, 0.6931471805599453, -0.5 * q));
        if (lj == 0.0) lj = 2.2250738585072014e-308;
        L[j] = lj;
        if (ll0) ll0[j] = -0.5 * (log2pi_m + logdet_from_dinv<NZ>(dinv, m));
        FK_STAGE();
    }
    double sum = 0.0;
    FK_UNROLL for (int j = 0; j < NM; ++j) { mu[j] = cbar[j] * L[j]; sum += mu[j]; }
    // mu /= sum as a multiplication by the reciprocal (fk_rcp).  Every likelihood floored at DBL_MIN makes the sum subnormal,
    // whose reciprocal overflows: such a bank is scaled by 2^600 first (exact), by selects -- no branch in the time loop.
    {
        const bool tiny = sum < 0x1p-500;
        const double rsum = fk_rcp(tiny ? sum * 0x1p600 : sum);
        FK_UNROLL for (int j = 0; j < NM; ++j) mu[j] = (tiny ? mu[j] * 0x1p600 : mu[j]) * rsum;
    }
    return st;
}

}  // namespace fk
