// fk_poly.hpp -- the step functions of the fixed-gain polynomial filters (filterpy.gh, filterpy.memory, filterpy.leastsq):
// one recurrence on a state (x, dx, ddx) of ORDER + 1 components, ORDER 0..2 -- predict the polynomial one dt ahead, take the
// residual against z, add a gain times the residual to every component.  poly_kernels.hip instantiates this text; the test-only
// host harness (tests/hostcheck/hostcheck_poly.cpp) compiles the same text with g++.
//
// The bar is BIT IDENTITY with the reference (rlabbe/filterpy v1.4.5), so the association of every sum below is part of the
// specification, and the unit is built with -ffp-contract=off: every line is single IEEE operations.  Three operation orders
// exist in the reference; every scalar named "host" is computed by the Python class with the reference's own expression and
// arrives by value.
//
//   A  multiply  GHFilter.batch_filter (gh/gh_filter.py:433-442), GHKFilter.batch_filter (:729-738), GHFilterOrder order 0
//                (:145-146), FadingMemoryFilter (memory/fading_memory.py:164-194), LeastSquaresFilter order 0
//                (leastsq/least_squares.py:131-133):
//                  xp = (x + dx*dt) + (0.5*ddx)*T2 ; dxp = dx + ddx*dt ; r = z - xp
//                  x' = xp + g0*r ; dx' = dxp + g1*r ; ddx' = ddx + g2*r             (g1 = h/dt, g2 = 2*K/dt**2: host)
//   B  divide    GHFilter.update (:368-375), GHKFilter.update (:666-678), GHFilterOrder orders 1 and 2 (:153-181):
//                  xp, dxp, r as in A ; x' = xp + g0*r ; dx' = dxp + (g1*r)/dt ; ddx' = ddx + (g2*r)/T2
//                                                                                    (g0 = g, g1 = h, g2 = 2*k: host)
//   C  Zarchan   LeastSquaresFilter orders 1 and 2 (:136-154):
//                  y = ((z - x0) - dt*x1) - c*x2
//                  x0' = x0 + (((K0*y) + x1*dt) + c*x2) ; x1' = x1 + ((K1*y) + x2*dt) ; x2' = x2 + K2*y
//                  every right-hand side reads the OLD state; c = 0.5*dt**2 (host)
//
// Terms of a component the order does not have are absent, not multiplied by zero.  Order 0 is x + g0*(z - x).  T2 = dt**2. is
// a host scalar: the device never calls pow.  Form B's `/` is the compiler's fp64 division for gfx950 -- the IEEE scale /
// refine / fix-up sequence (fk_math.hpp, fk_resample_math.hpp), correctly rounded -- not fk_rcp.
//
// `pred` is the predicted position xp (forms A and B: what GHFilter calls x_prediction; order 0: the old x).  Form C never
// forms it in the reference; there pred = (x0 + dt*x1) + c*x2, one more sum that touches no state.  `y` is the residual.
#pragma once

#include "fk_math.hpp"

namespace fk {

enum : int { POLY_FORM_A = 0, POLY_FORM_B = 1, POLY_FORM_C = 2 };

struct PolyConst {
    double dt, T2, c;
};

// is (order, form) one of the seven recurrences?
FK_HD bool poly_supported(int order, int form)
{
    if (form == POLY_FORM_A) return order >= 0 && order <= 2;
    if (form == POLY_FORM_B || form == POLY_FORM_C) return order == 1 || order == 2;
    return false;
}

// One step of one track.  s: the state, in and out; g: the step's gains (g[0..ORDER] are read).
template <int ORDER, int FORM>
FK_HD void poly_step(double (&s)[ORDER + 1], double z, const PolyConst &k, const double (&g)[3], double &pred, double &y)
{
    static_assert(ORDER >= 0 && ORDER <= 2, "order 0..2");
    static_assert(FORM == POLY_FORM_A || ORDER >= 1, "forms B and C start at order 1");
    if constexpr (FORM == POLY_FORM_C) {
        const double x0 = s[0], x1 = s[1];
        if constexpr (ORDER == 1) {
            const double r = (z - x0) - k.dt * x1;
            pred = x0 + k.dt * x1;
            s[0] = x0 + ((g[0] * r) + x1 * k.dt);
            s[1] = x1 + (g[1] * r);
            y = r;
        } else {
            const double x2 = s[2];
            const double r = ((z - x0) - k.dt * x1) - k.c * x2;
            pred = (x0 + k.dt * x1) + k.c * x2;
            s[0] = x0 + (((g[0] * r) + x1 * k.dt) + k.c * x2);
            s[1] = x1 + ((g[1] * r) + x2 * k.dt);
            s[2] = x2 + g[2] * r;
            y = r;
        }
    } else {
        double xp = s[0], dxp = 0.0;
        if constexpr (ORDER >= 1) {
            xp = s[0] + s[1] * k.dt;
            dxp = s[1];
        }
        if constexpr (ORDER == 2) {
            xp = xp + (0.5 * s[2]) * k.T2;
            dxp = s[1] + s[2] * k.dt;
        }
        const double r = z - xp;
        s[0] = xp + g[0] * r;
        if constexpr (ORDER >= 1) s[1] = (FORM == POLY_FORM_A) ? dxp + g[1] * r : dxp + (g[1] * r) / k.dt;
        if constexpr (ORDER == 2) s[2] = (FORM == POLY_FORM_A) ? s[2] + g[2] * r : s[2] + (g[2] * r) / k.T2;
        pred = xp;
        y = r;
    }
}

// The arguments of one launch (poly_dispatch.cpp fills them, poly_kernels.hip reads them).  Strides in doubles: element e of
// track i of a state record sits at e * es + i * ts (soa: es = N, ts = 1; aos: es = 1, ts = order + 1); a history step is
// (order + 1) * N doubles, a step of z / pred / y is N.
struct PolyArgs {
    long N, T, es, ts;
    PolyConst k;
    double g[3];
    const double *gains, *z;
    double *x, *xs, *pred, *y;
};

}  // namespace fk
