// Host harness for the step functions of the polynomial filters: filterpy_amd/csrc/fk_poly.hpp -- the very text
// poly_kernels.hip instantiates -- compiled with g++ -O1 -ffp-contract=off (tests/test_hostcheck_poly.py builds it) and run
// track by track, step by step, as the kernel's lanes run it.  Everything is held BIT-IDENTICAL to the goldens and to the port.
#include "../../filterpy_amd/csrc/fk_poly.hpp"

using namespace fk;

template <int ORDER, int FORM>
static void run(long N, long T, const PolyConst &k, const double *g3, const double *gains, const double *z, double *x, double *xs,
                double *pred, double *y)
{
    constexpr int C = ORDER + 1;
    for (long i = 0; i < N; ++i) {
        double s[C];
        for (int e = 0; e < C; ++e) s[e] = x[e * N + i];
        double g[3] = {g3[0], g3[1], g3[2]};
        for (long t = 0; t < T; ++t) {
            if (gains)
                for (int e = 0; e < C; ++e) g[e] = gains[t * C + e];
            double p, r;
            poly_step<ORDER, FORM>(s, z[t * N + i], k, g, p, r);
            for (int e = 0; e < C; ++e) xs[(t * C + e) * N + i] = s[e];
            pred[t * N + i] = p;
            y[t * N + i] = r;
        }
        for (int e = 0; e < C; ++e) x[e * N + i] = s[e];
    }
}

// x [c][N] in/out, z / pred / y [T][N], xs [T][c][N], g3 [3], gains [T][c] or NULL; returns 0, or -2 for an (order, form) that
// does not exist
extern "C" int hc_poly_run(int order, int form, long N, long T, double dt, double T2, double c, const double *g3,
                           const double *gains, const double *z, double *x, double *xs, double *pred, double *y)
{
    if (!poly_supported(order, form)) return -2;
    const PolyConst k{dt, T2, c};
    switch (form * 3 + order) {
    case POLY_FORM_A * 3 + 0: run<0, POLY_FORM_A>(N, T, k, g3, gains, z, x, xs, pred, y); break;
    case POLY_FORM_A * 3 + 1: run<1, POLY_FORM_A>(N, T, k, g3, gains, z, x, xs, pred, y); break;
    case POLY_FORM_A * 3 + 2: run<2, POLY_FORM_A>(N, T, k, g3, gains, z, x, xs, pred, y); break;
    case POLY_FORM_B * 3 + 1: run<1, POLY_FORM_B>(N, T, k, g3, gains, z, x, xs, pred, y); break;
    case POLY_FORM_B * 3 + 2: run<2, POLY_FORM_B>(N, T, k, g3, gains, z, x, xs, pred, y); break;
    case POLY_FORM_C * 3 + 1: run<1, POLY_FORM_C>(N, T, k, g3, gains, z, x, xs, pred, y); break;
    case POLY_FORM_C * 3 + 2: run<2, POLY_FORM_C>(N, T, k, g3, gains, z, x, xs, pred, y); break;
    }
    return 0;
}
