// poly_dispatch.cpp -- fk_poly_run (include/filterhip.h): the fixed-gain polynomial filters of filterpy.gh, filterpy.memory
// and filterpy.leastsq for a bank of tracks.  Everything is validated before any device call; the kernels are in
// poly_kernels.hip, the recurrences in fk_poly.hpp.
#include "fk_dispatch.hpp"
#include "fk_poly.hpp"

static_assert(FK_POLY_FORM_A == fk::POLY_FORM_A && FK_POLY_FORM_B == fk::POLY_FORM_B && FK_POLY_FORM_C == fk::POLY_FORM_C,
              "the header's form numbers are the step functions'");

namespace fk {
int launch_poly(int order, int form, const PolyArgs &a, hipStream_t stream);
}

extern "C" int fk_poly_run(int32_t order, int32_t form, int64_t N, int64_t T, int32_t layout,
                           double dt, double T2, double c, double g0, double g1, double g2,
                           const double *gains, const double *z, double *x,
                           double *xs, double *pred, double *y_out, void *stream)
{
    using namespace fk;
    if (N < 0 || T < 0) return fail(FK_ERR_BAD_ARG, "fk_poly_run: N and T must be >= 0");
    if (layout != FK_LAYOUT_AOS && layout != FK_LAYOUT_SOA) return fail(FK_ERR_BAD_ARG, "fk_poly_run: bad layout");
    if (!poly_supported(order, form))
        return fail(FK_ERR_UNSUPPORTED, "fk_poly_run: form A takes order 0..2, forms B and C order 1 and 2");
    if (N == 0 || T == 0) return FK_OK;
    if (!z || !x) return fail(FK_ERR_BAD_ARG, "fk_poly_run: z and x must not be NULL");

    PolyArgs a;
    a.N = N;
    a.T = T;
    a.es = layout == FK_LAYOUT_SOA ? N : 1;
    a.ts = layout == FK_LAYOUT_SOA ? 1 : order + 1;
    a.k = PolyConst{dt, T2, c};
    a.g[0] = g0; a.g[1] = g1; a.g[2] = g2;
    a.gains = gains;
    a.z = z;
    a.x = x;
    a.xs = xs;
    a.pred = pred;
    a.y = y_out;
    return launch_poly(order, form, a, (hipStream_t)stream);
}
