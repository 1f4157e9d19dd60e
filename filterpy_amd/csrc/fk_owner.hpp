// fk_owner.hpp -- "the value that row k's owner holds, in every lane of the group": the one ladder of the several-lanes-per-track
// kernels, as plain C++ over any exchange object (no HIP builtins: the kernels pass a LaneGroup of fk_ml.hpp, tests/hostcheck its
// fibers and a recording object).  An exchange object X has
//     template <int O> double bcast(double v)     the value lane O of the group passed to the same call, in every lane
//     static constexpr int LANES                  lanes per track (FK_OWNER_ROW only)
// A lane holds R consecutive rows (lane L: rows L R .. L R + R - 1), so the owner of row k is lane k / R -- also where the last
// lane's tail slots are clamped duplicates of row n-1: the ladder is over the owning lane, never over the row.  Cyclic rows
// (fk_ukf_quad.hpp: row j lives in lane j % LN) are the same ladder with R = 1 over the lane number.
// k is a constant wherever a kernel uses this, once its loops are unrolled: exactly one rung -- one broadcast -- survives.
// The ladder is written out flat on purpose: as a recursion over the rung (one function per rung, each optimised on its own before
// it is inlined) the several-lane UKF kernels came out with other schedules and register counts.
#pragma once
#include <type_traits>

#include "fk_math.hpp"

namespace fk {

template <int R, int LPT, class X>
FK_HD double owner_value(X &x, int k, double v)
{
    static_assert(R >= 1 && (LPT == 3 || LPT == 4 || LPT == 8), "R rows per lane, LPT lanes per track");
    const int o = k / R;
    if (o == 0) return x.template bcast<0>(v);
    if (o == 1) return x.template bcast<1>(v);
    if constexpr (LPT == 3) return x.template bcast<2>(v);
    else {
        if (o == 2) return x.template bcast<2>(v);
        if constexpr (LPT == 4) return x.template bcast<3>(v);
        else {
            if (o == 3) return x.template bcast<3>(v);
            if (o == 4) return x.template bcast<4>(v);
            if (o == 5) return x.template bcast<5>(v);
            if (o == 6) return x.template bcast<6>(v);
            return x.template bcast<7>(v);
        }
    }
}

}  // namespace fk

// Row k of a rows-per-lane matrix M[R][LEN], delivered into dst[LEN] in every lane of the group by its owner:
//     FK_OWNER_ROW(R, x, dst, M, k)
// A macro, not a third template: dst and M are register arrays of a kernel, and handed to a function by reference they escape
// until that call is inlined -- the optimiser's first scalar-replacement pass skips them, and the kernels come out with other
// operand orders and schedules (3 of the 8 kernels of kf_mlg.hip at (10, 2) did; with the loop in the caller none does).  The named
// temporary is part of that: the order of a kernel's locals decides ties in its schedule.
#define FK_OWNER_ROW(R, x, dst, M, k)                                                                        \
    FK_UNROLL for (int j_ = 0; j_ < (int)(sizeof(dst) / sizeof((dst)[0])); ++j_) {                           \
        const double v_ = (M)[(k) % (R)][j_];                                                                \
        (dst)[j_] = fk::owner_value<(R), std::remove_reference_t<decltype(x)>::LANES>((x), (k), v_);         \
    }
