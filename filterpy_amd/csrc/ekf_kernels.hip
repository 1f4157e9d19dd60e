// ekf_kernels.hip -- the extended Kalman filter (filterpy/kalman/EKF.py:319-332, 351, 367) for a bank of tracks (gfx950).
// One track per lane, one time step per launch: the Jacobian H = HJacobian(x) and the innovation y = residual(z, Hx(x)) of a
// step come from callables outside, so a launch cannot span two steps.  What it can span is the update of step k and the
// predict of step k + 1 (EKF_STEP): x and P cross HBM once per step instead of twice, the posterior leaves for the optional
// x_post / P_post records on the way.  EKF_PREDICT and EKF_UPDATE are the halves alone; all three are ONE call of ekf_step
// (fk_ekf.hpp) with a half switched off at run time, so a step is bit-identical to an update followed by a predict.
//
// H [m*n] and y [m] are always records of the track.  F, Q, R, B are shared (staged in LDS by bank_fill_model, B read through
// bank_control) or records of the track (FK_MODEL_PER_TRACK: read row by row where the arithmetic wants them, never held whole).
//   ekf_fast_kernel<NX, NZ>    exact (dim_x, dim_z): x, P, H in VGPRs, every loop unrolled.  Element-major records: lane loads
//       and stores.  NumPy order: x, P, H, y and the posterior pass through wave-private LDS transposes (wave_load_aos /
//       wave_store_aos: 1 KiB contiguous per instruction); the small by-products and a per-track model use lane accesses.
//       Compiled once per -DFK_NX/-DFK_NZ (fk_dims_ekf.def).
//   ekf_general_kernel         everything else (dim_x <= 16, dim_z <= 8): ONE padded (16, 8) instantiation with rolled loops
//       (arrays in scratch), lane accesses.  A correctness path.  Compiled with -DFK_EKF_GENERAL=1.
// Which one runs depends on (n, m) only (ekf_dispatch.cpp).
#if defined(FK_EKF_GENERAL) && FK_EKF_GENERAL
#define FK_ROLLED 1
#endif
#include "fk_bank.hpp"
#include "fk_ekf.hpp"

namespace fk {

// F, Q, R as records of the lane's track, padded like LdsModel
template <int NX, int NZ, int LAYOUT, bool EXACT>
struct EkfTrackModel {
    RecView<LAYOUT> f, q, r;
    int n, m;
    __device__ __forceinline__ EkfTrackModel(const EkfArgs &a, const Lane &ln, int n_, int m_)
        : f(a.F, ln, n_ * n_), q(a.Q, ln, n_ * n_), r(a.R, ln, m_ * m_), n(n_), m(m_)
    {
    }
    template <int LEN>
    __device__ __forceinline__ void row(const RecView<LAYOUT> &v, int i, int d, double pad, double (&o)[LEN]) const
    {
        FK_UNROLL for (int j = 0; j < LEN; ++j)
            o[j] = (EXACT || (i < d && j < d)) ? v.load(EXACT ? i * LEN + j : i * d + j) : (i == j ? pad : 0.0);
    }
    __device__ __forceinline__ void rowF(int i, double (&o)[NX]) const { row<NX>(f, i, n, 1.0, o); }
    __device__ __forceinline__ void rowQ(int i, double (&o)[NX]) const { row<NX>(q, i, n, 0.0, o); }
    __device__ __forceinline__ void rowR(int i, double (&o)[NZ]) const { row<NZ>(r, i, m, 1.0, o); }
};

// B u with the track's own B record [n][nu] (the shared B goes through bank_control)
template <int NX, int LAYOUT>
__device__ __forceinline__ void ekf_control_track(const EkfArgs &a, const Lane &ln, double (&bu)[NX])
{
    FK_UNROLL for (int r = 0; r < NX; ++r) bu[r] = 0.0;
    if (a.nu <= 0) return;
    const RecView<LAYOUT> uv(a.u, ln, a.nu), bv(a.B, ln, a.n * a.nu);
    for (int j = 0; j < a.nu; ++j) {
        const double uj = uv.load(j);
        FK_UNROLL for (int r = 0; r < NX; ++r) {
            if (r < a.n) {
                const double b = bv.load(r * a.nu + j);
                bu[r] = (j == 0) ? b * uj : fma(b, uj, bu[r]);
            }
        }
    }
}

// One record of the lane's track in.  WAVE: through the wave's LDS tile (every lane of the wave takes part; rows past the
// block's last track read as zeros).
template <int R, int C, int LAYOUT, bool EXACT, bool WAVE>
__device__ __forceinline__ void ekf_get(double (&v)[R * C], const double *base, const Lane &ln, int r, int c, double pad,
                                        double *tile, unsigned last_row)
{
    if constexpr (WAVE) {
        const unsigned lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
        wave_load_aos<R * C>(v, base + ln.blk0 * (R * C), wave * 64u, tile, lane, last_row);
    } else {
        load_rec<R, C, LAYOUT, EXACT>(v, base, ln, r, c, pad);
    }
}

// The whole launch for one lane: NX, NZ the register shapes (the real n, m when EXACT).  last_row: the block's last real
// track; lanes past it (WAVE only) take part in the transposes and store nothing of their own.
template <int NX, int NZ, int LAYOUT, bool EXACT, bool WAVE, bool PT, class Model>
__device__ __forceinline__ void ekf_lane(const EkfArgs &a, const Model &M, const Lane &ln, bool live, double *tile,
                                         unsigned last_row)
{
    const long track = ln.blk0 + ln.tid;
    const int n = EXACT ? NX : a.n, m = EXACT ? NZ : a.m;
    const bool do_update = a.phase != EKF_PREDICT, do_predict = a.phase != EKF_UPDATE;

    double x[NX], P[NX * NX];
    ekf_get<NX, 1, LAYOUT, EXACT, WAVE>(x, a.x, ln, n, 1, 0.0, tile, last_row);
    ekf_get<NX, NX, LAYOUT, EXACT, WAVE>(P, a.P, ln, n, n, 1.0, tile, last_row);
    double H[NZ * NX], y[NZ], bu[NX], K[NX * NZ], S[NZ * NZ], Lf[NZ * NZ], dinv[NZ];
    bool upd = false;
    if (do_update) {
        ekf_get<NZ, NX, LAYOUT, EXACT, WAVE>(H, a.H, ln, m, n, 0.0, tile, last_row);
        ekf_get<NZ, 1, LAYOUT, EXACT, WAVE>(y, a.y, ln, m, 1, 0.0, tile, last_row);
        upd = a.mask == nullptr || a.mask[track] != 0;
    }
    // between the halves (every lane of the wave arrives here: the posterior's stores are wave-cooperative in NumPy order)
    auto post = [&](const double (&xq)[NX], const double (&Pq)[NX * NX], bool updated) {
        // the by-products of the tracks that update
        if (updated && live) {
            if (a.K) store_rec<NX, NZ, LAYOUT, EXACT>(K, a.K, ln, n, m);
            if (a.S) store_rec<NZ, NZ, LAYOUT, EXACT>(S, a.S, ln, m, m);
            if (a.SI) {
                double SI[NZ * NZ];
                inv_from_ldlt<NZ>(Lf, dinv, SI);
                store_rec<NZ, NZ, LAYOUT, EXACT>(SI, a.SI, ln, m, m);
            }
            if (a.ll || a.maha) {
                double ll, maha;
                ekf_likelihood<NZ>(y, Lf, dinv, m, ll, maha);
                if (a.ll) a.ll[track] = ll;
                if (a.maha) a.maha[track] = maha;
            }
        }
        if (do_predict) {
            if (do_update) {
                if (a.x_post) bank_put<NX, 1, LAYOUT, EXACT, WAVE>(xq, a.x_post, 0, ln, n, 1, tile, last_row);
                if (a.P_post) bank_put<NX, NX, LAYOUT, EXACT, WAVE>(Pq, a.P_post, 0, ln, n, n, tile, last_row);
            }
            if constexpr (PT) ekf_control_track<NX, LAYOUT>(a, ln, bu);
            else bank_control<NX, LAYOUT>(a, ln, a.u, 0, bu);
        }
    };
    const int st = ekf_step<NX, NZ>(x, P, H, y, bu, M, K, S, Lf, dinv, a.rj_diag != 0, upd, do_predict, post);
    bank_put<NX, 1, LAYOUT, EXACT, WAVE>(x, a.x, 0, ln, n, 1, tile, last_row);
    bank_put<NX, NX, LAYOUT, EXACT, WAVE>(P, a.P, 0, ln, n, n, tile, last_row);
    if (a.status && live) a.status[track] = st;
}

template <int NX, int NZ, int LAYOUT, bool EXACT, bool WAVE, bool PT>
__device__ __forceinline__ void ekf_block(const EkfArgs &a, const double *s_model, double *tile, unsigned last_row)
{
    const long blk0 = (long)blockIdx.x * BLOCK;
    const bool live = threadIdx.x <= last_row;
    const Lane ln{blk0, live ? threadIdx.x : last_row, a.N};
    if constexpr (PT) {
        const EkfTrackModel<NX, NZ, LAYOUT, EXACT> M(a, ln, EXACT ? NX : a.n, EXACT ? NZ : a.m);
        ekf_lane<NX, NZ, LAYOUT, EXACT, WAVE, true>(a, M, ln, live, tile, last_row);
    } else {
        const LdsModel<NX, NZ> M{s_model};
        ekf_lane<NX, NZ, LAYOUT, EXACT, WAVE, false>(a, M, ln, live, tile, last_row);
    }
}

template <class Args>
int ekf_launch(void (*soa)(Args), void (*aos)(Args), void (*soa_pt)(Args), void (*aos_pt)(Args), const char *name,
               const Args &a, int layout, hipStream_t stream)
{
    return a.per_track ? bank_launch(soa_pt, aos_pt, name, a, layout, stream) : bank_launch(soa, aos, name, a, layout, stream);
}

#if !(defined(FK_EKF_GENERAL) && FK_EKF_GENERAL)

template <int NX, int NZ, int LAYOUT, bool PT>
__global__ void __launch_bounds__(BLOCK)
ekf_fast_kernel(const EkfArgs a)
{
    static_assert(NZ <= NX, "the tile is sized by P's record");
    constexpr bool WAVE = LAYOUT == LAYOUT_AOS;
    constexpr int TILE = 64 * ((NX * NX) | 1);    // the wave's tile: 64 records of the longest one (P), odd row stride
    static_assert(((BLOCK / 64) * TILE + LdsModel<NX, NZ>::SIZE) * 8 <= 160 * 1024, "LDS");
    __shared__ double s_model[PT ? 1 : LdsModel<NX, NZ>::SIZE];
    __shared__ double s_tile[WAVE ? (BLOCK / 64) * TILE : 1];
    if constexpr (!PT) bank_fill_model<NX, NZ>(s_model, a.F, a.Q, nullptr, a.R, a.n, a.m);     // (the only barrier)
    const long left = a.N - (long)blockIdx.x * BLOCK;
    const unsigned last_row = (unsigned)(left < BLOCK ? left : BLOCK) - 1u;
    if (!WAVE && threadIdx.x > last_row) return;
    ekf_block<NX, NZ, LAYOUT, true, WAVE, PT>(a, s_model, s_tile + (WAVE ? (threadIdx.x >> 6) * TILE : 0), last_row);
}

#define FK_CAT_(a, b, c) a##b##_##c
#define FK_CAT(a, b, c) FK_CAT_(a, b, c)

int FK_CAT(launch_ekf_fast_, FK_NX, FK_NZ)(const EkfArgs &a, int layout, hipStream_t stream)
{
    return ekf_launch(ekf_fast_kernel<FK_NX, FK_NZ, LAYOUT_SOA, false>, ekf_fast_kernel<FK_NX, FK_NZ, LAYOUT_AOS, false>,
                      ekf_fast_kernel<FK_NX, FK_NZ, LAYOUT_SOA, true>, ekf_fast_kernel<FK_NX, FK_NZ, LAYOUT_AOS, true>,
                      "ekf_fast_kernel", a, layout, stream);
}

#else  // FK_EKF_GENERAL

constexpr int GX = 16, GZ = 8;

template <int LAYOUT, bool PT>
__global__ void __launch_bounds__(BLOCK)
ekf_general_kernel(const EkfArgs a)
{
    __shared__ double s_model[PT ? 1 : LdsModel<GX, GZ>::SIZE];
    if constexpr (!PT) bank_fill_model<GX, GZ>(s_model, a.F, a.Q, nullptr, a.R, a.n, a.m);
    const long left = a.N - (long)blockIdx.x * BLOCK;
    const unsigned last_row = (unsigned)(left < BLOCK ? left : BLOCK) - 1u;
    if (threadIdx.x > last_row) return;
    ekf_block<GX, GZ, LAYOUT, false, false, PT>(a, s_model, nullptr, last_row);
}

int launch_ekf_general(const EkfArgs &a, int layout, hipStream_t stream)
{
    return ekf_launch(ekf_general_kernel<LAYOUT_SOA, false>, ekf_general_kernel<LAYOUT_AOS, false>,
                      ekf_general_kernel<LAYOUT_SOA, true>, ekf_general_kernel<LAYOUT_AOS, true>, "ekf_general_kernel", a, layout,
                      stream);
}

#endif

}  // namespace fk
