"""Fixed-lag Kalman smoother with filterpy's call surface, computed by the gfx950 kernels.

Mirrors rlabbe/filterpy v1.4.5 filterpy/kalman/fixed_lag_smoother.py:

    FixedLagSmoother.__init__ (:72-131)  smooth (:133-215)  smooth_batch (:217-311)  __repr__ (:313-330)

`FixedLagSmoother` is ONE smoother, like the reference (the GPU runs a bank of one); `FixedLagSmootherBank` is the same
arithmetic for n_tracks independent tracks that share F, Q, H, R and B (x (N, n), P (N, n, n), zs (T, N, m)).  Every step is
one launch of fk_fls_batch_f64 (include/filterhip.h): smooth_batch is ONE launch for the whole run, smooth() a launch of one
step that carries the still-pending rows of the lag window in and out.

The reference's semantics are kept, quirks included: xSmooth[k] starts as the PRIOR x_pre; for k >= N the rows k-N+1 .. k gain
PS_i H' S^-1 y; for k < N xSmooth[k] is the filtered x.  So N <= 0 returns the priors and N >= len(zs) the filtered states, and
row j is final only after step j+N-1.  The lag loop is reassociated (P ((F - KH)')^i H' S^-1 y instead of the reference's
PS_i = PS_{i-1} (F - KH)' matrices; csrc/fk_fls.hpp): agreement ~1e-13.  S^-1 is applied through an L D L' factorisation, so
S must be positive definite; a failed factorisation raises numpy.linalg.LinAlgError like KalmanFilter.

Shapes the reference broadcasts into nonsense raise ValueError instead:
  * x that is neither (dim_x,) nor (dim_x, 1);
  * a measurement whose shape does not match x: with a column x, z must be (dim_z, 1) (or a scalar / (1,) when dim_z == 1) --
    a (dim_z,) z with dim_z > 1 makes the reference's y a (dim_z, dim_z) matrix; with a 1-D x, z must be (dim_z,) (or a
    scalar when dim_z == 1) -- a column z makes x a matrix;
  * a control input whose size is not B's column count; with the default scalar B = b, u must have dim_x entries (b u is then
    (b I) u); b == 0 means no control input;
  * a control input whose orientation does not match x: with a column x, u must be (dim_u, 1) (or (dim_u,) when dim_x == 1),
    with a 1-D x it must be (dim_u,) -- otherwise the reference's x_pre += dot(B, u) makes x_pre an (n, n) matrix or fails.
"""
import numpy as np

from .. import _engine as E
from .._abi import FK_KF_FLAG_R_JOSEPH_DIAG
from ._bank import _bank_controls, _check_u_orientation, _control, _desc, _device_zs, _host_zs, _xshape, _z
from .kalman_filter import _mat

__all__ = ["FixedLagSmoother", "FixedLagSmootherBank"]

_I32_MAX = 2 ** 31 - 1


def _lag(N):
    """the reference compares `k >= N` and loops `range(N)`: any integer; beyond int32 it behaves like int32's maximum"""
    if N is None:
        raise TypeError("the lag N must be an integer")
    return int(max(-_I32_MAX, min(int(N), _I32_MAX)))


def _model(F, Q, H, R, n, m):
    """attributes -> (F, Q, H, R, desc flags) with KalmanFilter's scalar rules: a scalar Q / R attribute is used raw by
    numpy (`FPF' + q` adds q to every element; `HPH' + r` likewise, `dot(K, r)` is r K: r K K' -- FK_KF_FLAG_R_JOSEPH_DIAG)"""
    Fm, Hm = _mat(F, n, n, "F"), _mat(H, m, n, "H")
    Qm = _mat(Q, n, n, "Q", scalar="full")
    if (np.isscalar(R) or np.ndim(R) == 0) and m > 1:
        Rm, flags = np.full((m, m), float(R)), FK_KF_FLAG_R_JOSEPH_DIAG
    else:
        Rm, flags = _mat(R, m, m, "R", scalar="full"), 0
    return Fm, Qm, Hm, Rm, flags


def _run(n, m, N, layout, lag, k0, x, P, z, F, Q, H, R, rflags, B=None, u=None, pend=None, want_yS=False):
    """One fk_fls_batch_f64 launch.  x (N, n), P (N, n, n) host arrays or device records; z (T, N, m) host or device records;
    u (T, N, nu) or None; pend: device records of the W = min(max(lag, 1) - 1, k0) pending rows (W, N, n), or None when W = 0.
    Returns device tensors (xs [W + T] rows, xhat [T], x, P, y, S) in `layout`."""
    import torch
    dev = E.require_gpu()
    rec = lambda a, lead: a if isinstance(a, torch.Tensor) else E.to_records(a, layout, lead)   # noqa: E731
    dx, dP, dz = rec(x, 0).clone(), rec(P, 0).clone(), rec(z, 1)
    T = int(dz.shape[0])
    W = min(max(lag, 1) - 1, k0)
    xs = E.alloc_records((W + T,), N, n, layout, dev)
    if W > 0:
        xs[:W].copy_(pend)
    xhat = E.alloc_records((T,), N, n, layout, dev)
    y = E.alloc_records((), N, m, layout, dev) if want_yS else None
    S = E.alloc_records((), N, m * m, layout, dev) if want_yS else None
    st = torch.zeros(N, dtype=torch.int32, device=dev)
    nu = 0 if B is None else int(B.shape[1])
    dB = E.dev(B) if nu else None
    du = rec(u, 1) if nu else None
    E.fls_batch(_desc(n, m, nu, N, T, layout, flags=rflags), lag, k0, E.dev(F), E.dev(Q), E.dev(H), E.dev(R), dz, dx, dP, xs, xhat,
                B=dB, u=du, y=y, S=S, status=st)
    E.raise_on_status(st, "fixed-lag smoother")
    return xs, xhat, dx, dP, y, S


class FixedLagSmoother(object):
    """filterpy.kalman.FixedLagSmoother (fixed_lag_smoother.py:26-330) on the GPU: same attributes, defaults and results."""

    def __init__(self, dim_x, dim_z, N=None):
        self.dim_x = dim_x
        self.dim_z = dim_z
        self.N = N
        self.x = np.zeros((dim_x, 1))
        self.x_s = np.zeros((dim_x, 1))
        self.P = np.eye(dim_x)
        self.Q = np.eye(dim_x)
        self.F = np.eye(dim_x)
        self.H = np.eye(dim_z, dim_x)
        self.R = np.eye(dim_z)
        self.K = np.zeros((dim_x, 1))
        self.y = np.zeros((dim_z, 1))
        self.B = 0.
        self.S = np.zeros((dim_z, dim_z))
        self._I = np.eye(dim_x)
        self.count = 0
        if N is not None:
            self.xSmooth = []

    # -- shapes -------------------------------------------------------------------------------------------------------------
    def _zs(self, zs, xshape):
        m = self.dim_z
        return np.stack([_z(z, m, xshape).reshape(m) for z in zs]) if len(zs) else np.zeros((0, self.dim_z))

    def _us(self, us, T, xshape=None):
        """us (T steps) -> (B (n, nu), u (T, nu)) or (None, None); each u in x's orientation (xshape)"""
        if us is None:
            return None, None
        ua = [np.asarray(u, dtype=np.float64) for u in us]
        if len(ua) < T:
            raise ValueError(f"us has {len(ua)} entries, zs {T}")
        ua = ua[:T]
        shapes = {u.shape for u in ua}
        if len(shapes) > 1:
            raise ValueError("every control input must have the same shape")
        B, nu = _control(self.B, self.dim_x, ua[0].shape if ua else (self.dim_x,))
        if ua and xshape is not None:
            _check_u_orientation(ua[0].shape, nu, self.dim_x, xshape)
        if B is None:
            return None, None
        return B, np.stack([u.reshape(nu) for u in ua])

    def _state(self):
        n = self.dim_x
        return (np.asarray(self.x, dtype=np.float64).reshape(1, n), _mat(self.P, n, n, "P")[None])

    # -- the reference's methods --------------------------------------------------------------------------------------------
    def smooth_batch(self, zs, N, us=None):
        """fixed_lag_smoother.py:217-311: (xSmooth, xhat) of shape (T, dim_x) for a 1-D x, (T, dim_x, 1) for a column x.
        One launch; the object's x and P are left alone."""
        n, m = self.dim_x, self.dim_z
        xshape = _xshape(self.x, n)
        zs = list(zs) if not isinstance(zs, np.ndarray) else zs
        T = len(zs)
        out_shape = (T,) + xshape
        if T == 0:
            return np.zeros(out_shape), np.zeros(out_shape)
        z = self._zs(zs, xshape)
        B, u = self._us(us, T, xshape)
        F, Q, H, R, rflags = _model(self.F, self.Q, self.H, self.R, n, m)
        x, P = self._state()
        xs, xhat, *_ = _run(n, m, 1, "aos", _lag(N), 0, x, P, z.reshape(T, 1, m), F, Q, H, R, rflags,
                            B=B, u=None if u is None else u.reshape(T, 1, -1))
        return (xs.cpu().numpy().reshape(out_shape), xhat.cpu().numpy().reshape(out_shape))

    def smooth(self, z, u=None):
        """fixed_lag_smoother.py:133-215: one step.  Appends this step's row to xSmooth and refreshes the rows of the lag
        window it changed; sets x, P, y, S, count (K and x_s stay as they are)."""
        xSmooth = self.xSmooth                       # AttributeError without N, like the reference
        n, m = self.dim_x, self.dim_z
        lag, k = _lag(self.N), self.count
        xshape = _xshape(self.x, n)
        zr = _z(z, m, xshape)
        B, uu = (None, None) if u is None else self._us([u], 1, xshape)
        F, Q, H, R, rflags = _model(self.F, self.Q, self.H, self.R, n, m)
        x, P = self._state()
        W = min(max(lag, 1) - 1, k)
        pend = None
        if W > 0:
            if len(xSmooth) < k:
                raise ValueError(f"xSmooth has {len(xSmooth)} rows, count is {k}")
            rows = np.stack([np.asarray(r, dtype=np.float64).reshape(n) for r in xSmooth[k - W:k]])
            pend = E.to_records(rows.reshape(W, 1, n), "aos", 1)
        xs, _, dx, dP, y, S = _run(n, m, 1, "aos", lag, k, x, P, zr.reshape(1, 1, m), F, Q, H, R, rflags,
                                   B=B, u=None if uu is None else uu.reshape(1, 1, -1), pend=pend, want_yS=True)
        rows = xs.cpu().numpy().reshape(W + 1, n)
        for i in range(W):
            xSmooth[k - W + i] = rows[i].reshape(xshape).copy()
        xSmooth.append(rows[W].reshape(xshape).copy())
        self.x = dx.cpu().numpy().reshape(xshape)
        self.P = dP.cpu().numpy().reshape(n, n)
        self.y = y.cpu().numpy().reshape((m,) if len(xshape) == 1 else (m, 1))
        self.S = S.cpu().numpy().reshape(m, m)
        self.count += 1

    def __repr__(self):
        return "\n".join(["FixedLagSmoother object (filterpy_amd, gfx950)"] +
                         [f"{k} = {getattr(self, k)!r}" for k in
                          ("dim_x", "dim_z", "N", "x", "x_s", "P", "F", "Q", "R", "H", "K", "y", "S", "B")])


class FixedLagSmootherBank(object):
    """n_tracks independent fixed-lag smoothers that share F, Q, H, R and B, stepped in lock-step on the GPU:

        x (N, dim_x)   P (N, dim_x, dim_x)   zs (T, N, dim_z)   us (T, N, dim_u)   B (dim_x, dim_u)

    smooth_batch returns (xSmooth, xhat) of shape (T, N, dim_x) -- NumPy arrays, or with device_outputs=True the device
    tensors in `layout` ('aos' [T][N][n], 'soa' [T][n][N]).  smooth(z) keeps x, P and the pending rows of the lag window on the
    device between calls; a row of xSmooth crosses PCIe once, when it is final, and the pending window when xSmooth is read."""

    def __init__(self, dim_x, dim_z, n_tracks, N=None, dim_u=0, layout="soa"):
        if dim_x < 1 or dim_z < 1 or dim_u < 0 or n_tracks < 1:
            raise ValueError("dim_x, dim_z, n_tracks must be >= 1 and dim_u >= 0")
        if layout not in E.LAYOUTS:
            raise ValueError("layout must be 'soa' or 'aos'")
        self.dim_x, self.dim_z, self.dim_u, self.n_tracks, self.layout = dim_x, dim_z, dim_u, n_tracks, layout
        self.N = N
        self._x = np.zeros((n_tracks, dim_x))
        self._P = np.tile(np.eye(dim_x), (n_tracks, 1, 1))
        self.F, self.Q = np.eye(dim_x), np.eye(dim_x)
        self.H, self.R = np.eye(dim_z, dim_x), np.eye(dim_z)
        self.B = None
        self.count = 0
        self._dev = None            # (x, P) device records while smooth() owns the state
        self._final = []            # rows of xSmooth that are final, (N, n) each
        self._pend = None           # device records of the pending rows (W, N, n)

    # x and P live on the device between smooth() calls: read = download, write = the host copy wins again
    @property
    def x(self):
        if self._dev is not None:
            self._x = E.host_records(self._dev[0].cpu().numpy(), self.layout, 0, (self.dim_x,))
        return self._x

    @x.setter
    def x(self, v):
        self._sync_P()
        self._x = np.asarray(v, dtype=np.float64)
        self._dev = None

    @property
    def P(self):
        if self._dev is not None:
            self._P = E.host_records(self._dev[1].cpu().numpy(), self.layout, 0, (self.dim_x, self.dim_x))
        return self._P

    @P.setter
    def P(self, v):
        self._sync_x()
        self._P = np.asarray(v, dtype=np.float64)
        self._dev = None

    def _sync_x(self):
        if self._dev is not None:
            self._x = self.x

    def _sync_P(self):
        if self._dev is not None:
            self._P = self.P

    @property
    def xSmooth(self):
        """(count, N, dim_x): the final rows and the pending window (downloaded now)"""
        n, N = self.dim_x, self.n_tracks
        rows = list(self._final)
        if self._pend is not None and self._pend.shape[0] > 0:
            p = E.host_records(self._pend.cpu().numpy(), self.layout, 1, (n,))
            rows += [p[i] for i in range(p.shape[0])]
        return np.stack(rows) if rows else np.zeros((0, N, n))

    def _state(self):
        if self._dev is not None:
            return self._dev
        n, N = self.dim_x, self.n_tracks
        x = np.asarray(self._x, dtype=np.float64)
        if x.size != N * n:
            raise ValueError(f"x has shape {x.shape}, expected ({N}, {n})")
        P = np.asarray(self._P, dtype=np.float64)
        if P.shape != (N, n, n):
            try:
                P = np.broadcast_to(P, (N, n, n))
            except ValueError:
                raise ValueError(f"P has shape {P.shape}, expected ({N}, {n}, {n})") from None
        return x.reshape(N, n), np.ascontiguousarray(P)

    def _inputs(self, zs, us, T):
        """zs and us as _run takes them: device records or (T, N, m) host measurements (no missing rows here), B and u on
        the host"""
        import torch
        n, m, N = self.dim_x, self.dim_z, self.n_tracks
        z = _device_zs(zs, T, N, m, self.layout) if isinstance(zs, torch.Tensor) else _host_zs(zs, T, N, m)
        return (z,) + _bank_controls(self.B, us, T, N, n)

    def smooth_batch(self, zs, N, us=None, device_outputs=False):
        """(xSmooth, xhat), each (T, n_tracks, dim_x), for the whole run in one launch.  x and P are left alone."""
        n, m = self.dim_x, self.dim_z
        T = int(zs.shape[0]) if hasattr(zs, "shape") else len(zs)
        z, B, u = self._inputs(zs, us, T)
        F, Q, H, R, rflags = _model(self.F, self.Q, self.H, self.R, n, m)
        x, P = self._state()
        if T == 0:
            e = np.zeros((0, self.n_tracks, n))
            return e, e.copy()
        xs, xhat, *_ = _run(n, m, self.n_tracks, self.layout, _lag(N), 0, x, P, z, F, Q, H, R, rflags, B=B, u=u)
        if device_outputs:
            return xs, xhat
        return (E.host_records(xs.cpu().numpy(), self.layout, 1, (n,)),
                E.host_records(xhat.cpu().numpy(), self.layout, 1, (n,)))

    def smooth(self, z, u=None):
        """one step for every track: z (n_tracks, dim_z), u (n_tracks, dim_u) or None"""
        if self.N is None:
            raise AttributeError("FixedLagSmootherBank built without N has no xSmooth: smooth() needs the lag")
        n, m, Nt = self.dim_x, self.dim_z, self.n_tracks
        lag, k = _lag(self.N), self.count
        zz, B, uu = self._inputs(np.asarray(z, dtype=np.float64).reshape(1, Nt, m), None if u is None else
                                 np.asarray(u, dtype=np.float64).reshape(1, Nt, -1), 1)
        F, Q, H, R, rflags = _model(self.F, self.Q, self.H, self.R, n, m)
        x, P = self._state()
        W = min(max(lag, 1) - 1, k)
        xs, _, dx, dP, _, _ = _run(n, m, Nt, self.layout, lag, k, x, P, zz, F, Q, H, R, rflags, B=B, u=uu, pend=self._pend)
        Wn = min(max(lag, 1) - 1, k + 1)
        done = W + 1 - Wn                              # rows that became final: 0 or 1
        if done:
            self._final += list(E.host_records(xs[:done].cpu().numpy(), self.layout, 1, (n,)))
        self._pend = xs[done:].clone() if Wn > 0 else None
        self._dev = (dx, dP)
        self.count += 1

    def __repr__(self):
        return "\n".join(["FixedLagSmootherBank object (filterpy_amd, gfx950)"] +
                         [f"{k} = {getattr(self, k)!r}" for k in
                          ("dim_x", "dim_z", "dim_u", "n_tracks", "layout", "N", "count", "F", "Q", "R", "H", "B")])
