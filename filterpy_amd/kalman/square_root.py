"""Square-root Kalman filter with filterpy's call surface, computed by the gfx950 kernels.

Mirrors rlabbe/filterpy v1.4.5 filterpy/kalman/square_root.py:

    SquareRootKalmanFilter.__init__ (:124-170)  update (:172-224)  predict (:226-248)  residual_of / measurement_of_state
    (:250-272)  the P, Q, R setters and the P, Q, R, S, SI getters (:274-340)  __repr__ (:342-360)

`SquareRootKalmanFilter` is ONE filter, like the reference: each predict() / update() is one launch on a bank of one
(fk_srkf_predict_f64 / fk_srkf_update_f64, include/filterhip.h).  `SquareRootKalmanFilterBank` is the same arithmetic for
n_tracks filters that share F, H, Q, R and B, with a batch_filter that runs the whole time loop in ONE launch
(fk_srkf_batch_f64).  P is carried as its lower-triangular factor P1_2 and never formed on the device: each step is two
Householder QR factorisations in LAPACK's sign convention (csrc/fk_srkf.hpp), so P1_2 and S1_2 carry the reference's signs.

The reference's semantics are kept, quirks included: the P, Q and R setters store scipy.linalg.cholesky(., lower=True); P_post
returns the PRIOR's product (:300-303); update(None) only records z = [[None] * dim_z]' and the posterior copies; a scalar R2
means eye(dim_z) * R2; M holds the last update's [[R2', 0], [(H P1_2)', P1_2']].  Divergences:
  * pinv(S1_2) is the triangular inverse; when a diagonal entry of S1_2 is at or below dim_z eps max|diag| the call raises
    numpy.linalg.LinAlgError (the reference goes on with a pseudo-inverse);
  * the factors must be lower triangular (what the setters make): an R2 override, or a P1_2 / Q1_2 / R1_2 assigned by hand,
    with a nonzero entry above the diagonal raises ValueError -- the kernels do not read the upper triangles;
  * shapes the reference broadcasts into nonsense raise ValueError: x that is neither (dim_x,) nor (dim_x, 1); a measurement
    whose shape does not match x (as FixedLagSmoother); a control input whose size is not B's column count (dim_x with a
    scalar B) or whose orientation does not match x; a nonzero scalar u with a matrix B.  u = 0 (the default) is no control
    input whatever B is; a scalar u with a scalar B adds b u to every entry of x, as numpy does;
  * dim_x < 1 raises ValueError (the reference checks dim_z twice, :128-131).
"""
from copy import deepcopy

import numpy as np

from .. import _engine as E
from .._abi import FK_MODEL_SHARED
from .fixed_lag_smoother import _control
from .kalman_filter import _mat

__all__ = ["SquareRootKalmanFilter", "SquareRootKalmanFilterBank"]


def _cholesky(A):
    """scipy.linalg.cholesky(A, lower=True), imported on first use (the reference's setters, square_root.py:274-340)"""
    from scipy.linalg import cholesky
    return cholesky(A, lower=True)


def _factor(L, k, name):
    """a (k, k) lower-triangular factor as float64, or ValueError"""
    A = np.asarray(L, dtype=np.float64)
    if A.shape != (k, k):
        raise ValueError(f"{name} has shape {A.shape}, expected ({k}, {k})")
    if np.any(np.triu(A, 1) != 0):
        raise ValueError(f"{name} must be a lower-triangular factor (the kernels do not read its upper triangle)")
    return np.ascontiguousarray(A)


def _step_control(B, u, n, xshape):
    """predict's x = F x + dot(B, u) -> (B (n, nu), u (nu,)) or (None, None)"""
    if u is None:
        return None, None
    if np.ndim(u) == 0:
        if float(u) == 0.0:
            return None, None
        if not (np.isscalar(B) or np.ndim(B) == 0):
            raise ValueError("a nonzero scalar u with a matrix B: dot(B, u) would be an (n, dim_u) matrix")
        b = float(B)
        return (None, None) if b == 0.0 else (np.full((n, 1), b), np.array([float(u)]))
    ua = np.asarray(u, dtype=np.float64)
    Bm, nu = _control(B, n, ua.shape)
    sh = ua.shape
    ok = sh == (nu, 1) or (n == 1 and sh == (nu,)) if len(xshape) == 2 else sh == (nu,)
    if not ok:
        raise ValueError(f"control input of shape {sh} with x of shape {xshape}: expected "
                         + (f"({nu}, 1)" if len(xshape) == 2 else f"({nu},)"))
    if Bm is None:
        return None, None
    return Bm, ua.reshape(nu)


def _desc(n, m, nu, N, T, layout, update_first=False):
    return dict(n=n, m=m, nu=nu, model_mode=FK_MODEL_SHARED, N=N, T=T, layout=E.LAYOUTS[layout],
                update_first=int(bool(update_first)), alpha_sq=1.0, flags=0)


class SquareRootKalmanFilter(object):
    """filterpy.kalman.SquareRootKalmanFilter (square_root.py:27-360) on the GPU: same attributes, defaults and results."""

    def __init__(self, dim_x, dim_z, dim_u=0):
        if dim_x < 1:
            raise ValueError('dim_x must be 1 or greater')
        if dim_z < 1:
            raise ValueError('dim_z must be 1 or greater')
        if dim_u < 0:
            raise ValueError('dim_u must be 0 or greater')
        self.dim_x = dim_x
        self.dim_z = dim_z
        self.dim_u = dim_u
        self.x = np.zeros((dim_x, 1))
        self._P = np.eye(dim_x)
        self._P1_2 = np.eye(dim_x)
        self._Q = np.eye(dim_x)
        self._Q1_2 = np.eye(dim_x)
        self.B = 0.
        self.F = np.eye(dim_x)
        self.H = np.zeros((dim_z, dim_x))
        self._R1_2 = np.eye(dim_z)
        self._R = np.eye(dim_z)
        self.z = np.array([[None] * self.dim_z]).T
        self.K = np.zeros((dim_x, dim_z))
        self.S1_2 = np.zeros((dim_z, dim_z))
        self.SI1_2 = np.zeros((dim_z, dim_z))
        self.y = np.zeros((dim_z, 1))
        self._I = np.eye(dim_x)
        self.M = np.zeros((dim_z + dim_x, dim_z + dim_x))
        self.x_prior = np.copy(self.x)
        self._P1_2_prior = np.copy(self._P1_2)
        self.x_post = np.copy(self.x)
        self._P1_2_post = np.copy(self._P1_2)

    # -- shapes -------------------------------------------------------------------------------------------------------------
    def _xshape(self):
        n = self.dim_x
        x = np.asarray(self.x, dtype=np.float64)
        if x.shape not in ((n,), (n, 1)):
            raise ValueError(f"x has shape {x.shape}, expected ({n},) or ({n}, 1)")
        return x.shape

    def _z(self, z, xshape):
        """one measurement -> (m,) row, refusing the shapes the reference turns into nonsense"""
        m = self.dim_z
        za = np.asarray(z, dtype=np.float64)
        column = len(xshape) == 2
        if za.ndim == 0 and m == 1:
            ok = True
        elif column:
            ok = za.shape == (m, 1) or (m == 1 and za.shape == (1,))
        else:
            ok = za.shape == (m,)
        if not ok:
            raise ValueError(f"measurement of shape {za.shape} with x of shape {xshape}: expected "
                             + (f"({m}, 1)" if column else f"({m},)") + (" or a scalar" if m == 1 else ""))
        return za.reshape(m)

    # -- the reference's methods --------------------------------------------------------------------------------------------
    def update(self, z, R2=None):
        """square_root.py:172-224.  z None: bookkeeping only (:189-193)."""
        if z is None:
            self.z = np.array([[None] * self.dim_z]).T
            self.x_post = self.x.copy()
            self._P1_2_post = np.copy(self._P1_2)
            return
        n, m = self.dim_x, self.dim_z
        xshape = self._xshape()
        zr = self._z(z, xshape)
        if R2 is None:
            R2 = self._R1_2
        elif np.isscalar(R2):
            R2 = np.eye(m) * R2
        R2 = _factor(R2, m, "R2")
        H = _mat(self.H, m, n, "H")
        L = _factor(self._P1_2, n, "P1_2")
        import torch
        E.require_gpu()
        x = E.dev(np.asarray(self.x, dtype=np.float64).reshape(1, n))
        P12 = E.dev(L.reshape(1, n, n))
        y, K = E.alloc_records((), 1, m, "aos"), E.alloc_records((), 1, n * m, "aos")
        S12, SI12 = E.alloc_records((), 1, m * m, "aos"), E.alloc_records((), 1, m * m, "aos")
        st = torch.zeros(1, dtype=torch.int32, device=x.device)
        E.srkf_update(_desc(n, m, 0, 1, 1, "aos"), E.dev(H), E.dev(R2), E.dev(zr.reshape(1, m)), x, P12,
                      y=y, K=K, S12=S12, SI12=SI12, status=st)
        E.raise_on_status(st, "SquareRootKalmanFilter.update (S1_2 is singular: the reference would use a pseudo-inverse)")
        M = self.M
        M[0:m, 0:m] = R2.T
        M[m:, 0:m] = np.dot(H, L).T
        M[m:, m:] = L.T
        self.S1_2 = S12.cpu().numpy().reshape(m, m)
        self.SI1_2 = SI12.cpu().numpy().reshape(m, m)
        self.K = K.cpu().numpy().reshape(n, m)
        self.y = y.cpu().numpy().reshape((m,) if len(xshape) == 1 else (m, 1))
        self.x = x.cpu().numpy().reshape(xshape)
        self._P1_2 = P12.cpu().numpy().reshape(n, n)
        self.z = deepcopy(z)
        self.x_post = self.x.copy()
        self._P1_2_post = np.copy(self._P1_2)

    def predict(self, u=0):
        """square_root.py:226-248"""
        n = self.dim_x
        xshape = self._xshape()
        B, uu = _step_control(self.B, u, n, xshape)
        F = _mat(self.F, n, n, "F")
        Q12 = _factor(self._Q1_2, n, "Q1_2")
        L = _factor(self._P1_2, n, "P1_2")
        import torch
        E.require_gpu()
        x = E.dev(np.asarray(self.x, dtype=np.float64).reshape(1, n))
        P12 = E.dev(L.reshape(1, n, n))
        st = torch.zeros(1, dtype=torch.int32, device=x.device)
        nu = 0 if B is None else B.shape[1]
        E.srkf_predict(_desc(n, self.dim_z, nu, 1, 1, "aos"), E.dev(F), E.dev(Q12), x, P12,
                       B=None if B is None else E.dev(B), u=None if B is None else E.dev(uu.reshape(1, nu)), status=st)
        E.raise_on_status(st, "SquareRootKalmanFilter.predict")
        self.x = x.cpu().numpy().reshape(xshape)
        self._P1_2 = P12.cpu().numpy().reshape(n, n)
        self.x_prior = np.copy(self.x)
        self._P1_2_prior = np.copy(self._P1_2)

    def residual_of(self, z):
        """returns the residual for the given measurement (z); does not alter the state"""
        return z - np.dot(self.H, self.x)

    def measurement_of_state(self, x):
        """the measurement corresponding to the state x"""
        return np.dot(self.H, x)

    @property
    def Q(self):
        """Process uncertainty"""
        return np.dot(self._Q1_2, self._Q1_2.T)

    @Q.setter
    def Q(self, value):
        self._Q = value
        self._Q1_2 = _cholesky(self._Q)

    @property
    def Q1_2(self):
        """Sqrt Process uncertainty"""
        return self._Q1_2

    @property
    def P(self):
        """covariance matrix"""
        return np.dot(self._P1_2, self._P1_2.T)

    @P.setter
    def P(self, value):
        self._P = value
        self._P1_2 = _cholesky(self._P)

    @property
    def P_prior(self):
        """covariance matrix of the prior"""
        return np.dot(self._P1_2_prior, self._P1_2_prior.T)

    @property
    def P_post(self):
        """covariance matrix of the posterior -- the reference returns the PRIOR's product here (square_root.py:300-303)"""
        return np.dot(self._P1_2_prior, self._P1_2_prior.T)

    @property
    def P1_2(self):
        """sqrt of covariance matrix"""
        return self._P1_2

    @property
    def R(self):
        """measurement uncertainty"""
        return np.dot(self._R1_2, self._R1_2.T)

    @R.setter
    def R(self, value):
        self._R = value
        self._R1_2 = _cholesky(self._R)

    @property
    def R1_2(self):
        """sqrt of measurement uncertainty"""
        return self._R1_2

    @property
    def S(self):
        """system uncertainty (P projected to measurement space)"""
        return np.dot(self.S1_2, self.S1_2.T)

    @property
    def SI(self):
        """inverse system uncertainty"""
        return np.dot(self.SI1_2.T, self.SI1_2)

    def __repr__(self):
        return "\n".join(["SquareRootKalmanFilter object (filterpy_amd, gfx950)"] +
                         [f"{k} = {getattr(self, k)!r}" for k in
                          ("dim_x", "dim_z", "dim_u", "x", "P", "F", "Q", "R", "H", "K", "y", "S", "SI", "M", "B")])


class SquareRootKalmanFilterBank(object):
    """n_tracks independent square-root filters that share F, H, Q, R and B, stepped in lock-step on the GPU:

        x (N, dim_x)   P1_2 (N, dim_x, dim_x)   zs (T, N, dim_z)   us (T, N, dim_u)   B (dim_x, dim_u)

    The P, Q and R setters factor (per track for P) with a lower Cholesky factorisation, as the reference's do; P1_2 can be
    set directly (lower triangular).  predict(u) / update(z, R2, mask) are one launch each; a NaN row of z is a missing
    measurement.  batch_filter returns (means, sqrt_covs, means_p, sqrt_covs_p) -- (T, N, n) and (T, N, n, n) NumPy arrays, or
    with device_outputs=True the device tensors in `layout` ('aos' [T][N][..], 'soa' [T][..][N]) -- from ONE launch; x and P1_2
    are left alone."""

    def __init__(self, dim_x, dim_z, n_tracks, dim_u=0, layout="soa"):
        if dim_x < 1 or dim_z < 1 or dim_u < 0 or n_tracks < 1:
            raise ValueError("dim_x, dim_z, n_tracks must be >= 1 and dim_u >= 0")
        if layout not in E.LAYOUTS:
            raise ValueError("layout must be 'soa' or 'aos'")
        self.dim_x, self.dim_z, self.dim_u, self.n_tracks, self.layout = dim_x, dim_z, dim_u, n_tracks, layout
        self.x = np.zeros((n_tracks, dim_x))
        self._P1_2 = np.tile(np.eye(dim_x), (n_tracks, 1, 1))
        self._Q1_2 = np.eye(dim_x)
        self._R1_2 = np.eye(dim_z)
        self.F = np.eye(dim_x)
        self.H = np.zeros((dim_z, dim_x))
        self.B = None
        # the last update's by-products per track (update() sets them for the tracks that update)
        self.y = np.zeros((n_tracks, dim_z))
        self.K = np.zeros((n_tracks, dim_x, dim_z))
        self.S1_2 = np.zeros((n_tracks, dim_z, dim_z))
        self.SI1_2 = np.zeros((n_tracks, dim_z, dim_z))

    @property
    def P(self):
        return np.matmul(self._P1_2, np.swapaxes(self._P1_2, -1, -2))

    @P.setter
    def P(self, value):
        n, N = self.dim_x, self.n_tracks
        P = np.asarray(value, dtype=np.float64)
        try:
            P = np.broadcast_to(P, (N, n, n))
        except ValueError:
            raise ValueError(f"P has shape {P.shape}, expected ({N}, {n}, {n}) or ({n}, {n})") from None
        self._P1_2 = np.ascontiguousarray(np.linalg.cholesky(P))

    @property
    def P1_2(self):
        return self._P1_2

    @P1_2.setter
    def P1_2(self, value):
        n, N = self.dim_x, self.n_tracks
        L = np.ascontiguousarray(np.broadcast_to(np.asarray(value, dtype=np.float64), (N, n, n)))
        if np.any(np.triu(L, 1) != 0):
            raise ValueError("P1_2 must be lower triangular")
        self._P1_2 = L

    @property
    def Q(self):
        return self._Q1_2 @ self._Q1_2.T

    @Q.setter
    def Q(self, value):
        self._Q1_2 = _cholesky(_mat(value, self.dim_x, self.dim_x, "Q"))

    @property
    def Q1_2(self):
        return self._Q1_2

    @property
    def R(self):
        return self._R1_2 @ self._R1_2.T

    @R.setter
    def R(self, value):
        self._R1_2 = _cholesky(_mat(value, self.dim_z, self.dim_z, "R"))

    @property
    def R1_2(self):
        return self._R1_2

    # -- plumbing -----------------------------------------------------------------------------------------------------------
    def _model(self):
        n, m = self.dim_x, self.dim_z
        return (E.dev(_mat(self.F, n, n, "F")), E.dev(_factor(self._Q1_2, n, "Q1_2")), E.dev(_mat(self.H, m, n, "H")),
                E.dev(_factor(self._R1_2, m, "R1_2")))

    def _state(self):
        n, N = self.dim_x, self.n_tracks
        x = np.asarray(self.x, dtype=np.float64)
        if x.size != N * n:
            raise ValueError(f"x has shape {x.shape}, expected ({N}, {n})")
        L = np.asarray(self._P1_2, dtype=np.float64)
        if L.shape != (N, n, n):
            raise ValueError(f"P1_2 has shape {L.shape}, expected ({N}, {n}, {n})")
        if np.any(np.triu(L, 1) != 0):
            raise ValueError("P1_2 must be lower triangular")
        return (E.to_records(x.reshape(N, n), self.layout, 0).clone(),
                E.to_records(L.reshape(N, n * n), self.layout, 0).clone())

    def _controls(self, us, T):
        n, N = self.dim_x, self.n_tracks
        if us is None:
            return None, None
        ua = np.asarray(us, dtype=np.float64)
        if ua.ndim == 2:
            ua = ua[:, :, None]
        if ua.ndim != 3 or ua.shape[:2] != (T, N):
            raise ValueError(f"us has shape {ua.shape}, expected ({T}, {N}, dim_u)")
        if self.B is None:
            raise ValueError("us given but B is None")
        B, nu = _control(self.B, n, ua.shape[2:], "us")
        if B is None:
            return None, None
        return E.dev(B), E.to_records(np.ascontiguousarray(ua), self.layout, 1)

    def _measurements(self, zs, T, mask):
        """zs (T, N, m) host (NaN rows missing) or device records -> (device z, device uint8 mask or None)"""
        import torch
        n, m, N = self.dim_x, self.dim_z, self.n_tracks
        if isinstance(zs, torch.Tensor):
            want = (T, N, m) if self.layout == "aos" else (T, m, N)
            if tuple(zs.shape) != want:
                raise ValueError(f"device zs has shape {tuple(zs.shape)}, expected {want} ({self.layout} records)")
            z = zs.to(dtype=torch.float64).contiguous()
            keep = None
        else:
            za = np.asarray(zs, dtype=np.float64)
            if za.shape != (T, N, m) and not (m == 1 and za.shape == (T, N)):
                raise ValueError(f"zs has shape {za.shape}, expected ({T}, {N}, {m})")
            za = za.reshape(T, N, m)
            nan = np.isnan(za).any(axis=2)
            keep = None if not nan.any() else ~nan
            if keep is not None:
                za = np.where(nan[:, :, None], 0.0, za)
            z = E.to_records(za, self.layout, 1)
        if mask is not None:
            mk = np.asarray(mask, dtype=bool).reshape(T, N)
            keep = mk if keep is None else (keep & mk)
        dm = None if keep is None else torch.from_numpy(np.ascontiguousarray(keep, dtype=np.uint8)).to(E.require_gpu())
        return z, dm

    def _host(self, t, lead, rec_shape):
        return E.host_records(t.cpu().numpy(), self.layout, lead, rec_shape)

    # -- steps --------------------------------------------------------------------------------------------------------------
    def predict(self, u=None):
        """one predict for every track: u (n_tracks, dim_u) or None"""
        import torch
        n, N = self.dim_x, self.n_tracks
        F, Q12, _, _ = self._model()
        B, du = self._controls(None if u is None else np.asarray(u, dtype=np.float64).reshape(1, N, -1), 1)
        x, P12 = self._state()
        st = torch.zeros(N, dtype=torch.int32, device=x.device)
        nu = 0 if B is None else int(B.shape[1])
        E.srkf_predict(_desc(n, self.dim_z, nu, N, 1, self.layout), F, Q12, x, P12, B=B,
                       u=None if du is None else du.reshape(du.shape[1:]), status=st)
        E.raise_on_status(st, "SquareRootKalmanFilterBank.predict")
        self.x = self._host(x, 0, (n,))
        self._P1_2 = self._host(P12, 0, (n, n))

    def update(self, z, R2=None, mask=None):
        """one update for every track: z (n_tracks, dim_z), NaN rows missing; R2 a lower-triangular factor or a scalar
        (eye * R2) for this call; mask (n_tracks,) bool, False = missing.  Sets y, K, S1_2, SI1_2 of the tracks that update."""
        import torch
        n, m, N = self.dim_x, self.dim_z, self.n_tracks
        _, _, H, R12 = self._model()
        if R2 is not None:
            R12 = E.dev(_factor(np.eye(m) * R2 if np.isscalar(R2) else R2, m, "R2"))
        dz, dm = self._measurements(np.asarray(z, dtype=np.float64).reshape(1, N, m), 1,
                                    None if mask is None else np.asarray(mask).reshape(1, N))
        x, P12 = self._state()
        shapes = ((m,), (n, m), (m, m), (m, m))
        outs = [E.to_records(np.asarray(getattr(self, k), dtype=np.float64).reshape(N, -1), self.layout, 0).clone()
                for k in ("y", "K", "S1_2", "SI1_2")]
        st = torch.zeros(N, dtype=torch.int32, device=x.device)
        E.srkf_update(_desc(n, m, 0, N, 1, self.layout), H, R12, dz.reshape(dz.shape[1:]), x, P12,
                      mask=None if dm is None else dm.reshape(N), y=outs[0], K=outs[1], S12=outs[2], SI12=outs[3], status=st)
        E.raise_on_status(st, "SquareRootKalmanFilterBank.update (S1_2 is singular)")
        self.x = self._host(x, 0, (n,))
        self._P1_2 = self._host(P12, 0, (n, n))
        self.y, self.K, self.S1_2, self.SI1_2 = (self._host(o, 0, shp) for o, shp in zip(outs, shapes))

    def batch_filter(self, zs, mask=None, us=None, update_first=False, device_outputs=False):
        """(means, sqrt_covs, means_p, sqrt_covs_p) of the whole run, ONE launch; x and P1_2 are left alone.  zs (T, N, dim_z)
        with NaN rows missing (or device records in `layout`), mask (T, N) bool (False = missing), us (T, N, dim_u)."""
        import torch
        n, m, N = self.dim_x, self.dim_z, self.n_tracks
        T = int(zs.shape[0]) if hasattr(zs, "shape") else len(zs)
        if T == 0:
            e = np.zeros((0, N, n))
            return e, np.zeros((0, N, n, n)), e.copy(), np.zeros((0, N, n, n))
        F, Q12, H, R12 = self._model()
        dz, dm = self._measurements(zs, T, mask)
        B, du = self._controls(us, T)
        x, P12 = self._state()
        dev = x.device
        means, means_p = E.alloc_records((T,), N, n, self.layout, dev), E.alloc_records((T,), N, n, self.layout, dev)
        covs, covs_p = E.alloc_records((T,), N, n * n, self.layout, dev), E.alloc_records((T,), N, n * n, self.layout, dev)
        st = torch.zeros(N, dtype=torch.int32, device=dev)
        nu = 0 if B is None else int(B.shape[1])
        E.srkf_batch(_desc(n, m, nu, N, T, self.layout, update_first), F, Q12, H, R12, dz, x, P12, B=B, u=du, mask=dm,
                     means=means, covs=covs, means_p=means_p, covs_p=covs_p, status=st)
        E.raise_on_status(st, "SquareRootKalmanFilterBank.batch_filter (S1_2 is singular)")
        if device_outputs:
            return means, covs, means_p, covs_p
        return (self._host(means, 1, (n,)), self._host(covs, 1, (n, n)),
                self._host(means_p, 1, (n,)), self._host(covs_p, 1, (n, n)))

    def __repr__(self):
        return "\n".join(["SquareRootKalmanFilterBank object (filterpy_amd, gfx950)"] +
                         [f"{k} = {getattr(self, k)!r}" for k in
                          ("dim_x", "dim_z", "dim_u", "n_tracks", "layout", "F", "Q", "R", "H", "B")])
