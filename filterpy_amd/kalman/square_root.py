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
from ._bank import _SharedModelBank, _desc, _step_control, _xshape, _z
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

    # -- the reference's methods --------------------------------------------------------------------------------------------
    def update(self, z, R2=None):
        """square_root.py:172-224.  z None: bookkeeping only (:189-193)."""
        if z is None:
            self.z = np.array([[None] * self.dim_z]).T
            self.x_post = self.x.copy()
            self._P1_2_post = np.copy(self._P1_2)
            return
        n, m = self.dim_x, self.dim_z
        xshape = _xshape(self.x, n)
        zr = _z(z, m, xshape)
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
        xshape = _xshape(self.x, n)
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


class SquareRootKalmanFilterBank(_SharedModelBank):
    """n_tracks independent square-root filters that share F, H, Q, R and B, stepped in lock-step on the GPU:

        x (N, dim_x)   P1_2 (N, dim_x, dim_x)   zs (T, N, dim_z)   us (T, N, dim_u)   B (dim_x, dim_u)

    The P, Q and R setters factor (per track for P) with a lower Cholesky factorisation, as the reference's do; P1_2 can be
    set directly (lower triangular).  predict(u) / update(z, R2, mask) are one launch each; a NaN row of z is a missing
    measurement.  batch_filter returns (means, sqrt_covs, means_p, sqrt_covs_p) -- (T, N, n) and (T, N, n, n) NumPy arrays, or
    with device_outputs=True the device tensors in `layout` ('aos' [T][N][..], 'soa' [T][..][N]) -- from ONE launch; x and P1_2
    are left alone."""

    _ENGINE, _COV = "srkf", "_P1_2"
    _BYPRODUCTS = (("y", "y", "m"), ("K", "K", "nm"), ("S1_2", "S12", "mm"), ("SI1_2", "SI12", "mm"))
    _SINGULAR = {"update": " (S1_2 is singular)", "batch_filter": " (S1_2 is singular)"}

    def __init__(self, dim_x, dim_z, n_tracks, dim_u=0, layout="soa"):
        super().__init__(dim_x, dim_z, n_tracks, dim_u, layout)
        self._P1_2 = np.tile(np.eye(dim_x), (n_tracks, 1, 1))
        self._Q1_2 = np.eye(dim_x)
        self._R1_2 = np.eye(dim_z)

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

    # -- what the shared plumbing asks for ------------------------------------------------------------------------------------
    def _model(self, R2=None):
        n, m = self.dim_x, self.dim_z
        model = (E.dev(_mat(self.F, n, n, "F")), E.dev(_factor(self._Q1_2, n, "Q1_2")), E.dev(_mat(self.H, m, n, "H")),
                 E.dev(_factor(self._R1_2, m, "R1_2")))
        if R2 is not None:
            model = model[:3] + (E.dev(_factor(np.eye(m) * R2 if np.isscalar(R2) else R2, m, "R2")),)
        return model

    def _state(self):
        n, N = self.dim_x, self.n_tracks
        x = self._x_records()
        L = np.asarray(self._P1_2, dtype=np.float64)
        if L.shape != (N, n, n):
            raise ValueError(f"P1_2 has shape {L.shape}, expected ({N}, {n}, {n})")
        if np.any(np.triu(L, 1) != 0):
            raise ValueError("P1_2 must be lower triangular")
        return x, E.to_records(L.reshape(N, n * n), self.layout, 0).clone()

    def update(self, z, R2=None, mask=None):
        """one update for every track: z (n_tracks, dim_z), NaN rows missing; R2 a lower-triangular factor or a scalar
        (eye * R2) for this call; mask (n_tracks,) bool, False = missing.  Sets y, K, S1_2, SI1_2 of the tracks that update."""
        self._update(z, R2, mask)

    def __repr__(self):
        return "\n".join(["SquareRootKalmanFilterBank object (filterpy_amd, gfx950)"] +
                         [f"{k} = {getattr(self, k)!r}" for k in
                          ("dim_x", "dim_z", "dim_u", "n_tracks", "layout", "F", "Q", "R", "H", "B")])
