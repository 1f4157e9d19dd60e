"""Information filter with filterpy's call surface, computed by the gfx950 kernels.

Mirrors rlabbe/filterpy v1.4.5 filterpy/kalman/information_filter.py:

    InformationFilter.__init__ (:130-175)  update (:178-243)  predict (:245-289)  batch_filter (:291-326, NotImplementedError)
    the F and P properties (:365-379)  __repr__ (:381-404)

The information filter is the inverse-covariance form of the Kalman filter: its state is x and P_inv, its measurement noise
is R_inv.  `InformationFilter` is ONE filter, like the reference: each predict() / update() is one launch on a bank of one
(fk_info_predict_f64 / fk_info_update_f64, include/filterhip.h).  `InformationFilterBank` is the same arithmetic for n_tracks
filters that share F, H, Q, R_inv and B, with a batch_filter that runs the whole time loop in ONE launch (fk_info_batch_f64)
-- the reference's own batch_filter raises NotImplementedError.  Where the reference calls numpy.linalg.inv three times per
step (on F^-T P_inv F^-1, on its inverse plus Q, on S), the kernel factors two symmetric positive definite matrices as L D L'
(csrc/fk_info.hpp) and never needs F^-1; the results agree to rounding.

The reference's semantics are kept: S is the updated P_inv; update(None) only records z = None and the posterior copies; a
scalar R_inv argument means eye(dim_z) * R_inv; the F setter computes _F_inv with self.inv (only __repr__ shows it);
log_likelihood / likelihood are logpdf(y, cov=S) on the host, evaluated when read.  Divergences:
  * a singular matrix raises numpy.linalg.LinAlgError: when a pivot of P_inv (predict), of F P F' + Q (predict) or of the
    updated P_inv (update) is at or below dim_x eps max|diag|.  The reference's _no_information branch (an exactly singular
    F^-T P_inv F^-1, e.g. P_inv = 0) is not ported: it leaves x holding an information vector, never stores the predicted
    P_inv and, with dim_z < dim_x, goes on with rounding noise;
  * inv other than numpy.linalg.inv raises NotImplementedError on predict() / update() (the device inverts);
  * P_inv, Q and R_inv (the attribute and the argument given as a matrix) must be matrices of the right shape: a scalar raises
    ValueError (the reference adds a scalar P_inv to every entry of H' R_inv H).  P_inv is symmetric: its lower triangle is read;
  * shapes the reference broadcasts into nonsense raise ValueError: x that is neither (dim_x,) nor (dim_x, 1); a measurement
    whose shape does not match x; a control input whose size is not B's column count (dim_x with a scalar B) or whose
    orientation does not match x; a nonzero scalar u with a matrix B (as SquareRootKalmanFilter);
  * with 1 < dim_z < dim_x the reference's logpdf(y, cov=S) cannot broadcast y against the (dim_x, dim_x) S and update()
    raises ValueError there unless compute_log_likelihood is False; here that ValueError appears when log_likelihood is read.
"""
import math
import sys
from copy import deepcopy

import numpy as np

from .. import _engine as E
from ..common.helpers import logpdf
from ._bank import _SharedModelBank, _desc, _step_control, _xshape, _z
from .kalman_filter import _mat

__all__ = ["InformationFilter", "InformationFilterBank"]


def _square(A, k, name):
    """a (k, k) float64 matrix, or ValueError (scalars included)"""
    M = np.asarray(A, dtype=np.float64)
    if M.shape != (k, k):
        raise ValueError(f"{name} has shape {M.shape}, expected ({k}, {k})")
    return np.ascontiguousarray(M)


def _r_inv(R_inv, m):
    """the R_inv argument of update(): a scalar means eye * R_inv (information_filter.py:200-203)"""
    return _square(np.eye(m) * R_inv if np.isscalar(R_inv) else R_inv, m, "R_inv")


class InformationFilter(object):
    """filterpy.kalman.InformationFilter (information_filter.py:30-404) on the GPU: same attributes, defaults and results."""

    def __init__(self, dim_x, dim_z, dim_u=0, compute_log_likelihood=True):
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
        self.P_inv = np.eye(dim_x)
        self.Q = np.eye(dim_x)
        self.B = 0.
        self._F = 0.
        self._F_inv = 0.
        self.H = np.zeros((dim_z, dim_x))
        self.R_inv = np.eye(dim_z)
        self.K = 0.
        self.y = np.zeros((dim_z, 1))
        self.z = np.zeros((dim_z, 1))
        self.S = 0.
        self._I = np.eye(dim_x)
        self._no_information = False
        self.compute_log_likelihood = compute_log_likelihood
        self._log_likelihood = math.log(sys.float_info.min)
        self._likelihood = sys.float_info.min
        self.inv = np.linalg.inv
        self.x_prior = np.copy(self.x)
        self.P_inv_prior = np.copy(self.P_inv)
        self.x_post = np.copy(self.x)
        self.P_inv_post = np.copy(self.P_inv)

    def _check_inv(self):
        if self.inv is not np.linalg.inv:
            raise NotImplementedError("InformationFilter.inv other than numpy.linalg.inv: the inverses are taken on the device")

    # -- the reference's methods --------------------------------------------------------------------------------------------
    def update(self, z, R_inv=None):
        """information_filter.py:178-243.  z None: bookkeeping only (:194-198)."""
        if z is None:
            self.z = None
            self.x_post = self.x.copy()
            self.P_inv_post = self.P_inv.copy()
            return
        self._check_inv()
        n, m = self.dim_x, self.dim_z
        xshape = _xshape(self.x, n)
        za = _z(z, m, xshape)
        Ri = _square(self.R_inv, m, "R_inv") if R_inv is None else _r_inv(R_inv, m)
        H = _mat(self.H, m, n, "H")
        Pi = _square(self.P_inv, n, "P_inv")
        import torch
        E.require_gpu()
        x = E.dev(np.asarray(self.x, dtype=np.float64).reshape(1, n))
        dPi = E.dev(Pi.reshape(1, n, n))
        y, K = E.alloc_records((), 1, m, "aos"), E.alloc_records((), 1, n * m, "aos")
        st = torch.zeros(1, dtype=torch.int32, device=x.device)
        E.info_update(_desc(n, m, 0, 1, 1, "aos"), E.dev(H), E.dev(Ri), E.dev(za.reshape(1, m)), x, dPi, y=y, K=K, status=st)
        E.raise_on_status(st, "InformationFilter.update (P_inv + H' R_inv H is singular)")
        # y has z's shape minus dot(H, x)'s, as numpy broadcasts them: a scalar or (1,) z against a column x gives (1, 1)
        yshape = np.broadcast_shapes(za.shape, (m,) + xshape[1:])
        self.y = y.cpu().numpy().reshape(yshape)
        self.K = K.cpu().numpy().reshape(n, m)
        self.x = x.cpu().numpy().reshape(xshape)
        self.P_inv = dPi.cpu().numpy().reshape(n, n)
        self.S = self.P_inv.copy()
        if self.compute_log_likelihood:
            self._log_likelihood = self._likelihood = None
        self.z = deepcopy(z)
        self.x_post = self.x.copy()
        self.P_inv_post = self.P_inv.copy()

    def predict(self, u=0):
        """information_filter.py:245-289, the invertible branch"""
        self._check_inv()
        n = self.dim_x
        xshape = _xshape(self.x, n)
        B, uu = _step_control(self.B, u, n, xshape)
        F = _mat(self._F, n, n, "F")
        Q = _square(self.Q, n, "Q")
        Pi = _square(self.P_inv, n, "P_inv")
        import torch
        E.require_gpu()
        x = E.dev(np.asarray(self.x, dtype=np.float64).reshape(1, n))
        dPi = E.dev(Pi.reshape(1, n, n))
        st = torch.zeros(1, dtype=torch.int32, device=x.device)
        nu = 0 if B is None else B.shape[1]
        E.info_predict(_desc(n, self.dim_z, nu, 1, 1, "aos"), E.dev(F), E.dev(Q), x, dPi,
                       B=None if B is None else E.dev(B), u=None if B is None else E.dev(uu.reshape(1, nu)), status=st)
        E.raise_on_status(st, "InformationFilter.predict (P_inv or F P F' + Q is singular: the reference's no-information "
                              "branch is not supported)")
        self.x = x.cpu().numpy().reshape(xshape)
        self.P_inv = dPi.cpu().numpy().reshape(n, n)
        self.P_inv_prior = np.copy(self.P_inv)
        self.x_prior = np.copy(self.x)

    def batch_filter(self, zs, Rs=None, update_first=False, saver=None):
        """information_filter.py:291-326: not implemented in the reference either (InformationFilterBank.batch_filter is)"""
        raise NotImplementedError("this is not implemented yet")

    @property
    def log_likelihood(self):
        """log-likelihood of the last measurement: logpdf(y, cov=S) (:234-235), evaluated when read"""
        if self._log_likelihood is None:
            self._log_likelihood = logpdf(x=self.y, cov=self.S)
        return self._log_likelihood

    @log_likelihood.setter
    def log_likelihood(self, value):
        self._log_likelihood = value

    @property
    def likelihood(self):
        """likelihood of the last measurement, never below sys.float_info.min (:236-238)"""
        if self._likelihood is None:
            self._likelihood = math.exp(self.log_likelihood)
            if self._likelihood == 0:
                self._likelihood = sys.float_info.min
        return self._likelihood

    @likelihood.setter
    def likelihood(self, value):
        self._likelihood = value

    @property
    def F(self):
        """State Transition matrix"""
        return self._F

    @F.setter
    def F(self, value):
        self._F = value
        self._F_inv = self.inv(self._F)

    @property
    def P(self):
        """State covariance matrix"""
        return self.inv(self.P_inv)

    def __repr__(self):
        return "\n".join(["InformationFilter object (filterpy_amd, gfx950)"] +
                         [f"{k} = {getattr(self, k)!r}" for k in
                          ("dim_x", "dim_z", "dim_u", "x", "P_inv", "x_prior", "P_inv_prior", "F", "_F_inv", "Q", "R_inv", "H",
                           "K", "y", "z", "S", "B", "log_likelihood", "likelihood", "inv")])


class InformationFilterBank(_SharedModelBank):
    """n_tracks independent information filters that share F, H, Q, R_inv and B, stepped in lock-step on the GPU:

        x (N, dim_x)   P_inv (N, dim_x, dim_x)   zs (T, N, dim_z)   us (T, N, dim_u)   B (dim_x, dim_u)

    predict(u) / update(z, R_inv, mask) are one launch each; a NaN row of z is a missing measurement.  batch_filter returns
    (means, P_invs, means_p, P_invs_p) -- (T, N, n) and (T, N, n, n) NumPy arrays, or with device_outputs=True the device
    tensors in `layout` ('aos' [T][N][..], 'soa' [T][..][N]) -- from ONE launch; x and P_inv are left alone.  A singular P_inv
    (or F P F' + Q) raises numpy.linalg.LinAlgError."""

    _ENGINE, _COV = "info", "P_inv"
    _BYPRODUCTS = (("y", "y", "m"), ("K", "K", "nm"))
    _SINGULAR = {"predict": " (P_inv or F P F' + Q is singular)", "update": " (P_inv + H' R_inv H is singular)",
                 "batch_filter": " (P_inv or F P F' + Q is singular)"}

    def __init__(self, dim_x, dim_z, n_tracks, dim_u=0, layout="soa"):
        super().__init__(dim_x, dim_z, n_tracks, dim_u, layout)
        self.P_inv = np.tile(np.eye(dim_x), (n_tracks, 1, 1))
        self.Q = np.eye(dim_x)
        self.R_inv = np.eye(dim_z)

    @property
    def P(self):
        """the covariances, inv(P_inv) per track (host)"""
        return np.linalg.inv(self._p_inv())

    # -- what the shared plumbing asks for ------------------------------------------------------------------------------------
    def _p_inv(self):
        n, N = self.dim_x, self.n_tracks
        Pi = np.asarray(self.P_inv, dtype=np.float64)
        if Pi.shape == (n, n):
            Pi = np.broadcast_to(Pi, (N, n, n))
        if Pi.shape != (N, n, n):
            raise ValueError(f"P_inv has shape {Pi.shape}, expected ({N}, {n}, {n}) or ({n}, {n})")
        return np.ascontiguousarray(Pi)

    def _model(self, R_inv=None):
        n, m = self.dim_x, self.dim_z
        model = (E.dev(_mat(self.F, n, n, "F")), E.dev(_square(self.Q, n, "Q")), E.dev(_mat(self.H, m, n, "H")),
                 E.dev(_square(self.R_inv, m, "R_inv")))
        if R_inv is not None:
            model = model[:3] + (E.dev(_r_inv(R_inv, m)),)
        return model

    def _state(self):
        n, N = self.dim_x, self.n_tracks
        return self._x_records(), E.to_records(self._p_inv().reshape(N, n * n), self.layout, 0).clone()

    def update(self, z, R_inv=None, mask=None):
        """one update for every track: z (n_tracks, dim_z), NaN rows missing; R_inv a matrix or a scalar (eye * R_inv) for this
        call; mask (n_tracks,) bool, False = missing.  Sets y and K of the tracks that update."""
        self._update(z, R_inv, mask)

    def __repr__(self):
        return "\n".join(["InformationFilterBank object (filterpy_amd, gfx950)"] +
                         [f"{k} = {getattr(self, k)!r}" for k in
                          ("dim_x", "dim_z", "dim_u", "n_tracks", "layout", "F", "Q", "R_inv", "H", "B")])
