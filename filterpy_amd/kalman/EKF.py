"""Extended Kalman filter with filterpy's call surface, arithmetic on the GPU.

Mirrors rlabbe/filterpy v1.4.5 filterpy/kalman/EKF.py:

    __init__ (:132-170)   predict_update (:172-252)   update (:254-342)   predict_x (:344-351)   predict (:353-371)
    log_likelihood / likelihood / mahalanobis (:373-410)   __repr__ (:412-428)

What is nonlinear in an EKF -- the Jacobian H = HJacobian(x) and the innovation y = residual(z, Hx(x)) -- comes from the
caller's Python callables; everything else is three gfx950 kernels (csrc/ekf_kernels.hip) that take H and y as records of each
track: fk_ekf_predict_f64 (x = F x + B u, P = F P F' + Q), fk_ekf_update_f64 (S, K through an in-lane L D L', x += K y, the
Joseph form, log-likelihood and Mahalanobis distance) and fk_ekf_step_f64 (that update and the next predict in one launch).

Three ways to run the callables, chosen like CubatureKalmanFilter's:

* one filter, as the reference: ``HJacobian(x (n, 1), *args)`` returns (m, n), ``Hx(x, *hx_args)`` returns m values in any
  shape, ``residual(z, hx)`` their difference;
* ``n_tracks=N`` turns the object into a bank of N independent filters: x (N, n), P (N, n, n), z (N, m), K (N, n, m), y (N, m),
  S / SI (N, m, m); F, Q, R may be (n, n) or (N, n, n) (one matrix per track: FK_MODEL_PER_TRACK), B (n, dim_u) or
  (N, n, dim_u).  By default the callables run track by track with the single filter's shapes (x an (n, 1) column);
* ``vectorized=True``: once per call on NumPy arrays, ``HJacobian(x (N, n), *args)`` -> (N, m, n), ``Hx(x (N, n), *hx_args)`` ->
  (N, m), ``residual(z (N, m), hx (N, m))`` -> (N, m);
* ``device_callables=True`` (banks only): the same shapes on float64 CUDA tensors.  predict() / update() still hand x, P and
  the by-products back to the host attributes after every call; ``batch_filter`` keeps state and histories in HBM.

``update(..., mask=None)`` (banks only): a (N,) array, False = that track has no measurement; its x, P, K, S, SI, y and
likelihoods stay as they are.

``batch_filter(zs (T, N, m), HJacobian, Hx, args=(), hx_args=(), residual=np.subtract, us=None, saver=None,
device_outputs=False)`` (banks only; the reference has none) runs predict then update per step and returns (means,
covariances, means_p, covariances_p).  With device callables, no saver and no predict_x override it is one
fk_ekf_predict_f64, T - 1 fk_ekf_step_f64 and one fk_ekf_update_f64, bit-identical to the loop of predict() / update(); the model
goes to the device once, before the loop.  Inside a launch P crosses HBM once per step; the loop adds one device copy of x and P per
step, into the prior histories (the kernels work in place).  Otherwise it is the loop of predict() / update().

Speed: the shapes of csrc/fk_dims_ekf.def -- (1,1) (2,1) (2,2) (3,1) (3,2) (4,2) (4,4) (6,2) (6,3) (7,3) -- run register-resident
kernels near the memory bound.  EVERY OTHER size, (8,4) included, runs a padded general kernel that is a correctness path: at
(8,4) and 1e6 tracks an update takes 60 ms, 16-28 times what fk_kf_update_f64 with a per-track H takes (docs/MEASUREMENTS.md,
"Extended Kalman filter").

Kept from the reference:
  * predict_update evaluates HJacobian at the state BEFORE the predict and Hx at the predicted state (:222-238), forms
    y = z - Hx(x) without a residual function, stores the PRE-predict x and P as x_prior / P_prior (:229-230) and does not
    call predict_x;
  * update(None) only copies the posts (:297-301);
  * a scalar R argument is eye * R (:311-312); a scalar R ATTRIBUTE with dim_z > 1 adds r to every element of S and forms
    r K K' (:320, :332; FK_KF_FLAG_R_JOSEPH_DIAG);
  * a scalar z with dim_z == 1 is accepted (:212-213, :314-315);
  * predict() calls predict_x(u): a subclass that overrides it computes x itself, the kernel then supplies only P (:366-367);
  * the likelihoods are lazy attributes of the last update; x keeps the shape it was given ((n,) or (n, 1)), y the shape
    residual() returned.
Divergences:
  * predict_update(None, ...): the reference's docstring promises a predict-only step, its code raises TypeError half-way
    through (z - Hx(x), after S, SI and K were overwritten); here TypeError is raised before any state is touched;
  * an S with a non-positive pivot raises numpy.linalg.LinAlgError (the reference's inv raises for an exactly singular S only);
  * log_likelihood and mahalanobis are the kernel's by-products of the update (from the factorisation of S), not scipy's.
"""
import sys
from copy import deepcopy
from math import exp, log

import numpy as np

from .. import _engine as E
from .._abi import FK_KF_FLAG_R_JOSEPH_DIAG, FK_MODEL_PER_TRACK, FK_MODEL_SHARED
from ._bank import _step_control
from ._callable import _CallableHost, alloc_histories, as_records, host_histories, status, to_rec, track_rows

__all__ = ["ExtendedKalmanFilter"]


def _tuple(a):
    return a if isinstance(a, tuple) else (a,)


class ExtendedKalmanFilter(_CallableHost):
    """filterpy.kalman.ExtendedKalmanFilter (EKF.py:32-428) on the GPU: same attributes, defaults and results."""

    def __init__(self, dim_x, dim_z, dim_u=0, n_tracks=None, vectorized=False, layout="soa", device_callables=False):
        self._preamble(n_tracks, vectorized, device_callables, layout, dims=(dim_x, dim_z), vectorized_bank_only=True)
        self._resident = None                   # batch_filter's fused loop: the model's device operands, uploaded once
        self.dim_x = dim_x
        self.dim_z = dim_z
        self.dim_u = dim_u
        bank = n_tracks is not None
        lead = (n_tracks,) if bank else ()
        self.x = np.zeros((n_tracks, dim_x)) if bank else np.zeros((dim_x, 1))
        self.P = np.tile(np.eye(dim_x), lead + (1, 1)) if bank else np.eye(dim_x)
        self.B = 0
        self.F = np.eye(dim_x)
        self.R = np.eye(dim_z)
        self.Q = np.eye(dim_x)
        self.z = np.array([[None] * dim_z]).T
        self.K = np.zeros((n_tracks, dim_x, dim_z)) if bank else np.zeros(self.x.shape)
        self.y = np.zeros((n_tracks, dim_z)) if bank else np.zeros((dim_z, 1))
        self.S = np.zeros(lead + (dim_z, dim_z))
        self.SI = np.zeros(lead + (dim_z, dim_z))
        self._I = np.eye(dim_x)
        self._log_likelihood = np.full(n_tracks, log(sys.float_info.min)) if bank else log(sys.float_info.min)
        self._likelihood = np.full(n_tracks, sys.float_info.min) if bank else sys.float_info.min
        self._mahalanobis = None
        self.x_prior = self.x.copy()
        self.P_prior = self.P.copy()
        self.x_post = self.x.copy()
        self.P_post = self.P.copy()

    # ---------------------------------------------------------------------------------------------------------- helpers --
    def _matrix(self, A, r, c, name):
        """a model matrix: (r, c), or for a bank (N, r, c)"""
        M = np.asarray(A, dtype=np.float64)
        if M.shape == (r, c) or (self._N is not None and M.shape == (self._N, r, c)):
            return M
        raise ValueError(f"{name} has shape {M.shape}, expected ({r}, {c})" + (f" or ({self._N}, {r}, {c})" if self._N else ""))

    def _R(self, R):
        """update()'s R (:309-312) -> (matrix, descriptor flags)"""
        m = self.dim_z
        if R is None:
            R = self.R
        elif np.isscalar(R):
            R = np.eye(m) * R
        if np.ndim(R) == 0:                                    # a scalar ATTRIBUTE: :320 adds it to every element of S
            return np.full((m, m), float(R)), (FK_KF_FLAG_R_JOSEPH_DIAG if m > 1 else 0)
        return self._matrix(R, m, m, "R"), 0

    def _control(self, u):
        """predict's dot(B, u) -> (B (n, nu) or (N, n, nu), u (N, nu)) or (None, None)"""
        n, N = self.dim_x, self._N or 1
        if self._N is None:
            Bm, uv = _step_control(self.B, u, n, np.shape(self.x))
            return (None, None) if Bm is None else (Bm, uv.reshape(1, -1))
        if u is None or (np.ndim(u) == 0 and float(u) == 0.0):
            return None, None
        if np.ndim(self.B) == 0:
            if float(self.B) == 0.0:
                return None, None
            Bm = np.eye(n) * float(self.B)
        else:
            Bm = np.asarray(self.B, dtype=np.float64)
        if Bm.ndim not in (2, 3) or Bm.shape[-2] != n or (Bm.ndim == 3 and Bm.shape[0] != N):
            raise ValueError(f"B has shape {Bm.shape}, expected ({n}, dim_u) or ({N}, {n}, dim_u)")
        nu = Bm.shape[-1]
        import torch
        if isinstance(u, torch.Tensor):
            if tuple(u.shape) != (N, nu):
                raise ValueError(f"u has shape {tuple(u.shape)}, expected ({N}, {nu})")
            return Bm, u
        try:
            uv = np.ascontiguousarray(np.broadcast_to(np.asarray(u, dtype=np.float64), (N, nu)))
        except ValueError:
            raise ValueError(f"u has shape {np.shape(u)}, expected ({N}, {nu}) or ({nu},)") from None
        return Bm, uv

    def _operands(self, mats):
        """{name: host matrix, (r, c) or (N, r, c)} -> (model_mode, {name: device operand}): one matrix per track for all of
        them as soon as one of them is"""
        N, lay = self._N or 1, self._layout
        mats = {k: v for k, v in mats.items() if v is not None}
        if self._resident is not None and tuple(sorted(mats)) in self._resident:
            return self._resident[tuple(sorted(mats))]           # (batch_filter: the model went up before the loop)
        pt = any(v.ndim == 3 for v in mats.values())
        out = {}
        for k, v in mats.items():
            if pt:
                out[k] = E.to_records(np.ascontiguousarray(np.broadcast_to(v, (N,) + v.shape[-2:])), lay, 0)
            else:
                out[k] = E.dev(np.ascontiguousarray(v))
        res = (FK_MODEL_PER_TRACK if pt else FK_MODEL_SHARED), out
        if self._resident is not None:
            self._resident[tuple(sorted(mats))] = res
        return res

    def _desc(self, mode, nu=0, flags=0):
        return dict(n=self.dim_x, m=self.dim_z, nu=nu, model_mode=mode, N=self._N or 1, T=1, layout=E.LAYOUTS[self._layout],
                    update_first=0, alpha_sq=1.0, flags=flags)

    def _to_rec(self, t, shape, what):
        """(N,) + shape as a callable returned it (array or, with device callables, tensor) -> device records"""
        return to_rec(t, self._N or 1, shape, self._layout, self._mode == "torch", what)

    def _xview(self, dx):
        """x records -> (N, n) device tensor for the device callables"""
        return track_rows(dx, self._layout)

    def _jacobian(self, HJacobian, args, xb, dx=None):
        """H of every track -> device records [N][m*n]"""
        n, m, N = self.dim_x, self.dim_z, self._N or 1
        if self._mode == "torch":
            return self._to_rec(HJacobian(self._xview(dx), *args), (m, n), "HJacobian")
        if self._mode == "vec":
            return self._to_rec(HJacobian(xb.copy(), *args), (m, n), "HJacobian")
        if self._N is None:
            H = np.asarray(HJacobian(self.x, *args), dtype=np.float64)
            if H.shape != (m, n):
                raise ValueError(f"HJacobian returned shape {H.shape}, expected ({m}, {n})")
            return E.to_records(np.ascontiguousarray(H[None]), self._layout, 0)
        Hs = np.empty((N, m, n))
        for i in range(N):
            H = np.asarray(HJacobian(xb[i].reshape(n, 1).copy(), *args), dtype=np.float64)
            if H.shape != (m, n):
                raise ValueError(f"HJacobian returned shape {H.shape} for track {i}, expected ({m}, {n})")
            Hs[i] = H
        return E.to_records(Hs, self._layout, 0)

    def _innovation(self, z, Hx, hx_args, residual, xb, dx=None, x_single=None):
        """y = residual(z, Hx(x)) -> (the y attribute, device records [N][m])"""
        m, N = self.dim_z, self._N or 1
        if self._mode == "torch":
            import torch
            dz = z if isinstance(z, torch.Tensor) else E.dev(np.asarray(z, dtype=np.float64))
            if tuple(dz.shape) != (N, m):
                raise ValueError(f"measurement of shape {tuple(dz.shape)}, expected ({N}, {m})")
            if residual is np.subtract:                       # (NumPy's ufunc does not take device tensors)
                residual = torch.sub
            y = residual(dz, Hx(self._xview(dx), *hx_args))
            return None, self._to_rec(y, (m,), "residual")
        if self._N is None:
            y = np.asarray(residual(z, Hx(self.x if x_single is None else x_single, *hx_args)), dtype=np.float64)
            if y.size != m:
                raise ValueError(f"residual returned {y.size} values, expected dim_z = {m}")
            return y, E.to_records(np.ascontiguousarray(y.reshape(1, m)), self._layout, 0)
        zb = np.asarray(z, dtype=np.float64)
        if zb.shape != (N, m):
            raise ValueError(f"measurement of shape {zb.shape}, expected ({N}, {m})")
        if self._mode == "vec":
            y = np.asarray(residual(zb, np.asarray(Hx(xb.copy(), *hx_args))), dtype=np.float64)
            if y.shape != (N, m):
                raise ValueError(f"residual returned shape {y.shape}, expected ({N}, {m})")
        else:
            y = np.empty((N, m))
            n = self.dim_x
            for i in range(N):
                hx = np.asarray(Hx(xb[i].reshape(n, 1).copy(), *hx_args), dtype=np.float64)
                if hx.size != m:
                    raise ValueError(f"Hx returned {hx.size} values for track {i}, expected dim_z = {m}")
                y[i] = np.ravel(residual(zb[i].reshape(hx.shape), hx))
        return y, E.to_records(np.ascontiguousarray(y), self._layout, 0)

    def _set_state(self, dx, dP):
        n, lay = self.dim_x, self._layout
        x, P = E.from_records(dx, lay, 0, (n,)), E.from_records(dP, lay, 0, (n, n))
        if self._N is not None:
            self.x, self.P = np.array(x), np.array(P)
        else:
            self.x, self.P = x[0].reshape(np.shape(self.x)).copy(), P[0].copy()

    # ---------------------------------------------------------------------------------------------------------- predict --
    def _dev_predict(self, dx, dP, u, st):
        """:351, :367 on device records"""
        n = self.dim_x
        Bm, uv = self._control(u)
        mode, ops = self._operands(dict(F=self._matrix(self.F, n, n, "F"), Q=self._matrix(self.Q, n, n, "Q"), B=Bm))
        du = None if uv is None else (self._to_urec(uv))
        E.ekf_predict(self._desc(mode, nu=0 if Bm is None else Bm.shape[-1]), ops["F"], ops["Q"], dx, dP, B=ops.get("B"), u=du,
                      status=st)

    def _to_urec(self, uv):
        import torch
        if isinstance(uv, torch.Tensor):
            return as_records(uv.to(dtype=torch.float64), self._N or 1, self._layout)
        return E.to_records(uv, self._layout, 0)

    def _predict(self, u, keep_x):
        N, lay = self._N or 1, self._layout
        dx, dP = E.to_records(self._xb(), lay, 0).clone(), E.to_records(self._Pb(), lay, 0).clone()
        st = status(N, dx)
        self._dev_predict(dx, dP, u, st)
        E.raise_on_status(st, "ExtendedKalmanFilter.predict")
        x_own = self.x
        self._set_state(dx, dP)
        if keep_x:
            self.x = x_own

    def predict_x(self, u=0):
        """EKF.py:344-351: x = F x + B u.  Override it to propagate the state yourself; predict() then takes only P from the
        kernel."""
        P = self.P
        self._predict(u, keep_x=False)
        self.P = P

    def predict(self, u=0):
        """EKF.py:353-371"""
        if type(self).predict_x is not ExtendedKalmanFilter.predict_x:
            self.predict_x(u)                                  # the subclass's x (:366) ...
            self._predict(0, keep_x=True)                      # ... and the kernel's P = F P F' + Q (:367)
        else:
            self._predict(u, keep_x=False)
        self.x_prior = np.copy(self.x)
        self.P_prior = np.copy(self.P)

    # ----------------------------------------------------------------------------------------------------------- update --
    def _dev_update(self, dx, dP, dH, dy, Rm, flags, st, mask=None, by=None, step=None):
        """:319-332 on device records (step: dict(u=, x_post=, P_post=): fk_ekf_step_f64 -- the next predict in the same launch)"""
        n = self.dim_x
        by = by or {}
        kw = dict(mask=mask, K=by.get("K"), S=by.get("S"), SI=by.get("SI"), log_likelihood=by.get("ll"),
                  mahalanobis=by.get("maha"), status=st)
        if step is None:
            mode, ops = self._operands(dict(R=Rm))
            E.ekf_update(self._desc(mode, flags=flags), dH, ops["R"], dy, dx, dP, **kw)
            return
        Bm, uv = self._control(step.get("u"))
        mode, ops = self._operands(dict(R=Rm, F=self._matrix(self.F, n, n, "F"), Q=self._matrix(self.Q, n, n, "Q"), B=Bm))
        du = None if uv is None else self._to_urec(uv)
        E.ekf_step(self._desc(mode, nu=0 if Bm is None else Bm.shape[-1], flags=flags), dH, ops["R"], dy, ops["F"], ops["Q"],
                   dx, dP, B=ops.get("B"), u=du, x_post=step.get("x_post"), P_post=step.get("P_post"), **kw)

    def _by_products(self, dx, masked):
        """records for K, S, SI, log-likelihood and Mahalanobis distance; with a mask preset to the attributes, which the
        tracks without a measurement keep"""
        n, m, N, lay = self.dim_x, self.dim_z, self._N or 1, self._layout
        if not masked:
            import torch
            return dict(K=E.alloc_records((), N, n * m, lay), S=E.alloc_records((), N, m * m, lay),
                        SI=E.alloc_records((), N, m * m, lay), ll=torch.empty(N, dtype=torch.float64, device=dx.device),
                        maha=torch.empty(N, dtype=torch.float64, device=dx.device))
        maha = np.zeros(N) if self._mahalanobis is None else np.asarray(self._mahalanobis, dtype=np.float64)
        return dict(K=E.to_records(np.asarray(self.K, dtype=np.float64).reshape(N, n, m), lay, 0).clone(),
                    S=E.to_records(np.asarray(self.S, dtype=np.float64).reshape(N, m, m), lay, 0).clone(),
                    SI=E.to_records(np.asarray(self.SI, dtype=np.float64).reshape(N, m, m), lay, 0).clone(),
                    ll=E.dev(np.asarray(self._log_likelihood, dtype=np.float64).reshape(N)).clone(),
                    maha=E.dev(maha.reshape(N)).clone())

    def _take_by_products(self, by, y, dy, mk):
        n, m, N, lay = self.dim_x, self.dim_z, self._N or 1, self._layout
        K, S, SI = (E.from_records(by[k], lay, 0, s) for k, s in (("K", (n, m)), ("S", (m, m)), ("SI", (m, m))))
        ll, maha = by["ll"].cpu().numpy(), by["maha"].cpu().numpy()
        if y is None:
            y = E.from_records(dy, lay, 0, (m,))
        if self._N is not None:
            if mk is not None:
                y = np.where(mk[:, None], y, np.asarray(self.y, dtype=np.float64).reshape(N, m))
            self.K, self.S, self.SI, self.y = np.array(K), np.array(S), np.array(SI), np.array(y)
            self._log_likelihood, self._mahalanobis = ll.copy(), maha.copy()
            self._likelihood = np.maximum(np.exp(ll), sys.float_info.min)
        else:
            self.K, self.S, self.SI, self.y = K[0].copy(), S[0].copy(), SI[0].copy(), y
            self._log_likelihood, self._mahalanobis = float(ll[0]), float(maha[0])
            self._likelihood = exp(self._log_likelihood) or sys.float_info.min

    def _mask(self, mask, like):
        if mask is None:
            return None, None
        if self._N is None:
            raise ValueError("mask is a bank's keyword: pass n_tracks=N")
        import torch
        mk = np.asarray(mask).astype(bool).reshape(-1)
        if mk.shape != (self._N,):
            raise ValueError(f"mask has shape {np.shape(mask)}, expected ({self._N},)")
        return mk, torch.as_tensor(mk.astype(np.uint8), device=like.device)

    def update(self, z, HJacobian, Hx, R=None, args=(), hx_args=(), residual=np.subtract, mask=None):
        """EKF.py:254-342"""
        if z is None:
            self.z = np.array([[None] * self.dim_z]).T
            self.x_post = self.x.copy()
            self.P_post = self.P.copy()
            return
        args, hx_args = _tuple(args), _tuple(hx_args)
        Rm, flags = self._R(R)
        if np.isscalar(z) and self.dim_z == 1 and self._N is None:
            z = np.asarray([z], float)
        N, lay = self._N or 1, self._layout
        xb = self._xb()
        dx, dP = E.to_records(xb, lay, 0).clone(), E.to_records(self._Pb(), lay, 0).clone()
        mk, dmask = self._mask(mask, dx)
        dH = self._jacobian(HJacobian, args, xb, dx)
        y, dy = self._innovation(z, Hx, hx_args, residual, xb, dx)
        st = status(N, dx)
        by = self._by_products(dx, mk is not None)
        self._dev_update(dx, dP, dH, dy, Rm, flags, st, mask=dmask, by=by)
        E.raise_on_status(st, "ExtendedKalmanFilter.update (S is singular)")
        self._set_state(dx, dP)
        self._take_by_products(by, y, dy, mk)
        self.z = deepcopy(z)
        self.x_post = self.x.copy()
        self.P_post = self.P.copy()

    def predict_update(self, z, HJacobian, Hx, args=(), hx_args=(), u=0):
        """EKF.py:172-252"""
        if z is None:
            raise TypeError("predict_update(None, ...): the reference fails at z - Hx(x) with half of its attributes overwritten; "
                            "call predict() for a step without a measurement")
        args, hx_args = _tuple(args), _tuple(hx_args)
        if np.isscalar(z) and self.dim_z == 1 and self._N is None:
            z = np.asarray([z], float)
        Rm, flags = self._R(None)
        N, lay = self._N or 1, self._layout
        xb = self._xb()
        dx, dP = E.to_records(xb, lay, 0).clone(), E.to_records(self._Pb(), lay, 0).clone()
        dH = self._jacobian(HJacobian, args, xb, dx)           # at the state before the predict (:222)
        x_pre, P_pre = np.copy(self.x), np.copy(self.P)
        st = status(N, dx)
        self._dev_predict(dx, dP, u, st)
        E.raise_on_status(st, "ExtendedKalmanFilter.predict_update")
        xp = E.from_records(dx, lay, 0, (self.dim_x,))
        xp1 = None if self._N is not None else xp[0].reshape(np.shape(self.x)).copy()
        y, dy = self._innovation(z, Hx, hx_args, lambda a, b: a - b, np.ascontiguousarray(xp), dx, x_single=xp1)      # :238
        by = self._by_products(dx, False)
        self._dev_update(dx, dP, dH, dy, Rm, flags, st, by=by)
        E.raise_on_status(st, "ExtendedKalmanFilter.predict_update (S is singular)")
        self.x_prior, self.P_prior = x_pre, P_pre              # the PRE-predict state (:229-230)
        self._set_state(dx, dP)
        self._take_by_products(by, y, dy, None)
        self.z = deepcopy(z)
        self.x_post = self.x.copy()
        self.P_post = self.P.copy()

    # ----------------------------------------------------------------------------------------------------- batch_filter --
    def batch_filter(self, zs, HJacobian, Hx, args=(), hx_args=(), residual=np.subtract, us=None, saver=None,
                     device_outputs=False):
        """predict(us[t]) then update(zs[t]) for t = 0 .. T-1 on a bank; returns (means, covariances, means_p, covariances_p):
        (T, N, n) / (T, N, n, n) NumPy arrays, or with device_outputs=True the device tensors in `layout` ('aos' [T][N][..],
        'soa' [T][..][N])."""
        import torch
        if self._N is None:
            raise ValueError("batch_filter is a bank's method: pass n_tracks=N (use N = 1 for one filter)")
        args, hx_args = _tuple(args), _tuple(hx_args)
        n, m, N, lay = self.dim_x, self.dim_z, self._N, self._layout
        T = len(zs)
        if tuple(np.shape(zs)) != (T, N, m):
            raise ValueError(f"zs has shape {tuple(np.shape(zs))}, expected (T, {N}, {m})")
        if us is not None and len(us) != T:
            raise ValueError("us must have one entry per step")
        u_at = (lambda t: 0) if us is None else (lambda t: us[t])
        fused = (self._mode == "torch" and saver is None and type(self).predict_x is ExtendedKalmanFilter.predict_x)
        if not fused:
            outs = [np.zeros((T, N, n)), np.zeros((T, N, n, n)), np.zeros((T, N, n)), np.zeros((T, N, n, n))]
            for t in range(T):
                self.predict(u_at(t))
                outs[2][t], outs[3][t] = self.x, self.P
                self.update(zs[t], HJacobian, Hx, args=args, hx_args=hx_args, residual=residual)
                outs[0][t], outs[1][t] = self.x, self.P
                if saver is not None:
                    saver.save()
            if device_outputs:
                return tuple(E.to_records(o, lay, 1) for o in outs)
            return tuple(outs)
        dx, dP = E.to_records(self._xb(), lay, 0).clone(), E.to_records(self._Pb(), lay, 0).clone()
        dzs = zs if isinstance(zs, torch.Tensor) else E.dev(np.asarray(zs, dtype=np.float64))
        outs = alloc_histories(T, N, n, lay)
        if T:
            Rm, flags = self._R(None)
            st, stt = status(N, dx), status(N, dx)
            # F, Q, R, B go up once (the attributes as they stand now hold for all T steps), and so does a (T, N, dim_u) array
            # of controls.  Per step the loop then adds to the launches only the callables and ONE device copy of x and P into
            # the prior histories: the kernels work on x and P in place, so the prior a step leaves is copied out before the
            # next launch overwrites it (the posterior history is written by the fused launch itself).
            if us is not None and not isinstance(us, torch.Tensor) and np.ndim(us) == 3 and np.shape(us)[:2] == (T, N):
                dus = E.dev(np.asarray(us, dtype=np.float64))
                u_at = lambda t: dus[t]                      # noqa: E731
            self._resident = {}
            try:
                by, dy = self._fused_steps(T, dx, dP, dzs, outs, u_at, Rm, flags, st, stt, HJacobian, Hx, args, hx_args, residual)
            finally:
                self._resident = None
            E.raise_on_status(st, "ExtendedKalmanFilter.batch_filter (S is singular)")
            self._set_state(dx, dP)
            self._take_by_products(by, None, dy, None)
            self.x_prior = np.array(E.from_records(outs[2][T - 1], lay, 0, (n,)))
            self.P_prior = np.array(E.from_records(outs[3][T - 1], lay, 0, (n, n)))
            self.x_post, self.P_post = self.x.copy(), self.P.copy()
            zl = zs[T - 1]
            self.z = zl.cpu().numpy() if isinstance(zl, torch.Tensor) else deepcopy(zl)
        if device_outputs:
            return tuple(outs)
        return host_histories(outs, n, lay)

    def _fused_steps(self, T, dx, dP, dzs, outs, u_at, Rm, flags, st, stt, HJacobian, Hx, args, hx_args, residual):
        """one fk_ekf_predict_f64, T - 1 fk_ekf_step_f64, one fk_ekf_update_f64 on resident records -> the last update's
        by-product and innovation records"""
        by, dy = None, None
        self._dev_predict(dx, dP, u_at(0), st)
        for t in range(T):
            outs[2][t].copy_(dx.reshape(outs[2][t].shape))
            outs[3][t].copy_(dP.reshape(outs[3][t].shape))
            dH = self._jacobian(HJacobian, args, None, dx)
            _, dy = self._innovation(dzs[t], Hx, hx_args, residual, None, dx)
            if t < T - 1:
                self._dev_update(dx, dP, dH, dy, Rm, flags, stt, step=dict(u=u_at(t + 1), x_post=outs[0][t], P_post=outs[1][t]))
            else:
                by = self._by_products(dx, False)
                self._dev_update(dx, dP, dH, dy, Rm, flags, stt, by=by)
                outs[0][t].copy_(dx.reshape(outs[0][t].shape))
                outs[1][t].copy_(dP.reshape(outs[1][t].shape))
            st.bitwise_or_(stt)
        return by, dy

    # ------------------------------------------------------------------------------------------------- the lazy scalars --
    @property
    def log_likelihood(self):
        """log-likelihood of the last measurement (:373-381); per track for a bank"""
        return self._log_likelihood

    @property
    def likelihood(self):
        """likelihood of the last measurement, never below sys.float_info.min (:383-396)"""
        return self._likelihood

    @property
    def mahalanobis(self):
        """Mahalanobis distance of the innovation (:398-410)"""
        if self._mahalanobis is None:
            y, SI = np.asarray(self.y, dtype=np.float64), np.asarray(self.SI, dtype=np.float64)
            if self._N is None:
                return 0.0 if not SI.any() else float(np.sqrt(y.reshape(1, -1) @ SI @ y.reshape(-1, 1)).item())
            return np.zeros(self._N)
        return self._mahalanobis

    def __repr__(self):
        return "\n".join(["ExtendedKalmanFilter object (filterpy_amd, gfx950)"] +
                         [f"{k} = {v!r}" for k, v in
                          (("dim_x", self.dim_x), ("dim_z", self.dim_z), ("dim_u", self.dim_u), ("x", self.x), ("P", self.P),
                           ("x_prior", self.x_prior), ("P_prior", self.P_prior), ("F", self.F), ("Q", self.Q), ("R", self.R),
                           ("K", self.K), ("y", self.y), ("S", self.S), ("likelihood", self.likelihood),
                           ("log-likelihood", self.log_likelihood), ("mahalanobis", self.mahalanobis))])
