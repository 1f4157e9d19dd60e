"""Cubature Kalman filter with filterpy's call surface, arithmetic on the GPU.

Mirrors rlabbe/filterpy v1.4.5 filterpy/kalman/CubatureKalmanFilter.py:

    spherical_radial_sigmas (:32-61)   ckf_transform (:64-98)   CubatureKalmanFilter.__init__ (:240-290)
    predict (:292-327)   update (:329-390)   log_likelihood / likelihood / mahalanobis (:392-428)   __repr__ (:430-445)

The cubature filter is not a UKF with other weights: 2n points x +- sqrt(n) U[k] and no centre point, the Cholesky factor
scaled AFTER factoring (:56), an uncentred second moment sum (X X' - x x') / k + Q (:92-96) -- and update() draws no new
points from the predicted P: it pushes the points predict() left in sigmas_f through hx (:362-363), so Q never reaches Pxz or
S.  All of that is kept (the kernels sum centred terms: the same numbers without the cancellation, csrc/fk_ckf.hpp).

Four ways to run it, chosen like UnscentedKalmanFilter's:

* fx / hx Python callables, once per point like the reference (:320-321, :362-363): the points (fk_ckf_sigma_points_f64),
  the transform (fk_ckf_transform_f64) and the whole update -- zp, S, SI, Pxz, K, y, x, P in ONE launch, fk_ckf_update_f64 --
  are gfx950 kernels, the callables run on the host between them;
* ``vectorized=True``: the callables run once per call on NumPy arrays, fx(sigmas (N, 2n, n), dt, *fx_args) -> (N, 2n, n),
  hx(sigmas (N, 2n, n), *hx_args) -> (N, 2n, m), residual_z(z (N, m), zp (N, m)) -> (N, m);
* ``device_callables=True`` (banks only): the same shapes on float64 CUDA tensors; in batch_filter() the state, the points
  and the histories stay in HBM for all T steps (predict() / update() hand x, P, sigmas_f and the by-products back to the
  host attributes after every call, like UnscentedKalmanFilter's);
* ``fx=F, hx=H`` NumPy arrays: the fused kernels fk_ckf_linear_predict_f64 / fk_ckf_linear_update_f64, and batch_filter runs
  the whole time loop in ONE launch (fk_ckf_linear_batch_f64).  The points predict() leaves are then held as the centre F x and
  the n half-differences F U[k]; ``sigmas_f`` / ``sigmas_h`` are materialised from them when read.

``n_tracks=N`` turns the object into a bank of N independent filters: x (N, n), P (N, n, n), z (N, m), zs (T, N, m), sigmas_f
(N, 2n, n), K (N, n, m), y (N, m).  ``batch_filter(zs, Rs=None, saver=None, device_outputs=False)`` (the reference has none)
returns (means, covariances, means_p, covariances_p) and leaves the filter where the step loop would, except that the fused
launch does not produce K, y, S and SI of the last update (they keep their values).

Kept from the reference: x becomes an (n, 1) column at the first predict() whatever it was (:89, :323); update(None) only copies
the posts (:348-352); a scalar R means eye * R (:359-360); the likelihoods are lazy; x_mean_fn, z_mean_fn and residual_x are
stored (as x_mean, z_mean, residual_x, :257-267) and NEVER called -- only residual_z is (:376).  Divergences:
  * the reference raises for a 1-D z when dim_z > 1 ((m,) - (m, 1) broadcasts); here (m,) and (m, 1) are the same measurement;
  * a P that is not positive definite raises numpy.linalg.LinAlgError (the reference's cholesky raises the same); so does an S
    with a non-positive pivot;
  * update() with a 1-D x and dim_x > 1 (possible only before the first predict) raises ValueError: the reference's
    x + dot(K, y) broadcasts it into an (n, n) matrix;
  * P and R are symmetric: P's upper and R's lower triangle are read.
"""
import sys
from copy import deepcopy
from math import exp, log, sqrt

import numpy as np

from .. import _engine as E
from ..common.helpers import logpdf
from ._bank import _desc
from ._callable import _CallableHost, alloc_histories, as_records, host_histories, status, to_rec

__all__ = ["CubatureKalmanFilter", "spherical_radial_sigmas", "ckf_transform"]


def spherical_radial_sigmas(x, P):
    """CubatureKalmanFilter.py:32-61: the 2n cubature points of (x, P), (2n, n) -- or (N, 2n, n) for x (N, n), P (N, n, n)"""
    P = np.asarray(P, dtype=np.float64)
    n = P.shape[-1]
    bank = P.ndim == 3
    Pb = P.reshape(-1, n, n)
    N = Pb.shape[0]
    xb = np.broadcast_to(np.asarray(x, dtype=np.float64).reshape(-1, n), (N, n))
    dx, dP = E.to_records(xb, "aos", 0), E.to_records(Pb, "aos", 0)
    sig, st = E.alloc_records((), N, 2 * n * n, "aos"), status(N, dx)
    E.ckf_sigma_points(n, N, "aos", dx, dP, sig, st)
    E.raise_on_status(st, "spherical_radial_sigmas")
    out = E.from_records(sig, "aos", 0, (2 * n, n))
    return out if bank else out[0]


def ckf_transform(Xs, Q):
    """CubatureKalmanFilter.py:64-98: mean (d, 1) and covariance (d, d) of the points Xs (k, d) -- or (N, d) and (N, d, d) for
    Xs (N, k, d)"""
    Xs = np.asarray(Xs, dtype=np.float64)
    bank = Xs.ndim == 3
    Xb = Xs if bank else Xs[None]
    N, k, d = Xb.shape
    ds = E.to_records(Xb, "aos", 0)
    xo, Po = E.alloc_records((), N, d, "aos"), E.alloc_records((), N, d * d, "aos")
    E.ckf_transform(d, k, N, "aos", ds, None if Q is None else E.dev(np.broadcast_to(np.asarray(Q, dtype=np.float64), (d, d)).copy()),
                    xo, Po)
    x, P = E.from_records(xo, "aos", 0, (d,)), E.from_records(Po, "aos", 0, (d, d))
    return (x, P) if bank else (x[0].reshape(d, 1), P[0])


class CubatureKalmanFilter(_CallableHost):
    """filterpy.kalman.CubatureKalmanFilter (CubatureKalmanFilter.py:101-445) on the GPU: same attributes, defaults and results."""

    def __init__(self, dim_x, dim_z, dt, hx, fx, x_mean_fn=None, z_mean_fn=None, residual_x=None, residual_z=None,
                 n_tracks=None, vectorized=False, layout="soa", device_callables=False):
        self._preamble(n_tracks, vectorized, device_callables, layout, dims=(dim_x, dim_z))
        lead = () if n_tracks is None else (n_tracks,)
        self.Q = np.eye(dim_x)
        self.R = np.eye(dim_z)
        self.x = np.zeros(lead + (dim_x,))
        self.P = np.eye(dim_x) if n_tracks is None else np.tile(np.eye(dim_x), (n_tracks, 1, 1))
        self.K = 0
        self.dim_x = dim_x
        self.dim_z = dim_z
        self._dt = dt
        self._num_sigmas = 2 * dim_x
        self.hx = hx
        self.fx = fx
        self.x_mean = x_mean_fn                 # stored, never called: CubatureKalmanFilter.py:257-258
        self.z_mean = z_mean_fn
        self.y = 0
        self.z = np.array([[None] * dim_z]).T
        self.S = np.zeros(lead + (dim_z, dim_z))
        self.SI = np.zeros(lead + (dim_z, dim_z))
        self.residual_x = np.subtract if residual_x is None else residual_x     # stored, never called: :264-267
        self.residual_z = np.subtract if residual_z is None else residual_z
        self._sf = np.zeros(lead + (2 * dim_x, dim_x))       # sigmas_f as an array, or None: read off _pts
        self._sh = np.zeros(lead + (2 * dim_x, dim_z))
        self._pts = None                                      # matrix model: (N, n + n*n), centre and half-differences
        self._log_likelihood = log(sys.float_info.min)
        self._likelihood = sys.float_info.min
        self._mahalanobis = None
        self.x_prior = self.x.copy()
        self.P_prior = self.P.copy()
        self.x_post = self.x.copy()
        self.P_post = self.P.copy()

    # ---------------------------------------------------------------------------------------------------------- helpers --
    @property
    def _linear(self):
        """fx and hx were handed over as matrices"""
        return (not callable(self.fx)) and (not callable(self.hx))

    def _noise(self, A, k, name):
        M = np.asarray(A, dtype=np.float64)
        if M.ndim == 0:
            raise ValueError(f"{name} must be a ({k}, {k}) matrix")
        try:
            return np.ascontiguousarray(np.broadcast_to(M, (k, k)))
        except ValueError:
            raise ValueError(f"{name} has shape {M.shape}, expected ({k}, {k})") from None

    def _R(self, R):
        """update()'s R: None -> the attribute, a scalar -> eye * R (:357-360)"""
        m = self.dim_z
        if R is None:
            R = self.R
        elif np.isscalar(R):
            R = np.eye(m) * R
        return self._noise(R, m, "R")

    def _zb(self, z):
        """one measurement -> (N, m); (m,), (m, 1) and for dim_z 1 a scalar are the same measurement"""
        m, N = self.dim_z, self._N or 1
        za = np.asarray(z, dtype=np.float64)
        ok = za.shape == (N, m) if self._N is not None else (za.shape in ((m,), (m, 1)) or (m == 1 and za.ndim == 0))
        if not ok:
            raise ValueError(f"measurement of shape {za.shape}, expected " +
                             (f"({N}, {m})" if self._N is not None else f"({m},) or ({m}, 1)"))
        return np.ascontiguousarray(za.reshape(N, m))

    def _matrix(self, M, r, c, name):
        A = np.asarray(M, dtype=np.float64)
        if A.shape != (r, c):
            raise ValueError(f"{name} has shape {A.shape}, expected ({r}, {c})")
        return np.ascontiguousarray(A)

    def _to_rec(self, t, k, d):
        """(N, k, d) as a callable returned it (torch tensor or array) -> device records in the bank's layout"""
        return to_rec(t, self._N or 1, (k, d), self._layout, self._mode == "torch")

    def _by_products(self):
        """records for the y, K, S and SI of one update"""
        n, m, N, lay = self.dim_x, self.dim_z, self._N or 1, self._layout
        return dict(y=E.alloc_records((), N, m, lay), K=E.alloc_records((), N, n * m, lay), S=E.alloc_records((), N, m * m, lay),
                    SI=E.alloc_records((), N, m * m, lay))

    def _user(self, fn, sig, d_out, *args):
        """fx / hx on the points sig, a (N, k, d) device view, in the mode's calling convention -> records (N, k, d_out)"""
        N, k, d_in = sig.shape
        if not callable(fn):                                   # a matrix next to a callable: one kernel (fk_ut_linear_map_f64)
            M = self._matrix(fn, d_out, d_in, "the model matrix")
            out = E.alloc_records((), N, k * d_out, self._layout)
            E.ut_linear_map(d_in, d_out, k, N, self._layout, E.dev(M), as_records(sig, N, self._layout), out)
            return out
        if self._mode == "torch":
            return self._to_rec(fn(sig, *args), k, d_out)
        s = sig.cpu().numpy()
        if self._mode == "vec":
            return self._to_rec(fn(s, *args), k, d_out)
        out = [[np.ravel(fn(p, *args)) for p in trk] for trk in s]
        return self._to_rec(np.asarray(out, dtype=np.float64).reshape(N, k, -1), k, d_out)

    def _residual(self, dz, zp):
        """residual_z(z, zp) on device records (N, m) -> records; per track on (m, 1) columns like the reference (:376) in the
        default mode, once on (N, m) arrays / tensors otherwise"""
        m, N = self.dim_z, self._N or 1
        zv, pv = self._rec_view(dz, 1, m)[:, 0, :], self._rec_view(zp, 1, m)[:, 0, :]
        if self._mode == "torch":
            y = self.residual_z(zv, pv)
            return self._to_rec(y.reshape(N, 1, m), 1, m).reshape(dz.shape)
        zn, pn = zv.cpu().numpy(), pv.cpu().numpy()
        if self._mode == "vec":
            y = np.asarray(self.residual_z(zn, pn), dtype=np.float64)
        else:
            y = np.array([np.ravel(self.residual_z(zn[i].reshape(m, 1).copy(), pn[i].reshape(m, 1).copy())) for i in range(N)])
        return self._to_rec(y.reshape(N, 1, m), 1, m).reshape(dz.shape)

    # ------------------------------------------------------------------------------------- the points predict() leaves --
    @property
    def sigmas_f(self):
        """the points predict() left, (2n, n) / (N, 2n, n); on a matrix model materialised from the centre and the
        half-differences the kernel keeps: c + sqrt(n) E[k], c - sqrt(n) E[k]"""
        if self._sf is None:
            n = self.dim_x
            c, Eh = self._pts[:, None, :n], self._pts[:, n:].reshape(-1, n, n) * sqrt(n)
            self._sf = self._unb(np.concatenate([c + Eh, c - Eh], axis=1))
        return self._sf

    @sigmas_f.setter
    def sigmas_f(self, value):
        self._sf = value
        self._pts = None

    @property
    def sigmas_h(self):
        """the points update() pushed through hx; on a matrix model sigmas_f H'"""
        if self._sh is None:
            self._sh = np.asarray(self.sigmas_f) @ self._matrix(self.hx, self.dim_z, self.dim_x, "hx").T
        return self._sh

    @sigmas_h.setter
    def sigmas_h(self, value):
        self._sh = value

    def _points_records(self):
        """the matrix model's points record (N, n + n*n) on the host; read off sigmas_f where that was assigned"""
        n, N = self.dim_x, self._N or 1
        if self._pts is None:
            s = np.asarray(self._sf, dtype=np.float64).reshape(N, 2 * n, n)
            # every +- pair's midpoint is the centre; points that are no +- pairs about one centre have no such record
            mid, Eh = (s[:, :n] + s[:, n:]) / 2, (s[:, :n] - s[:, n:]) / (2 * sqrt(n))
            c = mid.mean(axis=1)
            if not np.allclose(mid, c[:, None, :], rtol=1e-9, atol=1e-9 * max(1.0, float(np.abs(s).max()))):
                raise ValueError("sigmas_f was assigned points that are not +- pairs about one centre: the matrix model's update "
                                 "reads them as a centre and n half-differences (use callables for fx / hx instead)")
            self._pts = np.concatenate([c, Eh.reshape(N, n * n)], axis=1)
        return self._pts

    # ------------------------------------------------------------------------------------------------ device-side steps --
    def _dev_predict(self, dx, dP, dQ, dt, st, fx_args):
        """:317-323 on device records -> the propagated points (records)"""
        n, N, lay = self.dim_x, self._N or 1, self._layout
        sig = E.alloc_records((), N, 2 * n * n, lay)
        E.ckf_sigma_points(n, N, lay, dx, dP, sig, st)
        sf = self._user(self.fx, self._rec_view(sig, 2 * n, n), n, dt, *fx_args) if callable(self.fx) else \
            self._user(self.fx, self._rec_view(sig, 2 * n, n), n)
        E.ckf_transform(n, 2 * n, N, lay, sf, dQ, dx, dP)
        return sf

    def _dev_update(self, dx, dP, sf, dz, dR, st, hx_args, by=None):
        """:362-379 on device records; by: dict of by-product records to fill (zp, S, SI, K, y) -> sigmas_h records"""
        n, m, N, lay = self.dim_x, self.dim_z, self._N or 1, self._layout
        by = by or {}
        sh = self._user(self.hx, self._rec_view(sf, 2 * n, n), m, *hx_args)
        if self.residual_z is np.subtract:
            zp = by.get("zp")
            if zp is None:
                zp = E.alloc_records((), N, m, lay)
            E.ckf_update(n, m, N, lay, sf, sh, dR, dz, dx, dP, zp=zp, S=by.get("S"), SI=by.get("SI"), K=by.get("K"), y=by.get("y"),
                         status=st)
        else:                                                  # y = residual_z(z, zp) is the caller's: zp first, then the rest
            zp, S0 = E.alloc_records((), N, m, lay), E.alloc_records((), N, m * m, lay)
            E.ckf_transform(m, 2 * n, N, lay, sh, dR, zp, S0)
            dy = self._residual(dz, zp)
            E.ckf_update(n, m, N, lay, sf, sh, dR, dy, dx, dP, zp=None, S=by.get("S"), SI=by.get("SI"), K=by.get("K"),
                         y=by.get("y"), status=st)
        return sh

    # ---------------------------------------------------------------------------------------------------------- predict --
    def predict(self, dt=None, fx_args=()):
        """CubatureKalmanFilter.py:292-327"""
        if dt is None:
            dt = self._dt
        if not isinstance(fx_args, tuple):
            fx_args = (fx_args,)
        n, N, lay = self.dim_x, self._N or 1, self._layout
        dQ = E.dev(self._noise(self.Q, n, "Q"))
        dx, dP = E.to_records(self._xb(), lay, 0).clone(), E.to_records(self._Pb(), lay, 0).clone()
        st = status(N, dx)
        if self._linear:
            F = self._matrix(self.fx, n, n, "fx")
            pts = E.alloc_records((), N, n + n * n, lay)
            pts.zero_()
            E.ckf_linear_predict(_desc(n, self.dim_z, 0, N, 1, lay), E.dev(F), dQ, dx, dP, pts, status=st)
            E.raise_on_status(st, "CubatureKalmanFilter.predict (P is not positive definite)")
            self._pts, self._sf = E.from_records(pts, lay, 0, (n + n * n,)), None
        else:
            sf = self._dev_predict(dx, dP, dQ, dt, st, fx_args)
            E.raise_on_status(st, "CubatureKalmanFilter.predict (P is not positive definite)")
            self.sigmas_f = self._unb(E.from_records(sf, lay, 0, (2 * n, n)))
        x, P = E.from_records(dx, lay, 0, (n,)), E.from_records(dP, lay, 0, (n, n))
        self.x = x if self._N is not None else x[0].reshape(n, 1)            # a column from here on: :89, :323
        self.P = self._unb(P)
        self.x_prior = self.x.copy()
        self.P_prior = self.P.copy()

    # ----------------------------------------------------------------------------------------------------------- update --
    def update(self, z, R=None, hx_args=()):
        """CubatureKalmanFilter.py:329-390"""
        if z is None:
            self.z = np.array([[None] * self.dim_z]).T
            self.x_post = self.x.copy()
            self.P_post = self.P.copy()
            return
        if not isinstance(hx_args, tuple):
            hx_args = (hx_args,)
        n, m, N, lay = self.dim_x, self.dim_z, self._N or 1, self._layout
        Rm = self._R(R)
        zb, xb = self._zb(z), self._xb()
        if self._N is None and np.ndim(self.x) == 1 and n > 1:
            raise ValueError("update() with a 1-D x: the reference's x + dot(K, y) broadcasts it into an (n, n) matrix; "
                             "make x an (n, 1) column (predict() does)")
        dx, dP = E.to_records(xb, lay, 0).clone(), E.to_records(self._Pb(), lay, 0).clone()
        dz, dR = E.to_records(zb, lay, 0), E.dev(Rm)
        st = status(N, dx)
        by = self._by_products()
        if self._linear:
            H =self._matrix(self.hx, m, n, "hx")
            pts = E.to_records(self._points_records(), lay, 0)
            E.ckf_linear_update(_desc(n, m, 0, N, 1, lay), E.dev(H), dR, dz, dx, dP, pts, status=st, **by)
            self._sh = None
        else:
            sf = E.to_records(np.asarray(self.sigmas_f, dtype=np.float64).reshape(N, 2 * n, n), lay, 0)
            sh = self._dev_update(dx, dP, sf, dz, dR, st, hx_args, by)
            self.sigmas_h = self._unb(E.from_records(sh, lay, 0, (2 * n, m)))
        E.raise_on_status(st, "CubatureKalmanFilter.update (S is singular)")
        self.S = self._unb(E.from_records(by["S"], lay, 0, (m, m)))
        self.SI = self._unb(E.from_records(by["SI"], lay, 0, (m, m)))
        self.K = self._unb(E.from_records(by["K"], lay, 0, (n, m)))
        y, x = E.from_records(by["y"], lay, 0, (m,)), E.from_records(dx, lay, 0, (n,))
        self.y = y if self._N is not None else y[0].reshape(m, 1)
        self.x = x if self._N is not None else x[0].reshape(n, 1)
        self.P = self._unb(E.from_records(dP, lay, 0, (n, n)))
        self.z = deepcopy(z)
        self.x_post = self.x.copy()
        self.P_post = self.P.copy()
        self._log_likelihood = None
        self._likelihood = None
        self._mahalanobis = None

    # ----------------------------------------------------------------------------------------------------- batch_filter --
    def batch_filter(self, zs, Rs=None, saver=None, device_outputs=False):
        """predict() then update(z) for every z of zs (None: no measurement at that step); the reference has no batch_filter.
        Returns (means, covariances, means_p, covariances_p): (T, n) and (T, n, n) NumPy arrays ((T, N, ..) for a bank), or with
        device_outputs=True the device tensors in `layout` ('aos' [T][N][..], 'soa' [T][..][N]).  On a matrix model with
        Rs = None and no saver the whole loop is ONE launch (fk_ckf_linear_batch_f64); otherwise a step loop with the state, the
        points and the histories resident on the device (Rs[t]: that step's R, a matrix or a scalar)."""
        import torch
        n, m, N, lay = self.dim_x, self.dim_z, self._N or 1, self._layout
        try:
            T = len(zs)
        except TypeError:
            raise TypeError("zs must be list-like") from None
        if Rs is not None and len(Rs) != T:
            raise ValueError("Rs must have one entry per measurement")
        present = np.array([z is not None for z in zs], dtype=bool)
        zarr = np.zeros((T, N, m))
        for t, z in enumerate(zs):
            if z is not None:
                zarr[t] = self._zb(z)
        dQ = E.dev(self._noise(self.Q, n, "Q"))
        dx, dP = E.to_records(self._xb(), lay, 0).clone(), E.to_records(self._Pb(), lay, 0).clone()
        dzs = E.to_records(zarr, lay, 1)
        st = status(N, dx)
        outs = alloc_histories(T, N, n, lay)
        fused = self._linear and Rs is None and saver is None
        if fused:
            F, H = self._matrix(self.fx, n, n, "fx"), self._matrix(self.hx, m, n, "hx")
            pts = E.to_records(self._points_records(), lay, 0).clone()
            mask = None if present.all() else torch.as_tensor(np.repeat(present[:, None], N, axis=1).astype(np.uint8), device=dx.device)
            if T:
                E.ckf_linear_batch(_desc(n, m, 0, N, T, lay), E.dev(F), dQ, E.dev(H), E.dev(self._R(None)), dzs, dx, dP, pts,
                                   mask=mask, means=outs[0], covs=outs[1], means_p=outs[2], covs_p=outs[3], status=st)
                E.raise_on_status(st, "CubatureKalmanFilter.batch_filter (P is not positive definite)")
                self._pts, self._sf, self._sh = E.from_records(pts, lay, 0, (n + n * n,)), None, None
        elif saver is not None or self._linear:
            # the step loop through predict() / update(): every attribute is the object's own after each step
            for t in range(T):
                self.predict()
                self.update(zs[t], R=None if Rs is None else Rs[t])
                dx, dP = E.to_records(self._xb(), lay, 0), E.to_records(self._Pb(), lay, 0)
                xp_, Pp_ = np.asarray(self.x_prior).reshape(N, n), np.asarray(self.P_prior).reshape(N, n, n)
                for o, v in zip(outs, (dx, dP, E.to_records(xp_, lay, 0), E.to_records(Pp_, lay, 0))):
                    o[t].copy_(v.reshape(o[t].shape))
                if saver is not None:
                    saver.save()
        else:
            sf, last = None, None
            last_upd = max([t for t in range(T) if present[t]], default=-1)
            stt = status(N, dx)                              # each kernel writes its own status: OR them over the steps
            for t in range(T):
                sf = self._dev_predict(dx, dP, dQ, self._dt, stt, ())
                st.bitwise_or_(stt)
                outs[2][t].copy_(dx.reshape(outs[2][t].shape))
                outs[3][t].copy_(dP.reshape(outs[3][t].shape))
                if present[t]:
                    by = self._by_products() if t == last_upd else None   # (what the step loop would leave on the object)
                    sh = self._dev_update(dx, dP, sf, dzs[t], E.dev(self._R(None if Rs is None else Rs[t])), stt, (), by)
                    st.bitwise_or_(stt)
                    if by is not None:
                        last = (by, sh)
                outs[0][t].copy_(dx.reshape(outs[0][t].shape))
                outs[1][t].copy_(dP.reshape(outs[1][t].shape))
            E.raise_on_status(st, "CubatureKalmanFilter.batch_filter (P is not positive definite)")
            if T:
                self.sigmas_f = self._unb(E.from_records(sf, lay, 0, (2 * n, n)))
            if last is not None:
                by, sh = last
                self.sigmas_h = self._unb(E.from_records(sh, lay, 0, (2 * n, m)))
                self.S, self.SI = (self._unb(E.from_records(by[k], lay, 0, (m, m))) for k in ("S", "SI"))
                self.K = self._unb(E.from_records(by["K"], lay, 0, (n, m)))
                y = E.from_records(by["y"], lay, 0, (m,))
                self.y = y if self._N is not None else y[0].reshape(m, 1)
                self._log_likelihood = self._likelihood = self._mahalanobis = None
        if T and (fused or not (saver is not None or self._linear)):
            x, P = E.from_records(dx, lay, 0, (n,)), E.from_records(dP, lay, 0, (n, n))
            self.x = x if self._N is not None else x[0].reshape(n, 1)
            self.P = self._unb(P)
            xp_, Pp_ = E.from_records(outs[2][T - 1], lay, 0, (n,)), E.from_records(outs[3][T - 1], lay, 0, (n, n))
            self.x_prior = xp_ if self._N is not None else xp_[0].reshape(n, 1)
            self.P_prior = self._unb(Pp_)
            self.x_post, self.P_post = self.x.copy(), self.P.copy()
            self.z = deepcopy(zs[T - 1]) if present[T - 1] else np.array([[None] * m]).T
        if device_outputs:
            return tuple(outs)
        res = host_histories(outs, n, lay)
        return res if self._N is not None else tuple(r[:, 0] for r in res)

    # ------------------------------------------------------------------------------------------------- the lazy scalars --
    @property
    def log_likelihood(self):
        """log-likelihood of the last measurement (:392-399); per track for a bank"""
        if self._log_likelihood is None:
            if self._N is None:
                self._log_likelihood = logpdf(x=self.y, cov=self.S)
            else:
                self._log_likelihood = np.array([logpdf(x=self.y[i], cov=self.S[i]) for i in range(self._N)])
        return self._log_likelihood

    @property
    def likelihood(self):
        """likelihood of the last measurement, never below sys.float_info.min (:401-414)"""
        if self._likelihood is None:
            if self._N is None:
                self._likelihood = exp(self.log_likelihood)
                if self._likelihood == 0:
                    self._likelihood = sys.float_info.min
            else:
                self._likelihood = np.maximum(np.exp(self.log_likelihood), sys.float_info.min)
        return self._likelihood

    @property
    def mahalanobis(self):
        """Mahalanobis distance of the innovation (:416-428)"""
        if self._mahalanobis is None:
            y, SI = np.asarray(self.y, dtype=np.float64), np.asarray(self.SI, dtype=np.float64)
            if self._N is None:
                y = y.reshape(-1, 1) if y.ndim else np.zeros((self.dim_z, 1))
                self._mahalanobis = sqrt(float((y.T @ SI @ y).item()))
            else:
                self._mahalanobis = np.sqrt(np.einsum("ni,nij,nj->n", y, SI, y))
        return self._mahalanobis

    def __repr__(self):
        return "\n".join(["CubatureKalmanFilter object (filterpy_amd, gfx950)"] +
                         [f"{k} = {v!r}" for k, v in
                          (("dim_x", self.dim_x), ("dim_z", self.dim_z), ("dt", self._dt), ("x", self.x), ("P", self.P),
                           ("Q", self.Q), ("R", self.R), ("K", self.K), ("y", self.y), ("log-likelihood", self.log_likelihood),
                           ("likelihood", self.likelihood), ("mahalanobis", self.mahalanobis))])
