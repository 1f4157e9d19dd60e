"""Ensemble Kalman filter with filterpy's call surface, its ensemble resident on the GPU and reduced by the gfx950 kernels.

Mirrors rlabbe/filterpy v1.4.5 filterpy/kalman/ensemble_kalman_filter.py:

    EnsembleKalmanFilter.__init__ (:158-185)  initialize (:187-216)  update (:218-273)  predict (:275-290)  __repr__ (:292-309)

The reference calls itself "a toy as it is far too slow with large N": a Python loop over the N members and three
outer_product_sum passes per step.  Here the ensemble lives in device memory as records in `layout` ('soa': [dim_x][N],
member-minor and lane-coalesced; 'aos': NumPy order [N][dim_x]); each predict() / update() is a short chain of launches on the
current stream (fk_enkf_predict_f64: two, fk_enkf_update_f64: four; include/filterhip.h) that streams the members, adds the
means and covariances up in a fixed order (csrc/fk_enkf.hpp) and leaves x, P, K, S, SI -- small -- as NumPy arrays.

fx / hx come in three forms, with UKF.py's conventions:
  * Python callables (the default), called per member like the reference, or once on the whole (N, dim_x) NumPy array with
    vectorized=True.  The ensemble crosses to the host and back around the callable; everything after it runs on the GPU;
  * matrices (fx=F, hx=H as NumPy arrays): the fused path.  F s and H s are formed in-lane, no sigmas_h array exists and the
    ensemble never leaves device memory;
  * device_callables=True: fx(sigmas (N, dim_x), dt) -> (N, dim_x) and hx(sigmas (N, dim_x)) -> (N, dim_z) on float64 GPU
    tensors.  Nothing leaves device memory.

The filter is stochastic; the draws are INPUTS of the kernels.  `noise` says where the three draws of a cycle come from
(initialize: (x, P); predict: (0, Q); update: (0, R)):
  * "numpy" (the default): numpy.random.multivariate_normal(mean, cov, N) on the host, with the reference's arguments and in the
    reference's order -- in predict after all fx calls, in update after all hx calls -- so the same numpy.random.seed gives the
    reference's stream.  The draws are uploaded and added as they are;
  * a callable noise(mean, cov, N) -> (N, d) array or GPU tensor: the same call sites;
  * "device": standard normals from torch.randn on the GPU (generator= is passed through), multiplied in-lane by the d x d factor
    sqrt(s)[:, None] * v of numpy.linalg.svd(cov) -- the factorisation numpy.random.multivariate_normal itself uses, computed on
    the host, so a singular Q such as Q_discrete_white_noise works.  No N x d array of correlated noise is ever stored.

The reference's semantics are kept, quirks included: initialize keeps the given x and P, not the sample statistics; update
centres the members on self.x as it stands and sigmas_h on their own mean; P = P - K S K' uses the stored P; update(None) only
records z = None and the posterior copies; a scalar R argument means eye(dim_z) * R; x.ndim != 1 raises ValueError.
Divergences:
  * `sigmas` is a property: reading downloads an (N, dim_x) array and caches it until the next step, assigning uploads.
    In-place edits of the returned array (f.sigmas[3] += 1) are NOT seen by the filter: assign the array back.  `sigmas_device`
    is the tensor itself (in `layout`);
  * N < 2 raises ValueError (the reference divides by N - 1);
  * inv other than numpy.linalg.inv raises NotImplementedError on update() (the device inverts), as InformationFilter does;
  * S not positive definite -- a pivot of its L D L' at or below dim_z eps max|diag S| -- raises numpy.linalg.LinAlgError; the
    reference inverts whatever it gets;
  * dim_x > 16 or dim_z > 8 is refused (the kernels' compiled range);
  * the sums are taken in the kernels' order and every second moment is a one-pass sum of pivot-shifted products: x, P, K, S
    and the members agree with the reference to rounding (1e-10 relative at a mean 1e3 spreads away from 0; against a longdouble
    truth, within 5 x the reference's own error at a mean 1e4 spreads away and on stiff models: docs/MEASUREMENTS.md,
    "EnKF precision").
Out of scope: a bank of several ensembles (n_tracks); a one-launch batch_filter -- it would need workgroups to wait for each
other inside a launch, and a step is already a short chain of launches on the caller's stream; multi-GPU.
"""
from copy import deepcopy

import numpy as np

from .. import _engine as E
from ._bank import _desc

__all__ = ["EnsembleKalmanFilter"]


def _factor(cov):
    """the d x d matrix A with e = w @ A ~ N(0, cov) for standard normal w: numpy.random.multivariate_normal's own"""
    _, s, v = np.linalg.svd(np.asarray(cov, dtype=np.float64))
    return np.ascontiguousarray(np.sqrt(s)[:, None] * v)


class EnsembleKalmanFilter(object):
    """filterpy.kalman.EnsembleKalmanFilter (ensemble_kalman_filter.py:36-309) on the GPU: same attributes and defaults."""

    def __init__(self, x, P, dim_z, dt, N, hx, fx, *, noise="numpy", vectorized=False, device_callables=False, layout="soa",
                 generator=None):
        if dim_z <= 0:
            raise ValueError('dim_z must be greater than zero')
        if N < 2:
            raise ValueError('N must be at least 2 (the covariances divide by N - 1)')
        if layout not in E.LAYOUTS:
            raise ValueError(f"layout must be one of {sorted(E.LAYOUTS)}")
        if not (noise in ("numpy", "device") or callable(noise)):
            raise ValueError('noise must be "numpy", "device" or a callable (mean, cov, N) -> (N, d)')
        dim_x = len(x)
        if dim_x > 16 or dim_z > 8:
            raise NotImplementedError("dim_x/dim_z outside the compiled range (dim_x <= 16, dim_z <= 8)")
        self.dim_x = dim_x
        self.dim_z = dim_z
        self.dt = dt
        self.N = N
        self.hx = hx
        self.fx = fx
        self.noise = noise
        self.vectorized = vectorized
        self.device_callables = device_callables
        self.layout = layout
        self.generator = generator
        self.K = np.zeros((dim_x, dim_z))
        self.z = np.array([[None] * self.dim_z]).T
        self.S = np.zeros((dim_z, dim_z))
        self.SI = np.zeros((dim_z, dim_z))
        self._sig = self._sig_host = self._ws = None

        self.initialize(x, P)
        self.Q = np.eye(dim_x)
        self.R = np.eye(dim_z)
        self.inv = np.linalg.inv
        self._mean = np.zeros(dim_x)
        self._mean_z = np.zeros(dim_z)

    # -- the ensemble ---------------------------------------------------------------------------------------------------------
    @property
    def sigmas(self):
        """the ensemble as an (N, dim_x) NumPy array: downloaded on first read after a step, then cached"""
        if self._sig_host is None:
            self._sig_host = E.from_records(self._sig, self.layout, 0, (self.dim_x,)).copy()
        return self._sig_host

    @sigmas.setter
    def sigmas(self, value):
        a = np.asarray(value, dtype=np.float64)
        if a.shape != (self.N, self.dim_x):
            raise ValueError(f"sigmas has shape {a.shape}, expected ({self.N}, {self.dim_x})")
        self._sig = E.to_records(a, self.layout, 0)
        self._sig_host = None

    @property
    def sigmas_device(self):
        """the ensemble's device tensor, in `layout`: (dim_x, N) for 'soa', (N, dim_x) for 'aos'"""
        return self._sig

    def _members(self):
        """the device tensor as an (N, dim_x) view"""
        return self._sig.t() if self.layout == "soa" else self._sig

    def _records(self, t, d):
        """an (N, d) array or tensor -> device records in `layout`"""
        import torch
        if isinstance(t, torch.Tensor):
            t = E.dev(t)
            if tuple(t.shape) != (self.N, d):
                raise ValueError(f"expected an ({self.N}, {d}) tensor, got {tuple(t.shape)}")
            return t.t().contiguous() if self.layout == "soa" else t
        a = np.asarray(t, dtype=np.float64)
        if a.shape != (self.N, d):
            raise ValueError(f"expected an ({self.N}, {d}) array, got {a.shape}")
        return E.to_records(a, self.layout, 0)

    def _draw(self, mean, cov, d, init=False):
        """one draw of the cycle -> (noise records, factor or None).  noise "device": standard normals and cov's factor; otherwise
        the draws themselves, the mean included"""
        import torch
        if self.noise == "device":
            dev = E.require_gpu()
            shape = (d, self.N) if self.layout == "soa" else (self.N, d)
            w = torch.randn(shape, dtype=torch.float64, device=dev, generator=self.generator)
            return w, E.dev(_factor(cov))
        if callable(self.noise):
            e = self.noise(mean, cov, self.N)
        elif init:
            e = np.random.multivariate_normal(mean=mean, cov=cov, size=self.N)      # (:206)
        else:
            e = np.random.multivariate_normal(mean, cov, self.N)                    # (:263, :282)
        return self._records(e, d), None

    def _workspace(self):
        import torch
        if self._ws is None or self._ws.device != self._sig.device:
            nbytes = E.enkf_workspace_bytes(self.dim_x, self.dim_z, self.N)
            self._ws = torch.empty(max(nbytes, 8), dtype=torch.uint8, device=self._sig.device)
        return self._ws

    def _desc(self):
        return _desc(self.dim_x, self.dim_z, 0, self.N, 1, self.layout)

    # -- the reference's methods --------------------------------------------------------------------------------------------
    def initialize(self, x, P):
        """ensemble_kalman_filter.py:187-216: draws the ensemble from (x, P); keeps the given x and P"""
        import torch
        if x.ndim != 1:
            raise ValueError('x must be a 1D array')
        n, N = self.dim_x, self.N
        if self.noise == "device":
            dev = E.require_gpu()
            w, fac = self._draw(x, P, n)
            xd = E.dev(np.asarray(x, dtype=np.float64))
            self._sig = (xd[:, None].expand(n, N) if self.layout == "soa" else xd[None, :].expand(N, n)).contiguous()
            Pd = torch.empty((n, n), dtype=torch.float64, device=dev)
            E.enkf_predict(self._desc(), w, self._sig, xd, Pd, self._workspace(), F=None, factor=fac)
        else:
            self._sig = self._draw(x, P, n, init=True)[0]
        self._sig_host = None
        self.x = x
        self.P = P
        self.x_prior = self.x.copy()
        self.P_prior = self.P.copy()
        self.x_post = self.x.copy()
        self.P_post = self.P.copy()

    def _check_inv(self):
        if self.inv is not np.linalg.inv:
            raise NotImplementedError("EnsembleKalmanFilter.inv other than numpy.linalg.inv: the inverse is taken on the device")

    def _apply(self, fn, d, *args):
        """fx / hx as callables over the ensemble -> (N, d) device records (device_callables) or host array uploaded"""
        if self.device_callables:
            return self._records(fn(self._members(), *args), d)
        s = self.sigmas
        if self.vectorized:
            out = np.asarray(fn(s, *args), dtype=np.float64)
        else:
            out = np.zeros((self.N, d))
            for i in range(self.N):
                out[i] = fn(s[i], *args)
        return out

    def update(self, z, R=None):
        """ensemble_kalman_filter.py:218-273.  z None: bookkeeping only (:234-238)."""
        import torch
        if z is None:
            self.z = np.array([[None] * self.dim_z]).T
            self.x_post = self.x.copy()
            self.P_post = self.P.copy()
            return
        self._check_inv()
        n, m = self.dim_x, self.dim_z
        if R is None:
            R = self.R
        if np.isscalar(R):
            R = np.eye(m) * R
        R = np.asarray(R, dtype=np.float64)
        if R.shape != (m, m):
            raise ValueError(f"R has shape {R.shape}, expected ({m}, {m})")
        za = np.asarray(z, dtype=np.float64).reshape(-1)
        if za.shape != (m,):
            raise ValueError(f"z has {za.size} entries, expected dim_z = {m}")
        H = sh = None
        if isinstance(self.hx, np.ndarray):
            H = np.asarray(self.hx, dtype=np.float64)
            if H.shape != (m, n):
                raise ValueError(f"hx has shape {H.shape}, expected ({m}, {n})")
            H = E.dev(H)
        else:
            sh = self._apply(self.hx, m)
        noise, fac = self._draw(self._mean_z, R, m)          # (after every hx call, :263)
        if sh is not None and not isinstance(sh, torch.Tensor):
            sh = self._records(sh, m)
        x = E.dev(np.asarray(self.x, dtype=np.float64).reshape(n))
        P = E.dev(np.asarray(self.P, dtype=np.float64).reshape(n, n))
        S, SI, K = (torch.empty(s, dtype=torch.float64, device=x.device) for s in ((m, m), (m, m), (n, m)))
        st = torch.zeros(1, dtype=torch.int32, device=x.device)
        E.enkf_update(self._desc(), E.dev(R), E.dev(za), noise, self._sig, x, P, self._workspace(), H=H, sigmas_h=sh,
                      factor=fac, S=S, SI=SI, K=K, status=st)
        self._sig_host = None
        E.raise_on_status(st, "EnsembleKalmanFilter.update (S is not positive definite)")
        self.S = S.cpu().numpy()
        self.SI = SI.cpu().numpy()
        self.K = K.cpu().numpy()
        self.x = x.cpu().numpy()
        self.P = P.cpu().numpy()
        self.z = deepcopy(z)
        self.x_post = self.x.copy()
        self.P_post = self.P.copy()

    def predict(self):
        """ensemble_kalman_filter.py:275-290"""
        import torch
        n = self.dim_x
        F = None
        if isinstance(self.fx, np.ndarray):
            F = np.asarray(self.fx, dtype=np.float64)
            if F.shape != (n, n):
                raise ValueError(f"fx has shape {F.shape}, expected ({n}, {n})")
            F = E.dev(F)
        else:
            moved = self._apply(self.fx, n, self.dt)
        noise, fac = self._draw(self._mean, self.Q, n)       # (after every fx call, :282)
        if F is None:
            self._sig = moved if isinstance(moved, torch.Tensor) else self._records(moved, n)
        # the pivot of the one-pass sums: with a matrix the kernel takes F x; behind a callable the mean may have moved by
        # many spreads, and member 0 as fx left it is as close to the new mean as one member is (d spreads away it costs
        # eps d^2: at d = 30 the prior P is 2.8 x the two-pass form's error, tests/test_gpu_enkf_precision.py)
        if F is None:
            x = self._members()[0].clone()
        else:
            x = E.dev(np.asarray(self.x, dtype=np.float64).reshape(n))
        P = torch.empty((n, n), dtype=torch.float64, device=x.device)
        st = torch.zeros(1, dtype=torch.int32, device=x.device)
        E.enkf_predict(self._desc(), noise, self._sig, x, P, self._workspace(), F=F, factor=fac, status=st)
        self._sig_host = None
        E.raise_on_status(st, "EnsembleKalmanFilter.predict")
        self.x = x.cpu().numpy()
        self.P = P.cpu().numpy()
        self.x_prior = np.copy(self.x)
        self.P_prior = np.copy(self.P)

    def __repr__(self):
        return "\n".join(["EnsembleKalmanFilter object (filterpy_amd, gfx950)"] +
                         [f"{k} = {getattr(self, k)!r}" for k in
                          ("dim_x", "dim_z", "dt", "N", "layout", "noise", "x", "P", "x_prior", "P_prior", "Q", "R", "K", "S",
                           "sigmas", "hx", "fx")])
