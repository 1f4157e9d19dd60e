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
Many small ensembles -- hundreds to tens of thousands of targets with 2..2048 members each -- are EnsembleKalmanFilterBank
(below): one launch per predict() / update() for all of them, track by track the same bits as this class.
Out of scope: N > 2048 per ensemble in a bank; a one-launch batch_filter -- for one large ensemble it would need workgroups to
wait for each other inside a launch, and a step is already a short chain of launches on the caller's stream; multi-GPU.
"""
from copy import deepcopy

import numpy as np

from .. import _engine as E
from ._bank import _desc
from ._callable import status

__all__ = ["EnsembleKalmanFilter", "EnsembleKalmanFilterBank"]


def _factor(cov):
    """the d x d matrix A with e = w @ A ~ N(0, cov) for standard normal w: numpy.random.multivariate_normal's own"""
    _, s, v = np.linalg.svd(np.asarray(cov, dtype=np.float64))
    return np.ascontiguousarray(np.sqrt(s)[:, None] * v)


class _Ensemble(object):
    """What the one ensemble and the bank of them share.  `_lead` is () for EnsembleKalmanFilter and (n_tracks,) for the bank:
    every array of the surface is _lead + the single filter's shape, and the device tensor has the members on its last two
    axes.  A subclass states `_check_size`, `_given_x`, `_no_z`, `_draw`, `_apply`, `initialize`, `predict` and `update`."""
    _REPR = ("dim_x", "dim_z", "dt", "N", "layout", "noise", "x", "P", "x_prior", "P_prior", "Q", "R", "K", "S", "sigmas", "hx",
             "fx")

    def __init__(self, lead, x, P, dim_z, dt, N, hx, fx, noise, vectorized, device_callables, layout, generator):
        if dim_z <= 0:
            raise ValueError('dim_z must be greater than zero')
        if N < 2:
            raise ValueError('N must be at least 2 (the covariances divide by N - 1)')
        self._check_size(N, lead)
        if layout not in E.LAYOUTS:
            raise ValueError(f"layout must be one of {sorted(E.LAYOUTS)}")
        if not (noise in ("numpy", "device") or callable(noise)):
            raise ValueError('noise must be "numpy", "device" or a callable (mean, cov, N) -> (N, d)')
        x, dim_x = self._given_x(x)
        if dim_x > 16 or dim_z > 8:
            raise NotImplementedError("dim_x/dim_z outside the compiled range (dim_x <= 16, dim_z <= 8)")
        self._lead = lead
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
        self.K = np.zeros(lead + (dim_x, dim_z))
        self.z = self._no_z()
        self.S = np.zeros(lead + (dim_z, dim_z))
        self.SI = np.zeros(lead + (dim_z, dim_z))
        self._sig = self._sig_host = None

        self.initialize(x, P)
        self.Q = np.eye(dim_x)
        self.R = np.eye(dim_z)
        self.inv = np.linalg.inv
        self._mean = np.zeros(dim_x)
        self._mean_z = np.zeros(dim_z)

    def _check_size(self, N, lead):
        """the subclass's own refusals, between those of N and of the layout"""

    # -- the ensemble ---------------------------------------------------------------------------------------------------------
    @property
    def sigmas(self):
        """the members as a _lead + (N, dim_x) NumPy array: downloaded on first read after a step, then cached"""
        if self._sig_host is None:
            self._sig_host = E.from_records(self._sig, self.layout, len(self._lead), (self.dim_x,)).copy()
        return self._sig_host

    @sigmas.setter
    def sigmas(self, value):
        a = np.asarray(value, dtype=np.float64)
        if a.shape != self._lead + (self.N, self.dim_x):
            raise ValueError(f"sigmas has shape {a.shape}, expected {self._lead + (self.N, self.dim_x)}")
        self._sig = E.to_records(a, self.layout, len(self._lead))
        self._sig_host = None

    @property
    def sigmas_device(self):
        """the device tensor, in `layout`: _lead + (dim_x, N) for 'soa', _lead + (N, dim_x) for 'aos'"""
        return self._sig

    def _members(self):
        """the device tensor as a _lead + (N, dim_x) view"""
        return self._sig.transpose(-1, -2) if self.layout == "soa" else self._sig

    def _records(self, t, d):
        """a _lead + (N, d) array or tensor -> device records in `layout`"""
        import torch
        shape = self._lead + (self.N, d)
        if isinstance(t, torch.Tensor):
            t = E.dev(t)
            if tuple(t.shape) != shape:
                raise ValueError(f"expected an {shape} tensor, got {tuple(t.shape)}")
            return t.transpose(-1, -2).contiguous() if self.layout == "soa" else t
        a = np.asarray(t, dtype=np.float64)
        if a.shape != shape:
            raise ValueError(f"expected an {shape} array, got {a.shape}")
        return E.to_records(a, self.layout, len(self._lead))

    # -- the bookkeeping around a step --------------------------------------------------------------------------------------
    def _check_inv(self):
        if self.inv is not np.linalg.inv:
            raise NotImplementedError(f"{type(self).__name__}.inv other than numpy.linalg.inv: the inverse is taken on the device")

    def _given_R(self, R):
        """update()'s R: None -> the attribute, a scalar -> eye * R (:250-254); the subclass checks the shape"""
        if R is None:
            R = self.R
        if np.isscalar(R):
            R = np.eye(self.dim_z) * R
        return R

    def _copy_state(self, *to):
        """x_prior / P_prior ("prior") or x_post / P_post ("post") <- copies of x, P as they stand"""
        for k in to:
            setattr(self, "x_" + k, self.x.copy())
            setattr(self, "P_" + k, self.P.copy())

    def _skip_update(self):
        """update(None) (:234-238)"""
        self.z = self._no_z()
        self._copy_state("post")

    def _download(self, **tensors):
        """attribute = tensor: the small results of a step as NumPy arrays"""
        for k, t in tensors.items():
            setattr(self, k, t.cpu().numpy())

    def __repr__(self):
        return "\n".join([f"{type(self).__name__} object (filterpy_amd, gfx950)"] +
                         [f"{k} = {getattr(self, k)!r}" for k in self._REPR])


class EnsembleKalmanFilter(_Ensemble):
    """filterpy.kalman.EnsembleKalmanFilter (ensemble_kalman_filter.py:36-309) on the GPU: same attributes and defaults."""

    def __init__(self, x, P, dim_z, dt, N, hx, fx, *, noise="numpy", vectorized=False, device_callables=False, layout="soa",
                 generator=None):
        self._ws = None
        super().__init__((), x, P, dim_z, dt, N, hx, fx, noise, vectorized, device_callables, layout, generator)

    def _given_x(self, x):
        return x, len(x)

    def _no_z(self):
        return np.array([[None] * self.dim_z]).T

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
        self._copy_state("prior", "post")

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
            return self._skip_update()
        self._check_inv()
        n, m = self.dim_x, self.dim_z
        R = np.asarray(self._given_R(R), dtype=np.float64)
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
        st = status(1, x)
        E.enkf_update(self._desc(), E.dev(R), E.dev(za), noise, self._sig, x, P, self._workspace(), H=H, sigmas_h=sh,
                      factor=fac, S=S, SI=SI, K=K, status=st)
        self._sig_host = None
        E.raise_on_status(st, "EnsembleKalmanFilter.update (S is not positive definite)")
        self._download(S=S, SI=SI, K=K, x=x, P=P)
        self.z = deepcopy(z)
        self._copy_state("post")

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
        st = status(1, x)
        E.enkf_predict(self._desc(), noise, self._sig, x, P, self._workspace(), F=F, factor=fac, status=st)
        self._sig_host = None
        E.raise_on_status(st, "EnsembleKalmanFilter.predict")
        self._download(x=x, P=P)
        self._copy_state("prior")


class EnsembleKalmanFilterBank(_Ensemble):
    """n_tracks independent ensemble Kalman filters of N members each (2 <= N <= 2048), stepped together: predict() is ONE launch
    for all ensembles (fk_enkf_bank_predict_f64) and update() is one (fk_enkf_bank_update_f64; csrc/enkf_bank.hip) -- one wave per
    ensemble up to N = 64, one workgroup per ensemble above.  The arithmetic and its order are EnsembleKalmanFilter's: on the same
    draws track b has, bit for bit, the members, x, P, K, S and SI of a single filter.

    The surface is EnsembleKalmanFilter's with a leading n_tracks axis: x (n_tracks, dim_x) -- given as (dim_x,) it is repeated --,
    P (n_tracks, dim_x, dim_x), x_prior, P_prior, x_post, P_post, K, S, SI; Q and R are one matrix for all tracks or one per track
    ((n_tracks, d, d)).  `sigmas` is the (n_tracks, N, dim_x) array, downloaded on first read after a step and cached (assign to
    upload; in-place edits are not seen); `sigmas_device` is the tensor in `layout`: 'soa' (n_tracks, dim_x, N) -- slice b is the
    single class's tensor --, 'aos' (n_tracks, N, dim_x).  `z` is an (n_tracks, dim_z) object array: the measurement of the
    tracks that took part in the last update, None for the others.  `status` is the kernels' int32 word per track of the last call.

    fx / hx:
      * matrices, (dim_x, dim_x) / (dim_z, dim_x) for all tracks or (n_tracks, ., .) one per track: the fused path, the ensembles
        never leave device memory;
      * callables per member, fx(s, dt) / hx(s) as the reference calls them -- one callable, or a sequence of n_tracks of them;
      * vectorized=True: NumPy callables on the whole (n_tracks, N, dim_x) array;
      * device_callables=True: callables on (n_tracks, N, dim_x) float64 GPU tensors.

    update(z, R=None, mask=None): z (n_tracks, dim_z), or a sequence whose entry b may be None; mask (n_tracks,) of 0 / 1.  A track
    without a measurement, or with mask 0, gets the reference's update(None): its members, x, P, K, S and SI stay, its z becomes
    None and x_post, P_post copy x, P.  update(None) does that to every track and launches nothing.

    noise: "numpy" draws numpy.random.multivariate_normal(mean_b, cov_b, N) once per track that takes part, in track order, after
    the callables: predict() consumes the global stream as `for f in filters: f.predict()` does, update() as that loop's
    f.update(z_b) (a loop's update(None) draws nothing; neither does a masked track here).  A callable noise(mean, cov, N) has the
    same call sites.  "device": ONE torch.randn of the whole bank's shape; the per-track factors of Q / R are applied in-lane.

    S not positive definite raises numpy.linalg.LinAlgError naming the first such track, a non-finite state FloatingPointError
    (the other tracks' results are kept in the kernels' outputs; `status` says which).  inv other than numpy.linalg.inv, dim_x > 16
    or dim_z > 8 raise NotImplementedError, and so does N > 2048: larger ensembles are EnsembleKalmanFilter's, one at a time.
    Measured on an MI355X against a Python loop over EnsembleKalmanFilter objects (matrix fx / hx, noise="device"; B = 1e2 ... 1e4
    tracks, N = 32 ... 1024, (4, 2) and (6, 3)): no row is slower; one cycle takes 0.03 ms up to 1e3 tracks of 64 members and
    0.10-0.15 ms for 1e4, 250-8600 x less than the loop's launches alone.  At N = 256 the serial S^-1 and the barriers show
    (0.14-0.24 of 8 TB/s against 0.40-0.55 at N = 1024): docs/MEASUREMENTS.md, "EnKF bank"."""

    def __init__(self, x, P, dim_z, dt, N, hx, fx, n_tracks, *, noise="numpy", vectorized=False, device_callables=False,
                 layout="soa", generator=None):
        self.n_tracks = n_tracks
        super().__init__((n_tracks,), x, P, dim_z, dt, N, hx, fx, noise, vectorized, device_callables, layout, generator)
        self.status = np.zeros(n_tracks, dtype=np.int32)

    _REPR = ("n_tracks",) + _Ensemble._REPR

    def _check_size(self, N, lead):
        if N > E.ENKF_CHUNK:
            raise NotImplementedError(f"N = {N} > {E.ENKF_CHUNK} members per ensemble of a bank: use EnsembleKalmanFilter, one "
                                      "filter per ensemble")
        if lead[0] < 1:
            raise ValueError('n_tracks must be at least 1')

    def _given_x(self, x):
        x = np.asarray(x, dtype=np.float64)
        if x.ndim not in (1, 2):
            raise ValueError('x must be (dim_x,) or (n_tracks, dim_x)')
        return x, x.shape[-1]

    def _no_z(self):
        return np.full((self.n_tracks, self.dim_z), None, dtype=object)

    # -- shapes ---------------------------------------------------------------------------------------------------------------
    def _per_track(self, a, shape, name):
        """a: `shape`, or (n_tracks,) + shape -> float64 array as given (the leading axis says which)"""
        a = np.asarray(a, dtype=np.float64)
        if a.shape != tuple(shape) and a.shape != (self.n_tracks,) + tuple(shape):
            raise ValueError(f"{name} has shape {a.shape}, expected {tuple(shape)} or {(self.n_tracks,) + tuple(shape)}")
        return a

    def _full(self, a, shape):
        """... repeated to (n_tracks,) + shape"""
        return np.ascontiguousarray(np.broadcast_to(a, (self.n_tracks,) + tuple(shape)))

    def _model(self, parts):
        """the matrices of one call (None entries pass through) -> (model_mode, device tensors): all shared, or -- when any has a
        leading n_tracks axis -- all one per track"""
        per = any(p is not None and p.ndim == 3 for p in parts)
        out = [None if p is None else E.dev(self._full(p, p.shape[-2:]) if per else p) for p in parts]
        return (E.FK_MODEL_PER_TRACK if per else E.FK_MODEL_SHARED), out

    def _desc(self, mode):
        return dict(_desc(self.dim_x, self.dim_z, 0, self.N, 1, self.layout), model_mode=mode)

    # -- the ensembles ------------------------------------------------------------------------------------------------------
    def _draw(self, mean, cov, d, present=None, init=False):
        """one draw of the cycle for the tracks that take part -> (noise records, per-track-or-shared factor or None).  mean: (d,)
        or (n_tracks, d); cov: (d, d) or (n_tracks, d, d)"""
        import torch
        B, N = self.n_tracks, self.N
        if self.noise == "device":
            dev = E.require_gpu()
            shape = (B, d, N) if self.layout == "soa" else (B, N, d)
            w = torch.randn(shape, dtype=torch.float64, device=dev, generator=self.generator)
            fac = np.stack([_factor(c) for c in cov]) if cov.ndim == 3 else _factor(cov)
            return w, fac
        e = np.zeros((B, N, d))
        for b in range(B):
            if present is not None and not present[b]:
                continue
            mb, cb = (mean[b] if mean.ndim == 2 else mean), (cov[b] if cov.ndim == 3 else cov)
            if callable(self.noise):
                eb = self.noise(mb, cb, N)
                eb = eb.detach().cpu().numpy() if isinstance(eb, torch.Tensor) else np.asarray(eb, dtype=np.float64)
            elif init:
                eb = np.random.multivariate_normal(mean=mb, cov=cb, size=N)         # (:206)
            else:
                eb = np.random.multivariate_normal(mb, cb, N)                       # (:263, :282)
            if eb.shape != (N, d):
                raise ValueError(f"noise returned shape {eb.shape}, expected ({N}, {d})")
            e[b] = eb
        return self._records(e, d), None

    # -- the reference's methods ------------------------------------------------------------------------------------------------
    def initialize(self, x, P):
        """ensemble_kalman_filter.py:187-216 for every track: draws the ensembles from (x_b, P_b); keeps the given x and P"""
        import torch
        n, N, B = self.dim_x, self.N, self.n_tracks
        x = self._per_track(x, (n,), "x")
        P = self._per_track(P, (n, n), "P")
        if self.noise == "device":
            dev = E.require_gpu()
            w, fac = self._draw(x, P, n)
            xd = E.dev(self._full(x, (n,)))
            self._sig = (xd[:, :, None].expand(B, n, N) if self.layout == "soa" else xd[:, None, :].expand(B, N, n)).contiguous()
            Pd = torch.empty((B, n, n), dtype=torch.float64, device=dev)
            mode, (fac,) = self._model([fac])
            E.enkf_bank_predict(self._desc(mode), B, w, self._sig, xd, Pd, F=None, factor=fac)
        else:
            self._sig = self._draw(x, P, n, init=True)[0]
        self._sig_host = None
        self.x = self._full(x, (n,))
        self.P = self._full(P, (n, n))
        self._copy_state("prior", "post")

    def _apply(self, fn, d, *args, present=None):
        """fx / hx as callables over the ensembles -> (n_tracks, N, d) device records (device_callables) or host array"""
        if self.device_callables:
            return self._records(fn(self._members(), *args), d)
        s = self.sigmas
        if self.vectorized:
            return np.asarray(fn(s, *args), dtype=np.float64)
        out = np.zeros((self.n_tracks, self.N, d))
        for b in range(self.n_tracks):
            if present is not None and not present[b]:
                continue                                      # (the reference's update(None) calls no hx)
            f = fn if callable(fn) else fn[b]
            for i in range(self.N):
                out[b, i] = f(s[b, i], *args)
        return out

    def _matrix(self, f, shape, name):
        if isinstance(f, np.ndarray):
            return self._per_track(f, shape, name)
        return None

    def update(self, z, R=None, mask=None):
        """ensemble_kalman_filter.py:218-273 for every track that has a measurement and a nonzero mask; :234-238 for the others"""
        import torch
        B, n, m = self.n_tracks, self.dim_x, self.dim_z
        present = np.ones(B, dtype=bool)
        if mask is not None:
            mk = np.asarray(mask)
            if mk.shape != (B,):
                raise ValueError(f"mask has shape {mk.shape}, expected ({B},)")
            present &= mk != 0
        if z is None:
            present[:] = False
        else:
            if len(z) != B:
                raise ValueError(f"z has {len(z)} entries, expected n_tracks = {B}")
            za = np.zeros((B, m))
            for b in range(B):
                if z[b] is None:
                    present[b] = False
                    continue
                zb = np.asarray(z[b], dtype=np.float64).reshape(-1)
                if zb.shape != (m,):
                    raise ValueError(f"z[{b}] has {zb.size} entries, expected dim_z = {m}")
                za[b] = zb
        if not present.any():
            return self._skip_update()
        self._check_inv()
        R = self._per_track(self._given_R(R), (m, m), "R")
        H = self._matrix(self.hx, (m, n), "hx")
        sh = None if H is not None else self._apply(self.hx, m, present=present)
        noise, fac = self._draw(self._mean_z, R, m, present)             # (after every hx call, :263)
        if sh is not None and not isinstance(sh, torch.Tensor):
            sh = self._records(sh, m)
        mode, (H, Rd, fac) = self._model([H, R, fac])
        x = E.dev(self._full(self._per_track(self.x, (n,), "x"), (n,)))
        P = E.dev(self._full(self._per_track(self.P, (n, n), "P"), (n, n)))
        S, SI, K = (E.dev(self._full(self._per_track(a, s, k), s)) for a, s, k in
                    ((self.S, (m, m), "S"), (self.SI, (m, m), "SI"), (self.K, (n, m), "K")))
        st = status(B, x)
        mk = None if present.all() else torch.as_tensor(present.astype(np.uint8), device=x.device)
        E.enkf_bank_update(self._desc(mode), B, Rd, E.dev(za), noise, self._sig, x, P, H=H, sigmas_h=sh, mask=mk, factor=fac,
                           S=S, SI=SI, K=K, status=st)
        self._sig_host = None
        self.status = st.cpu().numpy()
        E.raise_on_status(st, "EnsembleKalmanFilterBank.update (S is not positive definite)")
        self._download(S=S, SI=SI, K=K, x=x, P=P)
        self.z = self._no_z()
        self.z[present] = za[present]
        self._copy_state("post")

    def predict(self):
        """ensemble_kalman_filter.py:275-290 for every track"""
        import torch
        B, n = self.n_tracks, self.dim_x
        F = self._matrix(self.fx, (n, n), "fx")
        if F is None:
            moved = self._apply(self.fx, n, self.dt)
        noise, fac = self._draw(self._mean, self._per_track(self.Q, (n, n), "Q"), n)       # (after every fx call, :282)
        if F is None:
            self._sig = moved if isinstance(moved, torch.Tensor) else self._records(moved, n)
            # the pivot behind a callable: member 0 of every track, as fx left it (EnsembleKalmanFilter.predict)
            x = self._members()[:, 0, :].clone().contiguous()
        else:
            x = E.dev(self._full(self._per_track(self.x, (n,), "x"), (n,)))
        mode, (F, fac) = self._model([F, fac])
        P = torch.empty((B, n, n), dtype=torch.float64, device=x.device)
        st = status(B, x)
        E.enkf_bank_predict(self._desc(mode), B, noise, self._sig, x, P, F=F, factor=fac, status=st)
        self._sig_host = None
        self.status = st.cpu().numpy()
        E.raise_on_status(st, "EnsembleKalmanFilterBank.predict")
        self._download(x=x, P=P)
        self._copy_state("prior")
