"""What the filters whose kernels take ONE model for every track share on the host (square_root.py, information_filter.py,
fixed_lag_smoother.py): the descriptor, the control-input rules, the shape checks of the single-filter classes and the
plumbing of the banks.  Private: the three modules import from here and not from each other.  The filters that run the
caller's callables between the kernels share _callable.py instead; the status word and the four histories come from there."""
import numpy as np

from .. import _engine as E
from .._abi import FK_MODEL_SHARED
from ._callable import alloc_histories, status


def _desc(n, m, nu, N, T, layout, update_first=False, flags=0):
    return dict(n=n, m=m, nu=nu, model_mode=FK_MODEL_SHARED, N=N, T=T, layout=E.LAYOUTS[layout],
                update_first=int(bool(update_first)), alpha_sq=1.0, flags=flags)


def _control(B, n, us_shape_tail, what="u"):
    """B attribute + the shape of one step's u -> (B (n, nu) matrix, nu), or (None, 0) for no control input"""
    size = int(np.prod(us_shape_tail)) if len(us_shape_tail) else 1
    if np.isscalar(B) or np.ndim(B) == 0:
        b = float(B)
        if size != n:
            raise ValueError(f"with a scalar B, {what} must have dim_x = {n} entries (b u = (b I) u), got shape {tuple(us_shape_tail)}")
        if b == 0.0:
            return None, 0
        return np.eye(n) * b, n
    Bm = np.asarray(B, dtype=np.float64)
    if Bm.ndim == 1 and n == 1:
        Bm = Bm.reshape(1, -1)
    if Bm.ndim != 2 or Bm.shape[0] != n:
        raise ValueError(f"B has shape {Bm.shape}, expected ({n}, dim_u)")
    if size != Bm.shape[1]:
        raise ValueError(f"{what} has {size} entries, B has {Bm.shape[1]} columns")
    return np.ascontiguousarray(Bm), Bm.shape[1]


def _check_u_orientation(sh, nu, n, xshape):
    """x += dot(B, u): u must keep x's orientation, else x becomes an (n, n) matrix or numpy refuses"""
    ok = sh == (nu, 1) or (n == 1 and sh == (nu,)) if len(xshape) == 2 else sh == (nu,)
    if not ok:
        raise ValueError(f"control input of shape {sh} with x of shape {xshape}: expected "
                         + (f"({nu}, 1)" if len(xshape) == 2 else f"({nu},)"))


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
    _check_u_orientation(ua.shape, nu, n, xshape)
    if Bm is None:
        return None, None
    return Bm, ua.reshape(nu)


def _xshape(x, n):
    """the shape of a single filter's x: (n,) or (n, 1), or ValueError"""
    shape = np.asarray(x, dtype=np.float64).shape
    if shape not in ((n,), (n, 1)):
        raise ValueError(f"x has shape {shape}, expected ({n},) or ({n}, 1)")
    return shape


def _z(z, m, xshape):
    """one measurement as float64 (m entries, in the shape given), refusing the shapes the reference turns into nonsense"""
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
    return za


def _device_zs(zs, T, N, m, layout):
    """device measurements must already be records of the bank's layout"""
    import torch
    want = (T, N, m) if layout == "aos" else (T, m, N)
    if tuple(zs.shape) != want:
        raise ValueError(f"device zs has shape {tuple(zs.shape)}, expected {want} ({layout} records)")
    return zs.to(dtype=torch.float64).contiguous()


def _host_zs(zs, T, N, m):
    za = np.asarray(zs, dtype=np.float64)
    if za.shape != (T, N, m) and not (m == 1 and za.shape == (T, N)):
        raise ValueError(f"zs has shape {za.shape}, expected ({T}, {N}, {m})")
    return za.reshape(T, N, m)


def _bank_controls(B, us, T, N, n):
    """a bank's us (T, N, dim_u) and its B -> (B (n, nu), us (T, N, nu)) host arrays, or (None, None)"""
    if us is None:
        return None, None
    ua = np.asarray(us, dtype=np.float64)
    if ua.ndim == 2:
        ua = ua[:, :, None]
    if ua.ndim != 3 or ua.shape[:2] != (T, N):
        raise ValueError(f"us has shape {ua.shape}, expected ({T}, {N}, dim_u)")
    if B is None:
        raise ValueError("us given but B is None")
    Bm, _ = _control(B, n, ua.shape[2:], "us")
    if Bm is None:
        return None, None
    return Bm, np.ascontiguousarray(ua)


class _SharedModelBank(object):
    """n_tracks filters that share their model, stepped in lock-step: one launch per predict() / update(), one for the whole
    time loop of batch_filter().  A subclass states its state (the attribute `_COV` next to x, `_state()`), its model
    (`_model(R=None)` -> the four device matrices the kernels take, R replacing the fourth for one update), the prefix of
    its engine functions, the by-products of an update and what a nonzero status means per method."""
    _ENGINE = None          # E.<_ENGINE>_predict / _update / _batch, looked up per call
    _COV = None             # the attribute that holds the (N, n, n) half of the state
    _BYPRODUCTS = ()        # (attribute, engine keyword, shape in letters of "nm") of the last update's by-products
    _SINGULAR = {}          # method name -> what a nonzero status means, appended to the error's label

    def __init__(self, dim_x, dim_z, n_tracks, dim_u=0, layout="soa"):
        if dim_x < 1 or dim_z < 1 or dim_u < 0 or n_tracks < 1:
            raise ValueError("dim_x, dim_z, n_tracks must be >= 1 and dim_u >= 0")
        if layout not in E.LAYOUTS:
            raise ValueError("layout must be 'soa' or 'aos'")
        self.dim_x, self.dim_z, self.dim_u, self.n_tracks, self.layout = dim_x, dim_z, dim_u, n_tracks, layout
        self.x = np.zeros((n_tracks, dim_x))
        self.F = np.eye(dim_x)
        self.H = np.zeros((dim_z, dim_x))
        self.B = None
        # the last update's by-products per track (update() sets them for the tracks that update)
        for attr, _, shape in self._BYPRODUCTS:
            setattr(self, attr, np.zeros((n_tracks,) + self._shape(shape)))

    def _shape(self, letters):
        return tuple({"n": self.dim_x, "m": self.dim_z}[c] for c in letters)

    # -- plumbing -----------------------------------------------------------------------------------------------------------
    def _x_records(self):
        n, N = self.dim_x, self.n_tracks
        x = np.asarray(self.x, dtype=np.float64)
        if x.size != N * n:
            raise ValueError(f"x has shape {x.shape}, expected ({N}, {n})")
        return E.to_records(x.reshape(N, n), self.layout, 0).clone()

    def _controls(self, us, T):
        B, ua = _bank_controls(self.B, us, T, self.n_tracks, self.dim_x)
        if B is None:
            return None, None
        return E.dev(B), E.to_records(ua, self.layout, 1)

    def _measurements(self, zs, T, mask):
        """zs (T, N, m) host (NaN rows missing) or device records -> (device z, device uint8 mask or None)"""
        import torch
        m, N = self.dim_z, self.n_tracks
        keep = None
        if isinstance(zs, torch.Tensor):
            z = _device_zs(zs, T, N, m, self.layout)
        else:
            za = _host_zs(zs, T, N, m)
            nan = np.isnan(za).any(axis=2)
            if nan.any():
                keep = ~nan
                za = np.where(nan[:, :, None], 0.0, za)
            z = E.to_records(za, self.layout, 1)
        if mask is not None:
            mk = np.asarray(mask, dtype=bool).reshape(T, N)
            keep = mk if keep is None else (keep & mk)
        dm = None if keep is None else torch.from_numpy(np.ascontiguousarray(keep, dtype=np.uint8)).to(E.require_gpu())
        return z, dm

    def _host(self, t, lead, rec_shape):
        return E.host_records(t.cpu().numpy(), self.layout, lead, rec_shape)

    def _engine(self, what):
        return getattr(E, f"{self._ENGINE}_{what}")

    def _raise_on_status(self, st, method):
        E.raise_on_status(st, f"{type(self).__name__}.{method}{self._SINGULAR.get(method, '')}")

    def _store_state(self, x, C):
        n = self.dim_x
        self.x = self._host(x, 0, (n,))
        setattr(self, self._COV, self._host(C, 0, (n, n)))

    # -- steps --------------------------------------------------------------------------------------------------------------
    def predict(self, u=None):
        """one predict for every track: u (n_tracks, dim_u) or None"""
        n, N = self.dim_x, self.n_tracks
        F, Q, _, _ = self._model()
        B, du = self._controls(None if u is None else np.asarray(u, dtype=np.float64).reshape(1, N, -1), 1)
        x, C = self._state()
        st = status(N, x)
        nu = 0 if B is None else int(B.shape[1])
        self._engine("predict")(_desc(n, self.dim_z, nu, N, 1, self.layout), F, Q, x, C, B=B,
                                u=None if du is None else du.reshape(du.shape[1:]), status=st)
        self._raise_on_status(st, "predict")
        self._store_state(x, C)

    def _update(self, z, R, mask):
        """one update for every track; R: what replaces the model's fourth matrix for this call (`_model(R)`), or None"""
        n, m, N = self.dim_x, self.dim_z, self.n_tracks
        _, _, H, Rm = self._model(R)
        dz, dm = self._measurements(np.asarray(z, dtype=np.float64).reshape(1, N, m), 1,
                                    None if mask is None else np.asarray(mask).reshape(1, N))
        x, C = self._state()
        outs = {kw: E.to_records(np.asarray(getattr(self, attr), dtype=np.float64).reshape(N, -1), self.layout, 0).clone()
                for attr, kw, _ in self._BYPRODUCTS}
        st = status(N, x)
        self._engine("update")(_desc(n, m, 0, N, 1, self.layout), H, Rm, dz.reshape(dz.shape[1:]), x, C,
                               mask=None if dm is None else dm.reshape(N), status=st, **outs)
        self._raise_on_status(st, "update")
        self._store_state(x, C)
        for attr, kw, shape in self._BYPRODUCTS:
            setattr(self, attr, self._host(outs[kw], 0, self._shape(shape)))

    def batch_filter(self, zs, mask=None, us=None, update_first=False, device_outputs=False):
        """(means, covs, means_p, covs_p) of the whole run in the subclass's form of the covariance, ONE launch; the state is
        left alone.  zs (T, N, dim_z) with NaN rows missing (or device records in `layout`), mask (T, N) bool (False =
        missing), us (T, N, dim_u)."""
        n, m, N = self.dim_x, self.dim_z, self.n_tracks
        T = int(zs.shape[0]) if hasattr(zs, "shape") else len(zs)
        if T == 0:
            e = np.zeros((0, N, n))
            return e, np.zeros((0, N, n, n)), e.copy(), np.zeros((0, N, n, n))
        F, Q, H, R = self._model()
        dz, dm = self._measurements(zs, T, mask)
        B, du = self._controls(us, T)
        x, C = self._state()
        means, covs, means_p, covs_p = alloc_histories(T, N, n, self.layout, x.device)
        st = status(N, x)
        nu = 0 if B is None else int(B.shape[1])
        self._engine("batch")(_desc(n, m, nu, N, T, self.layout, update_first), F, Q, H, R, dz, x, C, B=B, u=du, mask=dm,
                              means=means, covs=covs, means_p=means_p, covs_p=covs_p, status=st)
        self._raise_on_status(st, "batch_filter")
        if device_outputs:
            return means, covs, means_p, covs_p
        return (self._host(means, 1, (n,)), self._host(covs, 1, (n, n)),
                self._host(means_p, 1, (n,)), self._host(covs_p, 1, (n, n)))
