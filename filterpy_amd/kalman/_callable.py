"""What the filters that run the CALLER'S callables between the kernels share on the host (UKF.py, CubatureKalmanFilter.py,
EKF.py): the constructor's refusals and its (_N, _layout, _mode) triple, the bank-shaped views of x and P, the two directions
between what a callable takes or returns -- (N,) + shape, array or device tensor -- and device records in the bank's layout, and
the four histories of a batch_filter().  `status` also serves _bank.py and ensemble_kalman_filter.py.  Private; the filters whose
kernels take one MODEL for every track share _bank.py instead."""
import numpy as np
import torch

from .. import _engine as E


def status(N, like):
    """the kernels' int32 status word per track, zeroed, on like's device"""
    return torch.zeros(N, dtype=torch.int32, device=like.device)


def rec_view(rec, N, k, d, layout):
    """device records of N (k x d) blocks -> torch view (N, k, d), no copy"""
    if layout == "aos":
        return rec.view(N, k, d)
    return rec.view(k, d, N).permute(2, 0, 1)


def as_records(t, N, layout):
    """device tensor (N, d) or (N, k, d) -> device records in `layout`, [N][E] or [E][N]: at most one copy"""
    if layout == "aos":
        return t.contiguous().view(N, -1)
    return t.t().contiguous() if t.dim() == 2 else t.permute(1, 2, 0).contiguous().view(-1, N)


def track_rows(rec, layout):
    """device records of one vector per track, [N][d] or [d][N] -> contiguous (N, d) tensor (the records themselves for 'aos')"""
    return rec if layout == "aos" else rec.t().contiguous()


def to_rec(t, N, shape, layout, tensor, name=None):
    """(N,) + shape as a callable returned it -> device records in `layout`.  tensor: it has to be a float64 tensor on the GPU
    (device callables); otherwise anything numpy.asarray takes, uploaded.  name: the callable's, for the message"""
    full = (N,) + tuple(shape)
    if tensor:
        if (not isinstance(t, torch.Tensor) or t.device.type != E.require_gpu().type or t.dtype != torch.float64
                or tuple(t.shape) != full):
            raise TypeError(f"device callables{': ' + name if name else ''} must return a float64 CUDA tensor shaped {full}")
    else:
        a = np.asarray(t, dtype=np.float64)
        if a.shape != full:
            raise ValueError(f"{name or 'the callable'} returned shape {a.shape}, expected {full}")
        t = E.dev(a)
    return as_records(t, N, layout)


def alloc_histories(T, N, n, layout, device=None):
    """batch_filter's four histories as device records: [means, covariances, prior means, prior covariances]"""
    return [E.alloc_records((T,), N, e, layout, device) for e in (n, n * n, n, n * n)]


def host_histories(outs, n, layout):
    """... downloaded: (T, N, n), (T, N, n, n), (T, N, n), (T, N, n, n)"""
    return tuple(E.from_records(o, layout, 1, s) for o, s in zip(outs, ((n,), (n, n), (n,), (n, n))))


class _CallableHost(object):
    """mixin of the three classes: `_preamble` sets _N (None: one filter), _layout and _mode ("loop", "vec" or "torch": where
    and how the callables run); `_xb` / `_Pb` read x, P and dim_x"""

    def _preamble(self, n_tracks, vectorized, device_callables, layout, dims=None, vectorized_bank_only=False):
        """the constructor's refusals (dims: (dim_x, dim_z) where the class checks them and the layout) and the mode"""
        if device_callables and n_tracks is None:
            raise ValueError("device_callables=True needs a bank: pass n_tracks=N (use N = 1 for one filter)")
        if vectorized_bank_only and vectorized and n_tracks is None:
            raise ValueError("vectorized=True needs a bank: pass n_tracks=N")
        if dims is not None:
            if min(dims) < 1:
                raise ValueError("dim_x and dim_z must be 1 or greater")
            if layout not in E.LAYOUTS:
                raise ValueError(f"layout must be one of {sorted(E.LAYOUTS)}")
        self._N = n_tracks
        self._layout = layout
        self._mode = "torch" if device_callables else ("vec" if vectorized else "loop")

    def _unb(self, a):
        """bank-shaped -> what a single filter holds"""
        return a if self._N is not None else a[0]

    def _xb(self):
        """x as (N, n); a single filter's x is (n,) or (n, 1)"""
        n, N = self.dim_x, self._N or 1
        x = np.asarray(self.x, dtype=np.float64)
        ok = x.shape == (N, n) if self._N is not None else x.shape in ((n,), (n, 1))
        if not ok:
            raise ValueError(f"x has shape {x.shape}, expected " +
                             (f"({N}, {n})" if self._N is not None else f"({n},) or ({n}, 1)"))
        return np.ascontiguousarray(x.reshape(N, n))

    def _Pb(self):
        n, N = self.dim_x, self._N or 1
        P = np.asarray(self.P, dtype=np.float64)
        if P.shape == (n, n):
            P = np.broadcast_to(P, (N, n, n))
        if P.shape != (N, n, n):
            raise ValueError(f"P has shape {P.shape}, expected ({N}, {n}, {n})" + (f" or ({n}, {n})" if self._N else ""))
        return np.ascontiguousarray(P)

    def _rec_view(self, rec, k, d):
        return rec_view(rec, self._N or 1, k, d, self._layout)
