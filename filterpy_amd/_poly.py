"""Host side shared by filterpy_amd.gh, filterpy_amd.memory and filterpy_amd.leastsq: the fixed-gain polynomial filters all run
on one entry point, fk_poly_run (include/filterhip.h, csrc/fk_poly.hpp), and differ in the scalars they hand it.  Here: moving
a filter's state and measurements to the device and back in the array type the user chose, and the one call.

Residency: what the user gives decides what comes back.  NumPy arrays and Python numbers in: NumPy arrays and Python floats out
(uploaded and downloaded around the launch, large arrays through _transfer).  torch tensors in: device tensors out, nothing
crosses PCIe between steps.  The arithmetic always runs on the GPU; there is no CPU path."""
import numpy as np
import torch

from . import _abi
from . import _engine as E
from . import _transfer

FORM_A, FORM_B, FORM_C = _abi.FK_POLY_FORM_A, _abi.FK_POLY_FORM_B, _abi.FK_POLY_FORM_C


def is_tensor(a):
    return isinstance(a, torch.Tensor)


def scalar_gain(v, name):
    """a gain as a Python float; one gain per track is not served (include/filterhip.h)"""
    if getattr(v, "ndim", 0) != 0 or isinstance(v, (list, tuple)):
        raise NotImplementedError(f"{name}: one gain per track is not supported, every track of a bank shares the gains")
    return float(v)


def check_order(order):
    if order < 0 or order > 2:
        raise ValueError('order must be between 0 and 2')


def row(a):
    """one component of a state, or one step of measurements -> a device tensor (N,); a number is a bank of one"""
    if is_tensor(a):
        return E.dev(a).reshape(-1)
    return E.dev(np.atleast_1d(np.asarray(a, dtype=np.float64)).reshape(-1))


def rows(parts):
    """the components of a state -> the device tensor (c, N) fk_poly_run updates in place (FK_LAYOUT_SOA)"""
    return torch.stack([row(p) for p in parts])


def steps(zs, N):
    """measurements (T,) of one filter or (T, N) of a bank -> device tensor (T, N)"""
    t = E.dev(zs) if is_tensor(zs) else E.dev(np.asarray(zs, dtype=np.float64))
    if t.ndim == 0:
        t = t.reshape(1)
    if t.ndim == 1 and N == 1:
        t = t.reshape(-1, 1)
    if t.ndim != 2 or t.shape[1] != N:
        raise ValueError(f"measurements of shape {tuple(t.shape)} do not fit a bank of {N} track(s): (T, {N}) expected")
    return t.contiguous()


def host(t):
    return _transfer.to_host([t])[0]


def back(t, like):
    """a device result in the type of `like`: a tensor as it is, an array as an array, a number as a Python float"""
    if is_tensor(like):
        return t
    h = host(t)
    return float(h.reshape(-1)[0]) if np.ndim(like) == 0 else h


def run(order, form, dt, T2, c, g, x, z, *, layout="soa", gains=None, want=()):
    """T steps in one launch.  x: the device state in `layout`, updated in place; z: device (T, N); g: (g0, g1, g2); gains: None
    or a host (T, order + 1) table.  want: which of "xs", "pred", "y" to return (device tensors, in a dict)."""
    T, N = z.shape
    out = {k: (E.alloc_records((T,), N, order + 1, layout, z.device) if k == "xs"
               else torch.empty((T, N), dtype=torch.float64, device=z.device)) for k in want}
    table = None if gains is None else E.dev(np.ascontiguousarray(gains, dtype=np.float64).reshape(T, order + 1))
    E.poly_run(order, form, N, T, layout, dt, T2, c, g[0], g[1], g[2], z, x, gains=table,
               xs=out.get("xs"), pred=out.get("pred"), y=out.get("y"))
    return out


def pretty(label, arr):
    """`label = value`, the continuation lines of an array indented under its first"""
    label = label + " = "
    lines = str(arr).split("\n")
    return label + ("\n" + " " * len(label)).join(lines)
