"""A CPU stand-in for fk_poly_run: HOST-LOGIC tests of filterpy_amd.gh / .memory / .leastsq only.  The arithmetic inside is
tests/poly_port.py's; the kernels themselves are tested under -m gpu and, compiled for the host, by
tests/test_hostcheck_poly.py."""
import numpy as np
import torch

import poly_port as pp

CPU = torch.device("cpu")


def install(monkeypatch):
    """-> the list of calls, one dict(order, form, N, T, layout, table, outs) per launch"""
    from filterpy_amd import _engine as E
    calls = []

    def poly_run(order, form, N, T, layout, dt, T2, c, g0, g1, g2, z, x, *, gains=None, xs=None, pred=None, y=None):
        assert (order, form) in pp.COMBOS, (order, form)
        C = order + 1
        assert z.shape == (T, N) and x.numel() == C * N and z.is_contiguous() and x.is_contiguous()
        calls.append(dict(order=order, form=form, N=N, T=T, layout=layout, table=gains is not None,
                          outs=tuple(k for k, v in (("xs", xs), ("pred", pred), ("y", y)) if v is not None),
                          scalars=(dt, T2, c, g0, g1, g2)))
        x0 = x.numpy().reshape(C, N) if layout == "soa" else x.numpy().reshape(N, C).T
        hx, hp, hy = pp.run(order, form, x0, z.numpy(), dt, T2, c, (g0, g1, g2), None if gains is None else gains.numpy().reshape(T, C))
        if T:
            x.copy_(torch.as_tensor(np.ascontiguousarray(hx[-1] if layout == "soa" else hx[-1].T)).reshape(x.shape))
        if xs is not None:
            xs.copy_(torch.as_tensor(np.ascontiguousarray(hx if layout == "soa" else np.swapaxes(hx, 1, 2))).reshape(xs.shape))
        if pred is not None:
            pred.copy_(torch.as_tensor(hp))
        if y is not None:
            y.copy_(torch.as_tensor(hy))

    monkeypatch.setattr(E, "require_gpu", lambda: CPU)
    monkeypatch.setattr(E, "dev", lambda a, device=None: (a.to(dtype=torch.float64).contiguous() if isinstance(a, torch.Tensor)
                                                          else torch.as_tensor(np.array(a, dtype=np.float64))))
    monkeypatch.setattr(E, "alloc_records", lambda lead, N, Ee, layout, device=None:
                        torch.full((*lead, N, Ee) if layout == "aos" else (*lead, Ee, N), float("nan"), dtype=torch.float64))
    monkeypatch.setattr(E, "poly_run", poly_run)
    return calls
