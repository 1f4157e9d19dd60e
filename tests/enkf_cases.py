"""What the CPU and the GPU tests of EnsembleKalmanFilter share: the golden cases of tests/golden/enkf.npz built as filters in
each way fx / hx can be given, the recorded draws replayed through the filter's own call sites, and the comparison of every
attribute after every call."""
import numpy as np

from conftest import golden, rel_err
import enkf_port as ep

G = golden("enkf")
NC = int(G["n_cases"])
MODES = ("callable", "vectorized", "matrix", "device")


class Replay:
    """stands in for numpy.random.multivariate_normal / a `noise` callable: hands out op k's recorded draw and holds the
    request to the recorded (mean, cov, size) -- the call sites and their order are the reference's, or this fails"""

    def __init__(self, c, as_tensor=None):
        self.c, self.k, self.calls, self.as_tensor = c, 0, 0, as_tensor

    def __call__(self, mean, cov, size):
        i = ep.op_inputs(G, self.c, self.k)
        assert i["draw"] is not None, ("a draw was asked for in an op that has none", self.k)
        assert size == self.c["N"] and np.array_equal(np.asarray(mean, dtype=float), i["mean"]), (self.k, mean, i["mean"])
        assert np.array_equal(np.asarray(cov, dtype=float), i["cov"]), (self.k, cov, i["cov"])
        self.calls += 1
        return i["draw"].copy() if self.as_tensor is None else self.as_tensor(i["draw"])


def model_kw(c, mode, device=None):
    import torch
    F, H = c["F"], c["H"]
    if mode == "callable":
        return dict(fx=lambda s, dt: np.dot(F, s), hx=lambda s: np.dot(H, s))
    if mode == "vectorized":
        return dict(fx=lambda S, dt: S @ F.T, hx=lambda S: S @ H.T, vectorized=True)
    if mode == "matrix":
        return dict(fx=F.copy(), hx=H.copy())
    Ft, Ht = torch.as_tensor(F.T.copy(), device=device), torch.as_tensor(H.T.copy(), device=device)
    return dict(fx=lambda S, dt: S @ Ft, hx=lambda S: S @ Ht, device_callables=True)


def make_filter(c, mode, layout, noise, device=None):
    from filterpy_amd.kalman import EnsembleKalmanFilter
    f = EnsembleKalmanFilter(x=c["x0"].copy(), P=c["P0"].copy(), dim_z=c["m"], dt=1., N=c["N"], noise=noise, layout=layout,
                             **model_kw(c, mode, device))
    f.Q, f.R = c["Q"].copy(), c["R"].copy()
    return f


def check_attrs(f, c, k, tol):
    for a in ep.ATTRS:
        want, got = ep.attr(G, c, k, a), np.asarray(getattr(f, a))
        assert got.shape == want.shape and got.dtype == np.float64, (k, a, got.shape, want.shape)
        assert rel_err(got, want) <= tol, (c["p"], k, a, rel_err(got, want))
    z_none = bool(ep.attr(G, c, k, "z_is_none"))
    if z_none:
        assert f.z.shape == (c["m"], 1) and f.z[0, 0] is None
    else:
        last = max(j for j in range(k + 1) if ep.op_inputs(G, c, j)["z"] is not None)      # z stays until the next update
        assert np.array_equal(f.z, ep.op_inputs(G, c, last)["z"])
    assert f.sigmas_device.shape == ((c["n"], c["N"]) if f.layout == "soa" else (c["N"], c["n"]))


def run_case(ci, mode, layout, tol, noise_kind="callable", monkeypatch=None, device=None, as_tensor=None):
    """every op of golden case ci through the class, the draws replayed; every attribute after every call within tol"""
    c = ep.case(G, ci)
    rp = Replay(c, as_tensor)
    if noise_kind == "numpy":
        monkeypatch.setattr(np.random, "multivariate_normal", rp)
    f = make_filter(c, mode, layout, "numpy" if noise_kind == "numpy" else rp, device)
    draws = 1
    check_attrs(f, c, 0, tol)
    for k, op in enumerate(c["ops"]):
        if k == 0:
            continue
        rp.k = k
        ep.run_op(f, c, k, op, G)
        draws += op != ep.UPDATE_NONE
        assert rp.calls == draws, (k, op, rp.calls)
        check_attrs(f, c, k, tol)
    return f
