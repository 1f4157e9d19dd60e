"""The hard models of the information filter's precision tests (tests/test_gpu_info_precision.py on the GPU,
tests/test_host_info.py for the host-compiled step that fixes the bar's factor K_BAR) and the error measure they share.

Models: F, H, Q and zs as tests/test_gpu_srkf_precision.py draws them, R_inv = 1e2 I and a nearly uninformative prior per
track, P_inv0 = 10^u I with u uniform in [-7, -4]: the information added by one measurement is 1e6 .. 1e9 times the prior's.
The float64 port's own worst-track error against longdouble on these models is 0.9e-6 .. 3.5e-6 on the means and
3e-8 .. 1.5e-6 on P_inv."""
import numpy as np

import info_hp

DIMS = [(2, 1), (4, 2), (6, 3), (9, 3), (12, 4)]
NT, T = 64, 25
OUTPUTS = ("means", "P_invs", "means_p", "P_invs_p")

# The bar: err(kernel, hp) <= max(K_BAR * max_tracks err(info_port, hp), 1e-12) per track, and the medians K_BAR apart at most.
# K_BAR = 2 * (the worst per-output ratio of the host-compiled fk_info.hpp step to the port on exactly these models, 3.75:
# tests/test_host_info.py measures it and holds it below K_BAR / 2), rounded up to a power of two -- doubled because the device
# contracts differently and takes its pivot reciprocals from refined seeds.
K_BAR = 8


def model(dims):
    n, m = dims
    rs = np.random.RandomState(n * 10 + m)
    F = np.eye(n) + np.diag(np.ones(n - 1), 1) * 0.5 + 0.01 * rs.randn(n, n)
    H = rs.randn(m, n)
    Q = np.diag(10.0 ** rs.uniform(-8, -2, n))
    Rinv = np.eye(m) * 1e2
    x0 = rs.randn(NT, n)
    Pinv0 = np.eye(n)[None] * (10.0 ** rs.uniform(-7, -4, NT))[:, None, None]
    zs = rs.randn(T, NT, m) * 100
    return dict(n=n, m=m, F=F, H=H, Q=Q, Rinv=Rinv, x0=x0, Pinv0=Pinv0, zs=zs)


def err(a, hp):
    """worst normwise relative error over the steps, measured in longdouble"""
    d = np.abs(np.asarray(a, dtype=info_hp.LD) - hp).reshape(len(hp), -1).max(axis=1)
    return float(np.max(d / np.maximum(np.abs(hp).reshape(len(hp), -1).max(axis=1), 1e-300)))


_truth = {}


def truth(dims):
    """(hp, port errors): per track the longdouble histories, and err(info_port, hp) as a (4, NT) array; computed once"""
    if dims not in _truth:
        import info_port
        d = model(dims)
        hps, ep = [], np.zeros((4, NT))
        for i in range(NT):
            hp = info_hp.batch(d["x0"][i], d["Pinv0"][i], d["zs"][:, i], d["F"], d["Q"], d["H"], d["Rinv"])
            port = info_port.batch(d["x0"][i], d["Pinv0"][i], d["zs"][:, i], d["F"], d["Q"], d["H"], d["Rinv"])
            hps.append(hp)
            for j in range(4):
                ep[j, i] = err(port[j], hp[j])
        _truth[dims] = (hps, ep)
    return _truth[dims]


def errors(out, dims):
    """err(out, hp) per output and track, (4, NT); out: the four histories (T, NT, ...)"""
    hps, _ = truth(dims)
    eg = np.zeros((4, NT))
    for i in range(NT):
        for j in range(4):
            eg[j, i] = err(out[j][:, i], hps[i][j])
    return eg
