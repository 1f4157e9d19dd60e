"""The hard models of the cubature filter's precision tests (tests/test_gpu_ckf_precision.py on the GPU, tests/test_host_ckf.py
for the host-compiled step that fixes the bar's factor K_BAR) and the error measure they share.

Models: ill-scaled states, D = diag(10^-2 .. 10^2): F = D Fs D^-1 with Fs orthogonal (a small random rotation), H = Hs D^-1 with
Hs random, Q = D diag(1e-3 .. 1e-1) D, R = 0.5 I.  Per track P0 = D C D with C a well-conditioned correlation-like matrix:
condition 1e8; the state
mean starts up to 1e3 spreads away from the origin (x0_i = 1e3 sqrt(P0_ii) u, u uniform in [-1, 1]) -- where the reference's
uncentred second moment sum (X X' - x x') cancels six digits.  The measurements follow a simulated truth.  On these models the
float64 port's own worst-track error against longdouble stays below 1e-6 on P for all 30 steps (test_host_ckf.py asserts it)."""
import numpy as np

import ckf_hp

DIMS = [(2, 1), (4, 2), (6, 3), (9, 4), (12, 4)]
NT, T = 32, 30
OUTPUTS = ("means", "covs", "means_p", "covs_p")

# The bar: err(kernel, hp) <= max(K_BAR * max_tracks err(ckf_port, hp), 1e-12) per track, and the medians K_BAR apart at most.
# K_BAR = 2 * (the worst per-output ratio of the host-compiled fk_ckf.hpp step to the port on exactly these models, 0.00114
# -- the means of (12, 4); the covariances 0.0003 .. 0.0008: tests/test_host_ckf.py measures it and holds it below K_BAR / 2),
# rounded up to a power of two.  Far below one: the port (like the reference) sums X X' - x x' with the means 1e3 spreads out and
# loses six digits there, fk_ckf.hpp sums the +- pairs' half-differences and never forms the cancelling terms.
K_BAR = 2.0 ** -8


def model(dims):
    n, m = dims
    rs = np.random.RandomState(n * 10 + m)
    D = 10.0 ** np.linspace(-2, 2, n)
    Fs = np.linalg.qr(np.eye(n) + 0.1 * rs.randn(n, n))[0]          # orthogonal: the offsets neither grow nor die out
    F = Fs * D[:, None] / D[None, :]
    H = rs.randn(m, n) / D[None, :]
    Q = np.diag(D * D * 10.0 ** rs.uniform(-3, -1, n))
    R = np.eye(m) * 0.5
    P0 = np.zeros((NT, n, n))
    x0 = np.zeros((NT, n))
    zs = np.zeros((T, NT, m))
    for i in range(NT):
        A = rs.randn(n, n)
        C = A @ A.T / n + np.eye(n)
        P0[i] = (C * D[:, None]) * D[None, :]
        P0[i] = (P0[i] + P0[i].T) / 2
        x0[i] = 1e3 * np.sqrt(np.diag(P0[i])) * rs.uniform(-1, 1, n)
        xt = x0[i] + np.linalg.cholesky(P0[i]) @ rs.randn(n)
        for t in range(T):
            xt = F @ xt
            zs[t, i] = H @ xt + np.sqrt(0.5) * rs.randn(m)
    return dict(n=n, m=m, F=F, H=H, Q=Q, R=R, x0=x0, P0=P0, zs=zs)


def err(a, hp):
    """worst normwise relative error over the steps, measured in longdouble"""
    d = np.abs(np.asarray(a, dtype=ckf_hp.LD) - hp).reshape(len(hp), -1).max(axis=1)
    return float(np.max(d / np.maximum(np.abs(hp).reshape(len(hp), -1).max(axis=1), 1e-300)))


_truth = {}


def truth(dims):
    """(hp, port errors): per track the longdouble histories, and err(ckf_port, hp) as a (4, NT) array; computed once"""
    if dims not in _truth:
        import ckf_port
        d = model(dims)
        hps, ep = [], np.zeros((4, NT))
        for i in range(NT):
            hp = ckf_hp.batch(d["x0"][i], d["P0"][i], d["zs"][:, i], d["F"], d["Q"], d["H"], d["R"])
            port = ckf_port.batch(d["x0"][i], d["P0"][i], d["zs"][:, i], d["F"], d["Q"], d["H"], d["R"])
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
