"""tests/fls_port.py's fixed-lag smoother in extended precision (np.longdouble: the x87 80-bit format on x86-64, eps 1.08e-19),
vectorised over a set of tracks that share one model.  Same algorithm and operation order as the port (filterpy's
fixed_lag_smoother.py:217-311), so on any input it is the float64 arithmetic's "truth" up to ~1e-19 times the problem's
condition: the tests hold the GPU to `err(gpu, hp) <= max(4 err(fls_port, hp), floor)` per output, row and track.

    x0 (K, n)  P0 (K, n, n)  zs (T, K, m)  us (T, K, nu)   F, Q, H shared;  R (m, m) or a scalar;  B (n, nu) or a scalar

A scalar R follows numpy's rule, as the reference computes it and the kernels do with FK_KF_FLAG_R_JOSEPH_DIAG: `HPH' + r` adds r
to every element, `dot(K, r).dot(K.T)` is r K K'.  A scalar Q adds q to every element of FPF'; a scalar B is b u (u has n
entries).  A chained run is one long run: its truth is the truth of the whole run."""
import json
import os
import re

import numpy as np

LD = np.longdouble
assert np.finfo(LD).eps < 1e-18, "np.longdouble is no wider than float64 on this platform: fls_hp would not be a truth"


def ld(a):
    return np.asarray(a, dtype=LD)


def inv(S):
    """(K, m, m) -> (K, m, m): Gauss-Jordan with partial pivoting, in longdouble (np.linalg does not take it)"""
    S = ld(S)
    K, m, _ = S.shape
    A = np.concatenate([S, np.broadcast_to(np.eye(m, dtype=LD), (K, m, m))], axis=2)
    kk = np.arange(K)
    for c in range(m):
        p = c + np.argmax(np.abs(A[:, c:, c]), axis=1)
        rc, rp = A[kk, c].copy(), A[kk, p].copy()
        A[kk, p] = rc
        A[kk, c] = rp
        A[:, c] /= A[:, c, c][:, None]
        for r in range(m):
            if r != c:
                A[:, r] -= A[:, r, c][:, None] * A[:, c]
    return A[:, :, m:]


def _mv(A, v):
    """per-track A v: A (K, r, c) or (r, c), v (K, c)"""
    return np.einsum("...ij,...j->...i", A, v)


def smooth_batch(x0, P0, zs, lag, F, Q, H, R, B=None, us=None):
    """-> dict of longdouble arrays: xs (T, K, n), xhat (T, K, n), and after the last step x (K, n), P (K, n, n), y (K, m),
    S (K, m, m).  lag <= 0: xs are the priors; lag >= T: the filtered states (the reference's `k >= N`, `range(N)`)."""
    x, P = ld(x0).copy(), ld(P0).copy()
    zs = ld(zs)
    F, Q, H = ld(F), ld(Q), ld(H)
    scalar_R = np.ndim(R) == 0
    R = ld(R)
    T, K = zs.shape[0], x.shape[0]
    n, m = x.shape[1], zs.shape[2]
    I = np.eye(n, dtype=LD)
    if us is not None:
        us = ld(us)
        B = ld(B)
    xs = np.zeros((T, K, n), dtype=LD)
    xhat = np.zeros((T, K, n), dtype=LD)
    y = np.zeros((K, m), dtype=LD)
    S = np.zeros((K, m, m), dtype=LD)
    for k in range(T):
        x_pre = _mv(F, x)
        if us is not None:
            x_pre = x_pre + (B * us[k] if B.ndim == 0 else _mv(B, us[k]))
        P = (F @ P) @ F.T + Q
        y = zs[k] - _mv(H, x_pre)
        S = (H @ P) @ H.T + R
        SI = inv(S)
        Kg = (P @ H.T) @ SI
        x = x_pre + _mv(Kg, y)
        IKH = I - Kg @ H
        KRK = (Kg * R) @ np.swapaxes(Kg, 1, 2) if scalar_R else (Kg @ R) @ np.swapaxes(Kg, 1, 2)
        P = (IKH @ P) @ np.swapaxes(IKH, 1, 2) + KRK
        xhat[k] = x
        xs[k] = x_pre
        if k >= lag:
            HTSI = H.T @ SI
            F_LH = np.swapaxes(F - Kg @ H, 1, 2)
            PS = P.copy()
            for i in range(lag):
                Ks = PS @ HTSI
                PS = PS @ F_LH
                xs[k - i] += _mv(Ks, y)
        else:
            xs[k] = x
    return dict(xs=xs, xhat=xhat, x=x, P=P, y=y, S=S)


# ---- what the tests share ------------------------------------------------------------------------------------------------
DEF = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "filterpy_amd", "csrc", "fk_dims_fls.def")


def fast_entries():
    """the (NX, NZ, LMAX) of every FK_FLS_INST line of fk_dims_fls.def, in file order"""
    with open(DEF) as fh:
        return [tuple(int(v) for v in g) for g in re.findall(r"^FK_FLS_INST\(\s*(\d+)\s*,\s*(\d+)\s*,\s*(\d+)\s*\)", fh.read(), re.M)]


def random_model(n, m, K, T, seed, nu=0, scalar_R=False):
    """a benign shared model and K tracks: F near I, SPD Q and R, x0 ~ N(0, 1), P0 a multiple of I per track"""
    rs = np.random.RandomState(seed)
    F = np.eye(n) + 0.1 * rs.randn(n, n) / np.sqrt(n)
    A = rs.randn(n, n)
    Q = 0.01 * (A @ A.T + np.eye(n))
    H = rs.randn(m, n)
    Cr = rs.randn(m, m)
    R = 0.7 if scalar_R else 0.1 * (Cr @ Cr.T) + 0.8 * np.eye(m)
    x0 = rs.randn(K, n)
    P0 = np.eye(n)[None] * (1.0 + rs.rand(K, 1, 1))
    zs = rs.randn(T, K, m)
    B = us = None
    if nu:
        B = rs.randn(n, nu) / np.sqrt(nu)
        us = rs.randn(T, K, nu)
    return dict(F=F, Q=Q, H=H, R=R, x0=x0, P0=P0, zs=zs, B=B, us=us)


def row_errors(a, truth):
    """normwise relative error of every row (leading axis) of a against the longdouble truth"""
    t = ld(truth)
    d = (ld(a) - t).reshape(t.shape[0], -1)
    t = t.reshape(t.shape[0], -1)
    scale = np.max(np.abs(t), axis=1) if t.shape[1] else np.ones(t.shape[0], dtype=LD)
    scale[scale == 0] = 1
    return (np.max(np.abs(d), axis=1) / scale).astype(np.float64) if t.shape[1] else np.zeros(t.shape[0])


def assert_within_bar(what, got, port, truth, factor=4.0, floor=1e-12, family=None):
    """every row of `got` (one track's output: rows = steps, or one row for a final matrix) no further from the truth than
    `factor` times float64's own error in filterpy's order (`port`), or `floor`.  Returns the worst err / bar; with
    FK_PARITY_LOG set, appends it there."""
    eg, ep = row_errors(got, truth), row_errors(port, truth)
    bar = np.maximum(factor * ep, floor)
    ratio = eg / bar
    i = int(np.argmax(ratio)) if ratio.size else 0
    worst = float(ratio[i]) if ratio.size else 0.0
    path = os.environ.get("FK_PARITY_LOG")
    if path:
        with open(path, "a") as fh:
            fh.write(json.dumps({"test": os.environ.get("PYTEST_CURRENT_TEST", "").split(" ")[0], "family": family or what,
                                 "err": float(eg[i]) if eg.size else 0.0, "bar": float(bar[i]) if bar.size else floor,
                                 "ratio": worst}) + "\n")
    assert worst <= 1.0, (f"{what}: row {i} err(got, hp) = {eg[i]:.3e} > bar {bar[i]:.3e} "
                          f"(err(fls_port, hp) = {ep[i]:.3e})")
    return worst


def compare_track(tag, got, port, truth, k=0, family=None):
    """one track's xs, xhat (per step) and final x, P, y, S: `got` and `port` map names to that track's outputs, `truth` is
    smooth_batch's dict and k the track's index in it.  Names missing from `got` are not checked."""
    worst = 0.0
    for name in ("xs", "xhat", "x", "P", "y", "S"):
        if name not in got:
            continue
        t = truth[name][:, k] if name in ("xs", "xhat") else truth[name][k][None]
        g = np.asarray(got[name]).reshape(t.shape)
        p = np.asarray(port[name]).reshape(t.shape)
        worst = max(worst, assert_within_bar(f"{tag} {name}", g, p, t, family=family))
    return worst
