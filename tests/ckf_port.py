"""NumPy restatement of filterpy/kalman/CubatureKalmanFilter.py in the reference's own summation order -- the truth of the
cubature filter's tests where the live reference is not at hand (the GPU machine), held against goldens frozen from the live
reference by tests/test_host_ckf.py.

    spherical_radial_sigmas  :32-61     ckf_transform  :64-98     predict  :292-327     update  :329-390

`chol` (upper factor) and `inv` are parameters so that tests/ckf_hp.py runs the same lines in longdouble.  Also here: the
callables and call sequences of the golden cases (tests/golden/make_ckf_golden.py runs them on the live reference) and the
reader of tests/golden/ckf.npz.
"""
import math

import numpy as np


def _chol_upper(P):
    from scipy.linalg import cholesky          # the reference's own (:27): LAPACK's upper factor, to the bit
    return cholesky(P)


def _inv(A):
    from scipy.linalg import inv
    return inv(A)


def spherical_radial_sigmas(x, P, chol=_chol_upper):
    """:52-61"""
    n = P.shape[0]
    x = np.ravel(x)
    sigmas = np.empty((2 * n, n), dtype=P.dtype)
    U = chol(P) * np.sqrt(P.dtype.type(n))
    for k in range(n):
        sigmas[k] = x + U[k]
        sigmas[n + k] = x - U[k]
    return sigmas


def ckf_transform(Xs, Q):
    """:87-98"""
    m, n = Xs.shape
    x = sum(Xs, 0)[:, None] / m
    P = np.zeros((n, n), dtype=Xs.dtype)
    xf = x.flatten()
    for k in range(m):
        P += np.outer(Xs[k], Xs[k]) - np.outer(xf, xf)
    P *= Xs.dtype.type(1) / m
    P += Q
    return x, P


def outer_product_sum(A, B):
    """filterpy/common/helpers.py outer_product_sum: sum_k outer(A[k], B[k])"""
    return np.sum(np.einsum('ij,ik->ijk', A, B), axis=0)


class Port(object):
    """the reference's object, attribute for attribute (:240-290), without the lazy likelihoods"""

    def __init__(self, dim_x, dim_z, dt, hx, fx, residual_z=None, dtype=float, chol=_chol_upper, inv=_inv):
        T = dtype
        self.dim_x, self.dim_z, self._dt, self.hx, self.fx = dim_x, dim_z, dt, hx, fx
        self.Q, self.R = np.eye(dim_x, dtype=T), np.eye(dim_z, dtype=T)
        self.x, self.P = np.zeros(dim_x, dtype=T), np.eye(dim_x, dtype=T)
        self.K, self.y = 0, 0
        self.z = np.array([[None] * dim_z]).T
        self.S, self.SI = np.zeros((dim_z, dim_z), dtype=T), np.zeros((dim_z, dim_z), dtype=T)
        self.residual_z = np.subtract if residual_z is None else residual_z
        self.sigmas_f, self.sigmas_h = np.zeros((2 * dim_x, dim_x), dtype=T), np.zeros((2 * dim_x, dim_z), dtype=T)
        self.x_prior, self.P_prior, self.x_post, self.P_post = self.x.copy(), self.P.copy(), self.x.copy(), self.P.copy()
        self._T, self._chol, self._inv = T, chol, inv

    def predict(self, dt=None, fx_args=()):
        """:311-327"""
        if dt is None:
            dt = self._dt
        if not isinstance(fx_args, tuple):
            fx_args = (fx_args,)
        sigmas = spherical_radial_sigmas(self.x, self.P, self._chol)
        for k in range(2 * self.dim_x):
            self.sigmas_f[k] = self.fx(sigmas[k], dt, *fx_args)
        self.x, self.P = ckf_transform(self.sigmas_f, self.Q)
        self.x_prior, self.P_prior = self.x.copy(), self.P.copy()

    def update(self, z, R=None, hx_args=()):
        """:348-385"""
        if z is None:
            self.z = np.array([[None] * self.dim_z]).T
            self.x_post, self.P_post = self.x.copy(), self.P.copy()
            return
        if not isinstance(hx_args, tuple):
            hx_args = (hx_args,)
        if R is None:
            R = self.R
        elif np.isscalar(R):
            R = np.eye(self.dim_z, dtype=self._T) * R
        for k in range(2 * self.dim_x):
            self.sigmas_h[k] = self.hx(self.sigmas_f[k], *hx_args)
        zp, self.S = ckf_transform(self.sigmas_h, R)
        self.SI = self._inv(self.S)
        m = 2 * self.dim_x
        xf, zpf = self.x.flatten(), zp.flatten()
        Pxz = outer_product_sum(self.sigmas_f - xf, self.sigmas_h - zpf) / m
        self.K = np.dot(Pxz, self.SI)
        self.y = self.residual_z(z, zp)
        self.x = self.x + np.dot(self.K, self.y)
        self.P = self.P - np.dot(self.K, self.S).dot(self.K.T)
        self.z = np.array(z, copy=True)
        self.x_post, self.P_post = self.x.copy(), self.P.copy()


def batch(x0, P0, zs, F, Q, H, R, mask=None, dtype=float, chol=_chol_upper, inv=_inv, sigmas_f=None):
    """One track on the matrix model fx = F, hx = H, predict then update per step: (means (T, n), covs (T, n, n), means_p,
    covs_p, the filter).  mask[t] False: update(None).  sigmas_f: the points an earlier predict left (chained runs)."""
    F, Q, H, R = (np.asarray(a, dtype=dtype) for a in (F, Q, H, R))
    n, m = F.shape[0], H.shape[0]
    f = Port(n, m, 1.0, lambda s: H @ s, lambda s, dt: F @ s, dtype=dtype, chol=chol, inv=inv)
    f.x, f.P, f.Q, f.R = np.asarray(x0, dtype=dtype).reshape(n, 1).copy(), np.asarray(P0, dtype=dtype).copy(), Q, R
    if sigmas_f is not None:
        f.sigmas_f = np.asarray(sigmas_f, dtype=dtype).copy()
    T = len(zs)
    out = [np.zeros((T, n), dtype), np.zeros((T, n, n), dtype), np.zeros((T, n), dtype), np.zeros((T, n, n), dtype)]
    for t in range(T):
        f.predict()
        out[2][t], out[3][t] = f.x[:, 0], f.P
        if mask is None or mask[t]:
            f.update(np.asarray(zs[t], dtype=dtype).reshape(m, 1))
        out[0][t], out[1][t] = f.x[:, 0], f.P
    return out + [f]


def batch_tracks(x0, P0, zs, F, Q, H, R, mask=None):
    """batch() per track: x0 (N, n), P0 (N, n, n), zs (T, N, m), mask (T, N) -> the four histories (T, N, ...)"""
    N = len(x0)
    res = [batch(x0[i], P0[i], zs[:, i], F, Q, H, R, None if mask is None else mask[:, i])[:4] for i in range(N)]
    return [np.stack([r[j] for r in res], axis=1) for j in range(4)]


# ---- the callables of the golden cases: NumPy arrays or torch tensors, one point (d,) or any leading axes (..., d) ------------
def _xp(x):
    if isinstance(x, np.ndarray):
        return np
    import torch
    return torch


def fx_lin(x, dt, F):
    """a matrix model handed over as a callable with an argument: x (..., n) -> F x"""
    if isinstance(x, np.ndarray):
        return x @ np.asarray(F).T
    import torch
    return x @ torch.as_tensor(np.asarray(F, dtype=float), device=x.device).T


def hx_lin(x, H):
    return fx_lin(x, None, H)


def fx_poly(x, dt, a=0.02):
    """polynomial: x_i + 0.1 dt x_{i+1} + a dt x_i^2"""
    xp = _xp(x)
    return x + 0.1 * dt * xp.roll(x, -1, -1) + a * dt * x * x


def hx_rb(x, m, p=5.0, q=-4.0):
    """range / bearing style: output r is sqrt(a^2 + b^2 + 1) (r even) or atan2(b, a) (r odd) of a = x[r] - p, b = x[r+1] - q
    (indices mod n)"""
    xp = _xp(x)
    n = x.shape[-1]
    out = []
    for r in range(m):
        a, b = x[..., r % n] - p, x[..., (r + 1) % n] - q
        out.append(xp.sqrt(a * a + b * b + 1.0) if r % 2 == 0 else (np.arctan2(b, a) if xp is np else xp.atan2(b, a)))
    return xp.stack(out, -1)


def residual_wrap(a, b):
    """a custom residual_z: a - b with the odd (bearing) rows wrapped into [-pi, pi); rows on axis 0 for columns (m, 1) and one
    point (m,), on the last axis for (N, m)"""
    d = a - b
    xp = _xp(d)
    on0 = d.ndim == 1 or d.shape[-1] == 1          # (m,) / (m, 1) against (N, m) with m >= 2; m = 1 has no bearing row
    rows = d.shape[0] if on0 else d.shape[-1]
    d = d.copy() if xp is np else d.clone()
    for r in range(1, rows, 2):
        if on0:
            d[r] = (d[r] + math.pi) % (2 * math.pi) - math.pi
        else:
            d[..., r] = (d[..., r] + math.pi) % (2 * math.pi) - math.pi
    return d


# ---- the golden cases ---------------------------------------------------------------------------------------------------------
DIMS = [(1, 1), (2, 1), (2, 2), (4, 2), (6, 3), (9, 4), (12, 4), (16, 8)]
# ops: 0 predict(), 1 predict(dt=DT2), 2 update(z), 3 update(None), 4 update(z, R=R2 matrix), 5 update(z, R=R_SCALAR)
PREDICT, PREDICT_DT, UPDATE, UPDATE_NONE, UPDATE_R, UPDATE_RS = range(6)
SEQ = ([0, 2, 1, 4, 0, 3, 0, 5, 0, 2, 2],        # predict first; a dt override, R as a matrix, update(None), R as a scalar, two
       [2, 0, 2, 1, 5, 0, 3, 0, 4, 0, 2, 2])     # updates after one predict (last: P may lose definiteness) / an update before any predict
DT, DT2, R_SCALAR = 0.5, 0.8, 0.7
ATTRS = ("x", "P", "x_prior", "P_prior", "x_post", "P_post", "K", "y", "S", "SI", "sigmas_f", "sigmas_h",
         "log_likelihood", "likelihood", "mahalanobis")
LINEAR, NONLINEAR = 0, 1


def spd(rs, k, scale=1.0):
    a = rs.randn(k, k)
    return scale * (a @ a.T / k + 0.5 * np.eye(k))


def specs():
    """(ci, n, m, kind, seq, custom residual_z) of every golden case"""
    out = []
    for n, m in DIMS:
        for kind in (LINEAR, NONLINEAR):
            ci = len(out)
            out.append((ci, n, m, kind, (ci // 2 + kind) % 2, int(kind == NONLINEAR and (ci // 2) % 2 == 0)))
    return out


def n_ops(spec):
    """calls of a case: the whole sequence, the first eight at dim_x >= 12 (the fixture's size)"""
    return 8 if spec[1] >= 12 else len(SEQ[spec[4]])


def inputs(ci, n, m, kind):
    """the model and measurements of case ci (drawn here so that the generator and the tests share one definition)"""
    rs = np.random.RandomState(5000 + ci)
    d = dict(F=np.eye(n) + 0.1 * rs.randn(n, n) / np.sqrt(n), H=rs.randn(m, n), Q=spd(rs, n, 0.02), R=spd(rs, m, 0.5),
             R2=spd(rs, m, 0.8), P0=spd(rs, n, 0.6), x0=rs.randn(n))
    d["zs"] = rs.randn(max(len(s) for s in SEQ), m) * (2.0 if kind == LINEAR else 0.5)
    if kind == NONLINEAR:
        d["zs"][:, 0::2] += 6.5                   # ranges near |(-5, 4)|, bearings near 2.5 (+- pi to make the wrap matter)
        d["zs"][:, 1::2] += 2.5
        if (ci // 2) % 2 == 0:                    # the cases with residual_wrap (specs): every other bearing a turn away
            d["zs"][1::2, 1::2] -= 2 * math.pi
    return d


def callables(kind, d, m):
    """fx, hx, fx_args, hx_args of a case"""
    if kind == LINEAR:
        return fx_lin, hx_lin, (d["F"],), (d["H"],)
    return fx_poly, hx_rb, (0.03,), (m, 5.0, -4.0)


def setup(f, spec, d):
    """a fresh filter object (the reference's, the port or ours) -> configured for the case"""
    ci, n, m, kind, seq, custom = spec
    f.Q, f.R, f.P = d["Q"].copy(), d["R"].copy(), d["P0"].copy()
    f.x = d["x0"].copy() if SEQ[seq][0] in (PREDICT, PREDICT_DT) else d["x0"].reshape(n, 1).copy()
    return f


def run_op(f, spec, d, k):
    ci, n, m, kind, seq, custom = spec
    op = SEQ[seq][k]
    _, _, fa, ha = callables(kind, d, m)
    z = d["zs"][k].reshape(m, 1)
    if op == PREDICT:
        f.predict(fx_args=fa)
    elif op == PREDICT_DT:
        f.predict(dt=DT2, fx_args=fa)
    elif op == UPDATE:
        f.update(z, hx_args=ha)
    elif op == UPDATE_NONE:
        f.update(None)
    elif op == UPDATE_R:
        f.update(z, R=d["R2"], hx_args=ha)
    elif op == UPDATE_RS:
        f.update(z, R=R_SCALAR, hx_args=ha)
    return op


def make(cls, spec, d, **kw):
    ci, n, m, kind, seq, custom = spec
    fx, hx, _, _ = callables(kind, d, m)
    return setup(cls(n, m, DT, hx, fx, residual_z=residual_wrap if custom else None, **kw), spec, d)


def attr(G, p, k, a):
    """attribute a after call k of the sequence with prefix p: the latest stored k' <= k (the generator does not repeat an
    unchanged array); None where the reference cannot give it yet (mahalanobis before the first update)"""
    for kk in range(k, -1, -1):
        key = f"{p}k{kk}_{a}"
        if key in G.files:
            return G[key]
    return None
