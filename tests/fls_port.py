"""NumPy restatement of filterpy.kalman.FixedLagSmoother (fixed_lag_smoother.py:133-311) for the tests: the reference's
arithmetic step by step, with no dependency on the reference checkout (the GPU box has none).  `smooth_batch` returns
(xSmooth, xhat) shaped like the reference's; `SmoothPort` keeps the state of the step-by-step smooth()."""
import numpy as np
from numpy import dot

try:                                        # the reference inverts S with scipy.linalg.inv (fixed_lag_smoother.py:23)
    from scipy.linalg import inv
except ImportError:                         # (numpy's LU inverse: a few ulps apart)
    from numpy.linalg import inv


def _step(x, P, z, F, Q, H, R, B, u, I):
    x_pre = dot(F, x)
    if u is not None:
        x_pre = x_pre + dot(B, u)
    P = dot(F, P).dot(F.T) + Q
    y = z - dot(H, x_pre)
    S = dot(H, P).dot(H.T) + R
    SI = inv(S)
    K = dot(P, H.T).dot(SI)
    x = x_pre + dot(K, y)
    I_KH = I - dot(K, H)
    P = dot(I_KH, P).dot(I_KH.T) + dot(K, R).dot(K.T)
    return x_pre, x, P, y, S, SI, K


def _lag_update(rows, k, N, P, H, SI, K, F, y):
    HTSI = dot(H.T, SI)
    F_LH = (F - dot(K, H)).T
    PS = P.copy()
    for i in range(N):
        Ks = dot(PS, HTSI)
        PS = dot(PS, F_LH)
        rows[k - i] = rows[k - i] + dot(Ks, y)


def smooth_batch(x, P, zs, N, F, Q, H, R, B=0., us=None):
    """fixed_lag_smoother.py:217-311 (x 1-D or a column, as the reference takes it)"""
    return smooth_batch_state(x, P, zs, N, F, Q, H, R, B, us)[:2]


def smooth_batch_state(x, P, zs, N, F, Q, H, R, B=0., us=None):
    """smooth_batch, plus the state after the last step: (xSmooth, xhat, x, P, y, S)"""
    x = np.asarray(x, dtype=float)
    n = x.shape[0]
    I = np.eye(n)
    T = len(zs)
    xSmooth = np.zeros((T,) + x.shape)
    xhat = np.zeros((T,) + x.shape)
    y = S = None
    for k, z in enumerate(zs):
        x_pre, x, P, y, S, SI, K = _step(x, P, z, F, Q, H, R, B, None if us is None else us[k], I)
        xhat[k] = x.copy()
        xSmooth[k] = x_pre.copy()
        if k >= N:
            _lag_update(xSmooth, k, N, P, H, SI, K, F, y)
        else:
            xSmooth[k] = xhat[k]
    return xSmooth, xhat, x, P, y, S


class SmoothPort:
    """fixed_lag_smoother.py:133-215, one call per step"""

    def __init__(self, x, P, N, F, Q, H, R, B=0.):
        self.x, self.P, self.N = np.asarray(x, dtype=float).copy(), np.asarray(P, dtype=float).copy(), N
        self.F, self.Q, self.H, self.R, self.B = F, Q, H, R, B
        self.xSmooth, self.count, self.y, self.S = [], 0, None, None

    def smooth(self, z, u=None):
        k, N = self.count, self.N
        x_pre, x, P, y, S, SI, K = _step(self.x, self.P, z, self.F, self.Q, self.H, self.R, self.B, u, np.eye(len(self.x)))
        self.y, self.S = y, S
        self.xSmooth.append(x_pre.copy())
        if k >= N:
            _lag_update(self.xSmooth, k, N, P, self.H, SI, K, self.F, y)
        else:
            self.xSmooth[k] = x.copy()
        self.count += 1
        self.x, self.P = x, P
