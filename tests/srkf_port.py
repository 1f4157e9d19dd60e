"""NumPy restatement of filterpy.kalman.SquareRootKalmanFilter (square_root.py:172-248) for the tests, with a Householder QR of
its own in LAPACK's convention (dgeqr2 / dlarfg: R[j, j] = -sign(alpha) |column|; nothing reflected when the sub-column is
exactly zero or the column is the last row's) -- no dependency on the reference checkout or on scipy's qr (the GPU box has no
reference).  One track per call; `batch` runs the time loop the way fk_srkf_batch_f64 does."""
import numpy as np


def qr_r(A):
    """R of A (M x N, M >= N) as scipy.linalg.qr(A)[1] returns it: (M, N), zeros below the diagonal"""
    A = np.array(A, dtype=float)
    M, N = A.shape
    for j in range(min(M, N)):
        if M - j <= 1:
            continue                              # dlarfg with n = 1: nothing to reflect
        alpha, x = A[j, j], A[j + 1:, j]
        if not np.any(x != 0):
            continue                              # an exactly zero sub-column: tau = 0, R keeps alpha
        beta = -np.copysign(np.hypot(alpha, np.linalg.norm(x)), alpha)
        tau = (beta - alpha) / beta
        v = x / (alpha - beta)
        A[j, j] = beta
        A[j + 1:, j] = 0.0
        w = A[j, j + 1:] + v @ A[j + 1:, j + 1:]
        A[j, j + 1:] -= tau * w
        A[j + 1:, j + 1:] -= tau * np.outer(v, w)
    return np.triu(A)


def predict(x, L, F, Q12, B=None, u=None):
    """square_root.py:226-248 on x (n,), L = P1_2 (n, n)"""
    n = len(x)
    x = F @ x
    if B is not None:
        x = x + B @ u
    R = qr_r(np.hstack([F @ L, Q12]).T)
    return x, R[:n, :n].T.copy()


def update(x, L, z, H, R12):
    """square_root.py:172-224 -> x, L, y, K, S1_2, SI1_2"""
    m, n = H.shape
    M = np.zeros((m + n, m + n))
    M[:m, :m] = R12.T
    M[m:, :m] = (H @ L).T
    M[m:, m:] = L.T
    r = qr_r(M)
    S12 = r[:m, :m].T.copy()
    SI12 = np.linalg.pinv(S12)
    K = r[:m, m:].T @ SI12
    y = z - H @ x
    return x + K @ y, r[m:, m:].T.copy(), y, K, S12, SI12


def batch(x0, L0, zs, F, Q12, H, R12, B=None, us=None, mask=None, update_first=False):
    """fk_srkf_batch_f64 for one track: (means, sqrt_covs, means_p, sqrt_covs_p, last) with last = (x, L, y, K, S1_2, SI1_2)
    of the last update (None if none)"""
    x, L = np.array(x0, dtype=float), np.array(L0, dtype=float)
    T, n = len(zs), len(x)
    mu, cov, mu_p, cov_p = np.zeros((T, n)), np.zeros((T, n, n)), np.zeros((T, n)), np.zeros((T, n, n))
    last = None
    for t in range(T):
        if not update_first:
            x, L = predict(x, L, F, Q12, B, None if us is None else us[t])
            mu_p[t], cov_p[t] = x, L
        if mask is None or mask[t]:
            last = update(x, L, zs[t], H, R12)
            x, L = last[0], last[1]
        mu[t], cov[t] = x, L
        if update_first:
            x, L = predict(x, L, F, Q12, B, None if us is None else us[t])
            mu_p[t], cov_p[t] = x, L
    return mu, cov, mu_p, cov_p, last


# ---- the goldens (tests/golden/srkf.npz, tests/golden/make_srkf_golden.py) ----------------------------------------------------
ATTRS = ("x", "_P1_2", "x_prior", "_P1_2_prior", "x_post", "_P1_2_post", "K", "y", "S1_2", "SI1_2", "M")
PREDICT, PREDICT_U, UPDATE, UPDATE_NONE, UPDATE_R2, UPDATE_R2_SCALAR = range(6)
R2_SCALAR = 0.8


def case(G, ci):
    p = f"c{ci}_"
    n, m, nd, ctrl, order = (int(v) for v in G[p + "spec"])
    d = dict(p=p, n=n, m=m, nd=nd, ctrl=ctrl, order=order, ops=[int(o) for o in G[p + "ops"]])
    for k in ("F", "H", "Q", "R", "P0", "x0", "R2", "zs", "us", "B"):
        if p + k in G.files:
            d[k] = G[p + k]
    if "B" in d and d["B"].ndim == 0:
        d["B"] = float(d["B"])
    return d


def attr(G, p, k, a):
    """attribute a after call k (the generator stores an array only when it changed)"""
    for kk in range(k, -1, -1):
        key = f"{p}k{kk}_{a}"
        if key in G.files:
            return G[key]
    raise KeyError(f"{p} {a} before call {k}")


def run_op(f, c, k, op):
    """call k of golden case c on a filter object with the reference's interface (ours or the reference's)"""
    col = (lambda v: v) if c["nd"] == 1 else (lambda v: v.reshape(-1, 1))
    if op == PREDICT:
        f.predict()
    elif op == PREDICT_U:
        f.predict(col(c["us"][k]))
    elif op == UPDATE:
        f.update(col(c["zs"][k]))
    elif op == UPDATE_NONE:
        f.update(None)
    elif op == UPDATE_R2:
        f.update(col(c["zs"][k]), R2=c["R2"])
    else:
        f.update(col(c["zs"][k]), R2=R2_SCALAR)


def setup(f, c):
    """the case's attributes on a fresh filter object (setters factor P, Q, R)"""
    f.F, f.H, f.Q, f.R, f.P = c["F"], c["H"], c["Q"], c["R"], c["P0"]
    f.x = c["x0"].copy() if c["nd"] == 1 else c["x0"].reshape(-1, 1).copy()
    if "B" in c:
        f.B = c["B"]
    return f


class Port:
    """the port behind the reference's object interface (x as given, factors from numpy's lower Cholesky)"""

    def __init__(self, n, m):
        self.n, self.m = n, m
        self.B = 0.

    def set(self, c):
        self.F, self.H = c["F"], c["H"]
        self.Q12, self.R12, self.L = (np.linalg.cholesky(c[k]) for k in ("Q", "R", "P0"))
        self.x = c["x0"].astype(float).copy()
        self.B = c.get("B", 0.)
        self.K = self.y = self.S12 = self.SI12 = None
        return self

    def predict(self, u=None):
        if u is None:
            self.x, self.L = predict(self.x, self.L, self.F, self.Q12)
        else:
            u = np.ravel(u)
            B = self.B if np.ndim(self.B) else np.eye(self.n) * self.B
            self.x, self.L = predict(self.x, self.L, self.F, self.Q12, B, u)

    def update(self, z, R2=None):
        if z is None:
            return
        R12 = self.R12 if R2 is None else (np.eye(self.m) * R2 if np.isscalar(R2) else R2)
        self.x, self.L, self.y, self.K, self.S12, self.SI12 = update(self.x, self.L, np.ravel(z), self.H, R12)
