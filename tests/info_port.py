"""NumPy restatement of filterpy.kalman.InformationFilter (information_filter.py:178-289, the invertible branch) for the tests,
line for line: three numpy.linalg.inv per step, F^-1 included -- no dependency on the reference checkout (the GPU box has no
reference).  One track per call (`predict`, `update`, `batch`) and vectorised over tracks (`batch_tracks`); `batch` runs the
time loop the way fk_info_batch_f64 does."""
import numpy as np

inv = np.linalg.inv


def predict(x, Pi, F, Q, B=None, u=None, F_inv=None):
    """information_filter.py:245-289 on x (n,), Pi = P_inv (n, n)"""
    F_inv = inv(F) if F_inv is None else F_inv
    A = np.dot(F_inv.T, Pi).dot(F_inv)
    AI = inv(A)
    x = np.dot(F, x)
    if B is not None:
        x = x + np.dot(B, u)
    return x, inv(AI + Q)


def update(x, Pi, z, H, Ri):
    """information_filter.py:178-243 -> x, P_inv (= S), y, K"""
    y = z - np.dot(H, x)
    S = Pi + np.dot(H.T, Ri).dot(H)
    K = np.dot(inv(S), H.T).dot(Ri)
    return x + np.dot(K, y), S, y, K


def batch(x0, Pi0, zs, F, Q, H, Ri, B=None, us=None, mask=None, update_first=False):
    """fk_info_batch_f64 for one track: (means, P_invs, means_p, P_invs_p, last) with last = (x, P_inv, y, K) of the last
    update (None if none)"""
    x, Pi = np.array(x0, dtype=float), np.array(Pi0, dtype=float)
    T, n = len(zs), len(x)
    F_inv = inv(F)
    mu, cov, mu_p, cov_p = np.zeros((T, n)), np.zeros((T, n, n)), np.zeros((T, n)), np.zeros((T, n, n))
    last = None
    for t in range(T):
        if not update_first:
            x, Pi = predict(x, Pi, F, Q, B, None if us is None else us[t], F_inv)
            mu_p[t], cov_p[t] = x, Pi
        if mask is None or mask[t]:
            last = update(x, Pi, zs[t], H, Ri)
            x, Pi = last[0], last[1]
        mu[t], cov[t] = x, Pi
        if update_first:
            x, Pi = predict(x, Pi, F, Q, B, None if us is None else us[t], F_inv)
            mu_p[t], cov_p[t] = x, Pi
    return mu, cov, mu_p, cov_p, last


def batch_tracks(x0, Pi0, zs, F, Q, H, Ri, B=None, us=None, mask=None, update_first=False):
    """`batch` vectorised over tracks: x0 (N, n), Pi0 (N, n, n), zs (T, N, m), us (T, N, nu), mask (T, N) -> the four
    histories (T, N, ...).  The same lines, on stacks."""
    x, Pi = np.array(x0, dtype=float), np.array(Pi0, dtype=float)
    T, (N, n) = len(zs), x.shape
    F_inv = inv(F)
    G = np.dot(H.T, Ri).dot(H)
    mu, cov, mu_p, cov_p = np.zeros((T, N, n)), np.zeros((T, N, n, n)), np.zeros((T, N, n)), np.zeros((T, N, n, n))

    def pred(x, Pi, t):
        A = np.matmul(np.matmul(F_inv.T, Pi), F_inv)
        x = x @ F.T
        if B is not None:
            x = x + us[t] @ B.T
        return x, inv(inv(A) + Q)

    def upd(x, Pi, t):
        y = zs[t] - x @ H.T
        S = Pi + G
        K = np.matmul(np.matmul(inv(S), H.T), Ri)
        xn = x + np.einsum("nij,nj->ni", K, y)
        if mask is None:
            return xn, S
        k = np.asarray(mask[t], dtype=bool)
        return np.where(k[:, None], xn, x), np.where(k[:, None, None], S, Pi)

    for t in range(T):
        if not update_first:
            x, Pi = pred(x, Pi, t)
            mu_p[t], cov_p[t] = x, Pi
        x, Pi = upd(x, Pi, t)
        mu[t], cov[t] = x, Pi
        if update_first:
            x, Pi = pred(x, Pi, t)
            mu_p[t], cov_p[t] = x, Pi
    return mu, cov, mu_p, cov_p


# ---- the goldens (tests/golden/info.npz, tests/golden/make_info_golden.py) ----------------------------------------------------
ATTRS = ("x", "P_inv", "x_prior", "P_inv_prior", "x_post", "P_inv_post", "K", "y", "S", "log_likelihood", "likelihood")
PREDICT, PREDICT_U, UPDATE, UPDATE_NONE, UPDATE_RINV, UPDATE_RINV_SCALAR = range(6)
RINV_SCALAR = 1.7


def has_likelihood(n, m):
    """the reference's logpdf(y, cov=S) broadcasts only when dim_z is 1 or dim_x: the goldens of the other shapes were made with
    compute_log_likelihood=False"""
    return m == 1 or m == n


def case(G, ci):
    p = f"c{ci}_"
    n, m, nd, ctrl, order = (int(v) for v in G[p + "spec"])
    d = dict(p=p, n=n, m=m, nd=nd, ctrl=ctrl, order=order, ops=[int(o) for o in G[p + "ops"]])
    for k in ("F", "H", "Q", "Rinv", "Pinv0", "x0", "Rinv2", "zs", "us", "B"):
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
    elif op == UPDATE_RINV:
        f.update(col(c["zs"][k]), R_inv=c["Rinv2"])
    else:
        f.update(col(c["zs"][k]), R_inv=RINV_SCALAR)


def setup(f, c):
    """the case's attributes on a fresh filter object"""
    f.F, f.H, f.Q, f.R_inv, f.P_inv = c["F"], c["H"], c["Q"], c["Rinv"], c["Pinv0"].copy()
    f.x = c["x0"].copy() if c["nd"] == 1 else c["x0"].reshape(-1, 1).copy()
    if "B" in c:
        f.B = c["B"]
    return f


class Port:
    """the port behind the reference's object interface (x 1-D)"""

    def __init__(self, n, m):
        self.n, self.m = n, m
        self.B = 0.

    def set(self, c):
        self.F, self.H, self.Q, self.Rinv, self.Pi = c["F"], c["H"], c["Q"], c["Rinv"], c["Pinv0"].astype(float).copy()
        self.x = c["x0"].astype(float).copy()
        self.B = c.get("B", 0.)
        self.K = self.y = None
        return self

    def predict(self, u=None):
        if u is None:
            self.x, self.Pi = predict(self.x, self.Pi, self.F, self.Q)
        else:
            B = self.B if np.ndim(self.B) else np.eye(self.n) * self.B
            self.x, self.Pi = predict(self.x, self.Pi, self.F, self.Q, B, np.ravel(u))

    def update(self, z, R_inv=None):
        if z is None:
            return
        Ri = self.Rinv if R_inv is None else (np.eye(self.m) * R_inv if np.isscalar(R_inv) else R_inv)
        self.x, self.Pi, self.y, self.K = update(self.x, self.Pi, np.ravel(z), self.H, Ri)
