"""NumPy port of filterpy/kalman/ensemble_kalman_filter.py:187-290 that takes the random draws as ARGUMENTS, so that every
result is a function of its inputs: held to the goldens of the live reference on the CPU (tests/test_host_enkf.py), and the
reference of the GPU tests where goldens would be too big.  `moments` also restates the two one-pass forms of the second
moments (pivot-shifted, uncentred) for the spread table of tests/golden/make_enkf_golden.py."""
import numpy as np

INIT, PREDICT, UPDATE, UPDATE_RMAT, UPDATE_RSCALAR, UPDATE_NONE = range(6)
ATTRS = ("x", "P", "K", "S", "SI", "sigmas", "x_prior", "P_prior", "x_post", "P_post")


def factor(cov):
    """A with w @ A ~ N(0, cov) for standard normal w (numpy.random.multivariate_normal's own factor)"""
    _, s, v = np.linalg.svd(cov)
    return np.sqrt(s)[:, None] * v


def moments(a, ca, b, cb, mode="twopass", pa=None, pb=None):
    """sum (a - ca)(b - cb)' over the members.  twopass: as written (the reference); shifted: one pass over data shifted by
    the pivots pa, pb, corrected by the shifted sums; uncentred: one pass over the raw data"""
    N = len(a)
    if mode == "twopass":
        return (a - ca).T @ (b - cb)
    if mode == "shifted":
        da, db = a - pa, b - pb
        return da.T @ db - np.outer(da.sum(0), cb - pb) - np.outer(ca - pa, db.sum(0)) + N * np.outer(ca - pa, cb - pb)
    return a.T @ b - np.outer(a.sum(0), cb) - np.outer(ca, b.sum(0)) + N * np.outer(ca, cb)


def predict(sig, e, F=None, mode="twopass", pivot=None):
    """(:275-290) members (N, n) moved by F (None: already moved), plus the draws e -> sigmas, x, P"""
    sig = (sig @ F.T if F is not None else sig) + e
    N = len(sig)
    x = sig.mean(axis=0)
    P = moments(sig, x, sig, x, mode, pivot, pivot) / (N - 1)
    return sig, x, P


def update(sig, x, P, z, R, e, H=None, sigmas_h=None, mode="twopass"):
    """(:240-268) -> sigmas, x, P, K, S, SI.  The members are centred on the x GIVEN, sigmas_h on their own mean."""
    N = len(sig)
    sh = sig @ H.T if sigmas_h is None else sigmas_h
    zm = sh.mean(axis=0)
    ph = x @ H.T if H is not None else sh[0]
    S = moments(sh, zm, sh, zm, mode, ph, ph) / (N - 1) + R
    Pxz = moments(sig, x, sh, zm, mode, x, ph) / (N - 1)
    SI = np.linalg.inv(S)
    K = Pxz @ SI
    sig = sig + (z + e - sh) @ K.T
    return sig, sig.mean(axis=0), P - K @ S @ K.T, K, S, SI


class Port:
    """the reference's object, stepped with given draws (the golden cases' linear models)"""

    def __init__(self, x, P, dim_z, N, F, H, draw):
        self.n, self.m, self.N, self.F, self.H = len(x), dim_z, N, F, H
        self.K, self.S, self.SI = np.zeros((self.n, dim_z)), np.zeros((dim_z, dim_z)), np.zeros((dim_z, dim_z))
        self.initialize(x, P, draw)
        self.Q, self.R = np.eye(self.n), np.eye(dim_z)

    def initialize(self, x, P, draw):
        self.sigmas = np.array(draw, dtype=float)
        self.x, self.P = x.copy(), P.copy()
        self.x_prior, self.P_prior, self.x_post, self.P_post = x.copy(), P.copy(), x.copy(), P.copy()

    def predict(self, e):
        self.sigmas, self.x, self.P = predict(self.sigmas, e, self.F)
        self.x_prior, self.P_prior = self.x.copy(), self.P.copy()

    def update(self, z, e=None, R=None):
        if z is not None:
            R = self.R if R is None else R
            R = np.eye(self.m) * R if np.isscalar(R) else R
            self.sigmas, self.x, self.P, self.K, self.S, self.SI = update(self.sigmas, self.x, self.P, z, R, e, self.H)
        self.x_post, self.P_post = self.x.copy(), self.P.copy()


def case(G, ci):
    p = f"c{ci}_"
    c = {k: G[p + k] for k in ("F", "H", "x0", "P0", "Q", "R")}
    c.update(p=p, n=int(G[p + "n"]), m=int(G[p + "m"]), N=int(G[p + "N"]), ops=[int(o) for o in G[p + "ops"]])
    return c


def op_inputs(G, c, k):
    """what op k was called with: the recorded draw (None for update(None)), its (mean, cov), z, and the R argument"""
    q = f"{c['p']}k{k}_"
    has = (q + "draw") in G
    return dict(draw=G[q + "draw"] if has else None, mean=G[q + "mean"] if has else None, cov=G[q + "cov"] if has else None,
                z=G[q + "z"] if (q + "z") in G else None, R=G[q + "Rarg"] if (q + "Rarg") in G else None)


def attr(G, c, k, a):
    return G[f"{c['p']}k{k}_{a}"]


def run_op(f, c, k, op, G, draw=None):
    """op k of case c on a filter-like object f (the port, or the class under test with its noise replayed)"""
    i = op_inputs(G, c, k)
    d = i["draw"] if draw is None else draw
    port = isinstance(f, Port)
    if op == INIT:
        f.initialize(i["mean"], i["cov"], d) if port else f.initialize(i["mean"].copy(), i["cov"].copy())
    elif op == PREDICT:
        f.predict(d) if port else f.predict()
    elif op == UPDATE_NONE:
        f.update(None)
    else:
        R = None if op == UPDATE else (float(i["R"]) if op == UPDATE_RSCALAR else i["R"])
        f.update(i["z"], d, R) if port else f.update(i["z"], R)
