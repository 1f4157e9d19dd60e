"""NumPy restatement of the reference's UKF on SimplexSigmaPoints, in the reference's operation order (filterpy/kalman/
sigma_points.py:454-513, unscented_transform.py:99-128, UKF.py:364-504, :524-632, :634-739), for one filter with a linear model
fx(x, dt) = F x, hx(x) = H x -- and the reader of tests/golden/ukf_simplex.npz (tests/golden/make_ukf_simplex_golden.py).

What the tests hold the kernels, the host-compiled step functions and the Python layer against where the live reference is not
at hand (the GPU machines), and -- unlike the goldens -- for any weights: Wm / Wc of length n + 1 are used as given."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ukf_simplex.npz")
FUSED = [(1, 1), (2, 1), (2, 2), (3, 1), (4, 2), (5, 3), (6, 3), (7, 4), (8, 4), (9, 3), (9, 4)]     # the golden's fused sizes


def point_matrix(n):
    """I = sqrt(n) Istar, n x (n + 1): sigma_points.py:501-509, statement by statement"""
    lambda_ = n / (n + 1)
    Istar = np.array([[-1 / np.sqrt(2 * lambda_), 1 / np.sqrt(2 * lambda_)]])
    for d in range(2, n + 1):
        row = np.ones((1, Istar.shape[1] + 1)) * 1. / np.sqrt(lambda_ * d * (d + 1))
        row[0, -1] = -d / np.sqrt(lambda_ * d * (d + 1))
        Istar = np.r_[np.c_[Istar, np.zeros((Istar.shape[0]))], row]
    return np.sqrt(n) * Istar


def weights(n):
    """sigma_points.py:516-522"""
    return np.full(n + 1, 1. / (n + 1))


def sigma_points(x, P):
    """sigma_points.py:488-513 -> (n + 1, n); U = cholesky(P) upper, U' = the lower factor"""
    x = np.asarray(x, dtype=np.float64).reshape(-1)
    n = x.size
    P = np.eye(n) * P if np.isscalar(P) else np.atleast_2d(np.asarray(P, dtype=np.float64))
    U = np.linalg.cholesky(P).T
    scaled_unitary = (U.T).dot(point_matrix(n))
    return np.subtract(x.reshape(-1, 1), -scaled_unitary).T


def unscented_transform(sigmas, Wm, Wc, noise_cov=None):
    """unscented_transform.py:101-126 with the default mean and residual"""
    x = np.dot(Wm, sigmas)
    y = sigmas - x[np.newaxis, :]
    P = np.dot(y.T, np.dot(np.diag(Wc), y))
    if noise_cov is not None:
        P = P + noise_cov
    return x, P


def predict(x, P, F, Q, Wm, Wc):
    """UKF.py:400-411 -> x-, P-, the regenerated sigma points"""
    sf = sigma_points(x, P) @ F.T
    x, P = unscented_transform(sf, Wm, Wc, Q)
    return x, P, sigma_points(x, P)


def update(x, P, sigmas_f, z, H, R, Wm, Wc):
    """UKF.py:462-491 -> dict of the posterior and every intermediate"""
    sh = sigmas_f @ H.T
    zp, S = unscented_transform(sh, Wm, Wc, R)
    Pxz = np.zeros((x.size, zp.size))
    for i in range(sigmas_f.shape[0]):                      # UKF.py:493-504
        Pxz += Wc[i] * np.outer(sigmas_f[i] - x, sh[i] - zp)
    K = np.dot(Pxz, np.linalg.inv(S))
    y = np.asarray(z, dtype=np.float64).reshape(-1) - zp
    return dict(x=x + np.dot(K, y), P=P - np.dot(K, np.dot(S, K.T)), K=K, S=S, y=y, Pxz=Pxz, sigmas_h=sh)


def batch_filter(x0, P0, zs, F, H, Q, R, Wm=None, Wc=None):
    """UKF.py:524-632: zs a sequence of measurements or None -> means (T, n), covariances (T, n, n)"""
    x, P = np.array(x0, dtype=np.float64), np.array(P0, dtype=np.float64)
    n = x.size
    Wm = weights(n) if Wm is None else Wm
    Wc = Wm if Wc is None else Wc
    mu, cov = np.zeros((len(zs), n)), np.zeros((len(zs), n, n))
    for t, z in enumerate(zs):
        x, P, sf = predict(x, P, F, Q, Wm, Wc)
        if z is not None:
            u = update(x, P, sf, z, H, R, Wm, Wc)
            x, P = u["x"], u["P"]
        mu[t], cov[t] = x, P
    return mu, cov


def rts_smoother(Xs, Ps, F, Q, Wm=None, Wc=None):
    """UKF.py:700-739 (the filter's Q: Qs is never read) -> xs, ps, Ks"""
    Xs, Ps = np.asarray(Xs, dtype=np.float64), np.asarray(Ps, dtype=np.float64)
    T, n = Xs.shape
    Wm = weights(n) if Wm is None else Wm
    Wc = Wm if Wc is None else Wc
    xs, ps, Ks = Xs.copy(), Ps.copy(), np.zeros((T, n, n))
    for k in reversed(range(T - 1)):
        sig = sigma_points(xs[k], ps[k])
        sf = sig @ F.T
        xb, Pb = unscented_transform(sf, Wm, Wc, Q)
        Pxb = np.zeros((n, n))
        for i in range(n + 1):
            Pxb += Wc[i] * np.outer(sig[i] - Xs[k], sf[i] - xb)
        K = np.dot(Pxb, np.linalg.inv(Pb))
        xs[k] += np.dot(K, xs[k + 1] - xb)
        ps[k] += np.dot(K, ps[k + 1] - Pb).dot(K.T)
        Ks[k] = K
    return xs, ps, Ks


def rel(a, b):
    """the package's parity measure: max |a - b| / max |b| per array"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300))


class Golden(object):
    """tests/golden/ukf_simplex.npz: g.case(n, m) -> dict of the case's arrays (zs as a list with None where missing)"""

    def __init__(self):
        self.d = np.load(GOLDEN)
        self.cases = [tuple(int(v) for v in c) for c in self.d["cases"]]
        self.missing = tuple(int(v) for v in self.d["missing"])

    def I(self, n):
        return self.d["I%d" % n]

    def case(self, n, m):
        ci = self.cases.index((n, m))
        p = "c%d_" % ci
        c = {k[len(p):]: self.d[k] for k in self.d.files if k.startswith(p)}
        zl = [np.array(z) for z in c["zs"]]
        if ci == self.missing[0]:
            zl[self.missing[1]] = None
        c["zl"] = zl
        c["mask"] = np.array([z is not None for z in zl], dtype=np.uint8)
        return c
