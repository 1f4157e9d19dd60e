#!/usr/bin/env python3
"""Golden vectors for the UKF on SimplexSigmaPoints (n + 1 points) from the LIVE reference (rlabbe/filterpy v1.4.5;
sigma_points.py:386-534, unscented_transform.py:99-128, UKF.py:364-504, :524-632, :634-739).

Per (n, m) one random linear model; the weights, the constant point matrix I = sqrt(n) Istar (sigma_points.py:501-509, read
back from the reference's own points: with P = 1 and x = 0 the points ARE the columns of I) and sigma_points(x0, P0); one step
with every intermediate (sigmas_f, prior, sigmas_h, Pxz, K, S, y); a T-step batch_filter and the smoother over it.  The case
MISSING has no measurement (None) at step MISSING_AT.  (12, 4) is there for the building-block route: the fused kernels stop at
dim_x 9.  The point matrices of n = 1..16 are stored as well (I<n>): the package's own has to equal them bit for bit.
Run in the build container only:

    PYTHONDONTWRITEBYTECODE=1 MPLBACKEND=Agg python tests/golden/make_ukf_simplex_golden.py
"""
import os
import sys

import numpy as np

REF = os.environ.get("FILTERPY_REFERENCE", "/root/reference")
sys.path.insert(0, REF)
sys.dont_write_bytecode = True

from filterpy.kalman import UnscentedKalmanFilter, SimplexSigmaPoints  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))

CASES = [(1, 1), (2, 1), (2, 2), (3, 1), (4, 2), (5, 3), (6, 3), (7, 4), (8, 4), (9, 3), (9, 4), (12, 4)]
T = 12
MISSING, MISSING_AT = 4, 5          # case (4, 2): zs[5] is None


def spd(rs, n, scale=1.0):
    A = rs.randn(n, n)
    return scale * (A @ A.T / n + 0.5 * np.eye(n))


def stable_F(rs, n):
    F = np.eye(n) + 0.1 * rs.randn(n, n)
    return F / max(1.0, 1.05 * np.max(np.abs(np.linalg.eigvals(F))))


def point_matrix(n):
    """I (n x (n + 1)) as the reference forms it: sigma_points(0, 1) = (U' I)' with U = cholesky(eye) = eye, and 0 - (-v) = v"""
    return SimplexSigmaPoints(n).sigma_points(np.zeros(n), 1.0).T.copy()


def main():
    d = {"cases": np.array(CASES), "missing": np.array([MISSING, MISSING_AT])}
    for n in range(1, 17):
        d["I%d" % n] = point_matrix(n)
    for ci, (n, m) in enumerate(CASES):
        rs = np.random.RandomState(9100 + ci)
        pts = SimplexSigmaPoints(n)
        F, H = stable_F(rs, n), rs.randn(m, n)
        Q, R, P0, x0 = spd(rs, n, 0.01), spd(rs, m, 0.5), spd(rs, n, 5.0), rs.randn(n)
        zs = rs.randn(T, m) * 3
        p = f"c{ci}_"
        d.update({p + "F": F, p + "H": H, p + "Q": Q, p + "R": R, p + "P0": P0, p + "x0": x0, p + "zs": zs,
                  p + "Wm": pts.Wm, p + "sigmas": pts.sigma_points(x0, P0)})
        ukf = UnscentedKalmanFilter(n, m, dt=1.0, hx=lambda x: H @ x, fx=lambda x, dt: F @ x, points=pts)
        ukf.x, ukf.P, ukf.Q, ukf.R = x0.copy(), P0.copy(), Q.copy(), R.copy()
        ukf.predict()
        d.update({p + "s1_xp": ukf.x.copy(), p + "s1_Pp": ukf.P.copy(), p + "s1_sigmas_f": ukf.sigmas_f.copy()})
        ukf.update(zs[0])
        Pxz = ukf.cross_variance(ukf.x_prior, np.dot(pts.Wm, ukf.sigmas_h), ukf.sigmas_f, ukf.sigmas_h)
        d.update({p + "s1_x": ukf.x.copy(), p + "s1_P": ukf.P.copy(), p + "s1_K": ukf.K.copy(), p + "s1_S": ukf.S.copy(),
                  p + "s1_y": ukf.y.copy(), p + "s1_sigmas_h": ukf.sigmas_h.copy(), p + "s1_Pxz": Pxz})
        ukf.x, ukf.P = x0.copy(), P0.copy()
        zl = list(zs) if m > 1 else [np.array([z[0]]) for z in zs]
        if ci == MISSING:
            zl[MISSING_AT] = None
        mu, cov = ukf.batch_filter(zl)
        xs, Ps, Ks = ukf.rts_smoother(mu, cov)
        d.update({p + "mu": mu, p + "cov": cov, p + "rts_x": xs, p + "rts_P": Ps, p + "rts_K": Ks})
    np.savez_compressed(os.path.join(OUT, "ukf_simplex.npz"), **d)
    print("wrote ukf_simplex.npz:", len(d), "arrays")


if __name__ == "__main__":
    main()
