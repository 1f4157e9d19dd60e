"""tests/ckf_port.py in np.longdouble (80-bit on x86-64): the same lines of CubatureKalmanFilter.py:32-98, 292-390 with a
Cholesky factorisation of its own and tests/info_hp.py's Gauss-Jordan inverse (numpy's linear algebra does not take longdouble)
-- the truth the precision tests measure the GPU and the float64 port against."""
import numpy as np

import ckf_port
from info_hp import LD, inv, ld  # noqa: F401


def chol_upper(P):
    """U upper with U' U = P, in longdouble (the upper triangle of P is read, like scipy.linalg.cholesky)"""
    P = ld(P)
    n = P.shape[0]
    U = np.zeros((n, n), dtype=LD)
    for j in range(n):
        d = P[j, j] - U[:j, j] @ U[:j, j]
        U[j, j] = np.sqrt(d)
        for i in range(j + 1, n):
            U[j, i] = (P[j, i] - U[:j, j] @ U[:j, i]) / U[j, j]
    return U


def batch(x0, P0, zs, F, Q, H, R, mask=None):
    """means, covs (posterior) and means_p, covs_p of one track on the matrix model, predict first, in longdouble"""
    return ckf_port.batch(x0, P0, zs, F, Q, H, R, mask, dtype=LD, chol=chol_upper, inv=inv)[:4]
