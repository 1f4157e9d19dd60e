"""tests/ekf_port.py in np.longdouble (80-bit on x86-64; eps 1.08e-19): the same lines of EKF.py:319-332, 351, 367 with
tests/info_hp.py's Gauss-Jordan inverse (numpy's linear algebra does not take longdouble) -- the truth the precision tests
measure the GPU and the float64 port against.  The callables are handed longdouble states and compute in longdouble."""
import numpy as np

import ekf_port
from info_hp import LD, inv, ld  # noqa: F401


def batch(x0, P0, zs, F, Q, R, jac, hx, residual=np.subtract):
    """means, covs (posterior) and means_p, covs_p of one track, predict first, in longdouble"""
    return ekf_port.batch(x0, P0, zs, F, Q, R, jac, hx, residual, dtype=LD, inv=inv)
