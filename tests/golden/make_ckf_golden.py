#!/usr/bin/env python3
"""CubatureKalmanFilter (CubatureKalmanFilter.py:32-98, 292-390) on the LIVE reference: the call sequences of
tests/ckf_port.py (SEQ) for dims (1,1) .. (16,8), each with linear callables (fx_args = (F,), hx_args = (H,)) and with a
polynomial fx and a range / bearing style hx (fx_args, hx_args), a dt override, update(None), R given as a matrix and as a
scalar, two updates after one predict, an update before any predict, a custom residual_z on every other nonlinear case; and the
model of the reference's test_1d.  Every attribute of the object after every call (an array that did not change is not stored
again).  Measurements are (m, 1) columns: with dim_z > 1 the reference raises for a 1-D z.  Freezes outputs; the inputs are
drawn by tests/ckf_port.py inputs().

    PYTHONPATH=/root/reference MPLBACKEND=Agg python tests/golden/make_ckf_golden.py
writes tests/golden/ckf.npz
"""
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.environ.get("FILTERPY_REFERENCE", "/root/reference"))
from filterpy.kalman import CubatureKalmanFilter  # noqa: E402
import ckf_port as cp  # noqa: E402


def record(out, p, k, f):
    for a in cp.ATTRS:
        try:
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                v = np.array(getattr(f, a), dtype=float)
        except AttributeError:                       # mahalanobis before the first update: y is the int 0 (:427)
            continue
        prev = cp.attr(out_view(out), p, k - 1, a) if k else None
        if prev is None or prev.shape != v.shape or not np.array_equal(prev, v):
            out[f"{p}k{k}_{a}"] = v


class out_view(object):
    """a dict read like an NpzFile (cp.attr)"""

    def __init__(self, d):
        self.d, self.files = d, d

    def __getitem__(self, k):
        return self.d[k]


def main():
    out = {"dims": np.array(cp.DIMS)}
    for spec in cp.specs():
        ci, n, m, kind, seq, custom = spec
        d = cp.inputs(ci, n, m, kind)
        f = cp.make(CubatureKalmanFilter, spec, d)
        out[f"c{ci}_spec"] = np.array(spec)
        for k in range(cp.n_ops(spec)):
            cp.run_op(f, spec, d, k)
            record(out, f"c{ci}_", k, f)
    out["n_cases"] = np.array(len(cp.specs()))
    # the model of the reference's test (kalman/tests/test_ckf.py: test_1d): Q H' = 0 and H Q H' = 0, where the cubature filter
    # IS the linear Kalman filter
    rs = np.random.RandomState(78)
    ckf = CubatureKalmanFilter(dim_x=2, dim_z=1, dt=0.1, hx=lambda x: x[0:1],
                               fx=lambda x, dt: np.dot(np.array([[1., 1], [0, 1.1]]), x))
    ckf.x = np.array([[1.], [2.]])
    ckf.P = np.array([[1, 1.1], [1.1, 3]])
    ckf.R = np.eye(1) * .05
    ckf.Q = np.array([[0., 0], [0., .001]])
    zs = np.arange(50.) + rs.randn(50) * 0.5
    out["t_zs"] = zs
    for k in range(50):
        ckf.predict()
        record(out, "t_", 2 * k, ckf)
        ckf.update(np.array([[zs[k]]]))
        record(out, "t_", 2 * k + 1, ckf)
    np.savez_compressed(os.path.join(HERE, "ckf.npz"), **out)


if __name__ == "__main__":
    main()
