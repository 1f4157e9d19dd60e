#!/usr/bin/env python3
"""ExtendedKalmanFilter (EKF.py:132-428) on the LIVE reference: the call sequence tests/ekf_models.py OPS -- predict, update,
predict_update, update(None), update with a scalar R -- on its two golden models, the slant-range radar of the reference's own
test_ekf.py at (3, 1) (x 1-D, z shaped (1,)) and a range-bearing sensor with an angle-wrapping residual at (4, 2) (x a column,
z (2, 1)).  Every attribute of the object after every call.  Freezes outputs; the inputs are drawn by tests/ekf_models.py.

    PYTHONPATH=/root/reference MPLBACKEND=Agg python tests/golden/make_ekf_golden.py
writes tests/golden/ekf.npz
"""
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.environ.get("FILTERPY_REFERENCE", "/root/reference"))
from filterpy.kalman import ExtendedKalmanFilter  # noqa: E402
import ekf_models as em  # noqa: E402


def main():
    out = {}
    for case in sorted(em.CASES):
        f, d = em.make(ExtendedKalmanFilter, case)
        for k in range(len(em.OPS)):
            em.run_op(f, case, d, k)
            for a in em.ATTRS:
                with warnings.catch_warnings():
                    warnings.simplefilter("ignore")
                    out[f"{case}_k{k}_{a}"] = np.array(getattr(f, a), dtype=float)
    out["n_ops"] = np.array(len(em.OPS))
    np.savez_compressed(os.path.join(HERE, "ekf.npz"), **out)
    print("wrote ekf.npz:", len(out), "arrays")


if __name__ == "__main__":
    main()
