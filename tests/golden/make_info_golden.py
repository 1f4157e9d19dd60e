#!/usr/bin/env python3
"""InformationFilter (information_filter.py:178-289) on the LIVE reference: call sequences for dims (1,1) .. (16,8) in both call
orders (predict first / update first), with an update(None) step, an R_inv override as a matrix and as a scalar, a control
input through a matrix B and through the scalar B, both shapes of x; and the model of the reference's test_1d /
test_against_kf (F = [[1,1],[0,1]], H = [1, 0], R_inv = 1/5, Q = 1e-4 I, scalar measurements, update then predict).  Every
attribute of the object after every call.  Where 1 < dim_z < dim_x the reference's logpdf(y, cov=S) cannot broadcast and
update() raises, so those cases run with compute_log_likelihood=False.  Freezes inputs and outputs.

    PYTHONPATH=/root/reference MPLBACKEND=Agg python tests/golden/make_info_golden.py
writes tests/golden/info.npz
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.environ.get("FILTERPY_REFERENCE", "/root/reference"))
from filterpy.kalman import InformationFilter  # noqa: E402

DIMS = [(1, 1), (2, 1), (2, 2), (3, 2), (4, 2), (5, 3), (6, 3), (8, 4), (9, 3), (12, 4), (16, 8)]
# ops: 0 predict(), 1 predict(u), 2 update(z), 3 update(None), 4 update(z, R_inv matrix), 5 update(z, R_inv scalar)
ATTRS = ("x", "P_inv", "x_prior", "P_inv_prior", "x_post", "P_inv_post", "K", "y", "S", "log_likelihood", "likelihood")
RINV_SCALAR = 1.7


def spd(rs, k, scale=1.0):
    a = rs.randn(k, k)
    return scale * (a @ a.T / k + 0.5 * np.eye(k))


def ops_for(order, ctrl, steps):
    pre = 1 if ctrl else 0
    seq = []
    for s in range(steps):
        up = {2: 3, 3: 4, 5: 5}.get(s, 2)
        seq += [pre, up] if order == 0 else [up, pre]
    return seq


def record(out, p, k, f):
    """every attribute after call k; an array equal to the one after call k-1 is not stored again (the reader takes the latest
    stored k' <= k: tests/info_port.py attr)"""
    for a in ATTRS:
        v = np.array(getattr(f, a), dtype=float)
        for kk in range(k - 1, -1, -1):
            prev = out.get(f"{p}k{kk}_{a}")
            if prev is not None:
                break
        else:
            prev = None
        if prev is None or prev.shape != v.shape or not np.array_equal(prev, v):
            out[f"{p}k{k}_{a}"] = v


def main():
    out = {"dims": np.array(DIMS)}
    ci = 0
    for n, m in DIMS:
        for order in (0, 1):
            rs = np.random.RandomState(3000 + ci)
            nd = 1 + (ci % 2)
            ctrl = (0, 1, 2)[ci % 3]
            steps = 6
            F = np.eye(n) + 0.1 * rs.randn(n, n) / np.sqrt(n)
            Q, H, Rinv, Pinv0, x0 = spd(rs, n, 0.02), rs.randn(m, n), spd(rs, m, 2.0), spd(rs, n, 0.5), rs.randn(n)
            Rinv2 = spd(rs, m, 1.3)
            f = InformationFilter(n, m, compute_log_likelihood=(m == 1 or m == n))
            f.F, f.H, f.Q, f.R_inv, f.P_inv = F, H, Q, Rinv, Pinv0.copy()
            f.x = x0.copy() if nd == 1 else x0.reshape(n, 1).copy()
            B, us = None, None
            ops = ops_for(order, ctrl, steps)
            if ctrl == 1:
                B = rs.randn(n, 2)
                f.B = B
                us = rs.randn(len(ops), 2)
            elif ctrl == 2:
                f.B = 0.5
                us = rs.randn(len(ops), n)
            zs = rs.randn(len(ops), m) * 2.0
            p = f"c{ci}_"
            out[p + "spec"] = np.array([n, m, nd, ctrl, order])
            out[p + "ops"] = np.array(ops)
            out[p + "F"], out[p + "H"], out[p + "Q"], out[p + "Rinv"], out[p + "Pinv0"], out[p + "x0"] = F, H, Q, Rinv, Pinv0, x0
            out[p + "Rinv2"], out[p + "zs"] = Rinv2, zs
            if us is not None:
                out[p + "us"] = us
                out[p + "B"] = B if ctrl == 1 else np.array(0.5)
            for k, op in enumerate(ops):
                col = (lambda v: v) if nd == 1 else (lambda v: v.reshape(-1, 1))
                if op == 0:
                    f.predict()
                elif op == 1:
                    f.predict(col(us[k]))
                elif op == 2:
                    f.update(col(zs[k]))
                elif op == 3:
                    f.update(None)
                elif op == 4:
                    f.update(col(zs[k]), R_inv=Rinv2)
                elif op == 5:
                    f.update(col(zs[k]), R_inv=RINV_SCALAR)
                record(out, p, k, f)
            ci += 1
    out["n_cases"] = np.array(ci)
    # the model of the reference's tests (kalman/tests/test_information.py: test_1d, test_against_kf), column x, scalar
    # measurements, update then predict
    rs = np.random.RandomState(78)
    f = InformationFilter(dim_x=2, dim_z=1)
    f.x = np.array([[2.], [0.]])
    f.F = np.array([[1., 1.], [0., 1.]])
    f.H = np.array([[1., 0.]])
    f.R_inv *= 1. / 5
    f.Q *= 0.0001
    zs = np.arange(30.) + rs.randn(30) * 20
    out["t_zs"] = zs
    for k in range(30):
        f.update(float(zs[k]))
        record(out, "t_", 2 * k, f)
        f.predict()
        record(out, "t_", 2 * k + 1, f)
    np.savez_compressed(os.path.join(HERE, "info.npz"), **out)


if __name__ == "__main__":
    main()
