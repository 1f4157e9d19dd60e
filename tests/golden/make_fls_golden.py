#!/usr/bin/env python3
"""FixedLagSmoother (fixed_lag_smoother.py:133-311) on the LIVE reference: smooth_batch for dims (1,1) .. (16,8) and lags
0, 1, 2, 7, 8, 9, 16, 17, T-1, T+3 (around the fast kernel's capacities 8 and 16), both shapes of x, scalar measurements for
dim_z = 1, a control input through a matrix B and through the scalar B, scalar R and Q attributes; and smooth() sequences with
every attribute after every call.  Freezes inputs and outputs.

    PYTHONPATH=/root/reference MPLBACKEND=Agg python tests/golden/make_fls_golden.py
writes tests/golden/fls.npz
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, "/root/reference")
from filterpy.kalman import FixedLagSmoother  # noqa: E402

DIMS = [(1, 1), (2, 1), (3, 2), (4, 2), (5, 3), (6, 3), (8, 4), (9, 3), (12, 4), (16, 8)]
T = 20
LAGS = [0, 1, 2, 7, 8, 9, 16, 17, T - 1, T + 3]
# smooth() sequences: (dim_x, dim_z, lag, x.ndim, control)
SEQS = [(2, 1, 1, 2, 0), (4, 2, 3, 2, 1), (3, 2, 0, 1, 0), (4, 2, 9, 1, 2), (9, 3, 5, 2, 0), (5, 3, 17, 2, 1)]
TS = 12


def spd(rs, k, scale=1.0):
    a = rs.randn(k, k)
    return scale * (a @ a.T / k + 0.5 * np.eye(k))


def model(rs, n, m):
    F = np.eye(n) + 0.1 * rs.randn(n, n) / np.sqrt(n)
    return F, spd(rs, n, 0.02), rs.randn(m, n), spd(rs, m, 0.5), spd(rs, n, 2.0), rs.randn(n)


def options(i, n, m):
    """(x.ndim, control 0 none / 1 matrix B / 2 scalar B, scalar R and Q, scalar zs)"""
    return 1 + (i % 2), (0, 1, 0, 2)[i % 4], i % 5 == 2, m == 1 and i % 3 == 0


def main():
    out = {"dims": np.array(DIMS), "lags": np.array(LAGS), "seqs": np.array(SEQS)}
    ci = 0
    for n, m in DIMS:
        for lag in LAGS:
            rs = np.random.RandomState(1000 + ci)
            F, Q, H, R, P0, x0 = model(rs, n, m)
            nd, ctrl, scal, zsc = options(ci, n, m)
            zs = rs.randn(T, m) * 2.0
            fls = FixedLagSmoother(n, m)
            fls.F, fls.H, fls.P = F, H, P0
            fls.x = x0.copy() if nd == 1 else x0.reshape(n, 1).copy()
            if scal:
                fls.R, fls.Q = 1.5, 0.01
            else:
                fls.R, fls.Q = R, Q
            us, B = None, None
            if ctrl == 1:
                B = rs.randn(n, 2)
                fls.B = B
                us = rs.randn(T, 2) if nd == 1 else rs.randn(T, 2, 1)
            elif ctrl == 2:
                fls.B = 0.5
                us = rs.randn(T, n) if nd == 1 else rs.randn(T, n, 1)
            zin = zs[:, 0] if zsc else (zs if nd == 1 else zs.reshape(T, m, 1))
            xs, xhat = fls.smooth_batch(zin, lag, us=us)
            p = f"c{ci}_"
            out[p + "spec"] = np.array([n, m, lag, nd, ctrl, int(scal), int(zsc)])
            out[p + "F"], out[p + "H"], out[p + "P0"], out[p + "x0"], out[p + "zs"] = F, H, P0, x0, zs
            out[p + "Q"], out[p + "R"] = (np.array(0.01), np.array(1.5)) if scal else (Q, R)
            if us is not None:
                out[p + "us"] = np.asarray(us).reshape(T, -1)
                out[p + "B"] = B if ctrl == 1 else np.array(0.5)
            out[p + "xs"], out[p + "xhat"] = np.asarray(xs), np.asarray(xhat)
            ci += 1
    out["n_cases"] = np.array(ci)
    for si, (n, m, lag, nd, ctrl) in enumerate(SEQS):
        rs = np.random.RandomState(5000 + si)
        F, Q, H, R, P0, x0 = model(rs, n, m)
        zs = rs.randn(TS, m) * 2.0
        fls = FixedLagSmoother(n, m, N=lag)
        fls.F, fls.H, fls.P, fls.Q, fls.R = F, H, P0, Q, R
        fls.x = x0.copy() if nd == 1 else x0.reshape(n, 1).copy()
        us = None
        if ctrl == 1:
            fls.B = rs.randn(n, 2)
            us = rs.randn(TS, 2)
        elif ctrl == 2:
            fls.B = 0.5
            us = rs.randn(TS, n)
        p = f"s{si}_"
        out[p + "F"], out[p + "Q"], out[p + "H"], out[p + "R"], out[p + "P0"], out[p + "x0"], out[p + "zs"] = F, Q, H, R, P0, x0, zs
        if us is not None:
            out[p + "us"] = us
            out[p + "B"] = np.asarray(fls.B)
        for k in range(TS):
            z = zs[k] if nd == 1 else zs[k].reshape(m, 1)
            u = None if us is None else (us[k] if nd == 1 else us[k].reshape(-1, 1))
            fls.smooth(z, u)
            q = f"{p}k{k}_"
            out[q + "x"], out[q + "P"], out[q + "y"], out[q + "S"] = fls.x, fls.P, fls.y, fls.S
            out[q + "xSmooth"] = np.array(fls.xSmooth)
            out[q + "count"] = np.array(fls.count)
    np.savez_compressed(os.path.join(HERE, "fls.npz"), **out)


if __name__ == "__main__":
    main()
