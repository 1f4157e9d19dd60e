#!/usr/bin/env python3
"""Golden vectors for the fixed-gain polynomial filters from the LIVE reference (rlabbe/filterpy v1.4.5: filterpy/gh/gh_filter.py,
filterpy/memory/fading_memory.py, filterpy/leastsq/least_squares.py).

One set of T = 24 random-walk measurements for N = 5 tracks (zs).  Per class and order: a bank of the 5 tracks stepped with
update() -- the state after every step and the residual -- and one scalar filter on track 0; GHFilter / GHKFilter also
batch_filter with predictions; one GHFilter run whose g and h are overridden per call (least_squares_parameters);
FadingMemoryFilter's P and e; LeastSquaresFilter's K per step and errors() (from n = 3: below, the reference divides by zero);
the four helpers on a few arguments; VRF*, bias_error.  LeastSquaresFilter is one filter in the reference: its bank is five of
them side by side.  Run in the build container only:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_poly_golden.py
"""
import os
import sys
import warnings

import numpy as np

REF = os.environ.get("FILTERPY_REFERENCE", "/root/reference")
sys.path.insert(0, REF)
sys.dont_write_bytecode = True

from filterpy.gh import (GHFilter, GHKFilter, GHFilterOrder, optimal_noise_smoothing, least_squares_parameters,  # noqa: E402
                         critical_damping_parameters, benedict_bornder_constants)
from filterpy.memory import FadingMemoryFilter  # noqa: E402
from filterpy.leastsq import LeastSquaresFilter  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
T, N = 24, 5
DT, G, H, K, BETA, SIGMA = 0.3, 0.8, 0.2, 0.05, 0.7, 1.5


def main():
    warnings.simplefilter("ignore")
    rng = np.random.default_rng(20261021)
    zs = np.cumsum(rng.normal(size=(T, N)), axis=0) + 3.0
    x0 = rng.normal(size=(3, N))
    d = dict(zs=zs, x0=x0, params=np.array([DT, G, H, K, BETA, SIGMA]))

    # GHFilter: bank by update(), scalar by batch_filter, one run with the gains overridden per call
    f = GHFilter(x0[0].copy(), x0[1].copy(), DT, G, H)
    rec = {k: [] for k in ("x", "dx", "y", "xp", "dxp")}
    for z in zs:
        f.update(z)
        for k, v in zip(rec, (f.x, f.dx, f.y, f.x_prediction, f.dx_prediction)):
            rec[k].append(np.array(v))
    d.update({"gh_" + k: np.array(v) for k, v in rec.items()})
    f = GHFilter(float(x0[0, 0]), float(x0[1, 0]), DT, G, H)
    d["gh_batch"], d["gh_batch_pred"] = f.batch_filter(zs[:, 0], save_predictions=True)
    d["gh_vrf"] = np.array([f.VRF_prediction(), *f.VRF()])
    f = GHFilter(x0[0].copy(), x0[1].copy(), DT, 0., 0.)
    gains, xs = [], []
    for i, z in enumerate(zs):
        g, h = least_squares_parameters(i)
        f.update(z, g, h)
        gains.append((g, h))
        xs.append(np.array([f.x, f.dx]))
    d["gh_override_gains"], d["gh_override_x"] = np.array(gains), np.array(xs)

    # GHKFilter
    f = GHKFilter(x0[0].copy(), x0[1].copy(), x0[2].copy(), DT, G, H, K)
    rec = {k: [] for k in ("x", "dx", "ddx", "y", "xp", "dxp", "ddxp")}
    for z in zs:
        f.update(z)
        for k, v in zip(rec, (f.x, f.dx, f.ddx, f.y, f.x_prediction, f.dx_prediction, f.ddx_prediction)):
            rec[k].append(np.array(v))
    d.update({"ghk_" + k: np.array(v) for k, v in rec.items()})
    f = GHKFilter(float(x0[0, 0]), float(x0[1, 0]), float(x0[2, 0]), DT, G, H, K)
    d["ghk_batch"], d["ghk_batch_pred"] = f.batch_filter(zs[:, 0], save_predictions=True)
    d["ghk_vrf"] = np.array([f.VRF_prediction(), *f.VRF()])
    d["ghk_bias"] = np.array([f.bias_error(0.7)])

    for order in (0, 1, 2):
        c = order + 1
        # GHFilterOrder: bank and scalar
        for tag, start, meas in (("", x0[:c], zs), ("_s", x0[:c, 0], zs[:, 0])):
            f = GHFilterOrder(start.copy(), DT, order, G, H, K)
            xs, ys = [], []
            for z in meas:
                f.update(z)
                xs.append(f.x.copy())
                ys.append(np.array(f.y))
            d[f"gho{order}{tag}_x"], d[f"gho{order}{tag}_y"] = np.array(xs), np.array(ys)
        # FadingMemoryFilter
        for tag, start, meas in (("", x0[:c], zs), ("_s", x0[:c, 0], zs[:, 0])):
            f = FadingMemoryFilter(start.copy(), DT, order, BETA)
            xs = []
            for z in meas:
                f.update(z)
                xs.append(np.array(f.x, dtype=float).copy())
            d[f"fm{order}{tag}_x"] = np.array(xs)
        d[f"fm{order}_P"], d[f"fm{order}_e"] = f.P, f.e
        # LeastSquaresFilter: five filters side by side
        fs = [LeastSquaresFilter(DT, order, SIGMA) for _ in range(N)]
        xs, Ks, errs = [], [], []
        for t, z in enumerate(zs):
            for i, f in enumerate(fs):
                f.update(z[i])
            xs.append(np.stack([f.x for f in fs], axis=1))
            Ks.append(fs[0].K.copy())
            if fs[0].n >= 3:
                errs.append(np.array(fs[0].errors()))
        d[f"ls{order}_x"], d[f"ls{order}_K"], d[f"ls{order}_errors"] = np.array(xs), np.array(Ks), np.array(errs)

    # the helpers
    gs = [0.1, 0.35, 0.6, 0.9]
    d["h_gs"] = np.array(gs)
    d["h_optimal_noise_smoothing"] = np.array([optimal_noise_smoothing(g) for g in gs])
    d["h_least_squares_parameters"] = np.array([least_squares_parameters(n) for n in range(6)])
    d["h_critical_damping_2"] = np.array([critical_damping_parameters(g) for g in gs])
    d["h_critical_damping_3"] = np.array([critical_damping_parameters(g, 3) for g in gs])
    d["h_benedict_bordner"] = np.array([benedict_bornder_constants(g) for g in gs])
    d["h_benedict_bordner_critical"] = np.array([benedict_bornder_constants(g, True) for g in gs])

    np.savez(os.path.join(OUT, "poly_filters.npz"), **{k: np.asarray(v, dtype=np.float64) for k, v in d.items()})
    print("wrote poly_filters.npz:", len(d), "arrays")


if __name__ == "__main__":
    main()
