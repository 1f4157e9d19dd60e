#!/usr/bin/env python3
"""Fixed-lag smoother kernels (fk_fls_batch_f64, csrc/fls_kernels.hip) at 1e6 tracks x 100 steps: kernel time from HIP events
over several launches, track-steps/s, the fraction of 8 TB/s on algorithmic bytes (8 (m + 2n + nu) per track-step for z, xs and
xhat, plus 16 (n + n^2) per track once for x and P in and out), the step's FMAs as fk_fls.hpp issues them, and for scale the
plain filter at the same shape as KalmanFilterBank.batch_filter(device_outputs=True) launches it (all four histories, the two
covariance histories interleaved in one array -- the specialised kernel; a call with means only runs the generic one and is not
what the API does).  Which kernel serves a shape is read from csrc/fk_dims_fls.def.  One JSON line per row; --out writes them.

    python tools/bench_fls.py [--tracks 1000000] [--steps 100] [--reps 10] [--out profiles/fls/bench.json]
    python tools/bench_fls.py --cpu [--reference /path/to/filterpy] [--out profiles/fls/cpu.json]
        CPU figures, no GPU: tests/fls_port.py (the reference's arithmetic in NumPy) on a sample of tracks, one process on one
        core; with --reference also the live reference's FixedLagSmoother.smooth_batch on the same tracks.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(4, 2, 8), (4, 2, 16), (4, 4, 8), (5, 3, 8), (6, 2, 8), (6, 3, 8), (8, 4, 8), (9, 3, 8)]


def fast_table():
    """{(n, m): LMAX} of the fast kernel, from the instantiation list the library is built from"""
    import re
    src = open(os.path.join(ROOT, "filterpy_amd", "csrc", "fk_dims_fls.def")).read()
    return {(int(a), int(b)): int(c) for a, b, c in re.findall(r"^FK_FLS_INST\((\d+),\s*(\d+),\s*(\d+)\)", src, re.M)}


def cpu_rows(a):
    """tests/fls_port.py (and the live reference with --reference) on a sample of tracks, one core"""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import fls_port
    ref = None
    if a.reference:
        sys.path.insert(0, a.reference)
        from filterpy.kalman import FixedLagSmoother as ref
    rows = []
    for n, m, lag in SHAPES:
        rs = np.random.RandomState(n * 100 + m)
        F = np.eye(n) + 0.1 * rs.randn(n, n) / np.sqrt(n)
        Q, H, R = 0.01 * np.eye(n), rs.randn(m, n), np.eye(m)
        K, T = a.cpu_tracks, a.steps
        zs = rs.randn(K, T, m)
        x0 = rs.randn(K, n)
        t0 = time.perf_counter()
        for i in range(K):
            fls_port.smooth_batch(x0[i], np.eye(n), zs[i], lag, F, Q, H, R)
        tp = time.perf_counter() - t0
        row = dict(shape=[n, m], lag=lag, tracks=K, steps=T, cores=1, port_s=round(tp, 3), port_track_steps_per_s=K * T / tp)
        if ref is not None:
            t0 = time.perf_counter()
            for i in range(K):
                f = ref(n, m)
                f.F, f.Q, f.H, f.R, f.x, f.P = F, Q, H, R, x0[i].copy(), np.eye(n)
                f.smooth_batch(zs[i], lag)
            tr = time.perf_counter() - t0
            row.update(reference_s=round(tr, 3), reference_track_steps_per_s=K * T / tr, reference_over_port=round(tr / tp, 3))
        print(json.dumps(row), flush=True)
        rows.append(row)
    return rows


def fmas(n, m, lag):
    """the step's FMAs as fk_fls.hpp issues them (per track-step)"""
    predict = 2 * n ** 3 + n ** 2
    update = (n * n * m + n * m * m + m ** 3 // 3 + 2 * n * m * m          # P H', S, L D L', the solve for K
              + n * m + n * n * m + n ** 3 + n * n * m + n ** 3 + n * n * m)  # x, I - KH, (I-KH) P, K R, the Joseph product
    smooth = m * m + n * m + n * n * m + lag * n * n + (lag - 1) * n * n
    return predict + update + smooth


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tracks", type=int, default=1000000)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out")
    ap.add_argument("--cpu", action="store_true", help="CPU figures only (no GPU)")
    ap.add_argument("--cpu-tracks", type=int, default=20)
    ap.add_argument("--reference", help="a filterpy checkout: time its FixedLagSmoother too (--cpu)")
    a = ap.parse_args()
    if a.cpu:
        rows = cpu_rows(a)
        if a.out:
            with open(a.out, "w") as f:
                json.dump(dict(when=time.strftime("%Y-%m-%d"), cpu=os.uname().machine, rows=rows), f, indent=1)
        return
    import torch
    from filterpy_amd import _engine as E
    from filterpy_amd import _abi
    from filterpy_amd._abi import FK_MODEL_SHARED
    if os.environ.get("FK_LIB"):      # an experimental build of the library (A/B of two builds in one lease); tools only
        _abi.LIB_PATH = os.path.abspath(os.environ["FK_LIB"])
    fast = fast_table()
    torch.cuda.set_device(0)
    T = a.steps
    rows = []
    for n, m, lag in SHAPES:
        general = not ((n, m) in fast and max(lag, 1) <= fast[(n, m)])
        # the general kernel (scratch-resident, ~1e7 track-steps/s) runs a tenth of the bank: a launch is a second, not ten
        N = a.tracks // 10 if general else a.tracks
        for layout in ("soa", "aos"):
            rs = np.random.RandomState(n * 100 + m)
            F = np.eye(n) + 0.1 * rs.randn(n, n) / np.sqrt(n)
            Q, H, R = 0.01 * np.eye(n), rs.randn(m, n), np.eye(m)
            dF, dQ, dH, dR = (E.dev(v) for v in (F, Q, H, R))
            x0 = E.alloc_records((), N, n, layout).normal_()
            eye = torch.eye(n, dtype=torch.float64, device="cuda")
            P0 = eye.reshape(n * n, 1).repeat(1, N) if layout == "soa" else eye.reshape(1, n * n).repeat(N, 1)
            z = E.alloc_records((T,), N, m, layout).normal_()
            xs = E.alloc_records((T,), N, n, layout)
            xh = E.alloc_records((T,), N, n, layout)
            desc = dict(n=n, m=m, nu=0, model_mode=FK_MODEL_SHARED, N=N, T=T, layout=E.LAYOUTS[layout],
                        update_first=0, alpha_sq=1.0, flags=0)
            x, P = x0.clone(), P0.clone()
            reps = 2 if general else a.reps
            E.fls_batch(desc, lag, 0, dF, dQ, dH, dR, z, x, P, xs, xh)      # warm-up
            torch.cuda.synchronize()
            ms = []
            for _ in range(reps):
                x.copy_(x0)
                P.copy_(P0)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                E.fls_batch(desc, lag, 0, dF, dQ, dH, dR, z, x, P, xs, xh)
                e1.record()
                torch.cuda.synchronize()
                ms.append(e0.elapsed_time(e1))
            # for scale: the plain filter as KalmanFilterBank.batch_filter(device_outputs=True) launches it -- all four histories,
            # both covariance histories in one interleaved array (FK_KF_FLAG_COV_INTERLEAVED, the specialised kernel)
            kms = []
            if n < 9:
                cov2, c_il, cp_il = E.alloc_cov_pair(T, N, n, layout)
                kdesc = dict(desc, flags=_abi.FK_KF_FLAG_COV_INTERLEAVED)
            else:               # (dim_x >= 9 runs on the three-lane kernel, which takes two arrays -- as the API passes them)
                c_il, cp_il = E.alloc_records((T,), N, n * n, layout), E.alloc_records((T,), N, n * n, layout)
                cov2, kdesc = None, desc
            means, means_p = E.alloc_records((T,), N, n, layout), E.alloc_records((T,), N, n, layout)
            for _ in range(4):
                x.copy_(x0)
                P.copy_(P0)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                E.kf_batch_filter(kdesc, dF, dQ, dH, dR, z, x, P, means=means, covs=c_il, means_p=means_p, covs_p=cp_il)
                e1.record()
                torch.cuda.synchronize()
                kms.append(e0.elapsed_time(e1))
            kms = kms[1:]
            del cov2, c_il, cp_il, means, means_p
            med = float(np.median(ms))
            alg = 8.0 * (m + 2 * n) * N * T + 16.0 * (n + n * n) * N
            kern = "general" if general else "fast"
            row = dict(shape=[n, m], lag=lag, layout=layout, kernel=kern, tracks=N, steps=T, ms_median=round(med, 3),
                       ms_min=round(min(ms), 3), reps=reps, track_steps_per_s=N * T / (med * 1e-3),
                       hbm_fraction_8TBs=alg / (med * 1e-3) / 8e12, fma_per_track_step_formula=fmas(n, m, lag),
                       kalman_filter_bank_batch_filter_ms=round(float(np.median(kms)), 3))
            print(json.dumps(row), flush=True)
            rows.append(row)
            del x0, P0, z, xs, xh, x, P
            torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(dict(when=time.strftime("%Y-%m-%d"), rows=rows), f, indent=1)


if __name__ == "__main__":
    main()
