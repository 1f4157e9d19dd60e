#!/usr/bin/env python3
"""Ensemble Kalman filter kernels (fk_enkf_predict_f64 / fk_enkf_update_f64, csrc/enkf_kernels.hip): one predict + update per
step on the fused linear path with noise="device" (standard normals and the covariance's factor), as EnsembleKalmanFilter
launches them, at 2^20 and 2^23 members for (6, 3) and (16, 8).  Kernel time from HIP events around each step's six launches
(warm-up discarded; medians), the algorithmic bytes of the shapes -- predict 3 N n doubles (members in and out, the draws),
update (3 n + m) N doubles (members twice in and once out, the draws) -- and their fraction of 8 TB/s.  Which kernel serves a
shape is read from csrc/fk_dims_enkf.def; the general kernel is a correctness path.  torch.randn's own time is outside the
events: it is not this library's kernel.

For context only, the LIVE reference's seconds per step at N = 1e4 where a checkout exists (FILTERPY_REFERENCE): a CPU figure,
never to be read as a ratio of like things.  One JSON line per row; --out writes them.

    python tools/bench_enkf.py [--reps 10] [--members 1048576 8388608] [--out profiles/enkf/bench.json]
"""
import argparse
import json
import os
import re
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(6, 3), (16, 8)]


def fast_table():
    src = open(os.path.join(ROOT, "filterpy_amd", "csrc", "fk_dims_enkf.def")).read()
    return {(int(a), int(b)) for a, b in re.findall(r"^FK_ENKF_INST\((\d+),\s*(\d+)\)", src, re.M)}


def model(n, m):
    rs = np.random.RandomState(n * 100 + m)
    A = rs.randn(n, n)
    return (np.eye(n) + 0.05 * rs.randn(n, n) / np.sqrt(n), rs.randn(m, n) / np.sqrt(n), 0.01 * (A @ A.T / n + np.eye(n)),
            0.5 * np.eye(m))


def reference_row(N=10000, steps=3):
    ref = os.environ.get("FILTERPY_REFERENCE", "/root/reference")
    if not os.path.isdir(os.path.join(ref, "filterpy")):
        return None
    sys.path.insert(0, ref)
    try:
        from filterpy.kalman import EnsembleKalmanFilter as Ref
    finally:
        sys.path.remove(ref)
    n, m = 6, 3
    F, H, Q, R = model(n, m)
    f = Ref(x=np.zeros(n), P=np.eye(n), dim_z=m, dt=1., N=N, hx=lambda s: np.dot(H, s), fx=lambda s, dt: np.dot(F, s))
    f.Q, f.R = Q, R
    t0 = time.perf_counter()
    for _ in range(steps):
        f.predict()
        f.update(np.zeros(m))
    return dict(reference_cpu=True, shape=[n, m], members=N, s_per_step=(time.perf_counter() - t0) / steps,
                note="live reference on one CPU core: context, not a ratio of like things")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--members", type=int, nargs="+", default=[1 << 20, 1 << 23])
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch
    from filterpy_amd import _engine as E
    from filterpy_amd.kalman.ensemble_kalman_filter import _factor
    fast = fast_table()
    torch.cuda.set_device(0)
    rows = []
    for n, m in SHAPES:
        F, H, Q, R = model(n, m)
        dF, dH, dR, AQ, AR = (E.dev(v) for v in (F, H, R, _factor(Q), _factor(R)))
        for N in a.members:
            for layout in ("soa", "aos"):
                desc = dict(n=n, m=m, nu=0, model_mode=0, N=N, T=1, layout=E.LAYOUTS[layout], update_first=0, alpha_sq=1.0, flags=0)
                sig = E.alloc_records((), N, n, layout).normal_()
                w1, w2 = E.alloc_records((), N, n, layout).normal_(), E.alloc_records((), N, m, layout).normal_()
                x, P = torch.zeros(n, dtype=torch.float64, device="cuda"), torch.eye(n, dtype=torch.float64, device="cuda")
                S, SI, K = (torch.empty(s, dtype=torch.float64, device="cuda") for s in ((m, m), (m, m), (n, m)))
                z = torch.zeros(m, dtype=torch.float64, device="cuda")
                ws = torch.empty(E.enkf_workspace_bytes(n, m, N), dtype=torch.uint8, device="cuda")
                st = torch.zeros(1, dtype=torch.int32, device="cuda")

                def step():
                    E.enkf_predict(desc, w1, sig, x, P, ws, F=dF, factor=AQ, status=st)
                    E.enkf_update(desc, dR, z, w2, sig, x, P, ws, H=dH, factor=AR, S=S, SI=SI, K=K, status=st)
                step()                                                  # warm-up
                torch.cuda.synchronize()
                assert int(st[0]) == 0
                ms = []
                for _ in range(a.reps):
                    w1.normal_()
                    w2.normal_()
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    step()
                    e1.record()
                    torch.cuda.synchronize()
                    ms.append(e0.elapsed_time(e1))
                assert int(st[0]) == 0 and bool(torch.isfinite(x).all())
                med = float(np.median(ms))
                alg = 8.0 * N * (3 * n + (3 * n + m))
                row = dict(shape=[n, m], layout=layout, kernel="fast" if (n, m) in fast else "general", members=N,
                           ms_median=round(med, 4), ms_min=round(min(ms), 4), launches_timed=a.reps,
                           algorithmic_bytes_per_step=alg, hbm_fraction_8TBs=alg / (med * 1e-3) / 8e12,
                           member_steps_per_s=N / (med * 1e-3))
                print(json.dumps(row), flush=True)
                rows.append(row)
                del sig, w1, w2, ws
                torch.cuda.empty_cache()
    ref = reference_row()
    if ref:
        print(json.dumps(ref), flush=True)
        rows.append(ref)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(dict(when=time.strftime("%Y-%m-%d"), rows=rows), f, indent=1)


if __name__ == "__main__":
    main()
