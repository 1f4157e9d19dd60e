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

--bank measures EnsembleKalmanFilterBank's two launches (fk_enkf_bank_predict_f64 / fk_enkf_bank_update_f64,
csrc/enkf_bank.hip) against what the library offered for the same job before: a Python loop over B EnsembleKalmanFilter objects
with matrix fx / hx and noise="device".  Rows: B tracks x N members at (4, 2) and (6, 3), one predict + update cycle, element-major
records.  Per row: the bank's kernel time (HIP events around its two launches), the algorithmic bytes of the cycle -- predict
3 N n doubles per track, update (2 n + m) N on the one-wave route (N <= 64: the member stays in registers) and (3 n + m) N above
-- and their fraction of 8 TB/s; for the loop its launches alone (the six launches per track issued back to back on the slices of
the same arrays, no host synchronisation; HIP events) and the class loop's wall time, which is what a user pays: every
predict() / update() of the single class downloads x, P, K, S.  The class loop runs --loop-reps times (once at B >= 10000).

    python tools/bench_enkf.py --bank [--tracks 100 1000 10000] [--sizes 32 64 256 1024] [--out profiles/enkf/bank_bench.json]
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


def _events(fn, reps, before=None):
    import torch
    ms = []
    for _ in range(reps):
        if before:
            before()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return ms


def bank_rows(a):
    import torch
    from filterpy_amd import _engine as E
    from filterpy_amd.kalman import EnsembleKalmanFilter
    from filterpy_amd.kalman.ensemble_kalman_filter import _factor
    torch.cuda.set_device(0)
    rows, layout = [], "soa"
    for n, m in [(4, 2), (6, 3)]:
        F, H, Q, R = model(n, m)
        dF, dH, dR, AQ, AR = (E.dev(v) for v in (F, H, R, _factor(Q), _factor(R)))
        for B in a.tracks:
            for N in a.sizes:
                desc = dict(n=n, m=m, nu=0, model_mode=0, N=N, T=1, layout=E.LAYOUTS[layout], update_first=0, alpha_sq=1.0, flags=0)
                sig = torch.randn((B, n, N), dtype=torch.float64, device="cuda")
                w1, w2 = torch.randn((B, n, N), dtype=torch.float64, device="cuda"), torch.randn((B, m, N), dtype=torch.float64, device="cuda")
                x, P = torch.zeros((B, n), dtype=torch.float64, device="cuda"), torch.eye(n, dtype=torch.float64, device="cuda").repeat(B, 1, 1)
                S, SI, K = (torch.empty((B,) + s, dtype=torch.float64, device="cuda") for s in ((m, m), (m, m), (n, m)))
                z = torch.zeros((B, m), dtype=torch.float64, device="cuda")
                st = torch.zeros(B, dtype=torch.int32, device="cuda")
                ws = torch.empty(E.enkf_workspace_bytes(n, m, N), dtype=torch.uint8, device="cuda")

                def bank():
                    E.enkf_bank_predict(desc, B, w1, sig, x, P, F=dF, factor=AQ, status=st)
                    E.enkf_bank_update(desc, B, dR, z, w2, sig, x, P, H=dH, factor=AR, S=S, SI=SI, K=K, status=st)

                def loop_launches():
                    for b in range(B):
                        E.enkf_predict(desc, w1[b], sig[b], x[b], P[b], ws, F=dF, factor=AQ, status=st[b:b + 1])
                        E.enkf_update(desc, dR, z[b], w2[b], sig[b], x[b], P[b], ws, H=dH, factor=AR, S=S[b], SI=SI[b], K=K[b],
                                      status=st[b:b + 1])

                def redraw():
                    w1.normal_()
                    w2.normal_()
                bank()                                                  # warm-up
                torch.cuda.synchronize()
                assert int(st.abs().max()) == 0
                ms = _events(bank, a.reps, redraw)
                assert int(st.abs().max()) == 0 and bool(torch.isfinite(x).all())
                loop_launches()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                lms = _events(loop_launches, 1 if B >= 10000 else 3, redraw)
                launch_wall = (time.perf_counter() - t0) / len(lms)
                assert int(st.abs().max()) == 0
                # the class loop: B objects, as a user of the parent commit writes it
                gen = torch.Generator(device="cuda").manual_seed(1)
                fs = [EnsembleKalmanFilter(x=np.zeros(n), P=np.eye(n), dim_z=m, dt=1., N=N, hx=H, fx=F, noise="device", generator=gen)
                      for _ in range(B)]
                for f in fs:
                    f.Q, f.R = Q, R
                zs = np.zeros(m)
                walls = []
                for rep in range(1 + (1 if B >= 10000 else a.loop_reps)):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for f in fs:
                        f.predict()
                        f.update(zs)
                    torch.cuda.synchronize()
                    walls.append(time.perf_counter() - t0)
                del fs
                med = float(np.median(ms))
                per_n = (3 * n + (2 * n + m)) if N <= 64 else (3 * n + (3 * n + m))
                alg = 8.0 * B * N * per_n
                row = dict(bank=True, shape=[n, m], layout=layout, tracks=B, members=N, route="wave" if N <= 64 else "workgroup",
                           bank_ms_median=round(med, 4), bank_ms_min=round(min(ms), 4), launches_timed=a.reps,
                           algorithmic_bytes_per_cycle=alg, hbm_fraction_8TBs=alg / (med * 1e-3) / 8e12,
                           loop_launches_ms_median=round(float(np.median(lms)), 3), loop_launches_wall_ms=round(launch_wall * 1e3, 3),
                           loop_class_wall_ms=round(float(np.median(walls[1:])) * 1e3, 3), loop_class_reps=len(walls) - 1,
                           speedup_vs_loop_launches=round(float(np.median(lms)) / med, 1),
                           speedup_vs_class_loop_wall=round(float(np.median(walls[1:])) * 1e3 / med, 1))
                print(json.dumps(row), flush=True)
                rows.append(row)
                del sig, w1, w2
                torch.cuda.empty_cache()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--members", type=int, nargs="+", default=[1 << 20, 1 << 23])
    ap.add_argument("--bank", action="store_true")
    ap.add_argument("--tracks", type=int, nargs="+", default=[100, 1000, 10000])
    ap.add_argument("--sizes", type=int, nargs="+", default=[32, 64, 256, 1024])
    ap.add_argument("--loop-reps", type=int, default=2)
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.bank:
        rows = bank_rows(a)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                json.dump(dict(when=time.strftime("%Y-%m-%d"), rows=rows), f, indent=1)
        return
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
