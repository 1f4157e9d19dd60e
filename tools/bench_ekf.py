#!/usr/bin/env python3
"""Extended Kalman filter kernels (fk_ekf_predict_f64 / fk_ekf_update_f64 / fk_ekf_step_f64, csrc/ekf_kernels.hip) at 1e6 tracks,
one time step per launch, dims (4,2) (6,3) (8,4) in both record orders.  Device-event times over `reps` launches after a warm-up;
alternating in the same process, the route the library offered before for the same traffic: fk_kf_predict_f64, and
fk_kf_update_f64 with FK_MODEL_PER_TRACK (every track its own H; that route recomputes y = z - H x, which an EKF must not).
Per row: ms, the algorithmic bytes counted from the shapes (code below), the fraction of 8 TB/s they amount to, the fp64
operations counted from the loops of fk_ekf.hpp and which of the two bounds the launch.  The tool fails without a GPU.

    python tools/bench_ekf.py [--tracks 1000000] [--reps 10] [--out profiles/ekf/bench.json]
    python tools/bench_ekf.py --isa [--out profiles/ekf/isa.json]          (no GPU: ISA facts of the built objects)
"""
import argparse
import glob
import json
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(4, 2), (6, 3), (8, 4)]
HBM_BYTES_PER_S = 8e12
FP64_FMA_PER_S = 78.6e12 / 2          # MI355X vector fp64 peak, counted in FMA-class operations


def fast_table():
    src = open(os.path.join(ROOT, "filterpy_amd", "csrc", "fk_dims_ekf.def")).read()
    return {(int(a), int(b)) for a, b in re.findall(r"^FK_EKF_SHAPE\((\d+),\s*(\d+)\)", src, re.M)}


def algorithmic_bytes(phase, n, m, by_products):
    """bytes per track that a launch must move: records read + records written (the shared model is not counted)"""
    d = 8
    xP = n + n * n
    if phase == "predict":
        return d * 2 * xP
    hy = m * n + m
    by = (n * m + 2 * m * m + 2) if by_products else 0
    if phase == "update":
        return d * (2 * xP + hy + by)
    return d * (3 * xP + hy + by)                       # step: x, P in; posterior and next prior out


def fma_ops(phase, n, m):
    """FMA-class fp64 operations per track, counted from the loops of fk_ekf.hpp / fk_math.hpp (kf_predict; ekf_update)"""
    pred = n * n + 2 * n ** 3 + n * n + n
    ldlt = sum(2 * j + (m - 1 - j) * (2 * j + 1) for j in range(m)) if m > 1 else 0
    solve = n * (m * (m - 1) + m) if m > 1 else n
    upd = n * m * n + m * m * n + m * m + ldlt + solve + n * m + n * n * m + 2 * n ** 3 + n * m * m + n * n * m
    return dict(predict=pred, update=upd, step=pred + upd)[phase]


def isa_rows():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_lint
    import tempfile
    objs = sorted(glob.glob(os.path.join(ROOT, "filterpy_amd", "csrc", "build", "ekf_fast_*.o")))
    objs += [os.path.join(ROOT, "filterpy_amd", "csrc", "build", "ekf_general.o")]
    rows = []
    with tempfile.TemporaryDirectory() as tmp:
        for o in objs:
            for name, k in sorted(isa_lint.kernels(isa_lint.device_elf(o, tmp)).items()):
                if "ekf_" not in name:
                    continue
                row = dict(object=os.path.basename(o), kernel=isa_lint.short(name), **{a: int(k[a]) for a in ("vgpr", "scratch", "lds", "code")})
                print(json.dumps(row), flush=True)
                rows.append(row)
    return rows


def timed(run, reset, reps):
    import torch
    reset()
    run()                                                   # warm-up
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        reset()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        run()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return ms


def rows_for(n, m, layout, N, reps):
    import torch
    from filterpy_amd import _engine as E
    from filterpy_amd._abi import FK_MODEL_PER_TRACK, FK_MODEL_SHARED
    rs = np.random.RandomState(n * 100 + m)
    F = np.eye(n) + 0.1 * rs.randn(n, n) / np.sqrt(n)
    dF, dQ, dR = (E.dev(v) for v in (F, 0.01 * np.eye(n), np.eye(m)))
    x0 = E.alloc_records((), N, n, layout).normal_()
    eye = torch.eye(n, dtype=torch.float64, device="cuda")
    P0 = eye.reshape(n * n, 1).repeat(1, N) if layout == "soa" else eye.reshape(1, n * n).repeat(N, 1)
    H = E.alloc_records((), N, m * n, layout).normal_()
    y = E.alloc_records((), N, m, layout).normal_()
    x, P = x0.clone(), P0.clone()
    xp, Pp = E.alloc_records((), N, n, layout), E.alloc_records((), N, n * n, layout)
    K, S, SI = E.alloc_records((), N, n * m, layout), E.alloc_records((), N, m * m, layout), E.alloc_records((), N, m * m, layout)
    ll, maha = (torch.empty(N, dtype=torch.float64, device="cuda") for _ in range(2))
    st = torch.zeros(N, dtype=torch.int32, device="cuda")
    desc = dict(n=n, m=m, nu=0, model_mode=FK_MODEL_SHARED, N=N, T=1, layout=E.LAYOUTS[layout], update_first=0, alpha_sq=1.0, flags=0)
    pt = dict(desc, model_mode=FK_MODEL_PER_TRACK)
    by = dict(K=K, S=S, SI=SI, log_likelihood=ll, mahalanobis=maha)

    def reset():
        x.copy_(x0)
        P.copy_(P0)
    runs = {
        "predict": lambda: E.ekf_predict(desc, dF, dQ, x, P, status=st),
        "update": lambda: E.ekf_update(desc, H, dR, y, x, P, status=st, **by),
        "step": lambda: E.ekf_step(desc, H, dR, y, dF, dQ, x, P, x_post=xp, P_post=Pp, status=st, **by),
        # the earlier route: fk_kf_predict_f64, and the generic kernel with per-track H and R records (FK_MODEL_PER_TRACK wants R
        # per track too)
        "kf_predict": None, "kf_update_per_track": None,
    }
    Rpt = dR.reshape(1, m * m).repeat(N, 1) if layout == "aos" else dR.reshape(m * m, 1).repeat(1, N)
    yk, Kk, Sk, SIk = (E.alloc_records((), N, e, layout) for e in (m, n * m, m * m, m * m))
    runs["kf_predict"] = lambda: E.kf_predict(desc, dF, dQ, x, P, status=st)
    runs["kf_update_per_track"] = lambda: E.kf_update(pt, H, Rpt, y, x, P, y=yk, K=Kk, S=Sk, SI=SIk, status=st)
    ms = {k: [] for k in runs}
    for _ in range(2):                                      # the routes alternate: two passes of reps / 2 launches each
        for k, run in runs.items():
            ms[k] += timed(run, reset, max(1, reps // 2))
    out = []
    for k in runs:
        phase = k.replace("kf_", "").replace("_per_track", "")
        b = algorithmic_bytes(phase, n, m, True) + (8 * m * m if k == "kf_update_per_track" else 0)
        med = float(np.median(ms[k]))
        t_bytes, t_fma = b * N / HBM_BYTES_PER_S * 1e3, fma_ops(phase, n, m) * N / FP64_FMA_PER_S * 1e3
        out.append(dict(row=k, shape=[n, m], layout=layout, tracks=N, launches=len(ms[k]), ms_median=round(med, 4),
                        ms_min=round(min(ms[k]), 4), algorithmic_bytes_per_track=b, hbm_fraction_8TBs=round(t_bytes / med, 4),
                        fma_per_track=fma_ops(phase, n, m), floor_ms_bytes=round(t_bytes, 4), floor_ms_fp64=round(t_fma, 4),
                        bound="bytes" if t_bytes >= t_fma else "fp64 issue",
                        kernel=("fast" if (n, m) in fast_table() else "general") if not k.startswith("kf_") else "kf generic",
                        device=torch.cuda.get_device_name(0)))
    by_row = {r["row"]: r for r in out}
    s, u, p = (by_row[k]["ms_median"] for k in ("step", "update", "predict"))
    summary = dict(row="summary", shape=[n, m], layout=layout, step_ms=s, update_plus_predict_ms=round(u + p, 4),
                   step_is_faster=bool(s < u + p), ekf_update_vs_kf_per_track=round(u / by_row["kf_update_per_track"]["ms_median"], 4),
                   ekf_predict_vs_kf_predict=round(p / by_row["kf_predict"]["ms_median"], 4))
    return out + [summary]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tracks", type=int, default=1000000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out")
    ap.add_argument("--isa", action="store_true", help="ISA facts of the built objects only (no GPU)")
    a = ap.parse_args()
    if a.isa:
        rows = isa_rows()
        if a.out:
            with open(a.out, "w") as f:
                json.dump(dict(tool="tools/isa_lint.py", rows=rows), f, indent=1)
        return
    import torch
    if not torch.cuda.is_available():
        sys.exit("tools/bench_ekf.py needs a GPU (torch.cuda.is_available() is False)")
    torch.cuda.set_device(0)
    rows = []
    for n, m in SHAPES:
        for lay in ("soa", "aos"):
            for r in rows_for(n, m, lay, a.tracks, max(10, a.reps)):
                print(json.dumps(r), flush=True)
                rows.append(r)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(dict(tool="tools/bench_ekf.py", tracks=a.tracks, rows=rows), f, indent=1)


if __name__ == "__main__":
    main()
