#!/usr/bin/env python3
"""Cubature Kalman filter kernels (fk_ckf_linear_batch_f64, csrc/ckf_kernels.hip) at 1e6 tracks x 100 steps, as
CubatureKalmanFilter.batch_filter(device_outputs=True) launches them on a matrix model.  Every row is measured in a process of
its own (this script starts one child per row, one after the other): kernel time from HIP events over `--reps` launches after
a discarded warm-up launch (medians), track-steps/s, the fraction of 8 TB/s on algorithmic bytes (8 (m + 2n + 2n^2) per
track-step for z and the four histories, plus 16 (2n + 2n^2) per track once for x, P and the points record in and out), and the
step's FMA-class operations, square roots and divisions as fk_ckf.hpp issues them.  Rows:
    ckf       the fused kernel at its fast shapes (csrc/fk_dims_ckf.def), both layouts
    kf        KalmanFilterBank.batch_filter(device_outputs=True)'s launch on the same shape: it moves the same history bytes
    ukf       fk_ukf_linear_batch_f64 at (6, 3): posterior histories only, 8 (m + n + n^2) bytes per track-step
One JSON line per row; --out writes them.

    python tools/bench_ckf.py [--tracks 1000000] [--steps 100] [--reps 10] [--out profiles/ckf/bench.json]
    python tools/bench_ckf.py --isa [--out profiles/ckf/isa.json]
        no GPU: tools/isa_lint.py's facts (VGPRs, scratch, LDS, code bytes) of every object of the cubature filter
"""
import argparse
import glob
import json
import os
import re
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(2, 1), (4, 2), (6, 3), (7, 3)]


def fast_table():
    src = open(os.path.join(ROOT, "filterpy_amd", "csrc", "fk_dims_ckf.def")).read()
    return {(int(a), int(b)) for a, b in re.findall(r"^FK_CKF_SHAPE\((\d+),\s*(\d+)\)", src, re.M)}


def ops(n, m):
    """FMA-class operations (multiplies, FMAs, additions and subtractions), square roots and divisions per track-step, counted
    from the loops of fk_ckf.hpp (sqrt_rsqrt gives a pivot's root and reciprocal together: one of each per pivot; the L D L'
    of S takes one reciprocal per pivot)"""
    tri = n * (n + 1) // 2
    chol = sum(j + (n - 1 - j) * (j + 1) for j in range(n))
    points = n * n + n * sum(n - k for k in range(n))                 # c = F x;  E[k] = F U[k] on the triangle
    cov = tri * n                                                     # sum_k E[k] E[k]' + Q
    g = m * n + m + n * m * n                                         # zp, y, G
    s = (m * (m + 1) // 2) * n + n * m * n                            # S, Pxz
    ldlt = sum(2 * j + (m - 1 - j) * (2 * j + 1) for j in range(m)) if m > 1 else 0
    solve = n * (m * (m - 1) + m) if m > 1 else n
    corr = n * m + tri * m                                            # x += K y;  P -= K Pxz'
    return dict(fma=chol + points + cov + g + s + ldlt + solve + corr, sqrt=n, div=n + m)


def isa_rows():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_lint
    import tempfile
    objs = sorted(glob.glob(os.path.join(ROOT, "filterpy_amd", "csrc", "build", "ckf_fast_*.o")))
    objs += [os.path.join(ROOT, "filterpy_amd", "csrc", "build", "ckf_general.o")]
    rows = []
    with tempfile.TemporaryDirectory() as tmp:
        for o in objs:
            for name, k in sorted(isa_lint.kernels(isa_lint.device_elf(o, tmp)).items()):
                if "ckf_" not in name:
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


def one_row(kind, n, m, layout, N, T, reps):
    import torch
    from filterpy_amd import _engine as E
    from filterpy_amd import _abi
    from filterpy_amd._abi import FK_MODEL_SHARED
    torch.cuda.set_device(0)
    rs = np.random.RandomState(n * 100 + m)
    F = np.eye(n) + 0.1 * rs.randn(n, n) / np.sqrt(n)
    H = rs.randn(m, n)
    dF, dQ, dH, dR = (E.dev(v) for v in (F, 0.01 * np.eye(n), H, np.eye(m)))
    x0 = E.alloc_records((), N, n, layout).normal_()
    eye = torch.eye(n, dtype=torch.float64, device="cuda")
    P0 = eye.reshape(n * n, 1).repeat(1, N) if layout == "soa" else eye.reshape(1, n * n).repeat(N, 1)
    z = E.alloc_records((T,), N, m, layout).normal_()
    st = torch.zeros(N, dtype=torch.int32, device="cuda")
    desc = dict(n=n, m=m, nu=0, model_mode=FK_MODEL_SHARED, N=N, T=T, layout=E.LAYOUTS[layout], update_first=0, alpha_sq=1.0,
                flags=0)
    x, P = x0.clone(), P0.clone()

    def reset():
        x.copy_(x0)
        P.copy_(P0)
    means = E.alloc_records((T,), N, n, layout)
    row = dict(row=kind, shape=[n, m], layout=layout, tracks=N, steps=T, reps=reps)
    if kind == "ckf":
        means_p = E.alloc_records((T,), N, n, layout)
        covs, covs_p = E.alloc_records((T,), N, n * n, layout), E.alloc_records((T,), N, n * n, layout)
        pts = E.alloc_records((), N, n + n * n, layout).zero_()
        ms = timed(lambda: E.ckf_linear_batch(desc, dF, dQ, dH, dR, z, x, P, pts, means=means, covs=covs, means_p=means_p,
                                              covs_p=covs_p, status=st), reset, reps)
        assert int(st.abs().sum()) == 0
        per_step, once = 8 * (m + 2 * n + 2 * n * n), 16.0 * (2 * n + 2 * n * n)
        row.update(kernel="fast" if (n, m) in fast_table() else "general", **{k + "_per_track_step": v for k, v in ops(n, m).items()})
    elif kind == "kf":
        means_p = E.alloc_records((T,), N, n, layout)
        cov2, c_il, cp_il = E.alloc_cov_pair(T, N, n, layout)
        kdesc = dict(desc, flags=_abi.FK_KF_FLAG_COV_INTERLEAVED)
        ms = timed(lambda: E.kf_batch_filter(kdesc, dF, dQ, dH, dR, z, x, P, means=means, covs=c_il, means_p=means_p,
                                             covs_p=cp_il), reset, reps)
        per_step, once = 8 * (m + 2 * n + 2 * n * n), 16.0 * (n + n * n)
    else:
        from filterpy_amd.kalman import MerweScaledSigmaPoints
        pf = MerweScaledSigmaPoints(n, alpha=0.5, beta=2.0, kappa=3.0 - n)
        covs = E.alloc_records((T,), N, n * n, layout)
        Wm, Wc = E.dev(np.asarray(pf.Wm, dtype=np.float64)), E.dev(np.asarray(pf.Wc, dtype=np.float64))
        ms = timed(lambda: E.ukf_linear_batch(n, m, N, T, layout, pf.scale, dF, dH, dQ, dR, Wm, Wc, z, x, P, means=means,
                                              covs=covs, status=st), reset, reps)
        assert int(st.abs().sum()) == 0
        per_step, once = 8 * (m + n + n * n), 16.0 * (n + n * n)
    med = float(np.median(ms))
    row.update(ms_median=round(med, 3), ms_min=round(min(ms), 3), track_steps_per_s=N * T / (med * 1e-3),
               algorithmic_bytes_per_track_step=per_step, hbm_fraction_8TBs=(per_step * float(N) * T + once * N) / (med * 1e-3) / 8e12,
               device=torch.cuda.get_device_name(0))
    print(json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tracks", type=int, default=1000000)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out")
    ap.add_argument("--isa", action="store_true", help="ISA facts of the built objects only (no GPU)")
    ap.add_argument("--row", help="(internal) one row in this process: kind,n,m,layout")
    a = ap.parse_args()
    if a.isa:
        rows = isa_rows()
        if a.out:
            with open(a.out, "w") as f:
                json.dump(dict(tool="tools/isa_lint.py", rows=rows), f, indent=1)
        return
    if a.row:
        kind, n, m, layout = a.row.split(",")
        one_row(kind, int(n), int(m), layout, a.tracks, a.steps, a.reps)
        return
    todo = [("ckf", n, m, lay) for n, m in SHAPES for lay in ("soa", "aos")]
    todo += [("kf", n, m, lay) for n, m in SHAPES for lay in ("soa", "aos")]
    todo += [("ukf", 6, 3, lay) for lay in ("soa", "aos")]
    rows = []
    for kind, n, m, lay in todo:
        # a fresh process per row, one at a time; a child that fails ends the run (nothing more is started on the device)
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--row", f"{kind},{n},{m},{lay}", "--tracks", str(a.tracks),
                            "--steps", str(a.steps), "--reps", str(a.reps)], capture_output=True, text=True, timeout=600)
        if r.returncode != 0:
            print(r.stdout[-2000:], r.stderr[-2000:], file=sys.stderr)
            sys.exit(r.returncode if r.returncode > 0 else 1)
        line = [l for l in r.stdout.splitlines() if l.startswith("{")][-1]
        print(line, flush=True)
        rows.append(json.loads(line))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(dict(when=time.strftime("%Y-%m-%d"), rows=rows), f, indent=1)


if __name__ == "__main__":
    main()
