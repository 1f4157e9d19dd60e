#!/usr/bin/env python3
"""The polynomial-filter kernels (fk_poly_run, csrc/poly_kernels.hip) at 4e6 tracks x 100 steps, in one process: kernel time from
HIP events over >= 10 launches after a warm-up (medians and minima), track-steps/s, algorithmic bytes (8 in for z and
8 (order + 1) out for xs per track-step, 8 more per further history, 16 (order + 1) per track once for the state), the fraction
of 8 TB/s and the fraction of a device-to-device copy's bandwidth measured in the same process (the yardstick: the same
number of bytes, half read and half written).

Rows: the GHFilter.batch_filter shape (form A, order 1) in both layouts, xs only and xs + pred; form B order 2, form A order 0
and form C order 2 (the gains table); and the same g-h filter expressed as fk_kf_steadystate_f64 at (2,1) with K = [g, h/dt] --
the route a user had before.  That one gives other bits; its time is what is compared.  One JSON line per row; --out writes
them to a .jsonl file, written fresh.

    python tools/bench_poly.py [--tracks 4000000] [--steps 100] [--reps 10] [--out profiles/poly/bench.jsonl]
    python tools/bench_poly.py --isa [--out profiles/poly/isa.jsonl]
        no GPU: tools/isa_lint.py's facts (VGPRs, scratch, LDS, code bytes) of the seven kernels
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DT, G, H, K = 0.3, 0.8, 0.2, 0.05
# (name, order, form, layouts, output sets)
ROWS = [("GHFilter.batch_filter", 1, 0, ("soa", "aos"), (("xs",), ("xs", "pred"))),
        ("GHKFilter.update", 2, 1, ("soa",), (("xs",),)),
        ("order 0, multiply form", 0, 0, ("soa",), (("xs",),)),
        ("LeastSquaresFilter order 2", 2, 2, ("soa",), (("xs",),))]


def isa_rows():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import tempfile
    import isa_lint
    obj = os.path.join(ROOT, "filterpy_amd", "csrc", "build", "poly_kernels.o")
    rows = []
    with tempfile.TemporaryDirectory() as tmp:
        for name, k in sorted(isa_lint.kernels(isa_lint.device_elf(obj, tmp)).items()):
            rows.append(dict(object="poly_kernels.o", kernel=isa_lint.short(name), **{a: int(k[a]) for a in ("vgpr", "scratch", "lds", "code")}))
    return rows


def timed(run, reps, reset=None):
    import torch
    run()                                                   # warm-up
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        if reset:
            reset()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        run()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return float(np.median(ms)), float(min(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tracks", type=int, default=4000000)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out")
    ap.add_argument("--isa", action="store_true", help="ISA facts of the built kernels only (no GPU)")
    a = ap.parse_args()
    rows = []

    def emit(row):
        print(json.dumps(row), flush=True)
        rows.append(row)
    if a.isa:
        for r in isa_rows():
            emit(r)
    else:
        import torch
        from filterpy_amd import _engine as E
        from filterpy_amd._abi import FK_MODEL_SHARED
        from filterpy_amd.leastsq import LeastSquaresFilter
        torch.cuda.set_device(0)
        N, T, reps = a.tracks, a.steps, max(a.reps, 10)
        when = time.strftime("%Y-%m-%d")
        z = torch.empty((T, N), dtype=torch.float64, device="cuda").normal_().cumsum_(0)
        # the yardstick: a device-to-device copy that moves as many bytes as the xs-only g-h launch (8 + 16 per track-step)
        half = 12 * N * T
        src, dst = torch.empty(half, dtype=torch.uint8, device="cuda").zero_(), torch.empty(half, dtype=torch.uint8, device="cuda")
        med, mn = timed(lambda: dst.copy_(src), reps)
        copy_bw = 2.0 * half / (med * 1e-3)
        emit(dict(row="device-to-device copy", bytes=2 * half, ms_median=round(med, 3), ms_min=round(mn, 3), reps=reps,
                  bytes_per_s=copy_bw, hbm_fraction_8TBs=copy_bw / 8e12, when=when))
        del src, dst
        torch.cuda.empty_cache()
        for name, order, form, layouts, outsets in ROWS:
            C = order + 1
            lsq = LeastSquaresFilter(DT, order)
            table = E.dev(np.array([lsq._gains(n) for n in range(1, T + 1)])) if form == 2 else None
            for layout in layouts:
                x0 = E.alloc_records((), N, C, layout).normal_()
                x = x0.clone()
                for outs in outsets:
                    xs = E.alloc_records((T,), N, C, layout)
                    pred = torch.empty((T, N), dtype=torch.float64, device="cuda") if "pred" in outs else None

                    def run():
                        E.poly_run(order, form, N, T, layout, DT, DT**2., 0.5 * DT**2, G, H / DT if form == 0 else H,
                                   2 * K / DT**2 if form == 0 else 2 * K, z, x, gains=table, xs=xs, pred=pred)
                    med, mn = timed(run, reps, lambda: x.copy_(x0))
                    per = 8 * (1 + C + (1 if pred is not None else 0))
                    alg = float(per) * N * T + 16.0 * C * N
                    bw = alg / (med * 1e-3)
                    emit(dict(row=name, order=order, form="ABC"[form], layout=layout, outputs="+".join(outs), tracks=N, steps=T,
                              ms_median=round(med, 3), ms_min=round(mn, 3), reps=reps, track_steps_per_s=N * T / (med * 1e-3),
                              algorithmic_bytes_per_track_step=per, algorithmic_bytes=alg, hbm_fraction_8TBs=bw / 8e12,
                              fraction_of_copy=bw / copy_bw, when=when))
                    del xs, pred
                    torch.cuda.empty_cache()
                del x0, x
        # the g-h filter as a steady-state Kalman filter at (2,1): F = [[1, dt], [0, 1]], H = [1, 0], K = [g, h/dt]
        for layout in ("soa", "aos"):
            dF, dH, dK = E.dev(np.array([[1., DT], [0., 1.]])), E.dev(np.array([[1., 0.]])), E.dev(np.array([[G], [H / DT]]))
            x0 = E.alloc_records((), N, 2, layout).normal_()
            x = x0.clone()
            means = E.alloc_records((T,), N, 2, layout)
            desc = dict(n=2, m=1, nu=0, model_mode=FK_MODEL_SHARED, N=N, T=T, layout=E.LAYOUTS[layout], update_first=0, alpha_sq=1.0,
                        flags=0)
            med, mn = timed(lambda: E.kf_steadystate(desc, dF, dH, dK, z.reshape(T, N, 1) if layout == "aos" else z.reshape(T, 1, N),
                                                     x, means=means), reps, lambda: x.copy_(x0))
            alg = 24.0 * N * T + 32.0 * N
            bw = alg / (med * 1e-3)
            emit(dict(row="fk_kf_steadystate_f64 (2,1), the same g-h filter", layout=layout, outputs="means", tracks=N, steps=T,
                      ms_median=round(med, 3), ms_min=round(mn, 3), reps=reps, track_steps_per_s=N * T / (med * 1e-3),
                      algorithmic_bytes_per_track_step=24, algorithmic_bytes=alg, hbm_fraction_8TBs=bw / 8e12,
                      fraction_of_copy=bw / copy_bw, when=when))
            del x0, x, means
            torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
