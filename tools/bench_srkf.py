#!/usr/bin/env python3
"""Square-root Kalman filter kernels (fk_srkf_batch_f64, csrc/srkf_kernels.hip) at 1e6 tracks x 100 steps: kernel time from HIP
events over several launches, track-steps/s, the fraction of 8 TB/s on algorithmic bytes (8 (m + 2n + 2n^2) per track-step for
z and the four histories -- the factor records are full n x n --, plus 16 (n + n^2) per track once for x and P1_2 in and out),
the step's FMA-class operations, square roots and divisions as fk_srkf.hpp issues them, and for comparison the plain filter at
the same shape as KalmanFilterBank.batch_filter(device_outputs=True) launches it (all four histories, the two covariance
histories interleaved in one array).  Which kernel serves a shape is read from csrc/fk_dims_srkf.def; the general kernel runs a
tenth of the bank.  One JSON line per row; --out writes them.

    python tools/bench_srkf.py [--tracks 1000000] [--steps 100] [--reps 10] [--out profiles/srkf/bench.json]
    python tools/bench_srkf.py --isa [--out profiles/srkf/isa.json]
        no GPU: tools/isa_lint.py's facts (VGPRs, scratch, LDS, code bytes) of every object of the square-root filter
"""
import argparse
import glob
import json
import os
import re
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(2, 1), (4, 2), (6, 3), (9, 3)]


def fast_table():
    src = open(os.path.join(ROOT, "filterpy_amd", "csrc", "fk_dims_srkf.def")).read()
    return {(int(a), int(b)) for a, b in re.findall(r"^FK_SRKF_INST\((\d+),\s*(\d+)\)", src, re.M)}


def ops(n, m):
    """FMA-class operations (multiplies, FMAs, adds of the reflectors), square roots and divisions per track-step, counted from
    the loops of fk_srkf.hpp (no control input)"""
    # predict: x = F x, (F P1_2)', then n reflectors of n + 1 entries (sum of squares, scaling, w, the rank-1 update per column)
    pf = n * n + n * n * (n + 1) // 2 + sum(2 * n + 1 + (n - 1 - j) * (2 * n + 2) for j in range(n))
    # update: (H P1_2)', y; m measurement reflectors over one top row and the n bottom rows; the QR of the n x n block; the
    # triangular inverse of S1_2, K, x += K y
    uf = m * n * (n + 1) // 2 + m * n
    for j in range(m):
        uf += 2 * n + 1 + (m - 1 - j) * (2 * n + 2)
        uf += (n * (n + 1) // 2 + n + n * n) if j == 0 else n * (2 * n + 1)
    for k in range(n - 1):
        r = n - 1 - k
        uf += 2 * r + 1 + r * (2 * r + 2)
    uf += sum(i - j for i in range(m) for j in range(i)) + n * m * (m + 1) // 2 + n * m
    return dict(fma=pf + uf, sqrt=n + m + n - 1, div=2 * n + 2 * (m + n - 1) + m)


def isa_rows():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_lint
    import tempfile
    objs = sorted(glob.glob(os.path.join(ROOT, "filterpy_amd", "csrc", "build", "inst_srkf_*.o")))
    objs += [os.path.join(ROOT, "filterpy_amd", "csrc", "build", "srkf_general.o")]
    rows = []
    with tempfile.TemporaryDirectory() as tmp:
        for o in objs:
            for name, k in sorted(isa_lint.kernels(isa_lint.device_elf(o, tmp)).items()):
                if "srkf_" not in name:
                    continue
                row = dict(object=os.path.basename(o), kernel=isa_lint.short(name), **{a: int(k[a]) for a in ("vgpr", "scratch", "lds", "code")})
                print(json.dumps(row), flush=True)
                rows.append(row)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tracks", type=int, default=1000000)
    ap.add_argument("--steps", type=int, default=100)
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
    from filterpy_amd import _engine as E
    from filterpy_amd import _abi
    from filterpy_amd._abi import FK_MODEL_SHARED
    if os.environ.get("FK_LIB"):      # an experimental build of the library (A/B of two builds in one lease); tools only
        _abi.LIB_PATH = os.path.abspath(os.environ["FK_LIB"])
    fast = fast_table()
    torch.cuda.set_device(0)
    T = a.steps
    rows = []
    for n, m in SHAPES:
        general = (n, m) not in fast
        N = a.tracks // 10 if general else a.tracks
        for layout in ("soa", "aos"):
            rs = np.random.RandomState(n * 100 + m)
            F = np.eye(n) + 0.1 * rs.randn(n, n) / np.sqrt(n)
            H = rs.randn(m, n)
            dF, dQ12, dH, dR12 = (E.dev(v) for v in (F, 0.1 * np.eye(n), H, np.eye(m)))
            x0 = E.alloc_records((), N, n, layout).normal_()
            eye = torch.eye(n, dtype=torch.float64, device="cuda")
            P0 = eye.reshape(n * n, 1).repeat(1, N) if layout == "soa" else eye.reshape(1, n * n).repeat(N, 1)
            z = E.alloc_records((T,), N, m, layout).normal_()
            means, means_p = E.alloc_records((T,), N, n, layout), E.alloc_records((T,), N, n, layout)
            covs, covs_p = E.alloc_records((T,), N, n * n, layout), E.alloc_records((T,), N, n * n, layout)
            st = torch.zeros(N, dtype=torch.int32, device="cuda")
            desc = dict(n=n, m=m, nu=0, model_mode=FK_MODEL_SHARED, N=N, T=T, layout=E.LAYOUTS[layout],
                        update_first=0, alpha_sq=1.0, flags=0)
            x, P = x0.clone(), P0.clone()
            reps = 3 if general else a.reps

            def run():
                E.srkf_batch(desc, dF, dQ12, dH, dR12, z, x, P, means=means, covs=covs, means_p=means_p, covs_p=covs_p, status=st)
            run()                                                   # warm-up
            torch.cuda.synchronize()
            assert int(st.abs().sum()) == 0
            ms = []
            for _ in range(reps):
                x.copy_(x0)
                P.copy_(P0)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                run()
                e1.record()
                torch.cuda.synchronize()
                ms.append(e0.elapsed_time(e1))
            del means, means_p, covs, covs_p
            torch.cuda.empty_cache()
            # for comparison: the plain filter as KalmanFilterBank.batch_filter(device_outputs=True) launches it
            dQ, dR = E.dev(0.01 * np.eye(n)), E.dev(np.eye(m))
            if n < 9:
                cov2, c_il, cp_il = E.alloc_cov_pair(T, N, n, layout)
                kdesc = dict(desc, flags=_abi.FK_KF_FLAG_COV_INTERLEAVED)
            else:
                c_il, cp_il = E.alloc_records((T,), N, n * n, layout), E.alloc_records((T,), N, n * n, layout)
                cov2, kdesc = None, desc
            kmeans, kmeans_p = E.alloc_records((T,), N, n, layout), E.alloc_records((T,), N, n, layout)
            kms = []
            for _ in range(4):
                x.copy_(x0)
                P.copy_(P0)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                E.kf_batch_filter(kdesc, dF, dQ, dH, dR, z, x, P, means=kmeans, covs=c_il, means_p=kmeans_p, covs_p=cp_il)
                e1.record()
                torch.cuda.synchronize()
                kms.append(e0.elapsed_time(e1))
            kms = kms[1:]
            del cov2, c_il, cp_il, kmeans, kmeans_p
            med, kmed = float(np.median(ms)), float(np.median(kms))
            alg = 8.0 * (m + 2 * n + 2 * n * n) * N * T + 16.0 * (n + n * n) * N
            c = ops(n, m)
            row = dict(shape=[n, m], layout=layout, kernel="general" if general else "fast", tracks=N, steps=T,
                       ms_median=round(med, 3), ms_min=round(min(ms), 3), reps=reps, track_steps_per_s=N * T / (med * 1e-3),
                       algorithmic_bytes_per_track_step=8 * (m + 2 * n + 2 * n * n), hbm_fraction_8TBs=alg / (med * 1e-3) / 8e12,
                       fma_per_track_step=c["fma"], sqrt_per_track_step=c["sqrt"], div_per_track_step=c["div"],
                       kalman_filter_bank_batch_filter_ms=round(kmed, 3), srkf_over_kf=round(med / kmed, 3))
            print(json.dumps(row), flush=True)
            rows.append(row)
            del x0, P0, z, x, P, st
            torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(dict(when=time.strftime("%Y-%m-%d"), rows=rows), f, indent=1)


if __name__ == "__main__":
    main()
