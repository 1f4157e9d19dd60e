#!/usr/bin/env python3
"""bench.py -- headline benchmark: track-steps/sec (predict+update) at dim_x=4, dim_z=2.

Workload = BASELINE.json configs[1]: 1e6 independent dim_x=4 dim_z=2 constant-velocity
tracks x 100 steps, fp64, shared F/H/Q/R, one fk_kf_batch_filter_f64 launch per "step"
(= one full batch_filter pass: T predict+update per track, all four outputs of
KalmanFilter.batch_filter written: means, covariances, means_p, covariances_p).
Inputs (z, x0, P0) are resident in HBM before the timed region.

    python bench.py --gpus N --steps K --warmup W [--dump-outputs DIR] [--full]

A plain run sets up, warms up, times the K steps and prints the headline line.  --dump-outputs DIR then also writes
what the last timed step computed for a fixed, seeded sample of tracks (DIR/<name>.npy, float64, < 64 MB), so two
builds can be compared output for output.  --full adds everything else the line has carried: the parity check
against the oracle, the other placements' launch times, the roofline, GPU clocks, HBM probes, the CPU baseline and
the rows of BASELINE configs[2..4].

N > 1: one rank per GPU under torch.distributed.run -- either the caller launches it that way
(RANK / LOCAL_RANK / WORLD_SIZE / MASTER_* in the environment) or, when `python bench.py --gpus N`
is started bare, this file re-executes itself under torch.distributed.run with N ranks (and exits
with an error if the node has fewer than N GPUs).  Tracks shard across ranks (weak scaling: every
rank filters its own 1e6 tracks, no data-path collective), then one RCCL all-gather of the summary
state (final x of every track) per step.

Prints ONE JSON line (rank 0); with --full it also holds `roofline` (HBM) and, at N=1, `cpu_baseline`
(the NumPy oracle = the reference's algorithm, timed on this host's cores).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0          # MI355X spec (MI355X_MICROARCH.md: 8.0 TB/s; ~6.3 TB/s achievable)


# ---------------------------------------------------------------- workload --
def c2_model():
    """dt=1 constant velocity in 2-D; H picks the two positions."""
    F1 = np.array([[1., 1.], [0., 1.]])
    F = np.kron(np.eye(2), F1)
    H = np.array([[1., 0., 0., 0.], [0., 0., 1., 0.]])
    q = np.array([[.25, .5], [.5, 1.]]) * 0.01          # Q_discrete_white_noise(2, 1., 0.01)
    Q = np.kron(np.eye(2), q)
    R = 4.0 * np.eye(2)
    return F, Q, H, R


def c2_inputs(N, T, seed=1):
    """Host (NumPy) inputs for N tracks: x0 = 0, P0 = 100 I, z = H x_true + 2 randn."""
    F, _, H, _ = c2_model()
    rs = np.random.RandomState(seed)
    xt = rs.randn(N, 4) * np.array([10., 1., 10., 1.])
    zs = np.empty((T, N, 2))
    for t in range(T):
        xt = xt @ F.T
        zs[t] = xt @ H.T + 2.0 * rs.randn(N, 2)
    return np.zeros((N, 4)), np.tile(100.0 * np.eye(4), (N, 1, 1)), zs


def c2_inputs_device(N, T, layout, seed, device):
    """SURVEY 8d's C2 distribution drawn on the GPU (1.6 GB of z at N = 1e6: ~15 s of `RandomState.randn` on a host
    core, every run).  The ONE buffer made here feeds every path of the run: the timed kernel, the oracle of the parity
    check (2048 tracks downloaded from it) and the CPU baseline (its first 16384 tracks downloaded) -- GPU and CPU
    filter identical arrays.  Returns device records x0, P0, z in `layout`."""
    import torch
    from filterpy_amd import _engine as E
    F, _, H, _ = c2_model()
    g = torch.Generator(device=device)
    g.manual_seed(seed)
    Fd, Hd = E.dev(F), E.dev(H)
    xt = torch.randn(N, 4, generator=g, device=device, dtype=torch.float64) * torch.tensor(
        [10., 1., 10., 1.], device=device, dtype=torch.float64)
    z = E.alloc_records((T,), N, 2, layout)
    for t in range(T):
        xt = xt @ Fd.T
        zt = xt @ Hd.T + 2.0 * torch.randn(N, 2, generator=g, device=device, dtype=torch.float64)
        z[t] = zt if layout == "aos" else zt.T
    x0 = torch.zeros((N, 4) if layout == "aos" else (4, N), dtype=torch.float64, device=device)
    P0 = (100.0 * torch.eye(4, dtype=torch.float64, device=device)).reshape(1, 16).repeat(N, 1)
    P0 = P0.contiguous() if layout == "aos" else P0.T.contiguous()
    return x0, P0, z


# ------------------------------------------------------------ CPU baseline --
CPU_TRACKS_PER_PROC = 64


def _cpu_worker(args):
    zs, budget_s = args                                  # zs (T, 64, 2): this worker's tracks of the timed GPU buffer
    from oracle import kf_oracle
    F, Q, H, R = c2_model()
    T, ntracks = zs.shape[0], zs.shape[1]
    x0, P0 = np.zeros(4), 100.0 * np.eye(4)
    zl = [list(zs[:, i]) for i in range(ntracks)]
    done = 0
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < budget_s:
        kf_oracle.kf_batch_filter(x0, P0, zl[done % ntracks], F, Q, H, R)
        done += 1
    return done, time.perf_counter() - t0


def cpu_quota():
    """(cpus this process may run on, cgroup cpu.max as text) -- a container quota caps the host baseline"""
    avail = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    quota = None
    for path in ("/sys/fs/cgroup/cpu.max", "/sys/fs/cgroup/cpu/cpu.cfs_quota_us"):
        try:
            with open(path) as fh:
                quota = fh.read().strip()
            break
        except OSError:
            pass
    return avail, quota


def cpu_baseline(zs_host, budget_s=12.0, max_procs=None):
    """The NumPy oracle (= the reference's per-epoch NumPy loop, oracle/kf_oracle.py) on the host cores: single-threaded
    processes, each filtering 64 tracks of the SAME measurements the GPU just filtered (`zs_host` (T, K, 2), downloaded
    from the timed buffer).  The process count is swept -- 256 processes on these hosts measured HALF of what 64 did
    (SMT / quota: VERDICT r2 weak 10) -- and the best count is the stated baseline; the whole sweep is in `sample`."""
    import multiprocessing as mp
    avail, quota = cpu_quota()
    top = max(1, min(avail, max_procs) if max_procs else avail)
    qn = None                                           # cpus the cgroup quota allows ("max 100000" = no quota)
    try:
        a_, b_ = (quota or "").split()[:2]
        qn = max(1, int(a_) // int(b_)) if a_ != "max" else None
    except (ValueError, ZeroDivisionError):
        pass
    cand = {8, 16, 32, 64, 128, 256, top} | ({qn, 2 * qn} if qn else set())
    counts = sorted({c for c in cand if c <= top}) or [top]
    counts = [c for c in counts if c * CPU_TRACKS_PER_PROC <= zs_host.shape[1]] or [max(1, zs_host.shape[1] // CPU_TRACKS_PER_PROC)]
    per = max(1.0, budget_s / len(counts))
    T = zs_host.shape[0]
    for v in ("OMP_NUM_THREADS", "OPENBLAS_NUM_THREADS", "MKL_NUM_THREADS"):
        os.environ[v] = "1"
    # the workers are CPU-only: under `rocprofv3 -- python bench.py` they must not inherit the profiler (hundreds of
    # processes each attaching the tool -- and, in a --pmc pass, the counters -- stalled the r02 evidence run)
    scrubbed = {k: os.environ.pop(k) for k in list(os.environ)
                if k.startswith(("ROCP", "ROCPROF", "HSA_TOOLS", "ROCTRACER")) or
                (k == "LD_PRELOAD" and "rocprof" in os.environ[k])}
    ctx = mp.get_context("spawn")
    slices = [np.ascontiguousarray(zs_host[:, c * CPU_TRACKS_PER_PROC:(c + 1) * CPU_TRACKS_PER_PROC]) for c in range(max(counts))]
    sweep = []
    try:
        with ctx.Pool(max(counts)) as pool:
            pool.map(_cpu_worker, [(sl, 0.05) for sl in slices], chunksize=1)     # start-up / import warm-up
            for c in counts:             # c tasks of `per` seconds on a pool of max(counts) workers = c busy processes
                t0 = time.perf_counter()
                res = pool.map(_cpu_worker, [(slices[i], per) for i in range(c)], chunksize=1)
                wall = time.perf_counter() - t0
                tracks = sum(r[0] for r in res)
                sweep.append({"procs": c, "track_steps_per_s": tracks * T / wall, "tracks": tracks, "wall_s": round(wall, 2)})
    finally:
        os.environ.update(scrubbed)
    best = max(sweep, key=lambda r: r["track_steps_per_s"])
    return {"value": best["track_steps_per_s"], "unit": "track-steps/s", "cores": best["procs"], "kind": "port",
            "sample": f"best of a process-count sweep, {per:.1f} s each, single-threaded procs x 64 tracks x {T} steps of the "
                      f"measurements the GPU filtered (downloaded from the timed buffer) through the NumPy oracle of "
                      f"KalmanFilter.batch_filter; host: {avail} cpus, cgroup cpu.max = {quota!r}; sweep: "
                      + ", ".join(f"{r['procs']} procs -> {r['track_steps_per_s']:.3g}/s" for r in sweep),
            "sweep": sweep, "host_cpus": avail, "cgroup_cpu_max": quota}


def pmc_traffic(layout, placement="none"):
    """HBM bytes per launch of the dominant kernel from the COMMITTED rocprofv3 PMC summary of this same command
    (profiles/pmc_traffic.json: FETCH_SIZE x2 per the gfx950 correction + WRITE_SIZE, separate --pmc passes, reduced by
    tools/pmc_summary.py).  Counters cannot be read from inside an unprofiled run, so this is not a live measurement:
    the line says where the number comes from (`traffic_source`).  (None, None) if no summary is committed."""
    try:
        with open(os.path.join(ROOT, "profiles", "pmc_traffic.json")) as fh:
            allrec = json.load(fh)
            rec = allrec.get(f"{layout}_{placement}") or allrec[layout]
        return rec["hbm_bytes_per_launch"], ("committed rocprofv3 --pmc passes of this command (not collected in this run): "
                                             + rec.get("source", "profiles/pmc_traffic.json"))
    except (OSError, KeyError, ValueError):
        return None, None


def hbm_probes(device):
    """Streaming probes of the box next to the measurement (boxes of the pool differ by 15 % on the
    headline kernel with identical clock readings): a 4 GiB `fill_` (write-only) and a 2 GiB -> 2 GiB `copy_`
    (read + write), best of 5, in GB/s of bytes moved."""
    import torch
    out = {}
    try:
        buf = torch.empty(1 << 29, dtype=torch.float64, device=device)          # 4 GiB
        half = buf.numel() // 2
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]

        def best(fn, nbytes):
            fn()
            ts = []
            for _ in range(5):
                ev[0].record()
                fn()
                ev[1].record()
                torch.cuda.synchronize()
                ts.append(ev[0].elapsed_time(ev[1]))
            return nbytes / (min(ts) * 1e-3) / 1e9
        out["fill_GBs"] = best(lambda: buf.fill_(1.0), buf.numel() * 8.0)
        out["copy_GBs"] = best(lambda: buf[:half].copy_(buf[half:]), buf.numel() * 8.0)
        del buf
    except Exception as e:                     # the measurement does not depend on it
        out["error"] = repr(e)
    return out


def baseline_configs(reps=10):
    """The other GPU workloads of BASELINE.json -- configs[2] (1e5 tracks (9,3): batch_filter + rts_smoother), configs[3] (UKF
    (6,3), 1e5 tracks: Merwe sigma points / unscented transform standalone and the fused 100-step filter) and configs[4]
    (systematic_resample: 1000 filters x 8000 particles, and one GPU's share of 1000 x 8e6 = 125 filters x 8e6 particles) --
    AFTER the timed headline region, `reps` event-timed launches each (median), every row checked against the oracle on a
    sample (tools/bench_configs.py holds the workloads; the full-size parity tests are tests/test_gpu_baseline_configs.py).
    Not part of `value`; a row that fails is reported as {"name", "error"} and the line still prints."""
    import torch
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import bench_configs as bc
    rows, out = [], []
    bc.ROWS, bc.REPS = rows, max(1, int(reps))
    jobs = [("configs[2] " + lay, (lambda lay=lay: bc.config3(lay, 100_000, 100))) for lay in ("aos", "soa")]
    jobs += [("configs[3] " + lay, (lambda lay=lay: bc.config4(lay, 100_000, 100, sizes=(1,)))) for lay in ("aos", "soa")]
    jobs += [("configs[4]", lambda: bc.config5(shapes=((1000, 8000), (125, 8_000_000)), stratified=False))]
    try:
        for name, job in jobs:
            before = len(rows)
            try:
                job()
            except Exception as exc:                       # the headline does not depend on it
                out.append({"name": name, "error": repr(exc)[:300]})
            for r in rows[before:]:
                row = {"name": r["kernel"], "config": r.get("config"), "kernel": r.get("kernel_fn"), "kernel_ms": r["ms"],
                       "launches_timed": bc.REPS, "units": r["units"], "unit": r["unit"],
                       "algorithmic_bytes": r["units"] * r["alg_bytes_per_unit"], "achieved_GBs": r["achieved_GBs"],
                       "frac": r["frac_of_8TBs"]}
                for k in ("parity_max_rel", "bit_exact", "status_flagged"):
                    if k in r:
                        row[k] = r[k]
                out.append(row)
            torch.cuda.empty_cache()
    finally:
        bc.ROWS, bc.REPS = None, None
    return out


def parity_rel_err(got, ref):
    """Worst normwise relative error over (step, track) records: max|got - ref| / max|ref| per vector / matrix
    (tests/conftest.py::rel_err_rows).  A record whose reference is exactly zero (means_p at t = 0 with
    x0 = 0) is measured absolutely; any NaN / Inf in `got` makes the result non-finite, which fails."""
    g2 = np.asarray(got, dtype=float).reshape(got.shape[0] * got.shape[1], -1)
    r2 = np.asarray(ref, dtype=float).reshape(g2.shape)
    scale = np.max(np.abs(r2), axis=1)
    scale[scale == 0] = 1.0
    d = np.max(np.abs(g2 - r2), axis=1) / scale
    return float("nan") if not np.all(np.isfinite(g2)) else float(np.max(d))


DUMP_TRACKS = 1536                     # x 100 steps x 40 doubles (x, P, x_p, P_p) = 49 MB: under the 64 MB of --dump-outputs


def dump_sample(N, k=DUMP_TRACKS):
    """The tracks --dump-outputs writes: the first k/3 and a seeded random 2k/3 of the rest (all of them when N <= k).
    Fixed for a given N, so two runs with the same arguments write the same records."""
    if N <= k:
        return np.arange(N)
    head = k // 3
    rs = np.random.RandomState(20240613)
    return np.concatenate([np.arange(head), head + np.sort(rs.choice(N - head, size=k - head, replace=False))])


def dump_outputs(path, sample, got):
    """--dump-outputs: the four batch_filter outputs of the sampled tracks, (T, K, n) / (T, K, n, n) float64 in NumPy order
    whatever the layout, and the sampled track indices."""
    os.makedirs(path, exist_ok=True)
    arrays = dict(zip(("means", "covs", "means_p", "covs_p"), got), tracks=sample)
    for name, a in arrays.items():
        np.save(os.path.join(path, name + ".npy"), np.ascontiguousarray(a, dtype=np.float64))


def gpu_clocks():
    """sclk / mclk / power of GPU 0 from rocm-smi (recorded next to the measurement: boxes of the pool differ)."""
    import subprocess
    try:
        txt = subprocess.run(["rocm-smi", "-d", "0", "--showclocks", "--showpower", "--showperflevel", "--showmaxpower",
                              "--showmemorypartition", "--showcomputepartition", "--json"], capture_output=True,
                             text=True, timeout=30).stdout
        card = next(iter(json.loads(txt).values()))
        keep = {k: v for k, v in card.items()
                if any(t in k.lower() for t in ("sclk", "mclk", "fclk", "power", "perf", "partition"))}
        try:
            with open("/sys/kernel/mm/transparent_hugepage/enabled") as fh:
                keep["thp"] = fh.read().strip()
        except OSError:
            pass
        try:                                   # WHICH physical GPU this is: the boxes of the pool are not equally fast
            import re
            st = subprocess.run(["amd-smi", "static", "-g", "0"], capture_output=True, text=True, timeout=30).stdout
            for key in ("ASIC_SERIAL", "OAM_ID", "VERSION", "MODEL_NUMBER", "FRU_ID", "VENDOR"):   # (VENDOR: the first is the GPU's, see vram_vendor)
                mm = re.search(r"^\s*" + key + r":\s*(\S+)", st, re.M)
                if mm:
                    keep[key.lower()] = mm.group(1)
            mm = re.search(r"VRAM:\s*\n\s*TYPE:\s*(\S+)\s*\n\s*VENDOR:\s*(\S+)", st)
            if mm:
                keep["vram"] = mm.group(1) + " " + mm.group(2)
        except Exception:
            pass
        return keep or None
    except Exception as e:                     # the measurement does not depend on it
        return {"error": repr(e)}


def clocks_under_load(step, seconds=1.0):
    """sclk / power of THIS GPU sampled from sysfs WHILE the benchmark kernel runs back to back (two
    boxes with identical idle clock readings differ by 15-25 % on the headline kernel -- idle readings cannot show a
    box that holds a lower clock under this kernel's load).  Not part of the timed region."""
    import glob
    import re
    import subprocess
    import threading
    import torch
    out = {}
    try:
        bdf = None
        st = subprocess.run(["amd-smi", "static", "-g", "0"], capture_output=True, text=True, timeout=30).stdout
        mm = re.search(r"BDF:\s*(\S+)", st)
        if mm:
            bdf = mm.group(1).lower()
        cards = [d for d in glob.glob("/sys/class/drm/card*/device") if bdf and os.path.realpath(d).lower().endswith(bdf)]
        if not cards:
            return {"error": f"no sysfs card for BDF {bdf}"}
        dev = cards[0]
        hw = (glob.glob(os.path.join(dev, "hwmon", "hwmon*")) or [None])[0]
        samples = {"sclk_mhz": [], "power_w": [], "busy": []}
        stop = threading.Event()

        def read(path):
            try:
                with open(path) as fh:
                    return fh.read()
            except OSError:
                return ""

        def sampler():
            while not stop.is_set():
                cur = re.search(r"(\d+)Mhz \*", read(os.path.join(dev, "pp_dpm_sclk")))
                if cur:
                    samples["sclk_mhz"].append(int(cur.group(1)))
                if hw:
                    pw = read(os.path.join(hw, "power1_average")) or read(os.path.join(hw, "power1_input"))
                    if pw.strip().isdigit():
                        samples["power_w"].append(int(pw) / 1e6)
                b = read(os.path.join(dev, "gpu_busy_percent")).strip()
                if b.isdigit():
                    samples["busy"].append(int(b))
                time.sleep(0.004)
        th = threading.Thread(target=sampler, daemon=True)
        torch.cuda.synchronize()
        th.start()
        t0 = time.perf_counter()
        n = 0
        while time.perf_counter() - t0 < seconds:
            for _ in range(8):
                step()
            torch.cuda.synchronize()
            n += 8
        stop.set()
        th.join(timeout=2)
        out["launches"] = n
        out["ms_per_launch_in_burst"] = 1e3 * (time.perf_counter() - t0) / max(1, n)
        for k, v in samples.items():
            if v:
                vs = sorted(v)
                out[k] = {"min": vs[0], "median": vs[len(vs) // 2], "max": vs[-1], "n": len(vs)}
    except Exception as e:                     # the measurement does not depend on it
        out["error"] = repr(e)
    return out


def selftest_cpu(args):
    """--selftest-cpu: the N-rank control flow of this file (env -> process group -> contiguous shards -> per-step
    all-gather of the summary state -> barrier + max-over-ranks timing -> ONE JSON line on rank 0) on the gloo
    backend with CPU tensors.  The kernel launch is replaced by a stub that writes a known function of the
    global track index, so the gathered state can be checked; nothing here is a measurement."""
    import torch
    import torch.distributed as dist
    from filterpy_amd import parallel
    world_env = int(os.environ.get("WORLD_SIZE", "1"))
    if args.gpus != world_env:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world_env}: launch one rank per GPU")
    rank, world = parallel.init_from_env(backend="gloo", force=args.force_dist)
    exchange = world > 1 or args.force_dist
    n = 4
    if args.scaling == "strong":                   # --tracks in total (capped: 1001, so that two ranks get ragged shards)
        total = min(args.tracks, 1001)
        lo, hi = parallel.shard_bounds(total, rank, world)
        N, N_pad = hi - lo, -(-total // world)
    else:
        N = N_pad = min(args.tracks, 1000)
        lo, total = rank * N, N * world
    ragged = exchange and N != N_pad
    # the same double-buffered, overlapped exchange as the GPU path (parallel.SummaryExchange; async work handles on gloo)
    xb = [torch.empty(N, n, dtype=torch.float64) for _ in range(2)]
    sb = [torch.zeros(N_pad, n, dtype=torch.float64) for _ in range(2)] if ragged else None
    ex = parallel.SummaryExchange(like=sb[0] if ragged else xb[0], depth=2) if exchange else None

    def stub(k):                                   # a known function of (step, global track index)
        return (torch.arange(N * n, dtype=torch.float64).reshape(N, n) + lo * n) * 0.5 + 1000.0 * k

    def step(k):
        slot = k % 2
        if ex:
            ex.acquire(slot)
        xb[slot].copy_(stub(k))                                                                    # stub "kernel"
        if ex:
            if ragged:
                sb[slot][:N].copy_(xb[slot])
            ex.post(sb[slot] if ragged else xb[slot], slot)

    for k in range(args.warmup):
        step(k)
    if ex:
        ex.drain()
    parallel.barrier()
    t0 = time.perf_counter()
    for k in range(args.steps):
        step(k)
    if ex:
        ex.drain()
    parallel.barrier()
    elapsed = parallel.max_over_ranks(time.perf_counter() - t0)
    ok = True
    if exchange:
        for k in range(max(0, args.steps - 2), args.steps):         # the last two steps still sit in the two slots
            want = torch.arange(total * n, dtype=torch.float64).reshape(total, n) * 0.5 + 1000.0 * k
            got = torch.cat([ex.gathered[k % 2][r][:parallel.shard_bounds(total, r, world)[1] - parallel.shard_bounds(total, r, world)[0]]
                             if args.scaling == "strong" else ex.gathered[k % 2][r] for r in range(world)])
            ok = ok and bool(torch.equal(got, want))
    if rank == 0:
        print(json.dumps({"metric": "selftest", "value": None, "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
                          "ms_per_step": 1e3 * elapsed / max(1, args.steps), "data": "selftest-stub", "gather_ok": ok,
                          "scaling": args.scaling, "tracks_total": total, "tracks_rank0": N,
                          "collectives": parallel.collectives_active()}), flush=True)
    parallel.shutdown()
    if not ok:
        raise SystemExit("selftest: gathered summary state is wrong")


# -------------------------------------------------------------------- main --
def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--tracks", type=int, default=1_000_000, help="tracks per GPU (--scaling weak) / in total (--scaling strong)")
    ap.add_argument("--scaling", default=os.environ.get("FK_BENCH_SCALING", "weak"), choices=["weak", "strong"],
                    help="weak (default; the driver's scaling run): every rank filters --tracks tracks of its own.  strong: "
                         "BASELINE configs[1] read literally -- --tracks tracks IN TOTAL, rank r the contiguous shard "
                         "parallel.shard_bounds(tracks, r, N) (125000 per GPU at N = 8: launch and tail cost show)")
    ap.add_argument("--full", action="store_true",
                    help="besides the headline: the parity check against the oracle, the launch time of every placement, the "
                         "roofline, GPU clocks and HBM probes, the CPU baseline and the rows of BASELINE configs[2..4] (all after "
                         "the timed region).  Off: the run does only what the headline needs")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write the four outputs of the last step for a fixed, seeded sample of tracks "
                         "(rank 0's) as DIR/<name>.npy, float64, under 64 MB in all")
    ap.add_argument("--no-configs", action="store_true",
                    help="with --full: skip the rows of BASELINE configs[2..4] (the line's \"configs\" key; after the timed region, rank 0 at N = 1 only)")
    ap.add_argument("--config-reps", type=int, default=10, help="event-timed launches per row of \"configs\"")
    ap.add_argument("--T", type=int, default=100)
    ap.add_argument("--layout", default=os.environ.get("FK_BENCH_LAYOUT", "aos"), choices=["soa", "aos"],
                    help="record layout of z and the outputs: aos = NumPy C order [T][N][n][n] (default), soa = [T][n*n][N]")
    ap.add_argument("--no-cpu", action="store_true", help="with --full: skip the CPU baseline")
    ap.add_argument("--placement", default=os.environ.get("FK_BENCH_PLACEMENT", "auto"), choices=["auto", "interleave", "probe", "none"],
                    help="how the two covariance histories (76 %% of the bytes) are allocated -- every mode is a mode of the product "
                         "API KalmanFilterBank.batch_filter(device_outputs=True, ...).  auto (default) = the API called without "
                         "further arguments: what a caller gets without reading docs/PLACEMENT.md -- at this size (dim_x <= 4, "
                         "histories of 256 MiB and more) two arrays placed in HBM by timing this launch on candidate buffers "
                         "(filterpy_amd/placement.py: placed_pair; once per shape, candidates one at a time -- at most 11 / half of the free memory --, stopping at the first fast pair; the "
                         "losers freed), the interleaved array where that cannot run; interleave: placement='interleave', both "
                         "histories in ONE array, a track's posterior and prior record side by side (FK_KF_FLAG_COV_INTERLEAVED); "
                         "probe: placement='probe' (like auto, falling back to two plain arrays); none: cov_interleave=False, two "
                         "plain arrays.  The line reports the launch time of all three arrangements on this box (`placement`), the "
                         "timed loop runs the one named here.")
    ap.add_argument("--cpu-seconds", type=float, default=12.0, help="total budget of the CPU baseline's process-count sweep")
    ap.add_argument("--cpu-procs", type=int, default=0, help="cap the CPU baseline's process count (0 = every host core)")
    ap.add_argument("--force-dist", action="store_true",
                    help="with one rank: still create the (1-rank) RCCL process group and run the per-step all-gather, the barrier "
                         "and the max-over-ranks all-reduce on it -- executes the code an N-GPU run executes on a one-GPU box")
    ap.add_argument("--parity-tracks", type=int, default=1024,
                    help="parity sample: the first K tracks + K random tracks of the timed buffers against the oracle")
    ap.add_argument("--selftest-cpu", action="store_true",
                    help="TEST ONLY (tests/test_parallel_gloo.py): drive the launch / shard / all-gather / timing path with the "
                         "gloo backend on CPU tensors and a stub in place of the kernel launch; the line it prints is marked "
                         "\"data\": \"selftest-stub\" and carries no measurement")
    args = ap.parse_args()

    from filterpy_amd import parallel
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # `python bench.py --gpus N` without a launcher: become `torch.distributed.run` with one rank per GPU
        parallel.relaunch_under_torchrun(args.gpus, [os.path.abspath(__file__)] + sys.argv[1:],
                                         require_devices=not args.selftest_cpu)
    if args.selftest_cpu:
        return selftest_cpu(args)

    import torch
    import torch.distributed as dist
    from filterpy_amd import _engine as E, _abi
    from oracle import kf_oracle

    world = int(os.environ.get("WORLD_SIZE", "1"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if args.gpus != world:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}: launch one rank per GPU")
    if not torch.cuda.is_available() or torch.cuda.device_count() <= local_rank:
        raise SystemExit(f"rank {local_rank}: no GPU {local_rank} visible ({torch.cuda.device_count()} device(s)); "
                         "bench.py has no CPU path")
    torch.cuda.set_device(local_rank)
    device = torch.device("cuda", local_rank)
    rank, world = parallel.init_from_env(backend="nccl", device=device, force=args.force_dist)
    exchange = world > 1 or args.force_dist

    T, layout, n, m = args.T, args.layout, 4, 2
    if args.scaling == "strong":
        lo_, hi_ = parallel.shard_bounds(args.tracks, rank, world)
        N, N_total = hi_ - lo_, args.tracks
        N_pad = -(-args.tracks // world)                   # equal-shaped summary buffers for the all-gather (shards differ by <= 1)
    else:
        N, N_total, N_pad = args.tracks, args.tracks * world, args.tracks
    F, Q, H, R = c2_model()
    dF, dQ, dH, dR = (E.dev(M, device) for M in (F, Q, H, R))
    x0, P0, z = c2_inputs_device(N, T, layout, seed=1234 + rank, device=device)
    x, P = x0.clone(), P0.clone()
    # measurement knob (tools/gpu_scripts/slow_box_probe.sh): FK_BENCH_PAD_MB=k puts k MiB of unused allocation between
    # the output arrays -- it moves their relative placement in HBM and nothing else
    pad_mb = int(os.environ.get("FK_BENCH_PAD_MB", "0"))
    pads = []

    def records(width):
        if pad_mb:
            pads.append(torch.empty(pad_mb << 20, dtype=torch.uint8, device=device))
        return E.alloc_records((T,), N, width, layout, device)

    means, covs, means_p, covs_p = records(n), records(n * n), records(n), records(n * n)
    status = torch.zeros(N, dtype=torch.int32, device=device)
    # The summary exchange (final x of every track, all-gathered over RCCL / xGMI) is overlapped with the NEXT step's launch:
    # side stream + events, two x buffers and two gathered buffers (parallel.SummaryExchange).  The kernel never waits for
    # the collective; its duration is reported apart (allgather_ms).
    xbuf = [x, x0.clone()] if exchange else [x]
    # strong scaling with shards that differ by one track: the collective wants equal shapes, so the summary leaves through a
    # zero-padded copy of N_pad records (a 4 MB device copy on the exchange's side of the step, only in that case)
    ragged = exchange and N != N_pad
    sbuf = [torch.zeros((N_pad, n) if layout == "aos" else (n, N_pad), dtype=torch.float64, device=device) for _ in range(2)] if ragged else None
    ex = parallel.SummaryExchange(like=sbuf[0] if ragged else x, depth=2) if exchange else None
    desc = dict(n=n, m=m, nu=0, model_mode=0, N=N, T=T, layout=E.LAYOUTS[layout], update_first=0, alpha_sq=1.0)

    # Where the two covariance histories (76 % of the bytes) sit in HBM decides 5.2 .. 6.9 ms of this kernel on one and the
    # same GPU (filterpy_amd/placement.py): two write streams inside one class of physical memory are
    # slower than two streams in different classes, and the driver picks the backing.  Round 4 moved the cures into the
    # product API (KalmanFilterBank.batch_filter(device_outputs=True, ...)): its default gives both histories ONE array with a
    # track's posterior and prior record side by side, written together (one front: 5.5-5.75 ms on every allocation, where
    # two plain arrays range over 5.3-6.7); placement="probe" places two arrays by timing the launch on candidate buffers
    # (5.2 ms).  All of it outside the timed region; the arithmetic and every stored value are the same.
    def one_launch_ms(cv, cvp):
        x.copy_(x0)
        P.copy_(P0)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        E.kf_batch_filter(desc, dF, dQ, dH, dR, z, x, P, means=means, covs=cv, means_p=means_p, covs_p=cvp, status=status)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    # All three arrangements are timed on this box (3 launches each, outside the timed region) and reported in the line;
    # the timed loop then runs the one --placement names.
    placement_info = {"method": {"none": "two plain arrays", "interleave": "one array for both covariance histories "
                                 "(FK_KF_FLAG_COV_INTERLEAVED; KalmanFilterBank.batch_filter(device_outputs=True, placement='interleave'))",
                                 "probe": "two arrays placed by measurement (filterpy_amd.placement.placed_pair; "
                                          "KalmanFilterBank.batch_filter(device_outputs=True, placement='probe'))",
                                 "auto": "the API's default at this size: two arrays placed by measurement "
                                         "(filterpy_amd.placement.placed_pair; KalmanFilterBank.batch_filter(device_outputs=True))"}[args.placement]}
    med3 = lambda *b: (one_launch_ms(*b), float(np.median([one_launch_ms(*b) for _ in range(3)])))[1]  # noqa: E731
    if args.full:                                          # (a plain run allocates the same arrays in the same order, untimed)
        placement_info["two_arrays_ms"] = round(med3(covs, covs_p), 4)
    shape, csize = tuple(covs.shape), covs.numel() * 8
    if args.placement != "none":
        del covs, covs_p
        torch.cuda.empty_cache()
        cov2, c_il, cp_il = E.alloc_cov_pair(T, N, n, layout, device)
        desc["flags"] = _abi.FK_KF_FLAG_COV_INTERLEAVED
        if args.full:
            placement_info["interleave_ms"] = round(med3(c_il, cp_il), 4)
        if args.placement == "interleave":
            covs, covs_p = c_il, cp_il
        else:
            del cov2, c_il, cp_il
            torch.cuda.empty_cache()
            desc["flags"] = 0
            from filterpy_amd import placement
            as_records = lambda b: b.view(torch.float64).view(shape)          # noqa: E731
            try:
                a_, b_, info = placement.placed_pair(csize, lambda a, b: one_launch_ms(as_records(a), as_records(b)), device,
                                                     or_none=args.placement == "auto")
            except Exception as exc:                 # (e.g. another tenant holds most of the memory): plain allocation
                torch.cuda.empty_cache()
                a_ = None if args.placement == "auto" else torch.empty(csize, dtype=torch.uint8, device=device)
                b_ = None if args.placement == "auto" else torch.empty(csize, dtype=torch.uint8, device=device)
                info = {"method": "plain allocation (probe failed)", "error": repr(exc)[:200]}
            torch.cuda.empty_cache()                 # (the probe's losers sit in torch's cache: this process has other uses for the memory)
            if a_ is None:                           # auto, like the API: the interleaved array where the probe cannot run
                cov2, covs, covs_p = E.alloc_cov_pair(T, N, n, layout, device)
                desc["flags"] = _abi.FK_KF_FLAG_COV_INTERLEAVED
                info = dict(info, fell_back_to="interleave")
            else:
                covs, covs_p = as_records(a_), as_records(b_)
            placement_info["probe"] = info
            if world > 1:                            # every rank probes its own GPU: a rank that fell back shows in the line
                try:                                 # (a float pair per rank through the same collective the timing uses)
                    mine = torch.tensor([float(info.get("chosen_ms") or -1.0), 1.0 if info.get("method") in ("probe", "cached") else 0.0],
                                        dtype=torch.float64, device=device)
                    allr = torch.empty((world, 2), dtype=torch.float64, device=device)
                    dist.all_gather_into_tensor(allr, mine)
                    placement_info["per_rank"] = [{"rank": r, "chosen_ms": round(float(allr[r, 0]), 4), "placed": bool(allr[r, 1] > 0)}
                                                  for r in range(world)]
                except Exception as exc:             # the measurement does not depend on it
                    placement_info["per_rank_error"] = repr(exc)[:200]

    def step(k=0, ev=None, with_exchange=True):
        slot = k % 2 if (ex and with_exchange) else 0
        xs = xbuf[slot]
        if ex and with_exchange:
            ex.acquire(slot)                               # the collective of step k - 2 has read this buffer
        xs.copy_(x0)
        P.copy_(P0)
        if ev:
            ev[0].record()
        E.kf_batch_filter(desc, dF, dQ, dH, dR, z, xs, P, means=means, covs=covs, means_p=means_p,
                          covs_p=covs_p, status=status)
        if ev:
            ev[1].record()
        if ex and with_exchange:
            if ragged:
                (sbuf[slot][:N] if layout == "aos" else sbuf[slot][:, :N]).copy_(xs)
            ex.post(sbuf[slot] if ragged else xs, slot, timed=ev is not None)   # exchange stream, behind this launch; returns at once

    barrier = parallel.barrier

    for k in range(args.warmup):
        step(k)
    if ex:
        ex.drain()
    barrier()
    events = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
              for _ in range(args.steps)]
    t0 = time.perf_counter()
    for k in range(args.steps):
        step(k, events[k])
    if ex:
        ex.drain()                                         # the last collective belongs to the job
    barrier()
    elapsed = time.perf_counter() - t0
    elapsed = parallel.max_over_ranks(elapsed, device)
    kernel_ms = float(np.mean([a.elapsed_time(b) for a, b in events])) if events else float("nan")

    def download(sample):
        """z and the four outputs of the tracks `sample` from the timed buffers, (T, K, ...) in NumPy order whatever the layout"""
        idx = torch.as_tensor(sample, device=device)
        if layout == "aos":
            zs_h = z[:, idx].cpu().numpy()
            got = [means[:, idx].cpu().numpy(), covs[:, idx].cpu().numpy().reshape(T, -1, n, n),
                   means_p[:, idx].cpu().numpy(), covs_p[:, idx].cpu().numpy().reshape(T, -1, n, n)]
        else:
            zs_h = z[:, :, idx].cpu().numpy().transpose(0, 2, 1)
            tr = lambda a: a[:, :, idx].cpu().numpy().transpose(0, 2, 1)                  # noqa: E731
            got = [tr(means), tr(covs).reshape(T, -1, n, n), tr(means_p), tr(covs_p).reshape(T, -1, n, n)]
        return zs_h, got

    if args.dump_outputs and rank == 0:                    # what the last timed step computed (every step computes the same)
        dsample = dump_sample(N)
        dump_outputs(args.dump_outputs, dsample, download(dsample)[1])

    if args.full:
        assert int(status.abs().max()) == 0, "kernel flagged tracks"
        # parity on the timed buffers (not timed): the first K tracks + K random tracks, all T steps, all four
        # outputs, against the oracle (K = 1024); normwise per vector / matrix, NaN fails
        K = max(1, min(args.parity_tracks, N // 2))
        rs = np.random.RandomState(99 + rank)
        sample = np.concatenate([np.arange(K), K + np.sort(rs.choice(N - K, size=K, replace=False))])
        zs_h, got = download(sample)
        ref = kf_oracle.kf_batch_filter_tracks(np.zeros((len(sample), n)), np.tile(100.0 * np.eye(n), (len(sample), 1, 1)),
                                               zs_h, F, Q, H, R, tracks=range(len(sample)))
        worst = max(parity_rel_err(g_, r_) for g_, r_ in zip(got, ref))
        assert np.isfinite(worst) and worst < 1e-10, f"parity vs oracle failed: {worst}"

        if exchange:                                       # the gathered summary state is every rank's final x, in rank order
            last = (args.steps - 1) % 2
            mine = ex.gathered[last][rank]
            if ragged:
                mine = mine[:N] if layout == "aos" else mine[:, :N]
            assert torch.equal(mine, xbuf[last]), "all-gather returned something else than this rank's final state"
    per_rank = None
    if args.full and world > 1:                            # every rank's own launch time and shard (one small collective, after the timed region)
        try:
            mine = torch.tensor([kernel_ms, float(N)], dtype=torch.float64, device=device)
            allr = torch.empty((world, 2), dtype=torch.float64, device=device)
            dist.all_gather_into_tensor(allr, mine)
            per_rank = [{"rank": r, "kernel_ms": round(float(allr[r, 0]), 4), "tracks": int(allr[r, 1])} for r in range(world)]
        except Exception as exc:                           # the measurement does not depend on it
            per_rank = {"error": repr(exc)[:200]}
    if rank == 0:
        units = float(N_total) * T * args.steps
        out = {
            "metric": "track-steps/sec (predict+update) at dim_x=4 dim_z=2",
            "value": units / elapsed, "unit": "track-steps/s", "n_gpus": world, "steps": args.steps,
            "warmup": args.warmup, "ms_per_step": 1e3 * elapsed / args.steps, "higher_is_better": True,
            "scaling": args.scaling, "vs_baseline": None, "dtype": "f64", "data": "synthetic",
            "config": {"workload": f"BASELINE configs[1]: {N} independent dim_x=4 dim_z=2 tracks x {T} steps per GPU"
                                   + (f" ({N_total} in total, sharded)" if args.scaling == "strong" else "") +
                                   ", fp64, shared F/H/Q/R, KalmanFilter.batch_filter (all 4 outputs stored)",
                       "tracks_per_gpu": N, "tracks_total": N_total, "T": T, "layout": layout,
                       "placement": {"auto": "auto = KalmanFilterBank.batch_filter(device_outputs=True) as called without further "
                                             "arguments: at this size two covariance arrays placed in HBM by measurement",
                                     "interleave": "interleave = KalmanFilterBank.batch_filter(device_outputs=True, placement='interleave') "
                                                   "(one array for both covariance histories)",
                                     "probe": "probe = KalmanFilterBank.batch_filter(device_outputs=True, placement='probe')",
                                     "none": "none = KalmanFilterBank.batch_filter(device_outputs=True, cov_interleave=False)"}[args.placement],
                       "parallelism": f"tracks sharded over {world} GPU(s)" + (", RCCL all-gather of final x per step" if world > 1 else "")},
            "placement": placement_info,
        }
        if args.dump_outputs:
            out["dumped"] = {"dir": args.dump_outputs, "tracks": int(len(dsample))}
        if args.full:
            traffic, traffic_source = pmc_traffic(layout, "interleave" if desc.get("flags") else "none")
            alg_bytes = 8.0 * (m + 2 * n + 2 * n * n) * N * T + 2 * 8.0 * (n + n * n) * N   # per launch
            achieved = alg_bytes / (kernel_ms * 1e-3) / 1e9
            out.update({
                "roofline": {"bound": "hbm", "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                             "frac": achieved / HBM_PEAK_GBS, "traffic": traffic, "traffic_source": traffic_source,
                             "kernel": "fk::kf_fast_kernel<4,2," + layout + ",nomask,outs" + (",IL" if desc.get("flags") else "") + "> (variant " + os.environ.get("FK_FAST_VARIANT", "0") + ")", "kernel_ms": kernel_ms,
                             "algorithmic_bytes_per_launch": alg_bytes},
                # the same launch on two plain torch allocations (no placement): what the 55-pair probe of `placement` buys on this box
                "value_unplaced": float(N) * T / (placement_info["two_arrays_ms"] * 1e-3) * world,
                "parity_max_rel_vs_oracle": worst, "parity_tracks": int(len(sample)),
                "gpu_clocks": gpu_clocks(), "hbm_probes": hbm_probes(device), "under_load": clocks_under_load(lambda: step(0, None, False)),   # rank 0 alone: no collective in the burst
            })
        if per_rank is not None:
            out["per_rank"] = per_rank
        if exchange:
            out["allgather_ms"] = ex.gather_ms()
            out["exchange"] = ("all-gather of final x (%d MB per rank) on a side stream, overlapped with the next launch; "
                               "double-buffered x / gathered" % (x.numel() * 8 // 1000000))
        if args.force_dist:
            out["dist_forced"] = f"{world}-rank {dist.get_backend()} group: init_process_group(device_id), all_gather_into_tensor, barrier, all_reduce(MAX) executed"
        if args.full and world == 1 and args.placement in ("interleave", "none") and not os.environ.get("FK_BENCH_SKIP_PROBE"):
            # the third arrangement (two arrays placed by measurement), timed AFTER the measurement, for the record only
            try:
                del covs, covs_p, got
                if args.placement == "interleave":
                    del cov2, c_il, cp_il
                torch.cuda.empty_cache()
                desc["flags"] = 0
                from filterpy_amd import placement
                as_records = lambda b: b.view(torch.float64).view(shape)          # noqa: E731
                a_, b_, info = placement.placed_pair(csize, lambda a, b: one_launch_ms(as_records(a), as_records(b)), device)
                out["placement"]["probe_ms"] = round(float(np.median([one_launch_ms(as_records(a_), as_records(b_)) for _ in range(3)])), 4)
                out["placement"]["probe"] = {k: info.get(k) for k in ("method", "buffers_tried", "pairs", "chosen_ms", "median_ms", "worst_ms", "error") if k in info}
                del a_, b_
                torch.cuda.empty_cache()
            except Exception as exc:
                out["placement"]["probe_error"] = repr(exc)[:200]
        if args.full and world == 1 and not args.no_cpu:
            # the CPU baseline filters the same measurements: the first 64 x 256 tracks of the timed z buffer
            kc = min(N, CPU_TRACKS_PER_PROC * 256)
            zc = (z[:, :kc] if layout == "aos" else z[:, :, :kc].transpose(1, 2)).cpu().numpy()
            out["cpu_baseline"] = cpu_baseline(np.ascontiguousarray(zc), args.cpu_seconds, args.cpu_procs or None)
        if args.full and world == 1 and not args.no_configs:
            out["configs"] = baseline_configs(args.config_reps)
        print(json.dumps(out), flush=True)
    parallel.shutdown()


if __name__ == "__main__":
    main()
