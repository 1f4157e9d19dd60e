"""-m gpu: the Kalman filter's forward kernels on ill-conditioned models against tests/kf_hp.py, the reference's algorithm in
longdouble.

Every other GPU test of the forward pass compares with a float64 result at 1e-10 on benign models (P0 ~ 3 I, R ~ 0.5 I, condition
~10), where every legitimate float64 ordering sits near 1e-15: a kernel that loses four or five digits more than the reference
still passes.  The kernel families differ in their ARITHMETIC, not only in their data movement -- one lane per track with full or
packed-symmetric matrices (kf_fast.hip), three lanes (kf_ml.hip), four lanes (kf_mlg.hip), the exact / padded / rolled general
instantiations (kf_kernels.hip), and the EX instantiations that also store K, S, SI and y -- so each is run here, reached through
the switches kf_dispatch.cpp reads per call.

The bar (kf_hp.check): the float64 oracle (oracle/kf_oracle.py) is measured against the longdouble truth, on the given inputs and
on K_DRAWS = 8 copies of them perturbed by one ulp; the worst of those is a track's reference error `ref`; then per family, dims
and output

    every checked track   err(gpu, hp) <= max(8 max_tracks ref, 1e-13)
    the median over them  median err(gpu, hp) <= max(8 median ref, 1e-13)

with the MARGIN = 8 and the 1e-13 floor of tests/test_gpu_ukf_precision.py: no number is tuned to a kernel.  Errors are normwise
per step, the worst step counted, measured in longdouble (ukf_hp.err).

Models (ukf_hp.models: a fixed RandomState per (dim_x, dim_z); every track its own x0 and measurements; T = 16, the measurement of
step 8 missing and NaN in its place; a bank of 150 tracks, which ends inside a wave; 16 tracks checked: 0 1 15 16 63 64 143 144
149 and seven from the seed): benign (the control), stiff (P0 = 1e6 I, R = 1e-4 I, Q = diag(10^U(-6,-2))) and stiff_small_weights
(P0 = 1e4 I, R = 1e-2 I).  No track is left out: every test first asserts that the oracle finishes all 16 tracks with
err(oracle, hp) < 1e-3 on every output (kf_hp.measures_something; worst 1.2e-4, the means of the stiff model at (12,3); 2.2e-4
without the missing step).

The lane mix: the posterior means returned for checked track i are further than 1e-3 from the truth of track i + 1
(kf_hp.not_the_neighbour) -- tracks swapped between lanes would otherwise all sit inside a loose bar.

docs/MEASUREMENTS.md ("KF precision") has the figures of the GPU run and of the host builds (tests/test_host_kf_hp.py)."""
import numpy as np
import pytest

import kf_hp

pytestmark = pytest.mark.gpu

# (organisation, dim_x, dim_z, switches, per-track models)
CASES = [
    ("kf_fast full", 2, 1, {}, False),
    ("kf_fast full", 4, 2, {}, False),
    ("kf_fast packed", 6, 3, {}, False),
    ("kf_fast packed", 8, 4, {}, False),
    ("kf_fast packed", 9, 3, {"FK_NO_ML": "1"}, False),
    ("kf_fast packed", 9, 4, {"FK_ML9": "m"}, False),
    ("kf_fast variant 1 full", 6, 3, {"FK_FAST_VARIANT": "1"}, False),
    ("kf_ml three lanes", 9, 3, {}, False),
    ("kf_mlg four lanes", 9, 4, {}, False),
    ("kf_mlg four lanes", 12, 3, {}, False),
    ("kf_mlg four lanes", 16, 8, {}, False),
    ("kf_mlg four lanes", 9, 3, {"FK_ML9": "g"}, False),
    ("kf_kernels exact", 6, 3, {"FK_NO_FAST": "1"}, False),
    ("kf_kernels padded (6,6)", 5, 4, {"FK_NO_FAST": "1"}, False),
    ("kf_kernels rolled (16,8)", 12, 3, {"FK_NO_FAST": "1"}, False),
    ("kf_kernels exact per-track models", 8, 4, {}, True),
]
IDS = ["%s-%d-%d" % (c[0].replace(" ", "_"), c[1], c[2]) for c in CASES]


def _bank_inputs(M, masked):
    T, N = M["T"], M["N"]
    mask = np.repeat(M["mask"][:, None], N, axis=1) if masked else None
    zz = M["zs"] if mask is None else np.where(mask[..., None] != 0, M["zs"], np.nan)     # a masked measurement is never used
    return mask, zz


def _checked(a, M):
    """[T][N]... -> [16 checked tracks][T]..."""
    return np.swapaxes(a[:, list(M["tracks"])], 0, 1)


@pytest.mark.parametrize("layout", ["soa", "aos"])
@pytest.mark.parametrize("family", kf_hp.FAMILIES)
@pytest.mark.parametrize("org,n,m,env,per_track", CASES, ids=IDS)
def test_forward_pass_vs_extended_precision(org, n, m, env, per_track, family, layout, monkeypatch):
    from gpu_util import run_kf_batch, tile_tracks
    from filterpy_amd._abi import FK_MODEL_PER_TRACK, FK_MODEL_SHARED
    t = kf_hp.truth(family, n, m)                                         # computed once per (family, n, m), shared, unchanged
    kf_hp.measures_something(t)
    M = t["model"]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    mask, zz = _bank_inputs(M, True)
    mods = [M[k] for k in ("F", "Q", "H", "R")]
    if per_track:
        mods = [tile_tracks(a, M["N"]) for a in mods]
    res = run_kf_batch(M["x0"], M["P0"], zz, *mods, layout=layout, mode=FK_MODEL_PER_TRACK if per_track else FK_MODEL_SHARED,
                       mask=mask, check_status=False)
    out, status = res[:4], res[6]
    assert not status.any(), status[status != 0]                          # zero on EVERY track of the bank
    assert all(np.all(np.isfinite(a)) for a in out) and np.all(np.isfinite(res[4])) and np.all(np.isfinite(res[5]))
    eg = np.full((len(kf_hp.OUTPUTS), 16), np.nan)
    eg[kf_hp.FORWARD] = kf_hp.errors([_checked(a, M) for a in out], t["hp"][kf_hp.FORWARD])
    for name, eb, bo, ro in kf_hp.ratios(eg, t):
        print("%-34s (%d,%d) %-20s %s %-8s err/bar %.3f  gpu/oracle %6.2f  ref/oracle %6.2f" % (org, n, m, family, layout, name, eb, bo, ro))
    bad = kf_hp.check(f"{org} ({n},{m}) {family} {layout}", eg, t)          # asserts that no track and no output is missing
    assert not bad, (bad, eg.max(axis=1), t["ref"].max(axis=1))
    assert kf_hp.not_the_neighbour(_checked(out[0], M), t)


def _run_ex(M, zz, mask, layout):
    """fk_kf_batch_filter_ex_f64 with the K, S, SI and y histories, called the way tests/test_gpu_kf.py's
    test_saver_histories_from_* call it -> ({history: [T][N]...}, status)"""
    import torch
    from filterpy_amd import _engine as E
    n, m, N, T = M["n"], M["m"], M["N"], M["T"]
    dx, dP, dz = E.to_records(M["x0"], layout, 0), E.to_records(M["P0"], layout, 0), E.to_records(zz, layout, 1)
    dmask = None if mask is None else torch.as_tensor(np.ascontiguousarray(mask, dtype=np.uint8), device=dx.device)
    outs = [E.alloc_records((T,), N, w, layout).fill_(float("nan")) for w in (n, n * n, n, n * n)]
    shapes = dict(K=(n, m), S=(m, m), SI=(m, m), y=(m,))
    ex = {k: E.alloc_records((T,), N, int(np.prod(s)), layout).fill_(float("nan")) for k, s in shapes.items()}
    st = torch.full((N,), -1, dtype=torch.int32, device=dx.device)
    E.kf_batch_filter_ex(dict(n=n, m=m, nu=0, model_mode=0, N=N, T=T, layout=E.LAYOUTS[layout], update_first=0, alpha_sq=1.0),
                         E.dev(M["F"]), E.dev(M["Q"]), E.dev(M["H"]), E.dev(M["R"]), dz, dx, dP, ex, mask=dmask,
                         means=outs[0], covs=outs[1], means_p=outs[2], covs_p=outs[3], status=st)
    torch.cuda.synchronize()
    hist = {k: E.from_records(ex[k], layout, 1, shapes[k]) for k in shapes}
    return [E.from_records(o, layout, 1, s) for o, s in zip(outs, ((n,), (n, n), (n,), (n, n)))], hist, st.cpu().numpy()


@pytest.mark.parametrize("layout", ["soa", "aos"])
@pytest.mark.parametrize("n,m,masked", [(4, 2, True), (9, 3, False), (12, 3, False)],
                         ids=["kf_fast_EX-4-2", "kf_mlg_EX-9-3", "kf_mlg_EX-12-3"])
def test_histories_vs_extended_precision(n, m, masked, layout):
    """the EX instantiations on the stiff family: K, S, SI and y per step -- and the four regular outputs of the same call --
    against the longdouble K, S, SI, y, the same bar with `ref` from the oracle's Ks / Ss / SIs / ys.  (4,2): kf_fast's EX
    instantiation, with the mask (y = 0 and K, S, SI kept at the missing step); (9,3) and (12,3): kf_mlg's, which takes no mask."""
    t = kf_hp.truth("stiff", n, m, masked)
    kf_hp.measures_something(t)
    M = t["model"]
    mask, zz = _bank_inputs(M, masked)
    out, hist, status = _run_ex(M, zz, mask, layout)
    assert not status.any(), status[status != 0]
    got = out + [hist[k] for k in ("K", "S", "SI", "y")]
    assert all(np.all(np.isfinite(a)) for a in got)
    eg = kf_hp.errors([_checked(a, M) for a in got], t["hp"])
    for name, eb, bo, ro in kf_hp.ratios(eg, t, slice(None)):
        print("EX (%d,%d) stiff %s %-8s err/bar %.3f  gpu/oracle %6.2f  ref/oracle %6.2f" % (n, m, layout, name, eb, bo, ro))
    bad = kf_hp.check(f"EX ({n},{m}) stiff {layout}", eg, t, slice(None))
    assert not bad, (bad, eg.max(axis=1), t["ref"].max(axis=1))
    assert kf_hp.not_the_neighbour(_checked(out[0], M), t)
