"""-m gpu: the Kalman filter's RTS smoother kernels on ill-conditioned models against tests/rts_hp.py, the reference's smoother in
longdouble.

The other GPU tests of the smoother compare with a float64 result: at 1e-10 on benign models (condition ~10), or -- the one
test on hard models, test_smoother_margin_on_badly_conditioned_models -- at max(1e-10, 2 x the reference's spread) on 70
IDENTICAL copies of one track and on the default route of each dim only.  The smoother has the most arithmetic variants behind one
entry point (fk_kf_rts_f64, routed by route_rts in csrc/kf_dispatch.cpp), and P[k] += K (P[k+1] - Pp[k]) K' with
K = P F' inv(Pp) is where an LDL' solve, a packed-symmetric update and a cross-lane exchange can each lose digits separately.  So
every organisation is run here, reached through the switches route_rts reads per call (read there, not assumed):

    one lane per track, exact dims (rts_kernels.hip, rts_step_sym)   the default up to dim_x 8 (element-major) / 7 (NumPy order);
                                                                     dim_x 8 NumPy order with FK_ML9=m; dim_x 9 with FK_NO_ML=1
                                                                     and FK_ML9=m; EVERY per-step or per-track model of dim_x <= 9
    one lane, rolled / padded (16, 0) (rts_kernels.hip, rts_step)    dim_x 10..16 with FK_NO_MLG=1; EVERY per-step or per-track
                                                                     model of dim_x >= 10
    three lanes (rts_ml_9, kf_ml.hip)                                dim_x 9 element-major; NumPy order with FK_ML9=m
    four lanes (rts_mlg.hip)                                         dim_x 10..13 and 14 element-major; 8, 9 NumPy order; 9
                                                                     element-major with FK_ML9=g; the rest with FK_RTS_LANES=4
    eight lanes, LDS exchange (rts_mlx.hip)                          dim_x 15, 16 and 14 NumPy order; 13, 14 with FK_RTS_LANES=8
    caller-supplied inverse (kf_given_inv.hip)                       FK_KF_FLAG_PP_ONLY / FK_KF_FLAG_PPINV_GIVEN

Two things route_rts and the launchers say that a reader might not expect.  The several-lane launchers all decline a call with
per-step models (`a.model_t`: NOT_SERVED), so the per-step cases at (9,3) and (12,3) run the ONE-lane kernels -- the exact-9 and
the rolled instantiation with the model reloaded every step -- whatever their dim suggests.  And at 150 tracks and 12 steps
FK_RTS_PERSIST=1 does not start the persistent grid (launch_rts_ml_persistent wants more workgroups than the chip holds and time
chunks of 16 steps): that case runs the three-lane kernel's ordinary launch with the switch set, and the PERS instantiation is tied
to it bit for bit by test_three_lane_smoother_persistent_grid_is_bit_identical (tests/test_gpu_kf.py) on 33 003 tracks.

The inputs (rts_hp.truth): the float64 oracle's forward pass on ukf_hp.models -- 150 tracks with their own x0 and measurements,
16 steps, the measurement of step 8 missing -- from step 4 on (a window of 12), every covariance symmetrised; truth, oracle and
kernel get the same arrays.  Families: benign (the control), stiff (P0 = 1e6 I, R = 1e-4 I, Q = diag(10^U(-6,-2))) and
stiff_small_weights (P0 = 1e4 I, R = 1e-2 I).

Every case asserts
    1. status zero on every track and all four outputs finite (the buffers are NaN beforehand: an unwritten element shows);
    2. the bar (rts_hp.check), on the 16 checked tracks and all four outputs: with `ref` the worst error against the truth of the
       float64 oracle on the given inputs and on K_DRAWS = 8 copies perturbed by one ulp,
           every checked track   err(gpu, hp) <= max(8 max_tracks ref, 1e-13)
           the median over them  median err(gpu, hp) <= max(8 median ref, 1e-13)
       -- kf_hp's MARGIN and ukf_hp's FLOOR: no number is tuned to a kernel;
    3. the lane check on ALL 150 tracks: xs of track i within 1e-3 of its own truth and further than 1e-3 from the truth of track
       i + 1.  The checked set ends on multiples of 16 and 64; the three-lane kernel packs 21 tracks per wave and the eight-lane
       one 8, so their seams are covered only by looking at every track.
tests/test_host_rts_hp.py asserts on the CPU, for every key used here, that the oracle is within 1e-3 of the truth on all
outputs and that every track is further than 1e-3 from its neighbour.

docs/MEASUREMENTS.md ("RTS smoother precision") has the figures of the GPU run and of the host builds."""
import numpy as np
import pytest

import rts_hp

pytestmark = pytest.mark.gpu

SWITCHES = ("FK_NO_ML", "FK_NO_MLG", "FK_ML9", "FK_RTS_LANES", "FK_RTS_PERSIST", "FK_RTS_PERSIST_H")
BOTH = ("soa", "aos")
# (organisation, dim_x, dim_z of the model, switches, layouts)
CASES = [
    ("one lane exact", 2, 1, {}, BOTH),
    ("one lane exact", 4, 2, {}, BOTH),
    ("one lane exact", 6, 3, {}, BOTH),
    ("one lane exact", 8, 4, {}, ("soa",)),
    ("one lane exact", 8, 4, {"FK_ML9": "m"}, ("aos",)),
    ("one lane exact 9", 9, 3, {"FK_NO_ML": "1", "FK_ML9": "m"}, BOTH),
    ("one lane rolled (16,0)", 12, 3, {"FK_NO_MLG": "1"}, BOTH),
    ("one lane rolled (16,0)", 16, 8, {"FK_NO_MLG": "1"}, BOTH),
    ("three lanes", 9, 3, {}, ("soa",)),
    ("three lanes", 9, 3, {"FK_ML9": "m"}, ("aos",)),
    ("three lanes FK_RTS_PERSIST=1", 9, 3, {"FK_RTS_PERSIST": "1"}, ("soa",)),
    ("four lanes", 8, 4, {}, ("aos",)),
    ("four lanes", 9, 3, {}, ("aos",)),
    ("four lanes", 9, 3, {"FK_ML9": "g"}, ("soa",)),
    ("four lanes", 12, 3, {}, BOTH),
    ("four lanes", 14, 4, {}, ("soa",)),
    ("four lanes", 16, 8, {"FK_RTS_LANES": "4"}, BOTH),
    ("eight lanes", 14, 4, {}, ("aos",)),
    ("eight lanes", 13, 4, {"FK_RTS_LANES": "8"}, ("soa",)),
    ("eight lanes", 14, 4, {"FK_RTS_LANES": "8"}, ("soa",)),
    ("eight lanes", 16, 8, {}, BOTH),
]
SHARED = [(org, n, m, env, lay) for org, n, m, env, lays in CASES for lay in lays]
SHARED_IDS = ["%s-%d-%d-%s" % (c[0].replace(" ", "_"), c[1], c[2], c[4]) for c in SHARED]
# per-step models: the several-lane launchers decline them, so (9,3) and (12,3) run the one-lane kernels (see above)
PER_STEP = [("one lane exact, per-step models", 4, 2), ("one lane exact 9, per-step models", 9, 3),
            ("one lane rolled (16,0), per-step models", 12, 3)]


def _smooth(t, layout, per_track=False, flags=0, K_in=None):
    """fk_kf_rts_f64 on the whole bank of the truth `t`, called the way gpu_util.run_rts calls it, the four output buffers NaN
    beforehand (K_in: the caller's inverses in the K buffer) -> ([xs, Ps, K, Pp] as [N][T]..., status [N])"""
    import torch
    from filterpy_amd import _engine as E
    from filterpy_amd._abi import FK_MODEL_PER_STEP, FK_MODEL_PER_TRACK, FK_MODEL_SHARED
    from gpu_util import model_to_dev, tile_tracks
    Xs, Ps, F, Q = t["Xs"], t["Ps"], t["F"], t["Q"]
    T, N, n = Xs.shape
    mode = FK_MODEL_PER_STEP if F.ndim == 3 else FK_MODEL_PER_TRACK if per_track else FK_MODEL_SHARED
    if per_track:
        F, Q = tile_tracks(F, N), tile_tracks(Q, N)
    dX, dPs = E.to_records(Xs, layout, 1), E.to_records(Ps, layout, 1)
    dF, dQ = model_to_dev(F, mode, layout), model_to_dev(Q, mode, layout)
    o = [E.alloc_records((T,), N, n, layout)] + [E.alloc_records((T,), N, n * n, layout) for _ in range(3)]
    for b in o:
        b.fill_(float("nan"))
    if K_in is not None:
        o[2] = E.to_records(K_in, layout, 1)
    st = torch.zeros(N, dtype=torch.int32, device=dX.device)
    E.kf_rts(dict(n=n, m=1, nu=0, model_mode=mode, N=N, T=T, layout=E.LAYOUTS[layout], update_first=0, alpha_sq=1.0, flags=flags),
             dF, dQ, dX, dPs, o[0], o[1], o[2], o[3], convention=1 - t["off"], status=st)
    torch.cuda.synchronize()
    out = [E.from_records(o[0], layout, 1, (n,))] + [E.from_records(b, layout, 1, (n, n)) for b in o[1:]]
    return [np.swapaxes(a, 0, 1) for a in out], st.cpu().numpy()


def _hold(label, out, status, t, which=slice(None)):
    """the three assertions of a case on the outputs `which`"""
    assert not status.any(), status[status != 0]                          # zero on EVERY track of the bank
    assert all(np.all(np.isfinite(a)) for a in out[which]), [int(np.isnan(a).sum()) for a in out]
    tracks = list(t["model"]["tracks"])
    eg = np.full((len(rts_hp.OUTPUTS), 16), np.nan)
    eg[which] = rts_hp.errors([a[tracks] for a in out], t["hp"])[which]   # (an output the call does not write stays NaN)
    for name, eb, bo, ro in rts_hp.ratios(eg, t, which):
        print("%-44s %-3s err/bar %.3f  gpu/oracle %6.2f  ref/oracle %6.2f" % (label, name, eb, bo, ro))
    bad = rts_hp.check(label, eg, t, which)                                # asserts that no track and no output is missing
    assert not bad, (bad, eg.max(axis=1), t["ref"].max(axis=1))


def _lanes(out, t):
    own, other = rts_hp.lanes(out[0], t)
    assert own < 1e-3 < other, (own, other)


@pytest.fixture
def env(monkeypatch):
    """no routing switch of the smoother set, whatever the caller's shell holds; a case sets its own"""
    for v in SWITCHES:
        monkeypatch.delenv(v, raising=False)
    return monkeypatch


@pytest.mark.parametrize("family", rts_hp.FAMILIES)
@pytest.mark.parametrize("org,n,m,switches,layout", SHARED, ids=SHARED_IDS)
def test_smoother_vs_extended_precision(org, n, m, switches, layout, family, env):
    t = rts_hp.truth(family, n, m)                                        # computed once per key, shared, unchanged
    rts_hp.measures_something(t)
    for k, v in switches.items():
        env.setenv(k, v)
    out, status = _smooth(t, layout)
    _hold(f"{org} ({n},{m}) {family} {layout}", out, status, t)
    _lanes(out, t)


@pytest.mark.parametrize("layout", BOTH)
@pytest.mark.parametrize("family", rts_hp.FAMILIES)
def test_per_track_models_vs_extended_precision(family, layout, env):
    """FK_MODEL_PER_TRACK at (6,3): F and Q tiled, every lane's model in its registers (the UNIFORM = false instantiation)"""
    t = rts_hp.truth(family, 6, 3)
    rts_hp.measures_something(t)
    out, status = _smooth(t, layout, per_track=True)
    _hold(f"one lane exact, per-track models (6,3) {family} {layout}", out, status, t)
    _lanes(out, t)


@pytest.mark.parametrize("layout", BOTH)
@pytest.mark.parametrize("convention", [0, 1])
@pytest.mark.parametrize("family", rts_hp.FAMILIES)
@pytest.mark.parametrize("org,n,m", PER_STEP, ids=["%d-%d" % c[1:] for c in PER_STEP])
def test_per_step_models_vs_extended_precision(org, n, m, family, convention, layout, env):
    """FK_MODEL_PER_STEP, Fs[t] = F + 0.02 (t / T) subdiag(1) and Qs[t] = Q (1 + t / T): index_convention 0 takes Fs[k+1] (the
    class), 1 takes Fs[k] (the module function); the two truths are further apart than 1e-3 (tests/test_host_rts_hp.py), so the
    lane check's `own < 1e-3` also says that the kernel took the right one"""
    t = rts_hp.truth(family, n, m, "class" if convention == 0 else "module")
    rts_hp.measures_something(t)
    assert t["off"] == 1 - convention and t["F"].shape == (12, n, n)
    out, status = _smooth(t, layout)
    _hold(f"{org} conv {convention} ({n},{m}) {family} {layout}", out, status, t)
    _lanes(out, t)


@pytest.mark.parametrize("layout", BOTH)
@pytest.mark.parametrize("n,m", [(6, 3), (12, 3)])
def test_given_inverse_vs_extended_precision(n, m, layout, env):
    """the caller-supplied-inverse kernel on the stiff family, flagged as KalmanFilter.rts_smoother(inv=) flags it
    (tests/test_gpu_kf_inv.py).  FK_KF_FLAG_PP_ONLY: the Pp it returns is held to the Pp bar.  FK_KF_FLAG_PPINV_GIVEN: the
    inverses are the float64 rounding of the longdouble inv(Pp); the truth is the longdouble recursion with those very inverses
    and the reference error that of kf_oracle.rts_smoother(inv=) handing them back; xs, Ps, K (and the Pp it stores again) are
    held to the bar."""
    from filterpy_amd._abi import FK_KF_FLAG_PP_ONLY, FK_KF_FLAG_PPINV_GIVEN
    t = rts_hp.truth("stiff", n, m, "given")
    rts_hp.measures_something(t)
    out, status = _smooth(t, layout, flags=FK_KF_FLAG_PP_ONLY)
    _hold(f"given inverse PP_ONLY ({n},{m}) stiff {layout}", out, status, t, slice(3, 4))
    out, status = _smooth(t, layout, flags=FK_KF_FLAG_PPINV_GIVEN, K_in=t["invs"])
    _hold(f"given inverse PPINV_GIVEN ({n},{m}) stiff {layout}", out, status, t)
    _lanes(out, t)
