"""-m gpu: the options and variants of the linear Kalman filter on ill-conditioned models against tests/kf_opts_hp.py, the
reference's algorithm in longdouble -- the other half of tests/test_gpu_kf_precision.py, which holds the plain forward call.

Everything the linear filter does besides the plain call runs in instantiations of its own, with their own arithmetic and data
movement: kf_fast.hip's UF and CTRL instantiations, its model modes and alpha_sq; the VAR and VAR + UF families of kf_ml.hip and
kf_mlg.hip (per-step models prefetched one step ahead, B behind the model, run-time switches for the mask and nu); the general
kernel kf_kernels.hip with what the specialised ones do not serve, and the single-step fk_kf_predict_f64 / fk_kf_update_f64 behind
KalmanFilter.predict() / .update(); the three implementations of the log-likelihood and Mahalanobis histories; kf_variants.hip's
update_correlated (non-Joseph) and steady-state kernels; kf_given_inv.hip's update side.  Each is reached through the switches
kf_dispatch.cpp reads per call, and where the general kernel is meant the result is compared bit for bit with the FK_NO_FAST=1 run.

The bar is kf_hp's, unchanged (kf_opts_hp.check): with `ref` the worst error of the float64 oracle against the longdouble truth on
the given inputs and on K_DRAWS = 8 copies perturbed by one ulp,

    every checked track   err(gpu, hp) <= max(8 max_tracks ref, 1e-13)
    the median over them  median err(gpu, hp) <= max(8 median ref, 1e-13)

Every test first asserts that its model measures something (all 16 tracks finish in the oracle, err(oracle, hp) < 1e-3), checks
status zero on every track and finite outputs, and that no track got its neighbour's result.  tests/test_host_kf_options_hp.py
asserts the condition on the CPU for every key used here and shows that the characteristic mistakes sit above the bar.

docs/MEASUREMENTS.md ("KF options and variants precision") has the figures of the GPU run."""
import os
import subprocess
import sys

import numpy as np
import pytest

import kf_hp
import kf_opts_hp as oh
from kf_opts_hp import ALPHA_SQ, Opt

pytestmark = pytest.mark.gpu

SHARED, PER_TRACK, PER_TRACK_STEP, PER_STEP = "shared", "per_track", "per_track_step", "per_step"
NO_FAST = {"FK_NO_FAST": "1"}


def _all(nu):
    return Opt(nu=nu, per_step=True, alpha_sq=ALPHA_SQ, update_first=True)


# (organisation, dim_x, dim_z, switches, model mode, option set, the general kernel is meant)
FORWARD_CASES = [
    ("kf_fast UF", 4, 2, {}, SHARED, Opt(update_first=True), False),
    ("kf_fast UF", 6, 3, {}, SHARED, Opt(update_first=True), False),
    ("kf_fast CTRL nu 2", 4, 2, {}, SHARED, Opt(nu=2), False),
    ("kf_fast CTRL nu 4", 6, 3, {}, SHARED, Opt(nu=4), False),
    ("kf_fast CTRL nu 3", 6, 3, {}, SHARED, Opt(nu=3), False),
    ("kf_fast per-step", 6, 3, {}, PER_STEP, Opt(per_step=True), False),
    ("kf_fast per-track-step", 4, 2, {}, PER_TRACK_STEP, Opt(per_step=True), False),
    ("kf_fast per-track", 6, 3, {}, PER_TRACK, Opt(), False),
    ("kf_fast full alpha", 2, 1, {}, SHARED, Opt(alpha_sq=ALPHA_SQ), False),
    ("kf_fast packed alpha", 6, 3, {}, SHARED, Opt(alpha_sq=ALPHA_SQ), False),
    ("kf_fast one wave alpha", 8, 4, {}, SHARED, Opt(alpha_sq=ALPHA_SQ), False),
    ("kf_ml VAR nu 2", 9, 3, {}, SHARED, Opt(nu=2), False),
    ("kf_ml VAR per-step", 9, 3, {}, PER_STEP, Opt(per_step=True), False),
    ("kf_ml VAR per-step nu 2 mask", 9, 3, {}, PER_STEP, Opt(nu=2, per_step=True), False),
    ("kf_ml VAR+UF", 9, 3, {}, SHARED, Opt(update_first=True), False),
    ("kf_ml VAR+UF everything", 9, 3, {}, PER_STEP, _all(2), False),
    ("kf_ml plain alpha", 9, 3, {}, SHARED, Opt(alpha_sq=ALPHA_SQ), False),
    ("kf_mlg plain alpha", 12, 3, {}, SHARED, Opt(alpha_sq=ALPHA_SQ), False),
    ("general exact nu 2", 8, 4, {}, SHARED, Opt(nu=2), True),
    ("general exact UF", 8, 4, {}, SHARED, Opt(update_first=True), True),
    ("general exact per-track-step", 8, 4, {}, PER_TRACK_STEP, Opt(per_step=True), True),
    ("general rolled nu 5", 12, 3, {}, SHARED, Opt(nu=5), True),
    ("general rolled FK_ML_VAR=0 everything", 12, 3, {"FK_ML_VAR": "0"}, PER_STEP, _all(4), True),
    ("general padded alpha nu 2 UF", 5, 4, NO_FAST, SHARED, Opt(nu=2, alpha_sq=ALPHA_SQ, update_first=True), True),
]
for _n, _m in ((9, 4), (12, 3), (16, 8)):
    FORWARD_CASES += [("kf_mlg VAR nu 4", _n, _m, {}, SHARED, Opt(nu=4), False),
                      ("kf_mlg VAR per-step", _n, _m, {}, PER_STEP, Opt(per_step=True), False),
                      ("kf_mlg VAR+UF everything", _n, _m, {}, PER_STEP, _all(4), False)]
FORWARD_IDS = ["%s-%d-%d" % (c[0].replace(" ", "_"), c[1], c[2]) for c in FORWARD_CASES]

# (organisation, dim_x, dim_z, masked): the histories with log_likelihood and mahalanobis, on stiff
HISTORY_CASES = [("kf_fast extras", 4, 2, True), ("kf_mlg EX", 12, 3, False), ("general, missing step", 12, 3, True)]
CLASS_DIMS = [(4, 2), (9, 3), (12, 3)]
# update_correlated: the recursion where the truth itself stays positive definite, single updates on the stiff priors above that
CORR_RECURSION = [(f, n, m) for f in ("benign", "stiff_small_weights") for n, m in ((4, 2), (6, 3), (9, 4), (12, 8), (16, 8), (10, 5))] + \
                 [("stiff", 4, 2), ("stiff", 6, 3)]
CORR_SINGLE = [("stiff", n, m) for n, m in ((9, 4), (12, 8), (16, 8), (10, 5))]
# (what, dim_x, dim_z, per-track K, nu)
STEADY_CASES = [("exact", 2, 1, False, 0), ("exact", 6, 3, True, 2), ("exact", 9, 3, False, 4), ("guarded", 5, 2, False, 2),
                ("guarded", 5, 2, True, 0), ("KREG=false", 12, 8, False, 0), ("KREG", 12, 8, True, 2), ("KREG=false", 16, 8, False, 2),
                ("KREG", 16, 8, True, 0), ("padded", 14, 6, False, 2), ("padded", 14, 6, True, 0)]
STEADY_ROLLED = ("rolled", 12, 8, False, 2)
GIVEN_INV_DIMS = [(6, 3), (12, 3)]


def _checked(a, M, lead=1):
    """[T][N]... -> [16 checked tracks][T]... (lead = 0: [N]... -> [16]...)"""
    return np.swapaxes(a[:, list(M["tracks"])], 0, 1) if lead else a[list(M["tracks"])]


def _bank_zs(M):
    """(mask [T][N] or None, zs with NaN at a missing measurement: never used)"""
    if M["mask"].all():
        return None, M["zs"]
    mask = np.repeat(M["mask"][:, None], M["N"], axis=1)
    return mask, np.where(mask[..., None] != 0, M["zs"], np.nan)


def _report(label, eg, t, names, means):
    for name, eb, bo, ro in oh.ratios(eg, t, names):
        print("%-58s %-8s err/bar %.3f  gpu/oracle %6.2f  ref/oracle %6.2f" % (label, name, eb, bo, ro))
    bad = oh.check(label, eg, t, names)
    assert not bad, (bad, eg.max(axis=1), t["ref"].max(axis=1))
    assert oh.not_the_neighbour(means, t)


def _forward(M, bm, mode, o, layout):
    from gpu_util import run_kf_batch, tile_tracks
    from filterpy_amd import _abi
    N = M["N"]
    code = {SHARED: _abi.FK_MODEL_SHARED, PER_TRACK: _abi.FK_MODEL_PER_TRACK, PER_TRACK_STEP: _abi.FK_MODEL_PER_TRACK_STEP,
            PER_STEP: _abi.FK_MODEL_PER_STEP}[mode]
    spread = (lambda a: a) if mode in (SHARED, PER_STEP) else (lambda a: None if a is None else
                                                               tile_tracks(a, N, 0 if mode == PER_TRACK else 1))
    mask, zz = _bank_zs(M)
    return run_kf_batch(M["x0"], M["P0"], zz, *(spread(bm[k]) for k in ("F", "Q", "H", "R")), layout=layout, mode=code, mask=mask,
                        B=spread(bm["B"]), us=bm["us"], alpha_sq=o.alpha_sq, update_first=o.update_first, check_status=False)


@pytest.mark.parametrize("layout", ["soa", "aos"])
@pytest.mark.parametrize("family", kf_hp.FAMILIES)
@pytest.mark.parametrize("org,n,m,env,mode,o,general", FORWARD_CASES, ids=FORWARD_IDS)
def test_forward_options_vs_extended_precision(org, n, m, env, mode, o, general, family, layout, monkeypatch):
    t = oh.truth_opts(family, n, m, o)                                     # once per (family, n, m, option set), shared
    oh.measures_something(t, oh.FORWARD)
    M, bm = t["model"], t["inputs"]
    with monkeypatch.context() as mp:
        for k, v in env.items():
            mp.setenv(k, v)
        res = _forward(M, bm, mode, o, layout)
    out, status = res[:4], res[6]
    assert not status.any(), status[status != 0]                           # zero on EVERY track of the bank
    assert all(np.all(np.isfinite(a)) for a in res[:6])
    if general:                                                            # the route: the general kernel's own bits
        with monkeypatch.context() as mp:
            mp.setenv("FK_NO_FAST", "1")
            ref = _forward(M, bm, mode, o, layout)
        assert all(np.array_equal(a, b) for a, b in zip(res[:6], ref[:6])), org
    eg = np.full((len(oh.OUTPUTS), 16), np.nan)
    eg[:4] = oh.errors([_checked(a, M) for a in out], t["hp"][:4], oh.FORWARD)
    _report(f"{org} ({n},{m}) {family} {layout}", eg, t, oh.FORWARD, _checked(out[0], M))


def _run_ex(M, zz, mask, layout):
    """fk_kf_batch_filter_ex_f64 with all six histories -> the ten arrays of kf_opts_hp.OUTPUTS [T][N]..., status"""
    import torch
    from filterpy_amd import _engine as E
    n, m, N, T = M["n"], M["m"], M["N"], M["T"]
    dx, dP, dz = E.to_records(M["x0"], layout, 0), E.to_records(M["P0"], layout, 0), E.to_records(zz, layout, 1)
    dmask = None if mask is None else torch.as_tensor(np.ascontiguousarray(mask, dtype=np.uint8), device=dx.device)
    shapes = dict(means=(n,), covs=(n, n), means_p=(n,), covs_p=(n, n), K=(n, m), S=(m, m), SI=(m, m), y=(m,))
    rec = {k: E.alloc_records((T,), N, int(np.prod(s)), layout).fill_(float("nan")) for k, s in shapes.items()}
    sc = {k: torch.full((T, N), float("nan"), dtype=torch.float64, device=dx.device) for k in ("log_likelihood", "mahalanobis")}
    st = torch.full((N,), -1, dtype=torch.int32, device=dx.device)
    E.kf_batch_filter_ex(dict(n=n, m=m, nu=0, model_mode=0, N=N, T=T, layout=E.LAYOUTS[layout], update_first=0, alpha_sq=1.0),
                         E.dev(M["F"]), E.dev(M["Q"]), E.dev(M["H"]), E.dev(M["R"]), dz, dx, dP,
                         dict(sc, **{k: rec[k] for k in ("K", "S", "SI", "y")}), mask=dmask,
                         means=rec["means"], covs=rec["covs"], means_p=rec["means_p"], covs_p=rec["covs_p"], status=st)
    torch.cuda.synchronize()
    got = [E.from_records(rec[k], layout, 1, shapes[k]) for k in kf_hp.OUTPUTS]
    return got + [sc["log_likelihood"].cpu().numpy(), sc["mahalanobis"].cpu().numpy()], st.cpu().numpy()


@pytest.mark.parametrize("layout", ["soa", "aos"])
@pytest.mark.parametrize("org,n,m,masked", HISTORY_CASES, ids=[c[0].replace(" ", "_").replace(",", "") for c in HISTORY_CASES])
def test_likelihood_histories_vs_extended_precision(org, n, m, masked, layout, monkeypatch):
    """log_likelihood and mahalanobis per step next to K, S, SI, y and the four regular outputs, on the stiff family: kf_fast's
    extras with the mask, kf_mlg's EX instantiation (no mask), and the general kernel, which has the masked (12,3) call and
    stores y = 0 with the kept S and SI at the missing step"""
    t = oh.truth_opts("stiff", n, m, Opt(masked=masked))
    oh.measures_something(t)
    M = t["model"]
    mask, zz = _bank_zs(M)
    got, status = _run_ex(M, zz, mask, layout)
    assert not status.any(), status[status != 0]
    assert all(np.all(np.isfinite(a)) for a in got)
    if org.startswith("general"):
        with monkeypatch.context() as mp:
            mp.setenv("FK_NO_FAST", "1")
            mp.setenv("FK_NO_FAST_EX", "1")
            ref, _ = _run_ex(M, zz, mask, layout)
        assert all(np.array_equal(a, b) for a, b in zip(got, ref))
    eg = oh.errors([_checked(a, M) for a in got], t["hp"], oh.OUTPUTS)
    _report(f"{org} ({n},{m}) stiff {layout}", eg, t, oh.OUTPUTS, _checked(got[0], M))


@pytest.mark.parametrize("n,m", CLASS_DIMS)
def test_drop_in_class_step_by_step_vs_extended_precision(n, m):
    """one KalmanFilter through predict(u) / update(z), None at step 8, on checked track 0 of the stiff family with a control
    input: fk_kf_predict_f64 / fk_kf_update_f64 of the general kernel; x, P, the priors, K, S, SI, y and log_likelihood"""
    from filterpy_amd.kalman import KalmanFilter
    o = Opt(nu=2)
    t = oh.truth_opts("stiff", n, m, o)
    oh.measures_something(t)
    M, bm = t["model"], t["inputs"]
    trk = M["tracks"][0]
    assert trk == 0
    kf = KalmanFilter(dim_x=n, dim_z=m, dim_u=o.nu)
    kf.x, kf.P = M["x0"][trk].copy(), M["P0"][trk].copy()
    kf.F, kf.Q, kf.H, kf.R, kf.B = (bm[k].copy() for k in ("F", "Q", "H", "R", "B"))
    got = [[] for _ in oh.OUTPUTS]
    for s in range(M["T"]):
        kf.predict(u=bm["us"][s, trk])
        xp, Pp = kf.x.copy(), kf.P.copy()
        kf.update(M["zs"][s, trk] if M["mask"][s] else None)
        for lst, v in zip(got, (kf.x, kf.P, xp, Pp, kf.K, kf.S, kf.SI, np.ravel(kf.y), kf.log_likelihood, kf.mahalanobis)):
            lst.append(np.array(v, dtype=float))
    assert all(np.all(np.isfinite(v)) for v in got)
    one = dict(t, hp=[h[:1] for h in t["hp"]], ref=t["ref"][:, :1], eo=t["eo"][:, :1])
    eg = oh.errors([np.array(v)[None] for v in got], one["hp"], oh.OUTPUTS)
    for name, eb, bo, ro in oh.ratios(eg, one, oh.OUTPUTS):
        print("%-58s %-8s err/bar %.3f  gpu/oracle %6.2f  ref/oracle %6.2f" % (f"KalmanFilter ({n},{m}) stiff", name, eb, bo, ro))
    bad = oh.check(f"KalmanFilter ({n},{m}) stiff", eg, one, oh.OUTPUTS)
    assert not bad, (bad, eg[:, 0], one["ref"][:, 0])
    assert oh.err(np.array(got[0]), t["hp_next"][0]) > 1e-3


def _corr_bank(t, family, n, m, per_track, single, layout):
    """the bank through KalmanFilterBank.update_correlated -> the six arrays of CORR_OUTPUTS [steps][N]...; one track that is not
    checked is masked at every update and must keep its bits"""
    from filterpy_amd.kalman import KalmanFilterBank
    M = t["model"]
    N = M["N"]
    idle = next(i for i in range(N) if i not in M["tracks"])
    mask = np.ones(N, dtype=bool)
    mask[idle] = False
    bank = KalmanFilterBank(n, m, N, layout=layout)
    bank.F, bank.Q, bank.H, bank.R, bank.M = M["F"], M["Q"], M["H"], M["R"], t["M"]
    bank.x, bank.P = M["x0"].copy(), M["P0"].copy()
    got = [[] for _ in oh.CORR_OUTPUTS]
    for s in range(len(t["steps"])):
        if single:
            bank.x, bank.P = t["xp"][s].copy(), t["Pp"][s].copy()
        else:
            bank.predict()
        x, P = np.array(bank.x[idle]), np.array(bank.P[idle])
        bank.update_correlated(t["zs"][s], mask=mask)
        assert np.array_equal(bank.x[idle], x) and np.array_equal(bank.P[idle], P)
        for lst, v in zip(got, (bank.x, bank.P, bank.K, bank.S, bank.SI, bank.y)):
            lst.append(np.array(v))
    return [np.array(v) for v in got]


def _corr_case(family, n, m, per_track, single, layout):
    t = oh.truth_corr(family, n, m, per_track, single)
    oh.measures_something(t)
    M = t["model"]
    got = _corr_bank(t, family, n, m, per_track, single, layout)
    live = [_checked(a, M) for a in got]
    assert all(np.all(np.isfinite(a)) for a in live)
    eg = oh.errors(live, t["hp"], oh.CORR_OUTPUTS)
    what = "%s %s M" % ("single updates" if single else "recursion", "per-track" if per_track else "shared")
    _report(f"update_correlated {what} ({n},{m}) {family} {layout}", eg, t, oh.CORR_OUTPUTS, live[0])


@pytest.mark.parametrize("layout", ["soa", "aos"])
@pytest.mark.parametrize("per_track", [False, True], ids=["shared_M", "per_track_M"])
@pytest.mark.parametrize("family,n,m", CORR_RECURSION)
def test_update_correlated_recursion_vs_extended_precision(family, n, m, per_track, layout):
    """12 x {predict; update_correlated}: the exact classes up to (9,4), the rolled (12,8) and (16,8), (10,5) padded into (12,8)"""
    _corr_case(family, n, m, per_track, False, layout)


@pytest.mark.parametrize("layout", ["soa", "aos"])
@pytest.mark.parametrize("per_track", [False, True], ids=["shared_M", "per_track_M"])
@pytest.mark.parametrize("family,n,m", CORR_SINGLE)
def test_update_correlated_on_stiff_priors_vs_extended_precision(family, n, m, per_track, layout):
    """on stiff at (9,4) and above the non-Joseph recursion loses positive definiteness in the truth itself, so there: one
    update_correlated on the plain truth's priors of steps 0 and 12, rounded to float64"""
    _corr_case(family, n, m, per_track, True, layout)


def _steady_case(what, n, m, per_track, nu, family, layout):
    from filterpy_amd.kalman import KalmanFilterBank
    t = oh.truth_steady(family, n, m, per_track, nu)
    oh.measures_something(t)
    M = t["model"]
    mask, zz = _bank_zs(M)
    bank = KalmanFilterBank(n, m, M["N"], dim_u=nu, layout=layout)
    bank.x, bank.F, bank.H, bank.K, bank.B = M["x0"].copy(), M["F"], M["H"], t["K"], t["B"]
    got = bank.steadystate_filter(zz, mask=mask, us=t["us"])
    live = [_checked(np.asarray(a), M) for a in got]
    assert all(np.all(np.isfinite(np.asarray(a))) for a in got)
    eg = oh.errors(live, t["hp"], oh.STEADY_OUTPUTS)
    label = "steady %s %s K nu %d (%d,%d) %s %s" % (what, "per-track" if per_track else "shared", nu, n, m, family, layout)
    _report(label, eg, t, oh.STEADY_OUTPUTS, live[0])


@pytest.mark.parametrize("layout", ["soa", "aos"])
@pytest.mark.parametrize("family", kf_hp.FAMILIES)
@pytest.mark.parametrize("what,n,m,per_track,nu", STEADY_CASES, ids=["%s-%d-%d-%s-nu%d" % (c[0], c[1], c[2], "Kn" if c[3] else "K1", c[4])
                                                                     for c in STEADY_CASES])
def test_steadystate_filter_vs_extended_precision(what, n, m, per_track, nu, family, layout):
    """steady_kernel EXACT, guarded, with a shared gain in LDS (KREG = false) and a per-track gain in registers, and the padded
    (14,6); K is the float64 rounding of the truth's last gain, with and without a control input"""
    _steady_case(what, n, m, per_track, nu, family, layout)


def test_steadystate_filter_rolled_unit_vs_extended_precision():
    """FK_STEADY_ROLLED=1 is read once per process, so the rolled unit runs in a child process of its own"""
    code = ("import test_gpu_kf_options_precision as g\n"
            "for layout in ('soa', 'aos'):\n"
            "    g._steady_case(*g.STEADY_ROLLED, 'stiff', layout)\n")
    here = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, FK_STEADY_ROLLED="1", PYTHONPATH=os.pathsep.join([here, os.path.dirname(here), os.environ.get("PYTHONPATH", "")]))
    r = subprocess.run([sys.executable, "-c", code], env=env, cwd=here, capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert r.stdout.count("gpu/oracle") == 2 * len(oh.STEADY_OUTPUTS)                # both layouts ran and printed their rows


@pytest.mark.parametrize("layout", ["soa", "aos"])
@pytest.mark.parametrize("n,m", GIVEN_INV_DIMS)
def test_given_inverse_update_vs_extended_precision(n, m, layout):
    """kf_given_inv.hip's update side on the stiff priors of steps 0 and 12: FK_KF_FLAG_S_ONLY gives y and S and leaves x and P
    bit-identical; with SI = the float64 rounding of the longdouble inverse of the RETURNED S, FK_KF_FLAG_SI_GIVEN gives x, P, K"""
    import torch
    from filterpy_amd import _engine as E, _abi
    t = oh.truth_corr("stiff", n, m, single=True, joseph=True)             # the Joseph-form update on those priors
    oh.measures_something(t)
    M, N = t["model"], t["model"]["N"]
    rec = lambda a: E.to_records(np.ascontiguousarray(a), layout, 0)          # noqa: E731
    back = lambda a, shp: E.from_records(a, layout, 0, shp)                   # noqa: E731
    desc = dict(n=n, m=m, nu=0, model_mode=_abi.FK_MODEL_SHARED, N=N, T=1, layout=E.LAYOUTS[layout], update_first=0, alpha_sq=1.0)
    got = {k: [] for k in ("x", "P", "K", "S", "y")}
    for s in range(len(t["steps"])):
        x0, P0, z = t["xp"][s], t["Pp"][s], t["zs"][s]
        dx, dP = rec(x0), rec(P0)
        o = dict(y=E.alloc_records((), N, m, layout).zero_(), K=E.alloc_records((), N, n * m, layout).zero_(),
                 S=E.alloc_records((), N, m * m, layout).zero_(), SI=E.alloc_records((), N, m * m, layout).zero_())
        st = torch.zeros(N, dtype=torch.int32, device="cuda")
        E.kf_update(dict(desc, flags=_abi.FK_KF_FLAG_S_ONLY), E.dev(M["H"]), E.dev(M["R"]), rec(z), dx, dP, status=st, **o)
        assert not st.any()
        assert np.array_equal(back(dx, (n,)), x0) and np.array_equal(back(dP, (n, n)), P0)
        S, y = np.array(back(o["S"], (m, m))), np.array(back(o["y"], (m,)))
        o["SI"] = rec(np.array([oh.spd_inv(oh.ld(Si)).astype(np.float64) for Si in S]))
        E.kf_update(dict(desc, flags=_abi.FK_KF_FLAG_SI_GIVEN), E.dev(M["H"]), E.dev(M["R"]), rec(z), dx, dP, status=st, **o)
        assert not st.any()
        for k, v in dict(x=back(dx, (n,)), P=back(dP, (n, n)), K=back(o["K"], (n, m)), S=S, y=y).items():
            got[k].append(np.array(v))
    names = tuple(got)
    live = {k: _checked(np.array(v), M) for k, v in got.items()}
    assert all(np.all(np.isfinite(a)) for a in live.values())
    eg = oh.errors([live.get(k) for k in oh.CORR_OUTPUTS], t["hp"], oh.CORR_OUTPUTS)
    _report(f"given inverse ({n},{m}) stiff {layout}", eg, t, names, live["x"])
