"""CPU: the truth of tests/test_gpu_kf_options_precision.py (tests/kf_opts_hp.py: the reference's batch_filter with options, its
log-likelihood and Mahalanobis histories, update_correlated and the steady-state pair in longdouble) is a truth, its models measure
something for every key the GPU file uses, its inputs tell the characteristic mistakes of the kernels apart, and the host builds
that already take the options (hc_kf_batch with alpha_sq and update_first, hc_kf_batch_sym with alpha_sq) meet the same bar.

Every row prints its figures; docs/MEASUREMENTS.md ("KF options and variants precision") has the table."""
import numpy as np
import pytest

import kf_hp
import kf_opts_hp as oh
import test_gpu_kf_options_precision as gpu
from kf_opts_hp import ALPHA_SQ, Opt
from test_host_kf_hp import DIMS, SYM_DIMS
from test_hostcheck_math import hc_batch, hc_batch_sym

ALL2, ALL4 = gpu._all(2), gpu._all(4)
UF, ALPHA, STEP = Opt(update_first=True), Opt(alpha_sq=ALPHA_SQ), Opt(per_step=True)
# every (dim_x, dim_z, option set) of the GPU file's forward table, written out: the guard below compares
FORWARD_KEYS = [(4, 2, UF), (6, 3, UF), (4, 2, Opt(nu=2)), (6, 3, Opt(nu=4)), (6, 3, Opt(nu=3)), (6, 3, STEP), (4, 2, STEP),
                (6, 3, Opt()), (2, 1, ALPHA), (6, 3, ALPHA), (8, 4, ALPHA), (9, 3, Opt(nu=2)), (9, 3, STEP),
                (9, 3, Opt(nu=2, per_step=True)), (9, 3, UF), (9, 3, ALL2), (9, 3, ALPHA), (12, 3, ALPHA), (8, 4, Opt(nu=2)),
                (8, 4, UF), (8, 4, STEP), (12, 3, Opt(nu=5)), (12, 3, ALL4), (5, 4, Opt(nu=2, alpha_sq=ALPHA_SQ, update_first=True)),
                (9, 4, Opt(nu=4)), (9, 4, STEP), (9, 4, ALL4), (12, 3, Opt(nu=4)), (12, 3, STEP), (16, 8, Opt(nu=4)), (16, 8, STEP),
                (16, 8, ALL4)]
HISTORY_KEYS = [(4, 2, Opt()), (12, 3, Opt(masked=False)), (12, 3, Opt())]
CLASS_KEYS = [(4, 2, Opt(nu=2)), (9, 3, Opt(nu=2)), (12, 3, Opt(nu=2))]
CORR_DIMS = [(4, 2), (6, 3), (9, 4), (12, 8), (16, 8), (10, 5)]
CORR_KEYS = [(f, n, m, False) for f in ("benign", "stiff_small_weights") for n, m in CORR_DIMS] + \
            [("stiff", 4, 2, False), ("stiff", 6, 3, False)] + [("stiff", n, m, True) for n, m in CORR_DIMS[2:]]
STEADY_KEYS = [(2, 1, False, 0), (6, 3, True, 2), (9, 3, False, 4), (5, 2, False, 2), (5, 2, True, 0), (12, 8, False, 0),
               (12, 8, True, 2), (16, 8, False, 2), (16, 8, True, 0), (14, 6, False, 2), (14, 6, True, 0), (12, 8, False, 2)]
GIVEN_KEYS = [(6, 3), (12, 3)]


def _oid(o):
    return "nu%d%s%s%s%s" % (o.nu, "-step" if o.per_step else "", "-alpha" if o.alpha_sq != 1 else "", "-uf" if o.update_first else "",
                             "" if o.masked else "-nomask")


FWD_IDS = ["%d-%d-%s" % (n, m, _oid(o)) for n, m, o in FORWARD_KEYS]


def test_every_key_of_the_gpu_file_is_checked_here():
    """the GPU file's parametrisation against the keys this file asserts the condition for"""
    assert {(c[1], c[2], c[5]) for c in gpu.FORWARD_CASES} == set(FORWARD_KEYS)
    assert {(c[1], c[2], Opt(masked=c[3])) for c in gpu.HISTORY_CASES} == set(HISTORY_KEYS)
    assert {(n, m, Opt(nu=2)) for n, m in gpu.CLASS_DIMS} == set(CLASS_KEYS)
    assert {c + (False,) for c in gpu.CORR_RECURSION} | {c + (True,) for c in gpu.CORR_SINGLE} == set(CORR_KEYS)
    assert {c[1:] for c in gpu.STEADY_CASES + [gpu.STEADY_ROLLED]} == set(STEADY_KEYS)
    assert gpu.GIVEN_INV_DIMS == GIVEN_KEYS
    # every organisation of the issue's tables has a case, in both layouts and on all three families (the parametrisation)
    orgs = " | ".join(c[0] for c in gpu.FORWARD_CASES)
    for word in ("kf_fast UF", "kf_fast CTRL", "per-step", "per-track-step", "per-track", "full alpha", "packed alpha", "one wave alpha",
                 "kf_ml VAR", "kf_ml VAR+UF", "kf_mlg VAR", "kf_mlg VAR+UF", "kf_ml plain alpha", "kf_mlg plain alpha", "general exact",
                 "general rolled", "FK_ML_VAR=0", "general padded"):
        assert word in orgs, word


def _y_close(y_o, y_hp, z, tol=1e-13):
    """y = z - H x is a difference: it agrees to `tol` of its OPERANDS, max(|z|, |H x|) per step (tests/test_host_kf_hp.py)"""
    z = kf_hp.ld(z)
    scale = np.maximum(np.abs(z).max(axis=-1), np.abs(z - y_hp).max(axis=-1))
    return np.all(np.abs(kf_hp.ld(y_o) - y_hp).max(axis=-1) <= tol * scale)


def _agree(t, zs_of):
    """on benign: every output but y to 1e-13 by the test's own error, y to 1e-13 of its operands"""
    names = t["outputs"]
    rows = [j for j, k in enumerate(names) if k != "y"]
    assert t["eo"][rows].max() < 1e-13, dict(zip(names, t["eo"].max(axis=1)))
    j = names.index("y")
    for k, trk in enumerate(t["model"]["tracks"]):
        assert _y_close(t["oracle"][j][k], t["hp"][j][k], zs_of(trk)), (trk,)


@pytest.mark.parametrize("n,m,o", FORWARD_KEYS + HISTORY_KEYS + CLASS_KEYS[:1], ids=FWD_IDS + ["hist-%d-%d-%s" % (n, m, _oid(o)) for n, m, o in HISTORY_KEYS] + ["class-4-2"])
def test_the_truth_is_a_truth_with_options(n, m, o):
    """benign: the float64 oracle and the longdouble filter agree to 1e-13 on all ten outputs (ll and maha too) of every option set"""
    t = oh.truth_opts("benign", n, m, o)
    oh.measures_something(t)
    M = t["model"]
    _agree(t, lambda trk: M["zs"][:, trk] * M["mask"][:, None])
    miss = np.flatnonzero(M["mask"] == 0)
    for s in miss:                                                      # y = 0, S and SI kept: ll is the density's peak, maha 0
        assert not t["hp"][7][:, s].any() and not t["hp"][9][:, s].any()
        assert np.array_equal(t["hp"][5][:, s], t["hp"][5][:, s - 1]) and np.all(t["hp"][8][:, s] > t["hp"][8][:, s - 1])
    if o.update_first:                                                  # update -> posterior -> predict -> prior
        F0 = kf_hp.ld(t["inputs"]["F"][0] if o.per_step else t["inputs"]["F"])
        if not o.nu:
            assert oh.err((F0 @ t["hp"][0][:, 0].T).T, t["hp"][2][:, 0]) < 1e-17


@pytest.mark.parametrize("n,m", CORR_DIMS)
@pytest.mark.parametrize("per_track", [False, True])
def test_the_truth_is_a_truth_correlated(n, m, per_track):
    t = oh.truth_corr("benign", n, m, per_track)
    oh.measures_something(t)
    _agree(t, lambda trk: t["zs"][:, trk])
    M = t["model"]                                                       # the joint noise covariance is PSD: S stays PD
    Mc = t["M"][3] if per_track else t["M"]
    assert np.linalg.eigvalsh(np.block([[M["Q"], Mc], [Mc.T, M["R"]]])).min() > -1e-12 * np.abs(M["Q"]).max()


@pytest.mark.parametrize("n,m,per_track,nu", STEADY_KEYS)
def test_the_truth_is_a_truth_steadystate(n, m, per_track, nu):
    t = oh.truth_steady("benign", n, m, per_track, nu)
    oh.measures_something(t)
    M = t["model"]
    _agree(t, lambda trk: M["zs"][:, trk] * M["mask"][:, None])
    assert not t["hp"][2][:, kf_hp.ukf_hp.T_MISSING].any()
    assert np.array_equal(t["hp"][0][:, kf_hp.ukf_hp.T_MISSING], t["hp"][1][:, kf_hp.ukf_hp.T_MISSING])


def _row(label, t):
    print("%-52s oracle max %s | ref/oracle max %.1f" % (label, " ".join("%s %.1e" % kv for kv in zip(t["outputs"], t["eo"].max(axis=1))),
                                                        (t["ref"].max(axis=1) / np.maximum(t["eo"].max(axis=1), 1e-300)).max()))


@pytest.mark.parametrize("family", kf_hp.FAMILIES)
@pytest.mark.parametrize("n,m,o", FORWARD_KEYS + HISTORY_KEYS + CLASS_KEYS, ids=FWD_IDS + ["hist-%d-%d-%s" % (n, m, _oid(o)) for n, m, o in HISTORY_KEYS] +
                         ["class-%d-%d" % (n, m) for n, m, _ in CLASS_KEYS])
def test_models_measure_something_with_options(family, n, m, o):
    """the condition of the precision tests for every (family, dims, option set) of the GPU file: all 16 tracks finish in the
    oracle and in every perturbed run, err(oracle, hp) < 1e-3 on every output, and a track is not its neighbour.  ll and maha
    belong to the keys of the history and class tests: the oracle's log-likelihood is the reference's, scipy's logpdf with
    allow_singular, which drops an eigenvalue of S below 2.2e-10 of the largest and answers -inf -- as on stiff at (5,4) with
    update_first, where no test reads it."""
    t = oh.truth_opts(family, n, m, o)
    oh.measures_something(t, oh.OUTPUTS if (n, m, o) in HISTORY_KEYS + CLASS_KEYS else kf_hp.OUTPUTS)
    _row("%s (%d,%d) %s" % (family, n, m, _oid(o)), t)
    assert oh.not_the_neighbour(t["hp"][0], t) and oh.not_the_neighbour(t["oracle"][0], t)


@pytest.mark.parametrize("per_track", [False, True])
@pytest.mark.parametrize("family,n,m,single", CORR_KEYS)
def test_models_measure_something_correlated(family, n, m, single, per_track):
    t = oh.truth_corr(family, n, m, per_track, single)
    oh.measures_something(t)
    _row("corr %s %s (%d,%d) %s M" % ("singles" if single else "recursion", family, n, m, "per-track" if per_track else "shared"), t)
    assert oh.not_the_neighbour(t["hp"][0], t) and oh.not_the_neighbour(t["oracle"][0], t)


@pytest.mark.parametrize("n,m", GIVEN_KEYS)
def test_models_measure_something_given_inverse(n, m):
    t = oh.truth_corr("stiff", n, m, single=True, joseph=True)
    oh.measures_something(t)
    _row("Joseph singles stiff (%d,%d)" % (n, m), t)
    assert oh.not_the_neighbour(t["hp"][0], t)


@pytest.mark.parametrize("family", kf_hp.FAMILIES)
@pytest.mark.parametrize("n,m,per_track,nu", STEADY_KEYS)
def test_models_measure_something_steadystate(family, n, m, per_track, nu):
    t = oh.truth_steady(family, n, m, per_track, nu)
    oh.measures_something(t)
    _row("steady %s (%d,%d) %s K nu %d" % (family, n, m, "per-track" if per_track else "shared", nu), t)
    assert oh.not_the_neighbour(t["hp"][0], t) and oh.not_the_neighbour(t["oracle"][0], t)


# ---- the inputs tell the characteristic mistakes apart: each mistaken truth sits above the bar ------------------------------
MISTAKES = [("model_next", 6, 3, STEP), ("model_next", 9, 3, STEP), ("model_next", 12, 3, STEP), ("model_next", 16, 8, ALL4),
            ("B_prev", 9, 3, Opt(nu=2, per_step=True)), ("B_prev", 9, 3, ALL2), ("B_prev", 12, 3, ALL4), ("B_prev", 16, 8, ALL4),
            ("alpha_Q", 2, 1, ALPHA), ("alpha_Q", 6, 3, ALPHA), ("alpha_Q", 9, 3, ALPHA), ("alpha_Q", 12, 3, ALPHA),
            ("alpha_Q", 5, 4, Opt(nu=2, alpha_sq=ALPHA_SQ, update_first=True)),
            ("prior_early", 4, 2, UF), ("prior_early", 9, 3, UF), ("prior_early", 8, 4, UF), ("prior_early", 12, 3, ALL4)]


def _above_the_bar(label, wrong, t, names):
    eg = oh.errors(wrong["hp"], t["hp"], t["outputs"])
    for name, eb, _, _ in oh.ratios(eg, t, names):
        print("%-52s %-8s err/bar %.3g" % (label, name, eb))
    return oh.check(label, eg, t, names)


@pytest.mark.parametrize("family", kf_hp.FAMILIES)
@pytest.mark.parametrize("mistake,n,m,o", MISTAKES, ids=["%s-%d-%d-%s" % (k, n, m, _oid(o)) for k, n, m, o in MISTAKES])
def test_a_mistaken_filter_sits_above_the_bar(mistake, n, m, o, family):
    """model t + 1 used at step t, Bs[t - 1] with us[t], alpha applied to Q too, the prior stored before the predict: the truth
    recomputed with the mistake fails kf_opts_hp.check on the four forward outputs, on every family"""
    t = oh.truth_opts(family, n, m, o)
    oh.measures_something(t, oh.FORWARD)
    bad = _above_the_bar(f"{mistake} {family} ({n},{m})", oh.truth_opts(family, n, m, o, mutate=mistake), t, oh.FORWARD)
    assert bad, (mistake, family, n, m)


@pytest.mark.parametrize("per_track", [False, True])
@pytest.mark.parametrize("family,n,m,single", CORR_KEYS)
def test_a_dropped_M_sits_above_the_bar(family, n, m, single, per_track):
    """M' dropped from H P + M' fails the check of P wherever update_correlated is tested.  In the recursions on the stiff
    families the mistaken P loses positive definiteness within the 12 steps (the longdouble Cholesky factorisation of S raises):
    there the steps before that are compared, at least two of them, against the bar of the whole run"""
    t = oh.truth_corr(family, n, m, per_track, single)
    wrong = oh.truth_corr(family, n, m, per_track, single, mutate="drop_Mt")
    reached = [len(v) for v in wrong["hp"][1]]
    print("steps reached", reached)
    assert min(reached) >= 2
    j = t["outputs"].index("P")
    eg = np.full((len(t["outputs"]), 16), np.nan)
    eg[j] = [oh.err(w, t["hp"][j][k][:len(w)]) for k, w in enumerate(wrong["hp"][j])]
    bad = oh.check(f"drop_Mt {family} ({n},{m})", eg, t, ("P",))
    assert bad, (family, n, m, single, per_track)


# ---- the host builds that already take the options ---------------------------------------------------------------------------
def _hold(label, fn, family, n, m, o):
    t = oh.truth_opts(family, n, m, o)
    oh.measures_something(t, oh.FORWARD)
    M = t["model"]
    out = [[] for _ in range(4)]
    for trk in M["tracks"]:
        kw = dict(update_first=True) if o.update_first else {}
        res = fn(M["x0"][trk], M["P0"][trk], M["zs"][:, trk], M["F"], M["Q"], M["H"], M["R"], mask=M["mask"], alpha_sq=o.alpha_sq, **kw)
        assert res[-1] == 0, (trk, res[-1])
        for lst, a in zip(out, res[:4]):
            lst.append(a)
    eg = np.full((len(oh.OUTPUTS), 16), np.nan)
    eg[:4] = oh.errors([np.array(a) for a in out], t["hp"][:4], oh.FORWARD)
    for name, eb, bo, ro in oh.ratios(eg, t, oh.FORWARD):
        print("%-6s %-20s (%d,%d) %-12s %-8s err/bar %.3f  build/oracle %6.2f  ref/oracle %6.2f" % (label, family, n, m, _oid(o), name, eb, bo, ro))
    return oh.check(f"{label} {family} ({n},{m}) {_oid(o)}", eg, t, oh.FORWARD)


@pytest.mark.parametrize("n,m", DIMS)
@pytest.mark.parametrize("family", kf_hp.FAMILIES)
def test_full_host_build_with_alpha_and_update_first_meets_the_bar(family, n, m):
    """hc_kf_batch (fk_math.hpp: the arithmetic of kf_kernels.hip and of kf_fast's full instantiations) with alpha_sq = 1.05 and
    update_first at once: worst 0.438 of the bar (means_p, stiff (16,8)).  This is the test that found kf_update factorising one
    triangle of an S that is symmetric only up to rounding: stiff (16,8) was at 1.291 of the bar in the means (21.5 x the oracle's
    own error; 0.797 with alpha_sq alone) until the factorisation was given (S + S') / 2.  docs/MEASUREMENTS.md ("KF options and
    variants precision") has the rows before and after."""
    bad = _hold("full", hc_batch, family, n, m, Opt(alpha_sq=ALPHA_SQ, update_first=True))
    assert not bad, bad


@pytest.mark.parametrize("n,m", SYM_DIMS)
@pytest.mark.parametrize("family", kf_hp.FAMILIES)
def test_packed_symmetric_host_build_with_alpha_meets_the_bar(family, n, m):
    bad = _hold("packed", hc_batch_sym, family, n, m, ALPHA)
    assert not bad, bad
