"""The reference's Rauch-Tung-Striebel smoother of the linear Kalman filter for ONE track in np.longdouble (80-bit on x86-64),
written from the algorithm (KalmanFilter.rts_smoother, kalman_filter.py:1066-1072, F[k+1] / Q[k+1]; the module function,
:1851-1856, F[k] / Q[k]):

    Pp[k] = (F P[k]) F' + Q        K[k] = (P[k] F') inv(Pp[k])        x[k] += K (x[k+1] - F x[k])
    P[k] += (K (P[k+1] - Pp[k])) K'

with inv(Pp) from a longdouble Cholesky factorisation (ukf_hp.spd_inv); the last step is the filter's own, its gain zero.

This is the truth tests/test_gpu_rts_precision.py and tests/test_host_rts_hp.py measure the smoother kernels and the float64
oracle (oracle/kf_oracle.py's rts_smoother) against, on the model families of ukf_hp.models: N = 150 tracks with their own x0
and measurements, T = 16, the measurement of step 8 missing, 16 checked tracks.

The smoother's INPUTS are float64 and the same for the truth, the oracle and a kernel: the oracle's forward pass
(kf_oracle.kf_batch_filter), its means and covariances of the steps ukf_hp.SMOOTH_FROM = 4 .. 15 (a window of 12 steps; ukf_hp.py
says why the first four are left out: with P0 = 1e6 I their smoothed covariance cancels nine or ten digits in ANY float64
arithmetic), every covariance symmetrised to (P + P') / 2 first -- a kernel that reads one triangle and a reference that reads
both then have the same input.

Modes of a truth:
    "shared"            one F, Q for every step
    "class" / "module"  per-step models Fs[t] = F + 0.02 (t / T) subdiag(1), Qs[t] = Q (1 + t / T), t = 0 .. T-1 of the FILTER's
                        steps; the oracle's forward pass runs with them, the smoother over the slices [SMOOTH_FROM:], with
                        Fs[k+1] (off = 1, the class) or Fs[k] (off = 0, the module function)
    "given"             shared models, inv(Pp[k]) supplied by the caller: the float64 rounding of spd_inv(Pp_hp[k]); the truth is
                        the longdouble recursion with those very arrays, the oracle is rts_smoother(inv=) handing them back

The bar is kf_hp's, unchanged: the REFERENCE ERROR of a track and output is

    ref = max(err(oracle, hp), max over K_DRAWS = 8 draws of err(oracle on inputs moved by one ulp, hp))

(Xs, Ps, F and Q perturbed, symmetric matrices staying symmetric; hp always the truth of the UNPERTURBED inputs), and check()
holds a build to

    every checked track      err(build, hp) <= max(MARGIN * max_tracks ref, FLOOR)
    the median over tracks   median err(build, hp) <= max(MARGIN * median ref, FLOOR)

with kf_hp.MARGIN = 8 and ukf_hp.FLOOR = 1e-13.  Errors are normwise per step, the worst step counted (ukf_hp.err); K and Pp are
compared without their last step (zero / a copy of the input)."""
import os
import sys

import numpy as np

import kf_hp
import ukf_hp
from ukf_hp import LD, err, ld, spd_inv

MARGIN = kf_hp.MARGIN
FLOOR = ukf_hp.FLOOR
K_DRAWS = kf_hp.K_DRAWS
FAMILIES = kf_hp.FAMILIES
OUTPUTS = ("xs", "Ps", "K", "Pp")
MODES = ("shared", "class", "module", "given")
FROM = ukf_hp.SMOOTH_FROM
_CUT = {"xs": slice(None), "Ps": slice(None), "K": slice(None, -1), "Pp": slice(None, -1)}


# ------------------------------------------------------------------------------------------------------------ the truth
def _steps(M, T):
    """one matrix, or one per step -> [T]"""
    M = ld(M)
    return [M] * T if M.ndim == 2 else list(M)


def _inv(Pp, memo):
    """spd_inv(Pp); memo: the inverses already computed, by the bits of Pp -- the stiff families give every track the same P0,
    so the covariances (not the means) of all N tracks are the same numbers and need one factorisation each"""
    if memo is None:
        return spd_inv(Pp)
    key = Pp.tobytes()
    if key not in memo:
        memo[key] = spd_inv(Pp)
    return memo[key]


def rts_smoother(Xs, Ps, Fs, Qs, off, invs=None, memo=None):
    """xs, Ps, K, Pp [T] of one track.  off = 1: F, Q = Fs[k+1], Qs[k+1] (the class); off = 0: Fs[k], Qs[k] (the module
    function).  invs [T]: inverses of Pp[k] supplied by the caller, used in place of the Cholesky inverse."""
    Xs, Ps = ld(Xs), ld(Ps)
    T, n = Xs.shape
    Fs, Qs = _steps(Fs, T), _steps(Qs, T)
    x, P, Pp, K = Xs.copy(), Ps.copy(), Ps.copy(), np.zeros((T, n, n), LD)
    for k in range(T - 2, -1, -1):
        F, Q = Fs[k + off], Qs[k + off]
        Pp[k] = (F @ P[k]) @ F.T + Q
        K[k] = (P[k] @ F.T) @ (_inv(Pp[k], memo) if invs is None else ld(invs[k]))
        x[k] += K[k] @ (x[k + 1] - F @ x[k])
        P[k] += (K[k] @ (P[k + 1] - Pp[k])) @ K[k].T
    return x, P, K, Pp


# ------------------------------------------------------------------------------------------------------- inputs and reference
def step_models(F, Q, T):
    """the per-step variant: Fs[t] = F + 0.02 (t / T) subdiag(1), Qs[t] = Q (1 + t / T)"""
    n = F.shape[0]
    t = np.arange(T) / T
    return F + 0.02 * t[:, None, None] * np.diag(np.ones(n - 1), -1), Q * (1.0 + t)[:, None, None]


def _oracle():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if root not in sys.path:
        sys.path.insert(0, root)
    from oracle import kf_oracle
    return kf_oracle


def _smooth(Xs, Ps, F, Q, mode, invs=None):
    """oracle/kf_oracle.py's rts_smoother in the order of OUTPUTS; None where float64 itself breaks down"""
    kw = {}
    if invs is not None:
        it = iter(invs[-2::-1])                                  # asked for at k = T-2 .. 0: the same arrays, handed back
        kw["inv"] = lambda A: next(it)
    try:
        return _oracle().rts_smoother(np.array(Xs), np.array(Ps), F, Q, "module" if mode == "module" else "class", **kw)
    except np.linalg.LinAlgError:
        return None


def errors(got, hp):
    """[outputs][tracks]: err of `got` (four arrays [tracks][T]...) against hp, K and Pp without their last step"""
    out = np.full((len(OUTPUTS), len(hp[0])), np.nan)
    for j, name in enumerate(OUTPUTS):
        c = _CUT[name]
        out[j] = [err(np.asarray(got[j][i])[c], hp[j][i][c]) for i in range(len(hp[j]))]
    return out


_truth_cache = {}


def truth(family, n, m, mode="shared"):
    """Computed once per key and shared, never modified:
    model   the ukf_hp.models dict
    Xs, Ps  the smoother's float64 inputs of ALL N tracks, [12][N]...: the oracle's forward pass from step 4, symmetrised
    F, Q    the models as the smoother takes them: (n, n), or [12](n, n) for the per-step modes
    invs    mode "given": the supplied inverses [12][N](n, n), float64 (the last step's is never read: zero)
    off     1: Fs[k+1] (the class; index_convention 0 of the C ABI), 0: Fs[k] (the module function; index_convention 1)
    hp      the four longdouble outputs of the 16 checked tracks, [16][12]... each;  oracle: the same in float64
    eo      err(oracle, hp) [4][16];  ref: the reference error [4][16]
    hp_all  the truth's xs of all N tracks [N][12](n), for the lane check: a result that matches hp_all[i + 1] has been handed
            to the wrong track
    An oracle run that does not finish leaves inf in eo / ref (measures_something asserts finiteness: no track is left out)."""
    key = (family, n, m, mode)
    if key in _truth_cache:
        return _truth_cache[key]
    assert family in FAMILIES and mode in MODES, key
    ko = _oracle()
    M = ukf_hp.models(family, n, m)
    T, N, off = M["T"], M["N"], 0 if mode == "module" else 1
    F, Q = step_models(M["F"], M["Q"], T) if mode in ("class", "module") else (M["F"], M["Q"])
    Xs, Ps = np.empty((T - FROM, N, n)), np.empty((T - FROM, N, n, n))
    for i in range(N):
        zl = [M["zs"][t, i] if M["mask"][t] else None for t in range(T)]
        mu, cov = ko.kf_batch_filter(M["x0"][i], M["P0"][i], zl, F, Q, M["H"], M["R"])[:2]
        Xs[:, i], Ps[:, i] = mu[FROM:], 0.5 * (cov[FROM:] + np.swapaxes(cov[FROM:], -1, -2))
    if F.ndim == 3:
        F, Q = np.ascontiguousarray(F[FROM:]), np.ascontiguousarray(Q[FROM:])
    invs, memo = None, {}
    if mode == "given":                                           # Pp[k] is a function of the inputs alone
        invs = np.zeros_like(Ps)
        for i in range(N):
            for k in range(T - FROM - 1):
                invs[k, i] = _inv((ld(F) @ ld(Ps[k, i])) @ ld(F).T + ld(Q), memo).astype(np.float64)
    give = (lambda i: None) if invs is None else (lambda i: invs[:, i])
    hp_all = np.array([rts_smoother(Xs[:, i], Ps[:, i], F, Q, off, give(i), memo)[0] for i in range(N)])
    rs = np.random.RandomState(6007 * n + 37 * m + 5 * FAMILIES.index(family) + MODES.index(mode))
    hp, orc = [[] for _ in OUTPUTS], [[] for _ in OUTPUTS]
    ref = np.zeros((len(OUTPUTS), len(M["tracks"])))
    for k, trk in enumerate(M["tracks"]):
        h = rts_smoother(Xs[:, trk], Ps[:, trk], F, Q, off, give(trk), memo)
        o = _smooth(Xs[:, trk], Ps[:, trk], F, Q, mode, give(trk))
        for lst, v in zip(hp, h):
            lst.append(v)
        for lst, v in zip(orc, o if o is not None else [np.full(v.shape, np.inf) for v in h]):
            lst.append(v)
        runs = [o] + [_smooth(kf_hp.ulp(rs, Xs[:, trk]), kf_hp.ulp(rs, Ps[:, trk], True), kf_hp.ulp(rs, F), kf_hp.ulp(rs, Q, True),
                              mode, give(trk)) for _ in range(K_DRAWS)]
        for j, name in enumerate(OUTPUTS):
            c = _CUT[name]
            ref[j, k] = max(np.inf if r is None else err(r[j][c], h[j][c]) for r in runs)
    hp, orc = [np.array(v) for v in hp], [np.array(v, dtype=float) for v in orc]
    _truth_cache[key] = dict(model=M, Xs=Xs, Ps=Ps, F=F, Q=Q, invs=invs, off=off, hp=hp, oracle=orc, eo=errors(orc, hp), ref=ref,
                             hp_all=hp_all)
    return _truth_cache[key]


def measures_something(t):
    """the condition of every precision test: all 16 tracks finish in the oracle and in every perturbed run, err(oracle, hp) is
    finite and < 1e-3 on every output, and the inputs are what the module says (symmetric, the same for everybody)"""
    M = t["model"]
    assert len(M["tracks"]) == 16 == len(set(M["tracks"])) and set(ukf_hp.FIXED_TRACKS) <= set(M["tracks"])
    assert t["eo"].shape == t["ref"].shape == (len(OUTPUTS), 16)
    assert np.all(np.isfinite(t["eo"])) and np.all(np.isfinite(t["ref"])), (t["eo"].max(axis=1), t["ref"].max(axis=1))
    assert t["eo"].max() < 1e-3, t["eo"].max(axis=1)
    assert np.all(t["ref"] >= t["eo"])
    assert t["Xs"].shape == (M["T"] - FROM, M["N"], M["n"]) and np.array_equal(t["Ps"], np.swapaxes(t["Ps"], -1, -2))
    assert np.array_equal(t["hp"][0], t["hp_all"][list(M["tracks"])])


def check(label, eg, t, which=slice(None)):
    """ukf_hp.check with ref in place of the oracle's error, on the outputs `which`; nothing is excluded: every error of those
    outputs must be a number.  Prints one row per output; returns the failures."""
    names, eg, ref = OUTPUTS[which], np.asarray(eg)[which], t["ref"][which]
    assert eg.shape == ref.shape and not np.isnan(eg).any(), (label, eg)
    bad = []
    for j, name in enumerate(names):
        bad += ukf_hp.check(f"{label} {name}", eg[j:j + 1], ref[j:j + 1], MARGIN, FLOOR)
    return bad


def ratios(eg, t, which=slice(None)):
    """per output: (worst err / bar, build / oracle, ref / oracle), the last two as ratios of the worst track's errors"""
    rows = []
    for j in range(len(OUTPUTS))[which]:
        bar, mbar = max(MARGIN * t["ref"][j].max(), FLOOR), max(MARGIN * np.median(t["ref"][j]), FLOOR)
        eo = max(t["eo"][j].max(), 1e-300)
        rows.append((OUTPUTS[j], max(eg[j].max() / bar, np.median(eg[j]) / mbar), eg[j].max() / eo, t["ref"][j].max() / eo))
    return rows


def lanes(xs, t):
    """the lane check on ALL N tracks: (worst err(xs[i], hp_all[i]), least err(xs[i], hp_all[(i + 1) % N])).  Every track has its
    own x0 and measurements; a result within 1e-3 of its own truth and further than 1e-3 from its neighbour's is that track's.
    xs: [N][T](n)."""
    hp, N = t["hp_all"], len(t["hp_all"])
    assert len(xs) == N
    return (max(err(np.asarray(xs[i]), hp[i]) for i in range(N)),
            min(err(np.asarray(xs[i]), hp[(i + 1) % N]) for i in range(N)))
