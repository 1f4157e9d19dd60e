"""The reference's linear Kalman filter for ONE track in np.longdouble (80-bit on x86-64), written from the algorithm: predict
P = (F P) F' + Q (kalman_filter.py:472-478), the Joseph-form update (kalman_filter.py:533-556) with inv(S) from a longdouble
Cholesky factorisation (ukf_hp.spd_inv), batch_filter with missing measurements (kalman_filter.py:940-993) and the per-step K, S,
SI, y as filterpy.common.Saver records them (after a missing measurement y = 0 and K, S, SI keep their last values).

This is the truth tests/test_gpu_kf_precision.py and tests/test_host_kf_hp.py measure the forward kernels and the float64 oracle
(oracle/kf_oracle.py) against, on the model families of ukf_hp.models (their alpha / beta / kappa fields are not used).

The bar is not the oracle's error alone but the REFERENCE ERROR of a track and output:

    ref = max(err(oracle, hp), max over K_DRAWS draws of err(oracle on inputs perturbed by one ulp, hp))

with hp always the truth of the UNPERTURBED inputs: what a float64 implementation of this algorithm may lose on this model, by
its own rounding or by the conditioning of the problem (a last-bit change of x0, P0, z, F, Q, H, R; symmetric matrices stay
symmetric, as in tests/golden/make_rts_conditioning.py).  check() then holds a build to

    every checked track      err(build, hp) <= max(MARGIN * max_tracks ref, FLOOR)
    the median over tracks   median err(build, hp) <= max(MARGIN * median ref, FLOOR)

with the MARGIN = 8 of tests/test_gpu_ukf_precision.py and ukf_hp.FLOOR = 1e-13."""
import os
import sys

import numpy as np

import ukf_hp
from ukf_hp import LD, err, ld, spd_inv

MARGIN = 8.0
FLOOR = ukf_hp.FLOOR
K_DRAWS = 8
FAMILIES = ("benign", "stiff", "stiff_small_weights")
OUTPUTS = ("means", "covs", "means_p", "covs_p", "K", "S", "SI", "y")
FORWARD = slice(0, 4)                       # the four outputs of batch_filter
HISTORIES = slice(4, 8)                     # the by-products of the update, per step


# ------------------------------------------------------------------------------------------------------------ the truth
def predict(x, P, F, Q):
    return F @ x, (F @ P) @ F.T + Q


def update(x, P, z, H, R):
    """Joseph form -> x, P, K, S, SI, y"""
    y = z - H @ x
    PHT = P @ H.T
    S = H @ PHT + R
    SI = spd_inv(S)
    K = PHT @ SI
    I_KH = np.eye(x.size, dtype=LD) - K @ H
    return x + K @ y, (I_KH @ P) @ I_KH.T + (K @ R) @ K.T, K, S, SI, y


def batch_filter(x0, P0, zs, F, H, Q, R):
    """One track, predict first; a z that is None skips the update.  Returns the eight arrays of OUTPUTS, [T] each."""
    F, H, Q, R = map(ld, (F, H, Q, R))
    x, P = ld(x0).copy(), ld(P0).copy()
    T, n, m = len(zs), x.size, H.shape[0]
    out = [np.zeros((T,) + s, LD) for s in ((n,), (n, n), (n,), (n, n), (n, m), (m, m), (m, m), (m,))]
    K, S, SI = (np.zeros(s, LD) for s in ((n, m), (m, m), (m, m)))
    for t, z in enumerate(zs):
        x, P = predict(x, P, F, Q)
        out[2][t], out[3][t] = x, P
        y = np.zeros(m, LD)
        if z is not None:
            x, P, K, S, SI, y = update(x, P, ld(z), H, R)
        out[0][t], out[1][t], out[4][t], out[5][t], out[6][t], out[7][t] = x, P, K, S, SI, y
    return out


# ------------------------------------------------------------------------------------------------------- models and reference
def models(family, n, m):
    """ukf_hp.models: N = 150 tracks, T = 16, step 8 missing, every track its own x0 and measurements, 16 checked tracks"""
    assert family in FAMILIES, family
    return ukf_hp.models(family, n, m)


def ulp(rs, a, sym=False):
    """every element moved by -1, 0 or +1 ulp; a symmetric matrix stays symmetric"""
    a = np.array(a, dtype=float)
    s = rs.choice([-1.0, 0.0, 1.0], size=a.shape)
    if sym:
        s = np.triu(s) + np.swapaxes(np.triu(s, 1), -1, -2)
    return a + s * np.spacing(np.abs(a))


def _oracle(x0, P0, zl, F, H, Q, R):
    """oracle/kf_oracle.py's batch_filter in the order of OUTPUTS; None where float64 itself breaks down"""
    from oracle import kf_oracle
    try:
        mu, cov, mup, covp, Ks, ys, Ss, SIs = kf_oracle.kf_batch_filter(x0, P0, zl, F, Q, H, R, return_all=True)
    except np.linalg.LinAlgError:
        return None
    return [mu, cov, mup, covp, Ks, Ss, SIs, ys]


def errors(got, hp):
    """[outputs][tracks]: err of `got` (arrays [tracks][T]..., None where an output is not produced: NaN) against hp"""
    out = np.full((len(hp), len(hp[0])), np.nan)
    for j, g in enumerate(got):
        if g is not None:
            out[j] = [err(np.asarray(g[i]), hp[j][i]) for i in range(len(hp[j]))]
    return out


_truth_cache = {}


def truth(family, n, m, masked=True):
    """Computed once per key and shared, never modified.  For the 16 checked tracks:
    model   the ukf_hp.models dict (mask all ones where masked is False)
    hp      the eight longdouble outputs, [16][T]... each
    oracle  the same from oracle/kf_oracle.py (float64)
    eo      err(oracle, hp) [8][16]
    ref     the reference error [8][16]: max(eo, the K_DRAWS one-ulp draws' errors against the same hp)
    hp_next the longdouble posterior means of each checked track's NEIGHBOUR (i + 1) mod N: a result that matches those has
            been handed to the wrong track
    An oracle run that does not finish leaves inf in eo / ref (the tests assert finiteness: no track is ever left out)."""
    key = (family, n, m, masked)
    if key in _truth_cache:
        return _truth_cache[key]
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if root not in sys.path:
        sys.path.insert(0, root)
    M = dict(models(family, n, m))
    if not masked:
        M["mask"] = np.ones_like(M["mask"])
    F, H, Q, R, T, N = M["F"], M["H"], M["Q"], M["R"], M["T"], M["N"]
    rs = np.random.RandomState(7919 * n + 31 * m + FAMILIES.index(family))
    hp, orc, nxt = [[] for _ in OUTPUTS], [[] for _ in OUTPUTS], []
    ref = np.zeros((len(OUTPUTS), len(M["tracks"])))
    for k, trk in enumerate(M["tracks"]):
        zl = lambda zs: [zs[t] if M["mask"][t] else None for t in range(T)]  # noqa: E731
        h = batch_filter(M["x0"][trk], M["P0"][trk], zl(M["zs"][:, trk]), F, H, Q, R)
        o = _oracle(M["x0"][trk], M["P0"][trk], zl(M["zs"][:, trk]), F, H, Q, R)
        for lst, v in zip(hp, h):
            lst.append(v)
        for lst, v in zip(orc, o if o is not None else [np.full(v.shape, np.inf) for v in h]):
            lst.append(v)
        runs = [o] + [_oracle(ulp(rs, M["x0"][trk]), ulp(rs, M["P0"][trk], True), zl(ulp(rs, M["zs"][:, trk])), ulp(rs, F),
                              ulp(rs, H), ulp(rs, Q, True), ulp(rs, R, True)) for _ in range(K_DRAWS)]
        for j in range(len(OUTPUTS)):
            ref[j, k] = max(np.inf if r is None else err(r[j], h[j]) for r in runs)
        nb = (trk + 1) % N
        nxt.append(batch_filter(M["x0"][nb], M["P0"][nb], zl(M["zs"][:, nb]), F, H, Q, R)[0])
    hp, orc = [np.array(v) for v in hp], [np.array(v, dtype=float) for v in orc]
    _truth_cache[key] = dict(model=M, hp=hp, oracle=orc, eo=errors(orc, hp), ref=ref, hp_next=np.array(nxt))
    return _truth_cache[key]


def measures_something(t):
    """the condition of every precision test: all 16 tracks finish in the oracle (and in every perturbed run), and
    err(oracle, hp) is finite and < 1e-3 on every output"""
    M = t["model"]
    assert len(M["tracks"]) == 16 == len(set(M["tracks"])) and set(ukf_hp.FIXED_TRACKS) <= set(M["tracks"])
    assert t["eo"].shape == t["ref"].shape == (len(OUTPUTS), 16)
    assert np.all(np.isfinite(t["eo"])) and np.all(np.isfinite(t["ref"])), (t["eo"].max(axis=1), t["ref"].max(axis=1))
    assert t["eo"].max() < 1e-3, t["eo"].max(axis=1)
    assert np.all(t["ref"] >= t["eo"])


def check(label, eg, t, which=FORWARD):
    """ukf_hp.check with ref in place of the oracle's error, on the outputs `which`; nothing is excluded: every error of those
    outputs must be a number.  Prints one row per output; returns the failures."""
    names, eg, ref = OUTPUTS[which], np.asarray(eg)[which], t["ref"][which]
    assert eg.shape == ref.shape and not np.isnan(eg).any(), (label, eg)
    bad = []
    for j, name in enumerate(names):
        bad += ukf_hp.check(f"{label} {name}", eg[j:j + 1], ref[j:j + 1], MARGIN, FLOOR)
    return bad


def ratios(eg, t, which=FORWARD):
    """per output: (worst err / bar, build / oracle, ref / oracle), the last two as ratios of the worst track's errors"""
    rows = []
    for j in range(len(OUTPUTS))[which]:
        bar, mbar = max(MARGIN * t["ref"][j].max(), FLOOR), max(MARGIN * np.median(t["ref"][j]), FLOOR)
        eo = max(t["eo"][j].max(), 1e-300)
        rows.append((OUTPUTS[j], max(eg[j].max() / bar, np.median(eg[j]) / mbar), eg[j].max() / eo, t["ref"][j].max() / eo))
    return rows


def not_the_neighbour(got_means, t):
    """the lane-mix check: the posterior means a bank returns for checked track i are NOT those of track i + 1.  Every track has
    its own x0 and measurements, and the oracle is within 1e-3 of the truth on every track (measures_something), so a result
    further than 1e-3 from a track's truth is not that track's."""
    return min(err(np.asarray(got_means[i]), t["hp_next"][i]) for i in range(len(t["hp_next"]))) > 1e-3
