"""The reference's IMMEstimator and MMAEFilterBank for ONE track's bank in np.longdouble (80-bit on x86-64), written from the
algorithm on top of kf_hp.predict / kf_hp.update (the Joseph form, inv(S) from a longdouble Cholesky factorisation):

IMM   (IMM.py:160-249) mixing probabilities cbar = mu . M, omega[i, j] = M[i, j] mu[i] / cbar[j]; the mixed initial conditions,
      then every filter's own predict; the bank's prior estimate; every filter's update; its likelihood
      exp(-(m ln 2 pi + ln |S| + y' S^-1 y) / 2), ln |S| from the longdouble Cholesky factor and pi in longdouble; mu = cbar L,
      normalised; the posterior estimate.
MMAE  (mmae.py:140-207) no mixing, p *= L; the reference's own covariance loop: filter k is centred on the scalar x[k] and only
      the first min(dim_x, n_models) filters contribute (oracle/imm_oracle.py, mmae_batch).
A likelihood whose float64 value is 0 becomes DBL_MIN, as the reference does (kalman_filter.py:1221-1225).  A missing measurement
(z is None) leaves x and P untouched; the likelihood is then the density of a zero residual under the S of the last real update
(imm_oracle.imm_batch).

This is the truth tests/test_host_imm_hp.py and tests/test_gpu_imm_precision.py measure the IMM / MMAE kernels and the float64
oracle (oracle/imm_oracle.py) against.  The bar is that of kf_hp: the REFERENCE ERROR of a track and output,

    ref = max(err(oracle, hp), max over K_DRAWS draws of err(oracle on inputs perturbed by one ulp, hp))

(xs0, Ps0, zs, Fs, Qs, Hs, Rs perturbed, symmetric matrices kept symmetric; mu0 and M left alone: they sum to one), and
ukf_hp.check with MARGIN = 8 and FLOOR = 1e-13.  No number here is tuned to a kernel.

Banks (bank()): the models of ukf_hp.models(family, n, m) -- N = 150, T = 16, its 16 checked tracks -- spread into n_models
filters, F_j = F + c j diag(ones(n - 1), 1), Q_j = 10^j Q, R_j = (1 + j / 2) R, H_j = H; every track its own filter states
(x0[track] + 0.1 randn per filter), its own mu0, Ps0 = P0.  The measurements are SIMULATED: a true state started at
xs0[track, 0] + 0.3 randn and stepped with the model (t // 5) % n_models, its process and its measurement noise.  (The family's
own 10 randn measurements are hundreds of sigmas from every filter at R = 1e-4: every likelihood is floored, mu only repeats
cbar and nothing is measured.)  measures_something() asserts that a bank does measure: see there."""
import os
import sys

import numpy as np

import kf_hp
import ukf_hp
from ukf_hp import LD, err, ld

MARGIN = kf_hp.MARGIN
FLOOR = ukf_hp.FLOOR
K_DRAWS = 8
FAMILIES = kf_hp.FAMILIES
STIFF = ("stiff", "stiff_small_weights")
# per step [T]...: x, P, mu, x_prior, P_prior, L (MMAE has no priors); the bank's final state: the filters' xs [nm][n], Ps [nm][n][n]
# and the mode probabilities [1][nm]
OUTPUTS = ("x", "P", "mu", "x_prior", "P_prior", "L", "xs_final", "Ps_final", "mu_final")
PRIORS = (3, 4)
I_L = 5
DBL_MIN = sys.float_info.min
PI = LD("3.14159265358979323846264338327950288")
LOG_2PI = np.log(2 * PI)
# the likelihood's comparison: below L_FLOORED the truth is 0 in float64 and every implementation must return DBL_MIN exactly;
# in [L_FLOORED, L_SUBNORMAL] (float64's subnormal range and its neighbourhood) the flooring decision or the last bits may
# legitimately differ: such an entry is left out of the likelihood's comparison (and of nothing else)
L_FLOORED, L_SUBNORMAL, MAX_LEFT_OUT = LD("1e-330"), LD("1e-290"), 0.01

# What was changed to make a named bank meet measures_something (seed shift, c): nothing so far for the banks not listed.
SEED_SHIFT = {}
C_SPREAD = {}


# ------------------------------------------------------------------------------------------------------------ the truth
def likelihood(y, S):
    """exp(logpdf(y; 0, S)) -> (the value the reference would hold: floored at DBL_MIN, the unfloored value)"""
    U = ukf_hp.chol_upper(S)
    m = y.size
    w = np.zeros(m, LD)                                        # U' w = y
    for i in range(m):
        w[i] = (y[i] - U[:i, i] @ w[:i]) / U[i, i]
    raw = np.exp(-(m * LOG_2PI + 2 * np.sum(np.log(np.diag(U))) + w @ w) / 2)
    return (LD(DBL_MIN) if float(raw) == 0.0 else raw), raw


def estimate(xs, Ps, mu):
    x = sum(m * xj for xj, m in zip(xs, mu))
    P = sum(m * (np.outer(xj - x, xj - x) + Pj) for xj, Pj, m in zip(xs, Ps, mu))
    return x, P


def _update_bank(xs, Ps, z, Hs, Rs, S_last):
    nm, m = len(xs), Hs[0].shape[0]
    L, raw = np.zeros(nm, LD), np.zeros(nm, LD)
    for j in range(nm):
        if z is None:
            y, S = np.zeros(m, LD), S_last[j]
        else:
            xs[j], Ps[j], _, S, _, y = kf_hp.update(xs[j], Ps[j], z, Hs[j], Rs[j])
            S_last[j] = S
        L[j], raw[j] = (LD(DBL_MIN), LD(0)) if S is None else likelihood(y, S)   # (before any update the density is 0: floored)
    return L, raw


def imm_batch(xs0, Ps0, mu0, M, zs, Fs, Qs, Hs, Rs):
    """One bank, T x { predict; update(z or None) } -> the nine arrays of OUTPUTS and the unfloored likelihoods [T][nm]"""
    Fs, Qs, Hs, Rs = ([ld(a) for a in v] for v in (Fs, Qs, Hs, Rs))
    M = ld(M)
    xs, Ps = [ld(x).copy() for x in xs0], [ld(P).copy() for P in Ps0]
    mu = ld(mu0) / np.sum(ld(mu0))
    nm, T, n = len(Fs), len(zs), xs[0].size
    out = [np.zeros((T,) + s, LD) for s in ((n,), (n, n), (nm,), (n,), (n, n), (nm,))]
    raws, S_last = np.zeros((T, nm), LD), [None] * nm
    for t, z in enumerate(zs):
        cbar = mu @ M
        omega = M * mu[:, None] / cbar[None, :]
        mixed = [estimate(xs, Ps, omega[:, j]) for j in range(nm)]
        for j in range(nm):
            xs[j], Ps[j] = kf_hp.predict(mixed[j][0], mixed[j][1], Fs[j], Qs[j])
        out[3][t], out[4][t] = estimate(xs, Ps, mu)
        L, raws[t] = _update_bank(xs, Ps, None if z is None else ld(z), Hs, Rs, S_last)
        mu = cbar * L
        mu = mu / np.sum(mu)
        out[0][t], out[1][t] = estimate(xs, Ps, mu)
        out[2][t], out[5][t] = mu, L
    return out + [np.array(xs), np.array(Ps), mu[None], raws]


def mmae_batch(xs0, Ps0, p0, zs, Fs, Qs, Hs, Rs):
    """-> the nine arrays of OUTPUTS (None: the priors) and the unfloored likelihoods [T][nm]"""
    Fs, Qs, Hs, Rs = ([ld(a) for a in v] for v in (Fs, Qs, Hs, Rs))
    xs, Ps = [ld(x).copy() for x in xs0], [ld(P).copy() for P in Ps0]
    p = ld(p0).copy()
    nm, T, n = len(Fs), len(zs), xs[0].size
    out = [np.zeros((T,) + s, LD) for s in ((n,), (n, n), (nm,), (n,), (n, n), (nm,))]
    raws, S_last = np.zeros((T, nm), LD), [None] * nm
    for t, z in enumerate(zs):
        for j in range(nm):
            xs[j], Ps[j] = kf_hp.predict(xs[j], Ps[j], Fs[j], Qs[j])
        L, raws[t] = _update_bank(xs, Ps, None if z is None else ld(z), Hs, Rs, S_last)
        p = p * L
        p = p / np.sum(p)
        x = sum(pj * xj for xj, pj in zip(xs, p))
        P = np.zeros((n, n), LD)
        for xk, xj, Pj, pj in zip(x, xs, Ps, p):                # mmae.py:205-207, as written
            P = P + pj * (np.outer(xj - xk, xj - xk) + Pj)
        out[0][t], out[1][t], out[2][t], out[5][t] = x, P, p, L
    out[3] = out[4] = None
    return out + [np.array(xs), np.array(Ps), p[None], raws]


# --------------------------------------------------------------------------------------------------------------- banks
def _noise(rs, C):
    return np.linalg.cholesky(C) @ rs.randn(C.shape[0])


def bank(family, n, m, nm, masked=False):
    """-> dict: Fs Qs Hs Rs [nm]..., M, xs0 [N][nm][n], Ps0 [N][nm][n][n], mu0 [N][nm], zs [T][N][m], mask [T] (all ones unless
    masked: then step ukf_hp.T_MISSING is missing on every track), tracks, n m nm N T"""
    assert family in FAMILIES, family
    B = ukf_hp.models(family, n, m)
    key = (family, n, m, nm)
    c = C_SPREAD.get(key, 0.004 if family in STIFF else 0.02)
    rs = np.random.RandomState(104729 * FAMILIES.index(family) + 7919 * n + 31 * m + nm + SEED_SHIFT.get(key, 0))
    N, T = B["N"], B["T"]
    Fs = np.array([B["F"] + c * j * np.diag(np.ones(n - 1), 1) for j in range(nm)])
    Qs = np.array([10.0 ** j * B["Q"] for j in range(nm)])
    Rs = np.array([(1 + 0.5 * j) * B["R"] for j in range(nm)])
    Hs = np.array([B["H"]] * nm)
    M = rs.rand(nm, nm) + 2 * np.eye(nm)
    M /= M.sum(axis=1, keepdims=True)
    xs0 = B["x0"][:, None, :] + 0.1 * rs.randn(N, nm, n)
    mu0 = rs.rand(N, nm) + 0.1
    mu0 /= mu0.sum(axis=1, keepdims=True)
    Ps0 = np.ascontiguousarray(np.repeat(B["P0"][:, None], nm, axis=1))
    zs = np.zeros((T, N, m))
    for trk in range(N):
        x = xs0[trk, 0] + 0.3 * rs.randn(n)
        for t in range(T):
            j = (t // 5) % nm
            x = Fs[j] @ x + _noise(rs, Qs[j])
            zs[t, trk] = Hs[j] @ x + _noise(rs, Rs[j])
    mask = B["mask"].copy() if masked else np.ones(T, dtype=np.uint8)
    return dict(Fs=Fs, Qs=Qs, Hs=Hs, Rs=Rs, M=M, xs0=xs0, Ps0=Ps0, mu0=mu0, zs=zs, mask=mask, tracks=B["tracks"],
                n=n, m=m, nm=nm, N=N, T=T, family=family, c=c)


# ----------------------------------------------------------------------------------------------------- the reference error
def ulp(rs, a, sym=False):
    return kf_hp.ulp(rs, a, sym)


def _oracle(kind, xs0, Ps0, mu0, M, zl, Fs, Qs, Hs, Rs):
    """oracle/imm_oracle.py in the order of OUTPUTS (None for MMAE's priors); None where float64 itself breaks down"""
    from oracle import imm_oracle
    try:
        with np.errstate(all="ignore"):
            if kind == "mmae":
                x, P, p, L, xs, Ps = imm_oracle.mmae_batch(xs0, Ps0, mu0, zl, Fs, Qs, Hs, Rs, return_state=True)
                return [x, P, p, None, None, L, xs, Ps, p[-1:]]
            o = list(imm_oracle.imm_batch(xs0, Ps0, mu0, M, zl, Fs, Qs, Hs, Rs, return_state=True))
            return o + [o[2][-1:]]
    except (np.linalg.LinAlgError, ValueError):
        return None


def likelihood_view(L, raw):
    """the likelihood's comparison (above) -> (L with the left-out entries replaced by the truth's, so that they count as
    exact; how many were left out; whether every entry whose truth is below L_FLOORED is DBL_MIN exactly)"""
    L = np.asarray(L, dtype=float)
    below, mid = raw < L_FLOORED, (raw >= L_FLOORED) & (raw <= L_SUBNORMAL)
    out = ld(L).copy()
    out[mid] = raw[mid]
    return out, int(mid.sum()), bool(np.all(L[below] == DBL_MIN))


def one_errors(got, hp, raw):
    """one track: err per output of `got` (None where an output is not produced: NaN) -> (errors [len(OUTPUTS)], floor kept)"""
    e, ok = np.full(len(OUTPUTS), np.nan), True
    for j, g in enumerate(got):
        if g is None or hp[j] is None:
            continue
        if j == I_L:
            g, _, ok = likelihood_view(g, raw)
        e[j] = err(np.asarray(g), hp[j])
    return e, ok


def errors(got, t):
    """[outputs][tracks] of `got` (per output an array [16 tracks]..., or None) against a truth -> (errors, floor kept on
    every track)"""
    out, ok = np.full((len(OUTPUTS), len(t["raw"])), np.nan), True
    for i in range(len(t["raw"])):
        out[:, i], k = one_errors([None if g is None else g[i] for g in got], [None if h is None else h[i] for h in t["hp"]],
                                  t["raw"][i])
        ok = ok and k
    return out, ok


_truth_cache = {}


def truth(kind, family, n, m, nm, masked=False):
    """Computed once per key and shared (the layouts share it), never modified.  For the 16 checked tracks:
    model    the bank() dict
    hp       the longdouble outputs in the order of OUTPUTS, [16]... each (None: MMAE's priors); raw: the unfloored likelihoods
    oracle   the same from oracle/imm_oracle.py (float64)
    eo, ref  err(oracle, hp) and the reference error, [len(OUTPUTS)][16] (NaN rows: MMAE's priors); inf where an oracle run
             did not finish
    floor_ok whether the oracle and all its perturbed runs return DBL_MIN where the truth is below L_FLOORED
    hp_next  the longdouble posterior x of each checked track's NEIGHBOUR (i + 1) mod N"""
    key = (kind, family, n, m, nm, masked)
    if key in _truth_cache:
        return _truth_cache[key]
    assert kind in ("imm", "mmae"), kind
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if root not in sys.path:
        sys.path.insert(0, root)
    B = bank(family, n, m, nm, masked)
    Fs, Qs, Hs, Rs, M, T, N = B["Fs"], B["Qs"], B["Hs"], B["Rs"], B["M"], B["T"], B["N"]
    rs = np.random.RandomState(15485863 + 7919 * n + 31 * m + nm + 97 * FAMILIES.index(family))
    zl = lambda zs: [zs[t] if B["mask"][t] else None for t in range(T)]  # noqa: E731
    run = (lambda *a: mmae_batch(a[0], a[1], a[2], *a[4:])) if kind == "mmae" else imm_batch
    hp, orc, raws, nxt = [[] for _ in OUTPUTS], [[] for _ in OUTPUTS], [], []
    eo, ref = (np.full((len(OUTPUTS), len(B["tracks"])), np.nan) for _ in range(2))
    floor_ok = True
    for k, trk in enumerate(B["tracks"]):
        h = run(B["xs0"][trk], B["Ps0"][trk], B["mu0"][trk], M, zl(B["zs"][:, trk]), Fs, Qs, Hs, Rs)
        h, raw = h[:-1], h[-1]
        raws.append(raw)
        o = _oracle(kind, B["xs0"][trk], B["Ps0"][trk], B["mu0"][trk], M, zl(B["zs"][:, trk]), Fs, Qs, Hs, Rs)
        runs = [o] + [_oracle(kind, ulp(rs, B["xs0"][trk]), ulp(rs, B["Ps0"][trk], True), B["mu0"][trk], M,
                              zl(ulp(rs, B["zs"][:, trk])), ulp(rs, Fs), ulp(rs, Qs, True), ulp(rs, Hs), ulp(rs, Rs, True))
                      for _ in range(K_DRAWS)]
        es = []
        for r in runs:
            if r is None:
                es.append(np.where(np.array([v is None for v in h]), np.nan, np.inf))
            else:
                e, ok = one_errors(r, h, raw)
                floor_ok = floor_ok and ok
                es.append(e)
        eo[:, k], ref[:, k] = es[0], np.max(es, axis=0)
        for lst, v in zip(hp, h):
            lst.append(v)
        for lst, v, w in zip(orc, o if o is not None else [None] * len(h), h):
            lst.append(None if w is None else (np.full(w.shape, np.inf) if v is None else v))
        nb = (trk + 1) % N
        nxt.append(run(B["xs0"][nb], B["Ps0"][nb], B["mu0"][nb], M, zl(B["zs"][:, nb]), Fs, Qs, Hs, Rs)[0])
    arr = lambda lst, dt: None if lst[0] is None else np.array(lst, dtype=dt)  # noqa: E731
    _truth_cache[key] = dict(kind=kind, model=B, hp=[arr(v, LD) for v in hp], raw=np.array(raws), oracle=[arr(v, float) for v in orc],
                             eo=eo, ref=ref, floor_ok=floor_ok, hp_next=np.array(nxt))
    return _truth_cache[key]


def produced(t):
    """the rows of OUTPUTS this kind produces"""
    return [j for j in range(len(OUTPUTS)) if not (t["kind"] == "mmae" and j in PRIORS)]


def measures_something(t):
    """The condition of every precision test, asserted before any kernel result is looked at:
    * every oracle run finishes, the perturbed ones included: eo and ref are finite, and eo < 1e-3 on every output;
    * the floor: where the truth's likelihood is below 1e-330 the oracle returns DBL_MIN exactly; at most 1 % of the bank's checked
      likelihood entries lie in [1e-330, 1e-290] and are left out of the likelihood's comparison;
    * the best model's true likelihood is above 1e-100 at every checked step;
    * the second-largest true mode probability exceeds 1e-3 in at least a quarter of the checked (track, step) pairs: the mixing
      and the mu-weighted moments are in the measurement."""
    B, rows = t["model"], produced(t)
    assert len(B["tracks"]) == 16 == len(set(B["tracks"])) and set(ukf_hp.FIXED_TRACKS) <= set(B["tracks"])
    eo, ref = t["eo"][rows], t["ref"][rows]
    assert np.all(np.isfinite(eo)) and np.all(np.isfinite(ref)), (eo.max(axis=1), ref.max(axis=1))
    assert eo.max() < 1e-3, eo.max(axis=1)
    assert np.all(ref >= eo)
    assert t["floor_ok"]
    raw = t["raw"]
    left_out = int(((raw >= L_FLOORED) & (raw <= L_SUBNORMAL)).sum())
    assert left_out <= MAX_LEFT_OUT * raw.size, (left_out, raw.size)
    assert raw.max(axis=-1).min() > 1e-100, raw.max(axis=-1).min()
    second = np.sort(t["hp"][2], axis=-1)[..., -2]
    assert (second > 1e-3).mean() >= 0.25, (second > 1e-3).mean()


def stats(t):
    """what measures_something looks at, as numbers: left-out likelihood entries, entries in all, the worst best-model
    likelihood, the share of (track, step) pairs whose second mode probability exceeds 1e-3"""
    raw = t["raw"]
    return (int(((raw >= L_FLOORED) & (raw <= L_SUBNORMAL)).sum()), raw.size, float(raw.max(axis=-1).min()),
            float((np.sort(t["hp"][2], axis=-1)[..., -2] > 1e-3).mean()))


def check(label, eg, t):
    """ukf_hp.check with ref in place of the oracle's error, one row per produced output; every error of those must be a number.
    Returns the failures."""
    rows = produced(t)
    eg = np.asarray(eg)
    assert eg.shape == t["ref"].shape and not np.isnan(eg[rows]).any(), (label, eg)
    bad = []
    for j in rows:
        bad += ukf_hp.check(f"{label} {OUTPUTS[j]}", eg[j:j + 1], t["ref"][j:j + 1], MARGIN, FLOOR)
    return bad


def ratios(eg, t):
    """per produced output: (name, worst err / bar, worst oracle error, worst ref, worst build error)"""
    rows = []
    for j in produced(t):
        bar, mbar = max(MARGIN * t["ref"][j].max(), FLOOR), max(MARGIN * np.median(t["ref"][j]), FLOOR)
        rows.append((OUTPUTS[j], max(eg[j].max() / bar, np.median(eg[j]) / mbar), t["eo"][j].max(), t["ref"][j].max(), eg[j].max()))
    return rows


def not_the_neighbour(got_x, t):
    """kf_hp.not_the_neighbour on the posterior x: what a bank returns for checked track i is further than 1e-3 from the truth
    of track i + 1 (every track has its own filter states and measurements; the oracle is within 1e-3 of the truth)"""
    return min(err(np.asarray(got_x[i]), t["hp_next"][i]) for i in range(len(t["hp_next"]))) > 1e-3
