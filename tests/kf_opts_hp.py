"""The options and variants of the reference's linear Kalman filter for ONE track in np.longdouble, written from the algorithm,
beside tests/kf_hp.py (the plain forward call) and with its bar unchanged:

  batch_filter with options (kalman_filter.py:472-478, 940-993): per-step Fs / Qs / Hs / Rs / Bs, a control input (x = F x + B u
      only when both B and u are given), alpha_sq (P = alpha_sq ((F P) F') + Q) and update_first (update -> store the posterior
      -> predict -> store the prior), with the per-step K, S, SI, y, log_likelihood and mahalanobis:
      ll = -1/2 (m log 2 pi + log det S + y' SI y) with log det from the longdouble Cholesky factor, maha = sqrt(y' SI y); at a
      missing step y = 0 and S, SI are kept (the reference's lazy properties after update(None))
  update_correlated (kalman_filter.py:727-748, the reference's association order; the non-Joseph P = P - K (H P + M')), as a
      recursion of T_CORR = 12 x {predict; update_correlated} and as single updates on the plain truth's priors
  the steady-state pair (kalman_filter.py:563-668): means, means_p and y with a fixed gain

truth_opts / truth_corr / truth_steady are built exactly as kf_hp.truth builds `ref`: the 16 checked tracks of ukf_hp.models, the
float64 oracle (oracle/kf_oracle.py) on the given inputs and on K_DRAWS = 8 copies perturbed by one ulp (B, us, M and K too;
symmetric matrices stay symmetric), ref = the worst of those against the truth of the UNPERTURBED inputs, and hp_next for the
lane-mix check.  Each is computed once per key, shared and never modified.

The inputs come from a fixed RandomState per (n, m) on top of kf_hp.models(family, n, m): B = randn(n, nu), us = 10 randn(T, N, nu)
(every track its own), per-step models Fs = F + 0.01 randn, Hs = H + 0.05 randn, Qs = Q 10^U(-.5,.5), Rs = R 10^U(-.5,.5),
Bs = B + 0.05 randn, different at every step, and ALPHA_SQ = 1.05.  `mutate` recomputes a truth with one deliberate mistake, the
characteristic ones of the kernels (tests/test_host_kf_options_hp.py shows that each sits above the bar)."""
import os
import sys
from collections import namedtuple

import numpy as np

import kf_hp
import ukf_hp
from kf_hp import FAMILIES, FLOOR, K_DRAWS, MARGIN, ulp
from ukf_hp import LD, chol_upper, err, ld, spd_inv

ALPHA_SQ = 1.05
NU_MAX = 5
T_CORR = 12
SINGLE_STEPS = (0, 12)
OUTPUTS = kf_hp.OUTPUTS + ("ll", "maha")
FORWARD = OUTPUTS[:4]
CORR_OUTPUTS = ("x", "P", "K", "S", "SI", "y")
STEADY_OUTPUTS = ("means", "means_p", "y")
SCALARS = ("ll", "maha")
LOG_2PI = np.log(LD(8) * np.arctan(LD(1)))

Opt = namedtuple("Opt", "nu per_step alpha_sq update_first masked", defaults=(0, False, 1.0, False, True))
PLAIN = Opt()


def _root_on_path():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if root not in sys.path:
        sys.path.insert(0, root)


# ------------------------------------------------------------------------------------------------------------ the truth
def log_likelihood(y, S, SI):
    U = chol_upper(S)
    return -(S.shape[0] * LOG_2PI + 2 * np.sum(np.log(np.diag(U))) + y @ SI @ y) / 2


def mahalanobis(y, SI):
    return np.sqrt(y @ SI @ y)


def batch_filter(x0, P0, zs, Fs, Hs, Qs, Rs, Bs=None, us=None, alpha_sq=1.0, update_first=False, mutate=None):
    """One track; Fs, Hs, Qs, Rs (and Bs) are one matrix or [T] of them; a z that is None skips the update.  Returns the ten
    arrays of OUTPUTS, [T] each.  mutate: None, or the one deliberate mistake "model_next" (model t + 1 used at step t),
    "B_prev" (Bs[t - 1] with us[t]), "alpha_Q" (alpha applied to Q too), "prior_early" (update_first: the prior stored before the
    predict)."""
    T = len(zs)
    per = lambda a: None if a is None else (ld(a) if np.ndim(a) == 3 else [ld(a)] * T)  # noqa: E731
    Fs, Hs, Qs, Rs, Bs = map(per, (Fs, Hs, Qs, Rs, Bs))
    x, P = ld(x0).copy(), ld(P0).copy()
    n, m, a2 = x.size, Hs[0].shape[0], LD(alpha_sq)
    out = [np.zeros((T,) + s, LD) for s in ((n,), (n, n), (n,), (n, n), (n, m), (m, m), (m, m), (m,), (), ())]
    last = [np.zeros(s, LD) for s in ((n, m), (m, m), (m, m))]

    def do_predict(t):
        nonlocal x, P
        k = min(t + 1, T - 1) if mutate == "model_next" else t
        xn = Fs[k] @ x
        if Bs is not None and us is not None:
            xn = xn + Bs[max(k - 1, 0) if mutate == "B_prev" else k] @ ld(us[t])
        Q = a2 * Qs[k] if mutate == "alpha_Q" else Qs[k]
        x, P = xn, a2 * ((Fs[k] @ P) @ Fs[k].T) + Q
        out[2][t], out[3][t] = x, P

    def do_update(t):
        nonlocal x, P
        k = min(t + 1, T - 1) if mutate == "model_next" else t
        y = np.zeros(m, LD)
        if zs[t] is not None:
            x, P, K, S, SI, y = kf_hp.update(x, P, ld(zs[t]), Hs[k], Rs[k])
            last[:] = [K, S, SI]
        out[0][t], out[1][t], out[7][t] = x, P, y
        out[4][t], out[5][t], out[6][t] = last
        out[8][t], out[9][t] = log_likelihood(y, last[1], last[2]), mahalanobis(y, last[2])

    for t in range(T):
        if update_first:
            do_update(t)
            do_predict(t)
            if mutate == "prior_early":
                out[2][t], out[3][t] = out[0][t], out[1][t]
        else:
            do_predict(t)
            do_update(t)
    return out


def update_correlated(x, P, z, H, R, M, mutate=None):
    """-> x, P, K, S, SI, y.  mutate "drop_Mt": M' left out of H P + M'"""
    y = z - H @ x
    PHT = P @ H.T
    S = H @ PHT + H @ M + M.T @ H.T + R
    SI = spd_inv(S)
    K = (PHT + M) @ SI
    HP = H @ P if mutate == "drop_Mt" else H @ P + M.T
    return x + K @ y, P - K @ HP, K, S, SI, y


def corr_recursion(x0, P0, zs, F, H, Q, R, M, mutate=None):
    """[steps] of each of CORR_OUTPUTS; a mistaken recursion (mutate) that loses positive definiteness ends at that step and
    returns the steps before it"""
    F, H, Q, R, M = map(ld, (F, H, Q, R, M))
    x, P = ld(x0).copy(), ld(P0).copy()
    out = [[] for _ in CORR_OUTPUTS]
    for z in zs:
        x, P = F @ x, (F @ P) @ F.T + Q
        try:
            res = update_correlated(x, P, ld(z), H, R, M, mutate)
        except np.linalg.LinAlgError:
            if mutate is None:
                raise
            break
        x, P = res[0], res[1]
        for lst, v in zip(out, res):
            lst.append(v)
    return [np.array(v) for v in out]


def corr_singles(xs, Ps, zs, H, R, M, mutate=None, joseph=False):
    """one update on each prior; joseph: the plain Joseph-form update (kf_hp.update, M not used)"""
    H, R, M = map(ld, (H, R, M))
    res = [kf_hp.update(ld(x), ld(P), ld(z), H, R) if joseph else update_correlated(ld(x), ld(P), ld(z), H, R, M, mutate)
           for x, P, z in zip(xs, Ps, zs)]
    return [np.array([r[j] for r in res]) for j in range(len(CORR_OUTPUTS))]


def steadystate_filter(x0, zs, F, H, K, B=None, us=None):
    F, H, K = map(ld, (F, H, K))
    x, T = ld(x0).copy(), len(zs)
    out = [np.zeros((T, x.size), LD), np.zeros((T, x.size), LD), np.zeros((T, H.shape[0]), LD)]
    for t, z in enumerate(zs):
        x = F @ x + ld(B) @ ld(us[t]) if B is not None and us is not None else F @ x
        out[1][t] = x
        if z is not None:
            out[2][t] = ld(z) - H @ x
            x = x + K @ out[2][t]
        out[0][t] = x
    return out


# ------------------------------------------------------------------------------------------------------------ the inputs
_input_cache = {}


def inputs(family, n, m):
    """what the options add to kf_hp.models(family, n, m), from one fixed RandomState per (n, m): B, us at NU_MAX columns (an
    option set takes the first nu), the per-step models, G of spectral norm 1 and the per-track scale of M"""
    key = (family, n, m)
    if key not in _input_cache:
        M = kf_hp.models(family, n, m)
        rs = np.random.RandomState(50000 + 100 * n + m)
        T, N = M["T"], M["N"]
        B, us = rs.randn(n, NU_MAX), 10 * rs.randn(T, N, NU_MAX)
        Fs, Hs = M["F"] + 0.01 * rs.randn(T, n, n), M["H"] + 0.05 * rs.randn(T, m, n)
        Qs = M["Q"] * 10.0 ** rs.uniform(-.5, .5, (T, 1, 1))
        Rs = M["R"] * 10.0 ** rs.uniform(-.5, .5, (T, 1, 1))
        Bs = B + 0.05 * rs.randn(T, n, NU_MAX)
        G = rs.randn(n, m)
        G /= np.linalg.norm(G, 2)
        Mc = 0.5 * np.linalg.cholesky(M["Q"]) @ G @ np.linalg.cholesky(M["R"]).T
        _input_cache[key] = dict(B=B, us=us, Fs=Fs, Hs=Hs, Qs=Qs, Rs=Rs, Bs=Bs, Mc=Mc, Mscale=1 + 0.1 * rs.rand(N))
    return _input_cache[key]


def bank_models(family, n, m, o):
    """the bank's inputs of one option set: F H Q R ((a,b) or (T,a,b)), B, us (None without control), mask [T]"""
    M, I = kf_hp.models(family, n, m), inputs(family, n, m)
    F, H, Q, R = (I["Fs"], I["Hs"], I["Qs"], I["Rs"]) if o.per_step else (M["F"], M["H"], M["Q"], M["R"])
    B = us = None
    if o.nu:
        B, us = (I["Bs"] if o.per_step else I["B"])[..., :o.nu].copy(), I["us"][..., :o.nu].copy()
    return dict(F=F, H=H, Q=Q, R=R, B=B, us=us, mask=M["mask"] if o.masked else np.ones_like(M["mask"]))


def errors(got, hp, names):
    """[outputs][tracks]: ukf_hp.err (normwise per step, the worst step) of `got` against hp; the two scalars ll and maha as
    |got - hp| / max(1, |hp|), the worst step.  An output that is None stays NaN."""
    out = np.full((len(names), len(hp[0])), np.nan)
    for j, g in enumerate(got):
        if g is None:
            continue
        for i in range(len(hp[j])):
            if names[j] in SCALARS:
                out[j, i] = float(np.max(np.abs(ld(g[i]) - hp[j][i]) / np.maximum(1, np.abs(hp[j][i]))))
            else:
                out[j, i] = err(np.asarray(g[i]), hp[j][i])
    return out


def _ulp_list(rs, a, sym=False):
    return None if a is None else ulp(rs, a, sym)


# ------------------------------------------------------------------------------------------- batch_filter with options
def _oracle_opts(x0, P0, zl, B, o):
    from oracle import kf_oracle
    try:
        mu, cov, mup, covp, Ks, ys, Ss, SIs = kf_oracle.kf_batch_filter(
            x0, P0, zl, B["F"], B["Q"], B["H"], B["R"], B=B["B"], us=B["u"], alpha_sq=o.alpha_sq,
            update_first=o.update_first, return_all=True)
        ll = np.array([kf_oracle.log_likelihood(y, S) for y, S in zip(ys, Ss)])
        mh = np.array([kf_oracle.mahalanobis(y, SI) for y, SI in zip(ys, SIs)])
    except (np.linalg.LinAlgError, ValueError):
        return None
    return [mu, cov, mup, covp, Ks, Ss, SIs, ys, ll, mh]


_truth_cache = {}


def truth_opts(family, n, m, o=PLAIN, mutate=None):
    """kf_hp.truth for one option set `o` (an Opt): model, inputs (bank_models), hp, oracle, eo, ref [10][16], hp_next.  With
    `mutate` only hp is the mistaken truth, measured by the caller against the cached one."""
    key = (family, n, m, o, mutate)
    if key in _truth_cache:
        return _truth_cache[key]
    _root_on_path()
    M, bm = dict(kf_hp.models(family, n, m)), bank_models(family, n, m, o)
    M["mask"] = bm["mask"]
    T, N = M["T"], M["N"]
    rs = np.random.RandomState(7919 * n + 31 * m + FAMILIES.index(family) + 1000003)
    zl = lambda zs: [zs[t] if M["mask"][t] else None for t in range(T)]  # noqa: E731

    def hp_of(trk):
        return batch_filter(M["x0"][trk], M["P0"][trk], zl(M["zs"][:, trk]), bm["F"], bm["H"], bm["Q"], bm["R"], bm["B"],
                            None if bm["us"] is None else bm["us"][:, trk], o.alpha_sq, o.update_first, mutate)

    hp = [np.array(v) for v in zip(*[hp_of(trk) for trk in M["tracks"]])]
    if mutate is not None:
        _truth_cache[key] = dict(model=M, inputs=bm, hp=hp)
        return _truth_cache[key]
    orc, ref = [[] for _ in OUTPUTS], np.zeros((len(OUTPUTS), len(M["tracks"])))
    sym = dict(Q=True, R=True)
    for k, trk in enumerate(M["tracks"]):
        u = None if bm["us"] is None else bm["us"][:, trk]
        runs = [_oracle_opts(M["x0"][trk], M["P0"][trk], zl(M["zs"][:, trk]), dict(bm, u=u), o)]
        for _ in range(K_DRAWS):
            pm = {k2: _ulp_list(rs, bm[k2], sym.get(k2, False)) for k2 in ("F", "H", "Q", "R", "B")}
            pm["u"] = _ulp_list(rs, u)
            runs.append(_oracle_opts(ulp(rs, M["x0"][trk]), ulp(rs, M["P0"][trk], True), zl(ulp(rs, M["zs"][:, trk])), pm, o))
        h = [v[k] for v in hp]
        for lst, v in zip(orc, runs[0] if runs[0] is not None else [np.full(v.shape, np.inf) for v in h]):
            lst.append(v)
        for j in range(len(OUTPUTS)):
            ref[j, k] = max(np.inf if r is None else errors([r[j][None]], [h[j][None]], OUTPUTS[j:j + 1])[0, 0] for r in runs)
    orc = [np.array(v, dtype=float) for v in orc]
    nxt = np.array([hp_of((trk + 1) % N)[0] for trk in M["tracks"]])
    _truth_cache[key] = dict(model=M, inputs=bm, outputs=OUTPUTS, hp=hp, oracle=orc, eo=errors(orc, hp, OUTPUTS), ref=ref,
                             hp_next=nxt)
    return _truth_cache[key]


# ------------------------------------------------------------------------------- banks of priors and gains for the variants
_bank_cache = {}


def oracle_bank(family, n, m):
    """the plain masked filter of ALL N tracks in float64 (oracle), the checked tracks' values replaced by the float64 rounding of
    the longdouble truth's: priors x [T][N][n], P [T][N][n][n] (symmetrised after the rounding: a packed kernel reads one
    triangle) and gains K [T][N][n][m] -- the inputs of the single correlated updates and of the steady-state filters"""
    key = (family, n, m)
    if key not in _bank_cache:
        _root_on_path()
        from oracle import kf_oracle
        t = kf_hp.truth(family, n, m)
        M = t["model"]
        T, N = M["T"], M["N"]
        xp, Pp, K = np.zeros((T, N, n)), np.zeros((T, N, n, n)), np.zeros((T, N, n, m))
        for i in range(N):
            zl = [M["zs"][s, i] if M["mask"][s] else None for s in range(T)]
            r = kf_oracle.kf_batch_filter(M["x0"][i], M["P0"][i], zl, M["F"], M["Q"], M["H"], M["R"], return_all=True)
            xp[:, i], Pp[:, i], K[:, i] = r[2], r[3], r[4]
        for k, trk in enumerate(M["tracks"]):
            xp[:, trk], Pp[:, trk], K[:, trk] = (t["hp"][j][k].astype(np.float64) for j in (2, 3, 4))
        _bank_cache[key] = dict(xp=xp, Pp=(Pp + np.swapaxes(Pp, -1, -2)) / 2, K=K)
    return _bank_cache[key]


def _finish(M, names, hp, runs_of, nxt):
    """oracle / eo / ref of a variant from runs_of(k, trk, draw) (draw 0: the given inputs; None where float64 breaks down)"""
    orc, ref = [[] for _ in names], np.zeros((len(names), len(M["tracks"])))
    for k, trk in enumerate(M["tracks"]):
        runs = [runs_of(k, trk, d) for d in range(K_DRAWS + 1)]
        h = [v[k] for v in hp]
        for lst, v in zip(orc, runs[0] if runs[0] is not None else [np.full(v.shape, np.inf) for v in h]):
            lst.append(v)
        for j in range(len(names)):
            ref[j, k] = max(np.inf if r is None else err(r[j], h[j]) for r in runs)
    orc = [np.array(v, dtype=float) for v in orc]
    return dict(model=M, outputs=names, hp=hp, oracle=orc, eo=errors(orc, hp, names), ref=ref, hp_next=nxt)


def corr_M(family, n, m, per_track):
    """M = 0.5 chol(Q) G chol(R)' (the joint noise covariance stays PSD); per track scaled by 1 + 0.1 U -> (n,m) | (N,n,m)"""
    I = inputs(family, n, m)
    return I["Mc"] * I["Mscale"][:, None, None] if per_track else I["Mc"]


def truth_corr(family, n, m, per_track=False, single=False, mutate=None, joseph=False):
    """update_correlated on the 16 checked tracks: the recursion of T_CORR x {predict; update_correlated} from x0, P0, or
    (single) one update on each of the priors of SINGLE_STEPS (oracle_bank).  Adds `zs` [steps][N][m] and, for the singles,
    `xp`, `Pp` [steps][N]..., the bank's inputs.  joseph (with single): the plain Joseph-form update on the same priors, the truth
    of the update with a given inverse."""
    assert single or not joseph
    key = ("corr", family, n, m, per_track, single, mutate, joseph)
    if key in _truth_cache:
        return _truth_cache[key]
    _root_on_path()
    from oracle import kf_oracle
    M = kf_hp.models(family, n, m)
    Mc, N = corr_M(family, n, m, per_track), M["N"]
    Mof = lambda trk: Mc[trk] if per_track else Mc  # noqa: E731
    steps = list(SINGLE_STEPS) if single else list(range(T_CORR))
    zs = M["zs"][steps]
    if single:
        ob = oracle_bank(family, n, m)
        xp, Pp = ob["xp"][steps], ob["Pp"][steps]
        hp_of = lambda trk: corr_singles(xp[:, trk], Pp[:, trk], zs[:, trk], M["H"], M["R"], Mof(trk), mutate, joseph)  # noqa: E731
    else:
        hp_of = lambda trk: corr_recursion(M["x0"][trk], M["P0"][trk], zs[:, trk], M["F"], M["H"], M["Q"], M["R"],  # noqa: E731
                                           Mof(trk), mutate)
    if mutate is not None:                                   # [outputs][tracks][steps reached]: ragged where a track broke down
        _truth_cache[key] = dict(model=M, hp=[list(v) for v in zip(*[hp_of(trk) for trk in M["tracks"]])])
        return _truth_cache[key]
    hp = [np.array(v) for v in zip(*[hp_of(trk) for trk in M["tracks"]])]
    rs = np.random.RandomState(7919 * n + 31 * m + FAMILIES.index(family) + 2000003)

    def runs_of(k, trk, d):
        p = (lambda a, sym=False: a) if d == 0 else (lambda a, sym=False: ulp(rs, a, sym))
        H, R, Mt, z = p(M["H"]), p(M["R"], True), p(Mof(trk)), p(zs[:, trk])
        out = [[] for _ in CORR_OUTPUTS]
        try:
            if single:
                xs, Ps = p(xp[:, trk]), p(Pp[:, trk], True)
            else:
                x, P, F, Q = p(M["x0"][trk]), p(M["P0"][trk], True), p(M["F"]), p(M["Q"], True)
            for s in range(len(steps)):
                if single:
                    x, P = xs[s], Ps[s]
                else:
                    x, P = kf_oracle.kf_predict(x, P, F, Q)
                if joseph:
                    x, P, y, K, S, SI = kf_oracle.kf_update(x, P, z[s], R, H)
                else:
                    x, P, y, K, S, SI = kf_oracle.update_correlated(x, P, z[s], R, H, Mt)
                for lst, v in zip(out, (x, P, K, S, SI, y)):
                    lst.append(v)
        except np.linalg.LinAlgError:
            return None
        return [np.array(v) for v in out]

    t = _finish(M, CORR_OUTPUTS, hp, runs_of, np.array([hp_of((trk + 1) % N)[0] for trk in M["tracks"]]))
    t.update(zs=zs, M=Mc, steps=steps)
    if single:
        t.update(xp=xp, Pp=Pp)
    _truth_cache[key] = t
    return t


def steady_K(family, n, m, per_track):
    """the float64 rounding of the truth's gain at the last step: checked track 0's, shared, or every track's own"""
    K = oracle_bank(family, n, m)["K"][-1]
    return K.copy() if per_track else K[0].copy()


def truth_steady(family, n, m, per_track=False, nu=0):
    """the steady-state filter on the 16 checked tracks, step 8 missing; adds K, B, us, the bank's inputs"""
    key = ("steady", family, n, m, per_track, nu)
    if key in _truth_cache:
        return _truth_cache[key]
    _root_on_path()
    from oracle import kf_oracle
    M, I = kf_hp.models(family, n, m), inputs(family, n, m)
    K, N, T = steady_K(family, n, m, per_track), M["N"], M["T"]
    B, us = (I["B"][:, :nu].copy(), I["us"][..., :nu].copy()) if nu else (None, None)
    Kof = lambda trk: K[trk] if per_track else K  # noqa: E731
    zl = lambda zs: [zs[t] if M["mask"][t] else None for t in range(T)]  # noqa: E731
    hp_of = lambda trk: steadystate_filter(M["x0"][trk], zl(M["zs"][:, trk]), M["F"], M["H"], Kof(trk), B,  # noqa: E731
                                           None if us is None else us[:, trk])
    hp = [np.array(v) for v in zip(*[hp_of(trk) for trk in M["tracks"]])]
    rs = np.random.RandomState(7919 * n + 31 * m + FAMILIES.index(family) + 3000003)

    def runs_of(k, trk, d):
        p = (lambda a: a) if d == 0 else (lambda a: ulp(rs, a))
        return list(kf_oracle.steadystate_filter(p(M["x0"][trk]), zl(p(M["zs"][:, trk])), p(M["F"]), p(M["H"]), p(Kof(trk)),
                                                 None if B is None else p(B), None if us is None else p(us[:, trk])))

    t = _finish(M, STEADY_OUTPUTS, hp, runs_of, np.array([hp_of((trk + 1) % N)[0] for trk in M["tracks"]]))
    t.update(K=K, B=B, us=us)
    _truth_cache[key] = t
    return t


# ---------------------------------------------------------------------------------------------------------------- the bar
def measures_something(t, names=None):
    """kf_hp.measures_something on the outputs of this truth: all 16 tracks finish in the oracle and in every perturbed run,
    err(oracle, hp) is finite and < 1e-3 on every output, and ref >= err(oracle, hp)"""
    M, names = t["model"], t["outputs"] if names is None else names
    rows = [t["outputs"].index(k) for k in names]
    assert len(M["tracks"]) == 16 == len(set(M["tracks"])) and set(ukf_hp.FIXED_TRACKS) <= set(M["tracks"])
    assert t["eo"].shape == t["ref"].shape == (len(t["outputs"]), 16)
    eo, ref = t["eo"][rows], t["ref"][rows]
    assert np.all(np.isfinite(eo)) and np.all(np.isfinite(ref)), (eo.max(axis=1), ref.max(axis=1))
    assert eo.max() < 1e-3, dict(zip(names, eo.max(axis=1)))
    assert np.all(ref >= eo)


def check(label, eg, t, names):
    """kf_hp.check on the outputs `names` of this truth: every checked track <= max(MARGIN max ref, FLOOR), the median <=
    max(MARGIN median ref, FLOOR); eg is [len(t["outputs"])][16], and no error of a checked output may be missing"""
    bad = []
    for name in names:
        j = t["outputs"].index(name)
        assert not np.isnan(eg[j]).any(), (label, name, eg[j])
        bad += ukf_hp.check(f"{label} {name}", eg[j:j + 1], t["ref"][j:j + 1], MARGIN, FLOOR)
    return bad


def ratios(eg, t, names):
    """per output: (name, worst err / bar, build / oracle, ref / oracle), the last two as ratios of the worst track's errors"""
    rows = []
    for name in names:
        j = t["outputs"].index(name)
        bar, mbar = max(MARGIN * t["ref"][j].max(), FLOOR), max(MARGIN * np.median(t["ref"][j]), FLOOR)
        eo = max(t["eo"][j].max(), 1e-300)
        rows.append((name, max(eg[j].max() / bar, np.median(eg[j]) / mbar), eg[j].max() / eo, t["ref"][j].max() / eo))
    return rows


not_the_neighbour = kf_hp.not_the_neighbour
