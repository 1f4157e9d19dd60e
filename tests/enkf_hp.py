"""The reference's ensemble Kalman filter in np.longdouble (80-bit on x86-64), written from the algorithm tests/enkf_port.py
restates (filterpy/kalman/ensemble_kalman_filter.py:240-290), the draws being arguments: predict moves every member by F and
adds its draw, x is the mean and P the TWO-PASS centred second moment; update centres the members on the x GIVEN and sigmas_h
on their own mean, inverts S by a longdouble Cholesky factorisation (ukf_hp.spd_inv), and takes P - K S K' on the stored P.
The factor path is e = w @ A in longdouble from the float64 factor A.

Sums over members.  The truth must not depend on the order the members are added in: the stiff family amplifies a last-bit
change of a longdouble sum by the cancellation of P - K S K' (1e6 ... 1e8), which a plain longdouble sum over 34 819 members
does not survive at the FLOOR / 100 that truth() asserts.  So every sum over members is a pairwise tree of error-free additions
(TwoSum) whose low parts are carried along and added at the end: the sum of the rounded terms to ~1e-36, hence the same longdouble
whatever the order.  (The terms themselves -- a centred product -- are rounded once each, member by member, the same in any order.)

This is the truth tests/test_gpu_enkf_precision.py and tests/test_host_enkf_hp.py measure the kernels, the host build of
csrc/fk_enkf.hpp and the float64 oracle (enkf_port, mode="twopass") against.  The bar is kf_hp's: the REFERENCE ERROR of an output,

    ref = max(err(oracle, hp), max over K_DRAWS draws of err(oracle on inputs perturbed by one ulp, hp))

with hp the truth of the unperturbed inputs, and check() holds a build to err(build, hp) <= max(MARGIN * ref, FLOOR) on every
output.  Errors are normwise per step, the worst step counted; for the ensemble also the worst single MEMBER (max over steps
and members of |s_i - hp_i| / |hp_i|): one wrong tail member of 34 819 is invisible in the norm of the whole ensemble."""
import numpy as np

import enkf_port as ep
import ukf_hp
from kf_hp import ulp
from ukf_hp import LD, ld, spd_inv

MARGIN = 8.0
FLOOR = ukf_hp.FLOOR
K_DRAWS = 8
T_RUN = 6
T_SINGLE = 3                                 # the single-step paths start from the truth's rounded state at this step
FAMILIES = ("benign", "offset", "stiff")
# a chained run: the ensemble after predict and after update, the prior, the posterior and the by-products of the update
CHAIN = ("sig_prior", "sig_post", "x_prior", "P_prior", "x_post", "P_post", "K", "S", "SI")
MEMBER = ("sig_prior", "sig_post")           # ... these two are measured member by member as well
PREDICT = ("sig_prior", "x_prior", "P_prior")
UPDATE = ("sig_post", "x_post", "P_post", "K", "S", "SI")
# the cases of both precision files: every kernel (the fast ones at their four shapes, the general one at (5,2) and (16,8)) at
# N - 1 = 1, 3, a wave's tail, an exactly full chunk, one member more, and more slabs than the finalize has runs (at three
# shapes); stiff from N = 65 (at N <= 3 its S - R has rank N - 1 < m and the oracle's reference error is 3e-2 ... 8e-2)
CHUNK = 2048
BIG = 17 * CHUNK + 3
DIMS = ((2, 1), (4, 2), (5, 2), (6, 3), (9, 4), (16, 8))
BIG_DIMS = ((4, 2), (9, 4), (16, 8))
SIZES = {"benign": (2, 3, 65, CHUNK, CHUNK + 1), "offset": (2, 3, 65, CHUNK, CHUNK + 1), "stiff": (65, CHUNK + 1)}
MATRIX = ([(f, n, m, N) for f in FAMILIES for n, m in DIMS for N in SIZES[f]] +
          [(f, n, m, BIG) for f in FAMILIES for n, m in BIG_DIMS])
SINGLE_ROWS = [r for r in MATRIX if r[3] in (65, CHUNK + 1, BIG)]          # the single-step paths run at these
SELF_SCATTER = [0.0]                         # the largest truth-against-reversed-truth error any truth() has seen


# ---------------------------------------------------------------------------------------------------- sums over members
def _two_sum(a, b):
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


def _tree(hi, lo=None):
    """a pairwise tree over axis 0 of the pairs (hi, lo) (lo None: zeros): every addition of two high parts is error-free (its
    error joins the low parts) -> the root's pair, not yet rounded to one longdouble.  Each level adds the first half to the
    second (contiguous, and a tree like any other)."""
    while len(hi) > 1:
        h = len(hi) // 2
        odd_hi, odd_lo = hi[2 * h:], None if lo is None else lo[2 * h:]
        s, e = _two_sum(hi[:h], hi[h:2 * h])
        e = e if lo is None else (lo[:h] + lo[h:2 * h]) + e
        if len(odd_hi):                                       # the member left over rides along, unadded
            s, e = np.concatenate([s, odd_hi]), np.concatenate([e, np.zeros_like(odd_hi) if odd_lo is None else odd_lo])
        hi, lo = s, e
    return hi[0], (np.zeros_like(hi[0]) if lo is None else lo[0])


def _blocks(N, block, term):
    """the pairs of term(k0, k1) over blocks of members, put into one more tree unrounded (the blocks only keep the
    temporaries in cache) -> the sum, rounded once"""
    pairs = [_tree(term(k, min(k + block, N))) for k in range(0, N, block)]
    hi, lo = _tree(np.array([p[0] for p in pairs]), np.array([p[1] for p in pairs]))
    return hi + lo


def msum(a, block=256):
    """sum over axis 0 of a longdouble array (N >= 1), order-independent to ~1e-36 (see the module docstring)"""
    return _blocks(len(a), block, lambda k0, k1: a[k0:k1])


def cross(a, b=None, block=256):
    """sum_i a_i b_i' for a (N, p), b (N, q): the products rounded once each, member by member; their sum as in msum.
    b None: sum_i a_i a_i', its lower triangle computed and mirrored"""
    p = a.shape[1]
    if b is None:
        r, c = np.tril_indices(p)
        out = np.empty((p, p), dtype=LD)
        out[r, c] = out[c, r] = _blocks(len(a), block, lambda k0, k1: a[k0:k1, r] * a[k0:k1, c])
        return out
    return _blocks(len(a), block, lambda k0, k1: (a[k0:k1, :, None] * b[k0:k1, None, :]).reshape(k1 - k0, -1)).reshape(p, b.shape[1])


# ------------------------------------------------------------------------------------------------------------ the truth
def predict(sig, e, F=None, factor=None):
    """members (N, n) moved by F (None: already moved) plus the draws e (factor given: e = w @ factor) -> sigmas, x, P"""
    sig, e = ld(sig), ld(e)
    if factor is not None:
        e = e @ ld(factor)
    sig = (sig @ ld(F).T if F is not None else sig) + e
    N = len(sig)
    x = msum(sig) / N
    d = sig - x
    return sig, x, cross(d) / (N - 1)


def update(sig, x, P, z, R, e, H=None, sigmas_h=None, factor=None):
    """-> sigmas, x, P, K, S, SI.  The members are centred on the x given, sigmas_h on their own mean; P - K S K' on the P given"""
    sig, x, P, z, R, e = map(ld, (sig, x, P, z, R, e))
    if factor is not None:
        e = e @ ld(factor)
    N = len(sig)
    sh = sig @ ld(H).T if sigmas_h is None else ld(sigmas_h)
    dh = sh - msum(sh) / N
    S = cross(dh) / (N - 1) + R
    Pxz = cross(sig - x, dh) / (N - 1)
    SI = spd_inv(S)
    K = Pxz @ SI
    sig = sig + (z + e - sh) @ K.T
    return sig, msum(sig) / N, P - (K @ S) @ K.T, K, S, SI


def chain(sig0, e1, e2, zs, F, H, R, perm=None):
    """T predict + update cycles -> dict of CHAIN, [T]... each; perm: the order the members are held (and added up) in"""
    sig = ld(sig0)
    if perm is not None:
        sig, e1, e2 = sig[perm], e1[:, perm], e2[:, perm]
    out = {k: [] for k in CHAIN}
    for t in range(len(zs)):
        sig, x, P = predict(sig, e1[t], F)
        for k, v in zip(PREDICT, (sig, x, P)):
            out[k].append(v)
        sig, x, P, K, S, SI = update(sig, x, P, zs[t], R, e2[t], H)
        for k, v in zip(UPDATE, (sig, x, P, K, S, SI)):
            out[k].append(v)
    out = {k: np.array(v) for k, v in out.items()}
    if perm is not None:
        inv = np.argsort(perm)
        for k in MEMBER:
            out[k] = out[k][:, inv]
    return out


def oracle_chain(sig0, e1, e2, zs, F, H, R, mode="twopass"):
    """the same in float64 by tests/enkf_port.py (mode: its form of the second moments), feeding on its own state"""
    sig = np.array(sig0, dtype=float)
    out = {k: [] for k in CHAIN}
    for t in range(len(zs)):
        piv = sig[0] @ F.T + e1[t][0]                        # a pivot for the one-pass forms (the two-pass form takes none)
        sig, x, P = ep.predict(sig, e1[t], F, mode, piv)
        for k, v in zip(PREDICT, (sig, x, P)):
            out[k].append(v)
        sig, x, P, K, S, SI = ep.update(sig, x, P, zs[t], R, e2[t], H, mode=mode)
        for k, v in zip(UPDATE, (sig, x, P, K, S, SI)):
            out[k].append(v)
    return {k: np.array(v) for k, v in out.items()}


# ------------------------------------------------------------------------------------------------------------ the errors
def _rel(a, hp):
    """|a - hp| and |hp| per entry in longdouble; None where the shapes differ or a is not finite"""
    a = np.asarray(a)
    if a.shape != hp.shape or not np.all(np.isfinite(a)):
        return None
    return np.abs(a - hp), np.abs(hp)


def _norm_err(d, h):
    """worst normwise relative error over the leading axis (ukf_hp.err's measure)"""
    d, h = d.reshape(len(d), -1).max(axis=1), h.reshape(len(h), -1).max(axis=1)
    return float(np.max(d / np.maximum(h, 1e-300)))


def _member_err(d, h):
    """worst single member: max over the leading axes and members of |s_i - hp_i| / |hp_i| (max norms), arrays [..., N, n]"""
    return float(np.max(d.max(axis=-1) / np.maximum(h.max(axis=-1), 1e-300)))


def errors(got, hp, names=None):
    """{output: err, output + "_member": worst member} of a dict of arrays against the truth's; a missing output is NaN, one
    of another shape or not finite inf"""
    out = {}
    for k in (names or hp.keys()):
        g = got.get(k)
        r = None if g is None else _rel(g, hp[k])
        out[k] = np.nan if g is None else np.inf if r is None else _norm_err(*r)
        if k in MEMBER:
            out[k + "_member"] = np.nan if g is None else np.inf if r is None else _member_err(*r)
    return out


def _worst(runs):
    """per output the worst of several runs' errors; a NaN stays a NaN"""
    return {k: float(np.max([r[k] for r in runs])) for k in runs[0]}


def _finish(fn, hp):
    """errors of fn()'s outputs against hp; a run that does not finish (a singular S) leaves inf on every output"""
    try:
        with np.errstate(all="ignore"):
            return errors(fn(), hp)
    except np.linalg.LinAlgError:
        return {k: np.inf for k in errors({}, hp)}


# ------------------------------------------------------------------------------------------------------------ the models
def models(family, n, m, N, T=T_RUN):
    """One ensemble and the draws of T cycles, a fixed RandomState per (family, n, m, N):
    benign   F = I + 0.05 randn / sqrt(n), H = randn / sqrt(n), Q = 0.01 I, R = 0.5 I, spread 1, x0 = randn
    offset   the same with x0 = 1e4 (1 + U(0, 1)) + randn
    stiff    F = I + 0.5 superdiagonal + 0.01 randn, H = randn, Q = diag(10^U(-6, -2)), R = 1e-2 I, spread 1e2, x0 as offset,
             z = H x0 + 10 randn
    Returns F H Q R x0 sig0 (N, n) e1 (T, N, n) e2 (T, N, m) zs (T, m) and, for the factor path, w1 (N, n) w2 (N, m)."""
    assert family in FAMILIES, family
    rs = np.random.RandomState((1000003 * FAMILIES.index(family) + 10007 * n + 101 * m + N) % 2 ** 32)
    if family == "stiff":
        F = np.eye(n) + 0.5 * np.diag(np.ones(n - 1), 1) + 0.01 * rs.randn(n, n)
        H = rs.randn(m, n)
        Q = np.diag(10.0 ** rs.uniform(-6, -2, n))
        R, spread, zsd = 1e-2 * np.eye(m), 1e2, 10.0
    else:
        F = np.eye(n) + 0.05 * rs.randn(n, n) / np.sqrt(n)
        H = rs.randn(m, n) / np.sqrt(n)
        Q, R, spread, zsd = 0.01 * np.eye(n), 0.5 * np.eye(m), 1.0, 1.0
    x0 = rs.randn(n) if family == "benign" else 1e4 * (1.0 + rs.rand(n)) + rs.randn(n)
    sig0 = x0 + spread * rs.randn(N, n)
    e1 = rs.randn(T, N, n) * np.sqrt(np.diag(Q))
    e2 = rs.randn(T, N, m) * np.sqrt(np.diag(R))
    zs = H @ x0 + zsd * rs.randn(T, m)
    return dict(family=family, n=n, m=m, N=N, T=T, F=F, H=H, Q=Q, R=R, x0=x0, spread=spread, sig0=sig0, e1=e1, e2=e2, zs=zs,
                w1=rs.randn(N, n), w2=rs.randn(N, m))


def _perturbed(rs, M):
    return dict(sig0=ulp(rs, M["sig0"]), e1=ulp(rs, M["e1"]), e2=ulp(rs, M["e2"]), zs=ulp(rs, M["zs"]), F=ulp(rs, M["F"]),
                H=ulp(rs, M["H"]), R=ulp(rs, M["R"], True))


_ARGS = ("sig0", "e1", "e2", "zs", "F", "H", "R")
_truth_cache = {}


def _stable(label, a, b):
    """the truth against the truth with the members in reversed order: below FLOOR / 100 on every output, members included"""
    for k, v in errors(b, a).items():
        SELF_SCATTER[0] = max(SELF_SCATTER[0], v)
        assert v < FLOOR / 100, (label, k, v)


def truth(family, n, m, N):
    """Computed once per key and shared, never modified:
    model   the models() dict
    hp      the longdouble outputs of the chained run, {CHAIN: [T]...}
    eo      err(oracle, hp) per output (and per "_member" output)
    ref     the reference error: the worst of eo and of the K_DRAWS one-ulp draws against the same hp
    The oracle not finishing, or not finite, leaves inf (the tests assert finiteness: nothing is ever left out)."""
    key = (family, n, m, N)
    if key in _truth_cache:
        return _truth_cache[key]
    M = models(family, n, m, N)
    args = [M[k] for k in _ARGS]
    hp = chain(*args)
    _stable(key, hp, chain(*args, perm=np.arange(N)[::-1]))
    rs = np.random.RandomState(7919 * n + 31 * m + FAMILIES.index(family) + N)
    eo = _finish(lambda: oracle_chain(*args), hp)
    runs = [eo] + [_finish(lambda: oracle_chain(*[p[k] for k in _ARGS]), hp) for p in (_perturbed(rs, M) for _ in range(K_DRAWS))]
    _truth_cache[key] = dict(model=M, hp=hp, eo=eo, ref=_worst(runs))
    return _truth_cache[key]


# --------------------------------------------------------------------------------------- the single steps from step T_SINGLE
SINGLE = ("sigmas_h", "moved", "factor")
_single_cache = {}


def class_pivot(members):
    """the pivot EnsembleKalmanFilter.predict passes where fx is a callable: member 0 as fx left it"""
    return np.array(members[0], dtype=float)


def single_inputs(M, hp, path):
    """float64 inputs of one single step, from the truth's state at step T_SINGLE rounded:
    sigmas_h   update(sigmas_h = the predicted members' H s, rounded) from the prior of step T_SINGLE
    moved      predict(F=None): the posterior members of step T_SINGLE - 1 moved by F (rounded), the draw still to be added
    factor     predict and update from the same states with e = w @ factor(Q), w @ factor(R)"""
    t = T_SINGLE
    f64 = lambda a: np.asarray(a, dtype=np.float64)  # noqa: E731
    if path == "sigmas_h":
        sig = f64(hp["sig_prior"][t])
        return dict(sig=sig, x=f64(hp["x_prior"][t]), P=f64(hp["P_prior"][t]), z=M["zs"][t], R=M["R"], e=M["e2"][t],
                    sigmas_h=f64(ld(sig) @ ld(M["H"]).T))
    if path == "moved":
        return dict(sig=f64(hp["sig_post"][t - 1] @ ld(M["F"]).T), e=M["e1"][t])
    return dict(sig=f64(hp["sig_post"][t - 1]), x0=f64(hp["x_post"][t - 1]), F=M["F"], w1=M["w1"], A1=ep.factor(M["Q"]),
                sig2=f64(hp["sig_prior"][t]), x=f64(hp["x_prior"][t]), P=f64(hp["P_prior"][t]), z=M["zs"][t], R=M["R"], H=M["H"],
                w2=M["w2"], A2=ep.factor(M["R"]))


def far_member0(i, path, spreads=30.0):
    """the single step's inputs with member 0 moved to `spreads` ensemble spreads from the mean (in every coordinate)"""
    j = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in i.items()}
    key = "sigmas_h" if path == "sigmas_h" else "sig"
    a = j[key]
    a[0] = a[1:].mean(axis=0) + spreads * a[1:].std(axis=0)
    return j


def single_run(i, path, pred, upd, perm=None):
    """one single step by the functions pred(sig, x, e, F, factor) -> sig, x, P (x: the mean before the step, None where the
    members come already moved) and upd(sig, x, P, z, R, e, H, sigmas_h, factor) ->
    sig, x, P, K, S, SI: the truth's, the oracle's, or a build under test.  -> dict of outputs (leading axis 1)"""
    p = (lambda a: a) if perm is None else (lambda a: a[perm])
    back = (lambda a: a) if perm is None else (lambda a: a[np.argsort(perm)])
    out = {}
    if path == "sigmas_h":
        res = upd(p(i["sig"]), i["x"], i["P"], i["z"], i["R"], p(i["e"]), None, p(i["sigmas_h"]), None)
        out = dict(zip(UPDATE, res))
    elif path == "moved":
        out = dict(zip(PREDICT, pred(p(i["sig"]), None, p(i["e"]), None, None)))
    else:
        out = dict(zip(PREDICT, pred(p(i["sig"]), i["x0"], p(i["w1"]), i["F"], i["A1"])))
        out.update(zip(UPDATE, upd(p(i["sig2"]), i["x"], i["P"], i["z"], i["R"], p(i["w2"]), i["H"], None, i["A2"])))
    return {k: (back(np.asarray(v)) if k in MEMBER else np.asarray(v))[None] for k, v in out.items()}


def _hp_pred(sig, x, e, F, factor):
    return predict(sig, e, F, factor)


def _hp_upd(sig, x, P, z, R, e, H, sigmas_h, factor):
    return update(sig, x, P, z, R, e, H, sigmas_h, factor)


def _or_pred(sig, x, e, F, factor):
    return ep.predict(sig, e if factor is None else e @ factor, F)


def _or_upd(sig, x, P, z, R, e, H, sigmas_h, factor):
    return ep.update(sig, x, P, z, R, e if factor is None else e @ factor, H, sigmas_h)


def _perturbed_single(rs, i):
    sym = ("P", "R")
    fixed = ("A1", "A2")                     # the factors are inputs as they are: e = w @ A is taken from the float64 A given
    return {k: (v if k in fixed else ulp(rs, v, k in sym)) for k, v in i.items()}


def single_truth(family, n, m, N, path, inputs=None):
    """truth(), for one single step: {"in": inputs, "hp", "eo", "ref"}.  inputs: another set than single_inputs' (the pivot
    contract's ensembles); then nothing is cached"""
    key = (family, n, m, N, path)
    if inputs is None and key in _single_cache:
        return _single_cache[key]
    t = truth(family, n, m, N)
    i = single_inputs(t["model"], t["hp"], path) if inputs is None else inputs
    hp = single_run(i, path, _hp_pred, _hp_upd)
    _stable(key, hp, single_run(i, path, _hp_pred, _hp_upd, perm=np.arange(len(i["sig"]))[::-1]))
    rs = np.random.RandomState(104729 + 7919 * n + 31 * m + FAMILIES.index(family) + N + SINGLE.index(path))
    orc = lambda j: _finish(lambda: single_run(j, path, _or_pred, _or_upd), hp)  # noqa: E731
    eo = orc(i)
    runs = [eo] + [orc(_perturbed_single(rs, i)) for _ in range(K_DRAWS)]
    res = {"in": i, "hp": hp, "eo": eo, "ref": _worst(runs)}
    if inputs is None:
        _single_cache[key] = res
    return res


# --------------------------------------------------------------------------------------------------------------- the bar
def measures_something(t):
    """the condition of every precision test: the oracle finishes finite and is within 1e-3 of the truth on every output, and
    so is every one of its perturbed runs' worst"""
    assert t["eo"].keys() == t["ref"].keys() and len(t["eo"]) >= 3
    for k in t["eo"]:
        assert np.isfinite(t["eo"][k]) and np.isfinite(t["ref"][k]), (k, t["eo"][k], t["ref"][k])
        assert t["ref"][k] >= t["eo"][k] and t["ref"][k] < 1e-3, (k, t["eo"][k], t["ref"][k])


def check(label, eg, t, margin=MARGIN):
    """every output of the truth: err(build, hp) <= max(margin * ref, FLOOR), and none missing.  Prints one row per output
    (err/bar, build/oracle, ref/oracle); returns the failures."""
    assert set(eg) == set(t["ref"]), (label, sorted(set(t["ref"]) ^ set(eg)))
    bad = []
    for k, ref in t["ref"].items():
        assert not np.isnan(eg[k]), (label, k, "not produced")
        bar, eo = max(margin * ref, FLOOR), max(t["eo"][k], 1e-300)
        print("%-44s %-17s err/bar %.3f  build/oracle %8.2f  ref/oracle %6.2f  oracle %.1e" % (
            label, k, eg[k] / bar, eg[k] / eo, ref / eo, t["eo"][k]))
        if not eg[k] <= bar:
            bad.append((label, k, float(eg[k] / bar), float(eg[k])))
    return bad
