"""CPU: the host build of csrc/fk_enkf.hpp (tests/enkf_host.py: the kernels' arithmetic in the kernels' order -- pivot-shifted
one-pass sums, the workgroup's tree, the slabs in 16 runs, the L D L' inverse, P - K S K') against tests/enkf_hp.py, the
reference's algorithm in longdouble, through every case of tests/test_gpu_enkf_precision.py and against the same bar
(enkf_hp.check: MARGIN = 8 times the reference error of the float64 oracle, floor 1e-13).

This file is where the MARGIN is checked for the EnKF: it is the scatter between two legitimate float64 orderings (the two-pass
oracle and this build), never what the GPU reaches.  It also shows that the bar has teeth (the uncentred one-pass form and an
inverse from unrefined seeded pivots fail it) and measures the pivot contract: what a one-pass sum loses when its pivot, member 0,
is thirty spreads from the mean.  docs/MEASUREMENTS.md ("EnKF precision") has the figures."""
import numpy as np
import pytest

import enkf_hp as hp
import enkf_host
from enkf_host import hc_predict, hc_update

CHUNK, BIG, DIMS, MATRIX = hp.CHUNK, hp.BIG, hp.DIMS, hp.MATRIX


@pytest.fixture(scope="module")
def hc(tmp_path_factory):
    return enkf_host.libs(tmp_path_factory)


def host_chain(lib, M):
    """the chained run through one host build, feeding on its own state"""
    sig, x, P = M["sig0"].copy(), M["x0"].copy(), np.eye(M["n"])
    out = {k: [] for k in hp.CHAIN}
    for t in range(M["T"]):
        sig, x, P = hc_predict(lib, sig, x, M["e1"][t], M["F"])
        for k, v in zip(hp.PREDICT, (sig, x, P)):
            out[k].append(v)
        sig, x, P, K, S, SI, st = hc_update(lib, sig, x, P, M["zs"][t], M["R"], M["e2"][t], M["H"])
        assert st == 0, (t, st)
        for k, v in zip(hp.UPDATE, (sig, x, P, K, S, SI)):
            out[k].append(v)
    return {k: np.array(v) for k, v in out.items()}


def host_single(lib, i, path, pivot=hp.class_pivot):
    """one single step through one host build; the pivot of predict(F=None) is the class's"""
    def pred(sig, x, e, F, factor):
        return hc_predict(lib, sig, pivot(sig) if F is None else x, e, F, factor)

    def upd(sig, x, P, z, R, e, H, sigmas_h, factor):
        *out, st = hc_update(lib, sig, x, P, z, R, e, H, sigmas_h, factor)
        assert st == 0
        return out
    return hp.single_run(i, path, pred, upd)


def test_longdouble_is_extended_precision():
    assert np.finfo(np.longdouble).eps < 2e-19


def test_the_sums_over_members_do_not_depend_on_their_order():
    """what truth() relies on: msum / cross give the same longdouble for any order of the members, where plain sums do not"""
    rs = np.random.RandomState(1)
    a = hp.ld(1e4 + rs.randn(5000, 3)) * hp.ld(1 + 1e-3 * rs.randn(5000, 3))       # longdouble terms with low bits set
    p = rs.permutation(5000)
    assert np.array_equal(hp.msum(a), hp.msum(a[p])) and np.array_equal(hp.cross(a), hp.cross(a[p], a[p]))
    assert not np.array_equal(a.sum(axis=0), a[p].sum(axis=0))
    assert np.array_equal(hp.msum(a, block=4096), hp.msum(a)) and hp.ukf_hp.err(hp.msum(a)[None], a.sum(axis=0)[None]) < 1e-17


@pytest.mark.parametrize("n,m", DIMS)
def test_the_truth_is_a_truth(n, m):
    """on the benign family the oracle and the longdouble filter agree to 1e-12 on every output, every member included, at a
    lane's worth of members and over several chunks; the truth does not move when the members are reversed (truth() asserts it)"""
    for N in (65, CHUNK + 1):
        t = hp.truth("benign", n, m, N)
        hp.measures_something(t)
        assert max(t["eo"].values()) < 1e-12, t["eo"]
        assert set(t["eo"]) == set(hp.CHAIN) | {k + "_member" for k in hp.MEMBER}


def test_stiff_at_three_members_measures_nothing():
    """why stiff starts at N = 65: at N = 3 its S - R has rank 2 < m, the oracle's reference error is 3e-2 at (9,4) (8e-2 at
    (16,8)), and the condition every test asserts first refuses the model"""
    with pytest.raises(AssertionError):
        hp.measures_something(hp.truth("stiff", 9, 4, 3))


@pytest.mark.parametrize("family,n,m,N", MATRIX)
def test_host_build_meets_the_bar(hc, family, n, m, N):
    """every case of the GPU matrix through the build the dispatch's choice of kernel corresponds to; first the condition
    (the oracle finite and < 1e-3 on every output), then the bar"""
    t = hp.truth(family, n, m, N)
    hp.measures_something(t)
    eg = hp.errors(host_chain(enkf_host.lib_for(hc, n, m), t["model"]), t["hp"])
    bad = hp.check(f"host {family} ({n},{m}) N={N}", eg, t)
    assert not bad, bad
    assert hp.SELF_SCATTER[0] < hp.FLOOR / 100


@pytest.mark.parametrize("family", hp.FAMILIES)
def test_padded_build_at_an_exact_shape_meets_the_bar(hc, family):
    """(6,3) through the padded (16,8) build: what FK_ENKF_GENERAL=1 runs"""
    for N in (65, CHUNK + 1):
        t = hp.truth(family, 6, 3, N)
        hp.measures_something(t)
        bad = hp.check(f"host general {family} (6,3) N={N}", hp.errors(host_chain(hc[None], t["model"]), t["hp"]), t)
        assert not bad, bad


@pytest.mark.parametrize("path", hp.SINGLE)
@pytest.mark.parametrize("family,n,m,N", hp.SINGLE_ROWS)
def test_host_build_single_steps_meet_the_bar(hc, family, n, m, N, path):
    """sigmas_h given, predict behind a callable (F=None, the pivot the class passes), the factor path"""
    t = hp.single_truth(family, n, m, N, path)
    hp.measures_something(t)
    bad = hp.check(f"host {path} {family} ({n},{m}) N={N}", hp.errors(host_single(enkf_host.lib_for(hc, n, m), t["in"], path), t["hp"]), t)
    assert not bad, bad


# ---- the bar has teeth ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,m,N", [(4, 2, 65), (9, 4, CHUNK + 1), (16, 8, CHUNK + 1)])
def test_uncentred_sums_fail_the_bar_on_offset(n, m, N):
    """the one-pass sum of raw products (enkf_port mode="uncentred") loses |x|^2 / var = 1e8 of its digits at offset 1e4"""
    t = hp.truth("offset", n, m, N)
    M = t["model"]
    eg = hp._finish(lambda: hp.oracle_chain(*[M[k] for k in hp._ARGS], mode="uncentred"), t["hp"])
    bad = hp.check(f"uncentred offset ({n},{m}) N={N}", eg, t)
    assert {b[1] for b in bad} >= {"P_prior", "S", "K"}, bad
    assert max(b[2] for b in bad) > 100, bad


@pytest.mark.parametrize("n,m,N", [(4, 2, 65), (9, 4, CHUNK + 1)])
def test_shifted_sums_in_numpy_meet_the_bar_on_offset(n, m, N):
    """... while the pivot-shifted form in NumPy (mode="shifted", the pivot within a spread of the mean) is inside it"""
    t = hp.truth("offset", n, m, N)
    M = t["model"]
    eg = hp.errors(hp.oracle_chain(*[M[k] for k in hp._ARGS], mode="shifted"), t["hp"])
    bad = hp.check(f"shifted offset ({n},{m}) N={N}", eg, t)
    assert not bad, bad


_INV = np.linalg.inv


def _seeded_inverse(S, steps):
    """inv(S) by the L D L' of fk_ukf.hpp with every pivot's reciprocal from a float-rounded seed (the stand-in of
    tests/test_host_ukf_hp.py for the hardware's 2^-24) and `steps` Newton refinements (the kernels run two)"""
    m = len(S)
    L, d, di = np.eye(m), np.zeros(m), np.zeros(m)
    for j in range(m):
        d[j] = S[j, j] - (L[j, :j] ** 2) @ d[:j]
        r = float(np.float32(1.0 / d[j]))
        for _ in range(steps):
            r = r + r * (1.0 - d[j] * r)
        di[j] = r
        for i in range(j + 1, m):
            L[i, j] = (S[i, j] - (L[i, :j] * d[:j]) @ L[j, :j]) * di[j]
    Li = _INV(L)
    return Li.T @ (di[:, None] * Li)


@pytest.mark.parametrize("steps,passes", [(0, False), (2, True)])
def test_unrefined_seeded_pivots_fail_the_bar_on_stiff(monkeypatch, steps, passes):
    """the oracle with its inverse replaced: seeds alone (6e-8 per pivot) fail K, SI and the posterior on stiff at (9,4);
    refined twice, as the kernels do, the same inverse is inside the bar (0.12 of it).  ONE refinement (3.6e-15 per pivot) is
    inside it too on these families -- at most 0.51 of the bar (the posterior P at (16,8), N = 65; 4.1 x the oracle), 0.08-0.15
    elsewhere: S here has condition <= 1e6, and the bar would not tell a single-refinement kernel from this one; the UKF's stiff
    models (tests/test_host_ukf_hp.py) are what holds the refinement count of fk_ukf.hpp"""
    t = hp.truth("stiff", 9, 4, CHUNK + 1)
    M = t["model"]
    monkeypatch.setattr(np.linalg, "inv", lambda S: _seeded_inverse(S, steps))
    eg = hp.errors(hp.oracle_chain(*[M[k] for k in hp._ARGS]), t["hp"])
    monkeypatch.undo()
    bad = hp.check(f"seeded pivots, {steps} refinements, stiff (9,4)", eg, t)
    if passes:
        assert not bad, bad
    else:
        assert {b[1] for b in bad} >= {"SI", "K", "sig_post_member"}, bad


# ---- the pivot contract ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", ["sigmas_h", "moved"])
@pytest.mark.parametrize("n,m", [(4, 2), (9, 4)])
def test_pivot_contract_member0_at_30_spreads(hc, n, m, path):
    """offset 1e4, N = 2049, member 0 thirty spreads from the mean in every coordinate, and member 0 is the pivot: of sigmas_h in
    the update, of the members in a predict behind a callable (what EnsembleKalmanFilter.predict passes).  A one-pass sum pivoted
    d spreads from the mean loses eps d^2 against the two-pass form: measured here, S / SI / K / the posterior P are 100-210 x the
    oracle's own error on the same inputs (sigmas_h), the prior P 2.8 x (moved) -- and still 0.05 / 0.09 of the bar, because at
    offset 1e4 a one-ulp change of the inputs already moves the oracle by 500 x its own rounding (ref / oracle in the rows
    printed).  So the contract the comments state holds as far as the bar can see, and the kernels keep member 0."""
    N = CHUNK + 1
    i = hp.far_member0(hp.single_truth("offset", n, m, N, path)["in"], path)
    far = i["sigmas_h" if path == "sigmas_h" else "sig"]
    assert np.all(np.abs(far[0] - far[1:].mean(axis=0)) > 29 * far[1:].std(axis=0))
    t = hp.single_truth("offset", n, m, N, path, inputs=i)
    hp.measures_something(t)
    eg = hp.errors(host_single(enkf_host.lib_for(hc, n, m), i, path), t["hp"])
    bad = hp.check(f"host {path} member 0 at 30 spreads ({n},{m})", eg, t)
    assert not bad, bad
