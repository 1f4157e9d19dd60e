"""The EnKF kernels on the MI355X against tests/enkf_hp.py, the reference's algorithm in longdouble, at engine level
(E.enkf_predict / E.enkf_update) and in both record orders: the launch chain, the workgroup's tree, the slab indexing, the tails
of a lane, a wave and a chunk, the general kernel with its sums in scratch memory -- everything the host build of
csrc/fk_enkf.hpp (tests/test_host_enkf_hp.py, the same cases and the same bar) does not contain.

The bar (enkf_hp.check): every output of a run -- the ensemble after predict and after update in norm AND member by member, the
prior, the posterior, K, S, SI -- is within max(MARGIN * ref, 1e-13) of the truth, ref being the float64 oracle's own error on
these inputs and on K_DRAWS copies perturbed by one ulp.  Every case first asserts that the oracle measures something (finite,
ref < 1e-3 on every output), then status 0, every output finite, and the bar.  The truth is computed once per (family, dims, N)
and shared by the layouts (the three truths at (16,8) and N = 17 CHUNK + 3 take seven seconds each -- two longdouble runs over
34 819 members, the second to show that the truth does not move -- every other case a second or less).  Every row prints
err/bar, gpu/oracle and ref/oracle; docs/MEASUREMENTS.md ("EnKF precision") has the table.  Measured on an MI355X: worst
err/bar 0.19 (S, stiff, (2,1)), worst gpu/oracle 4.6 (the posterior P there); nothing fails and nothing is marked."""
import numpy as np
import pytest
import torch

import enkf_hp as hp
from filterpy_amd import _engine as E
from filterpy_amd.kalman import EnsembleKalmanFilter
from test_gpu_enkf import gpu_predict, gpu_update

pytestmark = pytest.mark.gpu

LAYOUTS = ("soa", "aos")
CHUNK = hp.CHUNK
# (6,3) once more with FK_ENKF_GENERAL=1: the general kernel at a shape the fast kernel serves
CASES = [r + (False,) for r in hp.MATRIX] + [r + (True,) for r in hp.MATRIX if (r[1], r[2]) == (6, 3)]
SINGLE_CASES = [r + (False,) for r in hp.SINGLE_ROWS] + [r + (True,) for r in hp.SINGLE_ROWS if (r[1], r[2]) == (6, 3)]


def test_the_chunk_is_the_kernels():
    assert E.ENKF_CHUNK == CHUNK


def _finite(out):
    return all(np.all(np.isfinite(v)) for v in out.values())


def gpu_chain(M, layout):
    """the chained run with F and H fused, feeding on its own state"""
    sig, x, P = M["sig0"], M["x0"], np.eye(M["n"])
    out = {k: [] for k in hp.CHAIN}
    for t in range(M["T"]):
        sig, x, P, st = gpu_predict(sig, x, M["e1"][t], layout, M["F"], m=M["m"])
        assert st == 0, (t, st)
        for k, v in zip(hp.PREDICT, (sig, x, P)):
            out[k].append(v)
        sig, x, P, K, S, SI, st = gpu_update(sig, x, P, M["zs"][t], M["R"], M["e2"][t], layout, M["H"])
        assert st == 0, (t, st)
        for k, v in zip(hp.UPDATE, (sig, x, P, K, S, SI)):
            out[k].append(v)
    return {k: np.array(v) for k, v in out.items()}


def gpu_single(i, path, layout, m):
    """one single step at engine level; behind F=None the pivot is passed as the class passes it"""
    def pred(sig, x, e, F, factor):
        *out, st = gpu_predict(sig, hp.class_pivot(sig) if F is None else x, e, layout, F, factor, m=m)
        assert st == 0
        return out

    def upd(sig, x, P, z, R, e, H, sigmas_h, factor):
        *out, st = gpu_update(sig, x, P, z, R, e, layout, H, sigmas_h, factor)
        assert st == 0
        return out
    return hp.single_run(i, path, pred, upd)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("family,n,m,N,general", CASES)
def test_chained_run_meets_the_bar(monkeypatch, family, n, m, N, general, layout):
    if general:
        monkeypatch.setenv("FK_ENKF_GENERAL", "1")           # read by the dispatch on every call
    t = hp.truth(family, n, m, N)
    hp.measures_something(t)
    out = gpu_chain(t["model"], layout)
    assert _finite(out)
    bad = hp.check(f"gpu{' general' if general else ''} {family} ({n},{m}) N={N} {layout}", hp.errors(out, t["hp"]), t)
    assert not bad, bad
    assert hp.SELF_SCATTER[0] < hp.FLOOR / 100


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("path", hp.SINGLE)
@pytest.mark.parametrize("family,n,m,N,general", SINGLE_CASES)
def test_single_steps_meet_the_bar(monkeypatch, family, n, m, N, general, path, layout):
    """from the truth's rounded state at step 3: the update with sigmas_h given, the predict with F=None (the members already
    moved, the pivot the class's), and the factor path (e = w @ factor(Q), w @ factor(R); on stiff the factor of Q spans
    1e-3 ... 1e-1)"""
    if general:
        monkeypatch.setenv("FK_ENKF_GENERAL", "1")
    t = hp.single_truth(family, n, m, N, path)
    hp.measures_something(t)
    out = gpu_single(t["in"], path, layout, m)
    assert _finite(out)
    bad = hp.check(f"gpu{' general' if general else ''} {path} {family} ({n},{m}) N={N} {layout}", hp.errors(out, t["hp"]), t)
    assert not bad, bad


# ---- the pivot contract: member 0 thirty spreads from the mean (tests/test_host_enkf_hp.py has the figures) -------------------
def _far(n, m, path):
    i = hp.far_member0(hp.single_truth("offset", n, m, CHUNK + 1, path)["in"], path)
    t = hp.single_truth("offset", n, m, CHUNK + 1, path, inputs=i)
    hp.measures_something(t)
    return i, t


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("n,m", [(4, 2), (9, 4)])
def test_pivot_contract_sigmas_h_with_member0_at_30_spreads(n, m, layout):
    i, t = _far(n, m, "sigmas_h")
    out = gpu_single(i, "sigmas_h", layout, m)
    assert _finite(out)
    bad = hp.check(f"gpu sigmas_h member 0 at 30 spreads ({n},{m}) {layout}", hp.errors(out, t["hp"]), t)
    assert not bad, bad


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("n,m", [(4, 2), (9, 4)])
def test_pivot_contract_predict_behind_a_callable_with_member0_at_30_spreads(n, m, layout):
    """through the class: a vectorized fx that leaves the (already moved) members as they are, a `noise` that replays the
    draws -- the ensemble at initialize, then the predict's"""
    i, t = _far(n, m, "moved")
    draws = iter([i["sig"], i["e"]])
    f = EnsembleKalmanFilter(x=i["sig"].mean(axis=0), P=np.eye(n), dim_z=m, dt=1., N=len(i["sig"]), hx=np.eye(m, n),
                             fx=lambda s, dt: s, vectorized=True, noise=lambda mean, cov, N: next(draws).copy(), layout=layout)
    assert np.array_equal(f.sigmas, i["sig"])
    f.predict()
    torch.cuda.synchronize()
    out = {k: np.asarray(v)[None] for k, v in zip(hp.PREDICT, (f.sigmas, f.x, f.P))}
    assert _finite(out)
    bad = hp.check(f"gpu class predict member 0 at 30 spreads ({n},{m}) {layout}", hp.errors(out, t["hp"]), t)
    assert not bad, bad
