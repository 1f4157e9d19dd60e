"""The fixed-gain polynomial filters without a GPU: the NumPy port (tests/poly_port.py) against the live-reference goldens and
against the live reference itself, the Python classes on a stand-in engine that calls the port (tests/fake_poly_engine.py), and
the entry point's refusals.  Everything is bit for bit."""
import ctypes
import os
import sys

import numpy as np
import pytest

import fake_poly_engine
import poly_cases
import poly_port as pp

REF = os.environ.get("FILTERPY_REFERENCE", "/root/reference")
same = poly_cases.same


@pytest.fixture(scope="module")
def gold():
    return pp.golden()


# ------------------------------------------------------------------------------------------------ the port and the goldens
def test_port_equals_the_goldens(gold):
    dt, g, h, k, beta, sigma = poly_cases.params(gold)
    zs, x0 = gold["zs"], gold["x0"]
    xs, pred, y = pp.run(1, x0=x0[:2], zs=zs, **pp.gh_update(g, h, dt))
    same(xs[:, 0], gold["gh_x"], "GHFilter.update x")
    same(xs[:, 1], gold["gh_dx"], "GHFilter.update dx")
    same(pred, gold["gh_xp"], "x_prediction")
    same(y, gold["gh_y"], "y")
    xs, pred, y = pp.run(1, x0=x0[:2, :1], zs=zs[:, :1], **pp.gh_batch(g, h, dt))
    same(xs[:, :, 0], gold["gh_batch"][1:], "GHFilter.batch_filter")
    same(pred[:, 0], gold["gh_batch_pred"], "GHFilter.batch_filter predictions")
    xs, pred, y = pp.run(2, x0=x0, zs=zs, **pp.ghk_update(g, h, k, dt))
    for i, key in enumerate(("x", "dx", "ddx")):
        same(xs[:, i], gold["ghk_" + key], "GHKFilter.update " + key)
    same(pred, gold["ghk_xp"], "GHKFilter x_prediction")
    same(y, gold["ghk_y"], "GHKFilter y")
    for order in (0, 1, 2):
        c = order + 1
        xs, _, y = pp.run(order, x0=x0[:c], zs=zs, **pp.gh_order(order, g, h, k, dt))
        same(xs, gold[f"gho{order}_x"], ("GHFilterOrder", order))
        same(y, gold[f"gho{order}_y"], ("GHFilterOrder y", order))
        xs, _, _ = pp.run(order, x0=x0[:c], zs=zs, **pp.fading(order, beta, dt))
        same(xs, gold[f"fm{order}_x"], ("FadingMemoryFilter", order))
        sc, table = pp.lsq(order, dt, 0, len(zs))
        same(table, gold[f"ls{order}_K"], ("LeastSquaresFilter.K", order))
        xs, _, _ = pp.run(order, x0=np.zeros((c, 5)), zs=zs, gains=table, **sc)
        same(xs, gold[f"ls{order}_x"], ("LeastSquaresFilter", order))
    # the per-call gain override: a run of single steps, each with its own scalars
    s = x0[:2].copy()
    for t, z in enumerate(zs):
        xs, _, _ = pp.run(1, x0=s, zs=z[None], **pp.gh_update(*gold["gh_override_gains"][t], dt))
        s = xs[-1]
        same(s, gold["gh_override_x"][t], ("override", t))


def test_port_equals_the_live_reference_on_fresh_cases():
    if not os.path.isdir(os.path.join(REF, "filterpy")):
        pytest.skip("no reference checkout here")
    sys.path.insert(0, REF)
    try:
        from filterpy.gh import GHFilter, GHKFilter, GHFilterOrder
        from filterpy.leastsq import LeastSquaresFilter
        from filterpy.memory import FadingMemoryFilter
    finally:
        sys.path.remove(REF)
    rng = np.random.default_rng(7)
    for case in range(6):
        N, T = 7, 11
        dt, g, h, k, beta = (float(v) for v in rng.uniform(0.05, 0.95, 5))
        zs = rng.normal(size=(T, N)) * 10.0 ** rng.integers(-3, 4)
        x0 = rng.normal(size=(3, N))
        f = GHFilter(x0[0].copy(), x0[1].copy(), dt, g, h)
        xs, pred, y = pp.run(1, x0=x0[:2], zs=zs, **pp.gh_update(g, h, dt))
        for t, z in enumerate(zs):
            f.update(z)
            same(xs[t], [f.x, f.dx], ("GHFilter", case, t))
        res = np.array([GHFilter(float(x0[0, i]), float(x0[1, i]), dt, g, h).batch_filter(zs[:, i]) for i in range(N)])
        xs, _, _ = pp.run(1, x0=x0[:2], zs=zs, **pp.gh_batch(g, h, dt))
        same(np.moveaxis(xs, 2, 0), res[:, 1:], ("GHFilter.batch_filter", case))
        f = GHKFilter(x0[0].copy(), x0[1].copy(), x0[2].copy(), dt, g, h, k)
        xs, _, _ = pp.run(2, x0=x0, zs=zs, **pp.ghk_update(g, h, k, dt))
        for t, z in enumerate(zs):
            f.update(z)
            same(xs[t], [f.x, f.dx, f.ddx], ("GHKFilter", case, t))
        for order in (0, 1, 2):
            c = order + 1
            f, m = GHFilterOrder(x0[:c].copy(), dt, order, g, h, k), FadingMemoryFilter(x0[:c].copy(), dt, order, beta)
            ls = [LeastSquaresFilter(dt, order) for _ in range(N)]
            xo, _, _ = pp.run(order, x0=x0[:c], zs=zs, **pp.gh_order(order, g, h, k, dt))
            xm, _, _ = pp.run(order, x0=x0[:c], zs=zs, **pp.fading(order, beta, dt))
            sc, table = pp.lsq(order, dt, 0, T)
            xl, _, _ = pp.run(order, x0=np.zeros((c, N)), zs=zs, gains=table, **sc)
            for t, z in enumerate(zs):
                f.update(z)
                m.update(z)
                same(xo[t], f.x, ("GHFilterOrder", case, order, t))
                same(xm[t], m.x, ("FadingMemoryFilter", case, order, t))
                same(xl[t], np.stack([l.update(z[i]).copy() for i, l in enumerate(ls)], axis=1), ("LeastSquaresFilter", case, order, t))


# ------------------------------------------------------------------------------------- the classes on the stand-in engine
@pytest.mark.parametrize("check", poly_cases.ALL, ids=lambda f: f.__name__)
def test_classes_equal_the_goldens_on_the_stand_in_engine(monkeypatch, gold, check):
    fake_poly_engine.install(monkeypatch)
    check(gold)


def test_routes_and_launch_counts(monkeypatch, gold):
    """which (order, form) each method runs, that a batch is ONE launch, and what the launch is asked to write"""
    from filterpy_amd.gh import GHFilter, GHKFilter, GHFilterOrder
    from filterpy_amd.leastsq import LeastSquaresFilter
    from filterpy_amd.memory import FadingMemoryFilter
    calls = fake_poly_engine.install(monkeypatch)
    zs, x0 = gold["zs"], gold["x0"]

    def last():
        c = calls[-1]
        return c["order"], c["form"], c["N"], c["T"], c["layout"], c["table"], c["outs"]
    f = GHFilter(x0[0].copy(), x0[1].copy(), 0.3, 0.8, 0.2)
    f.update(zs[0])
    assert last() == (1, pp.FORM_B, 5, 1, "soa", False, ("pred", "y"))
    f.batch_filter(zs)
    assert last() == (1, pp.FORM_A, 5, 24, "aos", False, ("xs",)) and len(calls) == 2
    assert calls[-1]["scalars"][3:5] == (0.8, 0.2 / 0.3)
    f = GHKFilter(x0[0].copy(), x0[1].copy(), x0[2].copy(), 0.3, 0.8, 0.2, 0.05)
    f.update(zs[0])
    assert last() == (2, pp.FORM_B, 5, 1, "soa", False, ("pred", "y")) and calls[-1]["scalars"][:2] == (0.3, 0.3**2)
    assert calls[-1]["scalars"][3:] == (0.8, 0.2, 2 * 0.05)
    f.batch_filter(zs, save_predictions=True)
    assert last() == (1, pp.FORM_A, 5, 24, "aos", False, ("xs", "pred"))
    for order, form in ((0, pp.FORM_A), (1, pp.FORM_B), (2, pp.FORM_B)):
        n = len(calls)
        GHFilterOrder(x0[:order + 1].copy(), 0.3, order, 0.8, 0.2, 0.05).batch_filter(zs)
        assert last()[:4] == (order, form, 5, 24) and len(calls) == n + 1
        FadingMemoryFilter(x0[:order + 1].copy(), 0.3, order, 0.7).batch_filter(zs)
        assert last()[:4] == (order, pp.FORM_A, 5, 24) and len(calls) == n + 2
        ls = LeastSquaresFilter(0.3, order, n_tracks=5)
        ls.batch_filter(zs)
        assert last()[:6] == (order, pp.FORM_A if order == 0 else pp.FORM_C, 5, 24, "soa", True) and len(calls) == n + 3
        ls.update(zs[0])
        assert last()[3:6] == (1, "soa", False) and ls.n == 25


def test_saver_is_called_once_per_step_on_the_unchanged_object(monkeypatch, gold):
    from filterpy_amd.gh import GHFilter
    fake_poly_engine.install(monkeypatch)

    class Saver:
        def __init__(self, f):
            self.f, self.seen = f, []

        def save(self):
            self.seen.append((self.f.x, self.f.dx))
    f = GHFilter(1.0, 0.5, 0.3, 0.8, 0.2)
    s = Saver(f)
    f.batch_filter(gold["zs"][:, 0], saver=s)
    assert s.seen == [(1.0, 0.5)] * 24


def test_refusals_and_shapes(monkeypatch, gold):
    import torch
    from filterpy_amd.gh import GHFilter, GHKFilter, GHFilterOrder, critical_damping_parameters
    from filterpy_amd.leastsq import LeastSquaresFilter
    from filterpy_amd.memory import FadingMemoryFilter
    fake_poly_engine.install(monkeypatch)
    for order in (-1, 3):
        for make in (lambda: GHFilterOrder(0., 1., order, 0.5), lambda: FadingMemoryFilter(0., 1., order, 0.5),
                     lambda: LeastSquaresFilter(1., order)):
            with pytest.raises(ValueError, match="order must be between 0 and 2"):
                make()
    with pytest.raises(ValueError, match="theta must be between 0 and 1"):
        critical_damping_parameters(1.5)
    with pytest.raises(ValueError, match="bad order specified: 4"):
        critical_damping_parameters(0.5, 4)
    per_track = np.full(5, 0.5)
    f = GHFilter(np.zeros(5), np.zeros(5), 1., 0.5, 0.1)
    with pytest.raises(NotImplementedError):
        f.update(np.ones(5), g=per_track)
    with pytest.raises(NotImplementedError):
        GHFilter(np.zeros(5), np.zeros(5), 1., per_track, 0.1).batch_filter(np.ones((3, 5)))
    with pytest.raises(NotImplementedError):
        GHKFilter(np.zeros(5), np.zeros(5), np.zeros(5), 1., 0.5, 0.1, 0.01).update(np.ones(5), k=per_track)
    with pytest.raises(NotImplementedError):
        GHFilterOrder(np.zeros((2, 5)), 1., 1, 0.5, per_track).update(np.ones(5))
    with pytest.raises(NotImplementedError):
        FadingMemoryFilter(np.zeros((2, 5)), 1., 1, per_track).update(np.ones(5))
    with pytest.raises(ValueError):
        GHFilterOrder(np.zeros((2, 5)), 1., 1, 0.5, 0.1).batch_filter(np.ones((3, 4)))
    # a number as x0: zeros for the higher components; tensors in, tensors out
    f = GHFilterOrder(2.5, 1., 2, 0.5, 0.1, 0.01)
    assert f.x.tolist() == [2.5, 0., 0.] and f.y.shape == (3,) and f.z.shape == (3,)
    t = GHFilter(torch.zeros(4, dtype=torch.float64), torch.ones(4, dtype=torch.float64), 0.5, 0.5, 0.1)
    x, dx = t.update(torch.ones(4, dtype=torch.float64))
    assert isinstance(x, torch.Tensor) and isinstance(t.y, torch.Tensor) and isinstance(t.x_prediction, torch.Tensor)
    res = t.batch_filter(torch.ones(3, 4, dtype=torch.float64))
    assert isinstance(res, torch.Tensor) and res.shape == (4, 4, 2)
    n = GHFilter(np.zeros(4), np.ones(4), 0.5, 0.5, 0.1)
    assert isinstance(n.batch_filter(np.ones((3, 4))), np.ndarray)
    assert isinstance(n.batch_filter(np.ones((3, 4)), device_outputs=True), torch.Tensor)
    ls = LeastSquaresFilter(0.5, 1, n_tracks=4)
    assert isinstance(ls.update(torch.ones(4, dtype=torch.float64)), torch.Tensor) and ls.x.shape == (2, 4)
    assert "GHFilter object" in repr(n) and "LeastSquaresFilter object" in repr(ls) and "x_prediction = " in repr(n)


def test_forms_b_and_c_refuse_order_zero_without_a_device():
    from filterpy_amd import _abi
    lib = _abi.lib()
    one = ctypes.c_void_p(8)

    def call(order, form, N=1, T=1, layout=1, z=one, x=one):
        return lib.fk_poly_run(order, form, N, T, layout, 1., 1., .5, .5, .1, .01, None, z, x, None, None, None, None)
    for form in (_abi.FK_POLY_FORM_B, _abi.FK_POLY_FORM_C):
        assert call(0, form) == _abi.FK_ERR_UNSUPPORTED and b"order" in lib.fk_last_error()
    for order, form in ((3, 0), (-1, 0), (1, 3), (1, -1), (3, 1)):
        assert call(order, form) == _abi.FK_ERR_UNSUPPORTED, (order, form)
    assert call(1, 1, N=-1) == _abi.FK_ERR_BAD_ARG and call(1, 1, T=-1) == _abi.FK_ERR_BAD_ARG
    assert call(1, 1, layout=2) == _abi.FK_ERR_BAD_ARG
    assert call(1, 1, z=None) == _abi.FK_ERR_BAD_ARG and call(1, 1, x=None) == _abi.FK_ERR_BAD_ARG
    assert call(1, 1, N=0, z=None, x=None) == _abi.FK_OK and call(2, 2, T=0, z=None, x=None) == _abi.FK_OK
