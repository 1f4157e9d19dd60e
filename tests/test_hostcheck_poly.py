"""The step functions of the polynomial-filter kernels (filterpy_amd/csrc/fk_poly.hpp: poly_step -- the very text
poly_kernels.hip instantiates) compiled for the host and held BIT-IDENTICAL to the live-reference goldens and to the NumPy port,
without a GPU.  The harness (tests/hostcheck/hostcheck_poly.cpp) is built here, into pytest's temporary directory, with
-ffp-contract=off as the device unit is: every line is single IEEE operations."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import poly_cases
import poly_port as pp

HERE = os.path.dirname(os.path.abspath(__file__))
same = poly_cases.same


@pytest.fixture(scope="module")
def hc(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("hostcheck_poly") / "libhostcheck_poly.so")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-w", "-o", so,
                           os.path.join(HERE, "hostcheck", "hostcheck_poly.cpp")])
    lib = ctypes.CDLL(so)
    lib.hc_poly_run.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_long, ctypes.c_long] + [ctypes.c_double] * 3 + [ctypes.c_void_p] * 7
    return lib


def run(hc, order, form, x0, zs, dt, T2=0.0, c=0.0, g=(0.0, 0.0, 0.0), gains=None):
    """the port's run() on the host-compiled step functions: -> xs (T, c, N), pred, y (T, N)"""
    x = np.ascontiguousarray(x0, dtype=np.float64).copy()
    z = np.ascontiguousarray(zs, dtype=np.float64)
    T, N = z.shape
    xs, pred, y = np.full((T, order + 1, N), np.nan), np.full((T, N), np.nan), np.full((T, N), np.nan)
    g3 = np.array(g, dtype=np.float64)
    tab = None if gains is None else np.ascontiguousarray(gains, dtype=np.float64)
    p = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    assert hc.hc_poly_run(order, form, N, T, dt, T2, c, p(g3), p(tab), p(z), p(x), p(xs), p(pred), p(y)) == 0
    same(x, xs[-1], "the state left in place is the last history row")
    return xs, pred, y


def test_host_compiled_steps_equal_the_goldens(hc):
    gold = pp.golden()
    dt, g, h, k, beta, sigma = poly_cases.params(gold)
    zs, x0 = gold["zs"], gold["x0"]
    xs, pred, y = run(hc, 1, x0=x0[:2], zs=zs, **pp.gh_update(g, h, dt))
    same(xs[:, 0], gold["gh_x"], "GHFilter.update x")
    same(xs[:, 1], gold["gh_dx"], "GHFilter.update dx")
    same(pred, gold["gh_xp"], "x_prediction")
    same(y, gold["gh_y"], "y")
    xs, pred, _ = run(hc, 1, x0=x0[:2, :1], zs=zs[:, :1], **pp.gh_batch(g, h, dt))
    same(xs[:, :, 0], gold["gh_batch"][1:], "GHFilter.batch_filter")
    same(pred[:, 0], gold["gh_batch_pred"], "GHFilter.batch_filter predictions")
    xs, pred, y = run(hc, 2, x0=x0, zs=zs, **pp.ghk_update(g, h, k, dt))
    for i, key in enumerate(("x", "dx", "ddx")):
        same(xs[:, i], gold["ghk_" + key], "GHKFilter.update " + key)
    same(pred, gold["ghk_xp"], "GHKFilter x_prediction")
    for order in (0, 1, 2):
        c = order + 1
        xs, _, y = run(hc, order, x0=x0[:c], zs=zs, **pp.gh_order(order, g, h, k, dt))
        same(xs, gold[f"gho{order}_x"], ("GHFilterOrder", order))
        same(y, gold[f"gho{order}_y"], ("GHFilterOrder y", order))
        xs, _, _ = run(hc, order, x0=x0[:c], zs=zs, **pp.fading(order, beta, dt))
        same(xs, gold[f"fm{order}_x"], ("FadingMemoryFilter", order))
        sc, table = pp.lsq(order, dt, 0, len(zs))
        xs, _, _ = run(hc, order, x0=np.zeros((c, 5)), zs=zs, gains=table, **sc)
        same(xs, gold[f"ls{order}_x"], ("LeastSquaresFilter", order))


@pytest.mark.parametrize("order,form", pp.COMBOS)
def test_host_compiled_steps_equal_the_port_on_random_states(hc, order, form):
    """every (order, form), scalar gains and the table, magnitudes from 1e-100 to 1e100 (one magnitude per case: a state, its
    measurements and dt**order of one scale, so that every term of every sum takes part)"""
    rs = np.random.RandomState(31 * order + form)
    N, T = 64, 9
    for exp in (-100, -30, -3, 0, 3, 30, 100):
        scale = 10.0 ** exp
        dt = float(rs.uniform(0.1, 3.0))
        x0 = rs.randn(order + 1, N) * scale
        zs = rs.randn(T, N) * scale
        g = tuple(float(v) for v in rs.uniform(0.05, 0.95, 3))
        gains = rs.uniform(0.05, 0.95, (T, order + 1))
        for table in (None, gains):
            kw = dict(dt=dt, T2=dt**2., c=0.5 * dt**2, g=g, gains=table)
            got, want = run(hc, order, form, x0, zs, **kw), pp.run(order, form, x0, zs, **kw)
            for name, a, b in zip(("xs", "pred", "y"), got, want):
                same(a, b, (order, form, exp, name, table is not None))


def test_unsupported_combinations_are_refused(hc):
    for order, form in ((0, 1), (0, 2), (3, 0), (-1, 0), (1, 3)):
        assert hc.hc_poly_run(order, form, 0, 0, 1., 1., 1., None, None, None, None, None, None, None) == -2
