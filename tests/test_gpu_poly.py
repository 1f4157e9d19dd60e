"""-m gpu: fk_poly_run (csrc/poly_kernels.hip) through filterpy_amd._engine against the NumPy port (tests/poly_port.py), and the
classes of filterpy_amd.gh / .memory / .leastsq against the live-reference goldens -- everything BITWISE (np.array_equal on
float64).  Every track carries its own state and measurements, so that a lane mix-up shows.

Shapes: N in {1, 63, 64, 65, 129, 1031} (one lane, a wave less one, a wave, a wave and one, two waves and one, more than one
workgroup with a tail); T in {1, 2, 3, 4, 5, 7, 33}: the kernel keeps POLY_DEPTH = 4 measurements in flight, so T = 3, 4 and 5
are depth - 1, depth and depth + 1, 7 leaves a tail of 3 behind a whole round, 33 a tail of 1 behind eight."""
import numpy as np
import pytest

import poly_cases
import poly_port as pp

pytestmark = pytest.mark.gpu
NS = (1, 63, 64, 65, 129, 1031)
TS = (1, 2, 3, 4, 5, 7, 33)
DT, G = 0.3, (0.8, 0.2, 0.05)
_ref = {}


def inputs(order, N, T):
    rs = np.random.RandomState(100 * order + N + 7 * T)
    return rs.randn(order + 1, N), np.cumsum(rs.randn(T, N), axis=0)


def scalars(order, form, T):
    """-> (T2, c, gains table or None for the scalar-gain run)"""
    return DT**2., 0.5 * DT**2, np.array([pp.lsq_gains(order, n + 1, DT) for n in range(T)]).reshape(T, order + 1)


def reference(order, form, N, T, table):
    key = (order, form, N, T, table)
    if key not in _ref:
        x0, zs = inputs(order, N, T)
        T2, c, gains = scalars(order, form, T)
        _ref[key] = pp.run(order, form, x0, zs, DT, T2, c, G, gains if table else None)
    return _ref[key]


def run_gpu(order, form, layout, N, T, table, outs=("xs", "pred", "y")):
    """-> dict of NumPy arrays in the port's shapes: xs (T, c, N), pred, y (T, N), x (c, N) the state left in place"""
    import torch
    from filterpy_amd import _engine as E
    x0, zs = inputs(order, N, T)
    T2, c, gains = scalars(order, form, T)
    C = order + 1
    x = E.dev(x0 if layout == "soa" else np.ascontiguousarray(x0.T))
    z = E.dev(zs)
    bufs = {k: torch.full((T, C, N) if k == "xs" and layout == "soa" else (T, N, C) if k == "xs" else (T, N), float("nan"),
                          dtype=torch.float64, device=x.device) for k in outs}
    E.poly_run(order, form, N, T, layout, DT, T2, c, G[0], G[1], G[2], z, x, gains=E.dev(gains) if table else None,
               xs=bufs.get("xs"), pred=bufs.get("pred"), y=bufs.get("y"))
    torch.cuda.synchronize()
    got = {k: v.cpu().numpy() for k, v in bufs.items()}
    if "xs" in got and layout == "aos":
        got["xs"] = np.swapaxes(got["xs"], 1, 2)
    got["x"] = x.cpu().numpy() if layout == "soa" else x.cpu().numpy().T
    return got


def check(got, ref, what):
    xs, pred, y = ref
    for k, r in (("xs", xs), ("pred", pred), ("y", y)):
        if k in got:
            poly_cases.same(got[k], r, what + (k,))
    poly_cases.same(got["x"], xs[-1], what + ("the final x is the last history row",))


@pytest.mark.parametrize("layout", ("soa", "aos"))
@pytest.mark.parametrize("order,form", pp.COMBOS)
def test_entry_point_equals_the_port_bitwise(order, form, layout):
    for N in NS:
        for T in TS:
            check(run_gpu(order, form, layout, N, T, False), reference(order, form, N, T, False), (order, form, layout, N, T))
    # the gains table, at every phase of the look-ahead
    for T in TS:
        check(run_gpu(order, form, layout, 65, T, True), reference(order, form, 65, T, True), (order, form, layout, 65, T, "table"))
    # each output alone, and none
    for outs in (("xs",), ("pred",), ("y",), ()):
        check(run_gpu(order, form, layout, 129, 7, False, outs), reference(order, form, 129, 7, False), (order, form, layout, outs))


def test_form_b_division_is_numpys():
    """One form-B step with x = dx = 0: r = z exactly and dx' = 0 + (h*z)/dt, so dx' IS the kernel's fp64 division.  4096 tracks
    per launch give h*r random mantissas and exponents in +-200; dt is one scalar per launch, so 16 launches give it 16 random
    mantissas and exponents in +-200.  Bitwise against NumPy: this is the test that decides whether form B can be held to
    the reference's bits on the hardware."""
    import torch
    from filterpy_amd import _abi, _engine as E
    rs = np.random.RandomState(5)
    N, bad = 4096, []
    for launch in range(16):
        dt = float(np.ldexp(1.0 + rs.rand(), rs.randint(-200, 201)) * (1 if launch % 2 else -1))
        h = float(1.0 + rs.rand())
        num = np.ldexp(1.0 + rs.rand(N), rs.randint(-200, 201, N)) * np.where(rs.rand(N) < 0.5, -1.0, 1.0)
        z = num / h                                   # h * z is then a number of num's magnitude with a mantissa of its own
        x = E.dev(np.zeros((2, N)))
        E.poly_run(1, _abi.FK_POLY_FORM_B, N, 1, "soa", dt, 0.0, 0.0, 0.5, h, 0.0, E.dev(z[None]), x)
        torch.cuda.synchronize()
        want = (h * z) / dt
        got = x.cpu().numpy()[1]
        bad.append(int((got != want).sum()))
    assert sum(bad) == 0, "quotients that differ from NumPy's, per launch of 4096: %s" % bad


@pytest.mark.parametrize("check_fn", poly_cases.ALL, ids=lambda f: f.__name__)
def test_classes_equal_the_goldens_bitwise(check_fn):
    check_fn(pp.golden())


def test_device_bank_stays_on_the_device():
    """a bank of 1031 device-tensor tracks stepped 5 times: every attribute and result is a device tensor; only the final
    comparison downloads"""
    import torch
    from filterpy_amd import _engine as E
    from filterpy_amd.gh import GHFilter, GHKFilter, GHFilterOrder
    from filterpy_amd.leastsq import LeastSquaresFilter
    from filterpy_amd.memory import FadingMemoryFilter
    N, T = 1031, 5
    x0, zs = inputs(2, N, T)
    dx0, dz = E.dev(x0), E.dev(zs)

    def on_device(*ts):
        return all(isinstance(t, torch.Tensor) and t.is_cuda for t in ts)
    f = GHFilter(dx0[0].clone(), dx0[1].clone(), DT, G[0], G[1])
    k = GHKFilter(dx0[0].clone(), dx0[1].clone(), dx0[2].clone(), DT, *G)
    o = GHFilterOrder(dx0.clone(), DT, 2, *G)
    m = FadingMemoryFilter(dx0.clone(), DT, 2, 0.7)
    ls = LeastSquaresFilter(DT, 2, n_tracks=N)
    for t in range(T):
        assert on_device(*f.update(dz[t]), f.y, f.x_prediction)
        assert on_device(*k.update(dz[t]), k.ddx, k.y, k.x_prediction, k.dx_prediction)
        o.update(dz[t])
        m.update(dz[t])
        assert on_device(o.x, o.y, m.x, ls.update(dz[t]))
    res, pred = GHFilter(dx0[0].clone(), dx0[1].clone(), DT, G[0], G[1]).batch_filter(dz, save_predictions=True)
    assert on_device(res, pred) and res.shape == (T + 1, N, 2)
    same = poly_cases.same
    same(torch.stack([f.x, f.dx]).cpu().numpy(), pp.run(1, x0=x0[:2], zs=zs, **pp.gh_update(G[0], G[1], DT))[0][-1], "GHFilter")
    same(torch.stack([k.x, k.dx, k.ddx]).cpu().numpy(), pp.run(2, x0=x0, zs=zs, **pp.ghk_update(*G, DT))[0][-1], "GHKFilter")
    same(o.x.cpu().numpy(), pp.run(2, x0=x0, zs=zs, **pp.gh_order(2, *G, DT))[0][-1], "GHFilterOrder")
    same(m.x.cpu().numpy(), pp.run(2, x0=x0, zs=zs, **pp.fading(2, 0.7, DT))[0][-1], "FadingMemoryFilter")
    sc, table = pp.lsq(2, DT, 0, T)
    same(ls.x.cpu().numpy(), pp.run(2, x0=np.zeros((3, N)), zs=zs, gains=table, **sc)[0][-1], "LeastSquaresFilter")
    xs, pr, _ = pp.run(1, x0=x0[:2], zs=zs, **pp.gh_batch(G[0], G[1], DT))
    same(res.cpu().numpy()[1:], np.swapaxes(xs, 1, 2), "GHFilter.batch_filter is the port's form A")
    same(pred.cpu().numpy(), pr, "predictions")
