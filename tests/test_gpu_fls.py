"""The fixed-lag smoother on the GPU (fk_fls_batch_f64, csrc/fls_kernels.hip) against the goldens frozen from the live reference:
every case through FixedLagSmoother, FixedLagSmootherBank and the ABI in both layouts; a 70 001-track bank against
tests/fls_port.py; the fast kernel against the general one (forced in a child process); chained calls bit-identical to one."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, golden, rel_err_rows
import fls_port
from filterpy_amd.kalman import FixedLagSmoother, FixedLagSmootherBank

pytestmark = pytest.mark.gpu

G = golden("fls")
NC = int(G["n_cases"])
TOL = 1e-10


def case(ci):
    p = f"c{ci}_"
    n, m, lag, nd, ctrl, scal, zsc = (int(v) for v in G[p + "spec"])
    d = dict(n=n, m=m, lag=lag, nd=nd, ctrl=ctrl, scal=scal, zsc=zsc)
    for k in ("F", "Q", "H", "R", "P0", "x0", "zs", "xs", "xhat", "us", "B"):
        if p + k in G.files:
            d[k] = G[p + k]
    for k in ("Q", "R", "B"):
        if k in d and d[k].ndim == 0:
            d[k] = float(d[k])
    return d


def ref_inputs(c):
    n, m, T = c["n"], c["m"], c["zs"].shape[0]
    x0 = c["x0"].copy() if c["nd"] == 1 else c["x0"].reshape(n, 1).copy()
    zs = c["zs"][:, 0] if c["zsc"] else (c["zs"] if c["nd"] == 1 else c["zs"].reshape(T, m, 1))
    us = None
    if "us" in c:
        us = c["us"] if c["nd"] == 1 else c["us"].reshape(T, -1, 1)
    return x0, zs, us, c.get("B", 0.)


@pytest.mark.parametrize("ci", range(NC))
def test_golden_cases_single_and_bank(ci):
    c = case(ci)
    n, m, T = c["n"], c["m"], c["zs"].shape[0]
    x0, zs, us, B = ref_inputs(c)
    f = FixedLagSmoother(n, m)
    f.F, f.H, f.P, f.Q, f.R, f.x, f.B = c["F"], c["H"], c["P0"], c["Q"], c["R"], x0, B
    xs, xhat = f.smooth_batch(zs, c["lag"], us=us)
    assert xs.shape == c["xs"].shape
    assert rel_err_rows(xs, c["xs"]) <= TOL and rel_err_rows(xhat, c["xhat"]) <= TOL
    Nt = 3
    for layout in ("soa", "aos"):
        b = FixedLagSmootherBank(n, m, Nt, layout=layout)
        b.F, b.H, b.P, b.Q, b.R = c["F"], c["H"], np.broadcast_to(c["P0"], (Nt, n, n)), c["Q"], c["R"]
        b.x = np.tile(c["x0"], (Nt, 1))
        bus = None
        if "us" in c:
            b.B = c["B"]
            bus = np.repeat(c["us"][:, None, :], Nt, axis=1)
        bx, bh = b.smooth_batch(np.repeat(c["zs"][:, None, :], Nt, axis=1), c["lag"], us=bus)
        for i in range(Nt):
            assert rel_err_rows(bx[:, i], c["xs"].reshape(T, n)) <= TOL, layout
            assert rel_err_rows(bh[:, i], c["xhat"].reshape(T, n)) <= TOL, layout


def test_smooth_sequences_attributes():
    for si, (n, m, lag, nd, ctrl) in enumerate(G["seqs"]):
        p = f"s{si}_"
        f = FixedLagSmoother(int(n), int(m), N=int(lag))
        f.F, f.Q, f.H, f.R, f.P = G[p + "F"], G[p + "Q"], G[p + "H"], G[p + "R"], G[p + "P0"]
        f.x = G[p + "x0"].copy() if nd == 1 else G[p + "x0"].reshape(n, 1).copy()
        if p + "B" in G.files:
            f.B = G[p + "B"] if G[p + "B"].ndim else float(G[p + "B"])
        for k in range(G[p + "zs"].shape[0]):
            z = G[p + "zs"][k] if nd == 1 else G[p + "zs"][k].reshape(m, 1)
            u = None
            if p + "us" in G.files:
                u = G[p + "us"][k] if nd == 1 else G[p + "us"][k].reshape(-1, 1)
            f.smooth(z, u)
            q = f"{p}k{k}_"
            assert f.count == k + 1
            assert rel_err_rows(np.array(f.xSmooth), G[q + "xSmooth"]) <= TOL
            for a in ("x", "P", "y", "S"):
                assert np.shape(getattr(f, a)) == G[q + a].shape, a
                assert rel_err_rows(np.atleast_2d(getattr(f, a)), np.atleast_2d(G[q + a])) <= TOL, a


def _bank_inputs(n, m, Nt, T, seed):
    rs = np.random.RandomState(seed)
    F = np.eye(n) + 0.1 * rs.randn(n, n) / np.sqrt(n)
    A = rs.randn(n, n)
    Q = 0.01 * (A @ A.T + np.eye(n))
    H = rs.randn(m, n)
    R = np.eye(m) * 0.8
    x0 = rs.randn(Nt, n)
    P0 = np.eye(n)[None] * (1.0 + rs.rand(Nt, 1, 1))
    zs = rs.randn(T, Nt, m)
    return F, Q, H, R, x0, P0, zs


@pytest.mark.parametrize("layout", ["soa", "aos"])
def test_large_bank_per_track_state_vs_port(layout):
    n, m, Nt, T, lag = 4, 2, 70001, 24, 8
    F, Q, H, R, x0, P0, zs = _bank_inputs(n, m, Nt, T, 11)
    b = FixedLagSmootherBank(n, m, Nt, layout=layout)
    b.F, b.Q, b.H, b.R, b.x, b.P = F, Q, H, R, x0, P0
    xs, xhat = b.smooth_batch(zs, lag)
    for i in (0, 1, 63, 64, 255, 256, 35000, Nt - 2, Nt - 1):
        a = fls_port.smooth_batch(x0[i], P0[i], zs[:, i], lag, F, Q, H, R)
        assert rel_err_rows(xs[:, i], a[0]) <= TOL and rel_err_rows(xhat[:, i], a[1]) <= TOL, i


CHILD = r'''
import sys, numpy as np
sys.path.insert(0, %r); sys.path.insert(0, %r)
from test_gpu_fls import _bank_inputs
from filterpy_amd.kalman import FixedLagSmootherBank
out = {}
for (n, m, lag) in ((1, 1, 16), (2, 1, 3), (3, 2, 16), (4, 2, 8), (5, 3, 8), (4, 2, 0)):
    for layout in ("soa", "aos"):
        F, Q, H, R, x0, P0, zs = _bank_inputs(n, m, 1000, 30, n * 10 + m)
        b = FixedLagSmootherBank(n, m, 1000, layout=layout)
        b.F, b.Q, b.H, b.R, b.x, b.P = F, Q, H, R, x0, P0
        xs, xh = b.smooth_batch(zs, lag)
        out["%%d_%%d_%%d_%%s_xs" %% (n, m, lag, layout)] = xs
        out["%%d_%%d_%%d_%%s_xh" %% (n, m, lag, layout)] = xh
np.savez(sys.argv[1], **out)
'''


def test_fast_kernel_matches_general_kernel(tmp_path):
    res = {}
    for general in ("0", "1"):
        out = tmp_path / f"g{general}.npz"
        env = dict(os.environ, FK_FLS_GENERAL=general)
        r = subprocess.run([sys.executable, "-c", CHILD % (ROOT, os.path.join(ROOT, "tests")), str(out)], env=env,
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        res[general] = np.load(out)
    for k in res["0"].files:
        assert rel_err_rows(res["0"][k], res["1"][k]) <= 1e-13, k


@pytest.mark.parametrize("n,m,lag", [(4, 2, 8), (4, 2, 20), (9, 3, 5), (3, 2, 1)])
@pytest.mark.parametrize("layout", ["soa", "aos"])
def test_chained_calls_are_bit_identical(n, m, lag, layout):
    Nt, T = 513, 17
    F, Q, H, R, x0, P0, zs = _bank_inputs(n, m, Nt, T, 5)
    b = FixedLagSmootherBank(n, m, Nt, N=lag, layout=layout)
    b.F, b.Q, b.H, b.R, b.x, b.P = F, Q, H, R, x0, P0
    xs, xhat = b.smooth_batch(zs, lag)
    for t in range(T):
        b.smooth(zs[t])
    assert np.array_equal(b.xSmooth, xs)
    # two chained ABI calls: steps 0..6 then 7..16, the pending window carried through
    from filterpy_amd import _engine as E
    from filterpy_amd.kalman.fixed_lag_smoother import _run, _model
    Fm, Qm, Hm, Rm, fl = _model(F, Q, H, R, n, m)
    t1 = 7
    xs1, xh1, dx, dP, _, _ = _run(n, m, Nt, layout, lag, 0, x0, P0, zs[:t1], Fm, Qm, Hm, Rm, fl)
    W = min(max(lag, 1) - 1, t1)
    xs2, xh2, *_ = _run(n, m, Nt, layout, lag, t1, dx, dP, zs[t1:], Fm, Qm, Hm, Rm, fl, pend=xs1[t1 - W:].clone())
    got = np.concatenate([E.host_records(xs1[:t1 - W].cpu().numpy(), layout, 1, (n,)),
                          E.host_records(xs2.cpu().numpy(), layout, 1, (n,))])
    assert np.array_equal(got, xs)
    assert np.array_equal(np.concatenate([E.host_records(xh1.cpu().numpy(), layout, 1, (n,)),
                                          E.host_records(xh2.cpu().numpy(), layout, 1, (n,))]), xhat)


def test_non_pd_S_raises_and_device_outputs():
    f = FixedLagSmoother(2, 2)            # S = F P F' + Q - 10 I = -8 I: the L D L' factorisation fails (dim_z = 1 divides)
    f.R = -10.0 * np.eye(2)
    with pytest.raises(np.linalg.LinAlgError):
        f.smooth_batch(np.ones((4, 2, 1)), 2)
    import torch
    n, m, Nt, T = 3, 2, 300, 6
    F, Q, H, R, x0, P0, zs = _bank_inputs(n, m, Nt, T, 9)
    for layout in ("soa", "aos"):
        b = FixedLagSmootherBank(n, m, Nt, layout=layout)
        b.F, b.Q, b.H, b.R, b.x, b.P = F, Q, H, R, x0, P0
        xs, xh = b.smooth_batch(zs, 2, device_outputs=True)
        assert isinstance(xs, torch.Tensor) and xs.is_cuda
        assert tuple(xs.shape) == ((T, Nt, n) if layout == "aos" else (T, n, Nt))
        hx, hh = b.smooth_batch(zs, 2)
        from filterpy_amd import _engine as E
        assert np.array_equal(E.host_records(xs.cpu().numpy(), layout, 1, (n,)), hx)
