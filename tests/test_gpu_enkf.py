"""EnsembleKalmanFilter on the GPU: the goldens of the live reference through the class in every way fx / hx can be given and
both layouts, ensemble sizes around every boundary of the kernels against tests/enkf_port.py, bit-identity, the offset case
that tells a centred kernel from an uncentred one, the factor path, noise="device", and the refusals.

Status: all 73 cases pass on the MI355X as written (first hardware run: worst error against the port 1.1e-13, (16,8) at N = 2;
1e-15 ... 1e-14 elsewhere).  The same arithmetic (csrc/fk_enkf.hpp compiled for the host, driven in the kernels' order) passes the
same comparisons at 1e-10 in tests/test_host_enkf.py; tests/test_gpu_enkf_precision.py holds the kernels to a longdouble truth on
hard ensembles, where 1e-10 against a float64 port on benign models would not see four lost digits."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT, rel_err
import enkf_port as ep
import enkf_cases as ec
from filterpy_amd import _abi, _engine as E
from filterpy_amd.kalman import EnsembleKalmanFilter

pytestmark = pytest.mark.gpu

TOL = 1e-10
CHUNK = E.ENKF_CHUNK
LAYOUTS = ("soa", "aos")


def _desc(n, m, N, layout):
    return dict(n=n, m=m, nu=0, model_mode=0, N=N, T=1, layout=E.LAYOUTS[layout], update_first=0, alpha_sq=1.0, flags=0)


def _ws(n, m, N):
    return torch.empty(E.enkf_workspace_bytes(n, m, N), dtype=torch.uint8, device="cuda")


def gpu_predict(sig, x, noise, layout, F=None, factor=None, m=1):
    """E.enkf_predict on host arrays -> sigmas, x, P (host), status.  m: the filter's dim_z (it takes part in the choice of kernel)"""
    N, n = sig.shape
    ds, dn, dx = E.to_records(sig, layout, 0), E.to_records(noise, layout, 0), E.dev(x)
    dP = torch.full((n, n), float("nan"), dtype=torch.float64, device="cuda")
    st = torch.full((1,), -1, dtype=torch.int32, device="cuda")
    E.enkf_predict(_desc(n, m, N, layout), dn, ds, dx, dP, _ws(n, m, N), F=None if F is None else E.dev(F),
                   factor=None if factor is None else E.dev(factor), status=st)
    return E.from_records(ds, layout, 0, (n,)), dx.cpu().numpy(), dP.cpu().numpy(), int(st[0])


def gpu_update(sig, x, P, z, R, noise, layout, H=None, sigmas_h=None, factor=None):
    """E.enkf_update on host arrays -> sigmas, x, P, K, S, SI (host), status"""
    N, n = sig.shape
    m = len(z)
    ds, dn, dx, dP = E.to_records(sig, layout, 0), E.to_records(noise, layout, 0), E.dev(x), E.dev(P)
    S, SI, K = (torch.full(s, float("nan"), dtype=torch.float64, device="cuda") for s in ((m, m), (m, m), (n, m)))
    st = torch.full((1,), -1, dtype=torch.int32, device="cuda")
    E.enkf_update(_desc(n, m, N, layout), E.dev(R), E.dev(z), dn, ds, dx, dP, _ws(n, m, N), H=None if H is None else E.dev(H),
                  sigmas_h=None if sigmas_h is None else E.to_records(sigmas_h, layout, 0),
                  factor=None if factor is None else E.dev(factor), S=S, SI=SI, K=K, status=st)
    return (E.from_records(ds, layout, 0, (n,)), dx.cpu().numpy(), dP.cpu().numpy(), K.cpu().numpy(), S.cpu().numpy(),
            SI.cpu().numpy(), int(st[0]))


def model(n, m, rs, offset=0.0):
    A = rs.randn(n, n)
    return dict(F=np.eye(n) + 0.05 * rs.randn(n, n) / np.sqrt(n), H=rs.randn(m, n) / np.sqrt(n),
                x0=offset * (1.0 + rs.rand(n)) + rs.randn(n), Q=0.01 * (A @ A.T / n + np.eye(n)), R=0.5 * np.eye(m))


def steps(n, m, N, layout, seed, offset=0.0, T=1, report=None):
    """T predict + update cycles at engine level with seeded draws, every output against the port.  The update runs once with
    H (fused) and once with sigmas_h read, from the same state."""
    rs = np.random.RandomState(seed)
    md = model(n, m, rs, offset)
    sig, x, P = md["x0"] + rs.randn(N, n), md["x0"].copy(), np.eye(n)
    worst = 0.0
    for _ in range(T):
        e1, e2 = rs.multivariate_normal(np.zeros(n), md["Q"], N), rs.randn(N, m) * np.sqrt(0.5)
        z = md["H"] @ x + rs.randn(m)
        *got, st = gpu_predict(sig, x, e1, layout, md["F"], m=m)
        want = ep.predict(sig, e1, md["F"])
        assert st == 0
        errs = [rel_err(a, b) for a, b in zip(got, want)]
        sig, x, P = want
        sh = sig @ md["H"].T
        for kw in (dict(H=md["H"]), dict(sigmas_h=sh)):
            *got, st = gpu_update(sig, x, P, z, md["R"], e2, layout, **kw)
            want = ep.update(sig, x, P, z, md["R"], e2, **kw)
            assert st == 0
            errs += [rel_err(a, b) for a, b in zip(got, want)]
        sig, x, P = want[:3]
        worst = max(worst, max(errs))
    print(f"enkf ({n},{m}) N={N} {layout} offset={offset:g}: worst rel err {worst:.2e}")
    assert worst <= TOL, worst
    return worst


# ---- 1. the goldens through the class ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("mode", ec.MODES)
@pytest.mark.parametrize("ci", range(ec.NC))
def test_class_on_every_golden_case(ci, mode, layout):
    ec.run_case(ci, mode, layout, TOL, device="cuda")


def test_class_default_noise_replays_numpy(monkeypatch):
    ec.run_case(1, "callable", "soa", TOL, noise_kind="numpy", monkeypatch=monkeypatch, device="cuda")


# ---- 2. ensemble sizes around every boundary -----------------------------------------------------------------------------
SIZES = [2, 63, 64, 65, 255, 257, CHUNK - 1, CHUNK + 1, 2 * CHUNK + 1, 3 * CHUNK + 5, 17 * CHUNK + 3]


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("dims", [(4, 2), (9, 4)])
def test_ensemble_sizes_around_the_kernel_boundaries(dims, layout):
    """a lane's tail, a wave's, a workgroup's, a chunk's; three slabs and more in the finalize, and more slabs than runs"""
    for N in SIZES:
        steps(dims[0], dims[1], N, layout, seed=N)


def test_general_kernel_sizes():
    for N in (2, 65, CHUNK + 1, 3 * CHUNK + 5):
        steps(5, 2, N, "soa", seed=N)
        steps(16, 8, N, "aos", seed=N + 1)


# ---- 3. bit-identity -----------------------------------------------------------------------------------------------------
def _one_cycle(n, m, N, layout, seed=11):
    rs = np.random.RandomState(seed)
    md = model(n, m, rs, 10.0)
    sig, x = md["x0"] + rs.randn(N, n), md["x0"].copy()
    e1, e2, z = rs.randn(N, n) * 0.1, rs.randn(N, m), md["H"] @ x + rs.randn(m)
    sig, x, P, st = gpu_predict(sig, x, e1, layout, md["F"], m=m)
    out = gpu_update(sig, x, P, z, md["R"], e2, layout, md["H"])
    assert st == 0 and out[-1] == 0
    return dict(sigmas=out[0], x=out[1], P=out[2], K=out[3], S=out[4])


@pytest.mark.parametrize("layout", LAYOUTS)
def test_the_same_call_twice_gives_the_same_bytes(layout):
    a, b = _one_cycle(6, 3, 5 * CHUNK + 17, layout), _one_cycle(6, 3, 5 * CHUNK + 17, layout)
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k


CHILD = r'''
import sys, numpy as np
sys.path.insert(0, %r); sys.path.insert(0, %r)
from test_gpu_enkf import _one_cycle
out = {}
for n, m in ((4, 2), (6, 3)):
    for layout in ("soa", "aos"):
        for k, v in _one_cycle(n, m, 2 * 2048 + 9, layout).items():
            out["%%d_%%d_%%s_%%s" %% (n, m, layout, k)] = v
np.savez(sys.argv[1], **out)
'''


def test_fast_kernel_agrees_with_the_general_one(tmp_path):
    """FK_ENKF_GENERAL=1 in a fresh child process forces the padded rolled kernel"""
    path = str(tmp_path / "general.npz")
    r = subprocess.run([sys.executable, "-c", CHILD % (ROOT, os.path.join(ROOT, "tests")), path],
                       env=dict(os.environ, FK_ENKF_GENERAL="1"), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    gen = np.load(path)
    for n, m in ((4, 2), (6, 3)):
        for layout in LAYOUTS:
            for k, v in _one_cycle(n, m, 2 * CHUNK + 9, layout).items():
                assert rel_err(v, gen[f"{n}_{m}_{layout}_{k}"]) <= TOL, (n, m, layout, k)


# ---- 4. the offset case ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", LAYOUTS)
def test_offset_1e3_at_1025_members(layout):
    """means 1e3 spreads from 0: an uncentred one-pass sum fails this by >= 28x (docs/MEASUREMENTS.md, "EnKF")"""
    steps(6, 3, 1025, layout, seed=5, offset=1e3, T=20)
    steps(16, 8, 1025, layout, seed=6, offset=1e3, T=3)


# ---- 5. the factor path ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", LAYOUTS)
def test_factor_path_with_a_singular_Q(layout):
    c = ep.case(ec.G, 1)                                      # (6, 2): two singular Q_discrete_white_noise blocks
    n, m, N = c["n"], c["m"], 3 * CHUNK + 1
    assert np.linalg.matrix_rank(c["Q"]) == 2
    rs = np.random.RandomState(8)
    A, AR = ep.factor(c["Q"]), ep.factor(c["R"])
    sig, x = c["x0"] + rs.randn(N, n), c["x0"].copy()
    w, w2 = rs.randn(N, n), rs.randn(N, m)
    *got, st = gpu_predict(sig, x, w, layout, c["F"], A, m=m)
    want = ep.predict(sig, w @ A, c["F"])
    assert st == 0 and all(rel_err(a, b) <= TOL for a, b in zip(got, want))
    sig, x, P = want
    z = c["H"] @ x
    *got, st = gpu_update(sig, x, P, z, c["R"], w2, layout, c["H"], factor=AR)
    want = ep.update(sig, x, P, z, c["R"], w2 @ AR, c["H"])
    assert st == 0 and all(rel_err(a, b) <= TOL for a, b in zip(got, want))


# ---- 6. noise="device" ---------------------------------------------------------------------------------------------------
def _device_filter(seed, N=4096):
    c = ep.case(ec.G, 0)
    gen = torch.Generator(device="cuda").manual_seed(seed)
    f = EnsembleKalmanFilter(x=c["x0"].copy(), P=c["P0"].copy(), dim_z=1, dt=1., N=N, hx=c["H"], fx=c["F"], noise="device",
                             generator=gen)
    f.Q, f.R = c["Q"], c["R"]
    f.predict()
    f.update(np.array([0.3]))
    return f


def test_device_noise_same_seed_same_bytes():
    a, b = _device_filter(3), _device_filter(3)
    for k in ("x", "P", "K", "S", "sigmas"):
        assert getattr(a, k).tobytes() == getattr(b, k).tobytes(), k
    assert not np.array_equal(a.sigmas, _device_filter(4).sigmas)
    assert np.all(np.isfinite(a.sigmas)) and a.sigmas.std(axis=0).min() > 0


def test_device_noise_has_the_covariance_asked_for():
    """all members equal, F = I, N = 20000: after one predict every entry of P is within 6 standard deviations of Q, the
    variance being a Gaussian sample covariance's, (Q_ii Q_jj + Q_ij^2) / (N - 1).  The seed is fixed."""
    n, N = 4, 20000
    rs = np.random.RandomState(2)
    B = rs.randn(n, n)
    Q = B @ B.T / n + 0.1 * np.eye(n)
    x = np.array([3., -2., 0.5, 10.])
    f = EnsembleKalmanFilter(x=x, P=np.eye(n), dim_z=2, dt=1., N=N, hx=np.eye(2, n), fx=np.eye(n), noise="device",
                             generator=torch.Generator(device="cuda").manual_seed(1234))
    f.sigmas = np.tile(x, (N, 1))
    f.Q = Q
    f.predict()
    sd = np.sqrt((np.outer(np.diag(Q), np.diag(Q)) + Q ** 2) / (N - 1))
    assert np.all(np.abs(f.P - Q) <= 6 * sd), np.abs(f.P - Q) / sd
    assert np.all(np.abs(f.x - x) <= 6 * np.sqrt(np.diag(Q) / N))
    assert np.abs(f.P - Q).max() > 0


# ---- 7. refusals -------------------------------------------------------------------------------------------------------------
def test_S_not_positive_definite_raises():
    n = m = 3
    rs = np.random.RandomState(1)
    f = EnsembleKalmanFilter(x=rs.randn(n), P=np.eye(n), dim_z=m, dt=1., N=2, hx=np.eye(m), fx=np.eye(n))
    f.R = np.zeros((m, m))                                    # two members span one direction: S has rank 1
    with pytest.raises(np.linalg.LinAlgError):
        f.update(rs.randn(m))


def test_short_workspace_is_refused():
    n, N = 4, 100
    sig, noise, x, P = (torch.zeros(s, dtype=torch.float64, device="cuda") for s in ((n, N), (n, N), (n,), (n, n)))
    ws = _ws(n, 2, N)
    with pytest.raises(_abi.FilterHipError) as ei:
        E.enkf_predict(_desc(n, 2, N, "soa"), noise, sig, x, P, ws, workspace_bytes=ws.numel() - 8)
    assert ei.value.code == _abi.FK_ERR_WORKSPACE
    E.enkf_predict(_desc(n, 2, N, "soa"), noise, sig, x, P, ws)
    torch.cuda.synchronize()
