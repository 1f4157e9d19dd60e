"""The ensemble Kalman filter on the CPU: tests/enkf_port.py against the goldens frozen from the live reference, the member /
slab / finalize arithmetic of filterpy_amd/csrc/fk_enkf.hpp compiled for the host and driven chunk by chunk in the kernels'
order, and the drop-in layer (EnsembleKalmanFilter) on a stand-in engine."""
import os

import numpy as np
import pytest

from conftest import ROOT, rel_err
import enkf_port as ep
import enkf_cases as ec
import enkf_host
from enkf_host import EXACT, hc_predict, hc_update
import fake_enkf_engine
from filterpy_amd.kalman import EnsembleKalmanFilter

G, NC = ec.G, ec.NC
TOL = 1e-10                      # the project's standing bar (tests/conftest.py::rel_err)


# ---- the goldens and the port ---------------------------------------------------------------------------------------------
def test_goldens_cover_what_they_should():
    shapes = [(ep.case(G, ci)["n"], ep.case(G, ci)["m"], ep.case(G, ci)["N"]) for ci in range(NC)]
    assert shapes == [(2, 1, 8), (6, 2, 30), (4, 2, 200), (3, 3, 2), (1, 1, 5), (9, 4, 70), (16, 8, 40)]
    for ci in range(NC):
        c = ep.case(G, ci)
        assert set(c["ops"]) == set(range(6)) and c["ops"][0] == ep.INIT
        assert any(a in (ep.UPDATE, ep.UPDATE_RMAT) and b in (ep.UPDATE, ep.UPDATE_RSCALAR) for a, b in zip(c["ops"], c["ops"][1:]))
    assert np.linalg.matrix_rank(ep.case(G, 0)["Q"]) == 1                   # the reference's singular Q_discrete_white_noise
    assert np.abs(ep.case(G, 2)["x0"]).min() > 900                          # the offset case
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "enkf.npz")) < os.path.getsize(
        os.path.join(ROOT, "tests", "golden", "info.npz"))


def drive(f, c, tol):
    for k, op in enumerate(c["ops"]):
        if k:
            ep.run_op(f, c, k, op, G)
        for a in ep.ATTRS:
            assert rel_err(getattr(f, a), ep.attr(G, c, k, a)) <= tol, (c["p"], k, a, rel_err(getattr(f, a), ep.attr(G, c, k, a)))


@pytest.mark.parametrize("ci", range(NC))
def test_port_matches_golden(ci):
    c = ep.case(G, ci)
    f = ep.Port(c["x0"], c["P0"], c["m"], c["N"], c["F"], c["H"], ep.op_inputs(G, c, 0)["draw"])
    f.Q, f.R = c["Q"], c["R"]
    drive(f, c, 1e-11)


def test_port_one_pass_forms_agree_where_the_data_is_centred():
    rs = np.random.RandomState(3)
    a, b = rs.randn(50, 3), rs.randn(50, 2)
    want = ep.moments(a, a.mean(0), b, b.mean(0))
    for mode in ("shifted", "uncentred"):
        assert rel_err(ep.moments(a, a.mean(0), b, b.mean(0), mode, a[0], b[0]), want) <= 1e-13


# ---- fk_enkf.hpp compiled for the host (the driver and its builds: tests/enkf_host.py) -----------------------------------------
@pytest.fixture(scope="module")
def hc(tmp_path_factory):
    """the padded (16, 8) build (what the general kernel runs) and the exact builds of the fast shapes (tests/enkf_host.py)"""
    return enkf_host.libs(tmp_path_factory)


class HostFilter(ep.Port):
    """the port's interface, computed by one build of the host driver (the fused linear path: F and H go to the members)"""

    def __init__(self, lib, *a):
        self.lib = lib
        super().__init__(*a)

    def predict(self, e):
        self.sigmas, self.x, self.P = hc_predict(self.lib, self.sigmas, self.x, e, self.F)
        self.x_prior, self.P_prior = self.x.copy(), self.P.copy()

    def update(self, z, e=None, R=None):
        if z is not None:
            R = self.R if R is None else R
            R = np.eye(self.m) * R if np.isscalar(R) else R
            *out, st = hc_update(self.lib, self.sigmas, self.x, self.P, z, R, e, self.H)
            assert st == 0
            self.sigmas, self.x, self.P, self.K, self.S, self.SI = out
        self.x_post, self.P_post = self.x.copy(), self.P.copy()


@pytest.mark.parametrize("ci", range(NC))
def test_host_build_of_the_kernel_arithmetic_matches_golden(hc, ci):
    """the padded general shape on every case (the offset case among them), the exact shapes on theirs"""
    c = ep.case(G, ci)
    for dims in [None] + [d for d in EXACT if d == (c["n"], c["m"])]:
        f = HostFilter(hc[dims], c["x0"], c["P0"], c["m"], c["N"], c["F"], c["H"], ep.op_inputs(G, c, 0)["draw"])
        f.Q, f.R = c["Q"], c["R"]
        drive(f, c, TOL)


def _offset_model(n, m, rs, offset=1e3):
    A = rs.randn(n, n)
    return dict(F=np.eye(n) + 0.05 * rs.randn(n, n) / np.sqrt(n), H=rs.randn(m, n) / np.sqrt(n),
                x0=offset * (1.0 + rs.rand(n)) + rs.randn(n), Q=0.01 * (A @ A.T / n + np.eye(n)), R=0.5 * np.eye(m))


@pytest.mark.parametrize("dims,N", [((4, 2), 2 * 2048 + 77), (None, 2048 + 1), ((4, 2), 17 * 2048 + 3), ((4, 2), 2047)])
def test_host_build_over_several_chunks_against_the_port(hc, dims, N):
    """N not a multiple of the chunk, three slabs and more, more slabs than runs (two slabs per run of the finalize): the
    offset-1e3 model against the two-pass port with the same draws; both forms of h; the factor path"""
    lib = hc[dims]
    from filterpy_amd import _engine as E
    assert lib.hc_chunk() == E.ENKF_CHUNK == 2048
    n, m = 4, 2
    rs = np.random.RandomState(N)
    md = _offset_model(n, m, rs)
    sig = md["x0"] + rs.randn(N, n)
    x, P = md["x0"].copy(), np.eye(n)
    A = ep.factor(md["Q"])
    for step in range(2):
        w, e2, z = rs.randn(N, n), rs.randn(N, m) * np.sqrt(0.5), md["H"] @ x + rs.randn(m)
        fac = A if step else None
        e1 = w @ A
        got = hc_predict(lib, sig, x, w if step else e1, md["F"], fac)
        want = ep.predict(sig, e1, md["F"])
        for a, b in zip(got, want):
            assert rel_err(a, b) <= TOL
        sig, x, P = want
        sh = sig @ md["H"].T
        for kw in (dict(H=md["H"]), dict(sigmas_h=sh)):
            *got, st = hc_update(lib, sig, x, P, z, md["R"], e2, **kw)
            want = ep.update(sig, x, P, z, md["R"], e2, **kw)
            assert st == 0
            for a, b in zip(got, want):
                assert rel_err(a, b) <= TOL
        sig, x, P = want[:3]


def test_host_build_flags_a_singular_S(hc):
    rs = np.random.RandomState(5)
    n, m, N = 3, 3, 2
    sig, H = rs.randn(N, n), rs.randn(m, n)
    st = hc_update(hc[None], sig, sig.mean(0), np.eye(n), rs.randn(m), np.zeros((m, m)), np.zeros((N, m)), H)[-1]
    assert st == 1                                            # two members span one direction: S of rank 1, R = 0
    assert hc_update(hc[None], sig, sig.mean(0), np.eye(n), rs.randn(m), np.eye(m), np.zeros((N, m)), H)[-1] == 0


# ---- the Python layer on the stand-in engine ---------------------------------------------------------------------------------
@pytest.fixture
def fake(monkeypatch):
    return fake_enkf_engine.install(monkeypatch)


@pytest.mark.parametrize("layout", ["soa", "aos"])
@pytest.mark.parametrize("mode", ec.MODES)
@pytest.mark.parametrize("ci", range(NC))
def test_class_on_every_golden_case(fake, ci, mode, layout):
    """all attributes and shapes after every call; the `noise` callable is asked at the reference's call sites, in its order"""
    f = ec.run_case(ci, mode, layout, 1e-11)
    fused = mode == "matrix"
    assert all(c[1] == fused and not c[2] for c in fake)
    repr(f)


@pytest.mark.parametrize("ci", [0, 2, 3])
def test_numpy_noise_calls_multivariate_normal_like_the_reference(fake, monkeypatch, ci):
    """noise="numpy": numpy.random.multivariate_normal is called with the recorded (mean, cov, size), once per op, in order"""
    ec.run_case(ci, "callable", "soa", 1e-11, noise_kind="numpy", monkeypatch=monkeypatch)


def test_noise_callable_may_return_a_tensor(fake):
    import torch
    ec.run_case(5, "matrix", "soa", 1e-11, as_tensor=lambda a: torch.as_tensor(a.copy()))


@pytest.mark.parametrize("layout", ["soa", "aos"])
def test_device_noise_hands_standard_normals_and_the_factor_of_the_covariance(fake, layout):
    """noise="device": every draw is torch.randn(generator=) with numpy.random.multivariate_normal's own factor of the
    covariance; the kernel's e = w @ A.  Replayed here from the same seed through the port."""
    import torch
    c = ep.case(G, 0)                                                     # singular Q
    n, m, N = c["n"], c["m"], c["N"]
    gen, gen2 = torch.Generator().manual_seed(7), torch.Generator().manual_seed(7)
    f = EnsembleKalmanFilter(x=c["x0"].copy(), P=c["P0"].copy(), dim_z=m, dt=1., N=N, hx=c["H"], fx=c["F"], noise="device",
                             layout=layout, generator=gen)
    f.Q, f.R = c["Q"], c["R"]

    def w(d):
        t = torch.randn((d, N) if layout == "soa" else (N, d), dtype=torch.float64, generator=gen2).numpy()
        return t.T if layout == "soa" else t
    sig = c["x0"] + w(n) @ ep.factor(c["P0"])
    assert rel_err(f.sigmas, sig) <= 1e-13 and np.array_equal(f.x, c["x0"]) and np.array_equal(f.P, c["P0"])
    f.predict()
    sig, x, P = ep.predict(sig, w(n) @ ep.factor(c["Q"]), c["F"])
    assert rel_err(f.sigmas, sig) <= 1e-13 and rel_err(f.P, P) <= 1e-13
    z = np.array([1.5])
    f.update(z)
    sig, x, P, K, S, SI = ep.update(sig, x, P, z, c["R"], w(m) @ ep.factor(c["R"]), c["H"])
    assert rel_err(f.sigmas, sig) <= 1e-13 and rel_err(f.x, x) <= 1e-13 and rel_err(f.K, K) <= 1e-13
    assert [k[2] for k in fake] == [True, True, True] and [k[0] for k in fake] == ["predict", "predict", "update"]


def test_sigmas_property_and_setter(fake):
    c = ep.case(G, 2)
    f = ec.make_filter(c, "matrix", "soa", ec.Replay(c))
    s = f.sigmas
    assert s.shape == (c["N"], c["n"]) and f.sigmas is s                 # cached until the next step
    s[3] += 1.0                                                          # an in-place edit is NOT seen ...
    assert not np.array_equal(np.asarray(f.sigmas_device).T[3], s[3])
    f.sigmas = s                                                         # ... until the array is assigned back
    assert np.array_equal(np.asarray(f.sigmas_device).T, s) and f.sigmas is not s and np.array_equal(f.sigmas, s)
    with pytest.raises(ValueError):
        f.sigmas = s[:-1]
    rp = f.noise
    rp.k = 1
    f.predict()
    assert f.sigmas is not s and not np.array_equal(f.sigmas, s)


def test_refusals(fake):
    x, P = np.zeros(2), np.eye(2)
    kw = dict(dim_z=1, dt=1., hx=np.eye(1, 2), fx=np.eye(2), noise=lambda mean, cov, N: np.zeros((N, len(mean))) + mean)
    with pytest.raises(ValueError):
        EnsembleKalmanFilter(x, P, N=1, **kw)                            # the reference divides by N - 1
    with pytest.raises(ValueError):
        EnsembleKalmanFilter(x, P, N=0, **kw)
    with pytest.raises(ValueError):
        EnsembleKalmanFilter(x, P, N=4, **dict(kw, dim_z=0))
    with pytest.raises(ValueError):
        EnsembleKalmanFilter(x.reshape(2, 1), P, N=4, **kw)              # x.ndim != 1
    with pytest.raises(ValueError):
        EnsembleKalmanFilter(x, P, N=4, **dict(kw, noise="curand"))
    with pytest.raises(ValueError):
        EnsembleKalmanFilter(x, P, N=4, layout="rows", **kw)
    with pytest.raises(NotImplementedError, match="dim_x <= 16, dim_z <= 8"):
        EnsembleKalmanFilter(np.zeros(17), np.eye(17), N=4, **kw)
    with pytest.raises(NotImplementedError, match="dim_x <= 16, dim_z <= 8"):
        EnsembleKalmanFilter(x, P, N=4, **dict(kw, dim_z=9))
    f = EnsembleKalmanFilter(x, P, N=4, **kw)
    assert f.inv is np.linalg.inv and np.array_equal(f.Q, np.eye(2)) and np.array_equal(f.R, np.eye(1))
    assert f.K.shape == (2, 1) and f.S.shape == f.SI.shape == (1, 1) and f.z.shape == (1, 1) and f.z[0, 0] is None
    assert np.array_equal(f._mean, np.zeros(2)) and np.array_equal(f._mean_z, np.zeros(1)) and f.dt == 1. and f.N == 4
    f.inv = np.linalg.pinv
    with pytest.raises(NotImplementedError):
        f.update(np.array([1.]))
    f.update(None)                                                       # bookkeeping only: no inverse, no refusal
    f.inv = np.linalg.inv
    with pytest.raises(ValueError):
        f.update(np.array([1., 2.]))
    with pytest.raises(np.linalg.LinAlgError):
        f.update(np.array([1.]), R=0.0)                                  # all members equal and R = 0: S = 0
    repr(f)


# ---- the built kernels -------------------------------------------------------------------------------------------------------
def test_fast_kernels_keep_their_sums_in_registers():
    """every exact instantiation of fk_dims_enkf.def: three pass kernels per record order, no scratch memory, and each is a row of
    profiles/enkf/isa.json with the LDS it records"""
    import glob
    import json
    import sys
    import tempfile
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_lint
    objs = sorted(glob.glob(os.path.join(ROOT, "filterpy_amd", "csrc", "build", "inst_enkf_*.o")))
    if not objs:
        pytest.skip("library not built here (the objects do not travel with the .so)")
    recorded = {(r["object"], r["kernel"]): r for r in json.load(open(os.path.join(ROOT, "profiles", "enkf", "isa.json")))["rows"]}
    seen = 0
    with tempfile.TemporaryDirectory() as tmp:
        for o in objs:
            ks = isa_lint.kernels(isa_lint.device_elf(o, tmp))
            assert len(ks) == 6, (o, sorted(ks))
            for name, k in ks.items():
                assert k["scratch"] == 0, (o, name, k)
                r = recorded[(os.path.basename(o), isa_lint.short(name))]
                assert (r["scratch"], r["lds"]) == (k["scratch"], k["lds"]), (name, r, k)
                seen += 1
    assert seen == 24
