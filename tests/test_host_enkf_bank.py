"""EnsembleKalmanFilterBank on the CPU: the drop-in layer on a stand-in engine against the goldens of the live reference's
lockstep loop (tests/golden/enkf_bank.npz), the draw-order contract, the refusals of the class and of the two C-ABI entry
points, and the bank kernels' order of operations -- csrc/fk_enkf.hpp compiled for the host and driven as the two routes of
csrc/enkf_bank.hip drive it (tests/enkf_bank_host.py) -- bit for bit against the single-ensemble driver (tests/enkf_host.py)."""
import ctypes
import os
import struct

import numpy as np
import pytest

from conftest import ROOT
import enkf_port as ep
import enkf_bank_cases as bc
import enkf_host
import enkf_bank_host
from enkf_host import hc_predict, hc_update
from enkf_bank_host import hb_predict, hb_update
import fake_enkf_bank_engine
from filterpy_amd import _abi, _engine as E
from filterpy_amd.kalman import EnsembleKalmanFilterBank

TOL = 1e-10                      # the bar tests/test_gpu_enkf.py holds the single class to on its goldens
LAYOUTS = ("soa", "aos")


# ---- the goldens ------------------------------------------------------------------------------------------------------------
def test_goldens_cover_what_they_should():
    cs = [bc.case(ci) for ci in range(bc.NC)]
    assert [(c["B"], c["n"], c["m"], c["N"], c["shared"]) for c in cs] == [(3, 4, 2, 20, True), (3, 6, 3, 70, False)]
    for c in cs:
        assert c["ops"] == [ep.INIT, ep.PREDICT, ep.UPDATE, bc.UPDATE_MISSING, ep.PREDICT, ep.UPDATE_RMAT, ep.UPDATE_NONE]
        assert bc.op(c, 3, "has_z").tolist() == [True, False, True] and bc.op(c, 3, "drew").tolist() == [True, False, True]
        assert not bc.op(c, 6, "drew").any()
    assert not np.array_equal(cs[1]["F"][0], cs[1]["F"][1]) and not np.array_equal(cs[1]["R"][0], cs[1]["R"][2])
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "enkf_bank.npz")) < 512 * 1024


# ---- 1. the class on a stand-in engine --------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("mode", bc.MODES)
@pytest.mark.parametrize("ci", range(bc.NC))
def test_class_on_every_golden_bank(monkeypatch, ci, mode, layout):
    calls = fake_enkf_bank_engine.install(monkeypatch)
    bc.run_case(ci, mode, layout, TOL)
    c = bc.case(ci)
    # predict, update, update with a track missing (a mask), predict, update with an R override; update(None) launches nothing
    assert [k[0] for k in calls] == ["predict", "update", "update", "predict", "update"]
    assert all(k[1] == (mode == "matrix") and not k[2] for k in calls)          # F / H given or not; the draws as they are
    if mode == "matrix":
        assert all(k[3] == (not c["shared"]) for k in calls)                    # one model for all, or one per track
    assert [k[4] for k in calls if k[0] == "update"] == [None, [1, 0, 1], None]


def test_device_noise_goes_through_the_factors(monkeypatch):
    calls = fake_enkf_bank_engine.install(monkeypatch)
    c = bc.case(1)
    f = bc.make_bank(c, "matrix", "soa", "device")
    f.predict()
    f.update(c["x0"] @ np.swapaxes(c["H"], -1, -2)[0])
    assert [(k[0], k[2], k[3]) for k in calls] == [("predict", True, True)] * 2 + [("update", True, True)]
    # the initial ensembles have the spread asked for: N = 70 draws per track around x0_b with P0_b = c_b I
    f0 = bc.make_bank(c, "matrix", "aos", "device")
    for b in range(c["B"]):
        assert np.abs(f0.sigmas[b].mean(axis=0) - c["x0"][b]).max() < 6 * np.sqrt(c["P0"][b][0, 0] / c["N"])


# ---- 2. the draw-order contract ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ci", range(bc.NC))
def test_seed_alone_reproduces_the_lockstep_loop(monkeypatch, ci):
    """noise="numpy", numpy.random.seed as the golden's loop had it, nothing replayed"""
    fake_enkf_bank_engine.install(monkeypatch)
    bc.run_case(ci, "callable", "soa", TOL, noise_kind="seed")


@pytest.mark.parametrize("mode", ("callable", "matrix"))
def test_numpy_draws_are_asked_for_per_present_track_in_track_order(monkeypatch, mode):
    """the replay stands in numpy.random.multivariate_normal's place and holds every request to the recorded (mean, cov, size)
    of the next track that drew in the reference's loop: a masked track asks for none"""
    fake_enkf_bank_engine.install(monkeypatch)
    bc.run_case(1, mode, "aos", TOL, noise_kind="numpy", monkeypatch=monkeypatch)


def test_a_masked_track_asks_for_no_draw_and_keeps_its_state(monkeypatch):
    fake_enkf_bank_engine.install(monkeypatch)
    c = bc.case(0)
    asked = []

    def noise(mean, cov, N):
        asked.append(np.asarray(mean).copy())
        return np.random.RandomState(len(asked)).multivariate_normal(mean, cov, N)
    f = bc.make_bank(c, "matrix", "soa", noise)
    f.predict()
    before = {a: np.array(getattr(f, a)) for a in ("x", "P", "K", "S", "SI", "sigmas")}
    asked.clear()
    z = f.x @ c["H"][0].T
    f.update(z, mask=[1, 0, 1])
    assert len(asked) == 2
    for a, v in before.items():
        assert np.array_equal(getattr(f, a)[1], v[1]), a
        assert not np.array_equal(getattr(f, a)[0], v[0]), a
    assert all(v is None for v in f.z[1]) and np.array_equal(np.asarray(f.z[0], dtype=float), z[0])
    assert np.array_equal(f.x_post, f.x) and np.array_equal(f.P_post, f.P)
    asked.clear()
    f.update(z, mask=[0, 0, 0])
    f.update(None)
    assert asked == [] and all(v is None for v in f.z.ravel())


# ---- 3. refusals --------------------------------------------------------------------------------------------------------------
def _bank(monkeypatch=None, **kw):
    if monkeypatch is not None:
        fake_enkf_bank_engine.install(monkeypatch)
    a = dict(x=np.zeros(4), P=np.eye(4), dim_z=2, dt=1., N=10, hx=np.eye(2, 4), fx=np.eye(4), n_tracks=3)
    a.update(kw)
    return EnsembleKalmanFilterBank(**a)


def test_class_refusals(monkeypatch):
    fake_enkf_bank_engine.install(monkeypatch)
    with pytest.raises(ValueError, match="at least 2"):
        _bank(N=1)
    with pytest.raises(NotImplementedError, match="EnsembleKalmanFilter"):
        _bank(N=2049)
    _bank(N=2048)
    with pytest.raises(ValueError, match="n_tracks"):
        _bank(n_tracks=0)
    with pytest.raises(NotImplementedError, match="compiled range"):
        _bank(x=np.zeros(17), P=np.eye(17), fx=np.eye(17), hx=np.eye(2, 17))
    with pytest.raises(NotImplementedError, match="compiled range"):
        _bank(dim_z=9, hx=np.eye(9, 4))
    with pytest.raises(ValueError, match="x has shape"):
        _bank(x=np.zeros((2, 4)))
    with pytest.raises(ValueError, match="P has shape"):
        _bank(P=np.eye(3))
    with pytest.raises(ValueError, match="P has shape"):
        _bank(P=np.stack([np.eye(4)] * 2))
    f = _bank()
    with pytest.raises(ValueError, match="z has 2 entries"):
        f.update(np.zeros((2, 2)))
    with pytest.raises(ValueError, match=r"z\[0\] has 3 entries"):
        f.update(np.zeros((3, 3)))
    with pytest.raises(ValueError, match="R has shape"):
        f.update(np.zeros((3, 2)), R=np.eye(3))
    with pytest.raises(ValueError, match="R has shape"):
        f.update(np.zeros((3, 2)), R=np.stack([np.eye(2)] * 2))
    with pytest.raises(ValueError, match="mask has shape"):
        f.update(np.zeros((3, 2)), mask=[1, 1])
    with pytest.raises(ValueError, match="sigmas has shape"):
        f.sigmas = np.zeros((3, 10, 3))
    f.inv = np.linalg.pinv
    with pytest.raises(NotImplementedError, match="inv"):
        f.update(np.zeros((3, 2)))
    f.update(None)                                            # (bookkeeping only: nothing to invert)
    g = _bank(hx=np.eye(3, 4))                                 # (a matrix of the wrong shape is found at the update)
    with pytest.raises(ValueError, match="hx has shape"):
        g.update(np.zeros((3, 2)))


def _raw_desc(n=4, m=2, N=10, mode=0):
    return _abi.fk_kf_desc(n=n, m=m, nu=0, model_mode=mode, N=N, T=1, layout=E.LAYOUTS["soa"], update_first=0, alpha_sq=1.0, flags=0)


def _last_error():
    return _abi.lib().fk_last_error().decode()


def test_abi_refusals_need_no_device():
    """the checks of enkf_dispatch.cpp come before any pointer is read or anything is launched: a non-NULL dummy address serves"""
    lib = _abi.lib()
    buf = (ctypes.c_double * 8)()
    p = ctypes.cast(buf, ctypes.c_void_p)

    def predict(desc, B, sigmas=p):
        return lib.fk_enkf_bank_predict_f64(ctypes.byref(desc), B, None, p, None, sigmas, p, p, None, None)

    def update(desc, B, H=p, sh=None, R=p):
        return lib.fk_enkf_bank_update_f64(ctypes.byref(desc), B, H, sh, R, p, None, p, None, p, p, p, None, None, None, None, None)
    for call in (predict, update):
        assert call(_raw_desc(N=1), 3) == _abi.FK_ERR_BAD_ARG and "N (the ensemble size) must be >= 2" in _last_error()
        assert call(_raw_desc(N=2049), 3) == _abi.FK_ERR_UNSUPPORTED and "must be <= 2048" in _last_error()
        assert call(_raw_desc(), 0) == _abi.FK_ERR_BAD_ARG and "number of ensembles must be >= 1" in _last_error()
        assert call(_raw_desc(), -1) == _abi.FK_ERR_BAD_ARG
        assert call(_raw_desc(n=17), 3) == _abi.FK_ERR_UNSUPPORTED and "compiled range" in _last_error()
        assert call(_raw_desc(mode=E.FK_MODEL_PER_STEP), 3) == _abi.FK_ERR_UNSUPPORTED and "FK_MODEL_SHARED" in _last_error()
    assert predict(_raw_desc(), 3, sigmas=None) == _abi.FK_ERR_BAD_ARG and "must not be NULL" in _last_error()
    assert update(_raw_desc(), 3, R=None) == _abi.FK_ERR_BAD_ARG and "must not be NULL" in _last_error()
    assert update(_raw_desc(), 3, H=p, sh=p) == _abi.FK_ERR_BAD_ARG and "exactly one of H and sigmas_h" in _last_error()
    assert update(_raw_desc(), 3, H=None, sh=None) == _abi.FK_ERR_BAD_ARG and "exactly one of H and sigmas_h" in _last_error()
    assert lib.fk_abi_version() == 4


# ---- 4. the bank kernels' order of operations, compiled for the host ------------------------------------------------------
@pytest.fixture(scope="module")
def hc(tmp_path_factory):
    return enkf_host.libs(tmp_path_factory)


@pytest.fixture(scope="module")
def hb(tmp_path_factory):
    return enkf_bank_host.libs(tmp_path_factory)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).tobytes()


def _model(n, m, rs, offset=30.0):
    A = rs.randn(n, n)
    return dict(F=np.eye(n) + 0.05 * rs.randn(n, n) / np.sqrt(n), H=rs.randn(m, n) / np.sqrt(n),
                x0=offset * (1.0 + rs.rand(n)) + rs.randn(n), Q=0.01 * (A @ A.T / n + np.eye(n)), R=0.5 * np.eye(m) + 0.1)


SIZES = [2, 63, 64, 65, 256, 257, 2047, 2048]


@pytest.mark.parametrize("dims", [(4, 2), (9, 4)])
@pytest.mark.parametrize("N", SIZES)
def test_host_build_of_both_routes_is_bit_identical_to_the_single_driver(hc, hb, dims, N):
    """two chained cycles on the exact build of the shape and on the padded (16, 8) build: fused H and read sigmas_h, the draws
    as they are and through a factor.  Every output, bit for bit."""
    n, m = dims
    rs = np.random.RandomState(100 * N + n)
    md = _model(n, m, rs)
    A, AR = ep.factor(md["Q"]), ep.factor(md["R"])
    for key in (dims, None):
        one, bank = hc[key], hb[key]
        sig, x = md["x0"] + rs.randn(N, n), md["x0"].copy()
        for cycle in range(2):
            w1, w2, z = rs.randn(N, n), rs.randn(N, m), md["H"] @ x + rs.randn(m)
            fac = cycle == 1
            want = hc_predict(one, sig, x, w1, md["F"], A if fac else None)
            got = hb_predict(bank, sig, x, w1, md["F"], A if fac else None)
            assert [_bits(a) for a in got] == [_bits(a) for a in want], (key, N, cycle, "predict")
            sig, x, P = want
            for kw in (dict(sigmas_h=sig @ md["H"].T), dict(H=md["H"])):
                want = hc_update(one, sig, x, P, z, md["R"], w2, factor=AR if fac else None, **kw)
                got = hb_update(bank, sig, x, P, z, md["R"], w2, factor=AR if fac else None, **kw)
                assert want[-1] == got[-1] == 0
                assert [_bits(a) for a in got[:-1]] == [_bits(a) for a in want[:-1]], (key, N, cycle, sorted(kw))
            sig, x, P = want[:3]
            assert np.all(np.isfinite(sig)) and np.all(np.isfinite(P))


@pytest.mark.parametrize("N", [2, 64, 65, 2048])
def test_a_shifted_sum_of_minus_zero_comes_out_as_plus_zero_on_both_drivers(hc, hb, N):
    """component 0 of every member is -0.0 and the centre's is +0.0: every shifted value (-0.0) - (+0.0) is -0.0.  The explicit
    `+ 0.0` steps -- the absent waves of the one-wave route, 0.0 + slab, the fifteen empty runs -- leave +0.0 in the new mean
    where a bare sum of the shifted values would leave -0.0, on the bank's driver as on the single one; the tree with the
    totals alone, fed -0.0 in every lane, gives +0.0 on both routes."""
    n, m = 4, 2
    rs = np.random.RandomState(N)
    sig = 5.0 + rs.randn(N, n)
    sig[:, 0] = -0.0
    x = np.array([0.0, 5.0, 5.0, 5.0])
    H, R = np.zeros((m, n)), np.eye(m)
    H[0, 1] = H[1, 2] = 1.0
    e, z = np.zeros((N, m)), np.array([5.0, 5.0])
    P = np.eye(n)
    P[0, :] = P[:, 0] = 0.0
    want = hc_update(hc[(n, m)], sig, x, P, z, R, e, H=H)
    got = hb_update(hb[(n, m)], sig, x, P, z, R, e, H=H)
    assert [_bits(a) for a in got[:-1]] == [_bits(a) for a in want[:-1]]
    assert got[0][:, 0].tolist() == [0.0] * N                                                  # (row 0 of K is zero)
    assert struct.pack("d", got[1][0]) == struct.pack("d", 0.0)                                # ... their mean is +0.0
    for G in (64, 256):
        assert struct.pack("d", hb[(n, m)].hb_tree(-0.0, G)) == struct.pack("d", 0.0)
        assert hb[(n, m)].hb_tree(1.5, G) == 1.5 * G


# ---- the built kernels -------------------------------------------------------------------------------------------------------
def test_exact_bank_kernels_use_no_scratch_memory():
    """every exact instantiation of enkf_bank.hip: predict and update, both routes, both record orders -- eight kernels per
    shape --, no scratch memory (the sums in VGPRs, the work arrays of enkf_spd_inverse_in in LDS), each a row of
    profiles/enkf/bank_isa.json with the LDS it records; the one-wave route's four ensembles fit 64 KB of LDS in the padded
    kernel too"""
    import glob
    import json
    import sys
    import tempfile
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_lint
    build = os.path.join(ROOT, "filterpy_amd", "csrc", "build")
    objs = sorted(glob.glob(os.path.join(build, "enkf_bank_[0-9]*.o")))
    if not objs:
        pytest.skip("library not built here (the objects do not travel with the .so)")
    recorded = {(r["object"], r["kernel"]): r for r in json.load(open(os.path.join(ROOT, "profiles", "enkf", "bank_isa.json")))["rows"]}
    seen = 0
    with tempfile.TemporaryDirectory() as tmp:
        for o in objs + [os.path.join(build, "enkf_bank_general.o")]:
            ks = isa_lint.kernels(isa_lint.device_elf(o, tmp))
            assert len(ks) == 8, (o, sorted(ks))
            for name, k in ks.items():
                r = recorded[(os.path.basename(o), isa_lint.short(name))]
                assert (r["scratch"], r["lds"]) == (k["scratch"], k["lds"]), (name, r, k)
                assert k["lds"] <= 65536
                if "general" not in o:
                    assert k["scratch"] == 0, (o, name, k)
                    seen += 1
    assert seen == 32
