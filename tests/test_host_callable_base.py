"""The host plumbing the callable-model filters share (filterpy_amd/kalman/_callable.py) and the base of the two ensemble
classes (ensemble_kalman_filter.py: _Ensemble), alone and on CPU tensors: the two directions between (N, k, d) blocks and device
records in both layouts at shapes that tell every axis apart (N = 3, k = 2, d = 3; and N = 1), and the refusals of
UnscentedKalmanFilter, CubatureKalmanFilter and ExtendedKalmanFilter word for word as each class has always raised them."""
import numpy as np
import pytest
import torch

import fake_kf_engine
from filterpy_amd import _engine as E
from filterpy_amd.kalman import (CubatureKalmanFilter, EnsembleKalmanFilter, EnsembleKalmanFilterBank, ExtendedKalmanFilter,
                                 MerweScaledSigmaPoints, UnscentedKalmanFilter)
from filterpy_amd.kalman import _callable as C

K, D = 2, 3
LAYOUTS = ("soa", "aos")


@pytest.fixture(autouse=True)
def cpu_engine(monkeypatch):
    fake_kf_engine.install(monkeypatch)


def blocks(N, k=K, d=D):
    return np.arange(N * k * d, dtype=np.float64).reshape(N, k, d) + 0.5


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("N", (3, 1))
def test_to_rec_and_rec_view_are_inverse_and_agree_with_the_engine(N, layout):
    a = blocks(N)
    t = torch.as_tensor(a)
    want = E.to_records(a.reshape(N, K * D), layout, 0)
    assert tuple(want.shape) == ((K * D, N) if layout == "soa" else (N, K * D))
    view = None
    for given, tensor in ((t, True), (a, False), (a.tolist(), False)):
        rec = C.to_rec(given, N, (K, D), layout, tensor)
        assert rec.is_contiguous() and rec.shape == want.shape and torch.equal(rec, want)
        view = C.rec_view(rec, N, K, D, layout)
        assert view.data_ptr() == rec.data_ptr() and torch.equal(view, t)                  # a view, and the callable's tensor
    assert torch.equal(C.to_rec(view, N, (K, D), layout, True), want)                      # strided, as a callable gets it
    assert torch.equal(C.as_records(t[:, 0], N, layout), E.to_records(a[:, 0], layout, 0))  # (N, d): one vector per track
    assert torch.equal(C.as_records(t, N, layout), want)
    rows = C.track_rows(E.to_records(a[:, 0], layout, 0), layout)                          # ... and back, as a callable takes x
    assert rows.is_contiguous() and torch.equal(rows, t[:, 0])


@pytest.mark.parametrize("layout", LAYOUTS)
def test_histories_and_status(layout):
    T, N, n = 2, 3, 2
    outs = C.alloc_histories(T, N, n, layout)
    assert [tuple(o.shape) for o in outs] == [(T, N, e) if layout == "aos" else (T, e, N) for e in (n, n * n, n, n * n)]
    vals = [np.arange(T * N * e, dtype=np.float64).reshape((T, N) + s) for e, s in zip((n, n * n, n, n * n), ((n,), (n, n)) * 2)]
    for o, v in zip(outs, vals):
        o.copy_(E.to_records(v, layout, 1).reshape(o.shape))      # (aos records keep the host array's trailing shape)
    got = C.host_histories(outs, n, layout)
    assert isinstance(got, tuple) and all(np.array_equal(g, v) for g, v in zip(got, vals))
    st = C.status(N, outs[0])
    assert st.dtype == torch.int32 and tuple(st.shape) == (N,) and not st.any() and st.device == outs[0].device


def make(cls, N, mode, layout):
    kw = dict(n_tracks=N, layout=layout, device_callables=mode == "torch", vectorized=mode == "vec")
    if cls is UnscentedKalmanFilter:
        return cls(D, 2, 1.0, None, None, MerweScaledSigmaPoints(D, 0.5, 2.0, 0.0), **kw)
    if cls is CubatureKalmanFilter:
        return cls(D, 2, 1.0, None, None, **kw)
    return cls(D, 2, **kw)


def to_rec_of(f, t):
    """the class's own _to_rec on a (N, K, D) result"""
    return f._to_rec(t, (K, D), "HJacobian") if isinstance(f, ExtendedKalmanFilter) else f._to_rec(t, K, D)


TYPE_ERROR = {UnscentedKalmanFilter: "device callables must return a float64 CUDA tensor shaped {}",
              CubatureKalmanFilter: "device callables must return a float64 CUDA tensor shaped {}",
              ExtendedKalmanFilter: "device callables: HJacobian must return a float64 CUDA tensor shaped {}"}
VALUE_ERROR = {CubatureKalmanFilter: "the callable returned shape {}, expected {}",
               ExtendedKalmanFilter: "HJacobian returned shape {}, expected {}"}


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("N", (3, 1))
@pytest.mark.parametrize("cls", (UnscentedKalmanFilter, CubatureKalmanFilter, ExtendedKalmanFilter))
def test_each_class_keeps_its_own_words(cls, N, layout):
    a = blocks(N)
    want = E.to_records(a.reshape(N, K * D), layout, 0)
    f = make(cls, N, "torch", layout)
    assert (f._N, f._layout, f._mode) == (N, layout, "torch")
    assert torch.equal(to_rec_of(f, torch.as_tensor(a)), want)
    assert torch.equal(f._rec_view(want, K, D), torch.as_tensor(a))
    for bad in (a, torch.as_tensor(a, dtype=torch.float32), torch.as_tensor(a).permute(0, 2, 1)):
        with pytest.raises(TypeError) as e:
            to_rec_of(f, bad)
        assert str(e.value) == TYPE_ERROR[cls].format((N, K, D))
    for mode in ("vec", "loop"):
        g = make(cls, N, mode, layout)
        assert g._mode == mode
        if cls is UnscentedKalmanFilter:               # tensors only, in every mode: the host modes' results come back as tensors
            assert torch.equal(to_rec_of(g, torch.as_tensor(a)), want)
            with pytest.raises(TypeError) as e:
                to_rec_of(g, a)
            assert str(e.value) == TYPE_ERROR[cls].format((N, K, D))
            continue
        assert torch.equal(to_rec_of(g, a), want)
        with pytest.raises(ValueError) as e:
            to_rec_of(g, a.transpose(0, 2, 1))
        assert str(e.value) == VALUE_ERROR[cls].format((N, D, K), (N, K, D))


def test_constructor_refusals_stay_each_class_s_own():
    bank = "device_callables=True needs a bank: pass n_tracks=N (use N = 1 for one filter)"
    for cls in (UnscentedKalmanFilter, CubatureKalmanFilter, ExtendedKalmanFilter):
        with pytest.raises(ValueError) as e:
            make(cls, None, "torch", "soa")
        assert str(e.value) == bank
        single = make(cls, None, "loop", "aos")
        assert (single._N, single._layout, single._mode) == (None, "aos", "loop")
        assert single._unb(np.zeros((1, 2, 3))).shape == (2, 3)
        assert make(cls, 1, "loop", "aos")._unb(np.zeros((1, 2))).shape == (1, 2)
    with pytest.raises(ValueError) as e:
        make(ExtendedKalmanFilter, None, "vec", "soa")
    assert str(e.value) == "vectorized=True needs a bank: pass n_tracks=N"
    assert make(CubatureKalmanFilter, None, "vec", "soa")._mode == "vec"          # EKF alone refuses that
    for cls in (CubatureKalmanFilter, ExtendedKalmanFilter):
        with pytest.raises(ValueError) as e:
            make(cls, 3, "loop", "rows")
        assert str(e.value) == "layout must be one of ['aos', 'soa']"
        for dims in ((0, 2), (2, 0)):
            with pytest.raises(ValueError) as e:
                cls(*dims, 1.0, None, None) if cls is CubatureKalmanFilter else cls(*dims)
            assert str(e.value) == "dim_x and dim_z must be 1 or greater"
    make(UnscentedKalmanFilter, 3, "loop", "rows")                                 # UKF checks neither the layout nor the dims


@pytest.mark.parametrize("cls", (CubatureKalmanFilter, ExtendedKalmanFilter))
def test_xb_and_Pb(cls):
    n = D                                                # dim_x = 3 against a bank of 2: every axis tells
    f = make(cls, 2, "loop", "soa")
    f.x, f.P = np.arange(6.).reshape(2, n), np.eye(n)
    assert np.array_equal(f._xb(), f.x) and f._Pb().shape == (2, n, n) and f._Pb().flags.c_contiguous
    f.x, f.P = np.zeros((n, 2)), np.zeros((2, n))
    for call, msg in ((f._xb, "x has shape (3, 2), expected (2, 3)"), (f._Pb, "P has shape (2, 3), expected (2, 3, 3) or (3, 3)")):
        with pytest.raises(ValueError) as e:
            call()
        assert str(e.value) == msg
    s = make(cls, None, "loop", "soa")
    for x in (np.arange(3.), np.arange(3.).reshape(n, 1)):
        s.x = x
        assert np.array_equal(s._xb(), np.arange(3.).reshape(1, n))
    assert s._Pb().shape == (1, n, n)
    s.x, s.P = np.zeros((1, n)), np.zeros((2, n, n))
    for call, msg in ((s._xb, "x has shape (1, 3), expected (3,) or (3, 1)"), (s._Pb, "P has shape (2, 3, 3), expected (1, 3, 3)")):
        with pytest.raises(ValueError) as e:
            call()
        assert str(e.value) == msg


# ---- the ensemble base ------------------------------------------------------------------------------------------------------
def ensemble(lead, layout):
    N, d = 3, 2
    if lead:
        return EnsembleKalmanFilterBank(np.zeros(d), np.eye(d), 1, 1.0, N, np.eye(1, d), np.eye(d), lead[0], layout=layout)
    return EnsembleKalmanFilter(np.zeros(d), np.eye(d), 1, 1.0, N, np.eye(1, d), np.eye(d), layout=layout)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("lead", ((), (2,)))
def test_ensemble_round_trip_and_refusals(lead, layout):
    N, d = 3, 2
    f = ensemble(lead, layout)
    assert f._lead == lead and f.sigmas.shape == lead + (N, d)
    a = np.arange(int(np.prod(lead + (N, d))), dtype=np.float64).reshape(lead + (N, d)) + 0.25
    f.sigmas = a
    assert f._sig_host is None
    assert tuple(f.sigmas_device.shape) == lead + ((d, N) if layout == "soa" else (N, d)) and f.sigmas_device.is_contiguous()
    assert tuple(f._members().shape) == lead + (N, d) and np.array_equal(f._members().numpy(), a)
    assert f._members().data_ptr() == f.sigmas_device.data_ptr()
    got = f.sigmas
    assert np.array_equal(got, a) and f.sigmas is got                              # downloaded once, then the cache
    for given in (a, torch.as_tensor(a)):
        assert torch.equal(f._records(given, d), f.sigmas_device)
    bad = np.zeros(lead + (d, N))
    with pytest.raises(ValueError) as e:
        f.sigmas = bad
    assert str(e.value) == f"sigmas has shape {bad.shape}, expected " + ("(2, 3, 2)" if lead else "(3, 2)")
    for given, what in ((bad, "array"), (torch.as_tensor(bad), "tensor")):
        with pytest.raises(ValueError) as e:
            f._records(given, d)
        assert str(e.value) == "expected an " + ("(2, 3, 2)" if lead else "(3, 2)") + f" {what}, got {bad.shape}"
    f.inv = np.linalg.pinv
    with pytest.raises(NotImplementedError) as e:
        f._check_inv()
    name = "EnsembleKalmanFilterBank" if lead else "EnsembleKalmanFilter"
    assert str(e.value) == name + ".inv other than numpy.linalg.inv: the inverse is taken on the device"
    assert repr(f).splitlines()[0] == name + " object (filterpy_amd, gfx950)"
    assert [line.split(" = ")[0] for line in repr(f).splitlines() if " = " in line and not line.startswith((" ", "["))][:2] == \
        (["n_tracks", "dim_x"] if lead else ["dim_x", "dim_z"])
