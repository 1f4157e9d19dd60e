"""-m gpu: the fused simplex UKF kernels (csrc/ukf_simplex.hip) through fk_ukf_linear_batch_f64 / fk_ukf_linear_rts_f64 with
FK_UKF_FLAG_SIMPLEX, and UnscentedKalmanFilter(points=SimplexSigmaPoints(n)) end to end, against the NumPy port of the
reference (tests/simplex_port.py) and the live-reference goldens (tests/golden/ukf_simplex.npz).  Every track of a bank carries
its own x0 and its own measurements, so that a lane mix-up shows.  Bar: the project's 1e-10 (max |d| / max |ref| per array,
per track).  The port's results are computed once per bank and shared between the layouts and the tests."""
import numpy as np
import pytest

import simplex_port as sp

pytestmark = pytest.mark.gpu
TOL = 1e-10
T = 12
N_BANK = 130                      # two full waves and a partial one
ST_NOT_PD = 1
_gold, _banks = [], {}


def gold():
    if not _gold:
        _gold.append(sp.Golden())
    return _gold[0]


def bank(n, m, N, masked=False):
    """the golden's model of (n, m) on N tracks: per-track x0 and zs (track 0: the golden's own), the port's filter output and
    smoother output per track; masked: a different missing step per track.  Cached, never modified."""
    key = (n, m, N, masked)
    if key not in _banks:
        c = gold().case(n, m)
        rs = np.random.RandomState(1000 * n + 10 * m + N)
        x0 = c["x0"][None] + 0.3 * rs.randn(N, n)
        x0[0] = c["x0"]
        P0 = np.tile(c["P0"], (N, 1, 1)) * (1.0 + 0.5 * rs.rand(N))[:, None, None]
        P0[0] = c["P0"]
        zs = np.swapaxes(c["zs"][None] + rs.randn(N, T, m), 0, 1).copy()          # (T, N, m)
        zs[:, 0] = c["zs"]
        mask = np.ones((T, N), dtype=np.uint8)
        if masked:
            mask[(np.arange(N) * 5 + 1) % T, np.arange(N)] = 0
        mu, cov = np.zeros((T, N, n)), np.zeros((T, N, n, n))
        xs, Ps, Ks = np.zeros((T, N, n)), np.zeros((T, N, n, n)), np.zeros((T, N, n, n))
        for i in range(N):
            zl = [zs[t, i] if mask[t, i] else None for t in range(T)]
            mu[:, i], cov[:, i] = sp.batch_filter(x0[i], P0[i], zl, c["F"], c["H"], c["Q"], c["R"])
            xs[:, i], Ps[:, i], Ks[:, i] = sp.rts_smoother(mu[:, i], cov[:, i], c["F"], c["Q"])
        for a in (x0, P0, zs, mask, mu, cov, xs, Ps, Ks):
            a.setflags(write=False)
        _banks[key] = dict(c=c, x0=x0, P0=P0, zs=zs, mask=mask, mu=mu, cov=cov, xs=xs, Ps=Ps, Ks=Ks)
    return _banks[key]


def per_track(got, want, what):
    """(T, N, ...) arrays: every track at the bar"""
    assert got.shape == want.shape, (what, got.shape, want.shape)
    for i in range(want.shape[1]):
        err = sp.rel(got[:, i], want[:, i])
        assert err < TOL, (what, i, err)


def run_fwd(b, layout, mask=None, means=True, covs=True, Wm=None, Wc=None, P0=None):
    import torch
    from filterpy_amd import _engine as E
    c = b["c"]
    n, m, N = c["F"].shape[0], c["H"].shape[0], b["x0"].shape[0]
    W = c["Wm"]
    dx, dP = E.to_records(np.array(b["x0"]), layout, 0), E.to_records(np.array(b["P0"] if P0 is None else P0), layout, 0)
    om = E.alloc_records((T,), N, n, layout) if means else None
    oc = E.alloc_records((T,), N, n * n, layout) if covs else None
    for o in (om, oc):
        if o is not None:
            o.fill_(float("nan"))
    st = torch.full((N,), 77, dtype=torch.int32, device=dx.device)
    dm = None if mask is None else torch.as_tensor(np.array(mask), device=dx.device)
    E.ukf_linear_batch(n, m, N, T, layout, float("nan"), E.dev(c["F"]), E.dev(c["H"]), E.dev(c["Q"]), E.dev(c["R"]),
                       E.dev(W if Wm is None else Wm), E.dev(W if Wc is None else Wc), E.to_records(np.array(b["zs"]), layout, 1),
                       dx, dP, mask=dm, means=om, covs=oc, status=st, paired=E.SIMPLEX)
    torch.cuda.synchronize()
    return (st.cpu().numpy(), None if om is None else E.from_records(om, layout, 1, (n,)),
            None if oc is None else E.from_records(oc, layout, 1, (n, n)),
            E.from_records(dx, layout, 0, (n,)), E.from_records(dP, layout, 0, (n, n)))


def run_rts(b, layout, gains=True, Wm=None, Wc=None, Xs=None, Ps=None):
    import torch
    from filterpy_amd import _engine as E
    c = b["c"]
    n, N = c["F"].shape[0], b["x0"].shape[0]
    W = c["Wm"]
    dX = E.to_records(np.array(b["mu"] if Xs is None else Xs), layout, 1)
    dP = E.to_records(np.array(b["cov"] if Ps is None else Ps), layout, 1)
    ox, oP = E.alloc_records((T,), N, n, layout), E.alloc_records((T,), N, n * n, layout)
    oK = E.alloc_records((T,), N, n * n, layout) if gains else None
    for o in (ox, oP, oK):
        if o is not None:
            o.fill_(float("nan"))
    st = torch.full((N,), 77, dtype=torch.int32, device=dX.device)
    E.ukf_linear_rts(n, N, T, layout, float("nan"), E.dev(c["F"]), E.dev(c["Q"]), E.dev(W if Wm is None else Wm),
                     E.dev(W if Wc is None else Wc), dX, dP, ox, oP, oK, st, paired=E.SIMPLEX)
    torch.cuda.synchronize()
    return (st.cpu().numpy(), E.from_records(ox, layout, 1, (n,)), E.from_records(oP, layout, 1, (n, n)),
            None if oK is None else E.from_records(oK, layout, 1, (n, n)))


def check_fwd(b, layout, mask=None):
    st, mu, cov, x, P = run_fwd(b, layout, mask)
    assert not st.any(), st
    per_track(mu, b["mu"], "mu"), per_track(cov, b["cov"], "cov")
    assert np.array_equal(x, mu[-1]) and np.array_equal(P, cov[-1])


def check_rts(b, layout):
    st, xs, Ps, Ks = run_rts(b, layout)
    assert not st.any(), st
    per_track(xs, b["xs"], "rts_x"), per_track(Ps, b["Ps"], "rts_P"), per_track(Ks, b["Ks"], "rts_K")
    assert np.array_equal(xs[-1], b["mu"][-1]) and np.array_equal(Ps[-1], b["cov"][-1]) and not Ks[-1].any()


@pytest.mark.parametrize("layout", ["soa", "aos"])
@pytest.mark.parametrize("n,m", sp.FUSED)
def test_fused_calls_every_size(n, m, layout):
    """both calls at every fused size of the golden (exact and padded instantiations), 130 tracks; track 0 is the golden's"""
    b = bank(n, m, N_BANK)
    c = b["c"]
    if gold().cases.index((n, m)) != gold().missing[0]:
        assert sp.rel(b["mu"][:, 0], c["mu"]) < TOL and sp.rel(b["xs"][:, 0], c["rts_x"]) < TOL       # the port, once more
    check_fwd(b, layout)
    check_rts(b, layout)


@pytest.mark.parametrize("layout", ["soa", "aos"])
@pytest.mark.parametrize("N", [1, 63, 65, 257])
@pytest.mark.parametrize("n,m", [(4, 2), (9, 3)])
def test_bank_tails(n, m, N, layout):
    b = bank(n, m, N)
    check_fwd(b, layout)
    check_rts(b, layout)


@pytest.mark.parametrize("layout", ["soa", "aos"])
@pytest.mark.parametrize("n,m", [(3, 1), (6, 3), (9, 4)])
def test_a_different_missing_step_per_track(n, m, layout):
    b = bank(n, m, N_BANK, masked=True)
    assert (b["mask"] == 0).sum() == N_BANK and len(set(np.argmin(b["mask"], axis=0))) == T
    check_fwd(b, layout, b["mask"])


@pytest.mark.parametrize("layout", ["soa", "aos"])
@pytest.mark.parametrize("n,m", [(6, 3), (7, 4)])
def test_optional_outputs_one_at_a_time(n, m, layout):
    b = bank(n, m, N_BANK)
    for means, covs in ((False, True), (True, False), (False, False)):
        st, mu, cov, x, P = run_fwd(b, layout, means=means, covs=covs)
        assert not st.any()
        if means:
            per_track(mu, b["mu"], "mu")
        if covs:
            per_track(cov, b["cov"], "cov")
        per_track(x[None], b["mu"][-1:], "x"), per_track(P[None], b["cov"][-1:], "P")
    st, xs, Ps, Ks = run_rts(b, layout, gains=False)
    assert not st.any() and Ks is None
    per_track(xs, b["xs"], "rts_x"), per_track(Ps, b["Ps"], "rts_P")


@pytest.mark.parametrize("layout", ["soa", "aos"])
@pytest.mark.parametrize("n,m", [(4, 2), (8, 4)])
def test_one_track_that_is_not_positive_definite(n, m, layout):
    """a status bit, not a fault: the bad track's status carries FK_STATUS_NOT_PD, its neighbours stay exact"""
    b = bank(n, m, N_BANK)
    bad = 70
    P0 = np.array(b["P0"])
    P0[bad, 1, 1] = -1.0
    st, mu, cov, _, _ = run_fwd(b, layout, P0=P0)
    good = np.arange(N_BANK) != bad
    assert st[bad] & ST_NOT_PD and not st[good].any()
    per_track(mu[:, good], b["mu"][:, good], "mu"), per_track(cov[:, good], b["cov"][:, good], "cov")
    Ps = np.array(b["cov"])
    Ps[4, bad, 0, 0] = -1.0
    st, xs, Pss, Ks = run_rts(b, layout, Ps=Ps)
    assert st[bad] & ST_NOT_PD and not st[good].any()
    per_track(xs[:, good], b["xs"][:, good], "rts_x"), per_track(Pss[:, good], b["Ps"][:, good], "rts_P")
    per_track(Ks[:, good], b["Ks"][:, good], "rts_K")


@pytest.mark.parametrize("layout", ["soa", "aos"])
def test_unequal_weights_are_used_as_given(layout):
    """Wm != Wc, neither constant, Wm not summing to 1 (no Wc above 1 / (n + 1): P - K S K' stays positive definite)"""
    n, m, N = 6, 3, 5
    b = bank(n, m, N)
    c = b["c"]
    rs = np.random.RandomState(11)
    Wm = rs.uniform(0.5, 1.5, n + 1)
    Wm *= 1.02 / Wm.sum()
    Wc = rs.uniform(0.7, 1.0, n + 1) / (n + 1)
    st, mu, cov, _, _ = run_fwd(b, layout, Wm=Wm, Wc=Wc)
    assert not st.any()
    for i in range(N):
        wmu, wcov = sp.batch_filter(b["x0"][i], b["P0"][i], list(b["zs"][:, i]), c["F"], c["H"], c["Q"], c["R"], Wm, Wc)
        assert sp.rel(mu[:, i], wmu) < TOL and sp.rel(cov[:, i], wcov) < TOL and sp.rel(wmu, b["mu"][:, i]) > 1e-3
    st, xs, Ps, Ks = run_rts(b, layout, Wm=Wm, Wc=Wc)
    assert not st.any()
    for i in range(N):
        for got, want in zip((xs, Ps, Ks), sp.rts_smoother(b["mu"][:, i], b["cov"][:, i], c["F"], c["Q"], Wm, Wc)):
            assert sp.rel(got[:, i], want) < TOL


def test_sigma_points_of_a_bank():
    from filterpy_amd.kalman import SimplexSigmaPoints
    for n, m in ((1, 1), (6, 3), (12, 4)):
        b = bank(n, m, N_BANK) if n <= 9 else None
        c = gold().case(n, m)
        if b is None:
            rs = np.random.RandomState(n)
            x0, P0 = c["x0"][None] + rs.randn(N_BANK, n), np.tile(c["P0"], (N_BANK, 1, 1)) * (1 + rs.rand(N_BANK))[:, None, None]
        else:
            x0, P0 = b["x0"], b["P0"]
        p = SimplexSigmaPoints(n)
        got = p.sigma_points(np.array(x0), np.array(P0))
        assert got.shape == (N_BANK, n + 1, n)
        for i in range(N_BANK):
            assert sp.rel(got[i], sp.sigma_points(x0[i], P0[i])) < TOL, i
        assert sp.rel(p.sigma_points(c["x0"], c["P0"]), c["sigmas"]) < TOL


def _filter(c, mode, N, layout):
    import torch
    from filterpy_amd.kalman import SimplexSigmaPoints, UnscentedKalmanFilter
    F, H = c["F"], c["H"]
    n, m = F.shape[0], H.shape[0]
    if mode == "matrix":
        kw = dict(fx=F, hx=H)
    elif mode == "loop":
        kw = dict(fx=lambda x, dt: F @ x, hx=lambda x: H @ x)
    else:
        Ft, Ht = torch.as_tensor(F, device="cuda"), torch.as_tensor(H, device="cuda")
        kw = dict(fx=lambda s, dt: s @ Ft.T, hx=lambda s: s @ Ht.T, device_callables=True)
    f = UnscentedKalmanFilter(n, m, dt=1.0, points=SimplexSigmaPoints(n), n_tracks=N, layout=layout, **kw)
    f.Q, f.R = c["Q"], c["R"]
    return f


@pytest.mark.parametrize("layout", ["soa", "aos"])
@pytest.mark.parametrize("n,m", [(4, 2), (6, 3), (9, 4), (12, 4)])
def test_class_end_to_end(n, m, layout, monkeypatch):
    """matrices run the fused route (dim_x <= 9), Python callables and device callables the building blocks; the three agree
    with each other and with the golden, for one filter and for a bank of 130, rts_smoother included; (4, 2) has a missing step"""
    from filterpy_amd import _engine as E
    c = gold().case(n, m)
    fused_calls = []
    real_batch, real_rts = E.ukf_linear_batch, E.ukf_linear_rts
    monkeypatch.setattr(E, "ukf_linear_batch", lambda *a, **k: (fused_calls.append(("batch", k.get("paired") == E.SIMPLEX)), real_batch(*a, **k))[1])
    monkeypatch.setattr(E, "ukf_linear_rts", lambda *a, **k: (fused_calls.append(("rts", k.get("paired") == E.SIMPLEX)), real_rts(*a, **k))[1])
    rs = np.random.RandomState(7 * n + m)
    shift = 0.3 * rs.randn(N_BANK, n)
    shift[0] = 0
    zshift = rs.randn(T, N_BANK, m)
    zshift[:, 0] = 0
    for N in (None, N_BANK):
        runs = {}
        for mode in ("matrix", "loop", "torch"):
            if mode == "torch" and N is None:
                continue
            del fused_calls[:]
            f = _filter(c, mode, N, layout)
            if N is None:
                f.x, f.P, zs = c["x0"].copy(), c["P0"].copy(), c["zl"]
            else:
                f.x, f.P = c["x0"][None] + shift, np.tile(c["P0"], (N, 1, 1))
                zs = [None if z is None else z[None] + zshift[t] for t, z in enumerate(c["zl"])]
            mu, cov = f.batch_filter(zs)
            xs, Ps, Ks = f.rts_smoother(mu, cov)
            want = [("batch", True), ("rts", True)] if (mode == "matrix" and n <= 9) else []
            assert fused_calls == want, (mode, N, fused_calls)
            runs[mode] = (mu, cov, xs, Ps, Ks)
            first = (lambda a: a[:, 0]) if N else (lambda a: a)
            for got, key in zip(runs[mode], ("mu", "cov", "rts_x", "rts_P", "rts_K")):
                assert sp.rel(first(got), c[key]) < TOL, (mode, N, key, sp.rel(first(got), c[key]))
        for mode in runs:
            for got, ref_, key in zip(runs[mode], runs["matrix"], ("mu", "cov", "rts_x", "rts_P", "rts_K")):
                if N is None:
                    assert sp.rel(got, ref_) < TOL, (mode, key)
                else:
                    per_track(got, ref_, (mode, key))
