"""SimplexSigmaPoints and the simplex routes of UnscentedKalmanFilter without a GPU: the NumPy port (tests/simplex_port.py)
against the live-reference goldens (and the live reference where its checkout exists), the package's point matrix bit for bit,
the class's attributes and quirks, the Python layer of the filter over CPU stand-ins for the kernels
(tests/fake_simplex_engine.py) in all three calling conventions and both layouts, and what the C ABI answers with
FK_UKF_FLAG_SIMPLEX: the table of fk_ukf_linear_supported, the refusals in their order and words, and -- on machines without a
device -- the kernel family every served size reaches.  Parity bar: the project's 1e-10 (max |d| / max |ref| per array)."""
import os
import sys

import numpy as np
import pytest

import simplex_port as sp
import test_host_refusals as hr

REF = os.environ.get("FILTERPY_REFERENCE", "/root/reference")
TOL = 1e-10
SIMPLEX, PAIR = 4, 1
DIMS_FWD = "fused linear UKF with FK_UKF_FLAG_SIMPLEX: dim_x 1..6 with dim_z 1..3, dim_x 7..9 with dim_z 1..4"
DIMS_RTS = "fused linear UKF smoother with FK_UKF_FLAG_SIMPLEX: dim_x 1..9"
SFWD, SRTS = "ukf_simplex_kernel", "ukf_simplex_rts_kernel"


@pytest.fixture(scope="module")
def gold():
    return sp.Golden()


def close(a, b, what, tol=TOL):
    err = sp.rel(a, b)
    assert err < tol, (what, err)


# ------------------------------------------------------------------------------------------------------- the port --

def test_golden_file_is_small_and_complete(gold):
    here = os.path.dirname(os.path.abspath(__file__))
    assert os.path.getsize(sp.GOLDEN) <= os.path.getsize(os.path.join(here, "golden", "ukf_dims.npz"))
    assert gold.cases == sp.FUSED + [(12, 4)]
    assert gold.cases[gold.missing[0]] == (4, 2) and gold.case(4, 2)["zl"][gold.missing[1]] is None


@pytest.mark.parametrize("n,m", sp.FUSED + [(12, 4)])
def test_port_against_golden(gold, n, m):
    c = gold.case(n, m)
    W = c["Wm"]
    assert np.array_equal(W, sp.weights(n))
    close(sp.sigma_points(c["x0"], c["P0"]), c["sigmas"], "sigmas")
    xp, Pp, sf = sp.predict(c["x0"], c["P0"], c["F"], c["Q"], W, W)
    close(xp, c["s1_xp"], "x prior"), close(Pp, c["s1_Pp"], "P prior"), close(sf, c["s1_sigmas_f"], "sigmas_f")
    u = sp.update(xp, Pp, sf, c["zs"][0], c["H"], c["R"], W, W)
    for k in ("x", "P", "K", "S", "y", "Pxz", "sigmas_h"):
        close(u[k], c["s1_" + k], k)
    mu, cov = sp.batch_filter(c["x0"], c["P0"], c["zl"], c["F"], c["H"], c["Q"], c["R"])
    close(mu, c["mu"], "mu"), close(cov, c["cov"], "cov")
    for got, key in zip(sp.rts_smoother(c["mu"], c["cov"], c["F"], c["Q"]), ("rts_x", "rts_P", "rts_K")):
        close(got, c[key], key)


@pytest.fixture(scope="module")
def ref():
    if not os.path.isdir(os.path.join(REF, "filterpy")):
        pytest.skip("no reference checkout here")
    os.environ.setdefault("MPLBACKEND", "Agg")
    sys.path.insert(0, REF)
    old_flag, sys.dont_write_bytecode = sys.dont_write_bytecode, True
    try:
        import filterpy.kalman as K
    finally:
        sys.dont_write_bytecode = old_flag
        sys.path.remove(REF)
    return K


@pytest.mark.parametrize("n,m", [(1, 1), (3, 2), (6, 3), (9, 4), (13, 5)])
def test_port_against_live_reference(ref, n, m):
    rs = np.random.RandomState(300 + n)
    A, B = rs.randn(n, n), rs.randn(m, m)
    F, H = np.eye(n) + 0.05 * rs.randn(n, n), rs.randn(m, n)
    Q, R, P0, x0 = 0.01 * (A @ A.T / n + np.eye(n)), B @ B.T / m + np.eye(m), 3.0 * (A.T @ A / n + np.eye(n)), rs.randn(n)
    zs = [None if t == 3 else rs.randn(m) for t in range(8)]
    pts = ref.SimplexSigmaPoints(n)
    assert sp.point_matrix(n).tobytes() == pts.sigma_points(np.zeros(n), 1.0).T.copy().tobytes()
    f = ref.UnscentedKalmanFilter(n, m, dt=1.0, hx=lambda x: H @ x, fx=lambda x, dt: F @ x, points=pts)
    f.x, f.P, f.Q, f.R = x0.copy(), P0.copy(), Q, R
    mu, cov = f.batch_filter(zs)
    pm, pc = sp.batch_filter(x0, P0, zs, F, H, Q, R)
    close(pm, mu, "mu"), close(pc, cov, "cov")
    for got, want, key in zip(sp.rts_smoother(mu, cov, F, Q), f.rts_smoother(mu, cov), "xPK"):
        close(got, want, "rts " + key)


# ------------------------------------------------------------------------------------------------------ the class --

def test_point_matrix_is_the_goldens_bit_for_bit(gold):
    from filterpy_amd.kalman.sigma_points import simplex_point_matrix
    for n in range(1, 17):
        I = simplex_point_matrix(n)
        assert I.shape == (n, n + 1) and I.tobytes() == gold.I(n).tobytes(), n
        assert sp.point_matrix(n).tobytes() == gold.I(n).tobytes(), n


def test_class_attributes_and_quirks(gold, monkeypatch):
    import fake_ut_engine
    from filterpy_amd.kalman import SimplexSigmaPoints
    fake_ut_engine.install(monkeypatch)
    p = SimplexSigmaPoints(4)
    assert p.num_sigmas() == 5 and p.n == 4 and p.alpha == 1 and SimplexSigmaPoints(4, alpha=7).alpha == 7
    assert p.Wc is p.Wm and np.array_equal(p.Wm, np.full(5, 1. / 5))
    assert p.subtract is np.subtract and callable(p.sqrt)
    lines = repr(p).split("\n")
    assert lines[0] == "SimplexSigmaPoints object"
    assert [l.split(" = ")[0] for l in lines[1:] if " = " in l and not l.startswith(" ")] == ["n", "alpha", "Wm", "Wc", "subtract", "sqrt"]
    with pytest.raises(ValueError, match=r"expected size\(x\) 4, but size is 3"):
        p.sigma_points(np.zeros(3), np.eye(4))
    with pytest.raises(ValueError, match=r"expected size\(x\) 4, but size is 8"):
        p.sigma_points(np.zeros((2, 4, 1)), np.eye(4))
    c = gold.case(4, 2)
    s = p.sigma_points(c["x0"], c["P0"])
    assert s.shape == (5, 4)
    close(s, c["sigmas"], "sigmas")
    # scalar x / scalar P (sigma_points.py:490-497)
    s1 = SimplexSigmaPoints(1).sigma_points(5., 9.)
    assert s1.shape == (2, 1)
    close(s1, sp.sigma_points(np.array([5.]), 9.), "scalar")
    close(p.sigma_points(c["x0"], 2.5), sp.sigma_points(c["x0"], 2.5), "scalar P")
    # a bank, like the two other classes take one
    rs = np.random.RandomState(5)
    xb = rs.randn(7, 4)
    Pb = np.array([c["P0"] * (1 + 0.1 * i) for i in range(7)])
    sb = p.sigma_points(xb, Pb)
    assert sb.shape == (7, 5, 4)
    for i in range(7):
        close(sb[i], sp.sigma_points(xb[i], Pb[i]), ("bank", i))


def test_custom_hooks_are_called_like_the_reference_calls_them(gold, monkeypatch):
    """sqrt_method per filter on P itself (no scaling); subtract ONCE per filter with (x (n, 1), -U' I (n, n + 1))"""
    import fake_ut_engine
    from scipy.linalg import cholesky
    from filterpy_amd.kalman import SimplexSigmaPoints
    fake_ut_engine.install(monkeypatch)
    c = gold.case(5, 3)
    seen = []

    def sub(a, b):
        seen.append((np.shape(a), np.shape(b)))
        return np.subtract(a, b)

    def root(A):
        seen.append(("sqrt", np.array(A)))
        return cholesky(A)
    for kw in (dict(subtract=sub), dict(sqrt_method=root, subtract=sub), dict(sqrt_method=root)):
        del seen[:]
        p = SimplexSigmaPoints(5, **kw)
        assert (p.subtract is sub) == ("subtract" in kw) and (p.sqrt is root) == ("sqrt_method" in kw)
        close(p.sigma_points(c["x0"], c["P0"]), c["sigmas"], kw.keys())
        assert [s for s in seen if s[0] != "sqrt"] == ([((5, 1), (5, 6))] if "subtract" in kw else [])
        roots = [s[1] for s in seen if s[0] == "sqrt"]
        assert len(roots) == (1 if "sqrt_method" in kw else 0) and all(np.array_equal(r, c["P0"]) for r in roots)
    del seen[:]
    SimplexSigmaPoints(5, subtract=sub).sigma_points(np.tile(c["x0"], (3, 1)), c["P0"])
    assert seen == [((5, 1), (5, 6))] * 3


# ------------------------------------------------------------------------- the filter's Python layer, on stand-ins --

def _filters(gold, n, m, mode, layout, bank):
    """one UnscentedKalmanFilter on the golden's model; bank: n_tracks = 3, each track its own x0 and measurements"""
    import torch
    from filterpy_amd.kalman import SimplexSigmaPoints, UnscentedKalmanFilter
    c = gold.case(n, m)
    F, H = c["F"], c["H"]
    N = 3 if bank else None
    if mode == "matrix":
        kw = dict(fx=F, hx=H)
    elif mode == "loop":
        kw = dict(fx=lambda x, dt: F @ x, hx=lambda x: H @ x)
    elif mode == "vec":
        kw = dict(fx=lambda s, dt: s @ F.T, hx=lambda s: s @ H.T, vectorized=True)
    else:
        Ft, Ht = torch.as_tensor(F), torch.as_tensor(H)
        kw = dict(fx=lambda s, dt: s @ Ft.T, hx=lambda s: s @ Ht.T, device_callables=True)
    f = UnscentedKalmanFilter(n, m, dt=1.0, points=SimplexSigmaPoints(n), n_tracks=N, layout=layout, **kw)
    shift = np.arange(N or 1)[:, None] * 0.25
    x0 = c["x0"][None] + shift
    zs = [None if z is None else (z[None] + shift[:, :1]) for z in c["zl"]]
    f.Q, f.R = c["Q"], c["R"]
    if bank:
        f.x, f.P = x0.copy(), np.tile(c["P0"], (N, 1, 1))
    else:
        f.x, f.P, zs = x0[0].copy(), c["P0"].copy(), [None if z is None else z[0] for z in zs]
    want = [sp.batch_filter(x0[i], c["P0"], [None if z is None else np.reshape(z, (-1, m))[i] for z in zs], F, H, c["Q"], c["R"])
            for i in range(N or 1)]
    rts = [sp.rts_smoother(mu, cov, F, c["Q"]) for mu, cov in want]
    return f, zs, want, rts, c


def _check_run(f, zs, want, rts, bank, what):
    mu, cov = f.batch_filter(zs)
    xs, Ps, Ks = f.rts_smoother(mu, cov)
    for i in range(len(want)):
        pick = (lambda a: a[:, i]) if bank else (lambda a: a)
        close(pick(mu), want[i][0], (what, "mu", i)), close(pick(cov), want[i][1], (what, "cov", i))
        for got, ref_, key in zip((xs, Ps, Ks), rts[i], "xPK"):
            close(pick(got), ref_, (what, "rts", key, i))
    close(f.x, mu[-1], (what, "x"))


@pytest.mark.parametrize("layout", ["soa", "aos"])
@pytest.mark.parametrize("mode", ["matrix", "loop", "vec", "torch"])
@pytest.mark.parametrize("n,m", [(4, 2), (9, 3), (12, 4)])
def test_filter_layer_in_every_convention(gold, monkeypatch, n, m, mode, layout):
    """batch_filter / rts_smoother with a simplex point set: matrices take the fused calls where the library serves the size
    ((12, 4): the building blocks), callables the building blocks; one filter and a bank of three; (4, 2) has a missing step"""
    import fake_simplex_engine
    calls = fake_simplex_engine.install(monkeypatch)
    for bank in (False, True):
        if mode == "torch" and not bank:
            continue
        del calls[:]
        f, zs, want, rts, _ = _filters(gold, n, m, mode, layout, bank)
        _check_run(f, zs, want, rts, bank, (n, m, mode, layout, bank))
        fused = mode == "matrix" and n <= 9
        assert ("simplex_batch" in calls) == fused and ("simplex_rts" in calls) == fused, calls
        assert "fused_batch" not in calls and "fused_rts" not in calls
        if not fused:
            assert "sigma" in calls and "ut" in calls and "correct" in calls and "rts" in calls


@pytest.mark.parametrize("mode", ["loop", "vec", "torch"])
def test_filter_layer_step_by_step(gold, monkeypatch, mode):
    """predict() / update() one epoch at a time, with every attribute of the golden's first step"""
    import fake_simplex_engine
    fake_simplex_engine.install(monkeypatch)
    for bank in (False, True):
        if mode == "torch" and not bank:
            continue
        f, zs, want, _, c = _filters(gold, 6, 3, mode, "soa", bank)
        first = (lambda a: np.asarray(a)[0]) if bank else np.asarray
        assert np.shape(f.sigmas_f) == ((3, 7, 6) if bank else (7, 6)) and np.shape(f.sigmas_h) == ((3, 7, 3) if bank else (7, 3))
        f.predict()
        close(first(f.x), c["s1_xp"], "x prior"), close(first(f.P), c["s1_Pp"], "P prior")
        close(first(f.sigmas_f), c["s1_sigmas_f"], "sigmas_f")
        f.update(zs[0])
        for k in ("x", "P", "K", "S", "y", "sigmas_h"):
            close(first(getattr(f, k)), c["s1_" + k], k)
        for t in range(1, len(zs)):
            f.predict()
            f.update(zs[t])
        for i in range(len(want)):
            close(np.asarray(f.x)[i] if bank else f.x, want[i][0][-1], ("x end", i))
            close(np.asarray(f.P)[i] if bank else f.P, want[i][1][-1], ("P end", i))


@pytest.mark.parametrize("mode", ["loop", "vec", "torch"])
def test_filter_layer_with_point_hooks(gold, monkeypatch, mode):
    """sqrt_method / subtract on the point set: the device route of the generator (_dev_simplex_sigmas), never the fused calls"""
    import torch
    from scipy.linalg import cholesky
    import fake_simplex_engine
    from filterpy_amd.kalman import SimplexSigmaPoints, UnscentedKalmanFilter
    calls = fake_simplex_engine.install(monkeypatch)
    c = gold.case(5, 3)
    F, H = c["F"], c["H"]
    shapes = []

    def sub(a, b):
        shapes.append((tuple(a.shape), tuple(b.shape)))
        return a - b
    if mode == "loop":
        root = cholesky
    elif mode == "vec":
        root = lambda A: np.array([cholesky(a) for a in A])                                  # noqa: E731
    else:
        root = lambda A: torch.linalg.cholesky(A).transpose(1, 2)                             # noqa: E731
    for kw in (dict(subtract=sub), dict(sqrt_method=root), dict(sqrt_method=root, subtract=sub)):
        del shapes[:], calls[:]
        N = 2
        f = UnscentedKalmanFilter(5, 3, dt=1.0, fx=F, hx=H, points=SimplexSigmaPoints(5, **kw), n_tracks=N,
                                  vectorized=mode == "vec", device_callables=mode == "torch")
        f.x, f.P, f.Q, f.R = np.tile(c["x0"], (N, 1)), np.tile(c["P0"], (N, 1, 1)), c["Q"], c["R"]
        mu, cov = f.batch_filter([np.tile(z, (N, 1)) for z in c["zs"]])
        assert "simplex_batch" not in calls
        for i in range(N):
            close(mu[:, i], c["mu"], (mode, kw.keys(), "mu")), close(cov[:, i], c["cov"], (mode, kw.keys(), "cov"))
        if "subtract" in kw:
            assert set(shapes) == ({((5, 1), (5, 6))} if mode == "loop" else {((N, 5, 1), (N, 5, 6))}), set(shapes)


# --------------------------------------------------------------------------------------------------- the C ABI --

def _table(n, m, smoother):
    if smoother:
        return int(1 <= n <= 9)
    return int((1 <= n <= 6 and 1 <= m <= 3) or (7 <= n <= 9 and 1 <= m <= 4))


def test_abi_constants():
    from filterpy_amd import _abi
    assert _abi.FK_UKF_FLAG_SIMPLEX == SIMPLEX and _abi.FK_UKF_FLAG_PAIR_WEIGHTS == PAIR
    assert _abi.lib().fk_abi_version() == 4
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "filterhip.h")).read()
    assert "FK_UKF_FLAG_SIMPLEX = 4" in src


def test_supported_with_the_simplex_bit(uenv_):
    from filterpy_amd import _abi, _engine as E
    q = _abi.lib().fk_ukf_linear_supported
    for flags in (SIMPLEX, SIMPLEX | PAIR, SIMPLEX | 2):
        for n in range(-1, 19):
            for m in range(-1, 11):
                assert q(n, m, flags, 0) == _table(n, m, False), (n, m, flags)
                assert q(n, m, flags, 1) == _table(n, m, True), (n, m, flags)
    assert q(6, 3, SIMPLEX, 7) == 1 and q(6, 4, SIMPLEX, -1) == 1 and q(6, 4, SIMPLEX, 0) == 0
    for n, m in ((6, 3), (6, 4), (9, 4), (10, 2), (12, 4)):
        assert E.ukf_linear_supported(n, m, simplex=True) == bool(_table(n, m, False))
        assert E.ukf_linear_rts_supported(n, simplex=True) == bool(_table(n, m, True))
    assert E.ukf_linear_supported(12, 4, True) and not E.ukf_linear_supported(12, 4, True, simplex=True)


@pytest.fixture
def uenv_(monkeypatch):
    for v in hr.U_SWITCHES:
        monkeypatch.delenv(v, raising=False)
    return monkeypatch


def test_refusals_with_the_simplex_bit_in_order(uenv_):
    """size -> bad argument -> the 4 GiB guard -> nothing to do, the words of the other route except for the size"""
    fwd, rts = hr.U_FUSED
    UNSUPPORTED, BAD_ARG = hr.UNSUPPORTED, hr.BAD_ARG
    for flags in (SIMPLEX, SIMPLEX | PAIR, SIMPLEX | 2):
        for over in (dict(n=0), dict(n=-1), dict(n=17), dict(m=0), dict(m=5), dict(n=6, m=4), dict(n=9, m=5), dict(n=10, m=1),
                     dict(n=12, m=4), dict(n=16, m=8)):
            assert hr._u(fwd, dict(over, N=-1, flags=flags), all_null=True) == (UNSUPPORTED, DIMS_FWD), over
        for over in (dict(n=0), dict(n=-1), dict(n=10), dict(n=16), dict(n=17)):
            assert hr._u(rts, dict(over, N=-1, flags=flags), all_null=True) == (UNSUPPORTED, DIMS_RTS), over
        assert hr._u(rts, dict(n=9, m=0, flags=flags), null=(0,)) == (BAD_ARG, hr._bad(rts))      # the smoother does not read dim_z
        for name in hr.U_FUSED:
            assert hr._u(name, dict(N=-1, flags=flags)) == (BAD_ARG, hr._bad(name))
            assert hr._u(name, dict(T=-1, flags=flags)) == (BAD_ARG, hr._bad(name))
            for i in hr.U_ENTRY[name][2]:
                assert hr._u(name, dict(flags=flags), null=(i,)) == (BAD_ARG, hr._bad(name)), (name, i)
            for layout in (0, 1, 2, -1):
                assert hr._u(name, dict(layout=layout, N=0, flags=flags))[0] == 0
                assert hr._u(name, dict(layout=layout, T=0, flags=flags))[0] == 0
            assert hr._u(name, dict(N=0, flags=flags), all_null=True) == (BAD_ARG, hr._bad(name))
            optional = [i for i in range(hr.U_ENTRY[name][1]) if i not in hr.U_ENTRY[name][2]]
            assert hr._u(name, dict(N=0, flags=flags), null=optional)[0] == 0
            assert hr._u(name, dict(T=0, flags=flags), null=optional)[0] == 0
    # the guards, where the other route's one-lane calls have them: 32 bytes short of 4 GiB / at 4 GiB, behind the pointers
    f = SIMPLEX
    assert hr._u(fwd, dict(n=1, N=2 ** 29 - 4, flags=f)) == (UNSUPPORTED, hr._guard(fwd))
    assert hr._u(fwd, dict(n=1, N=2 ** 29 - 4, T=0, flags=f)) == (UNSUPPORTED, hr._guard(fwd))
    assert hr._u(fwd, dict(n=1, N=2 ** 29 - 5, T=0, flags=f))[0] == 0
    assert hr._u(fwd, dict(n=1, N=2 ** 29, flags=f), null=(0,)) == (BAD_ARG, hr._bad(fwd))
    assert hr._u(rts, dict(n=1, N=2 ** 29, flags=f)) == (UNSUPPORTED, hr._guard(rts))
    assert hr._u(rts, dict(n=1, N=2 ** 29 - 1, T=0, flags=f))[0] == 0
    assert hr._u(rts, dict(n=9, N=6628036, T=0, flags=f)) == (UNSUPPORTED, hr._guard(rts))
    assert hr._u(rts, dict(n=9, N=6628035, T=0, flags=f))[0] == 0
    assert hr._u(rts, dict(n=1, N=2 ** 29, flags=f), null=(7,)) == (BAD_ARG, hr._bad(rts))
    # without the bit the words are today's
    assert hr._u(fwd, dict(n=6, m=4, N=-1), all_null=True) == (UNSUPPORTED, hr.UKF_DIMS_FWD)
    assert hr._u(rts, dict(n=17, N=-1, flags=2), all_null=True) == (UNSUPPORTED, hr.UKF_DIMS_RTS)


def test_every_served_size_reaches_the_simplex_kernels():
    """Without a device the launch fails and its error names the kernel family (tests/test_host_refusals.py); flags 0, 1 and 2
    reach exactly the families they reach today"""
    if not hr._no_device():
        return
    fwd, rts = hr.U_FUSED
    sizes = [(n, m) for n in range(1, 10) for m in range(1, 5) if _table(n, m, False)]
    calls = [(fwd, dict(n=n, m=m, N=300, layout=layout, flags=flags)) for n, m in sizes for layout in (0, 1)
             for flags in (SIMPLEX, SIMPLEX | PAIR, SIMPLEX | 2)]
    nf = len(calls)
    calls += [(rts, dict(n=n, N=300, layout=layout, flags=flags), () if gains else (8, 9)) for n in range(1, 10) for layout in (0, 1)
              for flags in (SIMPLEX, SIMPLEX | PAIR) for gains in (True, False)]
    ns = len(calls)
    old = [((n, m), layout, flags) for n, m in ((2, 1), (6, 3), (9, 4)) for layout in (0, 1) for flags in (0, PAIR, 2)]
    calls += [(fwd, dict(n=n, m=m, N=300, layout=layout, flags=flags)) for (n, m), layout, flags in old]
    calls += [(rts, dict(n=n, N=300, layout=layout, flags=flags)) for (n, m), layout, flags in old]
    got = hr._walk(calls, {})
    assert got[:nf] == [(hr.LAUNCH, SFWD)] * nf, [c for c, g in zip(calls, got[:nf]) if g != (hr.LAUNCH, SFWD)]
    assert got[nf:ns] == [(hr.LAUNCH, SRTS)] * (ns - nf)
    want = [(hr.LAUNCH, hr.FWD)] * len(old)
    want += [(hr.LAUNCH, hr.RQUAD if (n >= 7 and flags & PAIR) else hr.RTS) for (n, m), layout, flags in old]
    assert got[ns:] == want, [(c, g, w) for c, g, w in zip(calls[ns:], got[ns:], want) if g != w]
