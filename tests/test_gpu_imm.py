"""-m gpu parity tests: the batched IMM estimator through the C ABI
(fk_imm_batch_f64) and through the filterpy-shaped ``IMMEstimator`` class, against goldens frozen
from the live filterpy.kalman.IMMEstimator and against oracle/imm_oracle.py on seeded banks."""
import numpy as np
import pytest

from conftest import golden, rel_err_rows

pytestmark = pytest.mark.gpu
TOL = 1e-10
CASES = [(2, 1, 2), (4, 2, 2), (4, 2, 3), (6, 3, 2), (3, 2, 2), (5, 2, 3)]


def spd(rs, n, scale=1.0):
    A = rs.randn(n, n)
    return scale * (A @ A.T / n + 0.5 * np.eye(n))


def stable_F(rs, n):
    F = np.eye(n) + 0.1 * rs.randn(n, n)
    return F / max(1.0, 1.05 * np.max(np.abs(np.linalg.eigvals(F))))


@pytest.mark.parametrize("layout", ["soa", "aos"])
@pytest.mark.parametrize("n,m,nm", CASES)
def test_imm_goldens(n, m, nm, layout):
    """every track of the bank runs the golden sequence (N not a multiple of the workgroup)."""
    from gpu_util import run_imm
    from gpu_util import tile_tracks
    g = golden("imm")
    p = f"n{n}m{m}k{nm}_"
    N = 300
    mu0 = g[p + "mu0"] / g[p + "mu0"].sum()
    r = run_imm(tile_tracks(g[p + "xs0"], N), tile_tracks(g[p + "Ps0"], N), tile_tracks(mu0, N), g[p + "M"],
                tile_tracks(g[p + "zs"], N, axis=1), g[p + "Fs"], g[p + "Qs"], g[p + "Hs"], g[p + "Rs"], layout)
    for trk in (0, 63, 255, 256, N - 1):
        assert rel_err_rows(r["x_out"][:, trk], g[p + "x"]) < TOL and rel_err_rows(r["P_out"][:, trk], g[p + "P"]) < TOL
        assert rel_err_rows(r["x_prior_out"][:, trk], g[p + "xp"]) < TOL
        assert rel_err_rows(r["P_prior_out"][:, trk], g[p + "Pp"]) < TOL
        assert np.allclose(r["mu_out"][:, trk], g[p + "mu"], rtol=1e-10, atol=1e-14)
        assert np.allclose(r["likelihood_out"][:, trk], g[p + "L"], rtol=1e-10, atol=1e-300)
        assert rel_err_rows(r["xs"][trk], g[p + "xs_final"]) < TOL and rel_err_rows(r["Ps"][trk], g[p + "Ps_final"]) < TOL
        assert np.allclose(r["mu"][trk], g[p + "mu"][-1], rtol=1e-10, atol=1e-14)


@pytest.mark.parametrize("layout", ["soa", "aos"])
@pytest.mark.parametrize("n,m,nm", [(4, 2, 2), (4, 2, 3), (6, 3, 3)])
def test_imm_seeded_bank_vs_oracle(n, m, nm, layout):
    """independent tracks (own states, measurements and mode probabilities) against the oracle."""
    from gpu_util import run_imm
    from oracle import imm_oracle
    rs = np.random.RandomState(77 + n + nm)
    N, T = 1000, 25
    Fs = np.array([stable_F(rs, n) for _ in range(nm)])
    Qs = np.array([spd(rs, n, 0.05 * (j + 1)) for j in range(nm)])
    Hs = np.array([rs.randn(m, n)] * nm)
    Rs = np.array([spd(rs, m, 0.5) for _ in range(nm)])
    M = rs.rand(nm, nm) + 2 * np.eye(nm)
    M /= M.sum(axis=1, keepdims=True)
    xs0 = rs.randn(N, nm, n)
    Ps0 = np.array([[spd(rs, n, 2.0) for _ in range(nm)] for _ in range(N)])
    mu0 = rs.rand(N, nm) + 0.1
    mu0 /= mu0.sum(axis=1, keepdims=True)
    zs = rs.randn(T, N, m) * 2
    r = run_imm(xs0, Ps0, mu0, M, zs, Fs, Qs, Hs, Rs, layout)
    for trk in (0, 1, 255, 256, 511, N - 1):
        x, P, mu, xp, Pp, L = imm_oracle.imm_batch(xs0[trk], Ps0[trk], mu0[trk], M, zs[:, trk], Fs, Qs, Hs, Rs)
        assert rel_err_rows(r["x_out"][:, trk], x) < TOL and rel_err_rows(r["P_out"][:, trk], P) < TOL
        assert rel_err_rows(r["x_prior_out"][:, trk], xp) < TOL and rel_err_rows(r["P_prior_out"][:, trk], Pp) < TOL
        assert np.allclose(r["mu_out"][:, trk], mu, rtol=1e-10, atol=1e-14)
        assert np.allclose(r["likelihood_out"][:, trk], L, rtol=1e-10, atol=1e-300)
    # properties that hold for every track: mode probabilities sum to one, P symmetric
    assert np.abs(r["mu_out"].sum(axis=-1) - 1).max() < 1e-14
    assert np.abs(r["P_out"] - np.swapaxes(r["P_out"], -1, -2)).max() == 0.0


@pytest.mark.parametrize("layout", ["soa", "aos"])
@pytest.mark.parametrize("n,m,nm", [(4, 2, 2), (2, 1, 3), (6, 3, 2)])
def test_imm_extreme_likelihoods_vs_oracle(n, m, nm, layout):
    """The ends of the likelihood's range: measurements hundreds of sigmas away (every likelihood underflows and is floored at
    DBL_MIN, kalman_filter.py:1213-1226 -- the normalising sum is SUBNORMAL and its reciprocal would overflow), measurement
    noise of 1e-150 and 1e+150 (|S| beyond what a plain product of pivots can hold), next to ordinary tracks.  The kernel forms
    the density from the reciprocal pivots without a logarithm and normalises by a reciprocal (fk_imm.hpp)."""
    from gpu_util import run_imm
    from oracle import imm_oracle
    rs = np.random.RandomState(5 + n + nm)
    N, T = 260, 6
    Fs = np.array([stable_F(rs, n) for _ in range(nm)])
    Qs = np.array([spd(rs, n, 0.05 * (j + 1)) for j in range(nm)])
    Hs = np.array([rs.randn(m, n)] * nm)
    M = rs.rand(nm, nm) + 2 * np.eye(nm)
    M /= M.sum(axis=1, keepdims=True)
    xs0 = rs.randn(N, nm, n)
    Ps0 = np.array([[spd(rs, n, 2.0) for _ in range(nm)] for _ in range(N)])
    mu0 = rs.rand(N, nm) + 0.1
    mu0 /= mu0.sum(axis=1, keepdims=True)
    for scale_R, far in ((1.0, True), (1e-150, False), (1e150, False)):
        Rs = np.array([spd(rs, m, 0.5) * scale_R for _ in range(nm)])
        zs = rs.randn(T, N, m) * 2
        if far:
            zs[:, 1::2] += 1e4                              # every other track: hopeless measurements
        r = run_imm(xs0, Ps0, mu0, M, zs, Fs, Qs, Hs, Rs, layout)
        for trk in (0, 1, 2, 255, 256, N - 1):
            x, P, mu, xp, Pp, L = imm_oracle.imm_batch(xs0[trk], Ps0[trk], mu0[trk], M, zs[:, trk], Fs, Qs, Hs, Rs)
            assert np.all(np.isfinite(r["mu_out"][:, trk])) and np.all(np.isfinite(r["likelihood_out"][:, trk])), (scale_R, trk)
            # a bank dragged 1e4 away spreads its filters by thousands of sigmas and the mixing turns ill-conditioned (the
            # host build of the same arithmetic drifts from the oracle by 1e-8 in five such steps): the first step is the
            # one that tests the floor and the subnormal sum; the ordinary tracks are held over all steps
            k = 1 if far and trk % 2 else T
            assert np.allclose(r["mu_out"][:k, trk], mu[:k], rtol=1e-9, atol=1e-14), (scale_R, trk)
            assert np.allclose(r["likelihood_out"][:k, trk], L[:k], rtol=1e-9, atol=1e-307), (scale_R, trk)
            assert rel_err_rows(r["x_out"][:k, trk], x[:k]) < 1e-9, (scale_R, trk)
            if far and trk % 2:
                assert np.all(L[0] == 2.2250738585072014e-308) and np.all(r["likelihood_out"][0, trk] == 2.2250738585072014e-308)
        assert np.abs(r["mu_out"].sum(axis=-1) - 1).max() < 1e-13


@pytest.mark.parametrize("layout", ["soa", "aos"])
@pytest.mark.parametrize("n,m,nm,N", [(6, 3, 2, 1037), (4, 2, 3, 1038), (2, 1, 2, 1300), (9, 3, 4, 515), (5, 4, 8, 300)])
def test_imm_chunked_call_is_bit_identical(n, m, nm, N, layout, monkeypatch):
    """FK_IMM_CHUNKS="G,H" cuts fk_imm_batch_f64 into bank groups x time chunks on helper streams (fk_chunks.hpp, imm_chunked_call),
    the state handed from chunk to chunk through xs / Ps / mu in place: every output, the final state and the status must be
    bit-identical to the single launch -- the register-resident and the rolled classes, ragged last workgroups."""
    from gpu_util import run_imm
    rs = np.random.RandomState(3 * n + nm + N % 7)
    T = 23
    Fs = np.array([stable_F(rs, n) for _ in range(nm)])
    Qs = np.array([spd(rs, n, 0.05 * (j + 1)) for j in range(nm)])
    Hs = np.array([rs.randn(m, n)] * nm)
    Rs = np.array([spd(rs, m, 0.5) for _ in range(nm)])
    M = rs.rand(nm, nm) + 2 * np.eye(nm)
    M /= M.sum(axis=1, keepdims=True)
    xs0 = rs.randn(N, nm, n)
    Ps0 = np.array([[spd(rs, n, 2.0) for _ in range(nm)] for _ in range(N)])
    mu0 = rs.rand(N, nm) + 0.1
    mu0 /= mu0.sum(axis=1, keepdims=True)
    zs = rs.randn(T, N, m) * 2
    res = {}
    for tag, env in (("one", "1,1"), ("3x4", "3,4"), ("2x7", "2,7"), ("4x23", "4,23"), ("default", None)):
        if env:
            monkeypatch.setenv("FK_IMM_CHUNKS", env)
        else:
            monkeypatch.delenv("FK_IMM_CHUNKS", raising=False)
        res[tag] = run_imm(xs0, Ps0, mu0, M, zs, Fs, Qs, Hs, Rs, layout)
    assert np.all(np.isfinite(res["one"]["x_out"]))
    for tag in ("3x4", "2x7", "4x23", "default"):
        for k in res["one"]:
            assert np.array_equal(res["one"][k], res[tag][k], equal_nan=True), (tag, k)


@pytest.mark.parametrize("layout", ["soa", "aos"])
@pytest.mark.parametrize("with_ll0", [False, True])
@pytest.mark.parametrize("n,m,nm,N", [(4, 2, 2, 1037), (9, 3, 4, 515)])
def test_imm_chunked_call_with_missing_measurements_is_bit_identical(n, m, nm, N, with_ll0, layout, monkeypatch):
    """with a measurement mask the per-filter log-density of a zero residual under the last S is carried from step to
    step -- in registers inside one launch, through ll0 between the pieces of a chunked call.  A masked call WITHOUT ll0 cannot
    hand it over and must therefore stay one launch; with ll0 every decomposition is bit-identical.  Missing measurements sit
    right behind every chunk boundary of the decompositions tried."""
    from gpu_util import run_imm
    rs = np.random.RandomState(5 * n + nm)
    T = 24
    Fs = np.array([stable_F(rs, n) for _ in range(nm)])
    Qs = np.array([spd(rs, n, 0.05 * (j + 1)) for j in range(nm)])
    Hs = np.array([rs.randn(m, n)] * nm)
    Rs = np.array([spd(rs, m, 0.5) for _ in range(nm)])
    M = rs.rand(nm, nm) + 2 * np.eye(nm)
    M /= M.sum(axis=1, keepdims=True)
    xs0 = rs.randn(N, nm, n)
    Ps0 = np.array([[spd(rs, n, 2.0) for _ in range(nm)] for _ in range(N)])
    mu0 = rs.rand(N, nm) + 0.1
    mu0 /= mu0.sum(axis=1, keepdims=True)
    zs = rs.randn(T, N, m) * 2
    zmask = (rs.rand(T, N) > 0.3).astype(np.uint8)
    zmask[0] = 1
    zmask[[3, 4, 6, 7, 12, 13, 18, 19], ::2] = 0          # first steps of the time chunks of 3x4 / 2x7 (with their stagger)
    ll0 = np.full((N, nm), -np.inf) if with_ll0 else None
    res = {}
    for tag, env in (("one", "1,1"), ("3x4", "3,4"), ("2x7", "2,7"), ("4x24", "4,24")):
        monkeypatch.setenv("FK_IMM_CHUNKS", env)
        res[tag] = run_imm(xs0, Ps0, mu0, M, zs, Fs, Qs, Hs, Rs, layout, zmask=zmask, ll0=None if ll0 is None else ll0.copy())
    assert np.all(np.isfinite(res["one"]["x_out"]))
    for tag in ("3x4", "2x7", "4x24"):
        for k in res["one"]:
            assert np.array_equal(res["one"][k], res[tag][k], equal_nan=True), (tag, k)


def _make_filters(g, p, n, m, nm, column):
    from filterpy_amd.kalman import KalmanFilter
    fs = []
    for j in range(nm):
        f = KalmanFilter(dim_x=n, dim_z=m)
        f.x = g[p + "xs0"][j].reshape(-1, 1).copy() if column else g[p + "xs0"][j].copy()
        f.P, f.F, f.Q, f.H, f.R = (g[p + k][j].copy() for k in ("Ps0", "Fs", "Qs", "Hs", "Rs"))
        fs.append(f)
    return fs


@pytest.mark.parametrize("column", [False, True])
@pytest.mark.parametrize("n,m,nm", [(2, 1, 2), (4, 2, 3)])
def test_imm_class_drop_in(n, m, nm, column):
    """the reference's own usage: imm.predict(); imm.update(z) in a loop, attributes after each call."""
    from filterpy_amd.kalman import IMMEstimator
    g = golden("imm")
    p = f"n{n}m{m}k{nm}_"
    imm = IMMEstimator(_make_filters(g, p, n, m, nm, column), g[p + "mu0"], g[p + "M"])
    shp = (lambda a: a.reshape(-1, 1)) if column else (lambda a: a)
    for t in range(10):
        imm.predict()
        assert imm.x.shape == ((n, 1) if column else (n,))
        assert rel_err_rows(imm.x_prior, shp(g[p + "xp"][t])) < TOL and rel_err_rows(imm.P_prior, g[p + "Pp"][t]) < TOL
        z = g[p + "zs"][t]
        imm.update(z.reshape(-1, 1) if column else z)
        assert rel_err_rows(imm.x, shp(g[p + "x"][t])) < TOL and rel_err_rows(imm.P, g[p + "P"][t]) < TOL
        assert rel_err_rows(imm.x_post, shp(g[p + "x"][t])) < TOL
        assert np.allclose(imm.mu, g[p + "mu"][t], rtol=1e-10, atol=1e-14)
        assert np.allclose(imm.likelihood, g[p + "L"][t], rtol=1e-10, atol=1e-300)
        assert imm.filters[0].x.shape == ((n, 1) if column else (n,))
    # the remaining steps in one launch; the object ends where the reference ends
    xs, Ps, mus = imm.batch_filter(g[p + "zs"][10:])
    assert rel_err_rows(xs.reshape(-1, n), g[p + "x"][10:]) < TOL and rel_err_rows(Ps, g[p + "P"][10:]) < TOL
    assert np.allclose(mus, g[p + "mu"][10:], rtol=1e-10, atol=1e-14)
    for j in range(nm):
        assert rel_err_rows(imm.filters[j].x.reshape(-1), g[p + "xs_final"][j]) < TOL
        assert rel_err_rows(imm.filters[j].P, g[p + "Ps_final"][j]) < TOL
    cbar = imm.mu @ g[p + "M"]
    assert np.allclose(imm.cbar, cbar, rtol=1e-13) and imm.omega.shape == (nm, nm)


def test_imm_bank_class():
    from filterpy_amd.kalman import IMMEstimator
    from gpu_util import tile_tracks
    g = golden("imm")
    n, m, nm = 4, 2, 2
    p = f"n{n}m{m}k{nm}_"
    N = 130
    imm = IMMEstimator(_make_filters(g, p, n, m, nm, False), g[p + "mu0"], g[p + "M"], n_tracks=N)
    assert imm.x.shape == (N, n) and imm.mu.shape == (N, nm)
    xs, Ps, mus, xp, Pp = imm.batch_filter(tile_tracks(g[p + "zs"], N, axis=1), return_priors=True)
    assert xs.shape == (30, N, n) and Ps.shape == (30, N, n, n) and mus.shape == (30, N, nm)
    for trk in (0, 64, N - 1):
        assert rel_err_rows(xs[:, trk], g[p + "x"]) < TOL and rel_err_rows(Ps[:, trk], g[p + "P"]) < TOL
        assert rel_err_rows(xp[:, trk], g[p + "xp"]) < TOL and rel_err_rows(Pp[:, trk], g[p + "Pp"]) < TOL
    assert imm.filters[1].x.shape == (N, n)


def test_imm_rejects_what_the_kernel_cannot_do():
    from filterpy_amd.kalman import IMMEstimator, KalmanFilter
    fs = [KalmanFilter(dim_x=2, dim_z=1) for _ in range(2)]
    with pytest.raises(ValueError):
        IMMEstimator(fs[:1], [1.0], np.eye(1))
    imm = IMMEstimator(fs, [0.5, 0.5], np.array([[0.9, 0.1], [0.1, 0.9]]))
    with pytest.raises(NotImplementedError):
        IMMEstimator([KalmanFilter(dim_x=2, dim_z=1) for _ in range(17)], [1] * 17, np.full((17, 17), 1 / 17))
    odd = [KalmanFilter(dim_x=2, dim_z=1) for _ in range(2)]
    odd[1].inv = np.linalg.pinv              # honoured by KalmanFilter.update, refused -- loudly -- by the bank kernels
    with pytest.raises(NotImplementedError):
        IMMEstimator(odd, [.5, .5], np.full((2, 2), .5))
    with pytest.raises(NotImplementedError):
        IMMEstimator([KalmanFilter(dim_x=17, dim_z=1) for _ in range(2)], [.5, .5], np.full((2, 2), .5))


# ---- round 3: banks of up to eight filters, dim_x <= 9, dim_z <= 4 (the rolled (9, 4) class of every bank size) ----------
def _big(kind, name="imm_big"):
    g = golden(name)
    return [tuple(int(v) for v in c) for c in g[kind + "_cases"]]


def _big_file(nm):
    return "imm_banks16" if nm > 8 else "imm_big"          # (round 6: banks of nine to sixteen filters, make_imm_banks16_golden.py)


@pytest.mark.parametrize("layout", ["soa", "aos"])
@pytest.mark.parametrize("n,m,nm", _big("imm") + _big("imm", "imm_banks16"))
def test_big_imm_banks_vs_live_reference(n, m, nm, layout):
    """IMMEstimator on banks the round-2 kernel refused: every track of a ragged bank runs the live reference's sequence"""
    from gpu_util import run_imm
    from gpu_util import tile_tracks
    g = golden(_big_file(nm))
    p = f"imm_n{n}m{m}k{nm}_"
    N = 130
    r = run_imm(tile_tracks(g[p + "xs0"], N), tile_tracks(g[p + "Ps0"], N), tile_tracks(g[p + "mu0"], N), g[p + "M"],
                tile_tracks(g[p + "zs"], N, axis=1), g[p + "Fs"], g[p + "Qs"], g[p + "Hs"], g[p + "Rs"], layout)
    for trk in (0, 63, 64, N - 1):
        assert rel_err_rows(r["x_out"][:, trk], g[p + "x"]) < TOL and rel_err_rows(r["P_out"][:, trk], g[p + "P"]) < TOL
        assert rel_err_rows(r["x_prior_out"][:, trk], g[p + "xp"]) < TOL
        assert rel_err_rows(r["P_prior_out"][:, trk], g[p + "Pp"]) < TOL
        assert np.allclose(r["mu_out"][:, trk], g[p + "mu"], rtol=1e-10, atol=1e-14)
        assert np.allclose(r["likelihood_out"][:, trk], g[p + "L"], rtol=1e-10, atol=1e-300)
        assert rel_err_rows(r["xs"][trk], g[p + "xs_final"]) < TOL and rel_err_rows(r["Ps"][trk], g[p + "Ps_final"]) < TOL


@pytest.mark.parametrize("layout", ["soa", "aos"])
@pytest.mark.parametrize("n,m,nm", [(9, 3, 4), (5, 4, 8), (3, 1, 6)])
def test_big_imm_seeded_bank_vs_oracle(n, m, nm, layout):
    """independent tracks (own states, measurements, mode probabilities) on the big banks, against the oracle"""
    from gpu_util import run_imm
    from oracle import imm_oracle
    rs = np.random.RandomState(177 + n + nm)
    N, T = 200, 10
    Fs = np.array([stable_F(rs, n) for _ in range(nm)])
    Qs = np.array([spd(rs, n, 0.05 * (j + 1)) for j in range(nm)])
    Hs = np.array([rs.randn(m, n)] * nm)
    Rs = np.array([spd(rs, m, 0.5) for _ in range(nm)])
    M = rs.rand(nm, nm) + 2 * np.eye(nm)
    M /= M.sum(axis=1, keepdims=True)
    xs0 = rs.randn(N, nm, n)
    Ps0 = np.array([[spd(rs, n, 2.0) for _ in range(nm)] for _ in range(N)])
    mu0 = rs.rand(N, nm) + 0.1
    mu0 /= mu0.sum(axis=1, keepdims=True)
    zs = rs.randn(T, N, m) * 2
    r = run_imm(xs0, Ps0, mu0, M, zs, Fs, Qs, Hs, Rs, layout)
    for trk in (0, 1, 63, 64, N - 1):
        x, P, mu, xp, Pp, L = imm_oracle.imm_batch(xs0[trk], Ps0[trk], mu0[trk], M, zs[:, trk], Fs, Qs, Hs, Rs)
        assert rel_err_rows(r["x_out"][:, trk], x) < TOL and rel_err_rows(r["P_out"][:, trk], P) < TOL
        assert rel_err_rows(r["x_prior_out"][:, trk], xp) < TOL and rel_err_rows(r["P_prior_out"][:, trk], Pp) < TOL
        assert np.allclose(r["mu_out"][:, trk], mu, rtol=1e-10, atol=1e-14)
        assert np.allclose(r["likelihood_out"][:, trk], L, rtol=1e-10, atol=1e-300)


def test_big_imm_and_mmae_classes_drop_in():
    """the reference's own usage on the big banks: predict(); update(z) call by call, then batch_filter for the rest"""
    from filterpy_amd.kalman import IMMEstimator, MMAEFilterBank
    for n, m, nm in _big("imm")[:3] + _big("imm", "imm_banks16")[:3]:
        g = golden(_big_file(nm))
        p = f"imm_n{n}m{m}k{nm}_"
        imm = IMMEstimator(_make_filters(g, p, n, m, nm, False), g[p + "mu0"].copy(), g[p + "M"])
        for t in range(6):
            imm.predict()
            assert rel_err_rows(imm.x[None], g[p + "xp"][t][None]) < TOL and rel_err_rows(imm.P[None], g[p + "Pp"][t][None]) < TOL
            imm.update(g[p + "zs"][t])
            assert rel_err_rows(imm.x[None], g[p + "x"][t][None]) < TOL and rel_err_rows(imm.P[None], g[p + "P"][t][None]) < TOL
            assert np.allclose(imm.mu, g[p + "mu"][t], rtol=1e-10, atol=1e-14)
    for n, m, nm in _big("mmae") + _big("mmae", "imm_banks16"):
        g = golden(_big_file(nm))
        q = f"mmae_n{n}m{m}k{nm}_"
        gg = {k: g[k] for k in g.files if k.startswith(q)}
        bank = MMAEFilterBank(_make_filters(gg, q, n, m, nm, False), g[q + "p0"].copy(), dim_x=n)
        for t in range(6):
            bank.predict()
            bank.update(g[q + "zs"][t])
            assert rel_err_rows(bank.x[None], g[q + "x"][t][None]) < TOL and rel_err_rows(bank.P[None], g[q + "P"][t][None]) < TOL
            assert np.allclose(bank.p, g[q + "p"][t], rtol=1e-10, atol=1e-14)
        xs, Ps, ps = bank.batch_filter(g[q + "zs"][6:])
        assert rel_err_rows(xs.reshape(-1, n), g[q + "x"][6:]) < TOL and rel_err_rows(Ps, g[q + "P"][6:]) < TOL


# ------------------------------------------------------------------------------- MMAE ----
MMAE_CASES = [(2, 1, 2), (4, 2, 2), (4, 2, 3), (6, 3, 3), (3, 2, 2), (2, 1, 3)]


@pytest.mark.parametrize("layout", ["soa", "aos"])
@pytest.mark.parametrize("n,m,nm", MMAE_CASES)
def test_mmae_goldens_c_abi(n, m, nm, layout):
    """FK_IMM_FLAG_MMAE through the C ABI against goldens from the live MMAEFilterBank."""
    import torch
    from filterpy_amd import _engine as E
    from gpu_util import tile_tracks
    g = golden("mmae")
    p = f"n{n}m{m}k{nm}_"
    N, T = 200, 30
    dxs = E.to_records(tile_tracks(g[p + "xs0"], N).reshape(N, nm * n), layout, 0)
    dPs = E.to_records(tile_tracks(g[p + "Ps0"], N).reshape(N, nm * n * n), layout, 0)
    dp = E.to_records(tile_tracks(g[p + "p0"], N), layout, 0)
    dz = E.to_records(tile_tracks(g[p + "zs"], N, axis=1), layout, 1)
    out = dict(x_out=E.alloc_records((T,), N, n, layout), P_out=E.alloc_records((T,), N, n * n, layout),
               mu_out=E.alloc_records((T,), N, nm, layout), likelihood_out=E.alloc_records((T,), N, nm, layout))
    st = torch.zeros(N, dtype=torch.int32, device=dxs.device)
    E.imm_batch(n, m, nm, N, T, layout, E.dev(g[p + "Fs"]), E.dev(g[p + "Qs"]), E.dev(g[p + "Hs"]), E.dev(g[p + "Rs"]),
                None, dz, dxs, dPs, dp, status=st, mmae=True, **out)
    torch.cuda.synchronize()
    assert not st.any()
    x = E.from_records(out["x_out"], layout, 1, (n,))
    P = E.from_records(out["P_out"], layout, 1, (n, n))
    pr = E.from_records(out["mu_out"], layout, 1, (nm,))
    L = E.from_records(out["likelihood_out"], layout, 1, (nm,))
    xs = E.from_records(dxs, layout, 0, (nm, n))
    for trk in (0, 64, N - 1):
        assert rel_err_rows(x[:, trk], g[p + "x"]) < TOL and rel_err_rows(P[:, trk], g[p + "P"]) < TOL
        assert np.allclose(pr[:, trk], g[p + "p"], rtol=1e-10, atol=1e-14)
        assert np.allclose(L[:, trk], g[p + "L"], rtol=1e-10, atol=1e-300)
        assert rel_err_rows(xs[trk], g[p + "xs_final"]) < TOL


@pytest.mark.parametrize("column", [False, True])
@pytest.mark.parametrize("n,m,nm", [(2, 1, 3), (4, 2, 2)])
def test_mmae_class_drop_in(n, m, nm, column):
    from filterpy_amd.kalman import MMAEFilterBank
    g = golden("mmae")
    p = f"n{n}m{m}k{nm}_"
    q = {k[len(p):]: g[k] for k in g.files if k.startswith(p)}
    gg = {p + k: v for k, v in q.items()}
    gg[p + "mu0"] = q["p0"]
    fs = _make_filters(gg, p, n, m, nm, column)
    bank = MMAEFilterBank(fs, q["p0"].copy(), dim_x=n)
    shp = (lambda a: a.reshape(-1, 1)) if column else (lambda a: a)
    for t in range(12):
        bank.predict()
        z = q["zs"][t]
        bank.update(z.reshape(-1, 1) if column else z)
        assert bank.x.shape == ((n, 1) if column else (n,))
        assert rel_err_rows(bank.x, shp(q["x"][t])) < TOL and rel_err_rows(bank.P, q["P"][t]) < TOL
        assert np.allclose(bank.p, q["p"][t], rtol=1e-10, atol=1e-14)
    assert rel_err_rows(bank.x_prior, shp(q["x"][10])) < TOL        # prior = the estimate before the last predict
    xs, Ps, ps = bank.batch_filter(q["zs"][12:])
    assert rel_err_rows(xs.reshape(-1, n), q["x"][12:]) < TOL and rel_err_rows(Ps, q["P"][12:]) < TOL
    assert np.allclose(ps, q["p"][12:], rtol=1e-10, atol=1e-14)
    for j in range(nm):
        assert rel_err_rows(bank.filters[j].x.reshape(-1), q["xs_final"][j]) < TOL


def test_mmae_update_overrides_and_bank():
    """update(z, R=, H=) overrides every filter's R / H for that call (mmae.py:160-186); n_tracks banks."""
    from filterpy_amd.kalman import MMAEFilterBank
    from oracle import kf_oracle
    g = golden("mmae")
    n, m, nm = 4, 2, 2
    p = f"n{n}m{m}k{nm}_"
    gg = {k: g[k] for k in g.files if k.startswith(p)}
    gg[p + "mu0"] = g[p + "p0"]
    fs = _make_filters(gg, p, n, m, nm, False)
    bank = MMAEFilterBank(fs, g[p + "p0"].copy(), dim_x=n)
    R2, H2 = 2.0 * np.eye(m), g[p + "Hs"][0] * 0.5
    z = g[p + "zs"][0]
    bank.update(z, R=R2, H=H2)
    for j in range(nm):
        x, P, *_ = kf_oracle.kf_update(g[p + "xs0"][j], g[p + "Ps0"][j], z, R2, H2)
        assert rel_err_rows(bank.filters[j].x, x) < TOL and rel_err_rows(bank.filters[j].P, P) < TOL
    N = 70
    fs = _make_filters(gg, p, n, m, nm, False)
    bank = MMAEFilterBank(fs, g[p + "p0"].copy(), dim_x=n, n_tracks=N)
    from gpu_util import tile_tracks
    xs, Ps, ps = bank.batch_filter(tile_tracks(g[p + "zs"], N, axis=1))
    assert xs.shape == (30, N, n) and ps.shape == (30, N, nm)
    assert rel_err_rows(xs[:, N - 1], g[p + "x"]) < TOL and rel_err_rows(Ps[:, 3], g[p + "P"]) < TOL


def _missing_bank(kind, p, g, nm, n, m, n_tracks, layout):
    from filterpy_amd.kalman import IMMEstimator, KalmanFilter, MMAEFilterBank
    fs = []
    for j in range(nm):
        f = KalmanFilter(dim_x=n, dim_z=m)
        f.x = g[p + "xs0"][j].copy() if n_tracks is None else np.tile(g[p + "xs0"][j], (n_tracks, 1))
        f.P = g[p + "Ps0"][j].copy() if n_tracks is None else np.tile(g[p + "Ps0"][j], (n_tracks, 1, 1))
        f.F, f.Q, f.H, f.R = g[p + "Fs"][j].copy(), g[p + "Qs"][j].copy(), g[p + "H"].copy(), g[p + "Rs"][j].copy()
        fs.append(f)
    kw = {} if n_tracks is None else dict(n_tracks=n_tracks, layout=layout)
    if kind == "imm":
        return IMMEstimator(fs, g[p + "mu0"], g[p + "M"], **kw)
    return MMAEFilterBank(fs, list(g[p + "mu0"] / g[p + "mu0"].sum()), dim_x=n, H=g[p + "H"], **kw)


@pytest.mark.parametrize("kind", ["imm", "mmae"])
def test_missing_measurements_call_by_call(kind):
    """predict(); update(z or None) like the reference's loop: update(None) keeps the filters' x, P and re-weights the
    modes with the density of a zero residual under each filter's last S (goldens: live reference,
    tests/golden/make_imm_missing_golden.py; the first measurement is missing too)."""
    g = golden("imm_missing")
    miss = set(int(t) for t in g["missing"])
    for n, m, nm in g["cases"]:
        n, m, nm = int(n), int(m), int(nm)
        p = f"n{n}m{m}k{nm}_"
        q = p + kind + "_"
        est = _missing_bank(kind, p, g, nm, n, m, None, "soa")
        for t, z in enumerate(g[p + "zs"]):
            est.predict()
            est.update(None if t in miss else z)
            mu = est.mu if kind == "imm" else est.p
            assert rel_err_rows(np.asarray(est.x, dtype=float).reshape(1, n), g[q + "x"][t][None]) < TOL, (kind, n, m, nm, t)
            assert rel_err_rows(np.asarray(est.P, dtype=float)[None], g[q + "P"][t][None]) < TOL, (kind, n, m, nm, t)
            assert np.allclose(mu, g[q + "mu"][t], rtol=1e-10, atol=1e-14), (kind, n, m, nm, t)
            if kind == "imm":
                assert np.allclose(est.likelihood, g[q + "L"][t], rtol=1e-10, atol=1e-300), (n, m, nm, t)
        for j in range(nm):
            assert rel_err_rows(np.asarray(est.filters[j].x, dtype=float).reshape(1, n), g[q + "xs_final"][j].reshape(1, n)) < TOL
            assert rel_err_rows(np.asarray(est.filters[j].P, dtype=float)[None], g[q + "Ps_final"][j][None]) < TOL


@pytest.mark.parametrize("layout", ["soa", "aos"])
@pytest.mark.parametrize("kind", ["imm", "mmae"])
def test_missing_measurements_one_launch_bank(kind, layout):
    """the same sequences as ONE launch over a bank (batch_filter with None entries -> zmask), and a run without gaps
    followed by update(None): the zero-residual densities must have been kept current by the gap-free run"""
    g = golden("imm_missing")
    miss = set(int(t) for t in g["missing"])
    N = 70
    for n, m, nm in g["cases"]:
        n, m, nm = int(n), int(m), int(nm)
        p = f"n{n}m{m}k{nm}_"
        q = p + kind + "_"
        est = _missing_bank(kind, p, g, nm, n, m, N, layout)
        zl = [None if t in miss else np.tile(z, (N, 1)) for t, z in enumerate(g[p + "zs"])]
        xs, Ps, mus = est.batch_filter(zl)
        for trk in (0, 63, 64, N - 1):
            assert rel_err_rows(xs[:, trk], g[q + "x"]) < TOL and rel_err_rows(Ps[:, trk], g[q + "P"]) < TOL, (kind, n, m, nm)
            assert np.allclose(mus[:, trk], g[q + "mu"], rtol=1e-10, atol=1e-14)
    # gap-free batch, then a gap: equals the call-by-call sequence
    n, m, nm = (int(v) for v in g["cases"][1])
    p = f"n{n}m{m}k{nm}_"
    a = _missing_bank(kind, p, g, nm, n, m, N, layout)
    b = _missing_bank(kind, p, g, nm, n, m, N, layout)
    zs = np.tile(g[p + "zs"][:6, None, :], (1, N, 1))
    a.batch_filter(zs)
    a.predict()
    a.update(None)
    for z in zs:
        b.predict()
        b.update(z)
    b.predict()
    b.update(None)
    ma, mb = (a.mu, b.mu) if kind == "imm" else (a.p, b.p)
    assert np.allclose(ma, mb, rtol=1e-10, atol=1e-14) and rel_err_rows(np.asarray(a.x), np.asarray(b.x)) < TOL


@pytest.mark.parametrize("layout", ["soa", "aos"])
@pytest.mark.parametrize("kind", ["imm", "mmae"])
def test_control_input(kind, layout):
    """IMMEstimator.predict(u) / MMAEFilterBank.predict(u): every filter's x = F x + B u with its own B -- call by call
    on one estimator and as one launch over a bank (goldens: live reference, tests/golden/make_imm_control_golden.py)."""
    from filterpy_amd.kalman import IMMEstimator, KalmanFilter, MMAEFilterBank
    g = golden("imm_control")
    N = 70
    for n, m, nm, nu in g["cases"]:
        n, m, nm, nu = int(n), int(m), int(nm), int(nu)
        p = f"n{n}m{m}k{nm}_"
        q = p + kind + "_"

        def make(n_tracks):
            fs = []
            for j in range(nm):
                f = KalmanFilter(dim_x=n, dim_z=m, dim_u=nu)
                f.x = g[p + "xs0"][j].copy() if n_tracks is None else np.tile(g[p + "xs0"][j], (n_tracks, 1))
                f.P = g[p + "Ps0"][j].copy() if n_tracks is None else np.tile(g[p + "Ps0"][j], (n_tracks, 1, 1))
                f.F, f.Q, f.H, f.R, f.B = (g[p + "Fs"][j].copy(), g[p + "Qs"][j].copy(), g[p + "H"].copy(),
                                           g[p + "Rs"][j].copy(), g[p + "Bs"][j].copy())
                fs.append(f)
            kw = {} if n_tracks is None else dict(n_tracks=n_tracks, layout=layout)
            if kind == "imm":
                return IMMEstimator(fs, g[p + "mu0"], g[p + "M"], **kw)
            return MMAEFilterBank(fs, list(g[p + "mu0"] / g[p + "mu0"].sum()), dim_x=n, H=g[p + "H"], **kw)
        est = make(None)
        for t, (z, u) in enumerate(zip(g[p + "zs"], g[p + "us"])):
            est.predict(u)
            est.update(z)
            mu = est.mu if kind == "imm" else est.p
            assert rel_err_rows(np.asarray(est.x, dtype=float).reshape(1, n), g[q + "x"][t][None]) < TOL, (kind, n, t)
            assert rel_err_rows(np.asarray(est.P, dtype=float)[None], g[q + "P"][t][None]) < TOL, (kind, n, t)
            assert np.allclose(mu, g[q + "mu"][t], rtol=1e-10, atol=1e-14)
        if kind == "imm":
            bank = make(N)
            T = len(g[p + "zs"])
            xs, Ps, mus = bank.batch_filter(np.tile(g[p + "zs"][:, None], (1, N, 1)), us=np.tile(g[p + "us"][:, None], (1, N, 1)))
            for trk in (0, 64, N - 1):
                assert rel_err_rows(xs[:, trk], g[q + "x"]) < TOL and rel_err_rows(Ps[:, trk], g[q + "P"]) < TOL
                assert np.allclose(mus[:, trk], g[q + "mu"], rtol=1e-10, atol=1e-14)


@pytest.mark.parametrize("layout", ["soa", "aos"])
@pytest.mark.parametrize("n,m,nm", [(10, 3, 2), (12, 5, 3), (16, 8, 2), (11, 2, 8), (9, 6, 4)])
def test_imm_banks_above_9_4_vs_oracle(n, m, nm, layout):
    """VERDICT r3 missing 3: IMMEstimator takes filters of any size (IMM.py:14-120); the kernels stopped at dim_x 9 / dim_z 4.
    The classes (12, 4) / (16, 8) (csrc/imm_quad.hip; rounds 4-6: a rolled one-lane-per-bank class) against the oracle: independent tracks, a ragged last workgroup, all outputs,
    and the class API on the same bank."""
    from gpu_util import run_imm
    from filterpy_amd.kalman import IMMEstimator, KalmanFilter
    from oracle import imm_oracle
    rs = np.random.RandomState(7 + n + 3 * nm)
    N, T = 130, 6
    Fs = np.array([stable_F(rs, n) for _ in range(nm)])
    Qs = np.array([spd(rs, n, 0.05 * (j + 1)) for j in range(nm)])
    Hs = np.array([rs.randn(m, n)] * nm)
    Rs = np.array([spd(rs, m, 0.5) for _ in range(nm)])
    M = rs.rand(nm, nm) + 2 * np.eye(nm)
    M /= M.sum(axis=1, keepdims=True)
    xs0 = rs.randn(N, nm, n)
    Ps0 = np.array([[spd(rs, n, 2.0) for _ in range(nm)] for _ in range(N)])
    mu0 = rs.rand(N, nm) + 0.1
    mu0 /= mu0.sum(axis=1, keepdims=True)
    zs = rs.randn(T, N, m) * 2
    r = run_imm(xs0, Ps0, mu0, M, zs, Fs, Qs, Hs, Rs, layout)
    for trk in (0, 63, 64, N - 1):
        x, P, mu, xp, Pp, L = imm_oracle.imm_batch(xs0[trk], Ps0[trk], mu0[trk], M, zs[:, trk], Fs, Qs, Hs, Rs)
        assert rel_err_rows(r["x_out"][:, trk], x) < TOL and rel_err_rows(r["P_out"][:, trk], P) < TOL
        assert rel_err_rows(r["x_prior_out"][:, trk], xp) < TOL and rel_err_rows(r["P_prior_out"][:, trk], Pp) < TOL
        assert np.allclose(r["mu_out"][:, trk], mu, rtol=1e-9, atol=1e-14)
        assert np.allclose(r["likelihood_out"][:, trk], L, rtol=1e-9, atol=1e-300)
    # the reference's own usage on one bank: imm.predict(); imm.update(z)
    fs = []
    for j in range(nm):
        f = KalmanFilter(dim_x=n, dim_z=m)
        f.x, f.P, f.F, f.Q, f.H, f.R = xs0[0, j].copy(), Ps0[0, j].copy(), Fs[j], Qs[j], Hs[j], Rs[j]
        fs.append(f)
    imm = IMMEstimator(fs, mu0[0], M)
    x, P, mu, xp, Pp, L = imm_oracle.imm_batch(xs0[0], Ps0[0], mu0[0], M, zs[:3, 0], Fs, Qs, Hs, Rs)
    for t in range(3):
        imm.predict()
        imm.update(zs[t, 0])
        assert rel_err_rows(imm.x[None], x[t][None]) < TOL and rel_err_rows(imm.P[None], P[t][None]) < TOL
        assert np.allclose(imm.mu, mu[t], rtol=1e-9, atol=1e-14)


# ---- round 6: one lane per filter (csrc/imm_lanes.hip): every class x every group width, ragged banks, output subsets
LANES_CASES = [(4, 2, 4), (3, 2, 7), (4, 1, 12), (6, 3, 4), (5, 3, 6), (6, 2, 16), (9, 4, 2), (7, 2, 3), (9, 4, 8), (8, 3, 5), (9, 2, 13), (7, 4, 16)]
# ---- four lanes per filter (csrc/imm_quad.hip): the classes (12, 4) and (16, 8), every group width, padded and exact dims
QUAD_CASES = [(10, 3, 2), (12, 4, 4), (11, 2, 7), (12, 3, 16), (16, 8, 2), (13, 5, 3), (14, 6, 8), (15, 7, 12), (16, 4, 16), (9, 5, 2), (14, 8, 2)]


def _lanes_bank(n, m, nm, N, T, seed):
    rs = np.random.RandomState(seed)
    Fs = np.array([stable_F(rs, n) for _ in range(nm)])
    Qs = np.array([spd(rs, n, 0.05 * (j % 5 + 1)) for j in range(nm)])
    Hs = np.array([rs.randn(m, n) for _ in range(nm)])
    Rs = np.array([spd(rs, m, 0.5) for _ in range(nm)])
    M = rs.rand(nm, nm) + 2 * np.eye(nm)
    M /= M.sum(axis=1, keepdims=True)
    xs0 = rs.randn(N, nm, n)
    Ps0 = np.array([[spd(rs, n, 2.0) for _ in range(nm)] for _ in range(N)])
    mu0 = rs.rand(N, nm) + 0.1
    mu0 /= mu0.sum(axis=1, keepdims=True)
    zs = rs.randn(T, N, m) * 2
    return xs0, Ps0, mu0, M, zs, Fs, Qs, Hs, Rs


@pytest.mark.parametrize("layout", ["soa", "aos"])
@pytest.mark.parametrize("n,m,nm", LANES_CASES + QUAD_CASES)
def test_imm_lanes_kernel_vs_oracle(n, m, nm, layout):
    """banks the one-lane-per-filter kernel (and, above (9,4), the four-lanes-per-filter kernel) serves (IMM.py:160-249), N not a multiple of the banks of a wave or a block, every
    bank checked at its ends: per-step estimate, prior, mode probabilities, likelihoods and the bank's final state"""
    from gpu_util import run_imm
    from oracle import imm_oracle
    N, T = 203, 7
    b = _lanes_bank(n, m, nm, N, T, 500 + 10 * n + nm)
    xs0, Ps0, mu0, M, zs, Fs, Qs, Hs, Rs = b
    r = run_imm(*b, layout)
    assert np.isfinite(r["x_out"]).all() and np.isfinite(r["P_out"]).all() and np.isfinite(r["mu_out"]).all()
    for trk in (0, 1, 3, 4, 7, 8, 15, 16, 31, 32, 63, 64, 127, 128, 200, 201, N - 1):
        x, P, mu, xp, Pp, L = imm_oracle.imm_batch(xs0[trk], Ps0[trk], mu0[trk], M, zs[:, trk], Fs, Qs, Hs, Rs)
        assert rel_err_rows(r["x_out"][:, trk], x) < TOL and rel_err_rows(r["P_out"][:, trk], P) < TOL
        assert rel_err_rows(r["x_prior_out"][:, trk], xp) < TOL and rel_err_rows(r["P_prior_out"][:, trk], Pp) < TOL
        assert np.allclose(r["mu_out"][:, trk], mu, rtol=1e-10, atol=1e-14)
        assert np.allclose(r["likelihood_out"][:, trk], L, rtol=1e-10, atol=1e-300)
        assert np.allclose(r["mu"][trk], mu[-1], rtol=1e-10, atol=1e-14)
    # the bank's final state: a second call that continues from it equals one call over both halves
    r2 = run_imm(r["xs"], r["Ps"], r["mu"], M, zs[:3], Fs, Qs, Hs, Rs, layout)
    for trk in (0, 100, N - 1):
        x, P, mu, _, _, _ = imm_oracle.imm_batch(xs0[trk], Ps0[trk], mu0[trk], M, np.concatenate([zs[:, trk], zs[:3, trk]]), Fs, Qs, Hs, Rs)
        assert rel_err_rows(r2["x_out"][:, trk], x[T:]) < TOL and rel_err_rows(r2["P_out"][:, trk], P[T:]) < TOL


@pytest.mark.parametrize("layout", ["soa", "aos"])
@pytest.mark.parametrize("dims", [(8, 3, 6), (14, 6, 5)])
@pytest.mark.parametrize("outs", [("x_out",), ("P_out", "mu_out"), ("x_prior_out", "P_prior_out"), ("likelihood_out",), ()])
def test_imm_lanes_kernel_output_subsets(outs, layout, dims):
    """any subset of the per-step outputs (the pointers are tested at run time): what is asked for equals the all-outputs call
    bit for bit, and so does the final state of the bank"""
    from gpu_util import run_imm
    import torch
    from filterpy_amd import _engine as E
    (n, m, nm), N, T = dims, 77, 5
    b = _lanes_bank(n, m, nm, N, T, 77)
    xs0, Ps0, mu0, M, zs, Fs, Qs, Hs, Rs = b
    full = run_imm(*b, layout)
    dxs = E.to_records(xs0.reshape(N, nm * n), layout, 0)
    dPs = E.to_records(Ps0.reshape(N, nm * n * n), layout, 0)
    dmu = E.to_records(mu0, layout, 0)
    dz = E.to_records(zs, layout, 1)
    sizes = dict(x_out=n, P_out=n * n, mu_out=nm, likelihood_out=nm, x_prior_out=n, P_prior_out=n * n)
    shapes = dict(x_out=(n,), P_out=(n, n), mu_out=(nm,), likelihood_out=(nm,), x_prior_out=(n,), P_prior_out=(n, n))
    out = {k: E.alloc_records((T,), N, sizes[k], layout) for k in outs}
    st = torch.zeros(N, dtype=torch.int32, device=dxs.device)
    E.imm_batch(n, m, nm, N, T, layout, E.dev(Fs), E.dev(Qs), E.dev(Hs), E.dev(Rs), E.dev(M), dz, dxs, dPs, dmu, status=st, **out)
    torch.cuda.synchronize()
    assert not st.any()
    for k, v in out.items():
        assert np.array_equal(E.from_records(v, layout, 1, shapes[k]), full[k]), k
    assert np.array_equal(E.from_records(dxs, layout, 0, (nm, n)), full["xs"])
    assert np.array_equal(E.from_records(dPs, layout, 0, (nm, n, n)), full["Ps"])
    assert np.array_equal(E.from_records(dmu, layout, 0, (nm,)), full["mu"])


def test_imm_lanes_kernel_against_the_one_lane_per_bank_kernels():
    """The small banks (2 / 3 filters, dim_x <= 6, dim_z <= 3) run on the register-resident one-lane-per-BANK kernels of
    imm_kernels.hip by default and on imm_lanes.hip with FK_IMM_LANES=2 (read once per process: two subprocesses): two
    independent implementations of IMM.py:160-249, every record of both within 1e-11 of each other (normwise per bank and step).
    (Rounds 3-6 also built one-lane-per-bank kernels for the classes (9,4) and (16,8); they were compared with imm_lanes.hip /
    imm_quad.hip here -- profiles/r06/imm_lanes/ -- before they were removed from the build.)"""
    import os
    import subprocess
    import sys
    import tempfile
    code = r'''
import sys, numpy as np
sys.path.insert(0, "tests")
import test_gpu_imm as t
from gpu_util import run_imm
res = {}
for (n, m, nm) in [(6, 3, 3), (4, 2, 2), (2, 1, 3), (5, 2, 2)]:
    b = t._lanes_bank(n, m, nm, 150, 6, 9 + nm)
    for layout in ("soa", "aos"):
        r = run_imm(*b, layout)
        for k in ("x_out", "P_out", "mu_out", "likelihood_out", "x_prior_out", "P_prior_out", "xs", "Ps", "mu"):
            res[f"{n}_{m}_{nm}_{layout}_{k}"] = r[k]
np.savez(sys.argv[1], **res)
'''
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    got = {}
    with tempfile.TemporaryDirectory() as td:
        for mode in ("1", "2"):
            f = os.path.join(td, f"m{mode}.npz")
            env = dict(os.environ, FK_IMM_LANES=mode, PYTHONPATH=root + os.pathsep + os.environ.get("PYTHONPATH", ""))
            subprocess.run([sys.executable, "-c", code, f], check=True, cwd=root, env=env, timeout=600)
            got[mode] = dict(np.load(f))
    assert got["1"].keys() == got["2"].keys() and len(got["1"]) == 72
    for k in got["1"]:
        a, b = got["1"][k], got["2"][k]
        w = a.shape[-1] * (a.shape[-2] if k.endswith(("P_out", "Ps")) else 1)
        assert rel_err_rows(a.reshape(-1, w), b.reshape(-1, w)) < 1e-11, k


def test_imm_eight_lanes_per_filter_against_four():
    """Banks of two filters of the class (16,8) run on imm_quad.hip built with EIGHT lanes per filter (imm_oct_*); FK_IMM_OCT=0 (read once per
    process: two subprocesses) runs them on the four-lane build: same arithmetic, another distribution of it -- every record of both
    within 1e-11 of each other (normwise per bank and step)"""
    import os
    import subprocess
    import sys
    import tempfile
    code = r'''
import sys, numpy as np
sys.path.insert(0, "tests")
import test_gpu_imm as t
from gpu_util import run_imm
res = {}
for (n, m, nm) in [(16, 8, 2), (13, 5, 2), (10, 7, 2)]:
    b = t._lanes_bank(n, m, nm, 150, 6, 19 + n)
    for layout in ("soa", "aos"):
        r = run_imm(*b, layout)
        for k in ("x_out", "P_out", "mu_out", "likelihood_out", "x_prior_out", "P_prior_out", "xs", "Ps", "mu"):
            res[f"{n}_{m}_{nm}_{layout}_{k}"] = r[k]
np.savez(sys.argv[1], **res)
'''
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    got = {}
    with tempfile.TemporaryDirectory() as td:
        for mode in ("0", "1"):
            f = os.path.join(td, f"m{mode}.npz")
            env = dict(os.environ, FK_IMM_OCT=mode, PYTHONPATH=root + os.pathsep + os.environ.get("PYTHONPATH", ""))
            subprocess.run([sys.executable, "-c", code, f], check=True, cwd=root, env=env, timeout=600)
            got[mode] = dict(np.load(f))
    assert got["0"].keys() == got["1"].keys() and len(got["0"]) == 54
    differs = False
    for k in got["0"]:
        a, b = got["0"][k], got["1"][k]
        w = a.shape[-1] * (a.shape[-2] if k.endswith(("P_out", "Ps")) else 1)
        assert rel_err_rows(a.reshape(-1, w), b.reshape(-1, w)) < 1e-11, k
        differs = differs or not np.array_equal(a, b)


@pytest.mark.parametrize("layout", ["soa", "aos"])
@pytest.mark.parametrize("kind", ["imm", "mmae"])
@pytest.mark.parametrize("n,m,nm,nu", [(9, 4, 8, 2), (6, 3, 5, 1), (4, 2, 4, 3), (7, 2, 12, 0), (8, 3, 3, 4),
                                       (12, 4, 3, 2), (16, 8, 2, 1), (13, 5, 9, 0), (10, 6, 6, 4)])
def test_imm_lanes_kernel_missing_measurements_control_mmae_vs_oracle(n, m, nm, nu, kind, layout):
    """the extended instantiation of the one-lane-per-filter kernel: every bank its own pattern of missing measurements
    (update(None): IMM.py:171-179 + kalman_filter.py:511-520), a control input per bank and step with every filter's own B
    (kalman_filter.py:472-475), IMM and MMAE (mmae.py:140-207) -- one launch, against the oracle bank by bank; the zero-residual
    log-densities carried over a second call (ll0)"""
    import torch
    from filterpy_amd import _engine as E
    from oracle import imm_oracle
    N, T = 45, 9
    xs0, Ps0, mu0, M, zs, Fs, Qs, Hs, Rs = _lanes_bank(n, m, nm, N, T, 900 + n + nm)
    rs = np.random.RandomState(5 + n)
    mask = (rs.rand(T, N) > 0.3).astype(np.uint8)
    mask[0, ::3] = 0                                              # some banks start with update(None): S = 0, density floored
    Bs = rs.randn(nm, n, nu) if nu else None
    us = rs.randn(T, N, nu) if nu else None
    mmae = kind == "mmae"

    def call(xs_, Ps_, mu_, zs_, mask_, us_, ll0_):
        Tn = len(zs_)
        dxs = E.to_records(xs_.reshape(N, nm * n), layout, 0)
        dPs = E.to_records(Ps_.reshape(N, nm * n * n), layout, 0)
        dmu = E.to_records(mu_, layout, 0)
        out = dict(x_out=E.alloc_records((Tn,), N, n, layout), P_out=E.alloc_records((Tn,), N, n * n, layout),
                   mu_out=E.alloc_records((Tn,), N, nm, layout), likelihood_out=E.alloc_records((Tn,), N, nm, layout))
        st = torch.zeros(N, dtype=torch.int32, device=dxs.device)
        dll0 = E.to_records(ll0_, layout, 0)
        kw = dict(nu=nu, B=E.dev(Bs), u=E.to_records(us_, layout, 1)) if nu else {}
        E.imm_batch(n, m, nm, N, Tn, layout, E.dev(Fs), E.dev(Qs), E.dev(Hs), E.dev(Rs), None if mmae else E.dev(M),
                    E.to_records(zs_, layout, 1), dxs, dPs, dmu, status=st, mmae=mmae,
                    zmask=torch.as_tensor(np.ascontiguousarray(mask_), device=dxs.device), ll0=dll0, **kw, **out)
        torch.cuda.synchronize()
        assert not st.any()
        shapes = dict(x_out=(n,), P_out=(n, n), mu_out=(nm,), likelihood_out=(nm,))
        r = {k: E.from_records(v, layout, 1, shapes[k]) for k, v in out.items()}
        r.update(xs=E.from_records(dxs, layout, 0, (nm, n)), Ps=E.from_records(dPs, layout, 0, (nm, n, n)),
                 mu=E.from_records(dmu, layout, 0, (nm,)), ll0=E.from_records(dll0, layout, 0, (nm,)))
        return r

    T1 = 5
    r1 = call(xs0, Ps0, mu0, zs[:T1], mask[:T1], None if us is None else us[:T1], np.full((N, nm), -np.inf))
    r2 = call(r1["xs"], r1["Ps"], r1["mu"], zs[T1:], mask[T1:], None if us is None else us[T1:], r1["ll0"])
    for trk in (0, 1, 2, 3, 7, 8, 31, 32, N - 1):
        zl = [zs[t, trk] if mask[t, trk] else None for t in range(T)]
        ul = None if us is None else us[:, trk]
        if mmae:
            x, P, mu, L = imm_oracle.mmae_batch(xs0[trk], Ps0[trk], mu0[trk], zl, Fs, Qs, Hs, Rs, Bs, ul)
        else:
            x, P, mu, _, _, L = imm_oracle.imm_batch(xs0[trk], Ps0[trk], mu0[trk], M, zl, Fs, Qs, Hs, Rs, Bs, ul)
        for r, sl in ((r1, slice(0, T1)), (r2, slice(T1, T))):
            assert rel_err_rows(r["x_out"][:, trk], x[sl]) < TOL and rel_err_rows(r["P_out"][:, trk], P[sl]) < TOL
            assert np.allclose(r["mu_out"][:, trk], mu[sl], rtol=1e-9, atol=1e-14)
            assert np.allclose(r["likelihood_out"][:, trk], L[sl], rtol=1e-9, atol=1e-300)
