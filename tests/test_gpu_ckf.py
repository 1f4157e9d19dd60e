"""The cubature Kalman filter's kernels on an MI355X against tests/ckf_port.py, the restatement of the reference that
tests/test_host_ckf.py holds to the goldens of the live reference: the fused matrix-model kernel (fast and general, both
layouts), the building blocks, and the class in its four modes, on every output; chained calls, masks, NULL histories and a
track whose P is indefinite bit for bit.  Tolerance per case: max(K_BAR err(port, hp), 1e-12) normwise per step and track, the
worst step, no track excluded (K_BAR: tests/ckf_models.py; err(port, hp): the port's own worst error against tests/ckf_hp.py on
the case's model)."""
import math

import numpy as np
import pytest
import torch

import ckf_hp
import ckf_models
import ckf_port as cp
from filterpy_amd import _engine as E
from filterpy_amd import _abi
from filterpy_amd.kalman import CubatureKalmanFilter
from filterpy_amd.kalman._bank import _desc

pytestmark = pytest.mark.gpu

BLOCK = 256
DIMS = [(1, 1), (2, 1), (4, 2), (6, 3), (9, 4), (16, 8), (5, 4)]      # (5, 4), (9, 4), (16, 8): only the general kernel takes them
NS = (1, 63, 65, BLOCK + 1)
DISTINCT, TMAX = 65, 5
LAYOUTS = ("soa", "aos")
_cases = {}


def case(dims):
    """model, DISTINCT different tracks (the bank repeats them), the port's histories and the case's tolerance; computed once"""
    if dims not in _cases:
        n, m = dims
        rs = np.random.RandomState(100 * n + m)
        d = dict(F=np.eye(n) + 0.1 * rs.randn(n, n) / np.sqrt(n), H=rs.randn(m, n), Q=cp.spd(rs, n, 0.02), R=cp.spd(rs, m, 0.5),
                 x0=rs.randn(DISTINCT, n), P0=np.array([cp.spd(rs, n, 0.7) for _ in range(DISTINCT)]),
                 zs=rs.randn(TMAX, DISTINCT, m))
        port, sig, perr = {}, {}, 0.0
        for T in (1, TMAX):
            res = [cp.batch(d["x0"][i], d["P0"][i], d["zs"][:T, i], d["F"], d["Q"], d["H"], d["R"]) for i in range(DISTINCT)]
            port[T] = [np.stack([r[j] for r in res], axis=1) for j in range(4)]
            sig[T] = np.stack([r[4].sigmas_f for r in res])
        by = {k: np.zeros((TMAX, DISTINCT) + s) for k, s in BY_SHAPES(n, m).items()}
        for i in range(DISTINCT):
            for t, b in enumerate(port_by_products(d, i, float)):
                for k in by:
                    by[k][t, i] = b[k]
        for i in range(DISTINCT):
            hp = ckf_hp.batch(d["x0"][i], d["P0"][i], d["zs"][:, i], d["F"], d["Q"], d["H"], d["R"])
            perr = max(perr, max(ckf_models.err(port[TMAX][j][:, i], hp[j]) for j in range(4)))
            hb = port_by_products(d, i, ckf_hp.LD)
            perr = max(perr, max(ckf_models.err(by[k][:, i], np.stack([b[k] for b in hb])) for k in by))
        d.update(port=port, sig=sig, by=by, tol=max(ckf_models.K_BAR * perr, 1e-12))
        _cases[dims] = d
    return _cases[dims]


def BY_SHAPES(n, m):
    return dict(K=(n, m), S=(m, m), SI=(m, m), y=(m,), Pxz=(n, m), zp=(m,))


def port_by_products(d, i, dtype):
    """track i of a case through tests/ckf_port.py, step by step: K, S, SI, y, Pxz and zp after every update, in float64 or (the
    lines of tests/ckf_hp.py) in longdouble.  Pxz and zp as CubatureKalmanFilter.py:366-373 forms them."""
    kw = {} if dtype is float else dict(dtype=dtype, chol=ckf_hp.chol_upper, inv=ckf_hp.inv)
    F, Q, H, R = (np.asarray(d[k], dtype=dtype) for k in "FQHR")
    n, m = F.shape[0], H.shape[0]
    f = cp.Port(n, m, 1.0, lambda s: H @ s, lambda s, dt: F @ s, **kw)
    f.x, f.P, f.Q, f.R = np.asarray(d["x0"][i], dtype=dtype).reshape(n, 1), np.asarray(d["P0"][i], dtype=dtype).copy(), Q, R
    out = []
    for t in range(TMAX):
        f.predict()
        xf = f.x.flatten()
        f.update(np.asarray(d["zs"][t, i], dtype=dtype).reshape(m, 1))
        zp = sum(f.sigmas_h, 0) / (2 * n)
        out.append(dict(K=f.K, S=f.S, SI=f.SI, y=f.y[:, 0], zp=zp, Pxz=cp.outer_product_sum(f.sigmas_f - xf, f.sigmas_h - zp) / (2 * n)))
    return out


def check_by_products(d, dims, N, t, layout, recs, what):
    """every by-product record of every track against the port's at step t, at the case's bar"""
    n, m = dims
    for k, rec in recs.items():
        got = E.from_records(rec, layout, 0, BY_SHAPES(n, m)[k])
        e = _worst(got, tile(d["by"][k][t], N), 1)
        print(what, dims, layout, "N", N, "t", t, k, "err %.2e tol %.2e" % (e, d["tol"]))
        assert e <= d["tol"], (what, dims, N, t, k, e)


def tile(a, N, axis=0):
    idx = np.arange(N) % DISTINCT
    return np.take(a, idx, axis=axis)


def _worst(a, b, lead):
    """worst normwise relative error over the records of a against b; lead: the number of leading (step, track) axes"""
    a, b = np.asarray(a, dtype=float), np.asarray(b, dtype=float)
    assert a.shape == b.shape, (a.shape, b.shape)
    a2, b2 = a.reshape(int(np.prod(a.shape[:lead])), -1), b.reshape(int(np.prod(b.shape[:lead])), -1)
    scale = np.abs(b2).max(axis=1)
    scale[scale == 0] = 1.0
    return float((np.abs(a2 - b2).max(axis=1) / scale).max())


def sigmas_from_points(pts, n):
    c, Eh = pts[:, None, :n], pts[:, n:].reshape(-1, n, n) * math.sqrt(n)
    return np.concatenate([c + Eh, c - Eh], axis=1)


def run_batch(d, dims, N, T, layout, *, mask=None, outputs=True, x0=None, P0=None, pts0=None, zs=None, check=True):
    """fk_ckf_linear_batch_f64 through the C ABI -> (four histories or Nones, x, P, points, status), host arrays"""
    n, m = dims
    x0 = tile(d["x0"], N) if x0 is None else x0
    P0 = tile(d["P0"], N) if P0 is None else P0
    zs = tile(d["zs"][:T], N, axis=1) if zs is None else zs
    pts0 = np.zeros((N, n + n * n)) if pts0 is None else pts0
    dx, dP, dpts = (E.to_records(a, layout, 0).clone() for a in (x0, P0, pts0))
    dz = E.to_records(zs, layout, 1)
    outs = [None] * 4
    if outputs:
        outs = [E.alloc_records((T,), N, e, layout).fill_(float("nan")) for e in (n, n * n, n, n * n)]
    st = torch.zeros(N, dtype=torch.int32, device=dx.device)
    dm = None if mask is None else torch.as_tensor(np.ascontiguousarray(mask, dtype=np.uint8), device=dx.device)
    E.ckf_linear_batch(_desc(n, m, 0, N, T, layout), E.dev(d["F"]), E.dev(d["Q"]), E.dev(d["H"]), E.dev(d["R"]), dz, dx, dP, dpts,
                       mask=dm, means=outs[0], covs=outs[1], means_p=outs[2], covs_p=outs[3], status=st)
    torch.cuda.synchronize()
    res = [E.from_records(o, layout, 1, s) if o is not None else None for o, s in zip(outs, ((n,), (n, n), (n,), (n, n)))]
    res += [E.from_records(dx, layout, 0, (n,)), E.from_records(dP, layout, 0, (n, n)), E.from_records(dpts, layout, 0, (n + n * n,)),
            st.cpu().numpy()]
    if check:
        assert not res[-1].any(), res[-1][res[-1] != 0][:8]
    return res


def check_against_port(d, dims, N, T, got, what):
    n = dims[0]
    for j, name in enumerate(("means", "covs", "means_p", "covs_p")):
        e = _worst(got[j], tile(d["port"][T][j], N, axis=1), 2)
        print(what, dims, "N", N, "T", T, name, "err %.2e tol %.2e" % (e, d["tol"]))
        assert e <= d["tol"], (what, dims, N, T, name, e)
    assert np.array_equal(got[4], got[0][-1]) and np.array_equal(got[5], got[1][-1])         # the state out IS the last posterior
    e = _worst(sigmas_from_points(got[6], n), tile(d["sig"][T], N), 1)
    assert e <= d["tol"], (what, dims, N, T, "points", e)
    assert np.array_equal(got[1], np.swapaxes(got[1], -1, -2))                                 # P leaves exactly symmetric


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("dims", DIMS)
def test_fused_kernel_matches_port(dims, layout):
    d = case(dims)
    for N in NS:
        for T in (1, TMAX):
            check_against_port(d, dims, N, T, run_batch(d, dims, N, T, layout), "fused " + layout)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("dims", [(1, 1), (2, 1), (4, 2), (6, 3)])
def test_general_kernel_matches_port_at_the_fast_shapes(dims, layout, monkeypatch):
    """FK_CKF_GENERAL=1 (read at every call) sends a shape with a fast kernel to the padded general one"""
    d = case(dims)
    fast = run_batch(d, dims, 65, TMAX, layout)
    monkeypatch.setenv("FK_CKF_GENERAL", "1")
    for N in NS:
        check_against_port(d, dims, N, TMAX, run_batch(d, dims, N, TMAX, layout), "general " + layout)
    gen = run_batch(d, dims, 65, TMAX, layout)
    monkeypatch.delenv("FK_CKF_GENERAL")
    assert all(_worst(a, b, 1) <= d["tol"] for a, b in zip(gen[:7], fast[:7]))
    assert all(np.array_equal(a, b) for a, b in zip(run_batch(d, dims, 65, TMAX, layout)[:7], fast[:7]))


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("dims", DIMS)
def test_chained_calls_are_bit_identical(dims, layout):
    """one call against the run split at every step and at an odd split: histories and final state, the same bytes"""
    d = case(dims)
    n = dims[0]
    for N in (65, BLOCK + 1):
        whole = run_batch(d, dims, N, TMAX, layout)
        zs = tile(d["zs"], N, axis=1)
        for cuts in ([1, 2, 3, 4], [3]):
            x, P, pts = tile(d["x0"], N), tile(d["P0"], N), np.zeros((N, n + n * n))
            parts, t0 = [], 0
            for t1 in cuts + [TMAX]:
                r = run_batch(d, dims, N, t1 - t0, layout, x0=x, P0=P, pts0=pts, zs=zs[t0:t1])
                parts.append(r)
                x, P, pts, t0 = r[4], r[5], r[6], t1
            for j in range(4):
                assert np.array_equal(np.concatenate([p[j] for p in parts]), whole[j]), (dims, N, cuts, j)
            for j in (4, 5, 6):
                assert np.array_equal(parts[-1][j], whole[j]), (dims, N, cuts, j)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("dims", [(2, 1), (4, 2), (6, 3), (5, 4), (16, 8)])
def test_single_steps_chain_to_the_batch(dims, layout):
    """fk_ckf_linear_predict_f64 / fk_ckf_linear_update_f64 on the same state: T predict + update pairs are the batch's bytes,
    and their by-products match the port's"""
    d = case(dims)
    for N in NS:
        _single_steps(d, dims, N, layout)


def _single_steps(d, dims, N, layout):
    n, m = dims
    whole = run_batch(d, dims, N, TMAX, layout)
    dx, dP = E.to_records(tile(d["x0"], N), layout, 0).clone(), E.to_records(tile(d["P0"], N), layout, 0).clone()
    dpts = E.alloc_records((), N, n + n * n, layout).zero_()
    st = torch.zeros(N, dtype=torch.int32, device=dx.device)
    by = dict(y=E.alloc_records((), N, m, layout), K=E.alloc_records((), N, n * m, layout), S=E.alloc_records((), N, m * m, layout),
              SI=E.alloc_records((), N, m * m, layout))
    dF, dQ, dH, dR = (E.dev(d[k]) for k in "FQHR")
    for t in range(TMAX):
        E.ckf_linear_predict(_desc(n, m, 0, N, 1, layout), dF, dQ, dx, dP, dpts, status=st)
        assert np.array_equal(E.from_records(dx, layout, 0, (n,)), whole[2][t])
        assert np.array_equal(E.from_records(dP, layout, 0, (n, n)), whole[3][t])
        E.ckf_linear_update(_desc(n, m, 0, N, 1, layout), dH, dR, E.to_records(tile(d["zs"][t], N), layout, 0), dx, dP, dpts,
                            status=st, **by)
        assert np.array_equal(E.from_records(dx, layout, 0, (n,)), whole[0][t])
        assert np.array_equal(E.from_records(dP, layout, 0, (n, n)), whole[1][t])
        check_by_products(d, dims, N, t, layout, by, "single step")
    assert not st.cpu().numpy().any()


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("dims", [(2, 1), (4, 2), (5, 4)])
def test_masked_steps_are_update_none(dims, layout):
    """a missing first measurement, a missing last one and two missing in a row (per track, four patterns) = update(None)"""
    d = case(dims)
    for N in NS:
        _masked(d, dims, N, layout)


def _masked(d, dims, N, layout):
    T = TMAX
    pat = np.array([[0, 1, 1, 1, 1], [1, 1, 1, 1, 0], [1, 0, 0, 1, 1], [0, 1, 0, 0, 0]], dtype=bool)
    mask = pat[np.arange(N) % 4].T                                   # (T, N)
    got = run_batch(d, dims, N, T, layout, mask=mask)
    want = cp.batch_tracks(tile(d["x0"], N), tile(d["P0"], N), tile(d["zs"], N, axis=1), d["F"], d["Q"], d["H"], d["R"], mask)
    for j in range(4):
        assert _worst(got[j], want[j], 2) <= d["tol"], (dims, j)
    miss = ~mask
    assert np.array_equal(got[0][miss], got[2][miss]) and np.array_equal(got[1][miss], got[3][miss])      # untouched, bit for bit


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("dims", [(4, 2), (6, 3), (5, 4)])
def test_null_histories_leave_the_final_state_unchanged(dims, layout):
    d = case(dims)
    for N in NS:
        a, b = run_batch(d, dims, N, TMAX, layout), run_batch(d, dims, N, TMAX, layout, outputs=False)
        assert all(np.array_equal(a[j], b[j]) for j in (4, 5, 6, 7))


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("dims", [(4, 2), (6, 3), (5, 4)])
def test_indefinite_p_is_flagged_and_leaves_its_neighbours_alone(dims, layout):
    d = case(dims)
    for N, bad in ((1, 0), (63, 62), (65, 37), (BLOCK + 1, BLOCK)):
        _indefinite(d, dims, N, bad, layout)


def _indefinite(d, dims, N, bad, layout):
    n = dims[0]
    P0 = tile(d["P0"], N).copy()
    w, V = np.linalg.eigh(P0[bad])
    w[0] = -0.3                                                     # one negative eigenvalue
    P0[bad] = (V * w) @ V.T
    P0[bad] = (P0[bad] + P0[bad].T) / 2
    good = run_batch(d, dims, N, TMAX, layout)
    got = run_batch(d, dims, N, TMAX, layout, P0=P0, check=False)
    assert got[7][bad] & _abi.FK_STATUS_NOT_PD and not np.delete(got[7], bad).any()
    for j in range(4):
        assert np.array_equal(np.delete(got[j], bad, axis=1), np.delete(good[j], bad, axis=1))
    for j in (4, 5, 6):
        assert np.array_equal(np.delete(got[j], bad, axis=0), np.delete(good[j], bad, axis=0))
    f = CubatureKalmanFilter(n, dims[1], 1.0, d["H"], d["F"], n_tracks=N, layout=layout)
    f.x, f.P, f.Q, f.R = tile(d["x0"], N), P0, d["Q"], d["R"]
    with pytest.raises(np.linalg.LinAlgError):
        f.batch_filter(tile(d["zs"], N, axis=1))


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("dims", DIMS)
def test_building_blocks_match_port(dims, layout):
    """fk_ckf_sigma_points_f64, fk_ckf_transform_f64 and fk_ckf_update_f64 (one launch) through the C ABI, track by track"""
    d = case(dims)
    n, m = dims
    tol = d["tol"]
    for N in NS:
        x0, P0 = tile(d["x0"], N), tile(d["P0"], N)
        dx, dP = E.to_records(x0, layout, 0).clone(), E.to_records(P0, layout, 0).clone()
        sig = E.alloc_records((), N, 2 * n * n, layout)
        st = torch.zeros(N, dtype=torch.int32, device=dx.device)
        E.ckf_sigma_points(n, N, layout, dx, dP, sig, st)
        s = E.from_records(sig, layout, 0, (2 * n, n))
        want_s = np.stack([cp.spherical_radial_sigmas(d["x0"][i], d["P0"][i]) for i in range(min(N, DISTINCT))])
        assert _worst(s, tile(want_s, N), 1) <= tol
        sf = s @ d["F"].T
        dsf = E.to_records(sf, layout, 0)
        E.ckf_transform(n, 2 * n, N, layout, dsf, E.dev(d["Q"]), dx, dP)
        xp, Pp = E.from_records(dx, layout, 0, (n,)), E.from_records(dP, layout, 0, (n, n))
        assert _worst(xp, tile(d["port"][1][2][0], N), 1) <= tol and _worst(Pp, tile(d["port"][1][3][0], N), 1) <= tol
        sh = sf @ d["H"].T
        by = {k: E.alloc_records((), N, e, layout) for k, e in (("zp", m), ("S", m * m), ("SI", m * m), ("Pxz", n * m),
                                                                ("K", n * m), ("y", m))}
        E.ckf_update(n, m, N, layout, dsf, E.to_records(sh, layout, 0), E.dev(d["R"]), E.to_records(tile(d["zs"][0], N), layout, 0),
                     dx, dP, status=st, **by)
        assert not st.cpu().numpy().any()
        xo, Po = E.from_records(dx, layout, 0, (n,)), E.from_records(dP, layout, 0, (n, n))
        assert _worst(xo, tile(d["port"][1][0][0], N), 1) <= tol and _worst(Po, tile(d["port"][1][1][0], N), 1) <= tol
        check_by_products(d, dims, N, 0, layout, by, "update block")            # zp, S, SI, Pxz, K, y: every track
        zp = E.from_records(by["zp"], layout, 0, (m,))
        # zp == NULL: z already holds y -- the same update from the caller's residual
        dx2, dP2 = E.to_records(xp, layout, 0).clone(), E.to_records(Pp, layout, 0).clone()
        y = tile(d["zs"][0], N) - zp
        E.ckf_update(n, m, N, layout, dsf, E.to_records(sh, layout, 0), E.dev(d["R"]), E.to_records(y, layout, 0), dx2, dP2, zp=None,
                     status=st)
        assert np.array_equal(E.from_records(dx2, layout, 0, (n,)), xo) and np.array_equal(E.from_records(dP2, layout, 0, (n, n)), Po)


def _bank(mode, n, m, N, d, layout):
    kw = dict(n_tracks=N, layout=layout)
    if mode == "matrix":
        return CubatureKalmanFilter(n, m, 1.0, d["H"], d["F"], **kw)
    if mode == "loop":
        return CubatureKalmanFilter(n, m, 1.0, lambda s: d["H"] @ s, lambda s, dt: d["F"] @ s, **kw)
    if mode == "vec":
        return CubatureKalmanFilter(n, m, 1.0, lambda s: s @ d["H"].T, lambda s, dt: s @ d["F"].T, vectorized=True, **kw)
    Ft, Ht = E.dev(d["F"]), E.dev(d["H"])
    return CubatureKalmanFilter(n, m, 1.0, lambda s: s @ Ht.T, lambda s, dt: s @ Ft.T, device_callables=True, **kw)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_class_modes_agree(layout):
    """host callables, vectorized, device_callables and matrices at (4, 2), N = 65: batch_filter and the step methods"""
    dims, N = (4, 2), 65
    n, m = dims
    d = case(dims)
    want = [tile(a, N, axis=1) for a in d["port"][TMAX]]
    for mode in ("matrix", "loop", "vec", "torch"):
        b = _bank(mode, n, m, N, d, layout)
        b.x, b.P, b.Q, b.R = tile(d["x0"], N), tile(d["P0"], N), d["Q"], d["R"]
        got = b.batch_filter(tile(d["zs"], N, axis=1))
        for j in range(4):
            assert _worst(got[j], want[j], 2) <= d["tol"], (mode, j)
        assert _worst(b.sigmas_f, tile(d["sig"][TMAX], N), 1) <= d["tol"] and np.array_equal(b.x, got[0][-1])
        s = _bank(mode, n, m, N, d, layout)
        s.x, s.P, s.Q, s.R = tile(d["x0"], N), tile(d["P0"], N), d["Q"], d["R"]
        for t in range(2):
            s.predict()
            s.update(tile(d["zs"][t], N))
        assert _worst(s.x, want[0][1], 1) <= d["tol"] and _worst(s.P, want[1][1], 1) <= d["tol"]
        assert s.K.shape == (N, n, m) and s.y.shape == (N, m) and s.sigmas_h.shape == (N, 2 * n, m)


def test_single_filter_on_the_golden_sequences():
    """the class as one filter, Python callables per point: the nonlinear golden case (4, 2) with its custom residual_z, and the
    matrix model on the linear one -- every attribute after every call"""
    from conftest import golden, rel_err
    G = golden("ckf")
    for spec in [s for s in cp.specs() if (s[1], s[2]) == (4, 2)]:
        dd = cp.inputs(*spec[:4])
        fs = [cp.make(CubatureKalmanFilter, spec, dd)]
        if spec[3] == cp.LINEAR:
            fs.append(cp.setup(CubatureKalmanFilter(4, 2, cp.DT, dd["H"], dd["F"]), spec, dd))
        for k in range(cp.n_ops(spec)):
            for f in fs:
                cp.run_op(f, spec, dd, k)
                for a in ("x", "P", "K", "y", "S", "SI", "sigmas_f", "sigmas_h", "x_prior", "P_post", "log_likelihood", "mahalanobis"):
                    ref = cp.attr(G, f"c{spec[0]}_", k, a)
                    if ref is not None:
                        mine = np.asarray(getattr(f, a), dtype=float)
                        assert mine.shape == ref.shape and rel_err(mine, ref) <= 1e-10, (spec, k, a)
