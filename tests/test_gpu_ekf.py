"""The extended Kalman filter's kernels on an MI355X against tests/ekf_port.py, the restatement of the reference that
tests/test_host_ekf.py holds to the goldens of the live reference: the three entry points through filterpy_amd._engine on every
output and by-product (fast and general kernels, both layouts, shared and per-track F / Q / R / B, control input, masks, NULL
by-products), one track with an indefinite S bit for bit, the layouts and the fused step bit for bit, and the class in its three
callable modes.

Tolerance of the engine tests: max(K_BAR err(port, hp), 1e-12) normwise per record, no track excluded (K_BAR: tests/ekf_models.py;
err(port, hp): the port's own worst error against tests/ekf_hp.py on the case's model -- well conditioned, so the 1e-12 floor
of the project's bar decides)."""
import numpy as np
import pytest
import torch

import ekf_hp
import ekf_models as em
import ekf_port as ep
from filterpy_amd import _abi
from filterpy_amd import _engine as E
from filterpy_amd.kalman import ExtendedKalmanFilter

pytestmark = pytest.mark.gpu

BLOCK = 256
DIMS = [(1, 1), (2, 1), (3, 1), (4, 2), (6, 3), (8, 4), (5, 4), (9, 4), (16, 8)]    # from (8, 4) on: the general kernel
NS = (1, 63, 65, BLOCK + 1)
DISTINCT, NU = 65, 2
LAYOUTS = ("soa", "aos")
_cases = {}


def spd(rs, k, scale):
    A = rs.randn(k, k)
    return scale * (A @ A.T / k + np.eye(k))


def case(dims):
    """DISTINCT different tracks (a bank repeats them): inputs, per-track models and the port's results; computed once"""
    if dims not in _cases:
        n, m = dims
        rs = np.random.RandomState(100 * n + m)
        d = dict(x=rs.randn(DISTINCT, n), P=np.array([spd(rs, n, 0.7) for _ in range(DISTINCT)]), H=rs.randn(DISTINCT, m, n),
                 y=rs.randn(DISTINCT, m), u=rs.randn(DISTINCT, NU),
                 F=np.eye(n) + 0.1 * rs.randn(DISTINCT, n, n) / np.sqrt(n), Q=np.array([spd(rs, n, 0.02) for _ in range(DISTINCT)]),
                 R=np.array([spd(rs, m, 0.5) for _ in range(DISTINCT)]), B=rs.randn(DISTINCT, n, NU))
        perr = 0.0
        for pt in (False, True):
            r = {k: [] for k in ("xp", "Pp", "xu", "Pu", "K", "S", "SI", "ll", "maha", "xs", "Ps")}
            for i in range(DISTINCT):
                F, Q, R, B = (d[k][i if pt else 0] for k in "FQRB")
                xp, Pp = ep.predict(d["x"][i], d["P"][i], F, Q, B, d["u"][i])
                xu, Pu, K, S, SI = ep.update(d["x"][i], d["P"][i], d["H"][i], d["y"][i], R)
                xs, Ps = ep.predict(xu, Pu, F, Q, B, d["u"][i])
                for k, v in zip(r, (xp, Pp, xu, Pu, K, S, SI, ep.loglik(d["y"][i], S), ep.maha(d["y"][i], SI), xs, Ps)):
                    r[k].append(v)
                LD = ekf_hp.LD
                hx, hP, *_ = ep.update(*(np.asarray(v, dtype=LD) for v in (d["x"][i], d["P"][i], d["H"][i], d["y"][i], R)), inv=ekf_hp.inv)
                hx, hP = ep.predict(hx, hP, *(np.asarray(v, dtype=LD) for v in (F, Q, B, d["u"][i])))
                perr = max(perr, em.err(xs[None], hx[None]), em.err(Ps[None], hP[None]))
            d[pt] = {k: np.array(v) for k, v in r.items()}
        d["tol"] = max(em.K_BAR * perr, 1e-12)
        _cases[dims] = d
    return _cases[dims]


def tile(a, N):
    return np.take(a, np.arange(N) % DISTINCT, axis=0)


def worst(a, b):
    """worst normwise relative error over the records (leading axis: tracks); scalars per track: each against max(|ref|, 1)"""
    a, b = np.asarray(a, dtype=float), np.asarray(b, dtype=float)
    assert a.shape == b.shape, (a.shape, b.shape)
    if a.ndim == 1:
        return float((np.abs(a - b) / np.maximum(np.abs(b), 1.0)).max())
    a2, b2 = a.reshape(len(a), -1), b.reshape(len(b), -1)
    scale = np.abs(b2).max(axis=1)
    scale[scale == 0] = 1.0
    return float((np.abs(a2 - b2).max(axis=1) / scale).max())


def desc(dims, N, layout, pt, nu=0, flags=0):
    return dict(n=dims[0], m=dims[1], nu=nu, model_mode=_abi.FK_MODEL_PER_TRACK if pt else _abi.FK_MODEL_SHARED, N=N, T=1,
                layout=E.LAYOUTS[layout], update_first=0, alpha_sq=1.0, flags=flags)


class Bank(object):
    """the operands of a case on the device, in `layout`; P may be overridden (the indefinite track)"""

    def __init__(self, dims, N, layout, pt, P=None):
        d = case(dims)
        n, m = dims
        self.d, self.dims, self.N, self.layout, self.pt = d, dims, N, layout, pt
        rec = lambda a: E.to_records(np.ascontiguousarray(tile(a, N)), layout, 0)          # noqa: E731
        self.x0 = rec(d["x"])
        self.P0 = rec(d["P"]) if P is None else E.to_records(np.ascontiguousarray(P), layout, 0)       # (P: all N tracks)
        self.H, self.y, self.u = rec(d["H"]), rec(d["y"]), rec(d["u"])
        self.F, self.Q, self.R, self.B = (rec(d[k]) if pt else E.dev(d[k][0]) for k in "FQRB")
        self.shapes = dict(x=(n,), P=(n, n), x_post=(n,), P_post=(n, n), K=(n, m), S=(m, m), SI=(m, m))

    def state(self):
        return self.x0.clone(), self.P0.clone()

    def outs(self, names):
        n, m = self.dims
        o = {}
        for k in names:
            if k in ("log_likelihood", "mahalanobis"):
                o[k] = torch.full((self.N,), np.nan, dtype=torch.float64, device="cuda")
            else:
                o[k] = E.alloc_records((), self.N, int(np.prod(self.shapes[k])), self.layout).fill_(float("nan"))
        return o

    def host(self, t, k):
        if k in ("log_likelihood", "mahalanobis", "status"):
            return t.cpu().numpy()
        return np.array(E.from_records(t, self.layout, 0, self.shapes[k]))

    def status(self):
        return torch.full((self.N,), -1, dtype=torch.int32, device="cuda")

    def predict(self):
        x, P, st = *self.state(), self.status()
        E.ekf_predict(desc(self.dims, self.N, self.layout, self.pt, nu=NU), self.F, self.Q, x, P, B=self.B, u=self.u, status=st)
        return dict(x=self.host(x, "x"), P=self.host(P, "P"), status=self.host(st, "status"))

    BY = ("K", "S", "SI", "log_likelihood", "mahalanobis")

    def update(self, mask=None, by=BY, status=True):
        x, P, st, o = *self.state(), self.status() if status else None, self.outs(by)
        E.ekf_update(desc(self.dims, self.N, self.layout, self.pt), self.H, self.R, self.y, x, P, mask=mask, status=st, **o)
        r = dict(x=self.host(x, "x"), P=self.host(P, "P"), **{k: self.host(v, k) for k, v in o.items()})
        if status:
            r["status"] = self.host(st, "status")
        return r

    def step(self, mask=None, by=BY, post=True):
        x, P, st = *self.state(), self.status()
        o = self.outs(by + (("x_post", "P_post") if post else ()))
        E.ekf_step(desc(self.dims, self.N, self.layout, self.pt, nu=NU), self.H, self.R, self.y, self.F, self.Q, x, P, mask=mask,
                   B=self.B, u=self.u, status=st, **o)
        return dict(x=self.host(x, "x"), P=self.host(P, "P"), status=self.host(st, "status"), **{k: self.host(v, k) for k, v in o.items()})

    def update_then_predict(self, mask=None):
        x, P, st, st2 = *self.state(), self.status(), self.status()
        E.ekf_update(desc(self.dims, self.N, self.layout, self.pt), self.H, self.R, self.y, x, P, mask=mask, status=st)
        post = dict(x_post=self.host(x, "x"), P_post=self.host(P, "P"))
        E.ekf_predict(desc(self.dims, self.N, self.layout, self.pt, nu=NU), self.F, self.Q, x, P, B=self.B, u=self.u, status=st2)
        return dict(x=self.host(x, "x"), P=self.host(P, "P"), status=self.host(st, "status") | self.host(st2, "status"), **post)


def same(a, b, keys=None):
    for k in (keys or a):
        assert np.array_equal(a[k], b[k], equal_nan=True), k


@pytest.mark.parametrize("pt", [False, True], ids=["shared", "per_track"])
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("dims", DIMS)
def test_entry_points_every_output_against_the_port(dims, layout, pt):
    d = case(dims)
    ref, tol = d[pt], d["tol"]
    for N in NS:
        b = Bank(dims, N, layout, pt)
        p, u, s = b.predict(), b.update(), b.step()
        got = dict(xp=p["x"], Pp=p["P"], xu=u["x"], Pu=u["P"], K=u["K"], S=u["S"], SI=u["SI"], ll=u["log_likelihood"],
                   maha=u["mahalanobis"], xs=s["x"], Ps=s["P"])
        for k, v in got.items():
            e = worst(v, tile(ref[k], N))
            print(dims, layout, "per_track" if pt else "shared", "N", N, k, "err %.2e tol %.2e" % (e, tol))
            assert e <= tol, (dims, N, k, e)
        assert not p["status"].any() and not u["status"].any() and not s["status"].any()
        # the step is the update followed by the predict, bit for bit, on every output and by-product
        same(s, b.update_then_predict(), ("x", "P", "x_post", "P_post", "status"))
        same(s, u, Bank.BY)
        assert np.array_equal(s["x_post"], u["x"]) and np.array_equal(s["P_post"], u["P"])
        # NULL by-products, NULL status, NULL posterior records: the same state
        same(u, b.update(by=(), status=False), ("x", "P"))
        same(s, b.step(by=(), post=False), ("x", "P"))
        # a mask with the first and the last track missing: their x and P stay, their by-products are not written,
        # the predict half of a step still runs for them; everybody else is untouched by the mask
        mk = np.ones(N, dtype=np.uint8)
        mk[0] = mk[-1] = 0
        on = mk != 0
        dm = torch.as_tensor(mk, device="cuda")
        um, sm = b.update(mask=dm), b.step(mask=dm)
        x0, P0 = b.host(b.x0, "x"), b.host(b.P0, "P")
        assert np.array_equal(um["x"][~on], x0[~on]) and np.array_equal(um["P"][~on], P0[~on])
        assert np.array_equal(sm["x_post"][~on], x0[~on]) and np.array_equal(sm["P_post"][~on], P0[~on])
        assert np.array_equal(sm["x"][~on], p["x"][~on]) and np.array_equal(sm["P"][~on], p["P"][~on])
        for k in Bank.BY:
            assert np.isnan(um[k][~on]).all() and np.isnan(sm[k][~on]).all(), k
        for k in um:
            assert np.array_equal(um[k][on], u[k][on]), k
        for k in sm:
            assert np.array_equal(sm[k][on], s[k][on]), k
        same(sm, b.update_then_predict(mask=dm), ("x", "P", "x_post", "P_post", "status"))


@pytest.mark.parametrize("pt", [False, True], ids=["shared", "per_track"])
@pytest.mark.parametrize("dims", DIMS)
def test_layouts_are_bit_identical(dims, pt):
    for N in NS:
        a, b = Bank(dims, N, "soa", pt), Bank(dims, N, "aos", pt)
        same(a.predict(), b.predict())
        same(a.update(), b.update())
        same(a.step(), b.step())


@pytest.mark.parametrize("pt", [False, True], ids=["shared", "per_track"])
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("dims", [(2, 1), (4, 2), (9, 4)])
def test_one_track_with_an_indefinite_s_is_flagged_alone(dims, layout, pt):
    """an input, not a fault: P of one track is negative definite, so S = H P H' + R has a negative pivot.  That track's status
    says FK_STATUS_NOT_PD; every other track is bit-identical to a run without it."""
    d = case(dims)
    for N, bad in ((65, 64), (BLOCK + 1, 100), (BLOCK + 1, BLOCK)):
        P = tile(d["P"], N).copy()
        P[bad] = -1e3 * P[bad]
        good = Bank(dims, N, layout, pt)
        ill = Bank(dims, N, layout, pt, P=np.ascontiguousarray(P))
        assert ill.N == N and ill.P0.numel() == good.P0.numel()
        others = np.arange(N) != bad
        for run in ("update", "step"):
            g, i = getattr(good, run)(), getattr(ill, run)()
            assert i["status"][bad] & _abi.FK_STATUS_NOT_PD and not i["status"][others].any() and not g["status"].any()
            for k in g:
                assert np.array_equal(g[k][others], i[k][others]), (run, k)


def test_scalar_r_attribute_flag():
    """FK_KF_FLAG_R_JOSEPH_DIAG, as for fk_kf_update_f64: R = r * ones, r on every element of S, r K K' in the Joseph form"""
    for dims in ((3, 2), (9, 4)):
        n, m = dims
        d = case(dims)
        for layout in LAYOUTS:
            b = Bank(dims, 65, layout, False)
            b.R = E.dev(np.full((m, m), 0.3))
            x, P, o = *b.state(), b.outs(("K", "S"))
            E.ekf_update(desc(dims, 65, layout, False, flags=_abi.FK_KF_FLAG_R_JOSEPH_DIAG), b.H, b.R, b.y, x, P, **o)
            ref = [ep.update(d["x"][i], d["P"][i], d["H"][i], d["y"][i], None, scalar_r=0.3) for i in range(65)]
            for k, j in (("x", 0), ("P", 1), ("K", 2), ("S", 3)):
                got = b.host(dict(x=x, P=P, **o)[k], k)
                assert worst(got, np.array([r[j] for r in ref])) <= d["tol"], (dims, layout, k)


# ---- the class ----------------------------------------------------------------------------------------------------------
def _bank(mode, dims, N, layout, per_track):
    n, m = dims
    rs = np.random.RandomState(17 * n + m)
    b = ExtendedKalmanFilter(n, m, n_tracks=N, layout=layout, vectorized=mode == "vec", device_callables=mode == "torch")
    A = rs.randn(N, n, n)
    b.x, b.P = rs.randn(N, n), A @ np.swapaxes(A, 1, 2) / n + np.eye(n)
    b.F = np.eye(n) + 0.05 * rs.randn(*((N,) if per_track else ()), n, n)
    b.Q = 0.01 * np.eye(n) * (1 + np.arange(N)[:, None, None] % 7 if per_track else 1)
    b.R = 0.2 * np.eye(m) * (1 + np.arange(N)[:, None, None] % 5 if per_track else 1)
    b.B = rs.randn(*((N,) if per_track else ()), n, NU)
    return b, rs.randn(4, N, m), 0.1 * rs.randn(4, N, NU)


def _callables(mode, m):
    if mode == "loop":
        return (lambda x: em.jac(x[:, 0], m)), (lambda x: em.hx(x[:, 0], m))
    return (lambda x: em.jac(x, m)), (lambda x: em.hx(x, m))


@pytest.mark.parametrize("per_track", [False, True], ids=["shared", "per_track"])
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("dims", [(2, 1), (4, 2), (9, 4)])
def test_batch_filter_is_the_step_loop_bit_for_bit_in_every_mode(dims, layout, per_track):
    """device callables: one predict, T - 1 fused steps, one update -- the bits of the loop of predict() / update(); and the
    per-track and the vectorised mode give those bits too (the callables are + and x only: the same bits in NumPy and on the
    device); every track against the port on its own model"""
    n, m = dims
    N, T = 65, 4
    res = {}
    for mode in ("torch", "vec", "loop"):
        b, zs, us = _bank(mode, dims, N, layout, per_track)
        jac, hx = _callables(mode, m)
        res[mode] = b.batch_filter(zs, jac, hx, us=us)
        if mode == "torch":
            b2, _, _ = _bank(mode, dims, N, layout, per_track)
            hist = [[], [], [], []]
            for t in range(T):
                b2.predict(us[t])
                hist[2].append(b2.x.copy())
                hist[3].append(b2.P.copy())
                b2.update(zs[t], jac, hx)
                hist[0].append(b2.x.copy())
                hist[1].append(b2.P.copy())
            for a, c in zip(res[mode], hist):
                assert np.array_equal(np.asarray(a), np.asarray(c))
            for a in ("x", "P", "K", "S", "SI", "y", "x_prior", "P_prior", "x_post", "P_post", "log_likelihood", "mahalanobis"):
                assert np.array_equal(np.asarray(getattr(b, a)), np.asarray(getattr(b2, a))), a
            dev = b2.batch_filter(torch.as_tensor(zs, device="cuda"), jac, hx, us=us, device_outputs=True)
            assert all(t.is_cuda for t in dev) and tuple(dev[1].shape) == ((T, N, n * n) if layout == "aos" else (T, n * n, N))
    for mode in ("vec", "loop"):
        for a, c in zip(res["torch"], res[mode]):
            assert np.array_equal(a, c), mode
    b, zs, us = _bank("loop", dims, N, layout, per_track)
    tol = 1e-12          # well-conditioned models, four steps: the floor of the project's bar (see the head of the file)
    for i in (0, 1, 63, 64):
        g = ep.Port(n, m)
        g.x, g.P = b.x[i].reshape(n, 1).copy(), b.P[i].copy()
        g.F, g.Q, g.R, g.B = (np.asarray(M)[i] if np.ndim(M) == 3 else M for M in (b.F, b.Q, b.R, b.B))
        for t in range(T):
            g.predict(us[t, i].reshape(NU, 1))
            assert worst(res["torch"][2][t, i][None], g.x[:, 0][None]) < tol and worst(res["torch"][3][t, i][None], g.P[None]) < tol
            g.update(zs[t, i].reshape(m, 1), lambda x: em.jac(x[:, 0], m), lambda x: em.hx(x[:, 0], m).reshape(m, 1))
            assert worst(res["torch"][0][t, i][None], g.x[:, 0][None]) < tol and worst(res["torch"][1][t, i][None], g.P[None]) < tol


@pytest.mark.parametrize("case_name", sorted(em.CASES))
def test_golden_models_through_the_class(case_name):
    """the reference's attributes after every call of the golden sequences.  Tolerance 1e-11: twelve calls, each adding at most
    n eps cond(S) of relative error (the range-bearing S has condition 1e3: variances 0.09 and 4e-4), 12 * 4 * 1.1e-16 * 1e3 = 5e-12."""
    G = np.load(__import__("os").path.join(__import__("os").path.dirname(__file__), "golden", "ekf.npz"))
    f, d = em.make(ExtendedKalmanFilter, case_name)
    for k in range(len(em.OPS)):
        em.run_op(f, case_name, d, k)
        for a in em.ATTRS:
            ref, mine = G[f"{case_name}_k{k}_{a}"], np.array(getattr(f, a), dtype=float)
            assert mine.shape == ref.shape, (case_name, k, a, mine.shape, ref.shape)
            e = float(np.abs(mine - ref).max() / max(np.abs(ref).max(), 1e-300)) if ref.size else 0.0
            assert e <= 1e-11, (case_name, k, a, e)


def test_bank_mask_and_predict_update():
    dims, N = (4, 2), 65
    n, m = dims
    b, zs, us = _bank("vec", dims, N, "aos", False)
    jac, hx = _callables("vec", m)
    b.predict()
    b.update(zs[0], jac, hx)
    keep = {a: np.copy(getattr(b, a)) for a in ("x", "P", "K", "S", "SI", "y", "log_likelihood", "mahalanobis")}
    b2, _, _ = _bank("vec", dims, N, "aos", False)
    b2.predict()
    b2.update(zs[0], jac, hx)
    mask = np.ones(N, dtype=bool)
    mask[0] = mask[-1] = False
    b.update(zs[1], jac, hx, mask=mask)
    b2.update(zs[1], jac, hx)
    for a in keep:
        got, full = np.asarray(getattr(b, a)), np.asarray(getattr(b2, a))
        assert np.array_equal(got[~mask], keep[a][~mask]) and np.array_equal(got[mask], full[mask]), a
    x_pre, P_pre = b.x.copy(), b.P.copy()
    b.predict_update(zs[2], jac, hx, u=us[2])
    assert np.array_equal(b.x_prior, x_pre)
    for i in (0, 31, 64):
        g = ep.Port(n, m)
        g.x, g.P, g.F, g.Q, g.R, g.B = x_pre[i].reshape(n, 1), P_pre[i], b.F, b.Q, b.R, b.B
        g.predict_update(zs[2, i].reshape(m, 1), lambda x: em.jac(x[:, 0], m), lambda x: em.hx(x[:, 0], m).reshape(m, 1),
                         u=us[2, i].reshape(NU, 1))
        assert worst(b.x[i][None], g.x[:, 0][None]) < 1e-12 and worst(b.P[i][None], g.P[None]) < 1e-12
        assert worst(b.K[i][None], g.K[None]) < 1e-12 and abs(b.log_likelihood[i] - g.log_likelihood) < 1e-11 * max(1, abs(g.log_likelihood))
