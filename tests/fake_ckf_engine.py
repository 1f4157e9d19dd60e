"""CPU stand-in for the cubature filter's entry points (fk_ckf_sigma_points_f64, fk_ckf_transform_f64, fk_ckf_update_f64,
fk_ckf_linear_batch_f64 / _predict_f64 / _update_f64; include/filterhip.h), for HOST-LOGIC tests of
filterpy_amd.kalman.CubatureKalmanFilter: it reads its operands exactly as the ABI lays them out (records in `layout`, the uint8
mask, the points record [n + n*n] of the matrix model) and computes with tests/ckf_port.py, so the Python layer -- shapes,
attributes, modes, quirks -- can be held against the goldens of the live reference on the CPU.  Status: NOT_PD where numpy's
cholesky refuses P, or S has a non-positive pivot."""
import numpy as np
import torch

from fake_kf_engine import get, put, CPU
import ckf_port

NOT_PD = 1


def _pd(A):
    if not np.isfinite(A).all():
        return False
    try:
        np.linalg.cholesky(A)
        return True
    except np.linalg.LinAlgError:
        return False


def points_to_sigmas(pts, n):
    """(N, n + n*n) -> (N, 2n, n): c +- sqrt(n) E[k]"""
    c, Eh = pts[:, None, :n], pts[:, n:].reshape(-1, n, n) * np.sqrt(n)
    return np.concatenate([c + Eh, c - Eh], axis=1)


def install(monkeypatch):
    from filterpy_amd import _engine as E
    codes = {v: k for k, v in E.LAYOUTS.items()}
    calls = []
    monkeypatch.setattr(E, "require_gpu", lambda: CPU)
    real_dev = E.dev
    monkeypatch.setattr(E, "dev", lambda a, device=None: real_dev(a, device).clone())

    def mat(t, r, c):
        return t.detach().numpy().reshape(r, c)

    def set_status(status, st):
        if status is not None:
            status.copy_(torch.as_tensor(st))

    def ckf_sigma_points(n, N, layout, x, P, sigmas, status=None):
        calls.append(("points", N))
        xs, Ps = get(x, layout, 0, (n,)), get(P, layout, 0, (n, n))
        out, st = np.full((N, 2 * n, n), np.nan), np.zeros(N, dtype=np.int32)
        for i in range(N):
            if _pd(Ps[i]):
                out[i] = ckf_port.spherical_radial_sigmas(xs[i], Ps[i])
            else:
                st[i] = NOT_PD
        put(sigmas, layout, 0, out)
        set_status(status, st)

    def ckf_transform(d, k, N, layout, sigmas, noise, x_out, P_out):
        calls.append(("transform", N))
        s = get(sigmas, layout, 0, (k, d))
        Q = np.zeros((d, d)) if noise is None else mat(noise, d, d)
        res = [ckf_port.ckf_transform(s[i], Q) for i in range(N)]
        put(x_out, layout, 0, np.array([r[0][:, 0] for r in res]))
        put(P_out, layout, 0, np.array([r[1] for r in res]))

    def one_update(f, sf, sh, R, z, x, P, z_is_y):
        """the port's update() lines on given points -> x, P, zp, S, SI, K, y, status"""
        f.sigmas_f, f.x, f.P = sf, x.reshape(-1, 1), P
        hs = iter(sh)
        f.hx = lambda s: next(hs)
        if z_is_y:
            f.residual_z = lambda a, b: a
        f.update(z.reshape(-1, 1), R=R)
        zp = sh.mean(axis=0)
        return f.x[:, 0], f.P, zp, f.S, f.SI, f.K, f.y[:, 0], 0 if _pd(f.S) else NOT_PD

    def cross(sf, sh, x):
        return ckf_port.outer_product_sum(sf - x, sh - sh.mean(axis=0)) / len(sf)

    def ckf_update(n, m, N, layout, sigmas_f, sigmas_h, R, z, x, P, *, zp=None, S=None, SI=None, Pxz=None, K=None, y=None,
                   status=None):
        calls.append(("update", N))
        sf, sh = get(sigmas_f, layout, 0, (2 * n, n)), get(sigmas_h, layout, 0, (2 * n, m))
        zs, xs, Ps = get(z, layout, 0, (m,)), get(x, layout, 0, (n,)), get(P, layout, 0, (n, n))
        Rm = mat(R, m, m)
        st = np.zeros(N, dtype=np.int32)
        outs = {k: [] for k in ("zp", "S", "SI", "K", "y", "Pxz")}
        for i in range(N):
            f = ckf_port.Port(n, m, 1.0, None, None)
            outs["Pxz"].append(cross(sf[i], sh[i], xs[i]))
            xs[i], Ps[i], zpi, Si, SIi, Ki, yi, st[i] = one_update(f, sf[i], sh[i], Rm, zs[i], xs[i], Ps[i], zp is None)
            for k, v in zip(("zp", "S", "SI", "K", "y"), (zpi, Si, SIi, Ki, yi)):
                outs[k].append(v)
        put(x, layout, 0, xs)
        put(P, layout, 0, Ps)
        for k, rec in (("zp", zp), ("S", S), ("SI", SI), ("K", K), ("y", y), ("Pxz", Pxz)):
            if rec is not None:
                put(rec, layout, 0, np.array(outs[k]))
        set_status(status, st)

    def check(desc):
        assert desc["model_mode"] == 0 and desc["alpha_sq"] == 1.0 and desc["flags"] == 0 and desc["nu"] == 0
        assert desc["update_first"] == 0

    def lin_predict(x, P, Fm, Qm):
        """-> x, P, points record, status"""
        n = len(x)
        if not _pd(P):
            return np.full(n, np.nan), np.full((n, n), np.nan), np.full(n + n * n, np.nan), NOT_PD
        U = np.linalg.cholesky(P).T
        pts = np.concatenate([Fm @ x, (U @ Fm.T).ravel()])          # E[k] = F U[k]
        xn, Pn = ckf_port.ckf_transform(points_to_sigmas(pts[None], n)[0], Qm)
        return xn[:, 0], Pn, pts, 0

    def lin_update(x, P, pts, Hm, Rm, z):
        n, m = len(x), len(z)
        sf = points_to_sigmas(pts[None], n)[0]
        f = ckf_port.Port(n, m, 1.0, None, None)
        return one_update(f, sf, sf @ Hm.T, Rm, z, x, P, False)

    def ckf_linear_predict(desc, F, Q, x, P, points, *, status=None):
        check(desc)
        n, N, L = desc["n"], desc["N"], codes[desc["layout"]]
        calls.append(("lin_predict", N))
        Fm, Qm = mat(F, n, n), mat(Q, n, n)
        xs, Ps, pts = get(x, L, 0, (n,)), get(P, L, 0, (n, n)), get(points, L, 0, (n + n * n,))
        st = np.zeros(N, dtype=np.int32)
        for i in range(N):
            xs[i], Ps[i], pts[i], st[i] = lin_predict(xs[i], Ps[i], Fm, Qm)
        put(x, L, 0, xs)
        put(P, L, 0, Ps)
        put(points, L, 0, pts)
        set_status(status, st)

    def ckf_linear_update(desc, H, R, z, x, P, points, *, mask=None, y=None, K=None, S=None, SI=None, status=None):
        check(desc)
        n, m, N, L = desc["n"], desc["m"], desc["N"], codes[desc["layout"]]
        calls.append(("lin_update", N))
        Hm, Rm = mat(H, m, n), mat(R, m, m)
        zs, xs, Ps, pts = get(z, L, 0, (m,)), get(x, L, 0, (n,)), get(P, L, 0, (n, n)), get(points, L, 0, (n + n * n,))
        mk = None if mask is None else mask.detach().numpy().reshape(N) != 0
        outs = [get(o, L, 0, s) if o is not None else None for o, s in ((S, (m, m)), (SI, (m, m)), (K, (n, m)), (y, (m,)))]
        st = np.zeros(N, dtype=np.int32)
        for i in range(N):
            if mk is not None and not mk[i]:
                continue
            xs[i], Ps[i], _, *rest, st[i] = lin_update(xs[i], Ps[i], pts[i], Hm, Rm, zs[i])
            for o, v in zip(outs, rest):
                if o is not None:
                    o[i] = v
        put(x, L, 0, xs)
        put(P, L, 0, Ps)
        for rec, v in zip((S, SI, K, y), outs):
            if rec is not None:
                put(rec, L, 0, v)
        set_status(status, st)

    def ckf_linear_batch(desc, F, Q, H, R, z, x, P, points, *, mask=None, means=None, covs=None, means_p=None, covs_p=None,
                         status=None):
        check(desc)
        n, m, N, T, L = desc["n"], desc["m"], desc["N"], desc["T"], codes[desc["layout"]]
        calls.append(("lin_batch", N, T))
        Fm, Qm, Hm, Rm = mat(F, n, n), mat(Q, n, n), mat(H, m, n), mat(R, m, m)
        zs = get(z, L, 1, (m,))
        mk = None if mask is None else mask.detach().numpy().reshape(T, N) != 0
        xs, Ps, pts = get(x, L, 0, (n,)), get(P, L, 0, (n, n)), get(points, L, 0, (n + n * n,))
        out = [np.zeros((T, N, n)), np.zeros((T, N, n, n)), np.zeros((T, N, n)), np.zeros((T, N, n, n))]
        st = np.zeros(N, dtype=np.int32)
        for i in range(N):
            for t in range(T):
                xs[i], Ps[i], pts[i], s = lin_predict(xs[i], Ps[i], Fm, Qm)
                st[i] |= s
                out[2][t, i], out[3][t, i] = xs[i], Ps[i]
                if not s and (mk is None or mk[t, i]):
                    xs[i], Ps[i], *_, s = lin_update(xs[i], Ps[i], pts[i], Hm, Rm, zs[t, i])
                    st[i] |= s
                out[0][t, i], out[1][t, i] = xs[i], Ps[i]
        for rec, v in zip((means, covs, means_p, covs_p), out):
            put(rec, L, 1, v)
        put(x, L, 0, xs)
        put(P, L, 0, Ps)
        put(points, L, 0, pts)
        set_status(status, st)

    def ut_linear_map(n_in, n_out, k, N, layout, M, sig_in, sig_out):
        put(sig_out, layout, 0, get(sig_in, layout, 0, (k, n_in)) @ mat(M, n_out, n_in).T)

    for name, fn in (("ckf_sigma_points", ckf_sigma_points), ("ckf_transform", ckf_transform), ("ckf_update", ckf_update),
                     ("ckf_linear_predict", ckf_linear_predict), ("ckf_linear_update", ckf_linear_update),
                     ("ckf_linear_batch", ckf_linear_batch), ("ut_linear_map", ut_linear_map)):
        monkeypatch.setattr(E, name, fn)
    return calls
