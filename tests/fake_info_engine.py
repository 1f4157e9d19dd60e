"""CPU stand-in for fk_info_batch_f64 / fk_info_predict_f64 / fk_info_update_f64 (include/filterhip.h), for HOST-LOGIC tests of
filterpy_amd.kalman.InformationFilter / InformationFilterBank: it reads its operands exactly as the ABI lays them out (records
in `layout`, the uint8 mask, update_first) and computes with tests/info_port.py, so the Python layer -- shapes, attributes,
quirks, masking -- can be held against the goldens of the live reference on the CPU.  The status follows the ABI's rule: a
pivot of the L D L' of a matrix the step inverts at or below n eps max|diag|."""
import numpy as np
import torch

from fake_kf_engine import get, put, CPU
import info_port

NOT_PD = 1


def _singular(A):
    """a pivot of A's L D L' (lower triangle) at or below n eps max|diag A|"""
    n = A.shape[0]
    cut = n * np.finfo(float).eps * np.abs(np.diag(A)).max()
    L, d = np.eye(n), np.zeros(n)
    with np.errstate(all="ignore"):
        for j in range(n):
            d[j] = A[j, j] - (L[j, :j] ** 2) @ d[:j]
            if not d[j] > cut:
                return True
            for i in range(j + 1, n):
                L[i, j] = (A[i, j] - (L[i, :j] * L[j, :j]) @ d[:j]) / d[j]
    return False


def install(monkeypatch):
    from filterpy_amd import _engine as E
    codes = {v: k for k, v in E.LAYOUTS.items()}
    calls = []
    monkeypatch.setattr(E, "require_gpu", lambda: CPU)
    real_dev = E.dev
    monkeypatch.setattr(E, "dev", lambda a, device=None: real_dev(a, device).clone())

    def check(desc):
        assert desc["model_mode"] == 0 and desc["alpha_sq"] == 1.0 and desc["flags"] == 0

    def predict_one(x, Pi, Fm, Qm, Bm, u):
        """-> x, P_inv, status"""
        if _singular(Pi):
            return np.full_like(x, np.nan), np.full_like(Pi, np.nan), NOT_PD
        P = np.linalg.inv(Pi)
        bad = _singular(Fm @ P @ Fm.T + Qm)
        xn, Pn = info_port.predict(x, Pi, Fm, Qm, Bm, u)
        return xn, Pn, NOT_PD if bad else 0

    def info_batch(desc, F, Q, H, Rinv, z, x, Pinv, *, B=None, u=None, mask=None, means=None, covs=None, means_p=None,
                   covs_p=None, status=None):
        check(desc)
        n, m, nu, N, T, L = desc["n"], desc["m"], desc["nu"], desc["N"], desc["T"], codes[desc["layout"]]
        uf = bool(desc["update_first"])
        calls.append(("batch", N, T))
        Fm, Hm = F.detach().numpy().reshape(n, n), H.detach().numpy().reshape(m, n)
        Qm, Rm = Q.detach().numpy().reshape(n, n), Rinv.detach().numpy().reshape(m, m)
        Bm = B.detach().numpy().reshape(n, nu) if nu else None
        zs, us = get(z, L, 1, (m,)), (get(u, L, 1, (nu,)) if nu else None)
        mk = None if mask is None else mask.detach().numpy().reshape(T, N) != 0
        xo, Po = get(x, L, 0, (n,)), get(Pinv, L, 0, (n, n))
        out = [np.zeros((T, N, n)), np.zeros((T, N, n, n)), np.zeros((T, N, n)), np.zeros((T, N, n, n))]
        st = np.zeros(N, dtype=np.int32)
        for i in range(N):
            xi, Pi = xo[i], Po[i]
            for t in range(T):
                if not uf:
                    xi, Pi, s = predict_one(xi, Pi, Fm, Qm, Bm, None if us is None else us[t, i])
                    st[i] |= s
                    out[2][t, i], out[3][t, i] = xi, Pi
                if mk is None or mk[t, i]:
                    xi, Pi = info_port.update(xi, Pi, zs[t, i], Hm, Rm)[:2]
                    st[i] |= NOT_PD if _singular(Pi) else 0
                out[0][t, i], out[1][t, i] = xi, Pi
                if uf:
                    xi, Pi, s = predict_one(xi, Pi, Fm, Qm, Bm, None if us is None else us[t, i])
                    st[i] |= s
                    out[2][t, i], out[3][t, i] = xi, Pi
            xo[i], Po[i] = xi, Pi
        for rec, v in zip((means, covs, means_p, covs_p), out):
            put(rec, L, 1, v)
        put(x, L, 0, xo)
        put(Pinv, L, 0, Po)
        if status is not None:
            status.copy_(torch.as_tensor(st))

    def info_predict(desc, F, Q, x, Pinv, *, B=None, u=None, status=None):
        check(desc)
        n, nu, N, L = desc["n"], desc["nu"], desc["N"], codes[desc["layout"]]
        calls.append(("predict", N, 1))
        Fm, Qm = F.detach().numpy().reshape(n, n), Q.detach().numpy().reshape(n, n)
        Bm = B.detach().numpy().reshape(n, nu) if nu else None
        us = get(u, L, 0, (nu,)) if nu else None
        xo, Po = get(x, L, 0, (n,)), get(Pinv, L, 0, (n, n))
        st = np.zeros(N, dtype=np.int32)
        for i in range(N):
            xo[i], Po[i], st[i] = predict_one(xo[i], Po[i], Fm, Qm, Bm, None if us is None else us[i])
        put(x, L, 0, xo)
        put(Pinv, L, 0, Po)
        if status is not None:
            status.copy_(torch.as_tensor(st))

    def info_update(desc, H, Rinv, z, x, Pinv, *, mask=None, y=None, K=None, status=None):
        check(desc)
        n, m, N, L = desc["n"], desc["m"], desc["N"], codes[desc["layout"]]
        calls.append(("update", N, 1))
        Hm, Rm = H.detach().numpy().reshape(m, n), Rinv.detach().numpy().reshape(m, m)
        zs = get(z, L, 0, (m,))
        mk = None if mask is None else mask.detach().numpy().reshape(N) != 0
        xo, Po = get(x, L, 0, (n,)), get(Pinv, L, 0, (n, n))
        outs = [get(o, L, 0, s) if o is not None else None for o, s in ((y, (m,)), (K, (n, m)))]
        st = np.zeros(N, dtype=np.int32)
        for i in range(N):
            if mk is not None and not mk[i]:
                continue
            if _singular(Po[i] + Hm.T @ Rm @ Hm):
                st[i] |= NOT_PD
                continue
            xo[i], Po[i], *rest = info_port.update(xo[i], Po[i], zs[i], Hm, Rm)
            for o, v in zip(outs, rest):
                if o is not None:
                    o[i] = v
        put(x, L, 0, xo)
        put(Pinv, L, 0, Po)
        for rec, v in zip((y, K), outs):
            if rec is not None:
                put(rec, L, 0, v)
        if status is not None:
            status.copy_(torch.as_tensor(st))

    monkeypatch.setattr(E, "info_batch", info_batch)
    monkeypatch.setattr(E, "info_predict", info_predict)
    monkeypatch.setattr(E, "info_update", info_update)
    return calls
