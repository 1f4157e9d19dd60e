"""CPU stand-in for fk_srkf_batch_f64 / fk_srkf_predict_f64 / fk_srkf_update_f64 (include/filterhip.h), for HOST-LOGIC tests of
filterpy_amd.kalman.SquareRootKalmanFilter / SquareRootKalmanFilterBank: it reads its operands exactly as the ABI lays them out
(records in `layout`, lower-triangular factors whose upper triangles are not read, the uint8 mask, update_first) and computes
with tests/srkf_port.py, so the Python layer -- shapes, attributes, quirks, masking -- can be held against the live reference
on the CPU."""
import numpy as np
import torch

from fake_kf_engine import get, put, CPU
import srkf_port

NOT_PD = 1


def _not_pd(S12, m):
    d = np.abs(np.diag(S12))
    return bool(np.any(~(d > m * np.finfo(float).eps * d.max())))


def install(monkeypatch):
    from filterpy_amd import _engine as E
    codes = {v: k for k, v in E.LAYOUTS.items()}
    calls = []
    monkeypatch.setattr(E, "require_gpu", lambda: CPU)
    real_dev = E.dev
    monkeypatch.setattr(E, "dev", lambda a, device=None: real_dev(a, device).clone())
    tril = lambda A, k: np.tril(A.detach().numpy().reshape(k, k))          # noqa: E731

    def check(desc):
        assert desc["model_mode"] == 0 and desc["alpha_sq"] == 1.0 and desc["flags"] == 0

    def srkf_batch(desc, F, Q12, H, R12, z, x, P12, *, B=None, u=None, mask=None, means=None, covs=None, means_p=None,
                   covs_p=None, y=None, K=None, S12=None, SI12=None, status=None):
        check(desc)
        n, m, nu, N, T, L = desc["n"], desc["m"], desc["nu"], desc["N"], desc["T"], codes[desc["layout"]]
        calls.append(("batch", N, T))
        Fm, Hm = F.detach().numpy().reshape(n, n), H.detach().numpy().reshape(m, n)
        Qm, Rm = tril(Q12, n), tril(R12, m)
        Bm = B.detach().numpy().reshape(n, nu) if nu else None
        zs, us = get(z, L, 1, (m,)), (get(u, L, 1, (nu,)) if nu else None)
        mk = None if mask is None else mask.detach().numpy().reshape(T, N) != 0
        xo, Lo = get(x, L, 0, (n,)), np.tril(get(P12, L, 0, (n, n)))
        out = [np.zeros((T, N, n)), np.zeros((T, N, n, n)), np.zeros((T, N, n)), np.zeros((T, N, n, n))]
        st = np.zeros(N, dtype=np.int32)
        for i in range(N):
            r = srkf_port.batch(xo[i], Lo[i], zs[:, i], Fm, Qm, Hm, Rm, Bm, None if us is None else us[:, i],
                                None if mk is None else mk[:, i], bool(desc["update_first"]))
            for o, v in zip(out, r[:4]):
                o[:, i] = v
            xo[i], Lo[i] = (r[0][-1], r[1][-1]) if not desc["update_first"] else (r[2][-1], r[3][-1])
            if r[4] is not None and _not_pd(r[4][4], m):
                st[i] |= NOT_PD
        for rec, v in zip((means, covs, means_p, covs_p), out):
            put(rec, L, 1, v)
        put(x, L, 0, xo)
        put(P12, L, 0, Lo)
        if status is not None:
            status.copy_(torch.as_tensor(st))

    def srkf_predict(desc, F, Q12, x, P12, *, B=None, u=None, status=None):
        check(desc)
        n, nu, N, L = desc["n"], desc["nu"], desc["N"], codes[desc["layout"]]
        calls.append(("predict", N, 1))
        Fm, Qm = F.detach().numpy().reshape(n, n), tril(Q12, n)
        Bm = B.detach().numpy().reshape(n, nu) if nu else None
        us = get(u, L, 0, (nu,)) if nu else None
        xo, Lo = get(x, L, 0, (n,)), np.tril(get(P12, L, 0, (n, n)))
        for i in range(N):
            xo[i], Lo[i] = srkf_port.predict(xo[i], Lo[i], Fm, Qm, Bm, None if us is None else us[i])
        put(x, L, 0, xo)
        put(P12, L, 0, Lo)
        if status is not None:
            status.zero_()

    def srkf_update(desc, H, R12, z, x, P12, *, mask=None, y=None, K=None, S12=None, SI12=None, status=None):
        check(desc)
        n, m, N, L = desc["n"], desc["m"], desc["N"], codes[desc["layout"]]
        calls.append(("update", N, 1))
        Hm, Rm = H.detach().numpy().reshape(m, n), tril(R12, m)
        zs = get(z, L, 0, (m,))
        mk = None if mask is None else mask.detach().numpy().reshape(N) != 0
        xo, Lo = get(x, L, 0, (n,)), np.tril(get(P12, L, 0, (n, n)))
        outs = [get(o, L, 0, s) if o is not None else None for o, s in ((y, (m,)), (K, (n, m)), (S12, (m, m)), (SI12, (m, m)))]
        st = np.zeros(N, dtype=np.int32)
        for i in range(N):
            if mk is not None and not mk[i]:
                continue
            xo[i], Lo[i], *rest = srkf_port.update(xo[i], Lo[i], zs[i], Hm, Rm)
            for o, v in zip(outs, rest):
                if o is not None:
                    o[i] = v
            if _not_pd(rest[2], m):
                st[i] |= NOT_PD
        put(x, L, 0, xo)
        put(P12, L, 0, Lo)
        for rec, v in zip((y, K, S12, SI12), outs):
            if rec is not None:
                put(rec, L, 0, v)
        if status is not None:
            status.copy_(torch.as_tensor(st))

    monkeypatch.setattr(E, "srkf_batch", srkf_batch)
    monkeypatch.setattr(E, "srkf_predict", srkf_predict)
    monkeypatch.setattr(E, "srkf_update", srkf_update)
    return calls
