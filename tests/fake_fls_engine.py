"""CPU stand-in for fk_fls_batch_f64 (include/filterhip.h), for HOST-LOGIC tests of filterpy_amd.kalman.FixedLagSmoother /
FixedLagSmootherBank: it reads its operands exactly as the ABI lays them out (records in `layout`, the W pending rows at the head
of xs, FK_KF_FLAG_R_JOSEPH_DIAG) and computes with the reference's arithmetic (tests/fls_port.py's step), so the Python layer --
shapes, the xSmooth bookkeeping, the pending window, attribute updates -- can be held against the live reference on the CPU."""
import numpy as np
import torch

from fake_kf_engine import get, put, CPU
from fls_port import _step, _lag_update

FLAG_R_JOSEPH_DIAG = 1
NOT_PD = 1


def install(monkeypatch):
    from filterpy_amd import _engine as E
    codes = {v: k for k, v in E.LAYOUTS.items()}
    calls = []
    monkeypatch.setattr(E, "require_gpu", lambda: CPU)
    real_dev = E.dev
    monkeypatch.setattr(E, "dev", lambda a, device=None: real_dev(a, device).clone())

    def fls_batch(desc, lag, k0, F, Q, H, R, z, x, P, xs, xhat, *, B=None, u=None, y=None, S=None, status=None):
        n, m, nu, N, T, L = desc["n"], desc["m"], desc["nu"], desc["N"], desc["T"], codes[desc["layout"]]
        calls.append((lag, k0, T))
        assert desc["model_mode"] == 0 and desc["update_first"] == 0 and desc["alpha_sq"] == 1.0
        rj = bool(desc.get("flags", 0) & FLAG_R_JOSEPH_DIAG)
        Fm, Qm, Hm, Rm = (M.detach().numpy().reshape(s) for M, s in ((F, (n, n)), (Q, (n, n)), (H, (m, n)), (R, (m, m))))
        Bm = B.detach().numpy().reshape(n, nu) if nu else None
        zs = get(z, L, 1, (m,))
        us = get(u, L, 1, (nu,)) if nu else None
        Lf = max(lag, 1)
        W = min(Lf - 1, k0)
        rows_all = get(xs, L, 1, (n,))
        xo, Po = get(x, L, 0, (n,)), get(P, L, 0, (n, n))
        xh = np.zeros((T, N, n))
        yo, So = np.zeros((N, m)), np.zeros((N, m, m))
        st = np.zeros(N, dtype=np.int32)
        for i in range(N):
            xi, Pi = xo[i].copy(), Po[i].copy()
            rows = {k0 - W + r: rows_all[r, i].copy() for r in range(W)}
            for t in range(T):
                k = k0 + t
                Rj = Rm
                x_pre, xi, Pi_new, yy, SS, SI, K = _step(xi, Pi, zs[t, i], Fm, Qm, Hm, Rm, Bm,
                                                         None if us is None else us[t, i], np.eye(n))
                if rj:        # scalar R attribute: S gets r on every element, the Joseph term r K K'
                    Pp = Fm @ Pi @ Fm.T + Qm
                    I_KH = np.eye(n) - K @ Hm
                    Pi_new = (I_KH @ Pp) @ I_KH.T + (K @ np.diag(np.diag(Rj))) @ K.T
                if np.any(np.linalg.eigvalsh(SS) <= 0):
                    st[i] |= NOT_PD
                Pi = Pi_new
                xh[t, i] = xi
                rows[k] = x_pre.copy()
                if k >= lag:
                    _lag_update(rows, k, lag, Pi, Hm, SI, K, Fm, yy)
                else:
                    rows[k] = xi.copy()
            xo[i], Po[i] = xi, Pi
            yo[i], So[i] = yy, SS
            for r in range(W + T):
                rows_all[r, i] = rows[k0 - W + r]
        put(xs, L, 1, rows_all)
        put(xhat, L, 1, xh)
        put(x, L, 0, xo)
        put(P, L, 0, Po)
        put(y, L, 0, yo)
        put(S, L, 0, So)
        if status is not None:
            status.copy_(torch.as_tensor(st))

    monkeypatch.setattr(E, "fls_batch", fls_batch)
    return calls
