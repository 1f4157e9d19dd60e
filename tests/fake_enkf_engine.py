"""CPU stand-in for fk_enkf_workspace_bytes / fk_enkf_predict_f64 / fk_enkf_update_f64 (include/filterhip.h), for HOST-LOGIC
tests of filterpy_amd.kalman.EnsembleKalmanFilter: it reads its operands exactly as the ABI lays them out (records in
`layout`, the draws or standard normals with a factor, H or sigmas_h) and computes with tests/enkf_port.py, so the Python layer
-- call sites of the draws, shapes, attributes, quirks -- can be held against the goldens of the live reference on the CPU.
The status follows the ABI's rule: a pivot of the L D L' of S at or below m eps max|diag S|."""
import numpy as np
import torch

from fake_kf_engine import get, put, CPU
from fake_info_engine import _singular, NOT_PD
import enkf_port


def install(monkeypatch):
    from filterpy_amd import _engine as E
    codes = {v: k for k, v in E.LAYOUTS.items()}
    calls = []
    monkeypatch.setattr(E, "require_gpu", lambda: CPU)
    real_dev = E.dev
    monkeypatch.setattr(E, "dev", lambda a, device=None: real_dev(a, device).clone())

    def check(desc, workspace, workspace_bytes):
        assert desc["model_mode"] == 0 and desc["alpha_sq"] == 1.0 and desc["flags"] == 0 and desc["N"] >= 2
        need = workspace_bytes_fn(desc["n"], desc["m"], desc["N"])
        assert workspace.dtype == torch.uint8 and workspace.numel() >= need
        assert workspace_bytes is None or workspace_bytes >= need

    def workspace_bytes_fn(n, m, N):
        return 8 * (152 + 188 * max(1, -(-N // 2048)))

    def draws(noise, factor, L, d):
        w = get(noise, L, 0, (d,))
        return w if factor is None else w @ factor.detach().numpy().reshape(d, d)

    def enkf_predict(desc, noise, sigmas, x, P, workspace, *, F=None, factor=None, workspace_bytes=None, status=None):
        check(desc, workspace, workspace_bytes)
        n, L = desc["n"], codes[desc["layout"]]
        calls.append(("predict", F is not None, factor is not None))
        Fm = None if F is None else F.detach().numpy().reshape(n, n)
        sig, xn, Pn = enkf_port.predict(get(sigmas, L, 0, (n,)), draws(noise, factor, L, n), Fm)
        put(sigmas, L, 0, sig)
        x.copy_(torch.as_tensor(xn))
        P.copy_(torch.as_tensor(Pn))
        if status is not None:
            status.zero_()

    def enkf_update(desc, R, z, noise, sigmas, x, P, workspace, *, H=None, sigmas_h=None, factor=None, S=None, SI=None, K=None,
                    workspace_bytes=None, status=None):
        check(desc, workspace, workspace_bytes)
        assert (H is None) != (sigmas_h is None)
        n, m, L = desc["n"], desc["m"], codes[desc["layout"]]
        calls.append(("update", H is not None, factor is not None))
        Hm = None if H is None else H.detach().numpy().reshape(m, n)
        sh = None if sigmas_h is None else get(sigmas_h, L, 0, (m,))
        Rm = R.detach().numpy().reshape(m, m)
        with np.errstate(all="ignore"):
            sig, xn, Pn, Kn, Sn, SIn = enkf_port.update(get(sigmas, L, 0, (n,)), x.detach().numpy().copy(), P.detach().numpy().copy(),
                                                        z.detach().numpy().reshape(m), Rm, draws(noise, factor, L, m), Hm, sh) \
                if not _singular_S(get(sigmas, L, 0, (n,)), Hm, sh, Rm) else (None,) * 6
        if sig is None:
            status.fill_(NOT_PD)
            return
        put(sigmas, L, 0, sig)
        for t, v in ((x, xn), (P, Pn), (K, Kn), (S, Sn), (SI, SIn)):
            if t is not None:
                t.copy_(torch.as_tensor(np.ascontiguousarray(v)))
        if status is not None:
            status.zero_()

    def _singular_S(sig, Hm, sh, Rm):
        sh = sig @ Hm.T if sh is None else sh
        d = sh - sh.mean(axis=0)
        return _singular(d.T @ d / (len(sig) - 1) + Rm)

    monkeypatch.setattr(E, "enkf_workspace_bytes", workspace_bytes_fn)
    monkeypatch.setattr(E, "enkf_predict", enkf_predict)
    monkeypatch.setattr(E, "enkf_update", enkf_update)
    return calls
