"""CPU stand-in for fk_enkf_bank_predict_f64 / fk_enkf_bank_update_f64 (include/filterhip.h), for HOST-LOGIC tests of
filterpy_amd.kalman.EnsembleKalmanFilterBank: it reads its operands exactly as the ABI lays them out -- one contiguous block per
ensemble in `layout`, the models once or once per ensemble by desc model_mode, z, the mask and the status per ensemble -- and
computes track by track with tests/enkf_port.py, so the Python layer (call sites and order of the draws, shapes, the mask's
bookkeeping, per-track models) can be held against the goldens of the live reference's loop on the CPU."""
import numpy as np
import torch

from fake_kf_engine import get, put, CPU, SHARED, PER_TRACK
from fake_info_engine import _singular, NOT_PD
import enkf_port


def install(monkeypatch):
    from filterpy_amd import _engine as E
    codes = {v: k for k, v in E.LAYOUTS.items()}
    calls = []
    monkeypatch.setattr(E, "require_gpu", lambda: CPU)
    real_dev = E.dev
    monkeypatch.setattr(E, "dev", lambda a, device=None: real_dev(a, device).clone())

    def check(desc, B):
        assert desc["model_mode"] in (SHARED, PER_TRACK) and desc["alpha_sq"] == 1.0 and desc["flags"] == 0
        assert 2 <= desc["N"] <= 2048 and B >= 1
        return desc["n"], desc["m"], desc["N"], codes[desc["layout"]], desc["model_mode"] == PER_TRACK

    def mats(t, per, B, shape):
        """the model operand as the ABI defines it: [shape] once, or [B][shape]"""
        if t is None:
            return [None] * B
        a = t.detach().numpy()
        assert a.size == (B if per else 1) * int(np.prod(shape)), (a.shape, per, B, shape)
        a = a.reshape((B if per else 1,) + tuple(shape))
        return [a[b if per else 0] for b in range(B)]

    def records(t, L, B, N, d):
        assert t.is_contiguous() and tuple(t.shape) == ((B, d, N) if L == "soa" else (B, N, d)), (tuple(t.shape), L, B, N, d)
        return get(t, L, 1, (d,))

    def draws(noise, fac, L, B, N, d):
        w = records(noise, L, B, N, d)
        return [w[b] if fac[b] is None else w[b] @ fac[b] for b in range(B)]

    def enkf_bank_predict(desc, B, noise, sigmas, x, P, *, F=None, factor=None, status=None):
        n, m, N, L, per = check(desc, B)
        calls.append(("predict", F is not None, factor is not None, per))
        assert tuple(x.shape) == (B, n) and tuple(P.shape) == (B, n, n)
        Fs, e = mats(F, per, B, (n, n)), draws(noise, mats(factor, per, B, (n, n)), L, B, N, n)
        sig = records(sigmas, L, B, N, n)
        for b in range(B):
            sig[b], xb, Pb = enkf_port.predict(sig[b], e[b], Fs[b])
            x[b].copy_(torch.as_tensor(xb))
            P[b].copy_(torch.as_tensor(Pb))
        put(sigmas, L, 1, sig)
        if status is not None:
            assert tuple(status.shape) == (B,) and status.dtype == torch.int32
            status.zero_()

    def enkf_bank_update(desc, B, R, z, noise, sigmas, x, P, *, H=None, sigmas_h=None, mask=None, factor=None, S=None, SI=None,
                         K=None, status=None):
        n, m, N, L, per = check(desc, B)
        assert (H is None) != (sigmas_h is None)
        calls.append(("update", H is not None, factor is not None, per, None if mask is None else mask.tolist()))
        assert tuple(x.shape) == (B, n) and tuple(P.shape) == (B, n, n) and tuple(z.shape) == (B, m)
        assert mask is None or (mask.dtype == torch.uint8 and tuple(mask.shape) == (B,))
        assert status is not None and tuple(status.shape) == (B,) and status.dtype == torch.int32
        Hs, Rs = mats(H, per, B, (m, n)), mats(R, per, B, (m, m))
        e = draws(noise, mats(factor, per, B, (m, m)), L, B, N, m)
        sig = records(sigmas, L, B, N, n)
        sh = None if sigmas_h is None else records(sigmas_h, L, B, N, m)
        status.zero_()
        for b in range(B):
            if mask is not None and not int(mask[b]):
                continue                                      # untouched: members, x, P, K, S, SI
            shb = sig[b] @ Hs[b].T if sh is None else sh[b]
            dv = shb - shb.mean(axis=0)
            if _singular(dv.T @ dv / (N - 1) + Rs[b]):
                status[b] = NOT_PD
                continue
            with np.errstate(all="ignore"):
                sig[b], xb, Pb, Kb, Sb, SIb = enkf_port.update(sig[b], x[b].numpy().copy(), P[b].numpy().copy(), z[b].numpy(), Rs[b],
                                                               e[b], Hs[b], None if sh is None else sh[b])
            for t, v in ((x, xb), (P, Pb), (K, Kb), (S, Sb), (SI, SIb)):
                if t is not None:
                    t[b].copy_(torch.as_tensor(np.ascontiguousarray(v)))
        put(sigmas, L, 1, sig)

    monkeypatch.setattr(E, "enkf_bank_predict", enkf_bank_predict)
    monkeypatch.setattr(E, "enkf_bank_update", enkf_bank_update)
    return calls
