"""CPU stand-in for the extended filter's three entry points (fk_ekf_predict_f64, fk_ekf_update_f64, fk_ekf_step_f64;
include/filterhip.h), for HOST-LOGIC tests of filterpy_amd.kalman.ExtendedKalmanFilter: it reads its operands exactly as the ABI
lays them out (records in `layout`, shared or per-track F / Q / R / B by model_mode, the uint8 mask, the R_JOSEPH_DIAG flag) and
computes with tests/ekf_port.py, so the Python layer -- shapes, attributes, modes, quirks -- can be held against the goldens
of the live reference on the CPU.  Status: NOT_PD where S has a non-positive pivot."""
import numpy as np
import torch

from fake_kf_engine import get, put, CPU
import ekf_port

NOT_PD, NONFINITE = 1, 2
SHARED, PER_TRACK = 0, 1
FLAG_R_JOSEPH_DIAG = 1


def _pd(A):
    if not np.isfinite(A).all():
        return False
    try:
        np.linalg.cholesky((A + A.T) / 2)
        return True
    except np.linalg.LinAlgError:
        return False


def install(monkeypatch):
    from filterpy_amd import _engine as E
    codes = {v: k for k, v in E.LAYOUTS.items()}
    calls = []
    monkeypatch.setattr(E, "require_gpu", lambda: CPU)
    real_dev = E.dev
    monkeypatch.setattr(E, "dev", lambda a, device=None: real_dev(a, device).clone())

    def model(t, desc, r, c):
        """-> (N, r, c)"""
        N, L = desc["N"], codes[desc["layout"]]
        if t is None:
            return None
        if desc["model_mode"] == PER_TRACK:
            return get(t, L, 0, (r, c))
        assert desc["model_mode"] == SHARED, desc
        return np.broadcast_to(t.detach().numpy().reshape(r, c), (N, r, c))

    def check(desc):
        assert desc["alpha_sq"] == 1.0 and desc["update_first"] == 0 and desc["flags"] in (0, FLAG_R_JOSEPH_DIAG), desc

    def do_predict(desc, F, Q, B, u, xs, Ps, st):
        n, nu, N, L = desc["n"], desc["nu"], desc["N"], codes[desc["layout"]]
        Fm, Qm = model(F, desc, n, n), model(Q, desc, n, n)
        Bm = model(B, desc, n, nu) if nu else None
        us = get(u, L, 0, (nu,)) if nu else None
        for i in range(N):
            xs[i], Ps[i] = ekf_port.predict(xs[i], Ps[i], Fm[i], Qm[i], None if Bm is None else Bm[i], None if us is None else us[i])
            if not (np.isfinite(xs[i]).all() and np.isfinite(Ps[i]).all()):
                st[i] |= NONFINITE

    def do_update(desc, H, R, y, mask, xs, Ps, outs, st):
        n, m, N, L = desc["n"], desc["m"], desc["N"], codes[desc["layout"]]
        Hs, ys, Rm = get(H, L, 0, (m, n)), get(y, L, 0, (m,)), model(R, desc, m, m)
        mk = None if mask is None else mask.detach().numpy().reshape(N) != 0
        arrs = {k: (get(t, L, 0, s) if t is not None else None) for k, (t, s) in outs.items()}
        for i in range(N):
            if mk is not None and not mk[i]:
                continue
            sr = float(Rm[i][0, 0]) if (desc["flags"] & FLAG_R_JOSEPH_DIAG) else None
            xs[i], Ps[i], K, S, SI = ekf_port.update(xs[i], Ps[i], Hs[i], ys[i], Rm[i], scalar_r=sr)
            if not _pd(S):
                st[i] |= NOT_PD
            vals = dict(K=K, S=S, SI=SI)
            if _pd(S):
                vals.update(ll=ekf_port.loglik(ys[i], S), maha=ekf_port.maha(ys[i], SI))
            else:
                vals.update(ll=np.nan, maha=np.nan)
            for k, a in arrs.items():
                if a is not None:
                    a[i] = vals[k]
        for k, (t, _) in outs.items():
            if t is not None:
                put(t, L, 0, arrs[k])

    def state(desc, x, P):
        n, L = desc["n"], codes[desc["layout"]]
        return get(x, L, 0, (n,)), get(P, L, 0, (n, n))

    def finish(desc, x, P, xs, Ps, status, st):
        L = codes[desc["layout"]]
        put(x, L, 0, xs)
        put(P, L, 0, Ps)
        if status is not None:
            status.copy_(torch.as_tensor(st))

    def by(desc, K, S, SI, ll, maha):
        n, m = desc["n"], desc["m"]
        return dict(K=(K, (n, m)), S=(S, (m, m)), SI=(SI, (m, m)), ll=(ll, ()), maha=(maha, ()))

    def ekf_predict(desc, F, Q, x, P, *, B=None, u=None, status=None):
        check(desc)
        calls.append(("predict", desc["model_mode"], desc["nu"]))
        xs, Ps = state(desc, x, P)
        st = np.zeros(desc["N"], dtype=np.int32)
        do_predict(desc, F, Q, B, u, xs, Ps, st)
        finish(desc, x, P, xs, Ps, status, st)

    def ekf_update(desc, H, R, y, x, P, *, mask=None, K=None, S=None, SI=None, log_likelihood=None, mahalanobis=None, status=None):
        check(desc)
        calls.append(("update", desc["model_mode"], desc["flags"]))
        xs, Ps = state(desc, x, P)
        st = np.zeros(desc["N"], dtype=np.int32)
        do_update(desc, H, R, y, mask, xs, Ps, by(desc, K, S, SI, log_likelihood, mahalanobis), st)
        finish(desc, x, P, xs, Ps, status, st)

    def ekf_step(desc, H, R, y, F, Q, x, P, *, mask=None, B=None, u=None, x_post=None, P_post=None, K=None, S=None, SI=None,
                 log_likelihood=None, mahalanobis=None, status=None):
        check(desc)
        calls.append(("step", desc["model_mode"], desc["nu"]))
        L = codes[desc["layout"]]
        xs, Ps = state(desc, x, P)
        st = np.zeros(desc["N"], dtype=np.int32)
        do_update(desc, H, R, y, mask, xs, Ps, by(desc, K, S, SI, log_likelihood, mahalanobis), st)
        put(x_post, L, 0, xs)
        put(P_post, L, 0, Ps)
        do_predict(desc, F, Q, B, u, xs, Ps, st)
        finish(desc, x, P, xs, Ps, status, st)

    for name, fn in (("ekf_predict", ekf_predict), ("ekf_update", ekf_update), ("ekf_step", ekf_step)):
        monkeypatch.setattr(E, name, fn)
    return calls
