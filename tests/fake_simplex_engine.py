"""CPU stand-ins for the fused UKF entry points with FK_UKF_FLAG_SIMPLEX, on top of tests/fake_ut_engine.py (whose building
blocks already take a point count): HOST-LOGIC tests of filterpy_amd.kalman.UKF with SimplexSigmaPoints only.  The arithmetic
inside is tests/simplex_port.py's; the kernels themselves are tested under -m gpu and, compiled for the host, by
tests/test_hostcheck_ukf_simplex.py."""
import numpy as np
import torch

import fake_ut_engine
import simplex_port as sp


def simplex_sizes(n, m, smoother):
    """the table of fk_ukf_linear_supported with FK_UKF_FLAG_SIMPLEX"""
    if smoother:
        return 1 <= n <= 9
    return (1 <= n <= 6 and 1 <= m <= 3) or (7 <= n <= 9 and 1 <= m <= 4)


def install(monkeypatch):
    """-> the list of calls (fake_ut_engine's, plus "simplex_batch" / "simplex_rts")"""
    from filterpy_amd import _engine as E
    calls = fake_ut_engine.install(monkeypatch)
    base_batch, base_rts = E.ukf_linear_batch, E.ukf_linear_rts

    def unrec(t, T, N, d, layout):
        return t.numpy().reshape(T, N, d).copy() if layout == "aos" else np.swapaxes(t.numpy().reshape(T, d, N), 1, 2).copy()

    def rerec(rec, arr, layout):
        if rec is not None:
            a = arr.reshape(arr.shape[0], arr.shape[1], -1)
            rec.copy_(torch.as_tensor(np.ascontiguousarray(a if layout == "aos" else np.swapaxes(a, 1, 2))).reshape(rec.shape))

    def ukf_linear_batch(n, m, N, T, layout, scale, F, H, Q, R, Wm, Wc, z, x, P, *, mask=None, means=None, covs=None, status=None,
                         paired=None):
        if paired != E.SIMPLEX:
            return base_batch(n, m, N, T, layout, scale, F, H, Q, R, Wm, Wc, z, x, P, mask=mask, means=means, covs=covs,
                              status=status, paired=paired)
        calls.append("simplex_batch")
        assert simplex_sizes(n, m, False) and Wm.numel() == n + 1 and Wc.numel() == n + 1
        Fh, Hh, Qh, Rh = F.numpy().reshape(n, n), H.numpy().reshape(m, n), Q.numpy().reshape(n, n), R.numpy().reshape(m, m)
        zs = unrec(z, T, N, m, layout)
        mk = None if mask is None else mask.numpy().reshape(T, N)
        xs, Ps = fake_ut_engine._get(x, layout, (n,)), fake_ut_engine._get(P, layout, (n, n))
        mu, cov = np.zeros((T, N, n)), np.zeros((T, N, n, n))
        for i in range(N):
            zl = [zs[t, i] if (mk is None or mk[t, i]) else None for t in range(T)]
            mu[:, i], cov[:, i] = sp.batch_filter(xs[i], Ps[i], zl, Fh, Hh, Qh, Rh, Wm.numpy(), Wc.numpy())
            xs[i], Ps[i] = mu[-1, i], cov[-1, i]
        fake_ut_engine._put(x, layout, xs)
        fake_ut_engine._put(P, layout, Ps)
        rerec(means, mu, layout)
        rerec(covs, cov, layout)

    def ukf_linear_rts(n, N, T, layout, scale, F, Q, Wm, Wc, Xs, Ps, xs, Ps_out, K=None, status=None, paired=None):
        if paired != E.SIMPLEX:
            return base_rts(n, N, T, layout, scale, F, Q, Wm, Wc, Xs, Ps, xs, Ps_out, K, status, paired)
        calls.append("simplex_rts")
        assert simplex_sizes(n, 1, True) and Wm.numel() == n + 1 and Wc.numel() == n + 1
        X, Pm = unrec(Xs, T, N, n, layout), unrec(Ps, T, N, n * n, layout).reshape(T, N, n, n)
        ox, oP, oK = np.zeros_like(X), np.zeros_like(Pm), np.zeros_like(Pm)
        for i in range(N):
            ox[:, i], oP[:, i], oK[:, i] = sp.rts_smoother(X[:, i], Pm[:, i], F.numpy().reshape(n, n), Q.numpy().reshape(n, n),
                                                           Wm.numpy(), Wc.numpy())
        rerec(xs, ox, layout)
        rerec(Ps_out, oP, layout)
        rerec(K, oK, layout)

    monkeypatch.setattr(E, "ukf_linear_supported", lambda n, m, paired=False, simplex=False: simplex_sizes(n, m, False) if simplex else True)
    monkeypatch.setattr(E, "ukf_linear_rts_supported", lambda n, paired=False, simplex=False: simplex_sizes(n, 1, True) if simplex else True)
    monkeypatch.setattr(E, "ukf_linear_batch", ukf_linear_batch)
    monkeypatch.setattr(E, "ukf_linear_rts", ukf_linear_rts)
    return calls
