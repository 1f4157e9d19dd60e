"""-m gpu: every entry point of include/filterhip.h that takes device arrays, run with ALL its arguments carved from a guarded
arena (tests/arena.py) at every pointer phase.

The rest of the suite hands the kernels buffers of their own from the caching allocator: every base pointer is 512-byte aligned
and nothing is looked at outside the outputs.  Here, per case, layout, bank size and phase:

    1. the call runs once on ordinary allocations;
    2. it runs again with every argument a view of one arena, the k-th argument at arena.phase_of(phase, k, dtype), outputs
       starting from the arena's NaN fill, every optional output requested;
    3. the return code is FK_OK (the _engine wrappers raise otherwise) and every status word is 0;
    4. arena.check(): every byte of the arena outside the `out` / `inout` views -- guards AND inputs -- holds what it held;
    5. every output and in-place argument is bit-identical to the ordinary run.

Bit identity is the expectation because alignment should select how bytes move, not how numbers are formed.  The one route this
file found where the alignment of a pointer regroups the arithmetic is the d = 4 gather of fk_resample_gather_mean_f64
(csrc/resample_kernels.hip:756 sends a 16-byte aligned `particles` to gather_mean4_kernel, whose two accumulator pairs and
unrolled index loads sum in another order than gather_mean_kernel): there the phases that change the route are held to the bar
tests/test_gpu_resample.py::test_gather_mean_vs_numpy holds the kernel to, against a longdouble mean.

The benign inputs are those of tests/test_gpu_tails.py (its spd / stable_F makers, the same scales), drawn from a RandomState
fixed per case and size.  Sizes: N in 1, 22 (one past the 21 tracks of a three-lane wave), 65, 130 (even: the pair-store routes),
257 (one past a workgroup); T = 3, so a fetch issued a step ahead wraps its double buffer.

The last tests run one stiff case of each family's *_hp module wholly inside an arena at the "mixed" phase, judged by that
module's own check, and read the header: an entry point added later fails test_every_entry_point_of_the_header_is_listed until it
has a case here."""
import os
import re

import numpy as np
import pytest

import arena as AR

NS = (1, 22, 65, 130, 257)
MEMBERS = (2, 65, 257)                  # ensemble sizes of the EnKF calls
NPS = (7, 2049, 8191)                   # particles per filter of the resamplers; Fn = 3
FN = 3
T = 3
BOTH = ("soa", "aos")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ----------------------------------------------------------------------------------------------------------------- inputs
def _makers():
    from test_gpu_tails import spd, stable_F
    return spd, stable_F


def kf_model(rs, n, m, nu=0):
    spd, stable_F = _makers()
    return dict(F=stable_F(rs, n), Q=spd(rs, n, 0.05), H=rs.randn(m, n), R=spd(rs, m, 0.5), B=0.1 * rs.randn(n, max(nu, 1)))


def kf_state(rs, N, n):
    spd, _ = _makers()
    return rs.randn(N, n), spd(rs, n, 2.0, (N,))


def D(n, m, N, L, T=1, nu=0, mode=0, flags=0, update_first=0):
    from filterpy_amd import _engine as E
    return dict(n=n, m=m, nu=nu, model_mode=mode, N=N, T=T, layout=E.LAYOUTS[L], update_first=update_first, alpha_sq=1.0, flags=flags)


def status(A, N):
    import torch
    return A.new((N,), torch.int32, "inout", fill=0, name="status")


def mask_of(A, rs, shape):
    return A.put((rs.rand(*shape) > 0.3).astype(np.uint8), name="mask")


def shared(A, M, *names):
    return [A.put(M[k], name=k) for k in names]


def merwe(n):
    from oracle import ukf_oracle
    alpha, beta, kappa = 0.5, 2.0, 3.0 - n
    Wm, Wc = ukf_oracle.merwe_weights(n, alpha, beta, kappa)
    return Wm, Wc, alpha ** 2 * (n + kappa)            # scale = lambda + n


# ------------------------------------------------------------------------------------------------------------------ cases
# Every case: fn(A, rs, N, L, **kw) carves its arguments from the allocator A (arena.ArenaAlloc / PlainAlloc) and returns the
# call as a thunk; the harness takes the arena's snapshot between the two.
def kf_batch(A, rs, N, L, n, m, mask=False, nu=0, inter=False, ex=False):
    from filterpy_amd import _engine as E
    M = kf_model(rs, n, m, nu)
    x0, P0 = kf_state(rs, N, n)
    dF, dQ, dH, dR = shared(A, M, "F", "Q", "H", "R")
    dB = A.put(M["B"], name="B") if nu else None
    du = A.put(rs.randn(T, N, nu), "in", L, 1, name="u") if nu else None
    dz = A.put(rs.randn(T, N, m) * 2, "in", L, 1, name="z")
    dm = mask_of(A, rs, (T, N)) if mask else None
    dx, dP = A.put(x0, "inout", L, 0, name="x"), A.put(P0, "inout", L, 0, name="P")
    means, means_p = A.records((T,), N, n, L, name="means"), A.records((T,), N, n, L, name="means_p")
    nn = n * n
    if inter:                      # FK_KF_FLAG_COV_INTERLEAVED: alloc_cov_pair's layout, carved by hand
        cov2 = A.new((T, N, 2, nn) if L == "aos" else (T, 2, nn, N), rec=2 * nn, name="cov2")
        covs, covs_p = (cov2[:, :, 0], cov2[:, :, 1]) if L == "aos" else (cov2[:, 0], cov2[:, 1])
    else:
        covs, covs_p = A.records((T,), N, nn, L, name="covs"), A.records((T,), N, nn, L, name="covs_p")
    st = status(A, N)
    d = D(n, m, N, L, T, nu, flags=2 if inter else 0)
    kw = dict(B=dB, u=du, mask=dm, means=means, covs=covs, means_p=means_p, covs_p=covs_p, status=st)
    if not ex:
        return lambda: E.kf_batch_filter(d, dF, dQ, dH, dR, dz, dx, dP, **kw)
    extras = {k: A.records((T,), N, e, L, name=k) for k, e in (("y", m), ("K", n * m), ("S", m * m), ("SI", m * m))}
    extras.update({k: A.new((T, N), name=k) for k in ("log_likelihood", "mahalanobis")})
    return lambda: E.kf_batch_filter_ex(d, dF, dQ, dH, dR, dz, dx, dP, extras, **kw)


def kf_predict(A, rs, N, L, n, m, nu=0):
    from filterpy_amd import _engine as E
    M = kf_model(rs, n, m, nu)
    x0, P0 = kf_state(rs, N, n)
    dF, dQ = shared(A, M, "F", "Q")
    dB = A.put(M["B"], name="B") if nu else None
    du = A.put(rs.randn(N, nu), "in", L, 0, name="u") if nu else None
    dx, dP, st = A.put(x0, "inout", L, 0, name="x"), A.put(P0, "inout", L, 0, name="P"), status(A, N)
    return lambda: E.kf_predict(D(n, m, N, L, nu=nu), dF, dQ, dx, dP, B=dB, u=du, status=st)


def kf_update(A, rs, N, L, n, m, mask=False, given=None):
    """given: None, "S_ONLY" or "SI_GIVEN" (the caller-supplied inverse, include/filterhip.h)"""
    from filterpy_amd import _engine as E
    from filterpy_amd._abi import FK_KF_FLAG_S_ONLY, FK_KF_FLAG_SI_GIVEN
    M = kf_model(rs, n, m)
    x0, P0 = kf_state(rs, N, n)
    z = rs.randn(N, m) * 2
    dH, dR = shared(A, M, "H", "R")
    dz = A.put(z, "in", L, 0, name="z")
    dm = mask_of(A, rs, (N,)) if mask else None
    dx, dP = A.put(x0, "inout", L, 0, name="x"), A.put(P0, "inout", L, 0, name="P")
    o = {k: A.records((), N, e, L, name=k) for k, e in (("y", m), ("K", n * m), ("S", m * m))}
    if given == "SI_GIVEN":
        S = M["H"] @ P0 @ M["H"].T + M["R"]
        o["SI"] = A.put(np.linalg.inv(S), "in", L, 0, name="SI")
    else:
        o["SI"] = A.records((), N, m * m, L, name="SI")
    st = status(A, N)
    flags = {None: 0, "S_ONLY": FK_KF_FLAG_S_ONLY, "SI_GIVEN": FK_KF_FLAG_SI_GIVEN}[given]
    return lambda: E.kf_update(D(n, m, N, L, flags=flags), dH, dR, dz, dx, dP, mask=dm, status=st, **o)


def _filter_output(rs, N, n):
    spd, _ = _makers()
    return rs.randn(T, N, n), spd(rs, n, 2.0, (T, N))


def kf_rts(A, rs, N, L, n, given=None):
    from filterpy_amd import _engine as E
    from filterpy_amd._abi import FK_KF_FLAG_PP_ONLY, FK_KF_FLAG_PPINV_GIVEN
    M = kf_model(rs, n, 1)
    Xs, Ps = _filter_output(rs, N, n)
    dF, dQ = shared(A, M, "F", "Q")
    dX, dPs = A.put(Xs, "in", L, 1, name="Xs"), A.put(Ps, "in", L, 1, name="Ps")
    xs, Ps_out = A.records((T,), N, n, L, name="xs"), A.records((T,), N, n * n, L, name="Ps_out")
    if given == "PPINV_GIVEN":
        Pp = M["F"] @ Ps @ M["F"].T + M["Q"]
        K = A.put(np.linalg.inv(Pp), "inout", L, 1, name="K")
    else:
        K = A.records((T,), N, n * n, L, name="K")
    Pp, st = A.records((T,), N, n * n, L, name="Pp"), status(A, N)
    flags = {None: 0, "PP_ONLY": FK_KF_FLAG_PP_ONLY, "PPINV_GIVEN": FK_KF_FLAG_PPINV_GIVEN}[given]
    return lambda: E.kf_rts(D(n, 1, N, L, T, flags=flags), dF, dQ, dX, dPs, xs, Ps_out, K, Pp, status=st)


def fls_batch(A, rs, N, L, n, m, lag=2, Tf=5, k0=0, nu=0):
    from filterpy_amd import _engine as E
    M = kf_model(rs, n, m, nu)
    x0, P0 = kf_state(rs, N, n)
    W = min(max(lag, 1) - 1, k0)
    dF, dQ, dH, dR = shared(A, M, "F", "Q", "H", "R")
    dB = A.put(M["B"], name="B") if nu else None
    du = A.put(rs.randn(Tf, N, nu), "in", L, 1, name="u") if nu else None
    dz = A.put(rs.randn(Tf, N, m) * 2, "in", L, 1, name="z")
    dx, dP = A.put(x0, "inout", L, 0, name="x"), A.put(P0, "inout", L, 0, name="P")
    xs = A.put(rs.randn(W + Tf, N, n), "inout", L, 1, name="xs")        # the first W rows: a previous call's pending window
    xhat = A.records((Tf,), N, n, L, name="xhat")
    y, S, st = A.records((), N, m, L, name="y"), A.records((), N, m * m, L, name="S"), status(A, N)
    return lambda: E.fls_batch(D(n, m, N, L, Tf, nu), lag, k0, dF, dQ, dH, dR, dz, dx, dP, xs, xhat, B=dB, u=du, y=y, S=S, status=st)


def _sqrt_model(rs, n, m, nu):
    M = kf_model(rs, n, m, nu)
    M["Q12"], M["R12"] = np.linalg.cholesky(M["Q"]), np.linalg.cholesky(M["R"])
    return M


def srkf(A, rs, N, L, n, m, what, mask=False, nu=0):
    from filterpy_amd import _engine as E
    M = _sqrt_model(rs, n, m, nu)
    x0, P0 = kf_state(rs, N, n)
    Tn = T if what == "batch" else 1
    lead = (Tn,) if what == "batch" else ()
    dB = A.put(M["B"], name="B") if nu and what != "update" else None
    du = A.put(rs.randn(*lead, N, nu), "in", L, len(lead), name="u") if nu and what != "update" else None
    dx, dP = A.put(x0, "inout", L, 0, name="x"), A.put(np.linalg.cholesky(P0), "inout", L, 0, name="P12")
    st = status(A, N)
    if what == "predict":
        dF, dQ = shared(A, M, "F", "Q12")
        return lambda: E.srkf_predict(D(n, m, N, L, nu=nu), dF, dQ, dx, dP, B=dB, u=du, status=st)
    dH, dR = shared(A, M, "H", "R12")
    dz = A.put(rs.randn(*lead, N, m) * 2, "in", L, len(lead), name="z")
    dm = mask_of(A, rs, (*lead, N)) if mask else None
    by = {k: A.records((), N, e, L, name=k) for k, e in (("y", m), ("K", n * m), ("S12", m * m), ("SI12", m * m))}
    if what == "update":
        return lambda: E.srkf_update(D(n, m, N, L), dH, dR, dz, dx, dP, mask=dm, status=st, **by)
    dF, dQ = shared(A, M, "F", "Q12")
    h = {k: A.records((T,), N, e, L, name=k) for k, e in (("means", n), ("covs", n * n), ("means_p", n), ("covs_p", n * n))}
    return lambda: E.srkf_batch(D(n, m, N, L, T, nu), dF, dQ, dH, dR, dz, dx, dP, B=dB, u=du, mask=dm, status=st, **h, **by)


def info(A, rs, N, L, n, m, what, mask=False, nu=0):
    from filterpy_amd import _engine as E
    M = kf_model(rs, n, m, nu)
    M["Rinv"] = np.linalg.inv(M["R"])
    x0, P0 = kf_state(rs, N, n)
    lead = (T,) if what == "batch" else ()
    dB = A.put(M["B"], name="B") if nu and what != "update" else None
    du = A.put(rs.randn(*lead, N, nu), "in", L, len(lead), name="u") if nu and what != "update" else None
    dx, dP = A.put(x0, "inout", L, 0, name="x"), A.put(np.linalg.inv(P0), "inout", L, 0, name="P_inv")
    st = status(A, N)
    if what == "predict":
        dF, dQ = shared(A, M, "F", "Q")
        return lambda: E.info_predict(D(n, m, N, L, nu=nu), dF, dQ, dx, dP, B=dB, u=du, status=st)
    dH, dR = shared(A, M, "H", "Rinv")
    dz = A.put(rs.randn(*lead, N, m) * 2, "in", L, len(lead), name="z")
    dm = mask_of(A, rs, (*lead, N)) if mask else None
    if what == "update":
        y, K = A.records((), N, m, L, name="y"), A.records((), N, n * m, L, name="K")
        return lambda: E.info_update(D(n, m, N, L), dH, dR, dz, dx, dP, mask=dm, y=y, K=K, status=st)
    dF, dQ = shared(A, M, "F", "Q")
    h = {k: A.records((T,), N, e, L, name=k) for k, e in (("means", n), ("covs", n * n), ("means_p", n), ("covs_p", n * n))}
    return lambda: E.info_batch(D(n, m, N, L, T, nu), dF, dQ, dH, dR, dz, dx, dP, B=dB, u=du, mask=dm, status=st, **h)


def _cubature_points(x0, P0, n):
    """(N, 2n, n): x +- sqrt(n) U[k], U = cholesky(P) upper (CubatureKalmanFilter.py:32-61)"""
    U = np.swapaxes(np.linalg.cholesky(P0), -1, -2)
    return np.concatenate([x0[:, None] + np.sqrt(n) * U, x0[:, None] - np.sqrt(n) * U], axis=1)


def ckf_block(A, rs, N, L, n, m, what):
    from filterpy_amd import _engine as E
    M = kf_model(rs, n, m)
    x0, P0 = kf_state(rs, N, n)
    sig = _cubature_points(x0, P0, n)
    if what == "sigma_points":
        dx, dP = A.put(x0, "in", L, 0, name="x"), A.put(P0, "in", L, 0, name="P")
        out, st = A.records((), N, 2 * n * n, L, name="sigmas"), status(A, N)
        return lambda: E.ckf_sigma_points(n, N, L, dx, dP, out, st)
    if what == "transform":
        ds, dQ = A.put(sig, "in", L, 0, name="sigmas"), A.put(M["Q"], name="Q")
        xo, Po = A.records((), N, n, L, name="x_out"), A.records((), N, n * n, L, name="P_out")
        return lambda: E.ckf_transform(n, 2 * n, N, L, ds, dQ, xo, Po)
    dsf, dsh = A.put(sig, "in", L, 0, name="sigmas_f"), A.put(sig @ M["H"].T, "in", L, 0, name="sigmas_h")
    dR, dz = A.put(M["R"], name="R"), A.put(x0 @ M["H"].T + rs.randn(N, m), "in", L, 0, name="z")
    dx, dP = A.put(x0, "inout", L, 0, name="x"), A.put(P0 + M["Q"], "inout", L, 0, name="P")
    by = {k: A.records((), N, e, L, name=k) for k, e in (("zp", m), ("S", m * m), ("SI", m * m), ("Pxz", n * m), ("K", n * m), ("y", m))}
    st = status(A, N)
    return lambda: E.ckf_update(n, m, N, L, dsf, dsh, dR, dz, dx, dP, status=st, **by)


def ckf_linear(A, rs, N, L, n, m, what, mask=False):
    from filterpy_amd import _engine as E
    M = kf_model(rs, n, m)
    x0, P0 = kf_state(rs, N, n)
    # the points record a predict leaves: the centre, then the n half-differences E[k] = F U[k] (include/filterhip.h)
    U = np.swapaxes(np.linalg.cholesky(P0), -1, -2)
    pts = np.concatenate([x0, (U @ M["F"].T).reshape(N, n * n)], axis=1)
    dx = A.put(x0, "inout", L, 0, name="x")
    # (update: the P the predict that left these points leaves, sum_k E[k] E[k]' + Q)
    dP = A.put(M["F"] @ P0 @ M["F"].T + M["Q"] if what == "update" else P0, "inout", L, 0, name="P")
    st = status(A, N)
    if what == "predict":
        dF, dQ = shared(A, M, "F", "Q")
        dp = A.records((), N, n + n * n, L, name="points")
        return lambda: E.ckf_linear_predict(D(n, m, N, L), dF, dQ, dx, dP, dp, status=st)
    dH, dR = shared(A, M, "H", "R")
    if what == "update":
        dz = A.put(rs.randn(N, m) * 2, "in", L, 0, name="z")
        dm = mask_of(A, rs, (N,)) if mask else None
        dp = A.put(pts, "in", L, 0, name="points")
        by = {k: A.records((), N, e, L, name=k) for k, e in (("y", m), ("K", n * m), ("S", m * m), ("SI", m * m))}
        return lambda: E.ckf_linear_update(D(n, m, N, L), dH, dR, dz, dx, dP, dp, mask=dm, status=st, **by)
    dF, dQ = shared(A, M, "F", "Q")
    dz = A.put(rs.randn(T, N, m) * 2, "in", L, 1, name="z")
    dm = mask_of(A, rs, (T, N)) if mask else None
    dp = A.put(np.zeros((N, n + n * n)), "inout", L, 0, name="points")
    h = {k: A.records((T,), N, e, L, name=k) for k, e in (("means", n), ("covs", n * n), ("means_p", n), ("covs_p", n * n))}
    return lambda: E.ckf_linear_batch(D(n, m, N, L, T), dF, dQ, dH, dR, dz, dx, dP, dp, mask=dm, status=st, **h)


def ekf(A, rs, N, L, n, m, what, per_track=False, mask=False, nu=0):
    from filterpy_amd import _engine as E
    M = kf_model(rs, n, m, nu)
    x0, P0 = kf_state(rs, N, n)

    def model(k, shape):
        if not per_track:
            return A.put(M[k], name=k)
        per = np.repeat(M[k][None], N, axis=0) * (1.0 + 0.01 * rs.rand(N, 1, 1))
        if k in ("Q", "R"):
            per = (per + np.swapaxes(per, -1, -2)) / 2
        return A.put(per, "in", L, 0, name=k)
    d = D(n, m, N, L, nu=nu, mode=1 if per_track else 0)
    upd = what in ("update", "step")
    if upd:
        dH, dR = A.put(np.repeat(M["H"][None], N, axis=0) + 0.05 * rs.randn(N, m, n), "in", L, 0, name="H"), model("R", (m, m))
        dy = A.put(rs.randn(N, m), "in", L, 0, name="y")
        dm = mask_of(A, rs, (N,)) if mask else None
    if what in ("predict", "step"):
        dF, dQ = model("F", (n, n)), model("Q", (n, n))
        dB = model("B", (n, nu)) if nu else None
        du = A.put(rs.randn(N, nu), "in", L, 0, name="u") if nu else None
    dx, dP = A.put(x0, "inout", L, 0, name="x"), A.put(P0, "inout", L, 0, name="P")
    st = status(A, N)
    if what == "predict":
        return lambda: E.ekf_predict(d, dF, dQ, dx, dP, B=dB, u=du, status=st)
    by = {k: A.records((), N, e, L, name=k) for k, e in (("K", n * m), ("S", m * m), ("SI", m * m))}
    by.update({k: A.new((N,), name=k) for k in ("log_likelihood", "mahalanobis")})
    if what == "update":
        return lambda: E.ekf_update(d, dH, dR, dy, dx, dP, mask=dm, status=st, **by)
    xp, Pp = A.records((), N, n, L, name="x_post"), A.records((), N, n * n, L, name="P_post")
    return lambda: E.ekf_step(d, dH, dR, dy, dF, dQ, dx, dP, mask=dm, B=dB, u=du, x_post=xp, P_post=Pp, status=st, **by)


def enkf(A, rs, N, L, n, m, what, factor=False, sigmas_h=False, bank=0, per_track=False, mask=False):
    """N: the members of an ensemble; bank: 0 = the single calls, else the number of ensembles of the bank calls"""
    import torch
    from filterpy_amd import _engine as E
    spd, _ = _makers()
    M = kf_model(rs, n, m)
    B = max(bank, 1)
    lead = (B,) if bank else ()
    x0 = rs.randn(*lead, n) * 3
    sig = x0[..., None, :] + rs.randn(*lead, N, n)
    d = D(n, m, N, L, mode=1 if per_track else 0)
    dim = n if what == "predict" else m
    fac = spd(rs, dim, 0.1, lead if per_track else ())
    dn = A.put(rs.randn(*lead, N, dim) * (1.0 if factor else 0.3), "in", L, len(lead), name="noise")
    df = A.put(fac, name="factor") if factor else None

    def model(k):
        return A.put(np.repeat(M[k][None], B, axis=0) * (1.0 + 0.01 * rs.rand(B, 1, 1)) if per_track else M[k], name=k)
    ds = A.put(sig, "inout", L, len(lead), name="sigmas")
    dx = A.put(sig.mean(axis=-2) + 0.01 * rs.randn(*lead, n), "inout", name="x")
    st = status(A, B)
    ws = None if bank else A.new((max(E.enkf_workspace_bytes(n, m, N), 8),), torch.uint8, "inout", name="workspace", align=8)
    if what == "predict":
        dF, dP = model("F"), A.new((*lead, n * n), name="P")
        if bank:
            return lambda: E.enkf_bank_predict(d, B, dn, ds, dx, dP, F=dF, factor=df, status=st)
        return lambda: E.enkf_predict(d, dn, ds, dx, dP, ws, F=dF, factor=df, status=st)
    dev = sig - sig.mean(axis=-2, keepdims=True)
    dP = A.put((np.swapaxes(dev, -1, -2) @ dev / (N - 1) + 0.1 * np.eye(n)).reshape(*lead, n * n), "inout", name="P")
    dR, dz = model("R"), A.put(rs.randn(*lead, m), name="z")
    dH = None if sigmas_h else model("H")
    dsh = A.put(sig @ M["H"].T, "in", L, len(lead), name="sigmas_h") if sigmas_h else None
    by = {k: A.new((*lead, e), name=k) for k, e in (("S", m * m), ("SI", m * m), ("K", n * m))}
    if bank:
        dm = mask_of(A, rs, (B,)) if mask else None
        return lambda: E.enkf_bank_update(d, B, dR, dz, dn, ds, dx, dP, H=dH, sigmas_h=dsh, mask=dm, factor=df, status=st, **by)
    return lambda: E.enkf_update(d, dR, dz, dn, ds, dx, dP, ws, H=dH, sigmas_h=dsh, factor=df, status=st, **by)


def ut_block(A, rs, N, L, n, m, what):
    from filterpy_amd import _engine as E
    M = kf_model(rs, n, m)
    x0, P0 = kf_state(rs, N, n)
    Wm, Wc, scale = merwe(n)
    k = 2 * n + 1
    U = np.swapaxes(np.linalg.cholesky(scale * P0), -1, -2)
    sig = np.concatenate([x0[:, None], x0[:, None] + U, x0[:, None] - U], axis=1)           # (N, 2n+1, n)
    R = lambda a, name, role="in": A.put(a, role, L, 0, name=name)  # noqa: E731
    if what == "sigma_points":
        dx, dP, out, st = R(x0, "x"), R(P0, "P"), A.records((), N, k * n, L, name="sigmas"), status(A, N)
        return lambda: E.ut_sigma_points(n, N, L, scale, dx, dP, out, st)
    if what == "transform":
        ds, dWm, dWc, dQ = R(sig, "sigmas"), A.put(Wm, name="Wm"), A.put(Wc, name="Wc"), A.put(M["Q"], name="Q")
        xo, Po = A.records((), N, n, L, name="x_out"), A.records((), N, n * n, L, name="P_out")
        return lambda: E.ut_transform(n, k, N, L, ds, dWm, dWc, dQ, xo, Po)
    if what == "cross_variance":
        sh = sig @ M["H"].T
        dx, dz, dsf, dsh = R(x0, "x"), R(sh[:, 0], "z"), R(sig, "sigmas_f"), R(sh, "sigmas_h")
        dWc, out = A.put(Wc, name="Wc"), A.records((), N, n * m, L, name="Pxz")
        return lambda: E.ut_cross_variance(n, m, k, N, L, dx, dz, dsf, dsh, dWc, out)
    if what == "linear_map":
        dM, din, out = A.put(M["H"], name="M"), R(sig, "in"), A.records((), N, k * m, L, name="out")
        return lambda: E.ut_linear_map(n, m, k, N, L, dM, din, out)
    if what == "correct":
        S = M["H"] @ P0 @ M["H"].T + M["R"]
        dPxz, dzp, dS = R(P0 @ M["H"].T, "Pxz"), R(x0 @ M["H"].T, "zp"), R(S, "S")
        dz = R(x0 @ M["H"].T + rs.randn(N, m), "z")
        dx, dP, K, st = R(x0, "x", "inout"), R(P0, "P", "inout"), A.records((), N, n * m, L, name="K"), status(A, N)
        return lambda: E.ukf_correct(n, m, N, L, dPxz, dzp, dS, dz, dx, dP, K, st)
    assert what == "rts_correct"
    spd, _ = _makers()
    Pb = M["F"] @ P0 @ M["F"].T + M["Q"]
    dPxb, dxb, dPb = R(P0 @ M["F"].T, "Pxb"), R(x0 @ M["F"].T, "xb"), R(Pb, "Pb")
    dxn, dPn = R(x0 @ M["F"].T + 0.1 * rs.randn(N, n), "xn"), R(spd(rs, n, 2.0, (N,)), "Pn")
    dx, dP, K, st = R(x0, "x", "inout"), R(P0, "P", "inout"), A.records((), N, n * n, L, name="K"), status(A, N)
    return lambda: E.ukf_rts_correct(n, N, L, dPxb, dxb, dPb, dxn, dPn, dx, dP, K, st)


def ukf_fused(A, rs, N, L, n, m, what, mask=False, paired=True):
    from filterpy_amd import _engine as E
    M = kf_model(rs, n, m)
    Wm, Wc, scale = merwe(n)
    dF, dQ, dWm, dWc = A.put(M["F"], name="F"), A.put(M["Q"], name="Q"), A.put(Wm, name="Wm"), A.put(Wc, name="Wc")
    st = status(A, N)
    if what == "rts":
        Xs, Ps = _filter_output(rs, N, n)
        dX, dPs = A.put(Xs, "in", L, 1, name="Xs"), A.put(Ps, "in", L, 1, name="Ps")
        xs, ps, K = (A.records((T,), N, e, L, name=k) for k, e in (("xs", n), ("Ps_out", n * n), ("K", n * n)))
        return lambda: E.ukf_linear_rts(n, N, T, L, scale, dF, dQ, dWm, dWc, dX, dPs, xs, ps, K, st, paired=paired)
    x0, P0 = kf_state(rs, N, n)
    dH, dR = shared(A, M, "H", "R")
    dz = A.put(rs.randn(T, N, m) * 2, "in", L, 1, name="z")
    dm = mask_of(A, rs, (T, N)) if mask else None
    dx, dP = A.put(x0, "inout", L, 0, name="x"), A.put(P0, "inout", L, 0, name="P")
    means, covs = A.records((T,), N, n, L, name="means"), A.records((T,), N, n * n, L, name="covs")
    return lambda: E.ukf_linear_batch(n, m, N, T, L, scale, dF, dH, dQ, dR, dWm, dWc, dz, dx, dP, mask=dm, means=means,
                                      covs=covs, status=st, paired=paired)


def steadystate(A, rs, N, L, n, m, per_track=False, mask=False, nu=0):
    from filterpy_amd import _engine as E
    M = kf_model(rs, n, m, nu)
    K = 0.2 * rs.randn(*((N,) if per_track else ()), n, m)
    dF, dH = shared(A, M, "F", "H")
    dK = A.put(K, "in", L, 0, name="K") if per_track else A.put(K, name="K")
    dB = A.put(M["B"], name="B") if nu else None
    du = A.put(rs.randn(T, N, nu), "in", L, 1, name="u") if nu else None
    dz = A.put(rs.randn(T, N, m), "in", L, 1, name="z")
    dm = mask_of(A, rs, (T, N)) if mask else None
    dx = A.put(rs.randn(N, n), "inout", L, 0, name="x")
    o = {k: A.records((T,), N, e, L, name=k) for k, e in (("means", n), ("means_p", n), ("y", m))}
    return lambda: E.kf_steadystate(D(n, m, N, L, T, nu, mode=1 if per_track else 0), dF, dH, dK, dz, dx, B=dB, u=du, mask=dm, **o)


def update_correlated(A, rs, N, L, n, m, per_track=False, mask=False):
    from filterpy_amd import _engine as E
    M = kf_model(rs, n, m)
    x0, P0 = kf_state(rs, N, n)
    Mx = 0.02 * rs.randn(*((N,) if per_track else ()), n, m)
    dH, dR = shared(A, M, "H", "R")
    dM = A.put(Mx, "in", L, 0, name="M") if per_track else A.put(Mx, name="M")
    dz = A.put(rs.randn(N, m), "in", L, 0, name="z")
    dm = mask_of(A, rs, (N,)) if mask else None
    dx, dP = A.put(x0, "inout", L, 0, name="x"), A.put(P0, "inout", L, 0, name="P")
    o = {k: A.records((), N, e, L, name=k) for k, e in (("y", m), ("K", n * m), ("S", m * m), ("SI", m * m))}
    st = status(A, N)
    return lambda: E.kf_update_correlated(D(n, m, N, L, mode=1 if per_track else 0), dH, dR, dM, dz, dx, dP, mask=dm, status=st, **o)


def imm(A, rs, N, L, n, m, nm, mmae=False, masked=False, nu=0, plain=False):
    """plain: fk_imm_batch_f64 itself (the wrapper _engine does not bind), through filterpy_amd._abi"""
    from filterpy_amd import _abi, _engine as E
    spd, stable_F = _makers()
    Fs = np.array([stable_F(rs, n) for _ in range(nm)])
    Qs = np.array([spd(rs, n, 0.05 * (j + 1)) for j in range(nm)])
    Hs = np.array([rs.randn(m, n)] * nm)
    Rs = np.array([spd(rs, m, 0.5) for _ in range(nm)])
    Mt = rs.rand(nm, nm) + 2 * np.eye(nm)
    Mt /= Mt.sum(axis=1, keepdims=True)
    mu0 = rs.rand(N, nm) + 0.1
    mu0 /= mu0.sum(axis=1, keepdims=True)
    dF, dQ, dH, dR = (A.put(a, name=k) for k, a in (("F", Fs), ("Q", Qs), ("H", Hs), ("R", Rs)))
    dM = None if mmae else A.put(Mt, name="M")
    dz = A.put(rs.randn(T, N, m) * 2, "in", L, 1, name="z")
    dm = mask_of(A, rs, (T, N)) if masked else None
    ll0 = A.put(np.full((N, nm), -np.inf), "inout", L, 0, name="ll0") if masked else None
    dB = A.put(0.1 * rs.randn(nm, n, nu), name="B") if nu else None
    du = A.put(rs.randn(T, N, nu), "in", L, 1, name="u") if nu else None
    dxs = A.put(rs.randn(N, nm * n), "inout", L, 0, name="xs")
    dPs = A.put(spd(rs, n, 2.0, (N, nm)).reshape(N, nm * n * n), "inout", L, 0, name="Ps")
    dmu = A.put(mu0, "inout", L, 0, name="mu")
    names = [("x_out", n), ("P_out", n * n), ("mu_out", nm), ("x_prior_out", n), ("P_prior_out", n * n), ("likelihood_out", nm)]
    if mmae:                              # (the prior outputs are not defined for MMAE, include/filterhip.h)
        names = [ke for ke in names if "prior" not in ke[0]]
    out = {k: A.records((T,), N, e, L, name=k) for k, e in names}
    st = status(A, N)
    if plain:
        def call():
            d = _abi.fk_imm_desc(n=n, m=m, n_models=nm, layout=E.LAYOUTS[L], N=N, T=T, phase=0, flags=0)
            p = [E._ptr(t) for t in (dF, dQ, dH, dR, dM, dz, dxs, dPs, dmu, *(out[k] for k, _ in names), st)]
            _abi.check(_abi.lib().fk_imm_batch_f64(d, *p, E._stream()), "fk_imm_batch_f64")
        return call
    return lambda: E.imm_batch(n, m, nm, N, T, L, dF, dQ, dH, dR, dM, dz, dxs, dPs, dmu, status=st, mmae=mmae, zmask=dm, ll0=ll0,
                               nu=nu, B=dB, u=du, **out)


def _weights(rs, Np):
    w = rs.rand(FN, Np) ** np.array([[1], [3], [1]])
    w[2, : Np // 2] = 0.0                                      # zero weights
    return w / w.sum(axis=1, keepdims=True)


def resample(A, rs, Np, L, what):
    import torch
    from filterpy_amd import _abi, _engine as E
    lib = _abi.lib()
    w = _weights(rs, Np)
    dw = A.put(w, name="w")
    if what == "cumsum":
        cs = A.new((FN, Np), name="cs")
        return lambda: E.cumsum_exact(FN, Np, dw, cs, force_last_one=True)
    if what in ("systematic", "stratified"):
        du = A.put(rs.rand(FN) if what == "systematic" else rs.rand(FN, Np), name="u")
        idx, st = A.new((FN, Np), torch.int32, name="idx"), status(A, FN)
        nb = E.resample_workspace_bytes(FN, Np)
        ws = A.new((max(nb, 16),), torch.uint8, "inout", name="workspace", align=16)       # its stated 16-byte alignment
        fn = getattr(lib, "fk_resample_%s_f64" % what)
        return lambda: _abi.check(fn(FN, Np, E._ptr(dw), E._ptr(du), E._ptr(idx), E._ptr(st), E._ptr(ws), nb, E._stream()), what)
    if what == "multinomial":
        Nu = Np + 3
        du, idx = A.put(rs.rand(FN, Nu), name="u"), A.new((FN, Nu), torch.int64, name="idx")
        nb = int(lib.fk_multinomial_workspace_bytes(FN, Np))
        ws = A.new((nb,), torch.uint8, "inout", name="workspace", align=16)
        return lambda: _abi.check(lib.fk_resample_multinomial_f64(FN, Np, Nu, E._ptr(dw), E._ptr(du), E._ptr(idx), E._ptr(ws), nb,
                                                                  E._stream()), what)
    if what == "residual_fill":
        idx, k = A.new((FN, Np), torch.int32, name="idx"), A.new((FN,), torch.int64, name="k")
        cs, st = A.new((FN, Np), name="cs"), status(A, FN)
        return lambda: E.resample_residual_fill(FN, Np, dw, idx, k, cs, st)
    assert what == "residual_draw"
    # the fill runs first, as set-up (before the snapshot): what it writes -- cs, k -- are the draw's inputs
    idx, k = A.new((FN, Np), torch.int32, "inout", name="idx"), A.new((FN,), torch.int64, "in", name="k")
    cs, st = A.new((FN, Np), role="in", name="cs"), status(A, FN)
    E.resample_residual_fill(FN, Np, dw, idx, k, cs, st)
    torch.cuda.synchronize()
    left = Np - k.cpu().numpy()
    assert (left >= 0).all() and left.sum() > 0
    uoff = A.put(np.concatenate([[0], np.cumsum(left)[:-1]]).astype(np.int64), name="uoff")
    du = A.put(rs.rand(int(left.sum())), name="u")
    return lambda: E.resample_residual_draw(FN, Np, cs, k, uoff, du, idx)


def gather_mean(A, rs, Np, L, d):
    import torch
    from filterpy_amd import _engine as E
    parts = rs.randn(FN, Np, d) + 3.0
    idx = np.sort(rs.randint(0, Np, size=(FN, Np)), axis=1).astype(np.int32)               # non-decreasing, as a resampler's
    dp, di = A.put(parts, name="particles"), A.put(idx, name="idx")
    mean = A.new((FN, d), torch.float64, name="mean")
    return lambda: E.resample_gather_mean(FN, Np, d, dp, di, mean)


# ------------------------------------------------------------------------------------------------------------------ table
class Case:
    def __init__(self, cid, entries, fn, kw=None, env=None, sizes=NS, layouts=BOTH):
        self.id, self.entries, self.fn, self.kw, self.env = cid, entries, fn, kw or {}, env or {}
        self.sizes, self.layouts = sizes, layouts


def _table():
    C, t = Case, []
    B, BX = "fk_kf_batch_filter_f64", "fk_kf_batch_filter_ex_f64"
    # KF forward: (4,2) kf_fast, (5,3) general, (9,3) three lanes, (12,3) and (16,8) four lanes -- the several-lane kernels first
    for n, m, org in ((9, 3, "ml3"), (12, 3, "mlg"), (16, 8, "mlg"), (4, 2, "fast"), (5, 3, "general")):
        t.append(C(f"kf_batch-{org}-{n}-{m}", [B], kf_batch, dict(n=n, m=m)))
        t.append(C(f"kf_batch-{org}-{n}-{m}-mask", [B], kf_batch, dict(n=n, m=m, mask=True)))
    for n, m in ((4, 2), (5, 3), (12, 3)):
        t.append(C(f"kf_batch-{n}-{m}-control-mask", [B], kf_batch, dict(n=n, m=m, mask=True, nu=2)))
    t.append(C("kf_batch-9-3-one_lane", [B], kf_batch, dict(n=9, m=3), {"FK_NO_ML": "1", "FK_ML9": "m"}))
    t.append(C("kf_batch-6-3-general", [B], kf_batch, dict(n=6, m=3, mask=True), {"FK_NO_FAST": "1"}))
    t.append(C("kf_batch-4-2-interleaved", [B], kf_batch, dict(n=4, m=2, inter=True)))
    t.append(C("kf_batch-6-3-interleaved-mask", [B], kf_batch, dict(n=6, m=3, inter=True, mask=True)))
    t.append(C("kf_batch_ex-4-2-mask", [BX], kf_batch, dict(n=4, m=2, mask=True, ex=True)))
    t.append(C("kf_batch_ex-9-3", [BX], kf_batch, dict(n=9, m=3, ex=True)))
    t.append(C("kf_batch_ex-12-3", [BX], kf_batch, dict(n=12, m=3, ex=True)))
    t.append(C("kf_batch_ex-5-3-control", [BX], kf_batch, dict(n=5, m=3, nu=2, ex=True)))
    for n, m in ((4, 2), (9, 3), (12, 3)):
        t.append(C(f"kf_predict-{n}-{m}", ["fk_kf_predict_f64"], kf_predict, dict(n=n, m=m, nu=2 if n == 4 else 0)))
        t.append(C(f"kf_update-{n}-{m}", ["fk_kf_update_f64"], kf_update, dict(n=n, m=m, mask=n == 9)))
    for g in ("S_ONLY", "SI_GIVEN"):
        t.append(C(f"kf_update-6-3-{g}", ["fk_kf_update_f64"], kf_update, dict(n=6, m=3, given=g)))
    # RTS: one, three (element-major) / four (NumPy order), four and eight lanes
    for n in (6, 9, 12, 15):
        t.append(C(f"kf_rts-{n}", ["fk_kf_rts_f64"], kf_rts, dict(n=n)))
    for g in ("PP_ONLY", "PPINV_GIVEN"):
        t.append(C(f"kf_rts-6-{g}", ["fk_kf_rts_f64"], kf_rts, dict(n=6, given=g)))
    for n, m in ((4, 2), (9, 3)):
        t.append(C(f"fls-{n}-{m}", ["fk_fls_batch_f64"], fls_batch, dict(n=n, m=m)))
    t.append(C("fls-4-2-chained-control", ["fk_fls_batch_f64"], fls_batch, dict(n=4, m=2, k0=4, nu=1)))
    for name, fn in (("srkf", srkf), ("info", info)):
        for n, m in ((4, 2), (9, 3)):
            t.append(C(f"{name}_batch-{n}-{m}", [f"fk_{name}_batch_f64"], fn, dict(n=n, m=m, what="batch", mask=n == 4, nu=2 if n == 9 else 0)))
            t.append(C(f"{name}_predict-{n}-{m}", [f"fk_{name}_predict_f64"], fn, dict(n=n, m=m, what="predict", nu=2 if n == 4 else 0)))
            t.append(C(f"{name}_update-{n}-{m}", [f"fk_{name}_update_f64"], fn, dict(n=n, m=m, what="update", mask=n == 9)))
    for n, m in ((6, 3), (9, 4)):
        for what in ("sigma_points", "transform", "update"):
            t.append(C(f"ckf_{what}-{n}-{m}", [f"fk_ckf_{what}_f64"], ckf_block, dict(n=n, m=m, what=what)))
        for what in ("batch", "predict", "update"):
            t.append(C(f"ckf_linear_{what}-{n}-{m}", [f"fk_ckf_linear_{what}_f64"], ckf_linear, dict(n=n, m=m, what=what, mask=n == 6)))
    for n, m in ((4, 2), (9, 4)):
        for pt in (False, True):
            tag = "per_track" if pt else "shared"
            t.append(C(f"ekf_predict-{n}-{m}-{tag}", ["fk_ekf_predict_f64"], ekf, dict(n=n, m=m, what="predict", per_track=pt, nu=2 if pt else 0)))
            t.append(C(f"ekf_update-{n}-{m}-{tag}", ["fk_ekf_update_f64"], ekf, dict(n=n, m=m, what="update", per_track=pt, mask=pt)))
            t.append(C(f"ekf_step-{n}-{m}-{tag}", ["fk_ekf_step_f64"], ekf, dict(n=n, m=m, what="step", per_track=pt, mask=not pt, nu=0 if pt else 2)))
    for n, m in ((4, 2), (9, 4)):
        t.append(C(f"enkf_predict-{n}-{m}", ["fk_enkf_predict_f64"], enkf, dict(n=n, m=m, what="predict", factor=n == 9), sizes=MEMBERS))
        t.append(C(f"enkf_update-{n}-{m}", ["fk_enkf_update_f64"], enkf, dict(n=n, m=m, what="update", factor=n == 4, sigmas_h=n == 9), sizes=MEMBERS))
        t.append(C(f"enkf_bank_predict-{n}-{m}", ["fk_enkf_bank_predict_f64"], enkf,
                   dict(n=n, m=m, what="predict", bank=5, per_track=n == 9, factor=n == 4), sizes=MEMBERS))
        t.append(C(f"enkf_bank_update-{n}-{m}", ["fk_enkf_bank_update_f64"], enkf,
                   dict(n=n, m=m, what="update", bank=5, per_track=n == 4, mask=True, sigmas_h=n == 9), sizes=MEMBERS))
    ut = dict(sigma_points="fk_ut_sigma_points_f64", transform="fk_ut_transform_f64", cross_variance="fk_ut_cross_variance_f64",
              linear_map="fk_ut_linear_map_f64", correct="fk_ukf_correct_f64", rts_correct="fk_ukf_rts_correct_f64")
    for n, m in ((6, 3), (9, 4)):
        for what, name in ut.items():
            t.append(C(f"ut_{what}-{n}-{m}", [name], ut_block, dict(n=n, m=m, what=what)))
    # fused UKF: (6,3) paired, element-major, even N takes the 16-byte pair stores at phase 0 and the plain kernel where means /
    # covs are only 8-byte aligned (ukf_sp_ok, csrc/ukf_kernels.hip:284); (12,3) four lanes, (16,8) eight lanes
    for n, m in ((6, 3), (12, 3), (16, 8)):
        t.append(C(f"ukf_batch-{n}-{m}", ["fk_ukf_linear_batch_f64"], ukf_fused, dict(n=n, m=m, what="batch", mask=n == 12)))
        t.append(C(f"ukf_rts-{n}", ["fk_ukf_linear_rts_f64"], ukf_fused, dict(n=n, m=m, what="rts")))
    t.append(C("ukf_batch-6-3-mask-index_order", ["fk_ukf_linear_batch_f64"], ukf_fused, dict(n=6, m=3, what="batch", mask=True, paired=False)))
    for n, m in ((4, 2), (9, 3)):
        t.append(C(f"steadystate-{n}-{m}", ["fk_kf_steadystate_f64"], steadystate, dict(n=n, m=m, per_track=n == 9, mask=n == 4, nu=2 if n == 4 else 0)))
        t.append(C(f"update_correlated-{n}-{m}", ["fk_kf_update_correlated_f64"], update_correlated, dict(n=n, m=m, per_track=n == 4, mask=n == 9)))
    X = "fk_imm_batch_ex_f64"
    for n, m, nm in ((4, 2, 3), (9, 4, 4), (12, 3, 2)):
        t.append(C(f"imm-{n}-{m}x{nm}", [X], imm, dict(n=n, m=m, nm=nm)))
    t.append(C("mmae-4-2x3", [X], imm, dict(n=4, m=2, nm=3, mmae=True)))
    t.append(C("imm-4-2x3-missing-control", [X], imm, dict(n=4, m=2, nm=3, masked=True, nu=1)))
    t.append(C("imm-9-4x4-missing", [X], imm, dict(n=9, m=4, nm=4, masked=True)))
    t.append(C("imm_plain-4-2x3", ["fk_imm_batch_f64"], imm, dict(n=4, m=2, nm=3, plain=True)))
    rs_names = dict(systematic="fk_resample_systematic_f64", stratified="fk_resample_stratified_f64",
                    multinomial="fk_resample_multinomial_f64", residual_fill="fk_resample_residual_fill_f64",
                    residual_draw="fk_resample_residual_draw_f64", cumsum="fk_cumsum_exact_f64")
    for what, name in rs_names.items():
        t.append(C(f"resample_{what}", [name], resample, dict(what=what), sizes=NPS, layouts=("-",)))
    for what in ("systematic", "stratified"):          # the two kernels these sizes do not reach by themselves
        for path in ("local", "onepass"):
            t.append(C(f"resample_{what}-{path}", [rs_names[what]], resample, dict(what=what), {"FK_RESAMPLE_PATH": path},
                       sizes=NPS, layouts=("-",)))
    for d in (3, 4):
        t.append(C(f"gather_mean-d{d}", ["fk_resample_gather_mean_f64"], gather_mean, dict(d=d), sizes=NPS, layouts=("-",)))
    return t


TABLE = _table()
# the entry points that take no device array: nothing to carve
NOT_APPLICABLE = {}
# one test per case and layout; its sizes and the five phases run inside it (a failure names the size and the phase)
PARAMS = [pytest.param(c, L, id="%s-%s" % (c.id, L)) for c in TABLE for L in c.layouts]


def _switches(monkeypatch, case):
    """no routing switch set, whatever the caller's shell holds; a case sets its own, per call"""
    for k in [k for k in os.environ if k.startswith("FK_")]:
        monkeypatch.delenv(k, raising=False)
    for k, v in case.env.items():
        monkeypatch.setenv(k, v)


def _run(case, A, N, L, ar=None):
    """-> [(name, bytes)] of the outputs, the status words checked"""
    import torch
    import zlib
    rs = np.random.RandomState(zlib.crc32(case.id.encode()) % 100000 + N)
    call = case.fn(A, rs, N, L, **case.kw)
    if ar is not None:
        ar.snapshot()
    call()                                                   # (raises unless the return code is FK_OK)
    torch.cuda.synchronize()
    for name, _, t in A.views():
        if name == "status":
            assert not t.any(), (case.id, L, N, t.cpu().numpy()[t.cpu().numpy() != 0][:8])
    return AR.outputs(A)


def _gather_mean_bar(case, A, got):
    """the d = 4 gather where the phase changes the kernel: tests/test_gpu_resample.py::test_gather_mean_vs_numpy's bar, against
    the longdouble mean of the gathered records"""
    v = {name: t.cpu().numpy() for name, _, t in A.views()}
    ref = np.stack([v["particles"][f][v["idx"][f]].astype(np.longdouble).mean(axis=0) for f in range(FN)]).astype(float)
    assert np.allclose(v["mean"], ref, rtol=1e-11, atol=1e-13), (case.id, np.abs(v["mean"] - ref).max())


def _one_phase(case, L, N, phase, base, need, dev):
    """the call with every argument in an arena at `phase` -> the findings (strings; none: the phase holds)"""
    ar = AR.Arena(dev, need)
    A = AR.ArenaAlloc(ar, phase)
    what = "%s %s N=%d phase %s" % (case.id, L, N, phase)
    try:
        got = _run(case, A, N, L, ar)
        ar.check(what)
    except AssertionError as e:
        return ["%s: %s" % (what, e)]
    ptrs = {name: t.data_ptr() for name, _, t in A.views()}
    assert [n for n, _ in got] == [n for n, _ in base]
    found = []
    for (name, g), (_, b) in zip(got, base):
        if np.array_equal(g, b) or name == "workspace":      # (scratch: "contents need not survive between calls")
            continue
        if case.fn is gather_mean and case.kw["d"] == 4 and name == "mean" and ptrs["particles"] % 16 != 0:
            _gather_mean_bar(case, A, got)                   # csrc/resample_kernels.hip:756: another kernel, another order of the sums
            continue
        found.append("%s: output %r differs from the ordinary-allocation run in %d byte(s), the first at byte %d (pointer %% 512 = %d)"
                     % (what, name, int((g != b).sum()), int(np.argmax(g != b)), ptrs[name] % 512))
    return found


@pytest.mark.gpu
@pytest.mark.parametrize("case,L", PARAMS)
def test_entry_point_in_the_arena(case, L, monkeypatch):
    """every size of the case, at every phase; a launch error (anything but an AssertionError) ends the test at once"""
    from filterpy_amd import _engine as E
    dev = E.require_gpu()
    _switches(monkeypatch, case)
    found = []
    for N in case.sizes:
        plain = AR.PlainAlloc(dev)
        base = _run(case, plain, N, L)
        for phase in AR.PHASES:
            found += _one_phase(case, L, N, phase, base, plain.need, dev)
    assert not found, "%d finding(s):\n%s" % (len(found), "\n".join(found))


# -------------------------------------------------------------------------------------------- held to the truth, not to itself
def _stiff(family):
    """(the precision test of the family, its arguments with `layout` and `monkeypatch` left open): one stiff case per *_hp
    module, at dims those modules cache cheaply"""
    import importlib
    mod, fn, args = {
        "kf_hp": ("test_gpu_kf_precision", "test_forward_pass_vs_extended_precision",
                  lambda L, mp: ("kf_fast packed", 6, 3, {}, False, "stiff", L, mp)),
        "kf_hp-three_lanes": ("test_gpu_kf_precision", "test_forward_pass_vs_extended_precision",
                              lambda L, mp: ("kf_ml three lanes", 9, 3, {}, False, "stiff", L, mp)),
        "rts_hp": ("test_gpu_rts_precision", "test_smoother_vs_extended_precision",
                   lambda L, mp: ("one lane exact", 6, 3, {}, L, "stiff", mp)),
        "rts_hp-9": ("test_gpu_rts_precision", "test_smoother_vs_extended_precision",
                     lambda L, mp: ("three lanes" if L == "soa" else "four lanes", 9, 3, {}, L, "stiff", mp)),
        "imm_hp": ("test_gpu_imm_precision", "test_bank_vs_extended_precision",
                   lambda L, mp: ("imm_kernels", "imm", 6, 3, 3, False, "stiff", L)),
        "ukf_hp": ("test_gpu_ukf_precision", "test_fused_filter_and_smoother_vs_extended_precision",
                   lambda L, mp: (6, 3, True, True, "stiff", L)),
        "ckf_hp": ("test_gpu_ckf_precision", "test_offset_ill_scaled_models_vs_extended_precision", lambda L, mp: (L, (6, 3))),
        "ekf_hp": ("test_gpu_ekf_precision", "test_ill_scaled_bilinear_models_vs_extended_precision", lambda L, mp: (L, (6, 3))),
        "enkf_hp": ("test_gpu_enkf_precision", "test_chained_run_meets_the_bar", lambda L, mp: (mp, "stiff", 6, 3, 65, False, L)),
        "srkf_hp": ("test_gpu_srkf_precision", "test_ill_conditioned_vs_extended_precision", lambda L, mp: (L, (6, 3))),
        "info_hp": ("test_gpu_info_precision", "test_uninformative_prior_vs_extended_precision", lambda L, mp: (L, (6, 3))),
    }[family]
    return getattr(importlib.import_module(mod), fn), args


STIFF = ("kf_hp", "kf_hp-three_lanes", "rts_hp", "rts_hp-9", "imm_hp", "ukf_hp", "ckf_hp", "ekf_hp", "enkf_hp", "srkf_hp", "info_hp")


@pytest.mark.gpu
@pytest.mark.parametrize("layout", BOTH)
@pytest.mark.parametrize("family", STIFF)
def test_stiff_case_of_the_family_inside_a_mixed_arena(family, layout, monkeypatch):
    """The family's own precision test -- its inputs, its longdouble truth, its bar and its reference error, unchanged -- with
    every device array it and the package's classes allocate carved from an arena at the "mixed" phase (arena.allocations_in), and
    the guards of all of them intact afterwards.  Every pointer _engine hands to the library lies inside the arena."""
    from filterpy_amd import _engine as E
    for k in [k for k in os.environ if k.startswith("FK_")]:
        monkeypatch.delenv(k, raising=False)
    fn, args = _stiff(family)
    ar = AR.Arena(E.require_gpu(), 1 << 30)
    with AR.allocations_in(ar, "mixed", E) as outside:
        fn(*args(layout, monkeypatch))
    assert len(ar.views) >= 4, len(ar.views)
    assert not outside, ("arrays that reached the library from outside the arena", outside[:8])
    ar.check_guards("%s %s" % (family, layout))


@pytest.mark.gpu
@pytest.mark.parametrize("lag", [2, 8])
def test_stiff_fixed_lag_smoother_inside_a_mixed_arena(lag, monkeypatch):
    """fls_hp: the first fast instantiation of csrc/fk_dims_fls.def with that lag, through test_gpu_fls_precision's own test"""
    import test_gpu_fls_precision as TF
    from filterpy_amd import _engine as E
    e = next((e for e in TF.ENTRIES if e[2] >= lag), TF.ENTRIES[0])
    ar = AR.Arena(E.require_gpu(), 1 << 30)
    with AR.allocations_in(ar, "mixed", E) as outside:
        TF.test_fast_instantiation_vs_hp(e, monkeypatch)
    assert len(ar.views) >= 4 and not outside, (len(ar.views), outside[:8])
    ar.check_guards("fls_hp %s" % (e,))


@pytest.mark.gpu
@pytest.mark.parametrize("what", ["systematic", "stratified"])
@pytest.mark.parametrize("Np", NPS)
def test_resamplers_against_the_merge_loop_at_the_mixed_phase(what, Np):
    """the reference of tests/test_gpu_resample.py: oracle/resample_oracle.py's merge loop, bit for bit"""
    from filterpy_amd import _engine as E
    from oracle import resample_oracle as ro
    case = next(c for c in TABLE if c.id == "resample_" + what)
    plain = AR.PlainAlloc(E.require_gpu())
    _run(case, plain, Np, "-")
    ar = AR.Arena(E.require_gpu(), plain.need)
    A = AR.ArenaAlloc(ar, "mixed")
    _run(case, A, Np, "-", ar)
    ar.check(what)
    v = {name: t.cpu().numpy() for name, _, t in A.views()}
    for f in range(FN):
        ref, over = (ro.systematic_c(v["w"][f], float(v["u"][f])) if what == "systematic" else ro.stratified_c(v["w"][f], v["u"][f]))
        assert over == 0 and np.array_equal(v["idx"][f], ref), (what, Np, f)


# ---------------------------------------------------------------------------------------------------------------- coverage
def test_every_entry_point_of_the_header_is_listed():
    """(no GPU needed: it reads the header and the table)"""
    with open(os.path.join(ROOT, "include", "filterhip.h")) as fh:
        names = set(re.findall(r"^\s*int\s+(fk_\w+_f64)\s*\(", fh.read(), re.M))
    from filterpy_amd import _abi
    assert names == {k for k in _abi.SIGNATURES if k.endswith("_f64")}, "the pattern above no longer finds every declaration"
    covered = {e for c in TABLE for e in c.entries}
    assert not (covered & set(NOT_APPLICABLE))
    missing = names - covered - set(NOT_APPLICABLE)
    assert not missing, "entry points of include/filterhip.h without a case in tests/test_gpu_arena.py: %s" % sorted(missing)
    assert not (covered | set(NOT_APPLICABLE)) - names, "listed, but not in the header: %s" % sorted((covered | set(NOT_APPLICABLE)) - names)
