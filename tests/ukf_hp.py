"""The reference's linear-model UKF (fx = F x, hx = H x) for ONE track in np.longdouble (80-bit on x86-64), written from the
algorithm: Merwe / Julier weights (sigma_points.py:180-192, :358-372), sigma points from the upper Cholesky factor of
(n + lambda) P with its ROWS as offsets (sigma_points.py:153-177), the unscented transform (unscented_transform.py:101-126), the
cross variance (UKF.py:483-497), predict / update (UKF.py:400-411, 462-481), batch_filter with missing measurements
(UKF.py:524-632) and the RTS smoother with its gains (UKF.py:634-739).  inv(S) comes from a longdouble Cholesky factorisation
(numpy's linear algebra does not take longdouble).  A non-positive pivot raises numpy.linalg.LinAlgError.

This is the truth tests/test_gpu_ukf_precision.py and tests/test_host_ukf_hp.py measure the kernels and the float64 oracle
(oracle/ukf_oracle.py) against; models() builds the model families both files run."""
import numpy as np

LD = np.longdouble


def ld(a):
    return np.asarray(a, dtype=LD)


# ------------------------------------------------------------------------------------------------------------ weights
def merwe_weights(n, alpha, beta, kappa):
    """Wm, Wc in longdouble from the float64 alpha / beta / kappa"""
    alpha, beta, kappa = LD(alpha), LD(beta), LD(kappa)
    lam = alpha * alpha * (n + kappa) - n
    c = LD(0.5) / (n + lam)
    Wm, Wc = np.full(2 * n + 1, c, dtype=LD), np.full(2 * n + 1, c, dtype=LD)
    Wm[0] = lam / (n + lam)
    Wc[0] = lam / (n + lam) + (1 - alpha * alpha + beta)
    return Wm, Wc


def julier_weights(n, kappa):
    kappa = LD(kappa)
    W = np.full(2 * n + 1, LD(0.5) / (n + kappa), dtype=LD)
    W[0] = kappa / (n + kappa)
    return W, W.copy()


def merwe_scale(n, alpha, kappa):
    """n + lambda = alpha^2 (n + kappa)"""
    return LD(alpha) * LD(alpha) * (n + LD(kappa))


def kernel_scale(n, alpha, kappa):
    """the float64 lambda + n the PACKAGE hands its kernels (MerweScaledSigmaPoints.scale: lambda rounded first, like the
    reference's sigma_points.py:165-168, so that it is the very number the float64 weights divide by)"""
    lam = alpha ** 2 * (n + kappa) - n
    return lam + n


# ------------------------------------------------------------------------------------------------------ factorisations
def chol_upper(A):
    """U upper triangular with U' U = A (scipy.linalg.cholesky's default); a pivot that is not positive raises"""
    A = ld(A)
    n = A.shape[0]
    U = np.zeros((n, n), dtype=LD)
    for j in range(n):
        d = A[j, j] - U[:j, j] @ U[:j, j]
        if not d > 0:
            raise np.linalg.LinAlgError(f"pivot {j} is not positive: {d!r}")
        U[j, j] = np.sqrt(d)
        if j + 1 < n:
            U[j, j + 1:] = (A[j, j + 1:] - U[:j, j] @ U[:j, j + 1:]) / U[j, j]
    return U


def tri_inv_upper(U):
    """inverse of an upper-triangular matrix by back substitution"""
    n = U.shape[0]
    V = np.zeros_like(U)
    for j in range(n):
        V[j, j] = 1 / U[j, j]
        for i in range(j - 1, -1, -1):
            V[i, j] = -(U[i, i + 1:j + 1] @ V[i + 1:j + 1, j]) / U[i, i]
    return V


def spd_inv(S):
    """inv(S) = inv(U) inv(U)' from S = U' U"""
    V = tri_inv_upper(chol_upper(S))
    return V @ V.T


# --------------------------------------------------------------------------------------------------- the single blocks
def sigma_points(x, P, scale):
    """[x, x + U[k], x - U[k]] with U = chol_upper(scale P): the reference's subtract(x, -U[k]), subtract(x, U[k])"""
    x, P = ld(x), ld(P)
    n = x.size
    U = chol_upper(LD(scale) * P)
    s = np.empty((2 * n + 1, n), dtype=LD)
    s[0] = x
    s[1:n + 1] = x + U
    s[n + 1:] = x - U
    return s


def transform(sigmas, Wm, Wc, noise=None):
    sigmas, Wm, Wc = ld(sigmas), ld(Wm), ld(Wc)
    x = Wm @ sigmas
    y = sigmas - x
    P = (y.T * Wc) @ y
    if noise is not None:
        P = P + ld(noise)
    return x, P


def cross_variance(x, z, sigmas_f, sigmas_h, Wc):
    dx, dz = ld(sigmas_f) - ld(x), ld(sigmas_h) - ld(z)
    return (dx.T * ld(Wc)) @ dz


def correct(Pxz, zp, S, z, x, P):
    """K = Pxz inv(S); x + K (z - zp); P - K (S K')   ->  x, P, K"""
    Pxz, zp, S, z, x, P = map(ld, (Pxz, zp, S, z, x, P))
    K = Pxz @ spd_inv(S)
    return x + K @ (z - zp), P - K @ (S @ K.T), K


def rts_correct(Pxb, xb, Pb, xn, Pn, x, P):
    """K = Pxb inv(Pb); x + K (xn - xb); P + K (Pn - Pb) K'   ->  x, P, K"""
    Pxb, xb, Pb, xn, Pn, x, P = map(ld, (Pxb, xb, Pb, xn, Pn, x, P))
    K = Pxb @ spd_inv(Pb)
    return x + K @ (xn - xb), P + (K @ (Pn - Pb)) @ K.T, K


# ------------------------------------------------------------------------------------------------- filter and smoother
def predict(x, P, F, Q, Wm, Wc, scale):
    sf = sigma_points(x, P, scale) @ F.T
    x, P = transform(sf, Wm, Wc, Q)
    return x, P, sigma_points(x, P, scale)                     # the points regenerated from the prior (UKF.py:407)


def update(x, P, sigmas_f, z, H, R, Wm, Wc):
    sh = sigmas_f @ H.T
    zp, S = transform(sh, Wm, Wc, R)
    Pxz = cross_variance(x, zp, sigmas_f, sh, Wc)
    return correct(Pxz, zp, S, z, x, P)[:2]


def batch_filter(x0, P0, zs, F, H, Q, R, alpha, beta, kappa, weights=None):
    """means, covs [T] of one track, predict first; a z that is None skips the update"""
    F, H, Q, R = map(ld, (F, H, Q, R))
    x, P = ld(x0).copy(), ld(P0).copy()
    n = x.size
    Wm, Wc = merwe_weights(n, alpha, beta, kappa) if weights is None else map(ld, weights)
    scale = merwe_scale(n, alpha, kappa)
    means, covs = np.zeros((len(zs), n), LD), np.zeros((len(zs), n, n), LD)
    for t, z in enumerate(zs):
        x, P, sf = predict(x, P, F, Q, Wm, Wc, scale)
        if z is not None:
            x, P = update(x, P, sf, ld(z), H, R, Wm, Wc)
        means[t], covs[t] = x, P
    return means, covs


def rts_smoother(Xs, Ps, F, Q, alpha, beta, kappa):
    """xs, ps, Ks of one track (UKF.py:714-739); the last step is the filter's own, its gain zero"""
    F, Q, Xs, Ps = map(ld, (F, Q, Xs, Ps))
    T, n = Xs.shape
    Wm, Wc = merwe_weights(n, alpha, beta, kappa)
    scale = merwe_scale(n, alpha, kappa)
    xs, ps, Ks = Xs.copy(), Ps.copy(), np.zeros((T, n, n), LD)
    for k in range(T - 2, -1, -1):
        s = sigma_points(xs[k], ps[k], scale)
        sf = s @ F.T
        xb, Pb = transform(sf, Wm, Wc, Q)
        Pxb = cross_variance(Xs[k], xb, s, sf, Wc)
        xs[k], ps[k], Ks[k] = rts_correct(Pxb, xb, Pb, xs[k + 1], ps[k + 1], xs[k], ps[k])
    return xs, ps, Ks


def err(a, hp):
    """worst normwise relative error over the leading axis (steps, or tracks of a block), measured in longdouble"""
    hp = ld(hp)
    d = np.abs(ld(a) - hp).reshape(len(hp), -1).max(axis=1)
    return float(np.max(d / np.maximum(np.abs(hp).reshape(len(hp), -1).max(axis=1), 1e-300)))


# ------------------------------------------------------------------------------------------------------ the model families
FAMILIES = ("benign", "stiff", "stiff_small_weights", "alpha_1e-3")
N_BANK, T_RUN, T_MISSING = 150, 16, 8
# The smoother runs on the filter's steps SMOOTH_FROM .. T-1.  The first steps are left out of its window on every model: with
# P0 = 1e6 I the posterior still carries 1e6 in the directions the measurements so far do not see (dim_x / dim_z steps: 4 at
# (12,3), the largest ratio used), the smoothed covariance of such a step is ~1e-4, and ps[k] += K (ps[k+1] - Pb) K' cancels nine
# or ten digits there in ANY float64 arithmetic -- the oracle's own ps[0] is wrong by 1e3 relative on the stiff model (by 1e0
# with P0 and R softened a decade each), so those steps would measure nothing.  From step 4 on the oracle's smoothed outputs are
# good to 1e-3 or better on every model and dim, and the window still holds the missing measurement.
SMOOTH_FROM = 4
FIXED_TRACKS = (0, 1, 15, 16, 63, 64, 143, 144, 149)


def _spd(rs, n, scale=1.0, batch=()):
    A = rs.randn(*batch, n, n)
    return scale * (A @ np.swapaxes(A, -1, -2) / n + 0.5 * np.eye(n))


def models(family, n, m, N=N_BANK, T=T_RUN):
    """One bank of N different tracks (own x0 and measurements; the benign families own P0 too), a fixed RandomState per
    (n, m); the measurement of step T_MISSING is missing on every track.  Returns a dict: F H Q R x0[N] P0[N] zs[T][N] mask[T]
    alpha beta kappa tracks (the 16 that are checked)."""
    rs = np.random.RandomState(100 * n + m)
    beta, kappa = 2.0, 3.0 - n
    if family in ("benign", "alpha_1e-3"):                      # the _bank models of tests/test_gpu_ukf_mlg.py
        alpha = .5 if family == "benign" else 1e-3
        F = np.eye(n) + 0.1 * rs.randn(n, n)
        F /= max(1.0, 1.05 * np.max(np.abs(np.linalg.eigvals(F))))
        H, Q, R = rs.randn(m, n), _spd(rs, n, 0.05), _spd(rs, m, 0.5)
        x0, P0 = rs.randn(N, n), _spd(rs, n, 2.0, (N,))
        zs = rs.randn(T, N, m)
    elif family in ("stiff", "stiff_small_weights"):
        p0, r, alpha = (1e6, 1e-4, .5) if family == "stiff" else (1e4, 1e-2, 1e-2)
        F = np.eye(n) + 0.5 * np.diag(np.ones(n - 1), 1) + 0.01 * rs.randn(n, n)
        H = rs.randn(m, n)
        Q = np.diag(10.0 ** rs.uniform(-6, -2, n))
        R = np.eye(m) * r
        x0, P0 = rs.randn(N, n), np.tile(np.eye(n) * p0, (N, 1, 1))
        zs = 10 * rs.randn(T, N, m)
    else:
        raise ValueError(family)
    mask = np.ones(T, dtype=np.uint8)
    mask[T_MISSING] = 0
    rest = np.setdiff1d(np.arange(N), FIXED_TRACKS)
    tracks = tuple(FIXED_TRACKS) + tuple(int(i) for i in np.sort(rs.choice(rest, 16 - len(FIXED_TRACKS), replace=False)))
    return dict(F=F, H=H, Q=Q, R=R, x0=x0, P0=P0, zs=zs, mask=mask, alpha=alpha, beta=beta, kappa=kappa, tracks=tracks,
                n=n, m=m, N=N, T=T)


_truth_cache = {}


def truth(family, n, m):
    """hp and float64-oracle filter + smoother outputs of the 16 checked tracks, computed once per (family, n, m) and shared:
    {"hp": [5 arrays [16][T]...], "oracle": the same} in the order mu, cov, xs, Ps, K.  The oracle must finish every track
    (a non-positive pivot raises) -- no track is ever left out."""
    key = (family, n, m)
    if key not in _truth_cache:
        import os
        import sys
        root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
        if root not in sys.path:
            sys.path.insert(0, root)
        from oracle import ukf_oracle
        M = models(family, n, m)
        F, H, Q, R, a, b, k = M["F"], M["H"], M["Q"], M["R"], M["alpha"], M["beta"], M["kappa"]
        hp, orc = [[] for _ in range(5)], [[] for _ in range(5)]
        for trk in M["tracks"]:
            zl = [M["zs"][t, trk] if M["mask"][t] else None for t in range(M["T"])]
            mu, cov = batch_filter(M["x0"][trk], M["P0"][trk], zl, F, H, Q, R, a, b, k)
            for lst, v in zip(hp, (mu, cov) + rts_smoother(mu[SMOOTH_FROM:], cov[SMOOTH_FROM:], F, Q, a, b, k)):
                lst.append(v)
            mu, cov = ukf_oracle.ukf_batch_filter(M["x0"][trk], M["P0"][trk], zl, lambda s, dt: F @ s, lambda s: H @ s, 1.0,
                                                  Q, R, a, b, k)
            for lst, v in zip(orc, (mu, cov) + ukf_oracle.ukf_rts_smoother(mu[SMOOTH_FROM:], cov[SMOOTH_FROM:], lambda s, dt: F @ s,
                                                                           1.0, Q, a, b, k)):
                lst.append(v)
        _truth_cache[key] = dict(model=M, hp=[np.array(v) for v in hp], oracle=[np.array(v) for v in orc])
    return _truth_cache[key]


OUTPUTS = ("mu", "cov", "xs", "Ps", "K")
FLOOR = 1e-13


def errors(got, hp):
    """[outputs][tracks] errors of `got` (a list of arrays [tracks][T]..., None where an output is not produced) against hp;
    the smoother's gain is compared without its last step (zero in both)"""
    out = np.full((len(got), len(hp[0])), np.nan)
    for j, g in enumerate(got):
        if g is None:
            continue
        cut = slice(None, -1) if OUTPUTS[j] == "K" else slice(None)
        for i in range(len(hp[j])):
            out[j, i] = err(np.asarray(g[i])[cut], hp[j][i][cut])
    return out


def check(label, eg, eo, margin, floor=FLOOR):
    """The bar, per output: every track's err(got, hp) <= max(margin * max_tracks err(oracle, hp), floor) and the median over
    tracks <= max(margin * median err(oracle, hp), floor).  Prints worst err/bar and the ratio of medians; returns the failures."""
    bad = []
    for j in range(len(eg)):
        if np.isnan(eg[j]).all():
            continue
        assert np.all(np.isfinite(eg[j])) and np.all(np.isfinite(eo[j])), (label, j)
        bar, mbar = max(margin * eo[j].max(), floor), max(margin * np.median(eo[j]), floor)
        print(label, OUTPUTS[j] if len(eg) == len(OUTPUTS) else j, "worst err/bar %.3f" % (eg[j].max() / bar),
              "median/bar %.3f" % (np.median(eg[j]) / mbar),
              "got/oracle medians %.2f" % (np.median(eg[j]) / max(np.median(eo[j]), 1e-300)), "oracle max %.2e" % eo[j].max())
        if eg[j].max() > bar or np.median(eg[j]) > mbar:
            bad.append((label, j, float(eg[j].max() / bar), float(np.median(eg[j]) / mbar)))
    return bad


# ------------------------------------------------------------------------------------------ the split blocks on stiff inputs
N_BLOCK = 65
BLOCK_DIMS = ((6, 3), (9, 4), (16, 8))


def _stiff_spd(rs, n, lo, hi, N):
    """N matrices U diag(10^U(lo, hi)) U' with U a random orthogonal basis; the extremes are pinned: condition 10^(hi - lo)"""
    out = np.empty((N, n, n))
    for i in range(N):
        U, _ = np.linalg.qr(rs.randn(n, n))
        d = 10.0 ** rs.uniform(lo, hi, n)
        d[0], d[-1] = 10.0 ** lo, 10.0 ** hi
        A = (U * d) @ U.T
        out[i] = (A + A.T) / 2
    return out


_block_cache = {}


def blocks(n, m):
    """Inputs of the four split blocks on a bank of N_BLOCK tracks (covariances of condition 1e10, S of condition 1e8; alpha = 0.5,
    beta = 2, kappa = 3 - n) with the longdouble and the float64-oracle outputs of every track:
    {"in": {...}, "hp": {block: [arrays [N]...]}, "oracle": the same}.  Blocks and outputs:
    sigma (sigmas), transform (x, P), correct (x, P, K), rts_correct (x, P, K)."""
    if (n, m) in _block_cache:
        return _block_cache[(n, m)]
    import os
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if root not in sys.path:
        sys.path.insert(0, root)
    from oracle import ukf_oracle
    rs = np.random.RandomState(1000 * n + m)
    N, alpha, beta, kappa = N_BLOCK, .5, 2.0, 3.0 - n
    Wm, Wc = ukf_oracle.merwe_weights(n, alpha, beta, kappa)
    i = dict(alpha=alpha, beta=beta, kappa=kappa, Wm=Wm, Wc=Wc, scale=kernel_scale(n, alpha, kappa),
             x=rs.randn(N, n), P=_stiff_spd(rs, n, -4, 6, N), Q=np.diag(10.0 ** rs.uniform(-6, -2, n)),
             Pxz=rs.randn(N, n, m), zp=rs.randn(N, m), S=_stiff_spd(rs, m, -4, 4, N), z=rs.randn(N, m),
             Pxb=rs.randn(N, n, n), xb=rs.randn(N, n), Pb=_stiff_spd(rs, n, -4, 6, N), xn=rs.randn(N, n),
             Pn=_stiff_spd(rs, n, -4, 6, N))
    # the transform's input: the longdouble sigma points of (x, P), rounded to float64 -- the same numbers for everybody
    i["sigmas"] = np.array([sigma_points(i["x"][t], i["P"][t], LD(i["scale"])) for t in range(N)]).astype(np.float64)
    hp = dict(sigma=[[]], transform=[[], []], correct=[[], [], []], rts_correct=[[], [], []])
    orc = dict(sigma=[[]], transform=[[], []], correct=[[], [], []], rts_correct=[[], [], []])
    inv = np.linalg.inv
    for t in range(N):
        res = dict(sigma=(sigma_points(i["x"][t], i["P"][t], LD(i["scale"])),),
                   transform=transform(i["sigmas"][t], Wm, Wc, i["Q"]),
                   correct=correct(i["Pxz"][t], i["zp"][t], i["S"][t], i["z"][t], i["x"][t], i["P"][t]),
                   rts_correct=rts_correct(i["Pxb"][t], i["xb"][t], i["Pb"][t], i["xn"][t], i["Pn"][t], i["x"][t], i["P"][t]))
        for b, vals in res.items():
            for lst, v in zip(hp[b], vals):
                lst.append(v)
        K = np.dot(i["Pxz"][t], inv(i["S"][t]))                                  # UKF.py:470-481
        Kb = np.dot(i["Pxb"][t], inv(i["Pb"][t]))                                # UKF.py:732-737
        res = dict(sigma=(ukf_oracle.merwe_sigma_points(i["x"][t], i["P"][t], alpha, kappa),),
                   transform=ukf_oracle.unscented_transform(i["sigmas"][t], Wm, Wc, i["Q"]),
                   correct=(i["x"][t] + np.dot(K, i["z"][t] - i["zp"][t]), i["P"][t] - np.dot(K, np.dot(i["S"][t], K.T)), K),
                   rts_correct=(i["x"][t] + np.dot(Kb, i["xn"][t] - i["xb"][t]),
                                i["P"][t] + np.dot(Kb, i["Pn"][t] - i["Pb"][t]).dot(Kb.T), Kb))
        for b, vals in res.items():
            for lst, v in zip(orc[b], vals):
                lst.append(v)
    out = dict(hp={b: [np.array(v) for v in vs] for b, vs in hp.items()},
               oracle={b: [np.array(v) for v in vs] for b, vs in orc.items()})
    out["in"] = i
    _block_cache[(n, m)] = out
    return out


def block_errors(got, hp):
    """[outputs][tracks]: every track's normwise relative error of one block's outputs"""
    return np.array([[err(g[t][None], h[t][None]) for t in range(len(h))] for g, h in zip(got, hp)])
