"""tests/srkf_port.py in np.longdouble (80-bit on x86-64): the same Householder sequence in LAPACK's convention, with a
triangular inverse for S1_2 (numpy's linear algebra does not take longdouble) -- the truth the precision tests measure the GPU
and the float64 port against."""
import numpy as np

LD = np.longdouble


def ld(a):
    return np.asarray(a, dtype=LD)


def qr_r(A):
    A = ld(A).copy()
    M, N = A.shape
    for j in range(min(M, N)):
        if M - j <= 1:
            continue
        alpha, x = A[j, j], A[j + 1:, j]
        if not np.any(x != 0):
            continue
        beta = -np.copysign(np.sqrt(alpha * alpha + np.sum(x * x)), alpha)
        tau = (beta - alpha) / beta
        v = x / (alpha - beta)
        A[j, j] = beta
        A[j + 1:, j] = 0
        w = A[j, j + 1:] + v @ A[j + 1:, j + 1:]
        A[j, j + 1:] -= tau * w
        A[j + 1:, j + 1:] -= tau * np.outer(v, w)
    return np.triu(A)


def tri_inv(S):
    """inverse of a lower-triangular matrix by forward substitution"""
    m = S.shape[0]
    SI = np.zeros_like(S)
    for i in range(m):
        SI[i, i] = 1 / S[i, i]
        for j in range(i):
            SI[i, j] = -(S[i, j:i] @ SI[j:i, j]) * SI[i, i]
    return SI


def batch(x0, L0, zs, F, Q12, H, R12):
    """means, sqrt_covs (posterior) and means_p, sqrt_covs_p of one track, predict first, in longdouble"""
    F, Q12, H, R12 = ld(F), ld(Q12), ld(H), ld(R12)
    x, L = ld(x0).copy(), ld(L0).copy()
    m, n = H.shape
    T = len(zs)
    out = [np.zeros((T, n), LD), np.zeros((T, n, n), LD), np.zeros((T, n), LD), np.zeros((T, n, n), LD)]
    for t in range(T):
        x = F @ x
        L = qr_r(np.hstack([F @ L, Q12]).T)[:n, :n].T.copy()
        out[2][t], out[3][t] = x, L
        M = np.zeros((m + n, m + n), LD)
        M[:m, :m], M[m:, :m], M[m:, m:] = R12.T, (H @ L).T, L.T
        r = qr_r(M)
        K = r[:m, m:].T @ tri_inv(r[:m, :m].T.copy())
        x = x + K @ (ld(zs[t]) - H @ x)
        L = r[m:, m:].T.copy()
        out[0][t], out[1][t] = x, L
    return out
