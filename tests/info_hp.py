"""tests/info_port.py in np.longdouble (80-bit on x86-64): the same lines of information_filter.py:178-289, with a Gauss-Jordan
elimination with partial pivoting of its own for the inverse (numpy's linear algebra does not take longdouble) -- the truth
the precision tests measure the GPU and the float64 port against."""
import numpy as np

LD = np.longdouble


def ld(a):
    return np.asarray(a, dtype=LD)


def inv(A):
    """A^-1 by Gauss-Jordan elimination with partial pivoting, in longdouble"""
    A = ld(A).copy()
    n = A.shape[0]
    W = np.concatenate([A, np.eye(n, dtype=LD)], axis=1)
    for j in range(n):
        p = j + int(np.argmax(np.abs(W[j:, j])))
        if p != j:
            W[[j, p]] = W[[p, j]]
        W[j] = W[j] / W[j, j]
        for i in range(n):
            if i != j:
                W[i] = W[i] - W[i, j] * W[j]
    return W[:, n:].copy()


def batch(x0, Pi0, zs, F, Q, H, Ri):
    """means, P_invs (posterior) and means_p, P_invs_p of one track, predict first, in longdouble"""
    F, Q, H, Ri = ld(F), ld(Q), ld(H), ld(Ri)
    x, Pi = ld(x0).copy(), ld(Pi0).copy()
    n = len(x)
    T = len(zs)
    F_inv = inv(F)
    out = [np.zeros((T, n), LD), np.zeros((T, n, n), LD), np.zeros((T, n), LD), np.zeros((T, n, n), LD)]
    for t in range(T):
        A = F_inv.T @ Pi @ F_inv
        x = F @ x
        Pi = inv(inv(A) + Q)
        out[2][t], out[3][t] = x, Pi
        y = ld(zs[t]) - H @ x
        S = Pi + H.T @ Ri @ H
        K = inv(S) @ H.T @ Ri
        x = x + K @ y
        Pi = S
        out[0][t], out[1][t] = x, Pi
    return out
