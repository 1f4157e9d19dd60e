"""NumPy restatement of the fixed-gain polynomial filters (filterpy.gh, filterpy.memory, filterpy.leastsq): the three operation
orders of filterpy_amd/csrc/fk_poly.hpp and the host scalars each class hands to fk_poly_run.  NumPy evaluates one IEEE
operation per operator and never contracts, so the parentheses below ARE the arithmetic; the bar everywhere is bit identity
(np.array_equal on float64).  Tracks are the last axis: a state is (order + 1, N), measurements are (T, N)."""
import os

import numpy as np

FORM_A, FORM_B, FORM_C = 0, 1, 2
COMBOS = [(0, FORM_A), (1, FORM_A), (2, FORM_A), (1, FORM_B), (2, FORM_B), (1, FORM_C), (2, FORM_C)]
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "poly_filters.npz")


def step(order, form, s, z, dt, T2, c, g):
    """one step: s (order + 1, N) -> (s', pred, y).  g: the step's gains (g[0..order] are read)"""
    s = np.asarray(s, dtype=np.float64)
    out = np.empty_like(s)
    if form == FORM_C:
        x0, x1 = s[0], s[1]
        if order == 1:
            y = (z - x0) - dt * x1
            pred = x0 + dt * x1
            out[0] = x0 + ((g[0] * y) + x1 * dt)
            out[1] = x1 + (g[1] * y)
        else:
            x2 = s[2]
            y = ((z - x0) - dt * x1) - c * x2
            pred = (x0 + dt * x1) + c * x2
            out[0] = x0 + (((g[0] * y) + x1 * dt) + c * x2)
            out[1] = x1 + ((g[1] * y) + x2 * dt)
            out[2] = x2 + g[2] * y
        return out, pred, y
    xp = s[0]
    if order >= 1:
        xp = s[0] + s[1] * dt
        dxp = s[1]
    if order == 2:
        xp = xp + (0.5 * s[2]) * T2
        dxp = s[1] + s[2] * dt
    y = z - xp
    out[0] = xp + g[0] * y
    if order >= 1:
        out[1] = dxp + g[1] * y if form == FORM_A else dxp + (g[1] * y) / dt
    if order == 2:
        out[2] = s[2] + g[2] * y if form == FORM_A else s[2] + (g[2] * y) / T2
    return out, xp, y


def run(order, form, x0, zs, dt, T2=0.0, c=0.0, g=(0.0, 0.0, 0.0), gains=None):
    """T steps.  x0 (order + 1, N), zs (T, N); gains: None or a (T, order + 1) table -> xs (T, order + 1, N), pred, y (T, N)"""
    s = np.array(x0, dtype=np.float64)
    zs = np.asarray(zs, dtype=np.float64)
    T = zs.shape[0]
    xs, pred, y = np.empty((T,) + s.shape), np.empty(zs.shape), np.empty(zs.shape)
    for t in range(T):
        s, pred[t], y[t] = step(order, form, s, zs[t], np.float64(dt), np.float64(T2), np.float64(c),
                                [np.float64(v) for v in (g if gains is None else gains[t])])
        xs[t] = s
    return xs, pred, y


# ------------------------------------------------------------------------------------------------ each class's host scalars
# -> dict(form=, dt=, T2=, c=, g=(g0, g1, g2)), with the reference's own expressions on Python numbers
def gh_update(g, h, dt):
    return dict(form=FORM_B, dt=dt, T2=0.0, c=0.0, g=(g, h, 0.0))


def gh_batch(g, h, dt):
    return dict(form=FORM_A, dt=dt, T2=0.0, c=0.0, g=(g, h / dt, 0.0))


def ghk_update(g, h, k, dt):
    return dict(form=FORM_B, dt=dt, T2=dt**2, c=0.0, g=(g, h, 2 * k))


def gh_order(order, g, h, k, dt):
    if order == 0:
        return dict(form=FORM_A, dt=dt, T2=0.0, c=0.0, g=(g, 0.0, 0.0))
    if order == 1:
        return gh_update(g, h, dt)
    return dict(form=FORM_B, dt=dt, T2=dt**2., c=0.0, g=(g, h, 2 * k))


def fading(order, beta, dt):
    if order == 0:
        return dict(form=FORM_A, dt=dt, T2=0.0, c=0.0, g=(1 - beta, 0.0, 0.0))
    if order == 1:
        G = 1 - beta**2
        H = (1 - beta)**2
        return dict(form=FORM_A, dt=dt, T2=0.0, c=0.0, g=(G, H / dt, 0.0))
    G = 1 - beta**3
    H = 1.5 * (1 + beta) * (1 - beta)**2
    K = 0.5 * (1 - beta)**3
    return dict(form=FORM_A, dt=dt, T2=dt**2., c=0.0, g=(G, H / dt, 2 * K / (dt**2)))


def lsq_gains(order, n, dt):
    """LeastSquaresFilter's K after the n-th update (n = 1, 2, ...)"""
    if order == 0:
        return [1. / n]
    if order == 1:
        return [2. * (2 * n - 1) / (n * (n + 1)), 6. / (n * (n + 1) * dt)]
    den = n * (n + 1) * (n + 2)
    return [3. * (3 * n**2 - 3 * n + 2) / den, 18. * (2 * n - 1) / (den * dt), 60. / (den * dt**2)]


def lsq(order, dt, n0, T):
    """-> scalars and the (T, order + 1) gains table of updates n0 + 1 .. n0 + T"""
    table = np.array([lsq_gains(order, n0 + 1 + t, dt) for t in range(T)], dtype=np.float64).reshape(T, order + 1)
    return dict(form=FORM_A if order == 0 else FORM_C, dt=dt, T2=0.0, c=0.5 * dt**2, g=(0.0, 0.0, 0.0)), table


def golden():
    return np.load(GOLDEN)
