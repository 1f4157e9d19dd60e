"""The models of the extended filter's tests.

Golden models (tests/golden/make_ekf_golden.py freezes the live reference on them; tests/test_host_ekf.py and
tests/test_gpu_ekf.py run them): the slant-range radar of the reference's own kalman/tests/test_ekf.py at (3, 1), and a
range-bearing sensor with an angle-wrapping residual at (4, 2).

Precision models (tests/test_gpu_ekf_precision.py on the GPU, tests/test_host_ekf.py for the host-compiled step that fixes the
bar's factor K_BAR): ill-scaled states as in tests/ckf_models.py, D = diag(10^-2 .. 10^2): F = D Fs D^-1 with Fs orthogonal (a
small random rotation), Q = D diag(1e-3 .. 1e-1) D, per track P0 = D C D with C a well-conditioned correlation-like matrix
(condition 1e8), x0 a few spreads from the origin; and a bilinear measurement
    h_j(x) = x_j + c x_j x_(j+1 mod n),      Jacobian row j:  1 + c x_(j+1) at column j,  c x_j at column j+1,
j = 0 .. m-1, c = 1e-2, R = diag((0.1 D_j)^2).  The callables use only + and x as separate array operations, so NumPy and eager
torch on the GPU return the same bits and the bar measures the kernel alone.  The measurements follow a simulated truth."""
import math

import numpy as np

import ekf_hp

# ------------------------------------------------------------------------------------------------------ golden models --
DT = 0.05


def radar(rs=None):
    """kalman/tests/test_ekf.py: state (position, velocity, altitude), the radar measures the slant range"""
    F = np.eye(3) + np.array([[0, 1, 0], [0, 0, 0], [0, 0, 0]]) * DT
    rng = 5.0 ** 2
    Q = np.zeros((3, 3))
    Q[0:2, 0:2] = np.array([[DT ** 4 / 4, DT ** 3 / 2], [DT ** 3 / 2, DT ** 2]]) * 0.1
    Q[2, 2] = 0.1
    rs = rs or np.random.RandomState(3)
    pos, vel, alt, zs = 0.0, 100.0, 1000.0, []
    for _ in range(12):
        vel, alt = vel + 0.1 * rs.randn(), alt + 0.1 * rs.randn()
        pos += vel * DT
        zs.append(math.sqrt(pos ** 2 + alt ** 2) * (1 + 0.05 * rs.randn() * 0.1))
    return dict(n=3, m=1, F=F, Q=Q, R=np.eye(1) * rng, P=np.eye(3) * 50.0, x=np.array([-10.0, 90.0, 1100.0]),
                zs=[np.array([z]) for z in zs])


def radar_jac(x):
    hd, alt = x[0], x[2]
    d = np.sqrt(hd ** 2 + alt ** 2)
    return np.array([[float(hd / d), 0.0, float(alt / d)]])


def radar_hx(x):
    return (x[0] ** 2 + x[2] ** 2) ** 0.5


BEACON = (3.0, -4.0)


def range_bearing(rs=None):
    """state (px, vx, py, vy) as a column, a sensor at the origin measuring range and bearing of px - bx, py - by"""
    F = np.kron(np.eye(2), np.array([[1.0, DT], [0.0, 1.0]]))
    Q = np.kron(np.eye(2), np.array([[DT ** 3 / 3, DT ** 2 / 2], [DT ** 2 / 2, DT]])) * 0.5
    R = np.diag([0.3 ** 2, 0.02 ** 2])
    rs = rs or np.random.RandomState(5)
    xt, zs = np.array([-6.0, 4.0, -4.2, 1.0]), []        # crosses the bearing's branch cut (dy changes sign at dx < 0)
    for _ in range(12):
        xt = F @ xt
        dx, dy = xt[0] - BEACON[0], xt[2] - BEACON[1]
        zs.append(np.array([[math.hypot(dx, dy) + 0.3 * rs.randn()], [math.atan2(dy, dx) + 0.02 * rs.randn()]]))
    return dict(n=4, m=2, F=F, Q=Q, R=R, P=np.diag([1.0, 0.5, 1.0, 0.5]), x=np.array([[-5.5], [3.5], [-4.0], [1.5]]), zs=zs)


def rb_jac(x, beacon=BEACON):
    xr = np.ravel(x)
    dx, dy = float(xr[0]) - beacon[0], float(xr[2]) - beacon[1]
    r2 = dx * dx + dy * dy
    r = math.sqrt(r2)
    return np.array([[dx / r, 0.0, dy / r, 0.0], [-dy / r2, 0.0, dx / r2, 0.0]])


def rb_hx(x, beacon=BEACON):
    xr = np.ravel(x)
    dx, dy = float(xr[0]) - beacon[0], float(xr[2]) - beacon[1]
    return np.array([[math.hypot(dx, dy)], [math.atan2(dy, dx)]])


def rb_residual(a, b):
    y = np.subtract(a, b)
    y[1] = (y[1] + np.pi) % (2 * np.pi) - np.pi
    return y


CASES = {"radar": (radar, radar_jac, radar_hx, np.subtract), "rb": (range_bearing, rb_jac, rb_hx, rb_residual)}
# the call sequence of the goldens, one measurement per entry
OPS = ("predict", "update", "predict_update", "update_none", "predict", "update_scalar_R", "predict_update", "predict", "update",
       "predict", "update", "predict_update")
ATTRS = ("x", "P", "x_prior", "P_prior", "x_post", "P_post", "K", "y", "S", "SI", "log_likelihood", "likelihood", "mahalanobis")


def make(cls, case, **kw):
    """a filter object of class cls set up for the golden model `case` -> (object, model)"""
    d = CASES[case][0]()
    f = cls(d["n"], d["m"], **kw)
    f.x, f.P, f.F, f.Q, f.R = d["x"].copy(), d["P"].copy(), d["F"].copy(), d["Q"].copy(), d["R"].copy()
    return f, d


def run_op(f, case, d, k):
    _, jac_, hx_, res = CASES[case]
    op, z = OPS[k], d["zs"][k]
    if op == "predict":
        f.predict()
    elif op == "update":
        f.update(z, jac_, hx_, residual=res)
    elif op == "update_scalar_R":
        f.update(z, jac_, hx_, R=0.7, residual=res)
    elif op == "update_none":
        f.update(None, jac_, hx_)
    else:
        f.predict_update(z, jac_, hx_)


# --------------------------------------------------------------------------------------------------- precision models --
DIMS = [(2, 1), (4, 2), (6, 3), (9, 4), (12, 4)]
NT, T = 32, 30
C = 1e-2
OUTPUTS = ("means", "covs", "means_p", "covs_p")

# The bar: err(kernel, hp) <= max(K_BAR * max_tracks err(ekf_port, hp), 1e-12) per track, and the medians K_BAR apart at most.
# K_BAR = 2 * RATIO rounded up to a power of two; RATIO is the worst per-output ratio (worst tracks and medians) of the
# host-compiled fk_ekf.hpp step to the port on exactly these models -- tests/test_host_ekf.py measures it and asserts
# 2 * ratio <= K_BAR <= 32.  The doubling allows for the device's FMA contraction and refined reciprocal seeds.
RATIO = 2.117          # measured: means_p of (2, 1), worst tracks (the medians: 0.73 .. 1.75)
K_BAR = 8.0


def jac(x, m):
    """x (.., n) -> (.., m, n), NumPy or torch: + and x only, one operation at a time"""
    n = x.shape[-1]
    H = x.new_zeros(x.shape[:-1] + (m, n)) if hasattr(x, "new_zeros") else np.zeros(x.shape[:-1] + (m, n), dtype=x.dtype)
    for j in range(m):
        k = (j + 1) % n
        t = x[..., k] * C
        H[..., j, j] = t + 1.0
        H[..., j, k] = x[..., j] * C
    return H


def hx(x, m):
    """x (.., n) -> (.., m): h_j = x_j + (c x_j) x_(j+1)"""
    n = x.shape[-1]
    cols = []
    for j in range(m):
        t = x[..., j] * C
        t = t * x[..., (j + 1) % n]
        cols.append(x[..., j] + t)
    return _stack(cols)


def _stack(cols):
    if isinstance(cols[0], np.ndarray) or np.isscalar(cols[0]) or isinstance(cols[0], np.generic):
        return np.stack(cols, axis=-1)
    import torch
    return torch.stack(cols, dim=-1)


def model(dims):
    n, m = dims
    rs = np.random.RandomState(n * 10 + m)
    D = 10.0 ** np.linspace(-2, 2, n)
    Fs = np.linalg.qr(np.eye(n) + 0.1 * rs.randn(n, n))[0]
    F = Fs * D[:, None] / D[None, :]
    Q = np.diag(D * D * 10.0 ** rs.uniform(-3, -1, n))
    R = np.diag((0.1 * D[:m]) ** 2)
    P0 = np.zeros((NT, n, n))
    x0 = np.zeros((NT, n))
    zs = np.zeros((T, NT, m))
    for i in range(NT):
        A = rs.randn(n, n)
        Cm = A @ A.T / n + np.eye(n)
        P0[i] = (Cm * D[:, None]) * D[None, :]
        P0[i] = (P0[i] + P0[i].T) / 2
        x0[i] = 3.0 * np.sqrt(np.diag(P0[i])) * rs.uniform(-1, 1, n)
        xt = x0[i] + np.linalg.cholesky(P0[i]) @ rs.randn(n)
        for t in range(T):
            xt = F @ xt
            zs[t, i] = hx(xt, m) + np.sqrt(np.diag(R)) * rs.randn(m)
    return dict(n=n, m=m, F=F, Q=Q, R=R, x0=x0, P0=P0, zs=zs)


def err(a, hp):
    """worst normwise relative error over the steps, measured in longdouble"""
    d = np.abs(np.asarray(a, dtype=ekf_hp.LD) - hp).reshape(len(hp), -1).max(axis=1)
    return float(np.max(d / np.maximum(np.abs(hp).reshape(len(hp), -1).max(axis=1), 1e-300)))


_truth = {}


def truth(dims):
    """(hp, port errors): per track the longdouble histories, and err(ekf_port, hp) as a (4, NT) array; computed once"""
    if dims not in _truth:
        import ekf_port
        d = model(dims)
        m = d["m"]
        hps, ep = [], np.zeros((4, NT))
        for i in range(NT):
            a = (d["x0"][i], d["P0"][i], d["zs"][:, i], d["F"], d["Q"], d["R"], lambda x: jac(x, m), lambda x: hx(x, m))
            hp, port = ekf_hp.batch(*a), ekf_port.batch(*a)
            hps.append(hp)
            for j in range(4):
                ep[j, i] = err(port[j], hp[j])
        _truth[dims] = (hps, ep)
    return _truth[dims]


def errors(out, dims):
    """err(out, hp) per output and track, (4, NT); out: the four histories (T, NT, ...)"""
    hps, _ = truth(dims)
    eg = np.zeros((4, NT))
    for i in range(NT):
        for j in range(4):
            eg[j, i] = err(out[j][:, i], hps[i][j])
    return eg
