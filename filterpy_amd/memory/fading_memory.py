"""filterpy.memory on the GPU: FadingMemoryFilter (filterpy/memory/fading_memory.py), the fading-memory polynomial filter of
order 0, 1 or 2 after Zarchan.  update() runs in fk_poly_run (include/filterhip.h, form A: the gains G, H / dt and
2 K / dt**2 are host scalars, formed as the reference forms them) and gives the reference's bits.  x is (order + 1,) for one
filter or (order + 1, N) for a bank; a NumPy state answers in NumPy, a device tensor stays on the device."""
import numpy as np
import torch

from .. import _poly as P


def _series(beta, coeffs):
    """c0 + c1 beta + c2 beta^2 + ..., summed from the left"""
    total = coeffs[0]
    for power, c in enumerate(coeffs[1:], 1):
        total = total + c * beta**power
    return total


def _constants(order, beta, dt):
    """(P, e) of a filter: P, the variances of the estimates for unit measurement variance; e, the truncation errors per unit
    of the first polynomial coefficient the order leaves out.  Zarchan and Musoff's closed forms in q = 1 - beta, p = 1 + beta
    and r = beta / q, with the polynomials in beta as coefficient lists.  Constants: they do not move as the filter runs.  (The
    order-1 position error is evaluated as 2 dt 2 r^2, as the reference evaluates it.)"""
    q, p = 1 - beta, 1 + beta
    r = beta / q
    if order == 0:
        var = [q / p]
        err = [dt * beta / q]
    elif order == 1:
        var = [q * _series(beta, (1, 4, 5)) / p**3, 2 * q**3 / p**3]
        err = [2 * dt * 2 * r**2, dt * (_series(beta, (1, 3)) / q)]
    else:
        var = [q * (_series(beta, (1, 6, 16, 24, 19)) / p**5),
               q**3 * (_series(beta, (13, 50, 49)) / (2 * p**5 * dt**2)),
               6 * q**5 / (p**5 * dt**4)]
        err = [6 * dt**3 * r**3, dt**2 * _series(beta, (2, 5, 11)) / q**2, 6 * dt * _series(beta, (1, 2)) / q]
    return np.array(var, dtype=float), np.array(err, dtype=float)


class FadingMemoryFilter(object):

    def __init__(self, x0, dt, order, beta):
        P.check_order(order)
        if P.is_tensor(x0):
            self.x = x0.detach().to(dtype=torch.float64).clone()
        elif np.isscalar(x0):
            self.x = np.zeros(order + 1)
            self.x[0] = x0
        else:
            self.x = np.array(x0, dtype=float)
        if self.x.shape[0] != order + 1:
            raise ValueError(f"x0 must hold order + 1 = {order + 1} components, got {self.x.shape[0]}")
        self.dt = dt
        self.order = order
        self.beta = beta

        self.P, self.e = _constants(order, beta, dt)

    def __repr__(self):
        return '\n'.join(['FadingMemoryFilter object'] + [P.pretty(n, getattr(self, n)) for n in
                                                           ('dt', 'order', 'beta', 'x', 'P', 'e')])

    def _scalars(self):
        """(T2, gains) of the launch.  Zarchan's fading-memory gains with q = 1 - beta: the position gain is 1 - beta^(order + 1);
        order 1 adds H = q^2, order 2 H = 1.5 (1 + beta) q^2 and K = q^3 / 2.  The kernel multiplies the residual by H / dt and
        2 K / dt^2, formed here."""
        beta, dt = P.scalar_gain(self.beta, "beta"), self.dt
        q = 1 - beta
        position = 1 - beta**(self.order + 1)
        if self.order == 0:
            return 0.0, (position, 0.0, 0.0)
        if self.order == 1:
            return 0.0, (position, q**2 / dt, 0.0)
        rate, acc = 1.5 * (1 + beta) * q**2, 0.5 * q**3
        return dt**2., (position, rate / dt, 2 * acc / (dt**2))

    def _run(self, zs, want):
        T2, gains = self._scalars()
        N = 1 if self.x.ndim == 1 else self.x.shape[1]
        st = P.E.dev(self.x).reshape(self.order + 1, N).clone()
        out = P.run(self.order, P.FORM_A, self.dt, T2, 0.0, gains, st, P.steps(zs, N), want=want)
        new = st.reshape(self.x.shape) if P.is_tensor(self.x) else P.host(st).reshape(self.x.shape)
        if self.order == 0:
            self.x = new              # (the reference rebinds x at order 0 and writes in place at orders 1 and 2)
        elif P.is_tensor(self.x):
            self.x.copy_(new)
        else:
            self.x[...] = new
        return out

    def update(self, z):
        """one step with measurement z: a number, or one value per track"""
        self._run(P.row(z).reshape(1, -1), ())

    def batch_filter(self, zs, device_outputs=False):
        """T update() calls in one launch (an extension): zs (T,) or (T, N) -> the state after every step, (T, order + 1) or
        (T, order + 1, N).  The object is left exactly as the T calls would leave it."""
        if len(zs) == 0:
            return np.zeros((0,) + tuple(self.x.shape))
        xs = self._run(zs, ("xs",))["xs"]
        xs = xs.reshape((xs.shape[0],) + tuple(self.x.shape))
        return xs if (device_outputs or P.is_tensor(self.x)) else P.host(xs)
