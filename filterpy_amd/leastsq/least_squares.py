"""filterpy.leastsq on the GPU: LeastSquaresFilter (filterpy/leastsq/least_squares.py), the recursive least-squares polynomial
filter of order 0, 1 or 2 after Zarchan.  The gains depend on the step count alone: update() forms them on the host with the
reference's expressions and runs the step in fk_poly_run (include/filterhip.h; order 0 form A, orders 1 and 2 form C);
batch_filter() hands the launch the table of all T steps' gains.  The results are the reference's bits.

n_tracks is new: the reference is one filter (it raises on a vector z).  With n_tracks = N, x is (order + 1, N) and update()
takes N measurements.  A NumPy (or number) measurement keeps x in NumPy; once a device tensor is given, x lives on the
device."""
from math import sqrt

import numpy as np

from .. import _poly as P


class LeastSquaresFilter(object):

    def __init__(self, dt, order, noise_sigma=0., n_tracks=None):
        P.check_order(order)
        if n_tracks is not None and int(n_tracks) < 1:
            raise ValueError('n_tracks must be at least 1')
        self.dt = dt
        self.sigma = noise_sigma
        self._order = order
        self.n_tracks = None if n_tracks is None else int(n_tracks)
        self.reset()

    def reset(self):
        """back to the state at construction"""
        self.n = 0                       # updates so far
        shape = (self._order + 1,) if self.n_tracks is None else (self._order + 1, self.n_tracks)
        self.x = np.zeros(shape)
        self.K = np.zeros(self._order + 1)
        self.y = 0                       # (never updated: the reference assigns its residual to a local)

    def _gains(self, n):
        """K at the n-th update.  Zarchan's recursive least-squares gains: component i is a small integer polynomial in n
        over n (n + 1) ... (n + order) dt^i.  The integers are exact; the one rounding per gain is the final division (and the
        product with dt before it)."""
        dt = self.dt
        run = 1
        for j in range(self._order + 1):
            run *= n + j
        odd = 2 * n - 1
        tops = ([1.], [2. * odd, 6.], [3. * (3 * n**2 - 3 * n + 2), 18. * odd, 60.])[self._order]
        below = (run, run * dt, run * dt**2)
        return [top / low for top, low in zip(tops, below)]

    def _run(self, zs, want, on_device):
        order = self._order
        N = 1 if self.n_tracks is None else self.n_tracks
        z = P.steps(zs, N)
        T = z.shape[0]
        table = np.array([self._gains(self.n + 1 + t) for t in range(T)], dtype=np.float64).reshape(T, order + 1)
        if on_device and not P.is_tensor(self.x):
            self.x = P.E.dev(self.x)                       # from here on the state lives on the device
        st = P.E.dev(self.x).reshape(order + 1, N).clone()
        form = P.FORM_A if order == 0 else P.FORM_C
        if T == 1:
            g = list(table[0]) + [0.0] * (2 - order)
            out = P.run(order, form, self.dt, 0.0, 0.5 * self.dt**2, g, st, z, want=want)
        else:
            out = P.run(order, form, self.dt, 0.0, 0.5 * self.dt**2, (0.0, 0.0, 0.0), st, z, gains=table, want=want)
        self.n += T
        self.K[:] = table[-1]
        if P.is_tensor(self.x):
            self.x.copy_(st.reshape(self.x.shape))
        else:
            self.x[...] = P.host(st).reshape(self.x.shape)
        return out

    def update(self, z):
        """one step with measurement z (a number; N values with n_tracks = N); returns x"""
        self._run(P.row(z).reshape(1, -1), (), P.is_tensor(z))
        return self.x

    def batch_filter(self, zs, device_outputs=False):
        """T update() calls in one launch (an extension): zs (T,) or (T, N) -> the state after every step, (T, order + 1) or
        (T, order + 1, N).  n, K and x are left exactly as the T calls would leave them."""
        if len(zs) == 0:
            return np.zeros((0,) + tuple(self.x.shape))
        xs = self._run(zs, ("xs",), P.is_tensor(zs))["xs"]
        xs = xs.reshape((xs.shape[0],) + tuple(self.x.shape))
        return xs if (device_outputs or P.is_tensor(self.x)) else P.host(xs)

    def errors(self):
        """(error, std) of the estimate after n updates, order + 1 components each, for measurement noise sigma: Zarchan's
        closed forms.  Each variance is an integer polynomial in n over a product of consecutive integers around n, times
        sigma^2 / dt^(2 i) for component i.  `error` stays zero until the fit is determined (n > order); `std` is evaluated
        at every n >= 1 and divides by zero where the closed form does."""
        n, dt, sigma, order = self.n, self.dt, self.sigma, self._order
        if n == 0:
            return (np.zeros(order + 1), np.zeros(order + 1))
        if order == 0:
            spread = sigma / sqrt(n)
            return np.array([spread]), np.array([spread])
        if order == 1:
            tops = (2 * (2 * n - 1), 12)
            lows = (n * (n + 1), n * (n * n - 1))
            with_dt = (lows[0], lows[1] * dt * dt)
            front = (sigma, sigma / dt)
        else:
            step2 = dt * dt
            wide = n * (n * n - 1) * (n * n - 4)
            tops = (3 * (3 * n * n - 3 * n + 2), 12 * (16 * n * n - 30 * n + 11), 720)
            lows = (n * (n + 1) * (n + 2), wide, wide)
            with_dt = (lows[0], wide * step2, wide * step2 * step2)
            front = (sigma, sigma / dt, sigma / step2)
        error = np.zeros(order + 1)
        if n > order:
            error[:] = [sigma * sqrt(top / low) for top, low in zip(tops, with_dt)]
        std = np.array([f * sqrt(top / low) for f, top, low in zip(front, tops, lows)])
        return error, std

    def __repr__(self):
        return '\n'.join(['LeastSquaresFilter object'] + [P.pretty(n, getattr(self, n)) for n in
                                                           ('dt', 'sigma', '_order', 'x', 'K')])
