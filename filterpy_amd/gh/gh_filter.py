"""filterpy.gh on the GPU: GHFilter, GHKFilter, GHFilterOrder and the four gain-selection helpers
(filterpy/gh/gh_filter.py).  Constructors, attributes, return values and error texts are the reference's; every predict /
update runs in fk_poly_run (include/filterhip.h) and gives the reference's bits.  The state may be a number (one filter) or a
1-D array / device tensor (a bank, one track per element, as the reference's own elementwise update already allows); the array
type given at construction decides what comes back (_poly.py)."""
import numpy as np
import torch

from .. import _poly as P


def _scalar(x):
    """one filter, its state a number?"""
    return not P.is_tensor(x) and np.ndim(x) == 0


def _like(x, z):
    """whose type an update's results take: the state's -- but a one-number state fed N measurements answers in z's type, as
    the reference's elementwise arithmetic broadcasts"""
    return z if _scalar(x) and not _scalar(z) else x


def _zeros_like_state(x):
    if P.is_tensor(x):
        return torch.zeros_like(x, dtype=torch.float64)
    return 0. if np.ndim(x) == 0 else np.zeros(len(x))


class GHFilterOrder(object):
    """A g-h filter of order 0, 1 or 2 (gh_filter.py:31-194).  x is (order + 1,) for one filter or (order + 1, N) for a bank;
    update(z) takes a number or N measurements.  batch_filter(zs) is an extension: T steps in one launch."""

    def __init__(self, x0, dt, order, g, h=None, k=None):
        P.check_order(order)
        if P.is_tensor(x0):
            self.x = x0.detach().to(dtype=torch.float64).clone()
        elif np.isscalar(x0):
            self.x = np.zeros(order + 1)
            self.x[0] = x0
        else:
            self.x = np.copy(np.asarray(x0).astype(float))
        if self.x.shape[0] != order + 1:
            raise ValueError(f"x0 must hold order + 1 = {order + 1} components, got {self.x.shape[0]}")
        self.dt = dt
        self.order = order
        self.g = g
        self.h = h
        self.k = k
        if P.is_tensor(self.x):
            self.y = torch.zeros(len(self.x), dtype=torch.float64, device=self.x.device)
            self.z = torch.zeros(len(self.x), dtype=torch.float64, device=self.x.device)
        else:
            self.y = np.zeros(len(self.x))    # residual
            self.z = np.zeros(len(self.x))    # last measurement

    def _scalars(self, g, h, k):
        """(form, T2, gains) as the reference's update evaluates them (gh_filter.py:142-181)"""
        g = P.scalar_gain(self.g if g is None else g, "g")
        if self.order == 0:
            return P.FORM_A, 0.0, (g, 0.0, 0.0)
        h = P.scalar_gain(self.h if h is None else h, "h")
        if self.order == 1:
            return P.FORM_B, 0.0, (g, h, 0.0)
        k = P.scalar_gain(self.k if k is None else k, "k")
        return P.FORM_B, self.dt**2., (g, h, 2 * k)

    def _run(self, zs, g, h, k, want):
        form, T2, gains = self._scalars(g, h, k)
        N = 1 if self.x.ndim == 1 else self.x.shape[1]
        st = P.E.dev(self.x).reshape(self.order + 1, N).clone()
        z = P.steps(zs, N)
        out = P.run(self.order, form, self.dt, T2, 0.0, gains, st, z, want=want)
        y = out["y"][-1]
        if P.is_tensor(self.x):
            self.x.copy_(st.reshape(self.x.shape))
            self.y = y if self.x.ndim == 2 else y[0]
        else:
            self.x[...] = P.host(st).reshape(self.x.shape)
            self.y = P.host(y) if self.x.ndim == 2 else P.host(y)[0]
        return out

    def update(self, z, g=None, h=None, k=None):
        """one step with measurement z (a number, or one value per track); g, h, k override the filter's for this step"""
        self._run(P.row(z).reshape(1, -1), g, h, k, ("y",))
        if self.order == 1:
            self.z = z

    def batch_filter(self, zs, device_outputs=False):
        """T update() calls in one launch: zs (T,) or (T, N) -> the state after every step, (T, order + 1) or (T, order + 1, N).
        The object is left exactly as the T calls would leave it."""
        if len(zs) == 0:
            return np.zeros((0,) + tuple(self.x.shape))
        xs = self._run(zs, None, None, None, ("xs", "y"))["xs"]
        if self.order == 1:
            self.z = zs[-1]
        xs = xs.reshape((xs.shape[0],) + tuple(self.x.shape))
        return xs if (device_outputs or P.is_tensor(self.x)) else P.host(xs)

    def __repr__(self):
        return '\n'.join(['GHFilterOrder object'] + [P.pretty(n, getattr(self, n)) for n in
                                                      ('dt', 'order', 'x', 'g', 'h', 'k', 'y', 'z')])


class _GHBase(object):
    """what GHFilter and GHKFilter share: the g-h batch_filter (GHKFilter's ignores ddx and k, as the reference's does:
    gh_filter.py:717-748)"""

    def _batch(self, data, save_predictions, saver, device_outputs):
        bank = not _scalar(self.x)
        N = P.row(self.x).numel()
        dev_out = device_outputs or P.is_tensor(self.x)
        z = P.steps(data, N)
        T = z.shape[0]
        h_dt = P.scalar_gain(self.h, "h") / self.dt
        st = torch.stack([P.row(self.x), P.row(self.dx)], dim=-1).contiguous()             # [N][2]: FK_LAYOUT_AOS
        first = st.clone()
        want = ("xs", "pred") if save_predictions else ("xs",)
        out = P.run(1, P.FORM_A, self.dt, 0.0, 0.0, (P.scalar_gain(self.g, "g"), h_dt, 0.0), st, z, layout="aos", want=want)
        results = torch.cat([first.reshape(1, N, 2), out["xs"].reshape(T, N, 2)])
        results = results if bank else results.reshape(T + 1, 2)
        if saver is not None:
            for _ in range(T):
                saver.save()
        if not dev_out:
            results = P.host(results)
        if save_predictions:
            pred = out["pred"] if bank else out["pred"].reshape(T)
            return results, (pred if dev_out else P.host(pred))
        return results


class GHFilter(_GHBase):
    """The g-h filter (gh_filter.py:197-523).  x and dx are numbers (one filter) or 1-D arrays / device tensors (a bank)."""

    def __init__(self, x, dx, dt, g, h):
        self.x = x
        self.dx = dx
        self.dt = dt
        self.g = g
        self.h = h
        self.dx_prediction = self.dx
        self.x_prediction = self.x
        self.y = _zeros_like_state(x)     # residual
        self.z = _zeros_like_state(x)

    def update(self, z, g=None, h=None):
        """predict and update with measurement z; returns (x, dx).  g, h override the filter's for this step."""
        g = P.scalar_gain(self.g if g is None else g, "g")
        h = P.scalar_gain(self.h if h is None else h, "h")
        like = _like(self.x, z)
        st = P.rows([self.x, self.dx])
        N = st.shape[1]
        zt = P.row(z)
        if zt.numel() != N:
            if N != 1:
                raise ValueError(f"z holds {zt.numel()} value(s), the bank has {N} track(s)")
            st = st.expand(2, zt.numel()).contiguous()
            N = zt.numel()
        out = P.run(1, P.FORM_B, self.dt, 0.0, 0.0, (g, h, 0.0), st, zt.reshape(1, N), want=("pred", "y"))
        self.dx_prediction = self.dx
        self.x_prediction = P.back(out["pred"][0], like)
        self.y = P.back(out["y"][0], like)
        self.dx = P.back(st[1], like)
        self.x = P.back(st[0], like)
        return (self.x, self.dx)

    def batch_filter(self, data, save_predictions=False, saver=None, device_outputs=False):
        """The whole run with fixed g and h in one launch (gh_filter.py:380-455: h / dt is formed once and multiplied, so
        the last bit may differ from a loop of update()).  Changes no member.  One filter: data (T,) -> results (T + 1, 2), row
        0 the initial (x, dx); predictions (T,).  A bank of N: data (T, N) -> results (T + 1, N, 2), predictions (T, N).
        saver.save() is called T times on the unchanged object.  device_outputs: leave the results on the device."""
        return self._batch(data, save_predictions, saver, device_outputs)

    # Variance reduction factors (Asquith): the variance of an estimate over the measurement's, for constant g and h.  All
    # three share the quadratic 2 g^2 + 2 h and the divisor g (4 - 2 g - h); the operands are summed in the order written, which
    # is what the last bit depends on.
    def _vrf_parts(self):
        gain, rate = self.g, self.h
        return 2 * gain**2 + 2 * rate, gain * rate, gain * (4 - 2 * gain - rate)

    def VRF_prediction(self):
        """variance reduction factor of the one-step prediction of x"""
        quad, cross, divisor = self._vrf_parts()
        return (quad + cross) / divisor

    def VRF(self):
        """(VRF of x, VRF of dx) of the filtered estimates"""
        quad, _, divisor = self._vrf_parts()
        return ((quad - 3 * self.g * self.h) / divisor, 2 * self.h**2 / (self.dt**2 * divisor))

    def __repr__(self):
        return '\n'.join(['GHFilter object'] + [P.pretty(n, getattr(self, n)) for n in
                                                 ('dt', 'g', 'h', 'x', 'dx', 'x_prediction', 'dx_prediction', 'y', 'z')])


class GHKFilter(_GHBase):
    """The g-h-k filter (gh_filter.py:526-854)."""

    def __init__(self, x, dx, ddx, dt, g, h, k):
        self.x = x
        self.dx = dx
        self.ddx = ddx
        self.x_prediction = self.x
        self.dx_prediction = self.dx
        self.ddx_prediction = self.ddx
        self.dt = dt
        self.g = g
        self.h = h
        self.k = k
        self.y = _zeros_like_state(x)     # residual
        self.z = _zeros_like_state(x)

    def update(self, z, g=None, h=None, k=None):
        """predict and update with measurement z; returns (x, dx).  g, h, k override the filter's for this step."""
        g = P.scalar_gain(self.g if g is None else g, "g")
        h = P.scalar_gain(self.h if h is None else h, "h")
        k = P.scalar_gain(self.k if k is None else k, "k")
        dt = self.dt
        dt_sqr = dt**2
        like = _like(self.x, z)
        st = P.rows([self.x, self.dx, self.ddx])
        N = st.shape[1]
        zt = P.row(z)
        if zt.numel() != N:
            if N != 1:
                raise ValueError(f"z holds {zt.numel()} value(s), the bank has {N} track(s)")
            st = st.expand(3, zt.numel()).contiguous()
            N = zt.numel()
        self.ddx_prediction = self.ddx
        self.dx_prediction = self.dx + self.ddx*dt            # (an attribute only: the launch forms its own)
        out = P.run(2, P.FORM_B, dt, dt_sqr, 0.0, (g, h, 2*k), st, zt.reshape(1, N), want=("pred", "y"))
        self.x_prediction = P.back(out["pred"][0], like)
        self.y = P.back(out["y"][0], like)
        self.ddx = P.back(st[2], like)
        self.dx = P.back(st[1], like)
        self.x = P.back(st[0], like)
        return (self.x, self.dx)

    def batch_filter(self, data, save_predictions=False, device_outputs=False):
        """A g-h filter over the data, as in the reference: ddx and k take no part (gh_filter.py:683-748).  Shapes as
        GHFilter.batch_filter; changes no member."""
        return self._batch(data, save_predictions, None, device_outputs)

    # Variance reduction factors and bias of the g-h-k filter (Asquith and Woods).  Two combinations of the gains recur:
    # 4 - 2 g - h (with its negative, 2 g + h - 4, in the prediction's formula) and g h + g k - 2 k.
    def VRF_prediction(self):
        """variance reduction factor of the one-step prediction of x"""
        gain, rate, acc = self.g, self.h, self.k
        both = 2 * gain + rate
        short = both - 4
        top = gain * acc * short + rate * (gain * both + 2 * rate)
        return top / (2 * acc - gain * (rate + acc) * short)

    def bias_error(self, dddx):
        """the lag of x behind a constant jerk dddx: -dt^3 dddx / (2 k)"""
        cube = self.dt**3
        return -cube * dddx / (2 * self.k)

    def VRF(self):
        """(VRF of x, of dx, of ddx) of the filtered estimates"""
        gain, rate, acc = self.g, self.h, self.k
        margin = 4 - 2 * gain - rate
        mix = gain * rate + gain * acc - 2 * acc
        of_x = ((2 * rate * (2 * gain**2 + 2 * rate - 3 * gain * rate) - 2 * gain * acc * margin)
                / (2 * acc - gain * (rate + acc) * margin))
        of_dx = (2 * rate**3 - 4 * rate**2 * acc + 4 * acc**2 * (2 - gain)) / (2 * margin * mix)
        of_ddx = 8 * rate * acc**2 / (self.dt**4 * margin * mix)
        return (of_x, of_dx, of_ddx)

    def __repr__(self):
        # (the reference prints the title 'GHFilter object' and dx_prediction under the label ddx_prediction: kept)
        return '\n'.join(['GHFilter object'] + [P.pretty(n, getattr(self, a)) for n, a in
                                                 (('dt', 'dt'), ('g', 'g'), ('h', 'h'), ('k', 'k'), ('x', 'x'), ('dx', 'dx'),
                                                  ('ddx', 'ddx'), ('x_prediction', 'x_prediction'),
                                                  ('dx_prediction', 'dx_prediction'), ('ddx_prediction', 'dx_prediction'),
                                                  ('y', 'y'), ('z', 'z'))])


def optimal_noise_smoothing(g):
    """(g, h, k) with the least noise in the estimates for a given g (Polge and Bhagavan):
    h = (2 g^3 - 4 g^2 + sqrt(4 g^6 - 64 g^5 + 64 g^4)) / (8 (1 - g)),  k = (h (2 - g) - g^2) / g"""
    under_root = 4 * g**6 - 64 * g**5 + 64 * g**4
    rate = ((2 * g**3 - 4 * g**2) + under_root**.5) / (8 * (1 - g))
    return (g, rate, (rate * (2 - g) - g**2) / g)


def least_squares_parameters(n):
    """(g, h) that make a g-h filter the order-1 least-squares fit of measurements 0..n:
    g = 2 (2 n + 1) / ((n + 1) (n + 2)),  h = 6 / ((n + 1) (n + 2))"""
    span = (n + 2) * (n + 1)
    return (2 * (2 * n + 1) / span, 6 / span)


def critical_damping_parameters(theta, order=2):
    """(g, h) for order 2, (g, h, k) for order 3, of the critically damped (discounted least-squares) filter whose errors
    fade by theta per step: g = 1 - theta^order; h = (1 - theta)^2 or 1.5 (1 - theta^2)(1 - theta); k = (1 - theta)^3 / 2"""
    if theta < 0 or theta > 1:
        raise ValueError('theta must be between 0 and 1')
    if order not in (2, 3):
        raise ValueError('bad order specified: {}'.format(order))
    position, rest = 1. - theta**order, 1. - theta
    if order == 2:
        return (position, rest**2)
    return (position, 1.5 * (1. - theta**2) * rest, .5 * rest**3)


def benedict_bornder_constants(g, critical=False):
    """(g, h) of the Benedict-Bordner filter (least transient error): h = g^2 / (2 - g); critical: the nearly critically
    damped variant, h = 0.8 (2 - g^2 - 2 sqrt(1 - g^2)) / g^2"""
    sq = g**2
    rate = 0.8 * (2. - sq - 2 * (1 - sq)**.5) / sq if critical else sq / (2. - g)
    return (g, rate)
