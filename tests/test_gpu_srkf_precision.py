"""The square-root filter's kernels on ill-conditioned models (P0 ~ 1e10 I, R ~ 1e-6 I: what the square-root form is for)
against tests/srkf_hp.py, the same algorithm in longdouble.  Errors are normwise per step, the worst step counted.  On these
models the float64 error of ONE track is rounding noise amplified by the conditioning (~1e-9 on the means), and two float64
orderings of the same arithmetic scatter by several times either way track by track (the host build of fk_srkf.hpp against
tests/srkf_port.py: 0.2x .. 8x on the (4, 2) model, medians over 64 tracks 1.16x apart).  So the bar is per model and output: every track's
err(gpu, hp) <= max(4 max_tracks err(srkf_port, hp), 1e-12), and the median over tracks <= 4x the port's median.  A kernel
that formed P = P1_2 P1_2' and re-factored it fails these models outright: in float64 the re-formed P is not positive definite
after the first update."""
import numpy as np
import pytest

import srkf_hp
import srkf_port as sp
from filterpy_amd.kalman import SquareRootKalmanFilterBank

pytestmark = pytest.mark.gpu


def _err(a, hp):
    """worst normwise relative error over the steps, measured in longdouble"""
    d = np.abs(np.asarray(a, dtype=srkf_hp.LD) - hp).reshape(len(hp), -1).max(axis=1)
    return float(np.max(d / np.maximum(np.abs(hp).reshape(len(hp), -1).max(axis=1), 1e-300)))


@pytest.mark.parametrize("layout", ["soa", "aos"])
@pytest.mark.parametrize("dims", [(2, 1), (4, 2), (6, 3), (9, 3), (12, 4)])
def test_ill_conditioned_vs_extended_precision(layout, dims):
    n, m = dims
    rs = np.random.RandomState(n * 10 + m)
    Nt, T = 64, 25
    b = SquareRootKalmanFilterBank(n, m, Nt, layout=layout)
    b.F = np.eye(n) + np.diag(np.ones(n - 1), 1) * 0.5 + 0.01 * rs.randn(n, n)
    b.H = rs.randn(m, n)
    b.Q = np.diag(10.0 ** rs.uniform(-8, -2, n))
    b.R = np.eye(m) * 1e-6
    b.x = rs.randn(Nt, n)
    b.P = np.eye(n) * 1e10
    zs = rs.randn(T, Nt, m) * 100
    out = b.batch_filter(zs)
    eg, ep = np.zeros((4, Nt)), np.zeros((4, Nt))
    for k, i in enumerate(range(Nt)):
        hp = srkf_hp.batch(b.x[i], b.P1_2[i], zs[:, i], b.F, b.Q1_2, b.H, b.R1_2)
        port = sp.batch(b.x[i], b.P1_2[i], zs[:, i], b.F, b.Q1_2, b.H, b.R1_2)
        for j in range(4):
            eg[j, k], ep[j, k] = _err(out[j][:, i], hp[j]), _err(port[j], hp[j])
    for j, name in enumerate(("means", "sqrt_covs", "means_p", "sqrt_covs_p")):
        bar = max(4 * ep[j].max(), 1e-12)
        assert eg[j].max() <= bar, (name, eg[j], ep[j])
        assert np.median(eg[j]) <= max(4 * np.median(ep[j]), 1e-12), (name, eg[j], ep[j])
        print(dims, layout, name, "worst err/bar %.3f" % (eg[j].max() / bar), "gpu/port medians %.2f" %
              (np.median(eg[j]) / max(np.median(ep[j]), 1e-300)))
