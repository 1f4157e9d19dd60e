"""The extended filter's kernels on hard models (tests/ekf_models.py: P of condition 1e8, ill-scaled states, a bilinear
measurement, 32 tracks x 30 steps) against tests/ekf_hp.py, the reference's lines in longdouble.  The class runs with device
callables (one predict, 29 fused steps, one update); the callables are + and x only, as separate eager tensor operations, so they
return the bits NumPy returns -- asserted first on the initial states -- and the bar measures the kernels alone.  Errors are
normwise per step, the worst step counted.  The bar is per model and output: every track's err(gpu, hp) <= max(K_BAR max_tracks
err(ekf_port, hp), 1e-12), and the median over tracks <= K_BAR times the port's median (same floor).  K_BAR = 8: the
host-compiled fk_ekf.hpp step against the port on exactly these models is at most 2.117 times the port's error
(tests/test_host_ekf.py measures and asserts it), doubled for the device's contraction and refined seeds, rounded up to a power
of two.  No track is excluded.  Measured on an MI355X: docs/MEASUREMENTS.md, "Extended filter precision"."""
import numpy as np
import pytest
import torch

import ekf_models as em
from filterpy_amd.kalman import ExtendedKalmanFilter

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("layout", ["soa", "aos"])
@pytest.mark.parametrize("dims", em.DIMS)
def test_ill_scaled_bilinear_models_vs_extended_precision(layout, dims):
    n, m = dims
    d = em.model(dims)
    jac, hx = (lambda x: em.jac(x, m)), (lambda x: em.hx(x, m))
    x0 = torch.as_tensor(d["x0"], device="cuda")
    assert np.array_equal(jac(x0).cpu().numpy(), jac(d["x0"])) and np.array_equal(hx(x0).cpu().numpy(), hx(d["x0"]))
    b = ExtendedKalmanFilter(n, m, n_tracks=em.NT, layout=layout, device_callables=True)
    b.x, b.P, b.F, b.Q, b.R = d["x0"], d["P0"], d["F"], d["Q"], d["R"]
    out = b.batch_filter(d["zs"], jac, hx)
    eg, ep = em.errors(out, dims), em.truth(dims)[1]
    for j, name in enumerate(em.OUTPUTS):
        bar = max(em.K_BAR * ep[j].max(), 1e-12)
        print(dims, layout, name, "worst err/bar %.3f" % (eg[j].max() / bar), "gpu/port medians %.5f" %
              (np.median(eg[j]) / max(np.median(ep[j]), 1e-300)), "port worst %.1e gpu worst %.1e" % (ep[j].max(), eg[j].max()))
    for j, name in enumerate(em.OUTPUTS):
        bar = max(em.K_BAR * ep[j].max(), 1e-12)
        assert eg[j].max() <= bar, (name, eg[j], ep[j])
        assert np.median(eg[j]) <= max(em.K_BAR * np.median(ep[j]), 1e-12), (name, eg[j], ep[j])
