"""The cubature filter's kernels on hard models (tests/ckf_models.py: P of condition 1e8, state means 1e3 spreads away from the
origin, 30 steps) against tests/ckf_hp.py, the reference's lines in longdouble.  Errors are normwise per step, the worst step
counted.  On these models the float64 port's own worst-track error is 1e-11 .. 8e-10 on the means and 9e-9 .. 1e-7 on P: it sums
X X' - x x' like the reference.  The bar is per model and output: every track's err(gpu, hp) <= max(K_BAR max_tracks
err(ckf_port, hp), 1e-12), and the median over tracks <= K_BAR times the port's median.  K_BAR = 2^-8: the host-compiled
fk_ckf.hpp step against the port on exactly these models is at most 0.00114 times the port's error (tests/test_host_ckf.py
measures and asserts it), doubled for the device's contraction and refined seeds, rounded up to a power of two.  No track is
excluded.  Measured on an MI355X: docs/MEASUREMENTS.md, "Cubature filter precision"."""
import numpy as np
import pytest

import ckf_models as cm
from filterpy_amd.kalman import CubatureKalmanFilter

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("layout", ["soa", "aos"])
@pytest.mark.parametrize("dims", cm.DIMS)
def test_offset_ill_scaled_models_vs_extended_precision(layout, dims):
    n, m = dims
    d = cm.model(dims)
    b = CubatureKalmanFilter(n, m, 1.0, d["H"], d["F"], n_tracks=cm.NT, layout=layout)
    b.x, b.P, b.Q, b.R = d["x0"], d["P0"], d["Q"], d["R"]
    out = b.batch_filter(d["zs"])
    eg, ep = cm.errors(out, dims), cm.truth(dims)[1]
    for j, name in enumerate(cm.OUTPUTS):
        bar = max(cm.K_BAR * ep[j].max(), 1e-12)
        print(dims, layout, name, "worst err/bar %.3f" % (eg[j].max() / bar), "gpu/port medians %.5f" %
              (np.median(eg[j]) / max(np.median(ep[j]), 1e-300)), "port worst %.1e gpu worst %.1e" % (ep[j].max(), eg[j].max()))
    for j, name in enumerate(cm.OUTPUTS):
        bar = max(cm.K_BAR * ep[j].max(), 1e-12)
        assert eg[j].max() <= bar, (name, eg[j], ep[j])
        assert np.median(eg[j]) <= max(cm.K_BAR * np.median(ep[j]), 1e-12), (name, eg[j], ep[j])
