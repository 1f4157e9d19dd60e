"""The information filter's kernels on nearly uninformative priors (P_inv0 = 1e-7 .. 1e-4 I per track against R_inv = 1e2 I:
what the information form is for) against tests/info_hp.py, the reference's lines in longdouble.  Errors are normwise per step,
the worst step counted.  On these models (tests/info_models.py) the float64 port's own worst-track error is 0.9e-6 .. 3.5e-6 on the
means and 3e-8 .. 1.5e-6 on P_inv, and two float64 orderings of the arithmetic scatter by several times either way track by track.  So
the bar is per model and output: every track's err(gpu, hp) <= max(K_BAR max_tracks err(info_port, hp), 1e-12), and the median
over tracks <= K_BAR times the port's median.  K_BAR = 8: the host-compiled fk_info.hpp step against the port on exactly these
models is at most 3.75 times the port's error (tests/test_host_info.py measures and asserts it), doubled for the device's
contraction and refined reciprocal seeds, rounded up to a power of two.  No track is excluded.
Measured on an MI355X: docs/MEASUREMENTS.md, "Information filter precision"."""
import numpy as np
import pytest

import info_models as im
from filterpy_amd.kalman import InformationFilterBank

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("layout", ["soa", "aos"])
@pytest.mark.parametrize("dims", im.DIMS)
def test_uninformative_prior_vs_extended_precision(layout, dims):
    n, m = dims
    d = im.model(dims)
    b = InformationFilterBank(n, m, im.NT, layout=layout)
    b.F, b.H, b.Q, b.R_inv, b.x, b.P_inv = d["F"], d["H"], d["Q"], d["Rinv"], d["x0"], d["Pinv0"]
    out = b.batch_filter(d["zs"])
    eg, ep = im.errors(out, dims), im.truth(dims)[1]
    for j, name in enumerate(im.OUTPUTS):
        bar = max(im.K_BAR * ep[j].max(), 1e-12)
        print(dims, layout, name, "worst err/bar %.3f" % (eg[j].max() / bar), "gpu/port medians %.2f" %
              (np.median(eg[j]) / max(np.median(ep[j]), 1e-300)), "port worst %.1e" % ep[j].max())
    for j, name in enumerate(im.OUTPUTS):
        bar = max(im.K_BAR * ep[j].max(), 1e-12)
        assert eg[j].max() <= bar, (name, eg[j], ep[j])
        assert np.median(eg[j]) <= max(im.K_BAR * np.median(ep[j]), 1e-12), (name, eg[j], ep[j])
