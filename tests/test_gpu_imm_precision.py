"""-m gpu: the IMM / MMAE kernels on stiff banks against tests/imm_hp.py, the reference's IMMEstimator / MMAEFilterBank in
longdouble.

tests/test_gpu_imm.py runs benign banks (F stable, P0 ~ 2, R ~ 0.5) against the float64 oracle at 1e-10: a kernel that loses four
or five digits of the covariance more than the reference still passes.  The three kernel files differ in their ARITHMETIC --
imm_kernels.hip (a lane owns a bank, packed covariances, fk_imm.hpp), imm_lanes.hip (a lane owns a filter, the same packed
update, the moments over a group of lanes through LDS), imm_quad.hip (four or eight lanes own a filter, the full P in its own
Joseph form) -- so each is run here, plain and extended (MMAE; a missing measurement), at every group width of imm_lanes.hip
(G = 2, 4, 8, 16), through the C ABI call of tests/test_gpu_imm.py (gpu_util.run_imm).

The bar (imm_hp.check): the float64 oracle (oracle/imm_oracle.py) is measured against the longdouble truth, on the given inputs
and on K_DRAWS = 8 copies of them perturbed by one ulp; the worst of those is a track's reference error `ref`; then per bank and
output

    every checked track   err(gpu, hp) <= max(8 max_tracks ref, 1e-13)
    the median over them  median err(gpu, hp) <= max(8 median ref, 1e-13)

on the six per-step outputs (x, P, mu, x_prior, P_prior, L; MMAE has no priors) and on the bank's final state (the filters'
xs, Ps, and mu) against the truth's last step.  Errors are normwise per step (per filter for the final xs, Ps), the worst
counted, measured in longdouble.  Likelihoods: where the truth is below 1e-330 the kernel must return DBL_MIN exactly; an entry
whose truth lies in [1e-330, 1e-290] is left out of the likelihood's comparison (at most 1 % of a bank's entries:
imm_hp.measures_something, asserted before any kernel result is looked at).

Banks (imm_hp.bank): 150 tracks -- the bank ends inside a wave and inside a group --, T = 16, 16 tracks checked (0 1 15 16 63
64 143 144 149 and seven from the seed), families stiff (P0 = 1e6 I, R = 1e-4 I) and stiff_small_weights (P0 = 1e4 I,
R = 1e-2 I) everywhere, benign on one bank per kernel file.  (16,8) x 2 runs whichever of imm_quad.hip's four- and eight-lane
builds is the default: the other needs a process of its own (its switch is read once) and is not run here.

docs/MEASUREMENTS.md ("IMM precision") has the figures of the GPU run and of the host build (tests/test_host_imm_hp.py)."""
import numpy as np
import pytest

import imm_hp

pytestmark = pytest.mark.gpu

# (kernel file, kind, dim_x, dim_z, n_models, step 8 missing, families)
ALL = imm_hp.FAMILIES
CASES = [
    ("imm_kernels", "imm", 2, 1, 3, False, imm_hp.STIFF),
    ("imm_kernels", "imm", 4, 2, 2, False, imm_hp.STIFF),
    ("imm_kernels", "imm", 6, 3, 3, False, ALL),
    ("imm_kernels", "mmae", 6, 3, 2, False, imm_hp.STIFF),
    ("imm_kernels", "imm", 4, 2, 3, True, imm_hp.STIFF),
    ("imm_lanes G=2", "imm", 9, 4, 2, False, ALL),
    ("imm_lanes G=4", "imm", 9, 3, 4, False, imm_hp.STIFF),
    ("imm_lanes G=4", "imm", 8, 4, 4, False, imm_hp.STIFF),
    ("imm_lanes G=8", "imm", 9, 4, 8, False, imm_hp.STIFF),
    ("imm_lanes G=16", "imm", 4, 2, 13, False, imm_hp.STIFF),
    ("imm_lanes G=4", "mmae", 9, 3, 4, False, imm_hp.STIFF),
    ("imm_lanes G=8", "imm", 9, 4, 8, True, imm_hp.STIFF),
    ("imm_quad", "imm", 12, 3, 2, False, ALL),
    ("imm_quad", "imm", 14, 4, 3, False, imm_hp.STIFF),
    ("imm_quad", "imm", 16, 8, 2, False, imm_hp.STIFF),
    ("imm_quad", "mmae", 12, 3, 2, False, imm_hp.STIFF),
    ("imm_quad", "imm", 14, 4, 3, True, imm_hp.STIFF),
]
PARAMS = [c[:6] + (f,) for c in CASES for f in c[6]]
IDS = ["%s-%s-%d-%d-x%d%s-%s" % (p[0].replace(" ", "_").replace("=", ""), p[1], p[2], p[3], p[4], "-missing" if p[5] else "", p[6])
       for p in PARAMS]


def _checked(a, B):
    """[T][N]... -> [16 checked tracks][T]..."""
    return np.swapaxes(a[:, list(B["tracks"])], 0, 1)


@pytest.mark.parametrize("layout", ["soa", "aos"])
@pytest.mark.parametrize("org,kind,n,m,nm,masked,family", PARAMS, ids=IDS)
def test_bank_vs_extended_precision(org, kind, n, m, nm, masked, family, layout):
    from gpu_util import run_imm
    t = imm_hp.truth(kind, family, n, m, nm, masked)                      # computed once per bank, shared by the layouts, unchanged
    imm_hp.measures_something(t)
    B, mmae = t["model"], kind == "mmae"
    zmask = np.repeat(B["mask"][:, None], B["N"], axis=1) if masked else None
    r = run_imm(B["xs0"], B["Ps0"], B["mu0"], None if mmae else B["M"], B["zs"], B["Fs"], B["Qs"], B["Hs"], B["Rs"], layout,
                zmask=zmask, mmae=mmae, check_status=False)                                   # one launch: 150 tracks, 16 steps
    assert not r["status"].any(), r["status"][r["status"] != 0]           # zero on EVERY track of the bank
    assert all(np.all(np.isfinite(v)) for v in r.values())
    trk = list(B["tracks"])
    got = [_checked(r["x_out"], B), _checked(r["P_out"], B), _checked(r["mu_out"], B),
           None if mmae else _checked(r["x_prior_out"], B), None if mmae else _checked(r["P_prior_out"], B),
           _checked(r["likelihood_out"], B), r["xs"][trk], r["Ps"][trk], r["mu"][trk][:, None]]
    eg, floor_ok = imm_hp.errors(got, t)
    for name, eb, eo, ref, e in imm_hp.ratios(eg, t):
        print("%-15s %-4s (%d,%d)x%d%s %-20s %s %-8s err/bar %.3f  oracle %.2e  ref %.2e  gpu %.2e" % (
            org, kind, n, m, nm, " missing" if masked else "", family, layout, name, eb, eo, ref, e))
    assert floor_ok, "a likelihood whose truth is below 1e-330 is not DBL_MIN"
    bad = imm_hp.check(f"{org} {kind} ({n},{m})x{nm} {family} {layout}", eg, t)    # asserts that no track and no output is missing
    assert not bad, (bad, np.nanmax(eg, axis=1), np.nanmax(t["ref"], axis=1))
    assert imm_hp.not_the_neighbour(got[0], t)
