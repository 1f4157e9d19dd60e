"""-m gpu: the UKF kernels on ill-conditioned models against tests/ukf_hp.py, the reference's algorithm in longdouble.

Every other GPU test of the UKF compares with a float64 result at 1e-10 on benign models (P0 ~ 2 I, R ~ 0.5 I): 5e5 ulps, which a
kernel that loses four or five digits more than the reference still passes.  Here the float64 oracle (oracle/ukf_oracle.py: the
reference's own arithmetic) and the kernel are BOTH measured against the longdouble truth, and the kernel may be at most
MARGIN times less accurate than the oracle, per model family, dims and output:

    every checked track   err(gpu, hp) <= max(MARGIN max_tracks err(oracle, hp), 1e-13)
    the median over them  median err(gpu, hp) <= max(MARGIN median err(oracle, hp), 1e-13)

Errors are normwise per step, the worst step counted, measured in longdouble (ukf_hp.err).

MARGIN = 8 is the scatter between two legitimate float64 orderings of this arithmetic, measured on the CPU on these very models,
track by track: the oracle against the plain host build of fk_ukf.hpp / fk_ukf_quad.hpp (correctly rounded sqrt and division) at
(2,1) (4,2) (6,3) (8,4) (12,3) (16,8), four families, paired and index-order sums, filter and smoother.  Worst
max_tracks err(host) / max_tracks err(oracle): 6.8 (mu, alpha = 1e-3, (8,4), paired sums; 5.1 on the stiff model at (2,1), index
order); worst ratio of medians: 4.6 (mu / xs, alpha = 1e-3, (12,3)); every other output is below 4.  Rounded up to the next
power of two: 8.  tests/test_host_ukf_hp.py asserts that the plain host build stays inside this bar, and holds the DEVICE's
pivot arithmetic (seed + refinement, fk_ukf.hpp: sqrt_rsqrt / rcp_refined) to it on the CPU.  It is set by that scatter, never
by what the kernel reaches.  docs/MEASUREMENTS.md ("UKF precision") has the figures of the GPU run: worst err/bar 0.85 (the
pair-regrouped mean at alpha = 1e-3, the row that set the margin), 0.17 on the stiff families; with the pivots refined by one
step only, as they were before this file existed, the same GPU reaches 0.84 on the stiff model (it passes: its seeds are better
than their stated 2^-24), the CPU emulation with float-rounded seeds 5.4 (it fails); with no refinement every fused case fails.

Model families (ukf_hp.models; a fixed RandomState per (dim_x, dim_z); every track its own x0 and measurements; T = 16, the
measurement of step 8 missing; a bank of 150 tracks, which ends inside a wave; 16 tracks checked: 0 1 15 16 63 64 143 144 149
and seven from the seed):
    benign               the _bank models of tests/test_gpu_ukf_mlg.py, alpha = 0.5: the control
    stiff                F = I + 0.5 superdiagonal + 0.01 randn, H = randn, Q = diag(10^U(-6,-2)), R = 1e-4 I, P0 = 1e6 I,
                         measurements 10 randn, alpha = 0.5, beta = 2, kappa = 3 - n
    stiff_small_weights  the same with P0 = 1e4 I, R = 1e-2 I, alpha = 1e-2
    alpha_1e-3           the benign model at alpha = 1e-3: the bar is the reference's own cancellation (1e-9 on the means)

No track is left out: on every model and dim the float64 oracle finishes all 16 tracks (a non-positive pivot raises) with
err(oracle, hp) < 1e-3 (worst: 4.8e-4, the means of the stiff model at (16,8)), and every test asserts that.  The smoother runs
on the kernel's own filter output from step ukf_hp.SMOOTH_FROM = 4 on: while P still carries P0 = 1e6 in directions no measurement
has seen (dim_x / dim_z steps), the smoothed covariance is a cancellation of nine or ten digits in any float64 arithmetic -- the
oracle's own ps[0] is off by 1e3 relative -- and would measure nothing."""
import numpy as np
import pytest

import ukf_hp

pytestmark = pytest.mark.gpu
MARGIN = 8.0

# (dim_x, dim_z, paired sums, smoother too):  exact one-lane classes; the padded one-lane class (filter; the smoother at 7..9 runs
# on the several-lane kernels for paired weights); four lanes (12,3) and eight lanes (16,8) per track, filter and smoother
CASES = [(2, 1, True, True), (2, 1, False, True), (4, 2, True, True), (4, 2, False, True), (6, 3, True, True), (6, 3, False, True),
         (8, 4, True, True), (8, 4, False, False), (12, 3, True, True), (16, 8, True, True)]


def _gpu_run(M, layout, paired, smooth):
    """fk_ukf_linear_batch_f64 on the whole bank, then fk_ukf_linear_rts_f64 on its own output (device to device)"""
    import torch
    from filterpy_amd import _engine as E
    from oracle import ukf_oracle
    n, m, N, T = M["n"], M["m"], M["N"], M["T"]
    Wm, Wc = ukf_oracle.merwe_weights(n, M["alpha"], M["beta"], M["kappa"])
    scale = ukf_hp.kernel_scale(n, M["alpha"], M["kappa"])
    assert E.ukf_linear_supported(n, m, paired) and (not smooth or E.ukf_linear_rts_supported(n, paired))
    dx, dP = E.to_records(M["x0"], layout, 0), E.to_records(M["P0"], layout, 0)
    means, covs = E.alloc_records((T,), N, n, layout), E.alloc_records((T,), N, n * n, layout)
    st = torch.full((N,), -1, dtype=torch.int32, device=dx.device)
    mask = np.repeat(M["mask"][:, None], N, axis=1)
    zz = np.where(mask[..., None] != 0, M["zs"], np.nan)                  # a masked measurement is never used
    dF, dQ, dWm, dWc = E.dev(M["F"]), E.dev(M["Q"]), E.dev(Wm), E.dev(Wc)
    E.ukf_linear_batch(n, m, N, T, layout, scale, dF, E.dev(M["H"]), dQ, E.dev(M["R"]), dWm, dWc, E.to_records(zz, layout, 1),
                       dx, dP, mask=torch.as_tensor(mask, device=dx.device), means=means, covs=covs, status=st, paired=paired)
    status = [st.cpu().numpy()]
    out = [E.from_records(means, layout, 1, (n,)), E.from_records(covs, layout, 1, (n, n)), None, None, None]
    if smooth:
        s0, Ts = ukf_hp.SMOOTH_FROM, T - ukf_hp.SMOOTH_FROM
        oxs, ops, oK = (E.alloc_records((Ts,), N, e, layout) for e in (n, n * n, n * n))
        st2 = torch.full((N,), -1, dtype=torch.int32, device=dx.device)
        E.ukf_linear_rts(n, N, Ts, layout, scale, dF, dQ, dWm, dWc, means[s0:], covs[s0:], oxs, ops, oK, st2, paired=paired)
        status.append(st2.cpu().numpy())
        out[2:] = [E.from_records(oxs, layout, 1, (n,)), E.from_records(ops, layout, 1, (n, n)), E.from_records(oK, layout, 1, (n, n))]
    return out, status


@pytest.mark.parametrize("layout", ["soa", "aos"])
@pytest.mark.parametrize("family", ukf_hp.FAMILIES)
@pytest.mark.parametrize("n,m,paired,smooth", CASES)
def test_fused_filter_and_smoother_vs_extended_precision(n, m, paired, smooth, family, layout):
    t = ukf_hp.truth(family, n, m)                                        # computed once per (family, n, m), shared, unchanged
    M = t["model"]
    eo = ukf_hp.errors(t["oracle"], t["hp"])
    assert len(M["tracks"]) == 16 == len(set(M["tracks"])) and eo.shape == (5, 16)
    assert np.all(np.isfinite(eo)) and eo.max() < 1e-3, eo.max(axis=1)     # the model measures something, on every track
    out, status = _gpu_run(M, layout, paired, smooth)
    for st in status:
        assert not st.any(), st[st != 0]                                  # zero on EVERY track of the bank
    trk = list(M["tracks"])
    got = [None if a is None else np.swapaxes(a[:, trk], 0, 1) for a in out]
    eg = ukf_hp.errors(got, t["hp"])
    n_out = 5 if smooth else 2
    assert not np.isnan(eg[:n_out]).any() and np.isnan(eg[n_out:]).all()  # nothing excluded
    bad = ukf_hp.check(f"({n},{m}) {'paired' if paired else 'index'} {family} {layout}", eg, eo, MARGIN)
    assert not bad, (bad, eg.max(axis=1), eo.max(axis=1))
    # the rest of the bank: finite, and the smoother's last step is the filter's own
    assert all(np.all(np.isfinite(a)) for a in out if a is not None)
    if smooth:
        assert np.array_equal(out[2][-1], out[0][-1]) and np.array_equal(out[3][-1], out[1][-1]) and not out[4][-1].any()


# ------------------------------------------------------------------------------------------ the split blocks on stiff inputs
def _block_run(B, n, m, layout, block):
    import torch
    from filterpy_amd import _engine as E
    i, N, k = B["in"], ukf_hp.N_BLOCK, 2 * n + 1
    R = lambda a: E.to_records(a, layout, 0)  # noqa: E731
    st = torch.full((N,), -1, dtype=torch.int32, device=E.require_gpu())
    if block == "sigma":
        sig = E.alloc_records((), N, k * n, layout)
        E.ut_sigma_points(n, N, layout, i["scale"], R(i["x"]), R(i["P"]), sig, st)
        out = [E.from_records(sig, layout, 0, (k, n))]
    elif block == "transform":
        xo, Po = E.alloc_records((), N, n, layout), E.alloc_records((), N, n * n, layout)
        E.ut_transform(n, k, N, layout, R(i["sigmas"]), E.dev(i["Wm"]), E.dev(i["Wc"]), E.dev(i["Q"]), xo, Po)
        st.zero_()                                                        # (this block has no status)
        out = [E.from_records(xo, layout, 0, (n,)), E.from_records(Po, layout, 0, (n, n))]
    elif block == "correct":
        dx, dP, dK = R(i["x"]), R(i["P"]), E.alloc_records((), N, n * m, layout)
        E.ukf_correct(n, m, N, layout, R(i["Pxz"]), R(i["zp"]), R(i["S"]), R(i["z"]), dx, dP, dK, st)
        out = [E.from_records(dx, layout, 0, (n,)), E.from_records(dP, layout, 0, (n, n)), E.from_records(dK, layout, 0, (n, m))]
    else:
        dx, dP, dK = R(i["x"]), R(i["P"]), E.alloc_records((), N, n * n, layout)
        E.ukf_rts_correct(n, N, layout, R(i["Pxb"]), R(i["xb"]), R(i["Pb"]), R(i["xn"]), R(i["Pn"]), dx, dP, dK, st)
        out = [E.from_records(dx, layout, 0, (n,)), E.from_records(dP, layout, 0, (n, n)), E.from_records(dK, layout, 0, (n, n))]
    return out, st.cpu().numpy()


@pytest.mark.parametrize("layout", ["soa", "aos"])
@pytest.mark.parametrize("block", ["sigma", "transform", "correct", "rts_correct"])
@pytest.mark.parametrize("n,m", ukf_hp.BLOCK_DIMS)
def test_split_blocks_on_stiff_inputs(n, m, block, layout):
    """fk_ut_sigma_points_f64, fk_ut_transform_f64, fk_ukf_correct_f64, fk_ukf_rts_correct_f64 (csrc/ut_kernels.hip; their factor
    and solve are fk_math.hpp's chol_lower / ldlt2 with the compiler's sqrt and division -- no seeded pivots) on covariances of
    condition 1e10 (a random orthogonal basis times diag(10^U(-4,6))) and S of condition 1e8: EVERY track of a 65-track bank
    against the ukf_hp blocks, the same bar.  The other tests of these blocks use matrices of condition ~10."""
    B = ukf_hp.blocks(n, m)
    eo = ukf_hp.block_errors(B["oracle"][block], B["hp"][block])
    assert eo.shape[1] == ukf_hp.N_BLOCK and np.all(np.isfinite(eo)) and eo.max() < 1e-3, eo.max(axis=1)
    out, st = _block_run(B, n, m, layout, block)
    assert not st.any(), st[st != 0]
    eg = ukf_hp.block_errors(out, B["hp"][block])
    assert eg.shape == eo.shape and np.all(np.isfinite(eg))              # every track, every output
    bad = ukf_hp.check(f"{block} ({n},{m}) {layout}", eg, eo, MARGIN)
    assert not bad, (bad, eg.max(axis=1), eo.max(axis=1))
