"""CPU-side characterisation (no GPU) of what the dispatchers of the square-root filter, the information filter and the
fixed-lag smoother refuse: every refusal returns before any HIP call, so the return code and the exact fk_last_error() text
of each branch can be pinned without a device.  The seven entry points share one descriptor check, one record-block guard
and one B / u rule (csrc/fk_dispatch.hpp); what differs between the families -- the family name inside the messages, the
fields a family allows, the smoother's k0 and its narrower record -- is what the cases below hold still.

The second half does the same for the entry points of the Kalman filter and the IMM estimator (csrc/kf_dispatch.cpp,
csrc/imm_dispatch.cpp, on the same scaffold): their refusals in the order the code makes them, and -- on machines without a
device only -- which kernel family a call that passes every check reaches."""
import ctypes

import pytest

BAD_ARG, UNSUPPORTED = -1, -2
ONE = ctypes.c_void_p(8)          # a non-NULL pointer that is never dereferenced: every case returns before a launch

# entry point -> (family, pointer arguments after desc [and lag, k0], indices of the required ones, their message, (B, u))
ENTRY = {
    "fk_srkf_batch_f64": ("srkf", 20, (0, 1, 2, 3, 6, 8, 9), "F,Q1_2,H,R1_2,z,x,P1_2 must not be NULL", (4, 5)),
    "fk_srkf_predict_f64": ("srkf", 8, (0, 1, 4, 5), "F,Q1_2,x,P1_2 must not be NULL", (2, 3)),
    "fk_srkf_update_f64": ("srkf", 12, (0, 1, 2, 4, 5), "H,R1_2,z,x,P1_2 must not be NULL", None),
    "fk_info_batch_f64": ("info", 16, (0, 1, 2, 3, 6, 8, 9), "F,Q,H,R_inv,z,x,P_inv must not be NULL", (4, 5)),
    "fk_info_predict_f64": ("info", 8, (0, 1, 4, 5), "F,Q,x,P_inv must not be NULL", (2, 3)),
    "fk_info_update_f64": ("info", 10, (0, 1, 2, 4, 5), "H,R_inv,z,x,P_inv must not be NULL", None),
    "fk_fls_batch_f64": ("fls", 15, (0, 1, 2, 3, 6, 7, 8, 9, 10), "F,Q,H,R,z,x,P,xs,xhat must not be NULL", (4, 5)),
}
FAMILY = {"srkf": "square-root filter", "info": "information filter", "fls": "fixed-lag smoother"}
STEPS = ("fk_srkf_batch_f64", "fk_info_batch_f64", "fk_fls_batch_f64")       # the entry points that read desc->T

DIMS = "dim_x, dim_z must be >= 1, dim_u >= 0"
RANGE = "dim_x/dim_z outside the compiled range (dim_x <= 16, dim_z <= 8)"
GUARD = "N * dim^2 * 8 bytes must stay below 4 GiB (split the bank)"
CONTROL = "dim_u > 0 needs B and u"


def _call(name, desc=None, null=(), all_null=False, lag=2, k0=0, no_desc=False):
    """One call with fake pointers; returns (code, last error).  desc: the fields that differ from a valid small call."""
    from filterpy_amd import _abi
    lib = _abi.lib()
    fields = dict(n=2, m=1, nu=0, model_mode=_abi.FK_MODEL_SHARED, N=4, T=3, layout=_abi.FK_LAYOUT_AOS, update_first=0,
                  alpha_sq=1.0, flags=0)
    fields.update(desc or {})
    d = _abi.fk_kf_desc(**fields)
    nptr = ENTRY[name][1]
    ptrs = [None if (all_null or i in null) else ONE for i in range(nptr)]
    ptrs[-1] = None                                                            # stream
    head = [None if no_desc else ctypes.byref(d)] + ([lag, k0] if name == "fk_fls_batch_f64" else [])
    rc = getattr(lib, name)(*head, *ptrs)
    return rc, lib.fk_last_error().decode()


def _n_t_message(name):
    return "N, T and k0 must be >= 0" if ENTRY[name][0] == "fls" else "N and T must be >= 0"


@pytest.mark.parametrize("name", sorted(ENTRY))
def test_null_desc(name):
    assert _call(name, no_desc=True) == (BAD_ARG, "desc is NULL")


@pytest.mark.parametrize("name", sorted(ENTRY))
@pytest.mark.parametrize("field", [dict(n=0), dict(m=0), dict(nu=-1)], ids=["n0", "m0", "nu-1"])
def test_dimensions_below_range(name, field):
    assert _call(name, field) == (BAD_ARG, DIMS)


@pytest.mark.parametrize("name", sorted(ENTRY))
def test_negative_N(name):
    assert _call(name, dict(N=-1)) == (BAD_ARG, _n_t_message(name))


@pytest.mark.parametrize("name", sorted(ENTRY))
def test_negative_T(name):
    if name in STEPS:
        assert _call(name, dict(T=-1)) == (BAD_ARG, _n_t_message(name))
    else:                                   # the single steps do not read T: with no tracks the call is an FK_OK no-op
        assert _call(name, dict(T=-1, N=0), all_null=True)[0] == 0


@pytest.mark.parametrize("name", sorted(ENTRY))
def test_bad_layout(name):
    assert _call(name, dict(layout=2)) == (BAD_ARG, "bad layout")
    assert _call(name, dict(layout=-1)) == (BAD_ARG, "bad layout")


@pytest.mark.parametrize("name", sorted(ENTRY))
@pytest.mark.parametrize("field", [dict(n=17), dict(m=9)], ids=["n17", "m9"])
def test_dimensions_above_range(name, field):
    assert _call(name, field) == (UNSUPPORTED, RANGE)


@pytest.mark.parametrize("name", sorted(ENTRY))
@pytest.mark.parametrize("mode", [1, 2, 3])
def test_non_shared_model(name, mode):
    assert _call(name, dict(model_mode=mode)) == (UNSUPPORTED, FAMILY[ENTRY[name][0]] + ": FK_MODEL_SHARED only")


@pytest.mark.parametrize("name", sorted(ENTRY))
def test_alpha_sq(name):
    fam = ENTRY[name][0]
    msg = ": update_first 0 and alpha_sq 1 only" if fam == "fls" else ": alpha_sq 1 and flags 0 only"
    assert _call(name, dict(alpha_sq=1.5)) == (UNSUPPORTED, FAMILY[fam] + msg)


@pytest.mark.parametrize("name", sorted(ENTRY))
def test_flags(name):
    """The filters take no flag; the smoother takes FK_KF_FLAG_R_JOSEPH_DIAG (1) and nothing else."""
    fam = ENTRY[name][0]
    if fam == "fls":
        for flags in (2, 3, 4, 32):
            assert _call(name, dict(flags=flags)) == (UNSUPPORTED, FAMILY[fam] + ": flags 0 or FK_KF_FLAG_R_JOSEPH_DIAG only")
        assert _call(name, dict(flags=1, N=0), all_null=True)[0] == 0
    else:
        for flags in (1, 2, 32):
            assert _call(name, dict(flags=flags)) == (UNSUPPORTED, FAMILY[fam] + ": alpha_sq 1 and flags 0 only")


@pytest.mark.parametrize("name", sorted(ENTRY))
def test_update_first(name):
    """Refused by the smoother only."""
    if ENTRY[name][0] == "fls":
        assert _call(name, dict(update_first=1)) == (UNSUPPORTED, "fixed-lag smoother: update_first 0 and alpha_sq 1 only")
    else:
        assert _call(name, dict(update_first=1, N=0), all_null=True)[0] == 0


def test_fls_negative_k0():
    assert _call("fk_fls_batch_f64", k0=-1) == (BAD_ARG, "N, T and k0 must be >= 0")


@pytest.mark.parametrize("name", sorted(ENTRY))
def test_missing_required_pointer(name):
    _, _, required, msg, _ = ENTRY[name]
    for i in required:
        assert _call(name, null=(i,)) == (BAD_ARG, msg), i
    # ... and a refusal of desc comes first
    assert _call(name, dict(layout=2), null=required) == (BAD_ARG, "bad layout")


@pytest.mark.parametrize("name", sorted(n for n in ENTRY if ENTRY[n][4]))
def test_control_needs_B_and_u(name):
    b, u = ENTRY[name][4]
    assert _call(name, dict(nu=1), null=(b,)) == (BAD_ARG, CONTROL)
    assert _call(name, dict(nu=1), null=(u,)) == (BAD_ARG, CONTROL)
    assert _call(name, dict(nu=1), null=(b, u)) == (BAD_ARG, CONTROL)
    # a missing required pointer is reported first
    assert _call(name, dict(nu=1), null=(0, b)) == (BAD_ARG, ENTRY[name][3])


@pytest.mark.parametrize("name", sorted(ENTRY))
def test_record_block_guard(name):
    """One step's record block stays below 4 GiB - 32 bytes.  Its widest record is max(n, m)^2 doubles for the two filters
    (the m x m by-products) and n * max(n, m) for the smoother (P, K): at (n, m) = (2, 4) that is 16 against 8, so 2^25
    tracks are refused by the filters alone and the smoother refuses from 2^26 on."""
    fam = ENTRY[name][0]
    first = 2 ** 26 if fam == "fls" else 2 ** 25
    assert _call(name, dict(n=2, m=4, N=first)) == (UNSUPPORTED, GUARD)
    assert _call(name, dict(n=2, m=4, N=2 ** 27)) == (UNSUPPORTED, GUARD)
    # the control record counts where it is the widest: nu = 32 > 16
    assert _call(name, dict(n=2, m=4, nu=32, N=2 ** 24)) == (UNSUPPORTED, GUARD)
    # the pointers are looked at before the guard
    assert _call(name, dict(n=2, m=4, N=2 ** 27), null=(0,)) == (BAD_ARG, ENTRY[name][3])


def test_record_block_guard_is_narrower_for_the_smoother():
    """2^25 tracks of (2, 4) pass the smoother's guard (8 doubles per record, 2^31 bytes): without a device the call then
    ends in the launch, which fails -- FK_ERR_LAUNCH, not the guard's FK_ERR_UNSUPPORTED.  (With a device present the call
    would launch on the fake pointers, so the passing side is pinned on device-less machines only.)"""
    import torch
    if torch.cuda.is_available():
        return
    rc, msg = _call("fk_fls_batch_f64", dict(n=2, m=4, N=2 ** 25))
    assert rc == -3 and msg.startswith("fls_"), (rc, msg)


@pytest.mark.parametrize("name", sorted(ENTRY))
def test_nothing_to_do_is_ok_with_null_pointers(name):
    assert _call(name, dict(N=0), all_null=True)[0] == 0
    assert _call(name, dict(N=0, nu=3), all_null=True)[0] == 0
    if name in STEPS:
        assert _call(name, dict(T=0), all_null=True)[0] == 0
    # ... but not before desc is checked
    assert _call(name, dict(N=0, n=17), all_null=True) == (UNSUPPORTED, RANGE)


# ---------------------------------------------------------------------------------------------------------------------
# The Kalman filter entry points (csrc/kf_dispatch.cpp) and the IMM estimator's (csrc/imm_dispatch.cpp).

LAUNCH = -3
# entry point -> (arguments after desc, indices of the required pointers, their message, (B, u))
KF_ENTRY = {
    "fk_kf_batch_filter_f64": (16, (0, 1, 2, 3, 6, 8, 9), "F,Q,H,R,z,x,P must not be NULL", (4, 5)),
    "fk_kf_batch_filter_ex_f64": (17, (0, 1, 2, 3, 6, 8, 9), "F,Q,H,R,z,x,P must not be NULL", (4, 5)),
    "fk_kf_predict_f64": (8, (0, 1, 4, 5), "F,Q,x,P must not be NULL", (2, 3)),
    "fk_kf_update_f64": (12, (0, 1, 2, 4, 5), "H,R,z,x,P must not be NULL", None),
    "fk_kf_rts_f64": (11, (0, 1, 2, 3, 4, 5), "F,Q,Xs,Ps,xs,Ps_out must not be NULL", None),
}
KF_BATCH = ("fk_kf_batch_filter_f64", "fk_kf_batch_filter_ex_f64")
KF_STEPS = KF_BATCH + ("fk_kf_rts_f64",)                # the entry points for which T == 0 is an FK_OK no-op
MEANS, COVS, MEANS_P, COVS_P, EX = 10, 11, 12, 13, 14     # batch_filter: the four outputs; _ex: the extras pointer
UPD_Y, UPD_K, UPD_S, UPD_SI = 6, 7, 8, 9
RTS_K, RTS_PP, RTS_CONV = 6, 7, 8
N_T = "N and T must be >= 0"
SOA_GUARD = ("element-major layout: N * dim^2 * 8 bytes must stay below 4 GiB (use FK_LAYOUT_AOS, which is split automatically, "
             "or split the bank)")
GIVEN_GUARD = "caller-supplied inverse: N * dim^2 * 8 bytes must stay below 4 GiB (split the bank)"
IL = "FK_KF_FLAG_COV_INTERLEAVED: "
# every environment variable the two dispatchers read on the way to a kernel
SWITCHES = ("FK_NO_FAST", "FK_NO_ML", "FK_NO_MLG", "FK_ML9", "FK_RTS_LANES", "FK_NO_FAST_EX", "FK_NO_MLG_EX", "FK_FAST_VARIANT",
            "FK_FAST_XCD", "FK_KF_WINDOW", "FK_ML_VAR", "FK_ML_CHUNKS", "FK_IMM_CHUNKS", "FK_ML_PERSIST", "FK_RTS_PERSIST")
BASE = 1 << 20                    # where the fake covariance histories start (never dereferenced)


@pytest.fixture
def env(monkeypatch):
    """No routing switch set, whatever the caller's shell holds; the test sets its own through the returned monkeypatch."""
    for v in SWITCHES:
        monkeypatch.delenv(v, raising=False)
    return monkeypatch


def _kf(name, desc=None, null=(), all_null=False, no_desc=False, at=None, conv=0, extras=False):
    """One call of a Kalman filter entry point with fake pointers; returns (code, last error).  at: {index: address}."""
    from filterpy_amd import _abi
    lib = _abi.lib()
    fields = dict(n=2, m=1, nu=0, model_mode=_abi.FK_MODEL_SHARED, N=4, T=3, layout=_abi.FK_LAYOUT_AOS, update_first=0,
                  alpha_sq=1.0, flags=0)
    fields.update(desc or {})
    d = _abi.fk_kf_desc(**fields)
    ptrs = [None if (all_null or i in null) else ONE for i in range(KF_ENTRY[name][0])]
    for i, address in (at or {}).items():
        ptrs[i] = ctypes.c_void_p(address)
    ptrs[-1] = None                                                            # stream
    if name == "fk_kf_batch_filter_ex_f64":
        ex = _abi.fk_kf_extras(*([8] * 6))
        ptrs[EX] = ctypes.byref(ex) if extras else None
    if name == "fk_kf_rts_f64":
        ptrs[RTS_CONV] = conv
    rc = getattr(lib, name)(None if no_desc else ctypes.byref(d), *ptrs)
    return rc, lib.fk_last_error().decode()


def _interleaved(n, N, layout):
    """covs / covs_p of a FK_KF_FLAG_COV_INTERLEAVED call: the two halves of one array."""
    return {COVS: BASE, COVS_P: BASE + 8 * (n * n if layout == 0 else n * n * N)}


@pytest.mark.parametrize("name", sorted(KF_ENTRY))
def test_kf_desc_refusals_in_order(name, env):
    """check_desc: each refusal, with everything after it in the order made wrong as well."""
    assert _kf(name, no_desc=True) == (BAD_ARG, "desc is NULL")
    for field in (dict(n=0), dict(m=0), dict(nu=-1)):
        assert _kf(name, dict(field, N=-1, layout=2)) == (BAD_ARG, DIMS)
    assert _kf(name, dict(N=-1, layout=2)) == (BAD_ARG, N_T)
    # predict and update never read T and refuse a negative one all the same
    assert _kf(name, dict(T=-1, layout=2)) == (BAD_ARG, N_T)
    for layout in (2, -1):
        assert _kf(name, dict(layout=layout, model_mode=4)) == (BAD_ARG, "bad layout")
    for mode in (-1, 4):
        assert _kf(name, dict(model_mode=mode, flags=64)) == (BAD_ARG, "bad model_mode")
    assert _kf(name, dict(flags=64, layout=1, N=2 ** 27)) == (BAD_ARG, "unknown desc flag")
    assert _kf(name, dict(flags=64 | 2)) == (BAD_ARG, "unknown desc flag")
    # ... all of it before a pointer is looked at
    assert _kf(name, dict(flags=64), all_null=True) == (BAD_ARG, "unknown desc flag")


@pytest.mark.parametrize("name", sorted(KF_ENTRY))
def test_kf_element_major_guard(name, env):
    """One step's record block, n * max(n, m) doubles per track, stays 32 bytes short of 4 GiB in the element-major layout;
    NumPy order is cut into track windows instead."""
    assert _kf(name, dict(n=2, m=4, layout=1, N=2 ** 26)) == (UNSUPPORTED, SOA_GUARD)              # 2^26 * 8 * 8 = 4 GiB
    assert _kf(name, dict(n=2, m=1, layout=1, N=2 ** 27), all_null=True) == (UNSUPPORTED, SOA_GUARD)
    # 32 bytes short of 4 GiB: (1, 1), one double per track -- 2^29 - 4 tracks are refused, an empty run of 2^29 - 5 is not
    assert _kf(name, dict(n=1, m=1, layout=1, N=2 ** 29 - 4)) == (UNSUPPORTED, SOA_GUARD)
    if name in KF_STEPS:
        assert _kf(name, dict(n=1, m=1, layout=1, N=2 ** 29 - 5, T=0), all_null=True)[0] == 0
    # NumPy order at the same N: not the guard -- the next refusal in line
    assert _kf(name, dict(n=2, m=4, layout=0, N=2 ** 26), null=(0,)) == (BAD_ARG, KF_ENTRY[name][2])


@pytest.mark.parametrize("name", sorted(KF_ENTRY))
def test_kf_nothing_to_do_is_ok_with_null_pointers(name, env):
    assert _kf(name, dict(N=0), all_null=True)[0] == 0
    assert _kf(name, dict(N=0, nu=3, n=17), all_null=True)[0] == 0          # the compiled range is looked at later
    if name in KF_STEPS:
        assert _kf(name, dict(T=0), all_null=True)[0] == 0
    else:                                                                    # the single steps: T is not read
        assert _kf(name, dict(T=0), all_null=True) == (BAD_ARG, KF_ENTRY[name][2])
    # ... but not before desc is checked
    assert _kf(name, dict(N=0, layout=2), all_null=True) == (BAD_ARG, "bad layout")
    assert _kf(name, dict(N=0, flags=64), all_null=True) == (BAD_ARG, "unknown desc flag")


@pytest.mark.parametrize("name", sorted(KF_ENTRY))
def test_kf_missing_required_pointer(name, env):
    _, required, msg, _ = KF_ENTRY[name]
    for i in required:
        assert _kf(name, null=(i,)) == (BAD_ARG, msg), i
    # before the compiled range, unlike the newer families
    assert _kf(name, dict(n=17), null=required[:1]) == (BAD_ARG, msg)
    assert _kf(name, dict(layout=2), null=required) == (BAD_ARG, "bad layout")


@pytest.mark.parametrize("name", sorted(n for n in KF_ENTRY if KF_ENTRY[n][3]))
def test_kf_control_needs_B_and_u(name, env):
    b, u = KF_ENTRY[name][3]
    for null in ((b,), (u,), (b, u)):
        assert _kf(name, dict(nu=1), null=null) == (BAD_ARG, CONTROL)
        assert _kf(name, dict(nu=1, n=17), null=null) == (BAD_ARG, CONTROL)
    assert _kf(name, dict(nu=1), null=(0, b)) == (BAD_ARG, KF_ENTRY[name][2])


@pytest.mark.parametrize("name", sorted(n for n in KF_ENTRY if n != "fk_kf_rts_f64"))
@pytest.mark.parametrize("field", [dict(n=17), dict(m=9)], ids=["n17", "m9"])
def test_kf_dimensions_above_range(name, field, env):
    """After the pointer checks (the newer families refuse the range with desc)."""
    assert _kf(name, field) == (UNSUPPORTED, RANGE)
    assert _kf(name, dict(field, flags=2)) == (UNSUPPORTED, RANGE)


def test_kf_rts_refusals(env):
    name = "fk_kf_rts_f64"
    for conv in (-1, 2):
        assert _kf(name, conv=conv) == (BAD_ARG, "index_convention must be 0 or 1")
        assert _kf(name, dict(n=17), conv=conv) == (BAD_ARG, "index_convention must be 0 or 1")
    assert _kf(name, conv=2, null=(5,)) == (BAD_ARG, KF_ENTRY[name][2])
    for conv in (0, 1):
        assert _kf(name, dict(n=17), conv=conv) == (UNSUPPORTED, "dim_x outside the compiled range (<= 16)")
    # ... before the caller-supplied-inverse flags are looked at
    assert _kf(name, dict(n=17, flags=16 | 32)) == (UNSUPPORTED, "dim_x outside the compiled range (<= 16)")


def test_kf_update_given_inverse_refusals(env):
    """FK_KF_FLAG_S_ONLY (4) / FK_KF_FLAG_SI_GIVEN (8)."""
    name = "fk_kf_update_f64"
    assert _kf(name, dict(flags=12, n=17)) == (BAD_ARG, "FK_KF_FLAG_S_ONLY and FK_KF_FLAG_SI_GIVEN exclude each other")
    for null in ((UPD_Y,), (UPD_S,), (UPD_Y, UPD_S)):
        assert _kf(name, dict(flags=4, n=17), null=null) == (BAD_ARG, "FK_KF_FLAG_S_ONLY: y and S must not be NULL")
    assert _kf(name, dict(flags=8, m=9), null=(UPD_SI,)) == (BAD_ARG, "FK_KF_FLAG_SI_GIVEN: SI (the input) must not be NULL")
    for flags in (4, 8, 4 | 1):
        assert _kf(name, dict(flags=flags, n=17)) == (UNSUPPORTED, RANGE)
        assert _kf(name, dict(flags=flags, m=9)) == (UNSUPPORTED, RANGE)
    # a bank beyond one track window is refused, not cut: forced on a small bank
    env.setenv("FK_KF_WINDOW", "256")
    for flags in (4, 8):
        assert _kf(name, dict(flags=flags, N=257)) == (UNSUPPORTED, GIVEN_GUARD)
        assert _kf(name, dict(flags=flags, N=257, n=17)) == (UNSUPPORTED, RANGE)
        assert _kf(name, dict(flags=flags, N=257, layout=1)) == (UNSUPPORTED, GIVEN_GUARD)
    assert _kf(name, dict(flags=4, N=257), null=(0,)) == (BAD_ARG, KF_ENTRY[name][2])


def test_kf_rts_given_inverse_refusals(env):
    """FK_KF_FLAG_PP_ONLY (16) / FK_KF_FLAG_PPINV_GIVEN (32)."""
    name = "fk_kf_rts_f64"
    assert _kf(name, dict(flags=48)) == (BAD_ARG, "FK_KF_FLAG_PP_ONLY and FK_KF_FLAG_PPINV_GIVEN exclude each other")
    assert _kf(name, dict(flags=16), null=(RTS_PP,)) == (BAD_ARG, "FK_KF_FLAG_PP_ONLY: Pp must not be NULL")
    assert _kf(name, dict(flags=32), null=(RTS_K,)) == (BAD_ARG, "FK_KF_FLAG_PPINV_GIVEN: K (inverses in, gains out) must not be NULL")
    assert _kf(name, dict(flags=48), conv=2) == (BAD_ARG, "index_convention must be 0 or 1")
    env.setenv("FK_KF_WINDOW", "256")
    for flags in (16, 32):
        for layout in (0, 1):
            assert _kf(name, dict(flags=flags, N=257, layout=layout)) == (UNSUPPORTED, GIVEN_GUARD)
    assert _kf(name, dict(flags=16, N=257), null=(RTS_PP,)) == (BAD_ARG, "FK_KF_FLAG_PP_ONLY: Pp must not be NULL")


@pytest.mark.parametrize("name", KF_BATCH)
def test_kf_interleaved_refusals(name, env):
    """FK_KF_FLAG_COV_INTERLEAVED (2): one covariance history of two halves, for the call the specialised kernel serves."""
    four = IL + "batch_filter with all four outputs"
    for i in (MEANS, COVS, MEANS_P, COVS_P):
        assert _kf(name, dict(flags=2), null=(i,)) == (BAD_ARG, four), i
    place = IL + "covs_p must be covs + n*n (AOS) / covs + n*n*N (SOA)"
    assert _kf(name, dict(flags=2)) == (BAD_ARG, place)                                       # covs == covs_p
    for layout in (0, 1):
        other = _interleaved(2, 4, 1 - layout)
        assert _kf(name, dict(flags=2, layout=layout), at=other) == (BAD_ARG, place)
        assert _kf(name, dict(flags=2, layout=layout, n=9, m=3), at=_interleaved(2, 4, layout)) == (BAD_ARG, place)
    # two histories in one block: 2 * N * dim_x^2 * 8 bytes below 4 GiB -- (2, 1): from 2^26 tracks on
    guard = IL + "2 * N * dim_x^2 * 8 bytes must stay below 4 GiB"
    for layout in (0, 1):
        assert _kf(name, dict(flags=2, layout=layout, N=2 ** 26), at=_interleaved(2, 2 ** 26, layout)) == (UNSUPPORTED, guard)
    # the several-lane kernels take two arrays
    nine_three = IL + "(9,3) runs on the three-lane kernel, which takes two arrays"
    lanes = IL + "dim_x >= 9 runs on the several-lane kernels, which take two arrays"
    for layout in (0, 1):
        assert _kf(name, dict(flags=2, layout=layout, n=9, m=3), at=_interleaved(9, 4, layout)) == (UNSUPPORTED, nine_three)
        for n, m in ((9, 1), (9, 4), (10, 2), (16, 8)):
            assert _kf(name, dict(flags=2, layout=layout, n=n, m=m), at=_interleaved(n, 4, layout)) == (UNSUPPORTED, lanes)
    env.setenv("FK_ML9", "g")
    assert _kf(name, dict(flags=2, n=9, m=3), at=_interleaved(9, 4, 0)) == (UNSUPPORTED, lanes)
    env.delenv("FK_ML9")
    # every call that does not reach the specialised kernel
    served = IL + "not a call the specialised kernel serves"
    il = _interleaved(2, 4, 0)
    assert _kf(name, dict(flags=2 | 1), at=il) == (UNSUPPORTED, served)                       # FK_KF_FLAG_R_JOSEPH_DIAG
    assert _kf(name, dict(flags=2, n=9, m=5), at=_interleaved(9, 4, 0))[1] == lanes
    env.setenv("FK_NO_FAST", "1")
    assert _kf(name, dict(flags=2), at=il) == (UNSUPPORTED, served)
    assert _kf(name, dict(flags=2, n=9, m=3), at=_interleaved(9, 4, 0)) == (UNSUPPORTED, served)
    assert _kf(name, dict(flags=2, n=12, m=4), at=_interleaved(12, 4, 0)) == (UNSUPPORTED, served)
    env.delenv("FK_NO_FAST")
    env.setenv("FK_NO_MLG", "1")                                                              # (10, 2): no one-lane instantiation
    assert _kf(name, dict(flags=2, n=10, m=2), at=_interleaved(10, 4, 0)) == (UNSUPPORTED, served)


def test_kf_interleaved_extras_refusals(env):
    """The by-product histories with the interleaved flag: served by the one-lane kernel's plain call only."""
    name = "fk_kf_batch_filter_ex_f64"
    served = IL + "not a call the specialised kernel serves"
    il = _interleaved(2, 4, 0)
    assert _kf(name, dict(flags=2, nu=1), at=il, extras=True) == (UNSUPPORTED, served)
    assert _kf(name, dict(flags=2, update_first=1), at=il, extras=True) == (UNSUPPORTED, served)
    for mode in (1, 2, 3):
        assert _kf(name, dict(flags=2, model_mode=mode), at=il, extras=True) == (UNSUPPORTED, served)
    # (the four-lane kernels' EX instantiations do not take the flag: dim_x >= 10 has no other kernel with histories)
    assert _kf(name, dict(flags=2, n=10, m=2), at=_interleaved(10, 4, 0), extras=True) == (UNSUPPORTED, served)
    env.setenv("FK_NO_FAST_EX", "1")
    assert _kf(name, dict(flags=2), at=il, extras=True) == (UNSUPPORTED, served)


@pytest.mark.parametrize("name", ["fk_kf_predict_f64", "fk_kf_update_f64"])
def test_kf_interleaved_single_steps(name, env):
    assert _kf(name, dict(flags=2)) == (BAD_ARG, IL + "batch_filter with all four outputs")


IMM_PLAIN = dict(F=0, Q=1, H=2, R=3, M=4, z=5, xs=6, Ps=7, mu=8, x_prior=12, P_prior=13)
IMM_EX = dict(F=0, Q=1, H=2, R=3, M=4, z=5, zmask=6, ll0=7, nu=8, B=9, u=10, xs=11, Ps=12, mu=13, x_prior=17, P_prior=18)
IMM_ARG = "IMM: bad argument"


def _imm(name, desc=None, null=(), all_null=False, no_desc=False, nu=0, only=None):
    """One call of an IMM entry point with fake pointers; null: argument names.  only: the outputs that are not NULL."""
    from filterpy_amd import _abi
    lib = _abi.lib()
    fields = dict(n=2, m=1, n_models=2, layout=_abi.FK_LAYOUT_AOS, N=4, T=3, phase=0, flags=0)
    fields.update(desc or {})
    d = _abi.fk_imm_desc(**fields)
    ex = name == "fk_imm_batch_ex_f64"
    index = IMM_EX if ex else IMM_PLAIN
    ptrs = [None if all_null else ONE for _ in range(22 if ex else 17)]
    for k in null:
        if k in index:
            ptrs[index[k]] = None
    if only is not None:                                    # x, P, mu, x_prior, P_prior, likelihood: six outputs after mu
        for j in range(6):
            ptrs[index["mu"] + 1 + j] = ONE if j in only else None
    ptrs[-1] = None                                                            # stream
    if ex:
        ptrs[index["nu"]] = nu
    rc = getattr(lib, name)(None if no_desc else ctypes.byref(d), *ptrs)
    return rc, lib.fk_last_error().decode()


@pytest.mark.parametrize("name", ["fk_imm_batch_f64", "fk_imm_batch_ex_f64"])
def test_imm_refusals_in_order(name, env):
    """Every refusal of imm_dispatch.cpp, each with what comes after it made wrong as well; fk_imm_batch_f64 is the extended
    entry point without mask, ll0 and control input.  (The file's last fail(), "IMM: no kernel holds this bank", cannot be
    reached: the three kernel families cover every size the first check lets through.)"""
    size = "IMM: dim_x 1..16, dim_z 1..8, 2..16 models"
    assert _imm(name, no_desc=True) == (BAD_ARG, "desc is NULL")
    for field in (dict(n=0), dict(n=17), dict(m=0), dict(m=9), dict(n_models=1), dict(n_models=17)):
        assert _imm(name, dict(field, layout=2)) == (UNSUPPORTED, size)
    for layout in (2, -1):
        assert _imm(name, dict(layout=layout, phase=3)) == (BAD_ARG, "IMM: bad layout")
    for phase in (-1, 3):
        assert _imm(name, dict(phase=phase, N=-1)) == (BAD_ARG, "IMM: bad phase")
    assert _imm(name, dict(N=-1)) == (BAD_ARG, IMM_ARG)
    assert _imm(name, dict(T=-1)) == (BAD_ARG, IMM_ARG)
    for k in ("F", "Q", "H", "R", "M", "xs", "Ps", "mu", "z"):
        assert _imm(name, dict(N=2 ** 30), null=(k,)) == (BAD_ARG, IMM_ARG), k
    # MMAE has no transition matrix; a run of no steps and a predict need no measurement, an update does
    assert _imm(name, dict(flags=1, N=0), null=("M",))[0] == 0
    assert _imm(name, dict(T=0, N=0), null=("z",))[0] == 0
    assert _imm(name, dict(phase=1, N=0), null=("z",))[0] == 0
    assert _imm(name, dict(phase=2, N=0), null=("z",)) == (BAD_ARG, IMM_ARG)
    assert _imm(name, dict(phase=2, T=0), null=("z",)) == (BAD_ARG, IMM_ARG)
    # N * n_models * dim_x^2 * 8 bytes below 4 GiB: (2, 1) x 2 from 2^26 banks on
    guard = "IMM: record block >= 4 GiB, split the batch"
    assert _imm(name, dict(N=2 ** 26)) == (UNSUPPORTED, guard)
    assert _imm(name, dict(N=2 ** 25, n_models=4), only=(3,)) == (UNSUPPORTED, guard)
    # an empty bank is FK_OK once the pointers are there -- not before
    assert _imm(name, dict(N=0))[0] == 0
    assert _imm(name, dict(N=0), all_null=True) == (BAD_ARG, IMM_ARG)
    assert _imm(name, dict(N=0, flags=1), only=(3,))[0] == 0                   # (what follows is not looked at)
    # MMAE defines no priors
    mmae = "MMAE: prior outputs are not defined"
    assert _imm(name, dict(flags=1), only=(3,)) == (BAD_ARG, mmae)
    assert _imm(name, dict(flags=1), only=(4,)) == (BAD_ARG, mmae)
    assert _imm(name, dict(flags=1, phase=1)) == (BAD_ARG, mmae)


def test_imm_control_refusals(env):
    name = "fk_imm_batch_ex_f64"
    control = "IMM: control input needs 1 <= dim_u <= 4, B and u"
    for nu in (-1, 5):
        assert _imm(name, nu=nu) == (BAD_ARG, control)
    for null in (("B",), ("u",), ("B", "u")):
        assert _imm(name, nu=1, null=null) == (BAD_ARG, control)
        assert _imm(name, dict(flags=1), nu=4, null=null) == (BAD_ARG, control)      # before the MMAE rule
    assert _imm(name, dict(N=0), nu=9)[0] == 0                                       # after the empty bank
    assert _imm(name, dict(N=2 ** 26), nu=9) == (UNSUPPORTED, "IMM: record block >= 4 GiB, split the batch")


# ---------------------------------------------------------------------------------------------------------------------
# Which kernel family a valid call reaches.  Without a device the launch fails and its error names the family
# ("<family>: <HIP error>", FK_ERR_LAUNCH); with one the call would run on the fake pointers, so these tables are walked on
# device-less machines only.  They see the family, not the instantiation inside it.

def _family(rc, msg):
    assert rc == LAUNCH, (rc, msg)
    return msg.split(":")[0]


# (dim_x, dim_z, desc fields, outputs, mask, switch or None, family); outputs: "all" four, "none", "two" (means, covs)
KF_ROUTES = [
    (6, 3, {}, "all", False, None, "kf_fast_kernel"),
    (6, 3, {}, "all", True, None, "kf_fast_kernel"),
    (6, 3, {}, "none", False, None, "kf_fast_kernel"),
    (6, 3, {}, "two", False, None, "kf_kernel"),
    (6, 3, dict(model_mode=1), "all", False, None, "kf_fast_kernel"),
    (6, 3, dict(model_mode=2, layout=1), "all", False, None, "kf_fast_kernel"),
    (6, 3, dict(nu=2), "all", False, None, "kf_fast_kernel"),
    (6, 3, dict(update_first=1), "all", False, None, "kf_fast_kernel"),
    (6, 3, dict(flags=1), "all", False, None, "kf_kernel"),
    (6, 3, {}, "all", False, "FK_NO_FAST=1", "kf_kernel"),
    (4, 2, dict(flags=2), "all", False, None, "kf_fast_kernel (interleaved)"),      # (dim_x <= 4: both halves in one store)
    (6, 3, dict(flags=2), "all", False, None, "kf_fast_kernel"),
    (6, 3, dict(flags=2, layout=1), "all", True, None, "kf_fast_kernel"),
    (7, 4, {}, "all", False, None, "kf_fast_kernel"),
    (7, 4, dict(layout=1), "none", False, None, "kf_kernel"),
    (7, 4, dict(model_mode=1), "all", False, None, "kf_kernel"),
    (7, 4, dict(nu=2), "all", False, None, "kf_kernel"),
    (7, 4, dict(update_first=1), "all", False, None, "kf_kernel"),
    (7, 5, {}, "all", False, None, "kf_kernel"),
    (8, 4, dict(model_mode=3), "all", False, None, "kf_kernel"),
    (9, 3, {}, "all", False, None, "kf_ml_kernel"),
    (9, 3, dict(layout=1), "none", True, None, "kf_ml_kernel"),
    (9, 3, dict(model_mode=3), "all", False, None, "kf_ml_kernel<var>"),
    (9, 3, dict(nu=2), "all", False, None, "kf_ml_kernel<var>"),
    (9, 3, dict(update_first=1, layout=1), "all", True, None, "kf_ml_kernel<var>"),
    (9, 3, dict(model_mode=1), "all", False, None, "kf_kernel"),
    (9, 3, {}, "two", False, None, "kf_kernel"),
    (9, 3, {}, "all", False, "FK_NO_ML=1", "kf_fast_kernel"),
    (9, 3, {}, "all", False, "FK_ML9=g", "kf_mlg_kernel"),
    (9, 3, {}, "all", False, "FK_ML9=m", "kf_ml_kernel"),
    (9, 1, {}, "all", False, None, "kf_mlg_kernel"),
    (9, 1, {}, "all", False, "FK_ML9=m", "kf_fast_kernel"),
    (9, 1, {}, "all", False, "FK_NO_MLG=1", "kf_fast_kernel"),
    (9, 1, {}, "all", False, "FK_NO_ML=1", "kf_mlg_kernel"),
    (9, 4, dict(layout=1), "all", True, None, "kf_mlg_kernel"),
    (9, 5, {}, "all", False, None, "kf_kernel"),
    (10, 2, {}, "all", False, None, "kf_mlg_kernel"),
    (10, 2, {}, "none", False, None, "kf_kernel"),
    (10, 2, dict(model_mode=3), "all", False, None, "kf_mlg_kernel<var>"),
    (10, 2, dict(nu=2, layout=1), "all", True, None, "kf_mlg_kernel<var>"),
    (10, 2, dict(update_first=1), "all", False, None, "kf_mlg_kernel<var>"),
    (10, 2, dict(model_mode=2), "all", False, None, "kf_kernel"),
    (10, 2, {}, "all", False, "FK_NO_MLG=1", "kf_kernel"),
    (10, 2, {}, "all", False, "FK_NO_FAST=1", "kf_kernel"),
    (13, 4, {}, "all", False, None, "kf_mlg_kernel"),
    (14, 8, {}, "all", False, None, "kf_mlg_kernel"),
    (14, 8, dict(layout=1), "all", False, None, "kf_mlg_kernel"),
    (15, 1, dict(layout=1), "all", True, None, "kf_mlg_kernel"),
    (16, 8, dict(flags=1), "all", False, None, "kf_kernel"),
]

# the same call with the update's by-products as histories (fk_kf_batch_filter_ex_f64, extras given)
KF_EX_ROUTES = [
    (6, 3, {}, "all", False, None, "kf_fast_kernel (extras)"),
    (6, 3, dict(layout=1), "all", True, None, "kf_fast_kernel (extras)"),
    (6, 3, {}, "all", False, "FK_NO_FAST_EX=1", "kf_kernel"),
    (6, 3, {}, "all", False, "FK_NO_FAST=1", "kf_kernel"),
    (6, 3, {}, "none", False, None, "kf_kernel"),
    (6, 3, dict(nu=2), "all", False, None, "kf_kernel"),
    (6, 3, dict(model_mode=3), "all", False, None, "kf_kernel"),
    (7, 4, {}, "all", False, None, "kf_fast_kernel (extras)"),
    (9, 3, {}, "all", False, None, "kf_mlg_kernel<ex>"),
    (9, 3, {}, "all", True, None, "kf_fast_kernel (extras)"),
    (9, 3, {}, "all", False, "FK_NO_MLG_EX=1", "kf_fast_kernel (extras)"),
    (9, 3, {}, "all", False, "FK_NO_MLG=1", "kf_fast_kernel (extras)"),
    (9, 1, dict(layout=1), "all", False, None, "kf_mlg_kernel<ex>"),
    (10, 2, {}, "all", False, None, "kf_mlg_kernel<ex>"),
    (10, 2, {}, "all", True, None, "kf_kernel"),
    (10, 2, {}, "all", False, "FK_NO_MLG_EX=1", "kf_kernel"),
    (10, 2, {}, "all", False, "FK_NO_FAST_EX=1", "kf_kernel"),
    (15, 8, dict(layout=1), "all", False, None, "kf_mlg_kernel<ex>"),
    (15, 8, dict(update_first=1), "all", False, None, "kf_kernel"),
]

# (dim_x, desc fields, K and Pp given, switch or None, family)
RTS_ROUTES = [
    (6, {}, True, None, "rts_kernel"),
    (7, {}, True, None, "rts_kernel"),
    (8, {}, True, None, "rts_mlg_kernel"),
    (8, dict(layout=1), True, None, "rts_kernel"),
    (8, {}, True, "FK_ML9=m", "rts_kernel"),
    (8, {}, True, "FK_NO_MLG=1", "rts_kernel"),
    (8, {}, False, None, "rts_kernel"),
    (8, dict(model_mode=1), True, None, "rts_kernel"),
    (9, {}, True, None, "rts_mlg_kernel"),
    (9, dict(layout=1), True, None, "rts_ml_kernel"),
    (9, dict(layout=1), True, "FK_ML9=g", "rts_mlg_kernel"),
    (9, {}, True, "FK_ML9=m", "rts_ml_kernel"),
    (9, dict(layout=1), True, "FK_NO_ML=1", "rts_kernel"),
    (9, {}, True, "FK_NO_MLG=1", "rts_kernel"),
    (9, dict(layout=1, model_mode=3), True, None, "rts_kernel"),
    (10, {}, True, None, "rts_mlg_kernel"),
    (10, {}, True, "FK_RTS_LANES=8", "rts_mlg_kernel"),
    (10, dict(model_mode=2), True, None, "rts_kernel"),
    (13, {}, True, None, "rts_mlg_kernel"),
    (13, {}, True, "FK_RTS_LANES=8", "rts_mlx_kernel"),
    (14, {}, True, None, "rts_mlx_kernel"),
    (14, dict(layout=1), True, None, "rts_mlg_kernel"),
    (14, {}, True, "FK_RTS_LANES=4", "rts_mlg_kernel"),
    (15, dict(layout=1), True, None, "rts_mlx_kernel"),
    (15, {}, True, "FK_RTS_LANES=4", "rts_mlg_kernel"),
    (15, {}, True, "FK_NO_MLG=1", "rts_kernel"),
    (16, {}, False, None, "rts_kernel"),
]

# (dim_x, dim_z, models, desc fields, extended call: mask + ll0 + control, family)
IMM_ROUTES = [
    (2, 1, 2, {}, False, "imm_kernel"),
    (2, 1, 3, dict(layout=1), True, "imm_kernel"),
    (4, 2, 2, dict(flags=1), False, "imm_kernel"),
    (5, 2, 3, {}, False, "imm_kernel"),
    (6, 3, 3, dict(phase=1), False, "imm_kernel"),
    (6, 3, 4, {}, False, "imm_lanes_kernel"),
    (2, 1, 16, {}, True, "imm_lanes_kernel"),
    (7, 3, 2, {}, False, "imm_lanes_kernel"),
    (6, 4, 2, dict(layout=1), False, "imm_lanes_kernel"),
    (9, 4, 9, dict(flags=1), False, "imm_lanes_kernel"),
    (9, 5, 2, {}, False, "imm_quad_kernel"),
    (10, 1, 5, {}, True, "imm_quad_kernel"),
    (12, 4, 16, dict(phase=2), False, "imm_quad_kernel"),
    (13, 4, 3, {}, False, "imm_quad_kernel"),
    (16, 8, 2, {}, False, "imm_quad_kernel"),
    (16, 8, 2, dict(layout=1), True, "imm_quad_kernel"),
    (16, 8, 3, {}, False, "imm_quad_kernel"),
]


def _switch(env, switch):
    if switch:
        env.setenv(*switch.split("="))


def _batch_call(name, n, m, fields, outs, mask, extras=False):
    null = {"all": (), "none": (MEANS, COVS, MEANS_P, COVS_P), "two": (MEANS_P, COVS_P)}[outs] + (() if mask else (7,))
    d = dict(n=n, m=m, N=300, T=3, **fields)
    at = _interleaved(n, 300, d.get("layout", 0)) if d.get("flags", 0) & 2 else None
    return _family(*_kf(name, d, null=null, at=at, extras=extras))


def test_kf_batch_filter_reaches_family(env):
    import torch
    if torch.cuda.is_available():
        return
    for n, m, fields, outs, mask, switch, family in KF_ROUTES:
        with env.context() as e:
            _switch(e, switch)
            for name in KF_BATCH:                   # the extras entry point without extras is the plain one
                assert _batch_call(name, n, m, fields, outs, mask) == family, (name, n, m, fields, outs, mask, switch)


def test_kf_batch_filter_ex_reaches_family(env):
    import torch
    if torch.cuda.is_available():
        return
    for n, m, fields, outs, mask, switch, family in KF_EX_ROUTES:
        with env.context() as e:
            _switch(e, switch)
            got = _batch_call("fk_kf_batch_filter_ex_f64", n, m, fields, outs, mask, extras=True)
            assert got == family, (n, m, fields, outs, mask, switch)


def test_kf_single_steps_reach_family(env):
    """predict() and update() run on the general kernel at every size; a caller-supplied inverse on its own."""
    import torch
    if torch.cuda.is_available():
        return
    for n, m in ((1, 1), (6, 3), (7, 4), (9, 3), (10, 2), (16, 8)):
        for fields in ({}, dict(layout=1, model_mode=1), dict(nu=2)):
            d = dict(n=n, m=m, N=300, T=3, **fields)
            assert _family(*_kf("fk_kf_predict_f64", d)) == "kf_kernel", d
            assert _family(*_kf("fk_kf_update_f64", d)) == "kf_kernel", d
        for flags in (4, 8):
            assert _family(*_kf("fk_kf_update_f64", dict(n=n, m=m, N=300, flags=flags))) == "kf_given_kernel"
        for flags in (16, 32):
            assert _family(*_kf("fk_kf_rts_f64", dict(n=n, m=m, N=300, flags=flags))) == "rts_given_kernel"


def test_kf_rts_reaches_family(env):
    import torch
    if torch.cuda.is_available():
        return
    for n, fields, gains, switch, family in RTS_ROUTES:
        with env.context() as e:
            _switch(e, switch)
            for conv in (0, 1):
                got = _family(*_kf("fk_kf_rts_f64", dict(n=n, m=1, N=300, T=3, **fields), null=() if gains else (RTS_K, RTS_PP), conv=conv))
                assert got == family, (n, fields, gains, switch, conv)


def test_imm_reaches_family(env):
    import torch
    if torch.cuda.is_available():
        return
    for n, m, models, fields, extended, family in IMM_ROUTES:
        d = dict(n=n, m=m, n_models=models, N=300, T=3, **fields)
        only = (0, 1, 2) if fields.get("flags") else (0, 1, 2, 3, 4, 5)           # MMAE defines no priors
        if extended:
            assert _family(*_imm("fk_imm_batch_ex_f64", d, nu=2, only=only)) == family, d
        else:                                           # the plain entry point is the extended one without the extras
            assert _family(*_imm("fk_imm_batch_f64", d, only=only)) == family, d
            assert _family(*_imm("fk_imm_batch_ex_f64", d, null=("zmask", "ll0", "B", "u"), only=only)) == family, d
