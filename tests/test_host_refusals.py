"""CPU-side characterisation (no GPU) of what the dispatchers of the square-root filter, the information filter and the
fixed-lag smoother refuse: every refusal returns before any HIP call, so the return code and the exact fk_last_error() text
of each branch can be pinned without a device.  The seven entry points share one descriptor check, one record-block guard
and one B / u rule (csrc/fk_dispatch.hpp); what differs between the families -- the family name inside the messages, the
fields a family allows, the smoother's k0 and its narrower record -- is what the cases below hold still.

The second half does the same for the entry points of the Kalman filter and the IMM estimator (csrc/kf_dispatch.cpp,
csrc/imm_dispatch.cpp, on the same scaffold): their refusals in the order the code makes them, and -- on machines without a
device only -- which kernel family a call that passes every check reaches.

The third part holds the unscented filter's entry points (csrc/ukf_dispatch.cpp) and the steady-state / correlated-noise
variants of the Kalman filter: eleven calls with rules of their own, oddities included."""
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


# ---------------------------------------------------------------------------------------------------------------------
# The unscented filter's entry points (csrc/ukf_dispatch.cpp) and the two Kalman filter variants that moved into
# csrc/kf_dispatch.cpp with them.  Their rules differ from the descriptor families above and from each other; every oddity
# below is what callers get (docs/MEASUREMENTS.md lists them as candidates for a bug-fix change) and is pinned as it is.

PAIR = 1                           # FK_UKF_FLAG_PAIR_WEIGHTS
# entry point -> (what precedes the pointers: "ukf" / "kf" descriptor, or the scalars of a valid small call in order;
#                 pointers after it, stream last; indices of the required ones; the words its messages start with)
U_ENTRY = {
    "fk_ukf_linear_batch_f64": ("ukf", 14, (0, 1, 2, 3, 4, 5, 6, 8, 9), "fused linear UKF"),
    "fk_ukf_linear_rts_f64": ("ukf", 11, (0, 1, 2, 3, 4, 5, 6, 7), "fused linear UKF smoother"),
    "fk_ut_sigma_points_f64": (dict(n=2, N=4, layout=0, scale=3.0), 5, (0, 1, 2), "sigma points"),
    "fk_ut_transform_f64": (dict(n=2, k=5, N=4, layout=0), 7, (0, 1, 2, 4, 5), "unscented transform"),
    "fk_ut_cross_variance_f64": (dict(n=2, m=1, k=5, N=4, layout=0), 7, (2, 3, 4, 5), "cross variance"),
    "fk_ut_linear_map_f64": (dict(n_in=2, n_out=1, k=5, N=4, layout=0), 4, (0, 1, 2), "linear map"),
    "fk_ukf_correct_f64": (dict(n=2, m=1, N=4, layout=0), 9, (0, 2, 3, 4, 5), "ukf correct"),
    "fk_ukf_rts_correct_f64": (dict(n=2, N=4, layout=0), 10, (0, 2, 3, 4, 5, 6), "ukf rts"),
    "fk_kf_steadystate_f64": ("kf", 12, (7,), "steady state"),
    "fk_kf_update_correlated_f64": ("kf", 13, (0, 1, 2, 3, 5, 6), "update_correlated"),
}
U_BLOCKS = sorted(n for n in U_ENTRY if isinstance(U_ENTRY[n][0], dict))          # the building blocks: scalar arguments
U_FUSED = ("fk_ukf_linear_batch_f64", "fk_ukf_linear_rts_f64")
U_VARIANTS = ("fk_kf_steadystate_f64", "fk_kf_update_correlated_f64")
# the range refusal of each building block (FK_ERR_UNSUPPORTED, also below 1) and the wrong values that draw it
U_RANGE = {
    "fk_ut_sigma_points_f64": ("sigma points: dim_x must be 1..16", [dict(n=0), dict(n=17)]),
    "fk_ut_transform_f64": ("unscented transform: dim must be 1..16", [dict(n=0), dict(n=17), dict(k=0)]),
    "fk_ut_cross_variance_f64": ("cross variance: dim_x must be 1..16", [dict(n=0), dict(n=17), dict(m=0), dict(k=0)]),
    "fk_ut_linear_map_f64": ("linear map: dims must be 1..16", [dict(n_in=0), dict(n_in=17), dict(n_out=0), dict(n_out=17), dict(k=0)]),
    "fk_ukf_correct_f64": ("ukf correct: dim_x 1..16, dim_z 1..8", [dict(n=0), dict(n=17), dict(m=0), dict(m=9)]),
    "fk_ukf_rts_correct_f64": ("ukf rts: dim_x 1..16", [dict(n=0), dict(n=17)]),
}
# the first track count each building block's record-block guard refuses: exactly 4 GiB, not 32 bytes short of it
U_FIRST = {
    "fk_ut_sigma_points_f64": (dict(n=1), 178956971),                  # 3 doubles per track: 2^32 / 24 rounded up
    "fk_ut_transform_f64": (dict(n=1, k=3), 178956971),
    "fk_ut_cross_variance_f64": (dict(n=1, m=3, k=1), 178956971),      # k * max(n, m)
    "fk_ut_linear_map_f64": (dict(n_in=1, n_out=3, k=1), 178956971),
    "fk_ukf_correct_f64": (dict(n=1, m=8), 2 ** 29),                   # n * n alone: the m x m and n x m records are not counted
    "fk_ukf_rts_correct_f64": (dict(n=1), 2 ** 29),
}
UKF_PAIR_FWD = ("fused linear UKF at dim_x 10..16: needs weights equal within every +- pair (FK_UKF_FLAG_PAIR_WEIGHTS; and "
                "FK_UKF_MLG != 0)")
UKF_PAIR_RTS = ("fused linear UKF smoother at dim_x 10..16: needs weights equal within every +- pair (FK_UKF_FLAG_PAIR_WEIGHTS; "
                "and FK_UKF_MLG != 0)")
UKF_DIMS_FWD = "fused linear UKF: dim_x 1..6 with dim_z 1..3, dim_x 7..9 with dim_z 1..4, dim_x 10..16 with dim_z 1..8"
UKF_DIMS_RTS = "fused linear UKF smoother: dim_x 1..9, 10..16"
# every environment variable these entry points and their launchers read
U_SWITCHES = ("FK_UKF_MLG", "FK_UKF_MLG_MIN_NX", "FK_UKF_MLG_RTS_MIN_NX", "FK_UKF_MLG_LANES", "FK_UKF_MLG_RTS_LANES", "FK_UKF_PADDED",
              "FK_UKF_PAIRED", "FK_UKF_DMA", "FK_UKF_SOA_PAIRS", "FK_UKF_CHUNKS", "FK_UKF_RTS_CHUNKS", "FK_UKF_PERSIST",
              "FK_UKF_PERSIST_H", "FK_UT_COOP", "FK_STEADY_ROLLED", "FK_STEADY_AOS_WAVES")


@pytest.fixture
def uenv(monkeypatch):
    for v in U_SWITCHES:
        monkeypatch.delenv(v, raising=False)
    return monkeypatch


def _u(name, over=None, null=(), all_null=False, no_desc=False):
    """One call with fake pointers; returns (code, last error).  over: the leading arguments that differ from a valid small
    call."""
    from filterpy_amd import _abi
    lib = _abi.lib()
    head, nptr = U_ENTRY[name][:2]
    over = dict(over or {})
    if head == "ukf":
        fields = dict(n=2, m=1, N=4, T=3, layout=_abi.FK_LAYOUT_AOS, flags=0, scale=3.0)
        fields.update(over)
        d = _abi.fk_ukf_desc(**fields)
        lead = [None if no_desc else ctypes.byref(d)]
    elif head == "kf":
        fields = dict(n=2, m=1, nu=0, model_mode=_abi.FK_MODEL_SHARED, N=4, T=3, layout=_abi.FK_LAYOUT_AOS, update_first=0,
                      alpha_sq=1.0, flags=0)
        fields.update(over)
        d = _abi.fk_kf_desc(**fields)
        lead = [None if no_desc else ctypes.byref(d)]
    else:
        assert set(over) <= set(head), over
        lead = [over.get(k, v) for k, v in head.items()]
    ptrs = [None if (all_null or i in null) else ONE for i in range(nptr)]
    ptrs[-1] = None                                                            # stream
    rc = getattr(lib, name)(*lead, *ptrs)
    return rc, lib.fk_last_error().decode()


def _bad(name):
    return U_ENTRY[name][3] + ": bad argument"


def _guard(name):
    return U_ENTRY[name][3] + ": record block >= 4 GiB" + ("" if name in U_VARIANTS + ("fk_ukf_rts_correct_f64",) else ", split the batch")


@pytest.mark.parametrize("name", U_FUSED + U_VARIANTS)
def test_u_null_desc(name, uenv):
    assert _u(name, no_desc=True) == (BAD_ARG, "desc is NULL")
    assert _u(name, no_desc=True, all_null=True) == (BAD_ARG, "desc is NULL")


def test_ukf_linear_supported_is_the_table_of_the_fused_calls(uenv):
    """No descriptor, no message: 1 where the fused call takes the size.  Sizes whose answer does not depend on the
    FK_UKF_MLG* switches (tests/test_host_logic.py gives those an interpreter each)."""
    from filterpy_amd import _abi
    q = _abi.lib().fk_ukf_linear_supported
    for flags in (0, PAIR, 2, PAIR | 2):
        for n in range(-1, 19):
            for m in range(-1, 11):
                small = (1 <= n <= 6 and 1 <= m <= 3) or (7 <= n <= 9 and 1 <= m <= 4)
                if not 10 <= n <= 16:
                    assert q(n, m, flags, 0) == int(small), (n, m, flags)
                    assert q(n, m, flags, 1) == int(1 <= n <= 9), (n, m, flags)            # the smoother does not read dim_z
                elif not flags & PAIR:
                    assert q(n, m, flags, 0) == 0 and q(n, m, flags, 1) == 0, (n, m, flags)
                elif not 1 <= m <= 8:
                    assert q(n, m, flags, 0) == 0, (n, m, flags)
    assert q(6, 3, 0, 7) == 1 and q(6, 4, 0, -1) == 1                                      # smoother: any nonzero value


def test_ukf_fused_refusals_in_order(uenv):
    fwd, rts = U_FUSED
    # the sizes: FK_ERR_UNSUPPORTED also below 1, and before anything else is looked at
    for over in (dict(n=0), dict(n=-1), dict(n=17), dict(m=0), dict(m=5), dict(n=6, m=4), dict(n=9, m=5), dict(n=10, m=9),
                 dict(n=16, m=0), dict(n=12, m=9, flags=PAIR)):
        assert _u(fwd, dict(over, N=-1), all_null=True) == (UNSUPPORTED, UKF_DIMS_FWD), over
    for over in (dict(n=0), dict(n=-1), dict(n=17), dict(n=17, flags=PAIR)):
        assert _u(rts, dict(over, N=-1), all_null=True) == (UNSUPPORTED, UKF_DIMS_RTS), over
    assert _u(rts, dict(n=9, m=0), null=(0,)) == (BAD_ARG, _bad(rts))                       # the smoother does not read dim_z
    # dim_x 10..16 without the pair-weight flag (any other bit does not count)
    for n in (10, 13, 16):
        for flags in (0, 2):
            assert _u(fwd, dict(n=n, m=8, flags=flags, T=-1), all_null=True) == (UNSUPPORTED, UKF_PAIR_FWD)
            assert _u(rts, dict(n=n, m=9, flags=flags, T=-1), all_null=True) == (UNSUPPORTED, UKF_PAIR_RTS)
    # N < 0, T < 0 and a missing pointer are one refusal, "bad argument"
    for name in U_FUSED:
        assert _u(name, dict(N=-1)) == (BAD_ARG, _bad(name))
        assert _u(name, dict(T=-1)) == (BAD_ARG, _bad(name))
        for i in U_ENTRY[name][2]:
            assert _u(name, null=(i,)) == (BAD_ARG, _bad(name)), (name, i)
        # layout is not looked at: with nothing to do any value is FK_OK
        for layout in (0, 1, 2, -1):
            assert _u(name, dict(layout=layout, N=0))[0] == 0
            assert _u(name, dict(layout=layout, T=0))[0] == 0
        # nothing to do is answered after the pointers, not before: an empty bank with NULL pointers is a bad argument
        assert _u(name, dict(N=0), all_null=True) == (BAD_ARG, _bad(name))
        assert _u(name, dict(T=0), all_null=True) == (BAD_ARG, _bad(name))
        optional = [i for i in range(U_ENTRY[name][1]) if i not in U_ENTRY[name][2]]
        assert _u(name, dict(N=0), null=optional)[0] == 0
        assert _u(name, dict(T=0), null=optional)[0] == 0


def test_ukf_fused_record_block_guards(uenv):
    """N * dim_x^2 * 8 bytes: the forward call refuses 32 bytes short of 4 GiB, the one-lane smoother at 4 GiB exactly; both
    after the pointers and before "nothing to do"."""
    fwd, rts = U_FUSED
    assert _u(fwd, dict(n=1, N=2 ** 29 - 4)) == (UNSUPPORTED, _guard(fwd))
    assert _u(fwd, dict(n=1, N=2 ** 29 - 4, T=0)) == (UNSUPPORTED, _guard(fwd))
    assert _u(fwd, dict(n=1, N=2 ** 29 - 5, T=0))[0] == 0
    assert _u(fwd, dict(n=6, m=3, N=14913081, T=0)) == (UNSUPPORTED, _guard(fwd))          # 288 bytes per track
    assert _u(fwd, dict(n=6, m=3, N=14913080, T=0))[0] == 0
    assert _u(fwd, dict(n=1, N=2 ** 29), null=(0,)) == (BAD_ARG, _bad(fwd))
    for flags in (0, PAIR):                                                                # dim_x 1 is never on several lanes
        assert _u(rts, dict(n=1, N=2 ** 29, flags=flags)) == (UNSUPPORTED, _guard(rts))
        assert _u(rts, dict(n=1, N=2 ** 29, T=0, flags=flags)) == (UNSUPPORTED, _guard(rts))
        assert _u(rts, dict(n=1, N=2 ** 29 - 1, T=0, flags=flags))[0] == 0
        assert _u(rts, dict(n=1, N=2 ** 29, flags=flags), null=(7,)) == (BAD_ARG, _bad(rts))
    assert _u(rts, dict(n=6, N=14913081, T=0)) == (UNSUPPORTED, _guard(rts))
    assert _u(rts, dict(n=6, N=14913080, T=0))[0] == 0


@pytest.mark.parametrize("name", U_BLOCKS)
def test_ut_block_refusals_in_order(name, uenv):
    """range (FK_ERR_UNSUPPORTED) -> [layout: fk_ukf_rts_correct_f64 only] -> N < 0 or a missing pointer ("bad argument") ->
    the 4 GiB guard -> nothing to do."""
    lead, nptr, required, _ = U_ENTRY[name]
    range_msg, wrong = U_RANGE[name]
    for over in wrong:
        assert _u(name, dict(over, N=-1, layout=2), all_null=True) == (UNSUPPORTED, range_msg), over
    if name == "fk_ukf_rts_correct_f64":
        for layout in (2, -1):
            assert _u(name, dict(layout=layout, N=-1), all_null=True) == (BAD_ARG, "ukf rts: bad layout")
    else:       # layout is not checked: whatever is not FK_LAYOUT_SOA runs the NumPy-order kernel
        for layout in (2, -1):
            assert _u(name, dict(layout=layout, N=0))[0] == 0
    assert _u(name, dict(N=-1)) == (BAD_ARG, _bad(name))
    for i in required:
        assert _u(name, null=(i,)) == (BAD_ARG, _bad(name)), i
    shape, first = U_FIRST[name]
    assert _u(name, dict(shape, N=first)) == (UNSUPPORTED, _guard(name))
    assert _u(name, dict(shape, N=2 ** 40)) == (UNSUPPORTED, _guard(name))
    assert _u(name, dict(shape, N=first), null=required[:1]) == (BAD_ARG, _bad(name))       # the pointers come first
    # nothing to do: FK_OK once the required pointers are there -- with every pointer NULL an empty bank is a bad argument
    optional = [i for i in range(nptr) if i not in required]
    assert _u(name, dict(N=0), null=optional)[0] == 0
    assert _u(name, dict(N=0), all_null=True) == (BAD_ARG, _bad(name))


def test_ut_block_oddities(uenv):
    # the transform reports k < 1 in the words of a dimension; cross variance has no upper bound on dim_z and k, and does not
    # ask for x and z (NULL: the caller applied its own residuals); the correction's zp, K and status are optional
    assert _u("fk_ut_transform_f64", dict(k=0)) == (UNSUPPORTED, "unscented transform: dim must be 1..16")
    assert _u("fk_ut_transform_f64", dict(k=-3, n=17)) == (UNSUPPORTED, "unscented transform: dim must be 1..16")
    assert _u("fk_ut_cross_variance_f64", dict(m=9, k=99, N=0))[0] == 0
    assert _u("fk_ut_cross_variance_f64", dict(N=0), null=(0, 1))[0] == 0
    assert _u("fk_ut_linear_map_f64", dict(k=99, N=0))[0] == 0
    assert _u("fk_ukf_correct_f64", dict(N=0), null=(1, 6, 7))[0] == 0
    assert _u("fk_ukf_rts_correct_f64", dict(N=0), null=(1, 7, 8))[0] == 0


@pytest.mark.parametrize("name", U_VARIANTS)
def test_kf_variant_refusals_in_order(name, uenv):
    """desc -> sizes (FK_ERR_UNSUPPORTED, also below 1) -> layout -> model mode -> "bad argument" -> the 4 GiB guard ->
    nothing to do."""
    words, steady = U_ENTRY[name][3], name == "fk_kf_steadystate_f64"
    sizes = words + (": dim_x 1..16, dim_z 1..8, dim_u 0..4" if steady else ": dim_x 1..16, dim_z 1..8")
    for over in (dict(n=0), dict(n=17), dict(m=0), dict(m=9)) + ((dict(nu=-1), dict(nu=5)) if steady else ()):
        assert _u(name, dict(over, layout=2, model_mode=2, N=-1), all_null=True) == (UNSUPPORTED, sizes), over
    if not steady:                                               # update_correlated does not read dim_u
        assert _u(name, dict(nu=-1, N=0))[0] == 0 and _u(name, dict(nu=5, N=0))[0] == 0
    for layout in (2, -1):
        assert _u(name, dict(layout=layout, model_mode=2, N=-1), all_null=True) == (BAD_ARG, words + ": bad layout")
    mode = words + (": K is shared or per track" if steady else ": M is shared or per track")
    for m in (2, 3, -1, 4):
        assert _u(name, dict(model_mode=m, N=-1), all_null=True) == (UNSUPPORTED, mode)
    assert _u(name, dict(model_mode=1, N=0))[0] == 0
    assert _u(name, dict(N=-1)) == (BAD_ARG, _bad(name))
    for i in U_ENTRY[name][2]:
        assert _u(name, null=(i,)) == (BAD_ARG, _bad(name)), i
    # the guard: N * dim_x * dim_z (steady state) / N * dim_x^2 (update_correlated) * 8 bytes, 4 GiB exactly, after the pointers
    first = 2 ** 28 if steady else 2 ** 27
    assert _u(name, dict(N=first)) == (UNSUPPORTED, _guard(name))
    assert _u(name, dict(N=first), null=U_ENTRY[name][2][:1]) == (BAD_ARG, _bad(name))
    # nothing to do, after the pointers; alpha_sq, update_first and flags are not read
    assert _u(name, dict(N=0, alpha_sq=2.0, update_first=1, flags=255))[0] == 0
    assert _u(name, dict(N=0), all_null=True) == (BAD_ARG, _bad(name))
    if steady:
        assert _u(name, dict(T=-1)) == (BAD_ARG, _bad(name))
        assert _u(name, dict(T=0))[0] == 0
        assert _u(name, dict(T=0, N=first)) == (UNSUPPORTED, _guard(name))
    else:                                                        # one step: T is not read
        assert _u(name, dict(T=-1, N=0))[0] == 0
        assert _u(name, dict(T=0), null=(0,)) == (BAD_ARG, _bad(name))


def test_kf_steadystate_argument_rule(uenv):
    """F H K B u z mask x means means_p y_out: x always; F (predict) or z (update) or both; an update needs H and K; a
    predict with dim_u > 0 needs B and u."""
    name = "fk_kf_steadystate_f64"
    F, H, K, B, U, Z = 0, 1, 2, 3, 4, 5
    bad = (BAD_ARG, _bad(name))
    assert _u(name, dict(N=0), null=(F, Z)) == bad
    assert _u(name, dict(N=0), null=(H,)) == bad
    assert _u(name, dict(N=0), null=(K,)) == bad
    assert _u(name, dict(N=0, nu=1), null=(B,)) == bad
    assert _u(name, dict(N=0, nu=4), null=(U,)) == bad
    assert _u(name, dict(N=0), null=(F, B, U, 6, 8, 9, 10))[0] == 0                         # update alone
    assert _u(name, dict(N=0, nu=2), null=(F, B, U))[0] == 0                               # ... needs no control input
    assert _u(name, dict(N=0), null=(Z, H, K, B, U))[0] == 0                               # predict alone
    assert _u(name, dict(N=0, nu=2), null=(Z, H, K))[0] == 0


# Which kernel family a valid call reaches, on device-less machines (see above).  The routing switches of these entry points
# are read once per process, so every setting walks its table in an interpreter of its own.

def _route_call(name, over, null=()):
    return list(_u(name, over, null=null))


def _walk(calls, switches):
    """[(name, over, null)] -> [(code, family or message)] from a fresh interpreter with only `switches` set."""
    import json
    import os
    import subprocess
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    code = ("import json, sys; sys.path[:0] = [%r, %r]; import test_host_refusals as t; "
            "print(json.dumps([t._route_call(*c) for c in json.load(sys.stdin)]))" % (os.path.dirname(here), here))
    e = {k: v for k, v in os.environ.items() if k not in U_SWITCHES}
    e.update(switches)
    out = subprocess.run([sys.executable, "-c", code], input=json.dumps(calls), capture_output=True, text=True, env=e, check=True)
    return [(rc, msg.split(":")[0] if rc == LAUNCH else msg if rc else "") for rc, msg in json.loads(out.stdout.splitlines()[-1])]


def _no_device():
    import torch
    return not torch.cuda.is_available()


FWD, RTS = "ukf_linear_kernel", "ukf_linear_rts_kernel"
QUAD, OCT = "ukf_mlg_kernel", "ukf_mlg_kernel<8 lanes>"
RQUAD, ROCT = "ukf_mlg_rts_kernel", "ukf_mlg_rts_kernel<8 lanes>"
NO_F, NO_R, PAIR_F, PAIR_R = (UKF_DIMS_FWD,) * 2, (UKF_DIMS_RTS,) * 2, (UKF_PAIR_FWD,) * 2, (UKF_PAIR_RTS,) * 2
# the first N with N * dim_x^2 * 8 >= 4 GiB, for the smoother's guards on its two routes
RTS_FIRST = {7: 10956550, 9: 6628036, 10: 5368710, 16: 2 ** 21}
_BAD, _GUARD = (BAD_ARG, "fused linear UKF smoother: bad argument"), (UNSUPPORTED, "fused linear UKF smoother: record block >= 4 GiB, split the batch")
_PAIR, _OK = (UNSUPPORTED, UKF_PAIR_RTS), (0, "")
# Per setting of the switches (one interpreter each; switches that do not meet share one):
#   fwd:    (dim_x, dim_z) -> what the fused forward call reaches (without, with the pair-weight flag), both layouts alike
#   rts:    dim_x -> the same for the fused smoother
#   guards: the smoother at RTS_FIRST[dim_x] tracks with F NULL, dim_x 7, 9, 10, 16 x (without, with the flag) -- where it runs
#           on several lanes per track the guard sits in front of the pointer checks (and 32 bytes short of 4 GiB; no
#           N * dim_x^2 * 8 falls into those 32 bytes for dim_x >= 7), on the one-lane route behind them --, then the four sizes one
#           track below with the flag, every pointer there and T = 0
UKF_ROUTES = {
    "": dict(
        fwd={(6, 3): (FWD, FWD), (6, 4): NO_F, (7, 4): (FWD, FWD), (9, 4): (FWD, FWD), (9, 5): NO_F, (10, 1): (UKF_PAIR_FWD, QUAD),
             (12, 8): (UKF_PAIR_FWD, QUAD), (13, 4): (UKF_PAIR_FWD, QUAD), (13, 5): (UKF_PAIR_FWD, OCT), (16, 8): (UKF_PAIR_FWD, OCT),
             (17, 1): NO_F},
        rts={6: (RTS, RTS), 7: (RTS, RQUAD), 9: (RTS, RQUAD), 10: (UKF_PAIR_RTS, RQUAD), 12: (UKF_PAIR_RTS, RQUAD),
             13: (UKF_PAIR_RTS, ROCT), 16: (UKF_PAIR_RTS, ROCT), 17: NO_R},
        guards=[_BAD, _GUARD, _BAD, _GUARD, _PAIR, _GUARD, _PAIR, _GUARD] + [_OK] * 4),
    "FK_UKF_MLG=0": dict(
        fwd={(6, 3): (FWD, FWD), (9, 4): (FWD, FWD), (10, 1): PAIR_F, (16, 8): PAIR_F, (16, 9): NO_F},
        rts={6: (RTS, RTS), 7: (RTS, RTS), 9: (RTS, RTS), 10: PAIR_R, 16: PAIR_R, 17: NO_R},
        guards=[_BAD] * 4 + [_PAIR] * 4 + [_OK, _OK, _PAIR, _PAIR]),
    "FK_UKF_MLG_MIN_NX=7 FK_UKF_MLG_RTS_MIN_NX=10 FK_UT_COOP=0 FK_STEADY_ROLLED=1": dict(
        fwd={(6, 3): (FWD, FWD), (7, 4): (FWD, QUAD), (9, 4): (FWD, QUAD), (9, 5): NO_F, (10, 1): (UKF_PAIR_FWD, QUAD)},
        rts={7: (RTS, RTS), 9: (RTS, RTS), 10: (UKF_PAIR_RTS, RQUAD)},
        guards=[_BAD] * 4 + [_PAIR, _GUARD, _PAIR, _GUARD] + [_OK] * 4),
    "FK_UKF_MLG_MIN_NX=9 FK_UKF_MLG_RTS_MIN_NX=9 FK_UKF_PADDED=1 FK_UKF_DMA=0 FK_UT_COOP=1 FK_STEADY_AOS_WAVES=3": dict(
        fwd={(6, 3): (FWD, FWD), (7, 4): (FWD, FWD), (9, 4): (FWD, QUAD), (10, 1): (UKF_PAIR_FWD, QUAD)},
        rts={6: (RTS, RTS), 7: (RTS, RTS), 9: (RTS, RQUAD)},
        guards=[_BAD, _BAD, _BAD, _GUARD, _PAIR, _GUARD, _PAIR, _GUARD] + [_OK] * 4),
    "FK_UKF_MLG_MIN_NX=7 FK_UKF_PAIRED=0 FK_STEADY_AOS_WAVES=1": dict(
        fwd={(6, 3): (FWD, FWD), (7, 4): (FWD, FWD), (9, 4): (FWD, FWD), (10, 1): (UKF_PAIR_FWD, QUAD), (16, 8): (UKF_PAIR_FWD, OCT)},
        rts={6: (RTS, RTS), 7: (RTS, RTS), 9: (RTS, RTS), 10: (UKF_PAIR_RTS, RQUAD)},
        guards=[_BAD] * 4 + [_PAIR, _GUARD, _PAIR, _GUARD] + [_OK] * 4),
    "FK_UKF_MLG_LANES=4 FK_UKF_MLG_RTS_LANES=4": dict(
        fwd={(13, 5): (UKF_PAIR_FWD, QUAD), (16, 8): (UKF_PAIR_FWD, QUAD)},
        rts={9: (RTS, RQUAD), 16: (UKF_PAIR_RTS, RQUAD)},
        guards=[_BAD, _GUARD, _BAD, _GUARD, _PAIR, _GUARD, _PAIR, _GUARD] + [_OK] * 4),
    "FK_UKF_MLG_LANES=8 FK_UKF_MLG_RTS_LANES=8": dict(
        fwd={(9, 4): (FWD, FWD), (10, 1): (UKF_PAIR_FWD, OCT)},
        rts={7: (RTS, RQUAD), 9: (RTS, ROCT), 10: (UKF_PAIR_RTS, ROCT)},
        guards=[_BAD, _GUARD, _BAD, _GUARD, _PAIR, _GUARD, _PAIR, _GUARD] + [_OK] * 4),
}


def _block_routes(coop):
    """The building blocks and the two variants: (entry point, leading arguments, family).  coop: FK_UT_COOP is not 0."""
    r = []
    for layout in (0, 1, 2):            # 2: not a layout; whatever is not element-major runs the NumPy-order kernel
        for n in (1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 12, 13, 16):
            tile = coop and layout == 0 and n in (2, 4, 6)
            r.append(("fk_ut_sigma_points_f64", dict(n=n, N=300, layout=layout), "sigma_coop_kernel" if tile else "sigma_kernel"))
            for k in (2 * n + 1, 2 * n, 1):
                standard = k == 2 * n + 1 and n in (2, 4, 6)
                family = "ut_coop_kernel" if tile and standard else "ut_reg_kernel" if standard else "ut_kernel"
                r.append(("fk_ut_transform_f64", dict(n=n, k=k, N=300, layout=layout), family))
            for m in (1, 4, 5, 8):
                r.append(("fk_ut_cross_variance_f64", dict(n=n, m=m, k=2 * n + 1, N=300, layout=layout), "cross_kernel"))
                r.append(("fk_ut_linear_map_f64", dict(n_in=n, n_out=m, k=2 * n + 1, N=300, layout=layout), "linear_map_kernel"))
                r.append(("fk_ut_linear_map_f64", dict(n_in=m, n_out=n, k=2 * n, N=300, layout=layout), "linear_map_kernel"))
                r.append(("fk_ukf_correct_f64", dict(n=n, m=m, N=300, layout=layout), "ukf_correct_kernel"))
            if layout < 2:
                r.append(("fk_ukf_rts_correct_f64", dict(n=n, N=300, layout=layout), "ukf_rts_kernel"))
    for layout in (0, 1):
        for n, m in ((2, 1), (2, 2), (4, 2), (6, 3), (6, 4), (9, 3), (9, 4), (10, 4), (9, 5), (12, 8), (13, 1), (16, 8)):
            for mode in (0, 1):
                r.append(("fk_kf_steadystate_f64", dict(n=n, m=m, N=300, layout=layout, model_mode=mode), "steady_kernel"))
                r.append(("fk_kf_steadystate_f64", dict(n=n, m=m, nu=2, N=300, layout=layout, model_mode=mode), "steady_kernel"))
                r.append(("fk_kf_update_correlated_f64", dict(n=n, m=m, N=300, layout=layout, model_mode=mode), "corr_update_kernel"))
    # one track below the first count a guard refuses the call reaches its launch: the building blocks' guards sit at 4 GiB
    # exactly (at 3 doubles per track that block ends 16 bytes short of 4 GiB, which a guard 32 bytes short would refuse)
    r += [(name, dict(U_FIRST[name][0], N=U_FIRST[name][1] - 1), None) for name in U_BLOCKS]
    r += [("fk_kf_steadystate_f64", dict(N=2 ** 28 - 1), None), ("fk_kf_update_correlated_f64", dict(N=2 ** 27 - 1), None)]
    return r


@pytest.mark.parametrize("switches", sorted(UKF_ROUTES))
def test_ukf_and_variants_reach_family(switches):
    if not _no_device():
        return
    fwd, rts, blocks = "fk_ukf_linear_batch_f64", "fk_ukf_linear_rts_f64", _block_routes("FK_UT_COOP=0" not in switches)
    t = UKF_ROUTES[switches]
    kf = [(nm, layout, flags) for nm in sorted(t["fwd"]) for layout in (0, 1) for flags in (0, PAIR)]
    kr = [(n, layout, flags, gains) for n in sorted(t["rts"]) for layout in (0, 1) for flags in (0, PAIR) for gains in (True, False)]
    calls = [(fwd, dict(n=n, m=m, N=300, layout=layout, flags=flags)) for (n, m), layout, flags in kf]
    calls += [(rts, dict(n=n, N=300, layout=layout, flags=flags), () if gains else (8, 9)) for n, layout, flags, gains in kr]
    calls += [(rts, dict(n=n, N=N, flags=flags), (0,)) for n, N in sorted(RTS_FIRST.items()) for flags in (0, PAIR)]
    calls += [(rts, dict(n=n, N=N - 1, flags=PAIR, T=0)) for n, N in sorted(RTS_FIRST.items())]
    calls += [(name, over) for name, over, _ in blocks]
    got = _walk(calls, dict(s.split("=") for s in switches.split()))
    code = lambda family: (UNSUPPORTED if family.startswith("fused") else LAUNCH, family)         # noqa: E731
    want = [code(t["fwd"][nm][flags]) for nm, layout, flags in kf] + [code(t["rts"][n][flags]) for n, layout, flags, gains in kr]
    want += t["guards"]
    want += [(LAUNCH, family) for _, _, family in blocks]
    got = [(rc, w[1] if w[1] is None else msg) for (rc, msg), w in zip(got, want)]               # (None: any family)
    assert got == want, [(c, g, w) for c, g, w in zip(calls, got, want) if g != w]


def test_ukf_chunked_calls_without_a_device(uenv):
    """FK_UKF_CHUNKS / FK_UKF_RTS_CHUNKS are read per call.  Without a device there are no helper streams: the call is one
    launch, which fails like any other."""
    if not _no_device():
        return
    for chunks in ("2,2", "4,3", "1,1", "nonsense"):
        uenv.setenv("FK_UKF_CHUNKS", chunks)
        uenv.setenv("FK_UKF_RTS_CHUNKS", chunks)
        for layout in (0, 1):
            rc, msg = _u("fk_ukf_linear_batch_f64", dict(n=6, m=3, N=2048, T=8, layout=layout))
            assert (rc, msg.split(":")[0]) == (LAUNCH, FWD), chunks
            rc, msg = _u("fk_ukf_linear_rts_f64", dict(n=6, N=2048, T=8, layout=layout))
            assert (rc, msg.split(":")[0]) == (LAUNCH, RTS), chunks
    uenv.delenv("FK_UKF_RTS_CHUNKS")
    rc, msg = _u("fk_ukf_linear_rts_f64", dict(n=6, N=100000, T=100))       # the default policy's shape: 1563 waves, 1024 slots
    assert (rc, msg.split(":")[0]) == (LAUNCH, RTS)
