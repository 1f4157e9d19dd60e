"""CPU-side characterisation (no GPU) of what the dispatchers of the square-root filter, the information filter and the
fixed-lag smoother refuse: every refusal returns before any HIP call, so the return code and the exact fk_last_error() text
of each branch can be pinned without a device.  The seven entry points share one descriptor check, one record-block guard
and one B / u rule (csrc/fk_dispatch.hpp); what differs between the families -- the family name inside the messages, the
fields a family allows, the smoother's k0 and its narrower record -- is what the cases below hold still."""
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
