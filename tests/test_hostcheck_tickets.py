"""The persistent ticket grids without a GPU: part 1 of csrc/fk_tickets.hpp -- what the launchers of kf_ml_kernel, rts_ml_kernel
and ukf_linear_kernel (6,3) ask before they allocate and launch (ticket_plan) and the split of a ticket that their kernels run
(ticket_window) -- compiled for the host (tests/hostcheck).  The plans are held against tests/golden/ticket_plans.json, recorded
from the three hand-written launchers before they were folded into one plan (their bodies on stubbed HIP calls:
docs/MEASUREMENTS.md)."""
import ctypes
import hashlib
import itertools
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

KF, RTS, UKF = range(3)
GROUP = {KF: 64, RTS: 64, UKF: 256}                       # tracks per group: a workgroup's
SWITCH = {KF: "FK_ML_PERSIST", RTS: "FK_RTS_PERSIST", UKF: "FK_UKF_PERSIST"}
ENVS = sorted(SWITCH.values()) + sorted(v + "_H" for v in SWITCH.values()) + ["FK_ML_SLAB"]
STEPS = (1, 2, 15, 16, 31, 32, 47, 48, 70, 100, 1000)
SWITCHES = (None, "0", "1", "2")
CHUNKS = (None, "0", "1", "2", "7", "T", "T+1")


@pytest.fixture(scope="module")
def hc(_helpers_built):
    lib = ctypes.CDLL(os.path.join(ROOT, "tests", "hostcheck", "libhostcheck.so"))
    lib.hc_ticket_plan.restype = ctypes.c_int
    lib.hc_ticket_plan.argtypes = [ctypes.c_int] + [ctypes.c_long] * 4 + [ctypes.c_int] * 3 + [ctypes.POINTER(ctypes.c_long)]
    lib.hc_ticket_windows.restype = None
    lib.hc_ticket_windows.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_long, ctypes.c_int, ctypes.POINTER(ctypes.c_long)]
    return lib


@pytest.fixture(autouse=True)
def _no_switches(monkeypatch):
    for name in ENVS:
        monkeypatch.delenv(name, raising=False)


def banks(family, n_cu):
    """(i0, cnt, N): track counts on both sides of the thresholds -- G = n_cu, n_cu + 1, 2 n_cu, 2 n_cu + 1 groups, the two that
    cross one also with a last group of a single track -- as a window of a larger bank, as the whole bank and, for the
    smoother, as its cnt == 0 form of the whole bank; the fused UKF also gets a prefix of a bank."""
    grp = GROUP[family]
    counts = [G * grp for G in (n_cu, n_cu + 1, 2 * n_cu, 2 * n_cu + 1)] + [n_cu * grp + 1, 2 * n_cu * grp + 1]
    out = []
    for cnt in counts:
        out += [(grp, cnt, grp + cnt + 11), (0, cnt, cnt)]
        if family == RTS:
            out.append((0, 0, cnt))
        if family == UKF:
            out.append((0, cnt, cnt + 11))
    return out


def grid():
    """Every call: (family, n_cu, i0, cnt, N, T, switch, chunk override, outs, aos, FK_ML_SLAB).  The cross product of the
    families, n_cu, banks(), STEPS, SWITCHES and CHUNKS for a forward call with outputs in NumPy order; then, for the forward
    filter, what its instantiations need beyond the policy: outputs x layout x FK_ML_SLAB unset / 0 / 1."""
    cases = []
    for family, n_cu in itertools.product((KF, RTS, UKF), (64, 256)):
        for (i0, cnt, N), T, switch, chunks in itertools.product(banks(family, n_cu), STEPS, SWITCHES, CHUNKS):
            cases.append((family, n_cu, i0, cnt, N, T, switch, chunks, 1, 1, None))
    for n_cu in (64, 256):
        for (i0, cnt, N), T, outs, aos, slab in itertools.product(banks(KF, n_cu), STEPS, (0, 1), (0, 1), (None, "0", "1")):
            cases.append((KF, n_cu, i0, cnt, N, T, None, None, outs, aos, slab))
    return cases


def plan(lib, monkeypatch, case):
    """[G, H, grid, ctl bytes, ws bytes] of a call the grid takes, 0 of one it does not"""
    family, n_cu, i0, cnt, N, T, switch, chunks, outs, aos, slab = case
    chunks = {None: None, "T": str(T), "T+1": str(T + 1)}.get(chunks, chunks)
    for name, value in ((SWITCH[family], switch), (SWITCH[family] + "_H", chunks), ("FK_ML_SLAB", slab)):
        if value is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, value)
    out = (ctypes.c_long * 6)()
    take = lib.hc_ticket_plan(family, i0, cnt, N, T, n_cu, outs, aos, out)
    assert take in (0, 1) and out[0] == take
    assert take or not any(out[1:])
    return list(out[1:]) if take else 0


def digest(cases):
    return hashlib.sha256(json.dumps(cases).encode()).hexdigest()


def test_plans_equal_the_golden(hc, monkeypatch):
    """take, G, H, grid, control bytes and hand-over bytes of every call of grid() equal what the parent's three launchers
    did with it."""
    with open(os.path.join(GOLDEN, "ticket_plans.json")) as fh:
        golden = json.load(fh)
    cases = grid()
    assert golden["cases"] == len(cases) == len(golden["plans"]) and golden["digest"] == digest(cases)
    taken = set()
    for case, want in zip(cases, golden["plans"]):
        got = plan(hc, monkeypatch, case)
        assert got == want, case
        if got:
            taken.add(case[:2] + (case[6], case[7]))
    # (the grid is not vacuous: every family starts a grid at both chip sizes under every switch value that turns it on and
    #  every chunk override that can pass)
    on = {KF: (None, "1", "2"), RTS: ("1", "2"), UKF: ("1",)}
    assert taken == {(f, n_cu, s, c) for f in on for n_cu in (64, 256) for s in on[f] for c in (None, "2", "7", "T", "T+1")
                     if not (f == UKF and c == "T+1") and not (f == RTS and c in ("T", "T+1"))}


def test_plans_the_comments_name(hc, monkeypatch):
    """BASELINE configs[2] (1e5 tracks x 100 steps: 1563 groups on 512 slots, three chunks) and the banks of the three GPU
    bit-identity tests (33 003 tracks: 516 groups against 512 slots)."""
    assert plan(hc, monkeypatch, (KF, 256, 0, 100000, 100000, 100, None, None, 1, 0, None)) == [1563, 3, 512, 6400, 72000000]
    assert plan(hc, monkeypatch, (KF, 256, 0, 100000, 100000, 100, "0", None, 1, 0, None)) == 0
    assert plan(hc, monkeypatch, (KF, 256, 0, 33003, 33003, 40, None, None, 1, 1, None)) == [516, 2, 512, 2304, 23762160]
    assert plan(hc, monkeypatch, (KF, 256, 0, 32768, 32768, 40, None, None, 1, 1, None)) == 0           # 512 groups: one round
    assert plan(hc, monkeypatch, (RTS, 256, 0, 0, 33003, 40, None, None, 1, 1, None)) == 0               # off unless asked for
    assert plan(hc, monkeypatch, (RTS, 256, 0, 0, 33003, 40, "1", None, 1, 1, None)) == [516, 2, 512, 2304, 23762160]
    assert plan(hc, monkeypatch, (RTS, 256, 0, 0, 150, 12, "1", None, 1, 1, None)) == 0
    assert plan(hc, monkeypatch, (UKF, 256, 0, 100000, 100000, 100, None, None, 1, 1, None)) == 0
    got = plan(hc, monkeypatch, (UKF, 256, 0, 100000, 100000, 100, "1", None, 1, 1, None))
    assert got[0] == 391 and 4 <= got[1] <= 16 and got[2] == 512 and got[3:] == [1792, 27 * 8 * 100000]
    assert plan(hc, monkeypatch, (UKF, 256, 0, 100000, 100000, 100, "1", "2", 1, 1, None))[:3] == [391, 2, 512]
    assert plan(hc, monkeypatch, (UKF, 256, 0, 66000, 66000, 32, "1", "2", 1, 1, None))[:3] == [258, 2, 512]
    assert plan(hc, monkeypatch, (UKF, 256, 0, 65536, 65536, 32, "1", "2", 1, 1, None)) == 0             # 256 groups: one per CU


def windows(lib, G, H, T, backward):
    out = (ctypes.c_long * (5 * G * H))()
    lib.hc_ticket_windows(G, H, T, int(backward), out)
    return np.array(out, dtype=np.int64).reshape(H, G, 5)           # [chunk drawn][group][g, chunk, t0, t1, cont]


def test_windows_tile_the_call(hc):
    """For every G <= 5 and H <= T <= 64, forward and backward: tickets 0 .. G H - 1 draw every (group, chunk) exactly once,
    chunk-major, so that a chunk's predecessor is the ticket G draws older; forward a group's windows tile [0, T) in order;
    backward they tile it from the end, every chunk but the first drawn continues from the step above its window -- the first
    step of its predecessor's window, which that one smoothed -- and runs one step more for it (RtsArgs::T of the chunk)."""
    for G, T, backward in itertools.product(range(1, 6), range(1, 65), (False, True)):
        for H in range(1, T + 1):
            w = windows(hc, G, H, T, backward)
            key = (G, H, T, backward)
            # ticket c * G + g is (group g, chunk c): each pair once, and ticket - G is the same group's chunk before
            assert (w[:, :, 0] == np.arange(G)[None, :]).all() and (w[:, :, 1] == np.arange(H)[:, None]).all(), key
            # every group gets the same windows
            assert (w[:, :, 2:] == w[:, :1, 2:]).all(), key
            t0, t1, cont = w[:, 0, 2], w[:, 0, 3], w[:, 0, 4]
            assert (t1 > t0).all(), key
            if not backward:
                assert t0[0] == 0 and t1[-1] == T and (t1[:-1] == t0[1:]).all() and not cont.any(), key
            else:
                assert t1[0] == T and t0[-1] == 0 and (t0[:-1] == t1[1:]).all(), key
                assert (cont == (np.arange(H) > 0)).all(), key
                steps = t1 - t0 + cont                              # what the smoother's kernel runs: records t0 .. t0 + steps - 1
                assert steps.sum() == T + H - 1 and (t0[1:] + steps[1:] - 1 == t0[:-1]).all(), key
