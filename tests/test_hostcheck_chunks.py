"""Chunked calls without a GPU: csrc/fk_chunk_plan.hpp -- the policy, the enumeration of a call's pieces and the driver that
libfilterhip runs on HIP streams -- compiled for the host (tests/hostcheck) and run on lanes that record every fork, wait,
piece and join.  The argument blocks carry the member names of KfArgs, RtsArgs, ImmArgs, UkfRtsArgs and UkfArgs; member
number k points at k * 1e9, so a piece's pointers read as element offsets (NULL: -1)."""
import ctypes
import itertools
import json
import os

import pytest

from conftest import GOLDEN, ROOT

KF, RTS, IMM, UKF_RTS, UKF = range(5)
SWITCH = {KF: "FK_ML_CHUNKS", RTS: "FK_ML_CHUNKS", IMM: "FK_IMM_CHUNKS", UKF_RTS: "FK_UKF_RTS_CHUNKS", UKF: "FK_UKF_CHUNKS"}
BACKWARD = (RTS, UKF_RTS)
FORK, WAIT, PIECE, JOIN = range(4)
N_PTRS = {KF: 18, RTS: 6, IMM: 10, UKF_RTS: 5, UKF: 4}
BASE = 10 ** 9
SWITCHES = sorted(set(SWITCH.values())) + ["FK_ML_NO_STAGGER"]


@pytest.fixture(scope="module")
def hc(_helpers_built):
    lib = ctypes.CDLL(os.path.join(ROOT, "tests", "hostcheck", "libhostcheck.so"))
    lib.hc_chunk_trace.restype = ctypes.c_long
    lib.hc_chunk_trace.argtypes = [ctypes.c_int, ctypes.POINTER(ctypes.c_long), ctypes.c_uint, ctypes.c_long,
                                   ctypes.POINTER(ctypes.c_long), ctypes.c_long]
    return lib


@pytest.fixture(autouse=True)
def _no_switches(monkeypatch):
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)


def bits(*members):
    return sum(1 << k for k in members)


def make_case(family, tracks, steps, i0=0, whole_bank=False, slots=1024, n=9, m=3, status_or=0, null=0, extra=(),
              switch=None, no_stagger=False):
    """One call: `tracks` tracks from i0 of a bank of i0 + tracks + 11 (whole_bank: the smoother's cnt == 0 form) over
    `steps` steps (a smoother of steps + 1 records); extra: what the family's call takes beyond that (hc_chunk_trace)."""
    N = tracks if whole_bank else i0 + tracks + 11
    T = steps + 1 if family in BACKWARD else steps
    cfg = [N, T, 0 if whole_bank else i0, 0 if whole_bank else tracks, status_or, slots, n, m] + list(extra)
    return {"family": family, "switch": switch, "no_stagger": no_stagger, "cfg": cfg, "null": null}


def kf_extra(N, n, tracks_per_wave=16, quantum=64, model_t=0, nu=0, extras_per_step=0, interleaved=False):
    return [tracks_per_wave, quantum, model_t, nu, extras_per_step, (2 if interleaved else 1) * N * n * n]


def run(hc, monkeypatch, case, fail_at=-1):
    """(what the call returned, the rows of its trace)"""
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    if case["switch"] is not None:
        monkeypatch.setenv(SWITCH[case["family"]], case["switch"])
    if case["no_stagger"]:
        monkeypatch.setenv("FK_ML_NO_STAGGER", "1")
    cfg = (ctypes.c_long * 16)(*case["cfg"])
    out = (ctypes.c_long * 8192)()
    n = hc.hc_chunk_trace(case["family"], cfg, case["null"], fail_at, out, len(out))
    assert 1 <= n <= len(out), n
    return out[0], list(out[1:n])


def rows(family, flat):
    width = {FORK: 1, WAIT: 2, JOIN: 2, PIECE: 7 + N_PTRS[family]}
    out, k = [], 0
    while k < len(flat):
        out.append(tuple(flat[k:k + width[flat[k]]]))
        k += width[flat[k]]
    assert k == len(flat)
    return out


def grid():
    """Forced decompositions: every (G, H) of G = 1..5 x H in {1, 2, 3, 5, L, 70}, twice, with L and the tracks rotating
    through {1, 2, 3, 16, 19, 23} and {130, 777, 1000, 1024, quantum * G - 1}; the optional members, the window's start and
    the families' own arguments vary with the case's number.  300 cases."""
    Ls, Hs = (1, 2, 3, 16, 19, 23), ("1", "2", "3", "5", "L", "70")
    cases = []
    for family in range(5):
        for sweep, (idx, ((iG, G), (iH, Hname))) in itertools.product(
                range(2), enumerate(itertools.product(enumerate(range(1, 6)), enumerate(Hs)))):
            idx += 30 * sweep
            L = Ls[(iG + iH + 3 * sweep) % 6]
            kf_fast = family == KF and idx % 5 == 0
            quantum = 64 if family in (KF, RTS) and not kf_fast else 256
            tracks = (130, 777, 1000, 1024, quantum * min(G, 4) - 1)[(iG + 2 * iH + sweep) % 5]
            i0 = (37, 256, 0)[idx % 3]
            n, m = ((9, 3), (7, 4))[idx % 2]
            kw = dict(i0=i0, n=n, m=m, status_or=int(idx % 4 == 3), no_stagger=idx % 7 == 3,
                      switch="%d,%s" % (G, L if Hname == "L" else Hname))
            if family == KF:
                nu = 2 if idx & 2 else 0
                null = (0, bits(7, 10, 11, 13, 15, 17))[idx // 2 % 2] | (0 if nu else bits(4, 5))
                extra = kf_extra(i0 + tracks + 11, n, 64 if kf_fast else 16, quantum, idx & 1, nu, idx >> 2 & 1, idx % 3 == 0)
                cases.append(make_case(KF, tracks, L, null=null, extra=extra, **kw))
            elif family == RTS:
                cases.append(make_case(RTS, tracks, L, whole_bank=idx % 4 == 1, null=(0, bits(4), bits(5), bits(4, 5))[idx // 2 % 4], **kw))
            elif family == IMM:
                null = (bits(1, 3), 0, bits(2, 7, 8, 9), bits(1), bits(1, 3, 4, 5), bits(3))[idx % 6]   # the last: masked, no ll0
                cases.append(make_case(IMM, tracks, L, null=null, extra=[3, 2 * (idx & 1)], **kw))
            elif family == UKF_RTS:
                cases.append(make_case(UKF_RTS, tracks, L, null=(0, bits(4))[idx // 2 % 2], extra=[int(idx % 3 == 0)], **kw))
            else:
                cases.append(make_case(UKF, tracks, L, null=(0, bits(1), bits(3), bits(1, 2))[idx % 4], **kw))
    return cases


@pytest.fixture(scope="module")
def golden_traces():
    with open(os.path.join(GOLDEN, "chunk_pieces.json")) as fh:
        return json.load(fh)["cases"]


def test_pieces_equal_the_golden_trace(hc, monkeypatch, golden_traces):
    """Every fork, wait, piece (stream, track window, steps, flags, every pointer) and join of the forced decompositions, in
    order, equals what the five hand-written drivers did before they were folded into one (tests/golden/chunk_pieces.json,
    recorded from those drivers on stubbed HIP calls: docs/MEASUREMENTS.md)."""
    cases = grid()
    assert [{k: v for k, v in g.items() if k not in ("rc", "trace")} for g in golden_traces] == cases
    cut = set()
    for case, g in zip(cases, golden_traces):
        rc, flat = run(hc, monkeypatch, case)
        assert (rc, flat) == (g["rc"], g["trace"]), case
        if flat[0] == FORK:
            cut.add((case["family"], case["switch"].split(",")[0]))
    # (the grid is not vacuous: every family is cut at every forced G; the rest are the one-launch cases -- "1,1", too
    #  few tracks, masked without ll0)
    assert cut == {(family, str(G)) for family in range(5) for G in range(1, 6)}


def test_pieces_tile_the_call(hc, monkeypatch):
    """In every trace the pieces of a group tile its tracks x steps rectangle exactly once and in order (a backward piece
    starts at the step that the piece before it ended with and shares it); the groups partition [i0, i0 + cnt) in
    multiples of the quantum; the optional members that are NULL stay NULL."""
    for case in grid():
        family, cfg = case["family"], case["cfg"]
        rc, flat = run(hc, monkeypatch, case)
        assert rc == 0
        tr = rows(family, flat)
        N, T, n, m = cfg[0], cfg[1], cfg[6], cfg[7]
        i0, cnt = (cfg[2], cfg[3]) if cfg[3] else (0, N)
        back = family in BACKWARD
        L = T - 1 if back else T
        quantum = cfg[9] if family == KF else 64 if family == RTS else 256
        nulls = [k for k in range(N_PTRS[family]) if case["null"] >> k & 1]
        pieces = [r for r in tr if r[0] == PIECE]
        assert all(r[7 + k] == -1 for r in pieces for k in nulls), case
        if tr[0][0] != FORK:                        # one launch: the call as it came
            assert [r[0] for r in tr] == [PIECE] and pieces[0][1:6] == (0, cfg[2], cfg[3], T, cfg[4]), case
            continue
        # what advances with time in every family: z [T][N][m] forward, Xs [T][N][n] backward
        zk, zw = {KF: (6, m), RTS: (0, n), IMM: (0, m), UKF_RTS: (0, n), UKF: (0, m)}[family]
        groups = sorted({r[1] for r in pieces})
        assert groups == list(range(len(groups))) and len(groups) <= 4
        # helper g waits on the fork before its first piece and is joined after the last piece of the call
        kinds = [r[:2] for r in tr if r[0] != PIECE]
        assert kinds == [(FORK,)] + [(WAIT, g) for g in groups[1:]] + [(JOIN, g) for g in groups[1:]], case
        assert all(r[0] == JOIN for r in tr[len(tr) - (len(groups) - 1):]), case
        at = i0
        for g in groups:
            mine = [r for r in tr if r[0] in (WAIT, PIECE) and r[1] == g]
            assert (mine[0][0] == WAIT) == (g > 0) and all(r[0] == PIECE for r in mine[1:]), case
            mine = [r for r in mine if r[0] == PIECE]
            assert {(r[2], r[3]) for r in mine} == {(at, mine[0][3])} and mine[0][3] > 0, case
            assert mine[0][3] % quantum == 0 or at + mine[0][3] == i0 + cnt, case
            at += mine[0][3]
            # the step windows [t0, t0 + steps) from the pointer that the kernel will read
            win = []
            for r in mine:
                off = r[7 + zk] - zk * BASE
                assert off % (N * zw) == 0
                win.append((off // (N * zw), off // (N * zw) + (r[4] - 1 if back else r[4])))
            if back:
                win.reverse()
            assert win[0][0] == 0 and win[-1][1] == L and all(a[0] < a[1] for a in win), case
            assert all(a[1] == b[0] for a, b in zip(win, win[1:])), case
            # the first piece of a stream keeps the call's flags, the later ones OR their status and continue
            cont0 = cfg[8] if family == UKF_RTS else 0
            assert [r[5] for r in mine] == [cfg[4]] + [1] * (len(mine) - 1), case
            assert [r[6] for r in mine] == ([cont0] + [1] * (len(mine) - 1) if back else [0] * len(mine)), case
        assert at == i0 + cnt, case


def test_default_policy(hc, monkeypatch):
    """The cases that the comments of fk_chunk_plan.hpp and of its callers name."""
    def cut(case):
        rc, flat = run(hc, monkeypatch, case)
        assert rc == 0
        tr = rows(case["family"], flat)
        if tr[0][0] != FORK:
            assert len(tr) == 1
            return None
        return len({r[1] for r in tr if r[0] == PIECE}), max(sum(1 for r in tr if r[0] == PIECE and r[1] == g) for g in range(4))

    def kf(tracks, steps=100, slots=2048, **kw):
        return make_case(KF, tracks, steps, slots=slots, extra=kf_extra(tracks + 11, 9, **kw))
    # BASELINE config 3: 1e5 tracks = 6250 waves on 2048 slots, 3.05 rounds -> 3 groups x 4 chunks (5 staggered windows)
    assert cut(kf(100000)) == (3, 5)
    assert cut(make_case(RTS, 100000, 100, slots=2048)) == (3, 5)
    assert cut(make_case(RTS, 100000, 100, slots=2048, whole_bank=True)) == (3, 5)
    assert cut(kf(98304)) is None                             # three full rounds
    assert cut(kf(100000 + 16 * 1024)) is None                # last round more than 40 % full
    assert cut(kf(100000, steps=15)) is None and cut(kf(60000)) is None          # a short run; two rounds
    assert cut(make_case(RTS, 100000, 15, slots=2048)) is None                   # (the smoother counts T - 1 steps)
    # kf_fast (8,4): 2e5 tracks = 3125 waves of 64 on 1024 slots
    assert cut(kf(200000, slots=1024, tracks_per_wave=64, quantum=256)) == (3, 5)
    # IMM: 3125 waves on 1024 slots (2e5 banks) are cut, 3072 (196 608: three full rounds) are not; nor more than four rounds
    imm = dict(slots=1024, extra=[2, 0])
    assert cut(make_case(IMM, 200000, 100, null=bits(1, 3), **imm)) == (3, 5)
    assert cut(make_case(IMM, 196608, 100, null=bits(1, 3), **imm)) is None
    assert cut(make_case(IMM, 64 * 4097, 100, null=bits(1, 3), **imm)) is None
    # ... and a masked call without ll0 never, forced or not
    assert cut(make_case(IMM, 200000, 100, null=0, **imm)) == (3, 5)
    assert cut(make_case(IMM, 200000, 100, null=bits(3), **imm)) is None
    assert cut(make_case(IMM, 200000, 100, null=bits(3), switch="2,3", **imm)) is None
    assert cut(make_case(IMM, 200000, 100, null=0, switch="2,3", **imm)) == (2, 4)
    # UKF smoother, BASELINE configs[3]: 1e5 tracks = 1563 waves on 1024 slots are cut, 1e6 = 15 625 (15.3 rounds) are not
    assert cut(make_case(UKF_RTS, 100000, 100, extra=[0])) == (3, 5)
    assert cut(make_case(UKF_RTS, 1000000, 100, extra=[0])) is None
    assert cut(make_case(UKF_RTS, 100000, 15, extra=[0])) is None
    # fused UKF: only on request
    assert cut(make_case(UKF, 100000, 100)) is None and cut(make_case(UKF, 100000, 100, switch="3,4")) == (3, 5)
    # "1,1" and what does not parse: one launch
    for switch in ("1,1", "3", "x", ""):
        assert cut(dict(kf(100000), switch=switch)) is None and cut(make_case(UKF_RTS, 100000, 100, extra=[0], switch=switch)) is None


def test_a_failed_launch_is_joined(hc, monkeypatch):
    """The launcher fails on piece k, for every k of a 3 x 4 plan (no test can make a launch fail on a GPU): no later piece
    is launched, every stream that waited on the fork is joined, and the launcher's error is what the call returns."""
    for family in range(5):
        extra = {KF: kf_extra(1511, 9), IMM: [2, 0], UKF_RTS: [0]}.get(family, [])
        case = make_case(family, 1500, 19, null=bits(3) if family == UKF else 0, extra=extra, switch="3,4", no_stagger=True)
        rc, flat = run(hc, monkeypatch, case)
        whole = rows(family, flat)
        assert rc == 0 and sum(r[0] == PIECE for r in whole) == 12
        for k in range(12):
            rc, flat = run(hc, monkeypatch, case, fail_at=k)
            tr = rows(family, flat)
            launched = [r for r in tr if r[0] != JOIN]
            assert rc == 7 and launched == [r for r in whole if r[0] != JOIN][:len(launched)], (family, k)
            assert sum(r[0] == PIECE for r in tr) == k + 1 and tr[len(launched) - 1][0] == PIECE, (family, k)
            waited = [r[1] for r in tr if r[0] == WAIT]
            assert waited == list(range(1, k // 4 + 1)), (family, k)
            assert [r for r in tr[len(launched):]] == [(JOIN, g) for g in waited], (family, k)
