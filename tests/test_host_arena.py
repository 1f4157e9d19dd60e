"""tests/arena.py itself, on the CPU: every carve lands on its phase, the guards have their stated size, and a single byte written
where a kernel must not write -- just past an output, just in front of it, inside an input, in the gap between two views -- is
reported with the right view and offset.  Together these are the proof that tests/test_gpu_arena.py can fail."""
import numpy as np
import pytest
import torch

import arena as AR

F64, I32, U8 = torch.float64, torch.int32, torch.uint8


def _arena():
    """in (130 x 6 doubles) | out (3 x 130 x 36 doubles) | inout status (130 int32) | in mask (3 x 130 bytes)"""
    a = AR.Arena("cpu", 1 << 20)
    rs = np.random.RandomState(5)
    views = dict(x=a.put(rs.randn(130, 6), 8, "in", "aos", 0, name="x"),
                 covs=a.carve((3, 130, 36), F64, 24, "out", rec=36, name="covs"),
                 status=a.carve((130,), I32, 12, "inout", name="status"),
                 mask=a.put(np.ones((3, 130), np.uint8), 3, "in", name="mask"))
    return a, views


def test_pattern_is_a_quiet_nan_and_a_nonzero_int32():
    a = AR.Arena("cpu", 4096)
    d = a.buf.view(F64).numpy()
    assert np.isnan(d).all()
    bits = a.buf.view(torch.int64).numpy()
    assert (bits == AR.PATTERN).all() and (AR.PATTERN >> 51) & 0xFFF == 0xFFF and AR.PATTERN & ((1 << 51) - 1) != 0   # quiet, payload
    w = a.buf.view(I32).numpy()
    assert (w[0::2] == AR.PATTERN_I32).all() and (w != 0).all()
    assert a.buf.data_ptr() % 512 == 0


@pytest.mark.parametrize("dtype,phases", [(F64, range(0, 512, 8)), (I32, range(0, 512, 4)), (U8, range(0, 64))],
                         ids=["f64", "i32", "u8"])
def test_every_carve_lands_on_its_phase(dtype, phases):
    phases = list(phases)
    a = AR.Arena("cpu", len(phases) * AR.span_bytes(17 * 8, 8) + 1024)
    for p in phases:
        t = a.carve((17,), dtype, p, "out")
        assert t.data_ptr() % 512 == p and t.is_contiguous() and t.dtype == dtype and t.shape == (17,)
    with pytest.raises(AssertionError):
        a.carve((4,), F64, 4, "in")                 # below the element size: not a legal call, never produced
    with pytest.raises(AssertionError):
        a.carve((4,), I32, 2, "in")


def test_guards_have_the_stated_size_and_views_do_not_touch():
    a, v = _arena()
    by = {w.name: w for w in a.views}
    assert by["x"].guard == 256 * 6 * 8 and by["covs"].guard == 256 * 36 * 8 and by["status"].guard == 4096 == by["mask"].guard
    assert a.views[0].start >= a.views[0].guard
    for p, q in zip(a.views, a.views[1:]):
        assert q.start - p.end >= p.guard + q.guard                      # a guard of its own on both sides
    assert a.buf.numel() - a.views[-1].end >= a.views[-1].guard
    # the fill is intact around every view, and the uploads are what was put
    pat = np.frombuffer(np.int64(AR.PATTERN).tobytes(), np.uint8)
    raw = a.buf.numpy()
    for w in a.views:
        for lo, hi in ((w.start - w.guard, w.start), (w.end, w.end + w.guard)):
            assert (raw[lo:hi] == pat[np.arange(lo, hi) % 8]).all(), w.name
    assert torch.equal(v["mask"], torch.ones(3, 130, dtype=U8))


def test_put_transposes_like_to_records():
    rs = np.random.RandomState(6)
    h = rs.randn(3, 22, 2, 2)
    a = AR.Arena("cpu", 1 << 18)
    soa, aos = a.put(h, 8, "in", "soa", 1), a.put(h, 16, "in", "aos", 1)
    assert soa.shape == (3, 4, 22) and aos.shape == (3, 22, 2, 2)
    assert np.array_equal(soa.numpy(), np.swapaxes(h.reshape(3, 22, 4), 1, 2)) and np.array_equal(aos.numpy(), h)
    assert a.views[0].guard == 256 * 4 * 8 == 8192
    p = AR.PlainAlloc("cpu")
    assert np.array_equal(p.put(h, "in", "soa", 1).numpy(), soa.numpy())


def test_untouched_arena_passes_and_outputs_may_change_freely():
    a, v = _arena()
    a.snapshot()
    a.check("untouched")
    v["covs"].fill_(1.5)
    v["status"].fill_(0)
    a.check("outputs written")
    assert a.first_difference() is None


def _poke(a, byte):
    a.buf[byte] = int(a.buf[byte]) ^ 0x01


@pytest.mark.parametrize("where,expect", [
    ("past_out", ("covs", "out", "end", 0)),
    ("before_out", ("covs", "out", "start", -1)),
    ("far_past_out", ("covs", "out", "end", 36 * 8 * 64)),          # a whole wave's slab further on: still this view's guard
    ("in_input", ("x", "in", "inside", 130 * 6 * 8 - 1)),
    ("in_mask", ("mask", "in", "inside", 0)),
    ("past_inout", ("status", "inout", "end", 3)),
    ("gap", None),
])
def test_one_byte_is_reported_with_view_and_offset(where, expect):
    a, _ = _arena()
    by = {w.name: w for w in a.views}
    a.snapshot()
    if where == "gap":                                                # the middle of the gap between x and covs, nearer to covs
        b = (by["x"].end + by["covs"].start) // 2 + 1
        expect = ("covs", "out", "start", b - by["covs"].start)
    else:
        w = by[expect[0]]
        b = {"end": w.end, "start": w.start, "inside": w.start}[expect[2]] + expect[3]
    was = int(a.buf[b])
    _poke(a, b)
    d = a.first_difference()
    assert d == expect + (was, was ^ 1), d
    with pytest.raises(AssertionError) as e:
        a.check(where)
    assert repr(expect[0]) in str(e.value) and "%+d" % expect[3] in str(e.value) and "1 byte(s)" in str(e.value)
    _poke(a, b)                                                       # put back: clean again
    a.check("restored")


def test_the_first_of_several_differences_is_named():
    a, _ = _arena()
    by = {w.name: w for w in a.views}
    a.snapshot()
    _poke(a, by["status"].end + 7)
    _poke(a, by["covs"].start - 16)
    assert a.first_difference()[:4] == ("covs", "out", "start", -16)


def test_phases_are_legal_and_cover_what_they_claim():
    assert AR.PHASES == (0, 8, 16, 56, "mixed")
    assert [AR.mixed_phase(k) for k in range(6)] == [8, 0, 24, 16, 40, 32]
    for ph in AR.PHASES:
        for k in range(40):
            assert AR.phase_of(ph, k, F64) % 8 == 0 and AR.phase_of(ph, k, I32) % 4 == 0
            assert AR.phase_of(ph, k, F64, align=16) % 16 == 0
    assert all(AR.phase_of(0, k, d) == 0 for k in range(5) for d in (F64, I32, U8))              # the control
    assert {AR.phase_of(p, 0, F64) % 16 for p in (8, 16, 56)} == {8, 0} and AR.phase_of(56, 0, F64) % 64 != 0
    assert {AR.phase_of(p, k, I32) % 16 for p in AR.PHASES[1:] for k in range(4)} >= {4, 12}
    assert {AR.phase_of(p, k, U8) % 4 for p in AR.PHASES[1:] for k in range(6)} == {1, 2, 3}
    # "mixed": a launcher that ORs the pointers of two successive double arguments sees one aligned to 16 and one not
    assert all((AR.phase_of("mixed", k, F64) % 16 == 0) != (AR.phase_of("mixed", k + 1, F64) % 16 == 0) for k in range(20))


def test_both_allocators_hand_out_the_same_arguments():
    rs = np.random.RandomState(7)
    x = rs.randn(22, 4)

    def call(A):
        A.put(x, "inout", "soa", 0, name="x")
        A.records((3,), 22, 16, "aos", name="covs")
        A.new((22,), I32, "inout", fill=0, name="status")
        A.put(np.ones(22, np.uint8), name="mask")
        return A

    p = call(AR.PlainAlloc("cpu"))
    for ph in AR.PHASES:
        ar = AR.Arena("cpu", p.need)
        q = call(AR.ArenaAlloc(ar, ph))
        ar.snapshot()
        ar.check(str(ph))
        assert [t.data_ptr() % 512 for _, _, t in q.views()] == [AR.phase_of(ph, k, t.dtype) for k, (_, _, t) in enumerate(q.views())]
        po, qo = AR.outputs(p), AR.outputs(q)
        assert [n for n, _ in po] == ["x", "covs", "status"] == [n for n, _ in qo]
        assert all(np.array_equal(u, w) for (_, u), (_, w) in zip(po, qo))           # unwritten outputs hold the same fill
        assert np.isnan(q.views()[1][2].numpy()).all()


def test_check_guards_needs_no_snapshot_and_sees_a_byte_in_any_gap():
    """the check of arena.allocations_in's arenas, whose views are carved while the calls run: every byte outside ALL views holds
    the fill; views of any role may change"""
    a, v = _arena()
    v["covs"].fill_(2.5)
    v["x"].fill_(0.0)                       # (roles are not known in that mode: an input may change too)
    a.check_guards("untouched")
    b = {w.name: w for w in a.views}["mask"].end + 5
    _poke(a, b)
    with pytest.raises(AssertionError) as e:
        a.check_guards("poked")
    assert "'mask'" in str(e.value) and "+5" in str(e.value)
