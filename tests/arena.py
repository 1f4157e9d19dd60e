"""A guarded arena for the memory side of the C ABI (tests/test_gpu_arena.py; tests/test_host_arena.py tests this file on the CPU).

The suite hands every kernel buffers of its own from the caching allocator: their bases are 512-byte aligned and nothing looks at
the bytes around them.  Here every argument of a call is a view into ONE uint8 tensor:

    [guard] view [guard] [guard] view [guard] ...

  - the tensor is filled with an 8-byte pattern that is a quiet NaN with a payload as a double (an out-of-range read that reaches
    arithmetic poisons an output) and a recognisable non-zero value as int32;
  - every view starts at a chosen PHASE relative to 512 bytes, so the caller decides the pointer alignment a launcher sees;
  - every view has a guard of its own on both sides, at least 4 KiB and at least 256 records of that array (one workgroup's
    worth: a whole misplaced wave slab lands in a guard, not in the next view);
  - snapshot() before the call, check() after it: every byte of the arena outside the `out` / `inout` views must still hold
    what it held -- guards and inputs in one comparison.

Nothing below the element size is ever misaligned (doubles stay on 8 bytes, int32 on 4): every phase is a call that
include/filterhip.h permits."""
import contextlib
import threading

import numpy as np
import torch

PATTERN = 0x7FF8A5A55AFEC0DE               # little endian: double = quiet NaN, payload 0xA5A55AFEC0DE; int32 = 0x5AFEC0DE, 0x7FF8A5A5
PATTERN_I32 = 0x5AFEC0DE
PATTERN_U8 = 0xDE
ALIGN = 512
MIN_GUARD = 4096
GUARD_RECORDS = 256
ROLES = ("in", "out", "inout")

# all relative to 512.  0: the control (what the caching allocator hands out); 8; 16 and 56: 16-byte aligned but not 64- / 128-byte
# aligned; "mixed": successive arguments of one call take 8, 0, 24, 16, 40, ... in turn, so a launcher that ORs two pointers sees
# one aligned and one not.
PHASES = (0, 8, 16, 56, "mixed")


def mixed_phase(k):
    """the k-th argument's phase under "mixed": 8, 0, 24, 16, 40, 32, ..."""
    return (16 * (k // 2) + (8 if k % 2 == 0 else 0)) % ALIGN


def phase_of(phase, k, dtype, align=1):
    """The phase of the k-th argument of a call made at `phase`.  Doubles (and int64) take the phase as it is.  int32 arrays
    (status, indices) add 4 off the control, which lands them on 12, 4 and 12 mod 16 at phases 8, 16 and 56; byte masks add 1, 2
    and 3 (1, 2, 3 mod 4).  `align` (a power of two) keeps an argument on a boundary the header states (the resampler workspace:
    16 bytes): the phase is rounded down to it."""
    p = mixed_phase(k) if phase == "mixed" else int(phase)
    size = torch.empty(0, dtype=dtype).element_size()
    if phase != 0:
        if size == 4:
            p += 4 if phase != "mixed" else (4, 12)[k % 2]
        elif size == 1:
            p += {8: 1, 16: 2, 56: 3}.get(phase, 1 + k % 3)
    p -= p % max(align, size)
    return p % ALIGN


def guard_bytes(rec_bytes):
    return max(MIN_GUARD, GUARD_RECORDS * int(rec_bytes))


def span_bytes(nbytes, rec_bytes):
    """what one view takes of an arena at most: both guards, the view, the rounding up to 512 and the phase (below 512 + 16)"""
    return 2 * guard_bytes(rec_bytes) + int(nbytes) + 3 * ALIGN


def fill_pattern(t):
    """the arena's fill, restated relative to the view (an output a call leaves alone then holds the same bytes at every phase)"""
    size = t.element_size()
    if size == 8:
        t.view(torch.int64).fill_(PATTERN)
    elif size == 4:
        t.view(torch.int32).fill_(PATTERN_I32)
    else:
        t.view(torch.uint8).fill_(PATTERN_U8)
    return t


def host_records(a, layout, lead):
    """the transposition of filterpy_amd._engine.to_records on the host: lead + (N,) + rec -> lead + (N, rec...) for 'aos' (as it
    is), lead + (rec, N) for 'soa'; layout None: the array as it is"""
    h = np.ascontiguousarray(a)
    if layout is None or layout == "aos":
        return h
    assert layout == "soa", layout
    shp = h.shape
    N = shp[lead]
    rec = int(np.prod(shp[lead + 1:])) if len(shp) > lead + 1 else 1
    return np.ascontiguousarray(np.swapaxes(h.reshape(*shp[:lead], N, rec), -1, -2))


class View:
    def __init__(self, name, start, nbytes, role, guard, tensor):
        self.name, self.start, self.end, self.role, self.guard, self.tensor = name, start, start + nbytes, role, guard, tensor


class Arena:
    def __init__(self, device, nbytes):
        nbytes = (int(nbytes) + 7) // 8 * 8
        raw = torch.empty(nbytes + ALIGN, dtype=torch.uint8, device=device)
        off = (-raw.data_ptr()) % ALIGN
        self.buf = raw[off:off + nbytes]
        assert self.buf.data_ptr() % ALIGN == 0 and self.buf.numel() == nbytes
        self.buf.view(torch.int64).fill_(PATTERN)
        self.views = []
        self.cursor = 0                    # end of the last view's trailing guard
        self.snap = None

    # ---------------------------------------------------------------------------------------------------------- carving
    def carve(self, shape, dtype, phase, role, rec=1, name=None):
        """A contiguous view of `shape` / `dtype` with data_ptr() % 512 == phase.  rec: elements per record of the array (its guard
        is at least 256 of them).  The bytes are the arena's fill."""
        assert role in ROLES, role
        assert self.snap is None, "carve before snapshot()"
        size = torch.empty(0, dtype=dtype).element_size()
        assert 0 <= phase < ALIGN and phase % size == 0, (phase, dtype)     # never below the element size
        shape = tuple(int(s) for s in shape)
        nbytes = int(np.prod(shape)) * size if shape else size
        guard = guard_bytes(rec * size)
        start = (self.cursor + guard + ALIGN - 1) // ALIGN * ALIGN + phase
        assert start + nbytes + guard <= self.buf.numel(), "arena too small: %d + %d + %d > %d" % (start, nbytes, guard, self.buf.numel())
        t = self.buf[start:start + nbytes].view(dtype).reshape(shape)
        assert t.is_contiguous() and t.data_ptr() % ALIGN == phase and t.data_ptr() == self.buf.data_ptr() + start
        self.views.append(View(name or "arg%d" % len(self.views), start, nbytes, role, guard, t))
        self.cursor = start + nbytes + guard
        return t

    def put(self, host_array, phase, role, layout=None, lead=0, name=None):
        """carve, then upload `host_array` (lead + (N,) + rec) through the record transposition of _engine.to_records"""
        h = host_records(host_array, layout, lead)
        rec = 1 if layout is None else int(np.prod(np.shape(host_array)[lead + 1:]))
        t = self.carve(h.shape, torch.from_numpy(h).dtype, phase, role, rec=rec, name=name)
        t.copy_(torch.from_numpy(h))
        return t

    # -------------------------------------------------------------------------------------------------- snapshot and check
    def snapshot(self):
        self._sync()
        self.snap = self.buf.clone()
        self.protected = torch.ones(self.buf.numel(), dtype=torch.bool, device=self.buf.device)
        for v in self.views:
            if v.role != "in":
                self.protected[v.start:v.end] = False

    def check_guards(self, what=""):
        """For an arena whose views were carved while the calls ran (allocations_in), so that no snapshot could precede them:
        every byte outside ALL views still holds the fill."""
        self._sync()
        pat = torch.tensor(list(PATTERN.to_bytes(8, "little")), dtype=torch.uint8, device=self.buf.device)
        self.snap = pat.repeat(self.buf.numel() // 8)
        self.protected = torch.ones(self.buf.numel(), dtype=torch.bool, device=self.buf.device)
        for v in self.views:
            self.protected[v.start:v.end] = False
        self.check(what)

    def _sync(self):
        if self.buf.is_cuda:
            torch.cuda.synchronize()

    def first_difference(self):
        """None, or the first byte outside the out / inout views that differs from the snapshot, as
        (view name, role, anchor, offset, was, is): anchor 'start' with offset < 0 (so many bytes in front of the view), 'end' with
        offset >= 0 (so many bytes past its last byte + 1) or 'inside' an `in` view (offset from its start); the nearest view."""
        assert self.snap is not None, "snapshot() first"
        self._sync()
        bad = ((self.buf != self.snap) & self.protected).nonzero()
        if bad.numel() == 0:
            return None
        b = int(bad[0])
        best = None
        for v in self.views:
            if v.start <= b < v.end:
                cand = (0, v, "inside", b - v.start)
            elif b < v.start:
                cand = (v.start - b, v, "start", b - v.start)
            else:
                cand = (b - v.end + 1, v, "end", b - v.end)
            if best is None or cand[0] < best[0]:
                best = cand
        if best is None:
            return (None, None, "arena", b, int(self.snap[b]), int(self.buf[b]))
        return (best[1].name, best[1].role, best[2], best[3], int(self.snap[b]), int(self.buf[b]))

    def check(self, what=""):
        d = self.first_difference()
        if d is not None:
            n = int(((self.buf != self.snap) & self.protected).sum())
            raise AssertionError("%s: %d byte(s) changed outside the outputs; the first: view %r (%s), %s %+d: 0x%02x -> 0x%02x"
                                 % ((what, n) + d))


# ------------------------------------------------------------------------------------------------------------ allocators
class ArenaAlloc:
    """The arguments of ONE call, carved in turn from an arena at `phase` (phase_of: the k-th argument's own phase)."""

    def __init__(self, arena, phase):
        self.arena, self.phase, self.k = arena, phase, 0

    def _phase(self, dtype, align):
        p = phase_of(self.phase, self.k, dtype, align)
        self.k += 1
        return p

    def put(self, host_array, role="in", layout=None, lead=0, name=None, align=1):
        h = np.ascontiguousarray(host_array)
        return self.arena.put(h, self._phase(torch.from_numpy(h).dtype, align), role, layout, lead, name)

    def new(self, shape, dtype=torch.float64, role="out", rec=1, fill=None, name=None, align=1):
        """an output: the NaN fill, or `fill` (a status array starts as zeros)"""
        t = self.arena.carve(shape, dtype, self._phase(dtype, align), role, rec=rec, name=name)
        return fill_pattern(t) if fill is None else t.fill_(fill)

    def records(self, lead_shape, N, E, layout, role="out", name=None):
        shape = (*lead_shape, N, E) if layout == "aos" else (*lead_shape, E, N)
        return self.new(shape, torch.float64, role, rec=E, name=name)

    def views(self):
        return [(v.name, v.role, v.tensor) for v in self.arena.views]


class PlainAlloc:
    """The same interface on ordinary allocations (the run every phase is compared with); `need` adds up the arena that holds
    the same arguments."""

    def __init__(self, device):
        self.device, self.need, self._views = device, 2 * ALIGN, []

    def _keep(self, t, role, rec, name):
        self.need += span_bytes(t.numel() * t.element_size(), rec * t.element_size())
        self._views.append((name or "arg%d" % len(self._views), role, t))
        return t

    def put(self, host_array, role="in", layout=None, lead=0, name=None, align=1):
        h = host_records(host_array, layout, lead)
        rec = 1 if layout is None else int(np.prod(np.shape(host_array)[lead + 1:]))
        t = torch.empty(h.shape, dtype=torch.from_numpy(h).dtype, device=self.device)
        t.copy_(torch.from_numpy(h))
        return self._keep(t, role, rec, name)

    def new(self, shape, dtype=torch.float64, role="out", rec=1, fill=None, name=None, align=1):
        t = torch.empty(tuple(int(s) for s in shape), dtype=dtype, device=self.device)
        t = fill_pattern(t) if fill is None else t.fill_(fill)
        return self._keep(t, role, rec, name)

    def records(self, lead_shape, N, E, layout, role="out", name=None):
        shape = (*lead_shape, N, E) if layout == "aos" else (*lead_shape, E, N)
        return self.new(shape, torch.float64, role, rec=E, name=name)

    def views(self):
        return list(self._views)


def outputs(alloc):
    """[(name, bytes as a NumPy uint8 array)] of the out / inout arguments, in carving order"""
    return [(name, t.detach().cpu().contiguous().view(torch.uint8).numpy().copy().reshape(-1))
            for name, role, t in alloc.views() if role != "in"]


# ------------------------------------------------------------------------------------ an existing runner, inside an arena
def adopted_record(shape):
    """elements per record assumed for an adopted array, whose layout is not known here: the larger of its last two extents (a
    record array is [..][N][E] or [..][E][N]), at most 16 x 16, the largest record of the ABI; 1 for a vector"""
    return min(256, max(shape[-2:])) if len(shape) >= 2 else 1


@contextlib.contextmanager
def allocations_in(arena, phase, E):
    """While this is open, every device array the test helpers and the package's classes make -- _engine.dev / to_records /
    alloc_records / alloc_cov_pair, torch.zeros / full / empty / as_tensor / tensor / zeros_like / empty_like with a CUDA device and
    what Tensor.clone / contiguous / to / cuda return on one -- is a view of `arena`, the k-th of them at phase_of(phase, k, dtype): an EXISTING runner (a precision test's own function)
    then runs wholly inside the arena, unchanged.  What is an input and what an output is not known here, so every view is
    `inout`: check() then holds the guards.  Yields a list that collects (name of the argument's dtype and shape) of every
    pointer _engine hands to the library that is NOT inside the arena -- the caller asserts that it stays empty."""
    base, size = arena.buf.data_ptr(), arena.buf.numel()
    k = [0]
    outside = []
    lock = threading.Lock()

    def inside(t):
        return base <= t.data_ptr() and t.data_ptr() + t.numel() * t.element_size() <= base + size

    def adopt(t):
        if not isinstance(t, torch.Tensor) or not t.is_cuda or t.numel() == 0 or not t.is_contiguous() or inside(t):
            return t
        with lock:                         # (the package's transfer pipeline allocates from worker threads)
            v = arena.carve(t.shape, t.dtype, phase_of(phase, k[0], t.dtype), "inout", rec=adopted_record(tuple(t.shape)))
            k[0] += 1
        v.copy_(t)
        return v

    def cuda(device):
        return device is not None and torch.device(device).type == "cuda"

    saved = []

    def patch(obj, name, fn):
        saved.append((obj, name, getattr(obj, name)))
        setattr(obj, name, fn)

    def adopting(orig, by_device=True):
        def f(*a, **kw):
            t = orig(*a, **kw)
            return adopt(t) if (not by_device or cuda(kw.get("device"))) else t
        return f

    def like(orig):
        def f(t, *a, **kw):
            return adopt(orig(t, *a, **kw))
        return f

    orig_pair, orig_ptr, orig_mask = E.alloc_cov_pair, E._ptr, E._mask_ptr

    def cov_pair(T, N, n, layout, device=None):
        cov2, _, _ = orig_pair(T, N, n, layout, device)
        cov2 = adopt(cov2)
        return (cov2, cov2[:, :, 0], cov2[:, :, 1]) if layout == "aos" else (cov2, cov2[:, 0], cov2[:, 1])

    def seen(t):
        if t is not None and t.numel() and not inside(t):
            outside.append((str(t.dtype), tuple(t.shape)))

    def ptr(t):
        seen(t)
        return orig_ptr(t)

    def mask_ptr(t, keep):
        if t is not None and not t.is_contiguous():
            t = adopt(t.contiguous())
        seen(t)
        return orig_mask(t, keep)

    try:
        for name in ("dev", "to_records", "alloc_records"):
            patch(E, name, adopting(getattr(E, name), by_device=False))
        patch(E, "alloc_cov_pair", cov_pair)
        patch(E, "_ptr", ptr)
        patch(E, "_mask_ptr", mask_ptr)
        for name in ("zeros", "full", "empty", "as_tensor", "tensor", "ones"):
            patch(torch, name, adopting(getattr(torch, name)))
        for name in ("zeros_like", "empty_like"):
            patch(torch, name, like(getattr(torch, name)))
        for name in ("clone", "contiguous", "to", "cuda"):             # (the classes copy their state with .clone())
            patch(torch.Tensor, name, like(getattr(torch.Tensor, name)))
        yield outside
    finally:
        for obj, name, fn in reversed(saved):
            setattr(obj, name, fn)
