"""-m gpu: fk_poly_run with every argument carved from ONE guarded, NaN-filled arena (tests/arena.py), at every pointer phase:
the outputs are bit-identical to the run on ordinary allocations, and every byte of the arena outside the outputs -- guards and
inputs -- holds what it held.  The phases take the pointers off 16-byte alignment (8, 56, mixed): the kernels' 8-byte accesses
must not care.  N in {1, 63, 65, 1031}, both layouts, each (order, form); T = 6 (a whole round of the look-ahead and a tail), the
gains from the table, all three histories written."""
import numpy as np
import pytest

import arena as AR
import poly_port as pp

pytestmark = pytest.mark.gpu
SIZES = (1, 63, 65, 1031)
T, DT = 6, 0.3


def call(A, order, form, N, layout):
    """carve every argument from the allocator A, run, return the outputs' bytes"""
    import torch
    from filterpy_amd import _engine as E
    C = order + 1
    rs = np.random.RandomState(10 * order + form + N)
    gains = A.put(np.array([pp.lsq_gains(order, n + 1, DT) for n in range(T)]).reshape(T, C), name="gains")
    z = A.put(np.cumsum(rs.randn(T, N), axis=0), name="z")
    x = A.put(rs.randn(N, C), role="inout", layout=layout, name="x")
    xs = A.records((T,), N, C, layout, name="xs")
    pred = A.new((T, N), name="pred")
    y = A.new((T, N), name="y_out")
    if isinstance(A, AR.ArenaAlloc):
        A.arena.snapshot()
    E.poly_run(order, form, N, T, layout, DT, DT**2., 0.5 * DT**2, 0.8, 0.2, 0.05, z, x, gains=gains, xs=xs, pred=pred, y=y)
    torch.cuda.synchronize()
    return AR.outputs(A)


@pytest.mark.parametrize("layout", ("soa", "aos"))
@pytest.mark.parametrize("order,form", pp.COMBOS)
def test_poly_run_in_the_arena(order, form, layout):
    from filterpy_amd import _engine as E
    dev = E.require_gpu()
    found = []
    for N in SIZES:
        plain = AR.PlainAlloc(dev)
        base = call(plain, order, form, N, layout)
        assert [n for n, _ in base] == ["x", "xs", "pred", "y_out"] and not any(np.isnan(b.view(np.float64)).any() for _, b in base)
        for phase in AR.PHASES:
            ar = AR.Arena(dev, plain.need)
            what = "fk_poly_run order %d form %d %s N=%d phase %s" % (order, form, layout, N, phase)
            got = call(AR.ArenaAlloc(ar, phase), order, form, N, layout)
            try:
                ar.check(what)
            except AssertionError as e:
                found.append(str(e))
            for (name, g), (_, b) in zip(got, base):
                if not np.array_equal(g, b):
                    found.append("%s: output %r differs from the ordinary-allocation run in %d byte(s)" % (what, name, int((g != b).sum())))
    assert not found, "%d finding(s):\n%s" % (len(found), "\n".join(found))
