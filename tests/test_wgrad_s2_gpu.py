"""GPU: the two routes of the single-bf16 3x3x3 stride-2 weight gradient (csrc/wgrad_bf16.hip) give the same slabs bit for bit.
cwf_debug_wgrad_s2(1) sends a launch behind TILED_7_1 / TILED_7_2 to wgrad_s2_kernel (all of a tile's loads in flight, the next
tile's loads issued behind this tile's MFMAs), cwf_debug_wgrad_s2(0) to the tiled kernel wgrad_bf16_kernel.  Per case, cwf_wgrad runs once per route into a NaN-filled
slab buffer: the first nsplit_used slabs must be equal as bit patterns, every float behind them still NaN, and the launch counter
moves on route 1 only.  The plan query (the same for both routes) is asked first and the case's range lengths are asserted, so
that a case cannot silently stop exercising its edge: ranges of 1, 2, 3, 4 and 5 tiles are the first, the last and the inner
trips of the tile loop, whose loads run ahead of the previous tile's MFMAs.  Operands live in buffers that are NaN outside the views.
Not here: a tile range with skipped tiles -- the stride-2 geometry has one class, whose tile grid is cut to its own extents, so the
kernels' skip test never fires; and the float64 bound of the new route, which tests/test_wgrad_bf16_exact_gpu.py holds through the
default route.  The dy4 form (dy rows that start 4 bytes off a 16-byte boundary) needs scalar dy loads: it stays on the tiled
kernel under both routes, so there the counter must not move at all."""
import collections
import ctypes

import pytest
import torch

import wgrad_bf16_cases as T
from cwf import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 64

# name: (cin, cout, size, n, form, prologue, instance, tiles of the longest range, last range shorter, a range crosses samples)
Edge = collections.namedtuple("Edge", "cin cout size n form prologue inst hi short cross")
CASES = {
    "c16_32_contig": Edge(16, 32, (11, 13, 35), 2, "contig", False, "TILED_7_2", 1, False, False),
    "c16_32_contig_norm": Edge(16, 32, (11, 13, 35), 2, "contig", True, "TILED_7_2", 1, False, False),
    "c16_32_slice": Edge(16, 32, (11, 13, 35), 2, "slice", False, "TILED_7_2", 1, False, False),
    "c16_32_slice_norm": Edge(16, 32, (11, 13, 35), 2, "slice", True, "TILED_7_2", 1, False, False),
    "c16_16": Edge(16, 16, (9, 7, 33), 2, "contig", True, "TILED_7_1", 1, False, False),
    "c20_40_ragged_ch": Edge(20, 40, (5, 6, 35), 2, "slice", True, "TILED_7_2", 1, False, False),     # chunk 1: 4 live channels, group 1: 8
    "c20_12_ragged_ch": Edge(20, 12, (5, 6, 35), 2, "contig", True, "TILED_7_1", 1, False, False),
    "ranges1": Edge(64, 128, (1, 3, 511), 2, "contig", True, "TILED_7_2", 1, False, False),            # 32 tiles on 32 ranges
    "ranges2_cross": Edge(64, 128, (1, 3, 541), 2, "contig", True, "TILED_7_2", 2, False, True),       # 17 tiles a sample: range 8 = [16, 18)
    "ranges3_short": Edge(64, 128, (1, 3, 1117), 2, "contig", True, "TILED_7_2", 3, True, True),       # 70 tiles: 23 ranges of 3 and one of 1
    "ranges4_cross": Edge(64, 128, (1, 3, 1599), 2, "contig", True, "TILED_7_2", 4, False, True),      # 50 tiles a sample: range 12 = [48, 52)
    "ranges5": Edge(64, 128, (1, 3, 2079), 2, "contig", False, "TILED_7_2", 5, False, False),          # 130 tiles
    "ranges5_short": Edge(64, 128, (5, 7, 1051), 1, "contig", True, "TILED_7_2", 5, True, False),      # 2 x 2 x 33 tiles: 26 ranges of 5, one of 2
    "dy4": Edge(16, 32, (5, 7, 35), 2, "dy4", True, "TILED_7_2", 1, False, False),
}


def _u(*shape, seed, lo=-1.0, hi=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(*shape, generator=g) * (hi - lo) + lo


def _counter(hip):
    return int(hip.lib.cwf_debug_wgrad_s2_launches())


def _run(hip, route, a, nsplit, slab):
    """one cwf_wgrad under cwf_debug_wgrad_s2(route) into NaN-filled slabs: (slab buffer, slabs used, launches counted)"""
    part = torch.full((nsplit * slab + GUARD,), float("nan"), device=DEV)
    a.partial = part.data_ptr()
    used = ctypes.c_int(0)
    old = hip.lib.cwf_debug_wgrad_s2(route)
    try:
        n0 = _counter(hip)
        assert hip.lib.cwf_wgrad(ctypes.addressof(a), ctypes.addressof(used), hip._stream()) == 0
        torch.cuda.synchronize()
        took = _counter(hip) - n0
    finally:
        hip.lib.cwf_debug_wgrad_s2(old)
    return part, used.value, took


def test_the_switch_returns_the_previous_value(hip):
    assert hip.lib.cwf_debug_wgrad_s2(1) == 1              # the default
    assert hip.lib.cwf_debug_wgrad_s2(0) == 1 and hip.lib.cwf_debug_wgrad_s2(1) == 0


@pytest.mark.parametrize("name", list(CASES))
def test_routes_give_the_same_slabs(hip, name):
    e = CASES[name]
    case = T.Case(name, T.S2, e.cin, e.cout, e.size, e.n, e.form, {"bf16": e.inst})
    m = T.memory(case)
    do, ho, wo = T.out_dims(T.S2, *e.size)
    ca = (e.cout + 3) // 4 * 4
    x = _u(e.n, *e.size, e.cin, seed=11)
    dy = _u(e.n, do, ho, wo, e.cout, seed=12)
    xbuf = torch.full((e.n, *e.size, m.x_width), float("nan"), device=DEV)
    dbuf = torch.full((e.n, do, ho, wo, m.dy_width), float("nan"), device=DEV)
    xbuf[..., m.x_off:m.x_off + e.cin] = x.to(DEV)
    dbuf[..., m.dy_off:m.dy_off + ca] = 0.0
    dbuf[..., m.dy_off:m.dy_off + e.cout] = dy.to(DEV)
    sc = sh = None
    slope = 1.0
    if e.prologue:
        sc, sh, slope = _u(e.n, e.cin, seed=13, lo=0.5, hi=1.5), _u(e.n, e.cin, seed=14), 0.01
        h = x * sc.view(e.n, 1, 1, 1, e.cin) + sh.view(e.n, 1, 1, 1, e.cin)
        assert bool((h < 0).any()) and bool((h > 0).any())          # both branches of the activation
        sc, sh = sc.to(DEV), sh.to(DEV)
    p = lambda t: 0 if t is None else t.data_ptr()
    a = T.descriptor(_lib, case, "bf16", xbuf.data_ptr(), dbuf.data_ptr(), 0, scale=p(sc), shift=p(sh), slope=slope)
    assert (a.dy % 16 == 0) == (e.form != "dy4") and a.x % 16 == 0
    nsplit, slab = hip.lib.cwf_wgrad_nsplit(T.S2, e.n, do, ho, wo, e.cin, e.cout), hip.lib.cwf_wgrad_slab_floats(T.S2, e.cin, e.cout)

    # the plan (route-independent) has the edge the case is here for
    a.partial = 0x70000000
    for route in (0, 1):
        old = hip.lib.cwf_debug_wgrad_s2(route)
        rc, plan = T.query(hip.lib, a)
        hip.lib.cwf_debug_wgrad_s2(old)
        assert rc == 0 and T.NAME_OF[plan.inst] == e.inst and plan.walk == T.WALK_RANGES and plan.slab == slab, (route, rc, plan)
        ranges = T.workgroup_items(plan)
        lens = [len(r) for r in ranges]
        assert max(lens) == plan.hi and (plan.hi == e.hi if e.hi < 5 else plan.hi >= 5), lens
        assert (lens[-1] < lens[0]) == e.short and all(n == lens[0] for n in lens[:-1]), lens
        per_sample = plan.items // e.n
        assert any(r[0] // per_sample != r[-1] // per_sample for r in ranges) == e.cross, (per_sample, lens)
        assert 1 <= plan.used <= nsplit

    got = {}
    for route in (0, 1):
        part, used, took = _run(hip, route, a, nsplit, slab)
        assert used == plan.used
        assert took == (1 if route == 1 and e.form != "dy4" else 0), (route, took)
        assert bool(torch.isfinite(part[:used * slab]).all()), (route, "a slab slot the reduce reads was not written")
        assert bool(part[used * slab:].isnan().all()), (route, "written beyond the slabs reported as used")
        got[route] = part[:used * slab].view(torch.int32)
    diff = got[0] != got[1]
    assert not bool(diff.any()), "%d of %d slab floats differ between the routes, first at %d" % (
        int(diff.sum()), diff.numel(), int(diff.nonzero()[0]))
    assert bool((got[1] != 0).any())
