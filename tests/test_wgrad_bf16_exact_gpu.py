"""GPU: every kernel instance of csrc/wgrad_bf16.hip -- the weight gradients of the bf16 and bf16x3 modes -- once per case of
tests/wgrad_bf16_cases.py, step for step as test_weight_gradient_is_operand_exact of tests/test_conv_fp32_exact_gpu.py holds the fp32
family: the read-only plan query says which instance the descriptor reaches (asserted against the table) and how many slabs it
writes; cwf_wgrad runs into a NaN-filled slab buffer with a guard (every float of the slabs it reports written is finite, every
float behind them still NaN); both reduces run into NaN-filled dW / db with guards; two whole runs are compared bit for bit; the
Python routes (hip.wgrad, wgrad_to + wgrad_flush, wgrad_to_grouped, the image forms) must end bit-equal to the direct call.
Bound: |got - ref| <= R.GAMMA_WGRAD * A against R.wgrad_ref in the operand form the query reports, exact where A == 0.  Probes:
  random    zero-mean operands, InstanceNorm + LeakyReLU(0.01) prologue with per-sample scale / shift (grouped launches have none)
  positive  all-positive operands (no cancellation: a dropped or doubled tile shows at full size)
  impulse   bf16-valued x, one isolated bf16 impulse per dy channel (corners, face centres, the last ragged tile of each axis, the
            last sample): every gradient element is ONE exact product -- bit for bit, in both modes
  constant  x = 0, scale 1, shift != 0: the activated shift must reach in-bounds taps only (padding after activation)
One line per case is printed (-s): instance, tiles per range, worst err / (gamma A); profiles/wgrad_bf16_exact.txt is one run's."""
import ctypes
import functools
import math
import struct

import pytest
import torch

import bf16_operand_ref as R
import wgrad_bf16_cases as T
from cwf import _lib, packing as pk

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 64                                               # guard floats around every buffer
LAUNCHED = {}                                            # (case, mode) -> instance id of a launch that succeeded
DY_SCALE = [1.25, 0.0, -0.7, 3.0, 1.25, 0.5, 0.0, 1.25, -2.0, 1.25, 0.0, 0.25, 1.25, 1.5, 1.25, -0.3]


def _u(*shape, seed, lo_=-1.0, hi_=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(*shape, generator=g) * (hi_ - lo_) + lo_


def _bf(t):
    return t.to(torch.bfloat16).float()


def _wshape(op, cin, cout):
    return (cin, cout, 2, 2, 2) if op == pk.CONVT2 else ((cout, cin, 1, 1, 1) if op == pk.CONV1 else (cout, cin, 3, 3, 3))


def _impulses(shape):
    """zero except one bf16-representable value per channel at voxels pairwise >= 3 apart: corners, face centres, the last (ragged)
    tile of each dimension, in the last and the first sample"""
    n, d, h, w, c = shape
    cand = []
    for nn in sorted({0, n - 1}, reverse=True):
        cand += [(nn, a, b, e) for a in (0, d - 1) for b in (0, h - 1) for e in (0, w - 1)]
        cand += [(nn, d // 2, h // 2, 0), (nn, d // 2, h // 2, w - 1), (nn, 0, h // 2, w // 2), (nn, d - 1, h // 2, w // 2),
                 (nn, d // 2, 0, w // 2), (nn, d // 2, h - 1, w // 2)]
        cand += [(nn, ((d - 1) // 4) * 4, h // 2, w // 2), (nn, d // 2, ((h - 1) // 4) * 4, w // 2),
                 (nn, d // 2, h // 2, ((w - 1) // 16) * 16), (nn, d - 2, h - 2, w - 2)]
    keep = []
    for p in cand:
        if min(p[1:]) >= 0 and all(p[0] != q[0] or max(abs(p[1] - q[1]), abs(p[2] - q[2]), abs(p[3] - q[3])) >= 3 for q in keep):
            keep.append(p)
    vals = [0.75, -1.5, 1.25, -0.5, 2.0, -1.125, 0.625, 1.875]
    x = torch.zeros(shape)
    for ch in range(c):
        x[keep[ch % len(keep)] + (ch,)] = vals[ch % len(vals)] * (1 + ch // len(keep))
    return x


def _field(shape, probe, seed):
    return _u(*shape, seed=seed, lo_=0.5, hi_=1.0) if probe == "positive" else _u(*shape, seed=seed)


@functools.lru_cache(maxsize=None)
def _inputs(op, cin, cout, size, n, probe, prologue, dys, q):
    """(x, dy, scale, shift, slope, dy_scale) on the CPU; q = group index of a grouped launch (other seeds)"""
    do, ho, wo = T.out_dims(op, *size)
    imp = probe == "impulse"
    x = _bf(_u(n, *size, cin, seed=71 + 10 * q)) if imp else _field((n, *size, cin), probe, seed=71 + 10 * q)
    dy = _impulses((n, do, ho, wo, cout)) if imp else _field((n, do, ho, wo, cout), probe, seed=72 + 10 * q)
    sc, sh, slope = None, None, 1.0
    if prologue and not imp:
        sc, sh, slope = _u(n, cin, seed=73, lo_=0.5, hi_=1.5), _u(n, cin, seed=74, lo_=0.0 if probe == "positive" else -1.0), 0.01
    if probe == "constant":
        assert prologue
        x = torch.zeros_like(x)
        sc, sh = torch.ones(n, cin), torch.linspace(-1.0, 1.0, cin).repeat(n, 1)
    s = None
    if dys:
        s = torch.tensor(DY_SCALE)
        s = torch.stack([s.roll(3 * i) for i in range(n)]).contiguous()
        if probe == "positive" or imp:
            s = s.abs() + 0.25 * (s == 0)
        if imp:
            s = _bf(s)                                    # dy * s then has <= 16 significant bits: hi + lo is exact
    return x, dy, sc, sh, slope, s


@functools.lru_cache(maxsize=None)
def _reference(op, cin, cout, size, n, probe, prologue, dys, q, form):
    """R.wgrad_ref of the inputs in operand form `form`, computed once and shared (S1_2 / S1D cases share shapes; the two modes of a
    pointwise stream case share the exact-product reference)"""
    x, dy, sc, sh, slope, s = _inputs(op, cin, cout, size, n, probe, prologue, dys, q)
    return R.wgrad_ref(op, x, dy, form, sc, sh, slope, dy_scale=s)


def _probes(case):
    return ["random", "positive", "impulse"] + ([] if T.groups_of(case.form) else ["constant"])      # (grouped launches: no prologue)


PARAMS = [(name, mode, probe) for name, mode in T.RUNS for probe in _probes(T.BY_NAME[name])]


def _reduce_batched(hip, part, inv, dw, db, slab, nsplit):
    raw = struct.pack("<QQQQqii", part.data_ptr(), inv.data_ptr(), dw.data_ptr(), 0 if db is None else db.data_ptr(), slab, nsplit, 0)
    table = torch.frombuffer(bytearray(raw), dtype=torch.uint8).to(DEV)
    assert hip.lib.cwf_wgrad_reduce_batched(table.data_ptr(), 1, hip._stream()) == 0
    torch.cuda.synchronize()


class _Operands:
    """the device buffers of a case as wgrad_bf16_cases.memory lays them out: NaN outside the views (another layer's channels), zero
    in the padding channels of dy's own rows"""

    def __init__(self, hip, case, probe):
        self.case, G = case, max(1, T.groups_of(case.form))
        m = self.m = T.memory(case)
        pro = not T.groups_of(case.form)
        ins = [_inputs(case.op, case.cin, case.cout, case.size, case.n, probe, pro, case.form == "dys", q) for q in range(G)]
        self.ins = ins
        x0, dy0 = ins[0][0], ins[0][1]
        ca = (case.cout + 3) // 4 * 4
        self.xbuf = torch.full((*x0.shape[:4], m.x_width), float("nan"), device=DEV)
        self.dbuf = torch.full((*dy0.shape[:4], m.dy_width), float("nan"), device=DEV)
        self.xs, self.dys = [], []
        for q in range(G):
            xo, do_ = m.x_off + q * m.x_goff, m.dy_off + q * m.dy_goff
            self.xbuf[..., xo:xo + case.cin] = ins[q][0].to(DEV)
            self.dbuf[..., do_:do_ + ca] = 0.0
            self.dbuf[..., do_:do_ + case.cout] = ins[q][1].to(DEV)
            self.xs.append(self.xbuf[..., xo:xo + case.cin])
            self.dys.append(self.dbuf[..., do_:do_ + case.cout])
        dv = lambda t: None if t is None else t.to(DEV)
        self.sc, self.sh, self.slope, self.s = dv(ins[0][2]), dv(ins[0][3]), ins[0][4], dv(ins[0][5])
        self.xa16 = self.dy16 = None
        if case.form == "images":
            self.xa16 = hip.to_bf16(self.xs[0], self.sc, self.sh, self.slope)
            self.dy16 = hip.to_bf16(self.dys[0])
            torch.cuda.synchronize()

    def descriptor(self, hip, mode, parts):
        c, p = self.case, (lambda t: 0 if t is None else t.data_ptr())
        kw = {}
        if c.form == "images":
            kw = dict(xa16=self.xa16.data_ptr(), dy16=self.dy16.data_ptr(), zero16=hip.zero16(DEV).data_ptr())
        part = [t.data_ptr() for t in parts] if T.groups_of(c.form) else parts[0].data_ptr()
        a = T.descriptor(_lib, c, mode, self.xbuf.data_ptr(), self.dbuf.data_ptr(), part, scale=p(self.sc), shift=p(self.sh),
                         slope=self.slope, dy_scale=p(self.s), **kw)
        if not T.groups_of(c.form):
            # the table's descriptor is the one the product's own builder makes for these views
            b = hip._wgrad_args(c.op, self.xs[0], self.m.x_ldc, self.sc, self.sh, self.slope, self.dys[0], self.m.dy_ldc, c.cout, parts[0], mode)
            b.dy_scale, b.xa16, b.dy16, b.zero16 = a.dy_scale, a.xa16, a.dy16, a.zero16
            assert bytes(a) == bytes(b)
            return b
        return a


def _launch(hip, ops, mode, nsplit, slab):
    """cwf_wgrad into NaN-filled slab buffers (one per group) with a guard: (plan, used, slab buffers)"""
    G = max(1, T.groups_of(ops.case.form))
    parts = [torch.full((nsplit * slab + GUARD,), float("nan"), device=DEV) for _ in range(G)]
    a = ops.descriptor(hip, mode, parts)
    rc, plan = T.query(hip.lib, a)
    assert rc == 0, rc
    assert T.NAME_OF[plan.inst] == ops.case.inst[mode], (T.NAME_OF[plan.inst], ops.case.inst[mode])
    used = ctypes.c_int(0)
    assert hip.lib.cwf_wgrad(ctypes.addressof(a), ctypes.addressof(used), hip._stream()) == 0
    torch.cuda.synchronize()
    LAUNCHED[(ops.case.name, mode)] = plan.inst
    return plan, used.value, parts


@pytest.mark.parametrize("name,mode,probe", PARAMS, ids=["%s-%s-%s" % p for p in PARAMS])
def test_case_is_operand_exact(hip, name, mode, probe):
    from cwf import functional as CF, kernels
    c = T.BY_NAME[name]
    op, cin, cout, G = c.op, c.cin, c.cout, max(1, T.groups_of(c.form))
    grouped = bool(T.groups_of(c.form))
    do, ho, wo = T.out_dims(op, *c.size)
    nsplit, slab = hip.lib.cwf_wgrad_nsplit(op, c.n, do, ho, wo, cin, cout), hip.lib.cwf_wgrad_slab_floats(op, cin, cout)
    spec = CF.ConvSpec(op, cin, cout).to(torch.device(DEV))
    assert spec.inv_map.numel() == slab
    has_b = spec.has_bias_map
    assert has_b == (op != pk.CONVT2)                    # (ConvTranspose slabs carry no bias row: its bias gradient is a channel sum)
    wn = math.prod(_wshape(op, cin, cout))
    ops = _Operands(hip, c, probe)
    worst = 0.0
    results = []
    for rep in range(2):
        plan, used, parts = _launch(hip, ops, mode, nsplit, slab)
        assert used == plan.used and plan.slab == slab and 1 <= used <= nsplit
        form = "fp32" if plan.exact else mode
        outs = []
        for q in range(G):
            assert bool(torch.isfinite(parts[q][:used * slab]).all()), "a slab slot the reduce reads was not written"
            assert bool(parts[q][used * slab:].isnan().all()), "written beyond the slabs reported as used"
            for which in ("reduce", "batched"):
                dw_all = torch.full((wn + 2 * GUARD,), float("nan"), device=DEV)
                db_all = torch.full((cout + 2 * GUARD,), float("nan"), device=DEV)
                dw, db = dw_all[GUARD:GUARD + wn], db_all[GUARD:GUARD + cout]
                dbp = db if has_b else None
                if which == "reduce":
                    assert hip.lib.cwf_wgrad_reduce(parts[q].data_ptr(), used, slab, spec.inv_map.data_ptr(), dw.data_ptr(),
                                                    0 if dbp is None else dbp.data_ptr(), hip._stream()) == 0
                    torch.cuda.synchronize()
                else:
                    _reduce_batched(hip, parts[q], spec.inv_map, dw, dbp, slab, used)
                for g_ in (dw_all[:GUARD], dw_all[GUARD + wn:], db_all[:GUARD], db_all[GUARD + cout:]) + (() if has_b else (db,)):
                    assert bool(g_.isnan().all()), (which, "wrote outside dW / db")
                assert bool(torch.isfinite(dw).all()) and (not has_b or bool(torch.isfinite(db).all())), (which, "dW / db not fully written")
                outs.append((dw.clone(), db.clone()))
            assert torch.equal(outs[-2][0], outs[-1][0]) and (not has_b or torch.equal(outs[-2][1], outs[-1][1])), "the two reduces differ"
            if rep == 0:
                dw_ref, db_ref, aw, ab = _reference(op, cin, cout, c.size, c.n, probe, not grouped, c.form == "dys", q, form)
                gw, gb = outs[-1][0].reshape(dw_ref.shape).cpu().double(), outs[-1][1].cpu().double()
                if probe == "impulse":
                    assert torch.equal(gw, dw_ref), (name, q, float((gw - dw_ref).abs().max()))
                    assert not has_b or torch.equal(gb, db_ref), (name, q, float((gb - db_ref).abs().max()))
                else:
                    worst = max(worst, R.assert_operand_exact(gw, dw_ref, aw, R.GAMMA_WGRAD, "%s %s %s dW[%d]" % (name, mode, probe, q)))
                    if has_b:
                        worst = max(worst, R.assert_operand_exact(gb, db_ref, ab, R.GAMMA_WGRAD, "%s %s %s db[%d]" % (name, mode, probe, q)))
        results.append(outs)
    for a_, b_ in zip(results[0], results[1]):            # a second whole run: bit for bit
        assert torch.equal(a_[0], b_[0]) and (not has_b or torch.equal(a_[1], b_[1])), "two runs differ"
    print("\nwgrad_bf16 %-20s %-6s %-8s %-22s tiles/range %d..%d of %-4d slabs %3d/%-3d  worst err/(gamma A) %s" % (
        name, mode, probe, T.instance_name(hip.lib, plan.inst), plan.lo, plan.hi, plan.items, used, nsplit,
        "exact" if probe == "impulse" else "%.3f" % (worst / R.GAMMA_WGRAD)))

    # ---- the Python routes end bit-equal to the direct call of the same instance (workspace and nsplit_used handling of kernels.py)
    direct = results[0]                                   # [group * 2 + (0: cwf_wgrad_reduce, 1: the batched reduce)]
    dev = torch.device(DEV)

    def sink():
        return [torch.full((wn,), float("nan"), device=DEV) for _ in range(G)], [torch.full((cout,), float("nan"), device=DEV) for _ in range(G)]

    def same(gws, gbs, k):
        torch.cuda.synchronize()
        for q in range(G):
            assert torch.equal(gws[q], direct[2 * q + k][0]), "a Python route differs from the direct call"
            assert not has_b or torch.equal(gbs[q], direct[2 * q + k][1])

    if c.form in ("dy4", "g2dy4"):
        return                                            # (kernels.cl copies a view that is not 16-byte aligned: Python never sends one)
    if grouped:
        gws, gbs = sink()
        hip.wgrad_to_grouped([("wgrad_bf16 exact", name, q) for q in range(G)], op, ops.xs, ops.dys, cout, [spec.inv_map] * G, gws, gbs, prec=mode)
        hip.wgrad_flush(dev)
        same(gws, gbs, 1)
        return
    if c.form in ("contig", "slice"):
        gw, gb = hip.wgrad(op, ops.xs[0], ops.sc, ops.sh, ops.slope, ops.dys[0], cout, spec.inv_map, has_b, wn, prec=mode)
        assert (gb is None) == (not has_b)
        same([gw], [gb], 0)
        gws, gbs = sink()
        hip.wgrad_to(("wgrad_bf16 exact", name), op, ops.xs[0], ops.sc, ops.sh, ops.slope, ops.dys[0], cout, spec.inv_map, gws[0],
                     gbs[0] if has_b else None, prec=mode)
        hip.wgrad_flush(dev)
        same(gws, gbs, 1)
        return
    # dy_scale and the image forms follow the precision setting, as in a training step
    kernels.set_precision("bf16x3", wgrad=mode, dgrad="bf16")
    try:
        nv = do * ho * wo
        if c.form == "dys":
            assert hip.dy_scale_ok(op, cin, cout, nv)
            variants = [dict(dy_scale=ops.s)]
        else:
            assert hip.bf16_operands_ok(op, cin, cout, nv) == (16 if cin == 16 else 32)
            variants = [dict(), dict(x16=ops.xa16), dict(dy16=ops.dy16), dict(x16=ops.xa16, dy16=ops.dy16)]      # images made inside / given
        for i, kw in enumerate(variants):
            gws, gbs = sink()
            hip.wgrad_to(("wgrad_bf16 exact", name, i), op, ops.xs[0], ops.sc, ops.sh, ops.slope, ops.dys[0], cout, spec.inv_map, gws[0], gbs[0], **kw)
            hip.wgrad_flush(dev)
            same(gws, gbs, 1)
    finally:
        kernels.set_precision("fp32")


def test_grouped_route_refuses_views_it_would_have_to_copy(hip):
    """wgrad_to_grouped passes the groups' own pointers with one shared row pitch: a group view that kernels.cl would copy (not 16-byte
    aligned) cannot be sent -- an error, not a launch with the copy's pitch on the original pointers"""
    from cwf import functional as CF
    c = T.BY_NAME["g2_dy4"]
    ops = _Operands(hip, c, "random")
    spec = CF.ConvSpec(c.op, c.cin, c.cout).to(torch.device(DEV))
    wn = math.prod(_wshape(c.op, c.cin, c.cout))
    gws, gbs = [torch.zeros(wn, device=DEV) for _ in range(2)], [torch.zeros(c.cout, device=DEV) for _ in range(2)]
    with pytest.raises(_lib.CwfError):
        hip.wgrad_to_grouped([("wgrad_bf16 refuse", q) for q in range(2)], c.op, ops.xs, ops.dys, c.cout, [spec.inv_map] * 2, gws, gbs, prec="bf16")
    hip.wgrad_flush(torch.device(DEV))
    torch.cuda.synchronize()
    assert all(bool((t == 0).all()) for t in gws + gbs)


def test_refused_descriptors_launch_nothing(hip):
    """what the query refuses, cwf_wgrad refuses with the same code before any launch: the slab buffer stays NaN"""
    refused = [("w16_cin16", "bf16", dict(dy_scale=True, dy_shift=4), T.E_BADARG), ("t71_s1_x3", "bf16x3", dict(x_shift=4), T.E_ALIGN),
               ("w16d", "bf16x3", {}, T.E_BADARG), ("s1d_32_32", "bf16", dict(groups=2), T.E_BADARG), ("g2_cout8", "bf16", dict(groups=4), T.E_BADARG)]
    for name, mode, edit, code in refused:
        c = T.BY_NAME[name]
        do, ho, wo = T.out_dims(c.op, *c.size)
        nsplit, slab = hip.lib.cwf_wgrad_nsplit(c.op, c.n, do, ho, wo, c.cin, c.cout), hip.lib.cwf_wgrad_slab_floats(c.op, c.cin, c.cout)
        ops = _Operands(hip, c, "random")
        parts = [torch.full((nsplit * slab + GUARD,), float("nan"), device=DEV) for _ in range(max(1, T.groups_of(c.form)))]
        a = ops.descriptor(hip, mode, parts)
        if edit.get("dy_scale"):
            a.dy_scale = torch.ones(c.n, c.cout, device=DEV).data_ptr()
        if "dy_shift" in edit:
            a.dy = a.dy + edit["dy_shift"]
        if "x_shift" in edit:
            a.x = a.x + edit["x_shift"]
        if "groups" in edit:
            a.groups = edit["groups"]
        assert T.query(hip.lib, a)[0] == code, name
        used = ctypes.c_int(-5)
        assert hip.lib.cwf_wgrad(ctypes.addressof(a), ctypes.addressof(used), hip._stream()) == code, name
        torch.cuda.synchronize()
        assert used.value == -5 and all(bool(p.isnan().all()) for p in parts), name


@pytest.mark.parametrize("batch,size", [(2, (128, 128, 128)), (1, (160, 192, 160))], ids=["bench_2x128", "patch_160x192x160"])
def test_model_layers_are_in_the_table(hip, batch, size):
    """every weight-gradient launch of one training step at the bench shape (batch 2 at 128^3) and at the 160 x 192 x 160 patch, in the
    bench precision, recorded as the descriptors cwf_wgrad receives: each maps to an (instance, tiles-per-range class) that a case of
    the table has as well.  A GPU test, because the list cannot be had from the ConvSpecs and the down / up-sampling structure alone: a
    ConvSpec holds (op, cin, cout) only, and what the plan depends on beyond the extents is decided per launch by the autograd glue
    while the step runs (cwf/functional.py) -- whether a layer hands over bf16 images, folds dy_scale, joins a grouped launch of the
    three heads, reads x or dy as a channel slice of a concatenation or head buffer (row pitch and pointer alignment), and which
    layers the fused specs of the couplers replace.  A hand-written list would be a second mirror of that glue, free to drift."""
    from cwf import kernels
    from cwf.trainer import Trainer
    from models.clswiseformer.cls_wise_former import get_cls_wise_former
    from utils import synthetic as syn
    table = set()
    for name, mode in T.RUNS:
        rc, p = T.query(hip.lib, T.dummy_descriptor(_lib, T.BY_NAME[name], mode))
        assert rc == 0
        table.add((p.inst, T.tiles_class(p)))
    seen, real_call = [], hip._call

    def recording_call(fn, *args):
        if fn == "cwf_wgrad":
            a = _lib.WgradArgs.from_buffer_copy(ctypes.string_at(args[0], ctypes.sizeof(_lib.WgradArgs)))
            seen.append(a)
        return real_call(fn, *args)

    kernels.set_precision("bf16x3", wgrad="bf16", dgrad="bf16")
    hip._call = recording_call
    try:
        torch.manual_seed(0)
        m = get_cls_wise_former(dataset="brats", _conv_repr=True, _pe_type="fixed").to(DEV).train()
        tr = Trainer(m)
        x, target, edge = syn.synthetic_batch(list(range(batch)), size)
        tr._fwd_bwd(x.to(DEV), target.to(DEV), edge.to(DEV))
        hip.join_wgrad_stream()
        torch.cuda.synchronize()
    finally:
        del hip._call
        kernels.set_precision("fp32")
    assert len(seen) >= 40, len(seen)
    missing, census = set(), {}
    for a in seen:
        rc, p = T.query(hip.lib, a)
        assert rc == 0, rc
        key = (p.inst, T.tiles_class(p))
        census[key] = census.get(key, 0) + 1
        if key not in table:
            missing.add((T.NAME_OF[p.inst], T.tiles_class(p), a.op, a.Cin, a.Cout, (a.Di, a.Hi, a.Wi), a.groups))
    print("\nmodel layers %d x %s: %d launches: %s" % (batch, size, len(seen), sorted((T.NAME_OF[k[0]], k[1], v) for k, v in census.items())))
    for row in sorted(missing):
        print("model layer outside the table:", row)
    assert not missing, sorted(missing)


def test_every_instance_launched(hip):
    """the census: the instances that LAUNCHED in this file are all of them.  Runs of the table that did not take place in this session
    (a selection with -k) are launched here on random operands, without the reference."""
    for name, mode in T.RUNS:
        if (name, mode) not in LAUNCHED:
            c = T.BY_NAME[name]
            do, ho, wo = T.out_dims(c.op, *c.size)
            _launch(hip, _Operands(hip, c, "random"), mode, hip.lib.cwf_wgrad_nsplit(c.op, c.n, do, ho, wo, c.cin, c.cout),
                    hip.lib.cwf_wgrad_slab_floats(c.op, c.cin, c.cout))
    assert set(LAUNCHED.values()) == set(range(T.COUNT)), sorted(T.NAME_OF[i] for i in set(range(T.COUNT)) - set(LAUNCHED.values()))
