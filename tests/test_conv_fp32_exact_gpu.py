"""GPU: the exact-fp32 conv family -- conv_mfma_kernel (forward, data gradient; csrc/conv_mfma.hip) and wgrad_mfma_kernel with both
slab reduces (csrc/wgrad_mfma.hip) -- against the operand-exact float64 reference of tests/bf16_operand_ref.py in "fp32" mode:
|got - ref| <= gamma_fp32(chain) * A elementwise, chain read from the launch (see the derivation there).  Probes:
  random    zero-mean operands with every prologue / epilogue feature the path takes, ragged extents, batch >= 2
  positive  all-positive operands (no cancellation: dropped or duplicated work shows at full size)
  impulse   input (or dy) zero except isolated bf16 values, bf16 weights: every output is ONE exact product -- bit for bit
  constant  x = 0, scale 1, shift != 0: the activated shift reaches only in-bounds taps (padding after activation)
Every configuration choose_cfg can return and every wgrad_mfma_kernel instance is asserted through the read-only plan queries
(cwf_debug_conv_fp32_cfg, cwf_debug_wgrad_fp32_plan); the slab chain runs on NaN-filled workspaces and outputs."""
import ctypes
import math
import struct

import pytest
import torch

import bf16_operand_ref as R
from cwf import _lib, packing as pk

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PROBES = ["random", "positive", "impulse"]
ALL_CFGS = {(4, 4, 1), (2, 4, 2), (2, 4, 4), (4, 2, 4), (4, 1, 4), (1, 4, 4), (1, 2, 4), (1, 2, 2), (1, 1, 4)}
NTAPS = {pk.CONV3_S1: 27, pk.CONV3_S2: 27, pk.CONV1: 1, pk.CONVT2: 1, pk.CONV3_S2_DGRAD: 8, pk.CONVT2_DGRAD: 8}
TILE_VOXELS = {pk.CONV3_S1: 256, pk.CONV3_S2: 64, pk.CONV1: 256, pk.CONVT2: 256}      # make_plan: MTOT 16 (4 for stride 2) x 16


def _u(*shape, seed, lo_=-1.0, hi_=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(*shape, generator=g) * (hi_ - lo_) + lo_


def _bf(t):
    return t.to(torch.bfloat16).float()


def _wshape(op, cin, cout):
    return (cin, cout, 2, 2, 2) if op == pk.CONVT2 else ((cout, cin, 1, 1, 1) if op == pk.CONV1 else (cout, cin, 3, 3, 3))


def _weights(op, cin, cout, probe, seed):
    shape = _wshape(op, cin, cout)
    s = 1.0 / math.sqrt(cin * shape[2] ** 3)
    w = _u(*shape, seed=seed, lo_=0.5 * s if probe == "positive" else -s, hi_=s)
    return _bf(w) if probe == "impulse" else w


def _impulses(shape, seed, per_channel=False):
    """zero except isolated bf16-representable values, pairwise >= 3 voxels apart: corners, face centres, the last (ragged) tile of
    each dimension, in the first and last sample (per_channel: one impulse per channel, for weight gradients)"""
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
    if per_channel:
        for ch in range(c):
            x[keep[ch % len(keep)] + (ch,)] = vals[ch % len(vals)] * (1 + ch // len(keep))
        return x
    for i, p in enumerate(keep):
        x[p + ((c - 1) if i % 2 == 0 else (i * 5) % c,)] = vals[i % len(vals)]
    return x


def _field(shape, probe, seed):
    if probe == "positive":
        return _u(*shape, seed=seed, lo_=0.5, hi_=1.0)
    if probe == "impulse":
        return _impulses(shape, seed)
    return _u(*shape, seed=seed)


def _packed(op, cin, cout, w):
    from cwf import functional as CF, kernels
    spec = CF.ConvSpec(op, cin, cout)
    packer = CF.WeightPacker()
    packer.add(spec, torch.nn.Parameter(w.to(DEV).contiguous()))
    kernels.set_precision("fp32")
    packer.refresh()
    spec._keepalive = packer
    return spec


def _record(path, worst, gamma):
    """one line per checked result (visible with -s): the worst err / A in units of the path's gamma"""
    print("\nworst err/(gamma A)  %-34s %.3f  (gamma 2^%.2f)" % (path, worst / gamma, math.log2(gamma)))


def _check(got, ref, gamma, path, probe, what):
    if probe == "impulse":
        g = ref.pick(got)
        assert torch.equal(g, ref.y), (path, what, float((g - ref.y).abs().max()))
        return
    _record(path + " " + probe, R.check(got, ref, gamma, "%s %s %s" % (path, probe, what)), gamma)


def _cfg(hip, op, n, in_dims, out_dims, cout):
    a = (ctypes.c_int * 3)()
    assert hip.lib.cwf_debug_conv_fp32_cfg(op, n, *in_dims, *out_dims, cout, a) == 0
    return tuple(a)


def _plan(hip, op, n, size, cin, cout):
    """cwf_debug_wgrad_fp32_plan: {tapsplit, CG, nsplit, tiles per split, slab floats, tiles}"""
    a = (ctypes.c_int64 * 6)()
    assert hip.lib.cwf_debug_wgrad_fp32_plan(op, n, *size, cin, *pk.out_dims(op, *size), cout, a) == 0
    return tuple(int(v) for v in a)


# ====================================================================================================== forward
# path: (op, cin, cout, size, n, features).  p = InstanceNorm + LeakyReLU(0.01) prologue, 1 = the prologue with slope 1 (affine only),
# b = bias, r = residual, o = out_scale, s = statistics, S = into a channel slice of a wider buffer (guard channels),
# X = input read from a channel slice of a concatenation buffer (x_ldc > cin)
FWD = {
    "s1_cin4_w33": (pk.CONV3_S1, 4, 16, (8, 12, 33), 2, "pbrosX"),
    "s1_cin8_cout2_w15": (pk.CONV3_S1, 8, 2, (6, 7, 15), 2, "pbos"),
    "s1_cin20_cout48_w17": (pk.CONV3_S1, 20, 48, (5, 9, 17), 2, "1brosSX"),
    "s1_cout4_w1": (pk.CONV3_S1, 16, 4, (5, 6, 1), 2, "pbs"),
    "s1_cin256": (pk.CONV3_S1, 256, 16, (6, 5, 33), 2, "pbrs"),
    "s1_cout256_441": (pk.CONV3_S1, 16, 256, (16, 32, 17), 2, "pbsS"),
    "s2": (pk.CONV3_S2, 32, 64, (10, 12, 35), 2, "pbosS"),
    "s2_cin8_cout8_w33": (pk.CONV3_S2, 8, 8, (9, 7, 33), 2, "1brsX"),
    "conv1": (pk.CONV1, 256, 128, (4, 5, 9), 2, "pboS"),
    "conv1_cin20_cout48": (pk.CONV1, 20, 48, (3, 5, 17), 2, "1brsX"),
    "convT_144": (pk.CONVT2, 16, 256, (2, 9, 2), 3, "pbsS"),
    "convT_cout8_w15": (pk.CONVT2, 32, 8, (3, 4, 15), 2, "pbrosX"),
}


@pytest.mark.parametrize("probe", PROBES + ["constant"])
@pytest.mark.parametrize("path", list(FWD))
def test_forward_is_operand_exact(hip, path, probe):
    op, cin, cout, size, n, feat = FWD[path]
    pro = "p" in feat or "1" in feat
    assert pro or probe != "constant"
    imp, pos = probe == "impulse", probe == "positive"
    x = _field((n, *size, cin), probe, seed=1)
    w = _weights(op, cin, cout, probe, seed=2)
    b = None if imp or "b" not in feat else _u(cout, seed=3, lo_=0.0 if pos else -0.1, hi_=0.1)
    sc = sh = None
    slope = 1.0
    if pro and not imp:
        sc, sh = _u(n, cin, seed=4, lo_=0.5, hi_=1.5), _u(n, cin, seed=5, lo_=0.0 if pos else -1.0)
        slope = 0.01 if "p" in feat else 1.0
    if probe == "constant":
        x = torch.zeros_like(x)
        sc, sh = torch.ones(n, cin), torch.linspace(-0.75, 1.5, cin).repeat(n, 1)
    do, ho, wo = pk.out_dims(op, *size)
    res = _field((n, do, ho, wo, cout), "positive" if pos else "random", seed=6) if ("r" in feat and not imp) else None
    osc = None
    if "o" in feat and not imp:
        osc = _u(n, cout, seed=7, lo_=0.5, hi_=1.5) if pos else (_u(n, cout, seed=7) > -0.5).float() * 1.25
    spec = _packed(op, cin, cout, w)
    st = hip.new_stats(n, cout, DEV) if "s" in feat else None
    xd = x.to(DEV)
    if "X" in feat:                                       # a channel slice of a concatenation buffer: x_ldc = cin + 12
        cat = torch.full((n, *size, cin + 12), float("nan"), device=DEV)
        cat[..., 8:8 + cin] = xd
        xd = cat[..., 8:8 + cin]
    kw = {}
    if "S" in feat:
        wide = torch.full((n, do, ho, wo, cout + 8), 7.0, device=DEV)
        kw["out"] = wide[..., 4:4 + cout]
    dv = lambda t: None if t is None else t.to(DEV)
    y = hip.conv(op, xd, spec.wpk_f, dv(b), cout, dv(sc), dv(sh), slope, dv(res), dv(osc), st, prec="fp32", **kw)
    torch.cuda.synchronize()
    ref = R.conv_ref(op, x, w, "fp32", bias=b, in_scale=sc, in_shift=sh, slope=slope, residual=res, out_scale=osc)
    gamma = R.gamma_fp32(R.conv_chain_fp32(cin, NTAPS[op]))
    _check(y, ref, gamma, "fwd " + path, probe, "forward")
    if st is not None and not imp:
        R.assert_stats(st, ref, gamma, path)
    if "S" in feat:
        assert bool((wide[..., :4] == 7.0).all()) and bool((wide[..., 4 + cout:] == 7.0).all()), "wrote outside its channel slice"


@pytest.mark.parametrize("probe", PROBES)
@pytest.mark.parametrize("cin,cout,size,n,G", [(32, 8, (8, 12, 16), 2, 3), (16, 16, (6, 8, 20), 2, 2), (8, 4, (5, 6, 17), 2, 3)])
def test_grouped_forward_is_operand_exact(hip, cin, cout, size, n, G, probe):
    """cwf_conv with groups in fp32: one conv_mfma_kernel launch per group; other groups' channels and the guard stay as written"""
    ca = cout + 4
    x_all = _field((n, *size, G * cin), probe, seed=21)
    ws = [_weights(pk.CONV3_S1, cin, cout, probe, seed=22 + q) for q in range(G)]
    bs = [None if probe == "impulse" else _u(cout, seed=32 + q, lo_=0.0 if probe == "positive" else -0.1, hi_=0.1) for q in range(G)]
    specs = [_packed(pk.CONV3_S1, cin, cout, w) for w in ws]
    y_all = torch.full((n, *size, G * ca + 4), 5.0, device=DEV)
    hip.conv_grouped(x_all.to(DEV), cin, [s.wpk_f for s in specs], [None if b is None else b.to(DEV) for b in bs], cout, y_all[..., :G * ca],
                     x_goff=cin, y_goff=ca, prec="fp32")
    gamma = R.gamma_fp32(R.conv_chain_fp32(cin, 27))
    for q in range(G):
        ref = R.conv_ref(pk.CONV3_S1, x_all[..., q * cin:(q + 1) * cin], ws[q], "fp32", bias=bs[q])
        _check(y_all[..., q * ca:q * ca + cout], ref, gamma, "grouped fwd", probe, "group %d" % q)
        assert bool((y_all[..., q * ca + cout:(q + 1) * ca] == 5.0).all()), "group %d wrote outside its channels" % q
    assert bool((y_all[..., G * ca:] == 5.0).all())


# ====================================================================================================== data gradient
# path: (forward op, cin, cout, forward input size, n, features): r = residual (carried gradient)
DGRAD = {
    "s1_transposed": (pk.CONV3_S1, 32, 16, (9, 10, 20), 2, "r"),
    "s1_cin4_w33": (pk.CONV3_S1, 4, 16, (8, 12, 33), 2, ""),
    "s1_cin256_w1": (pk.CONV3_S1, 256, 48, (4, 6, 1), 2, "r"),
    "s2_dgrad": (pk.CONV3_S2, 16, 32, (16, 16, 33), 2, "r"),
    "s2_dgrad_odd": (pk.CONV3_S2, 8, 16, (7, 9, 15), 2, ""),
    "convT_dgrad": (pk.CONVT2, 32, 32, (4, 5, 9), 2, "r"),
    "convT_dgrad_cin20": (pk.CONVT2, 20, 8, (3, 4, 17), 2, ""),
    "conv1": (pk.CONV1, 32, 16, (8, 8, 32), 2, "r"),
    "conv1_cin48_cout20": (pk.CONV1, 48, 20, (3, 5, 17), 2, ""),
}


@pytest.mark.parametrize("probe", PROBES)
@pytest.mark.parametrize("path", list(DGRAD))
def test_data_gradient_is_operand_exact(hip, path, probe):
    op, cin, cout, size, n, feat = DGRAD[path]
    w = _weights(op, cin, cout, probe, seed=51)
    do, ho, wo = pk.out_dims(op, *size)
    dy = _field((n, do, ho, wo, cout), probe, seed=52)
    imp = probe == "impulse"
    res = _field((n, *size, cin), "positive" if probe == "positive" else "random", seed=53) if ("r" in feat and not imp) else None
    spec = _packed(op, cin, cout, w)
    assert spec.cout_alloc == cout
    dx = hip.conv(pk.dgrad_op(op), dy.to(DEV), spec.wpk_d, None, cin, residual=None if res is None else res.to(DEV),
                  out=torch.empty((n, *size, cin), device=DEV), prec="fp32", fwd_op=op)
    torch.cuda.synchronize()
    ref = R.conv_ref(op, dy, w, "fp32", residual=res, dgrad=True, out_size=size)
    gamma = R.gamma_fp32(R.conv_chain_fp32(cout, NTAPS[pk.dgrad_op(op)]))
    _check(dx, ref, gamma, "dgrad " + path, probe, "dx")
    if op == pk.CONV3_S2:                                # each of the eight output-parity classes on its own
        got = dx.cpu().double()
        for c in range(8):
            p = ((c >> 2) & 1, (c >> 1) & 1, c & 1)
            sl = (slice(None), slice(p[0], None, 2), slice(p[1], None, 2), slice(p[2], None, 2))
            assert ref.y[sl].numel() > 0
            if imp:
                assert torch.equal(got[sl], ref.y[sl]), ("parity class", p)
            else:
                R.assert_operand_exact(got[sl], ref.y[sl], ref.A[sl], gamma, "%s parity class %s" % (path, p))


# ====================================================================================================== tile configurations
def _s2_dgrad_cfg(hip, n, size, cin):
    return _cfg(hip, pk.CONV3_S2_DGRAD, n, pk.out_dims(pk.CONV3_S2, *size), size, cin)


# stride-2 data gradients that reach each configuration of conv_fp32_launch: (expected cfg, forward cin, forward cout, forward input
# size, n)
CFG_CASES = [
    ((1, 1, 4), 16, 16, (4, 4, 5), 1),
    ((1, 2, 2), 128, 16, (5, 10, 6), 3),
    ((1, 2, 4), 256, 16, (5, 5, 6), 2),
    ((1, 4, 4), 256, 16, (4, 20, 5), 3),
    ((2, 4, 2), 256, 16, (10, 10, 33), 2),
    ((2, 4, 4), 256, 16, (10, 5, 33), 3),
    ((4, 1, 4), 128, 16, (8, 32, 9), 2),
    ((4, 2, 4), 256, 16, (8, 32, 9), 2),
    ((4, 4, 1), 256, 16, (32, 5, 33), 2),
]


def test_tile_configuration_table_reaches_every_configuration(hip):
    got = {_s2_dgrad_cfg(hip, n, size, cin) for (_, cin, _, size, n) in CFG_CASES}
    assert got == ALL_CFGS, sorted(ALL_CFGS - got)
    for cfg, cin, cout, size, n in CFG_CASES:
        assert _s2_dgrad_cfg(hip, n, size, cin) == cfg
    # the forward shapes of FWD that take distinct configurations
    assert _cfg(hip, pk.CONV3_S1, 2, (16, 32, 17), (16, 32, 17), 256) == (4, 4, 1)
    assert _cfg(hip, pk.CONVT2, 3, (2, 9, 2), (4, 18, 4), 256) == (1, 4, 4)
    assert _cfg(hip, pk.CONV3_S2, 2, (10, 12, 35), pk.out_dims(pk.CONV3_S2, 10, 12, 35), 64) == (1, 1, 4)
    # the stride-2 rule: no configuration with MT * WM > 4 for the stride-2 forward / ConvTranspose data gradient (2x input tile)
    seen = set()
    for op in (pk.CONV3_S2, pk.CONVT2_DGRAD):
        for dims in ((4, 4, 8), (8, 8, 16), (16, 16, 32), (32, 32, 64), (64, 64, 64)):
            for c in (16, 64, 256):
                for n in (1, 2):
                    m, nt, wm = _cfg(hip, op, n, tuple(2 * v for v in dims), dims, c)
                    assert m * wm <= 4, (op, dims, c, (m, nt, wm))
                    seen.add((m, nt, wm))
    assert len(seen) >= 3, seen                          # (the rule is exercised, not vacuous)


@pytest.mark.parametrize("probe", PROBES)
@pytest.mark.parametrize("cfg,cin,cout,size,n", CFG_CASES, ids=["%d%d%d" % c[0] for c in CFG_CASES])
def test_every_tile_configuration_is_operand_exact(hip, cfg, cin, cout, size, n, probe):
    """conv_mfma_kernel at each configuration, as the stride-2 data gradient (all eight parity classes) with a residual"""
    op = pk.CONV3_S2
    assert _s2_dgrad_cfg(hip, n, size, cin) == cfg
    w = _weights(op, cin, cout, probe, seed=61)
    dy = _field((n, *pk.out_dims(op, *size), cout), probe, seed=62)
    res = None if probe == "impulse" else _field((n, *size, cin), "positive" if probe == "positive" else "random", seed=63)
    spec = _packed(op, cin, cout, w)
    dx = hip.conv(pk.CONV3_S2_DGRAD, dy.to(DEV), spec.wpk_d, None, cin, residual=None if res is None else res.to(DEV),
                  out=torch.empty((n, *size, cin), device=DEV), prec="fp32", fwd_op=op)
    ref = R.conv_ref(op, dy, w, "fp32", residual=res, dgrad=True, out_size=size)
    _check(dx, ref, R.gamma_fp32(R.conv_chain_fp32(cout, 8)), "cfg %d%d%d" % cfg, probe, "dx")


@pytest.mark.parametrize("cfg,cin,cout,size,n", [((4, 4, 1), 16, 256, (16, 32, 17), 2), ((1, 4, 4), 16, 256, (2, 9, 2), 3)])
def test_forward_statistics_of_wide_tiles(hip, cfg, cin, cout, size, n):
    """the statistics of the widest tiles (512 (channel, sum) pairs for 256 threads at {4, 4, 1}) with the elementwise bound propagated"""
    op = pk.CONV3_S1 if cfg == (4, 4, 1) else pk.CONVT2
    assert _cfg(hip, op, n, size, pk.out_dims(op, *size), cout) == cfg
    x, w = _u(n, *size, cin, seed=91, lo_=0.0), _weights(op, cin, cout, "random", 92)
    spec = _packed(op, cin, cout, w)
    st = hip.new_stats(n, cout, DEV)
    y = hip.conv(op, x.to(DEV), spec.wpk_f, None, cout, stats=st, prec="fp32")
    ref = R.conv_ref(op, x, w, "fp32")
    gamma = R.gamma_fp32(R.conv_chain_fp32(cin, NTAPS[op]))
    _record("fwd stats %d%d%d" % cfg, R.check(y, ref, gamma, "fwd"), gamma)
    R.assert_stats(st, ref, gamma, "stats %s" % (cfg,))


# ====================================================================================================== large layers (sampled voxels)
@pytest.mark.parametrize("op,cin,cout,size,n", [(pk.CONV3_S1, 16, 16, (64, 64, 64), 2), (pk.CONV3_S2, 16, 32, (64, 66, 70), 1),
                                                (pk.CONV3_S1, 4, 16, (68, 64, 65), 1)])
def test_large_layers_at_sampled_voxels(hip, op, cin, cout, size, n):
    x, w = _u(n, *size, cin, seed=101), _weights(op, cin, cout, "random", 102)
    b, sc, sh = _u(cout, seed=103, lo_=-0.1, hi_=0.1), _u(n, cin, seed=104, lo_=0.5, hi_=1.5), _u(n, cin, seed=105)
    spec = _packed(op, cin, cout, w)
    y = hip.conv(op, x.to(DEV), spec.wpk_f, b.to(DEV), cout, sc.to(DEV), sh.to(DEV), 0.01, prec="fp32")
    dims = pk.out_dims(op, *size)
    vox = R.edge_voxels(n, dims)
    ref = R.conv_ref(op, x, w, "fp32", bias=b, in_scale=sc, in_shift=sh, slope=0.01, vox=vox)
    gamma = R.gamma_fp32(R.conv_chain_fp32(cin, 27))
    _record("fwd large %s" % (size,), R.check(y, ref, gamma, "large fwd"), gamma)
    dy = _u(n, *dims, cout, seed=106)
    dx = hip.conv(pk.dgrad_op(op), dy.to(DEV), spec.wpk_d, None, cin, out=torch.empty((n, *size, cin), device=DEV), prec="fp32", fwd_op=op)
    vox = R.edge_voxels(n, size)
    ref = R.conv_ref(op, dy, w, "fp32", dgrad=True, out_size=size, vox=vox)
    gamma = R.gamma_fp32(R.conv_chain_fp32(cout, NTAPS[pk.dgrad_op(op)]))
    _record("dgrad large %s" % (size,), R.check(dx, ref, gamma, "large dgrad"), gamma)


# ====================================================================================================== weight gradient
# case: (op, cin, cout, size, n, expected plan {tapsplit, CG, nsplit, tiles per split, ragged last split})
WGRAD = {
    "ts_cg1_nsplit1": (pk.CONV3_S1, 16, 16, (4, 4, 16), 1, (1, 1, 1, 1, False)),
    "ts_cg1_nsplit2_batch": (pk.CONV3_S1, 16, 16, (4, 4, 16), 2, (1, 1, 2, 1, False)),
    "ts_cg1_nsplit3_cin4": (pk.CONV3_S1, 4, 16, (12, 4, 16), 1, (1, 1, 3, 1, False)),
    "ts_cg1_nsplit5_w13": (pk.CONV3_S1, 16, 8, (20, 4, 13), 1, (1, 1, 5, 1, False)),
    "ts_cg2_nsplit17_ragged": (pk.CONV3_S1, 256, 32, (12, 44, 16), 1, (1, 2, 17, 2, True)),
    "ts_cg1_cin20_cout2": (pk.CONV3_S1, 20, 2, (6, 7, 15), 2, (1, 1, 8, 1, False)),
    "ts_cg2_s2": (pk.CONV3_S2, 16, 32, (16, 16, 33), 2, (1, 2, 64, 1, False)),
    "ts_cg2_cout48": (pk.CONV3_S1, 32, 48, (6, 8, 20), 2, (1, 2, 16, 1, False)),
    "1tap_cg1_conv1": (pk.CONV1, 32, 16, (8, 8, 32), 2, (0, 1, 64, 1, False)),
    "1tap_cg2_convT": (pk.CONVT2, 32, 32, (4, 5, 9), 2, (0, 2, 16, 1, False)),
    "1tap_cg4_conv1": (pk.CONV1, 16, 48, (5, 6, 17), 2, (0, 4, 64, 1, False)),
    "1tap_cg4_convT_cin20": (pk.CONVT2, 20, 48, (3, 5, 7), 2, (0, 4, 16, 1, False)),
    "large_64": (pk.CONV3_S1, 16, 16, (64, 64, 64), 2, (1, 1, 512, 4, False)),
}


def test_weight_gradient_plan_table_reaches_every_instance(hip):
    """the five wgrad_mfma_kernel instances {27-tap: CG 1, 2; 1-tap: CG 1, 2, 4} and the nsplit edges of the batched reduce (four
    lanes, step-16 main loop, step-4 tail): nsplit 1, 2, 3, 5, 17 (> 16, not a multiple of 4), a ragged last split"""
    inst, nsplits, ragged = set(), set(), False
    for name, (op, cin, cout, size, n, want) in WGRAD.items():
        p = _plan(hip, op, n, size, cin, cout)
        assert p[:4] == want[:4], (name, p)
        assert (p[5] % p[3] != 0) == want[4], (name, p)
        assert p[4] == hip.lib.cwf_wgrad_slab_floats(op, cin, cout), name          # the shape-only size Python allocates by
        assert p[2] == hip.lib.cwf_wgrad_nsplit(op, n, *pk.out_dims(op, *size), cin, cout), name
        inst.add(p[:2])
        nsplits.add(p[2])
        ragged |= want[4]
    assert inst == {(1, 1), (1, 2), (0, 1), (0, 2), (0, 4)}, inst
    assert {1, 2, 3, 5, 17} <= nsplits and ragged


def _wgrad_inputs(op, cin, cout, size, n, probe):
    do, ho, wo = pk.out_dims(op, *size)
    imp = probe == "impulse"
    x = _bf(_u(n, *size, cin, seed=71)) if imp else _field((n, *size, cin), probe, seed=71)
    dy = _impulses((n, do, ho, wo, cout), 0, per_channel=True) if imp else _field((n, do, ho, wo, cout), probe, seed=72)
    sc, sh, slope = None, None, 1.0
    if not imp:
        sc, sh, slope = _u(n, cin, seed=73, lo_=0.5, hi_=1.5), _u(n, cin, seed=74, lo_=0.0 if probe == "positive" else -1.0), 0.01
    if probe == "constant":
        x = torch.zeros_like(x)
        sc, sh = torch.ones(n, cin), torch.linspace(-1.0, 1.0, cin).repeat(n, 1)
    return x, dy, sc, sh, slope


def _reduce_batched(hip, part, inv, dw, db, slab, nsplit):
    raw = struct.pack("<QQQQqii", part.data_ptr(), inv.data_ptr(), dw.data_ptr(), 0 if db is None else db.data_ptr(), slab, nsplit, 0)
    table = torch.frombuffer(bytearray(raw), dtype=torch.uint8).to(DEV)
    assert hip.lib.cwf_wgrad_reduce_batched(table.data_ptr(), 1, hip._stream()) == 0
    torch.cuda.synchronize()


WGRAD_RUNS = [(p, q) for p in WGRAD for q in (PROBES + ["constant"] if p != "large_64" else ["random"])]     # (one probe at 64^3)


@pytest.mark.parametrize("path,probe", WGRAD_RUNS)
def test_weight_gradient_is_operand_exact(hip, path, probe):
    """cwf_wgrad (fp32) into a NaN-filled workspace, then each reduce into NaN-filled dW / db with guards: every slab slot of the
    nsplit slabs written, nothing beyond them; dW / db fully written, guards untouched; both reduces against the reference and
    bitwise reproducible; the Python paths (hip.wgrad, wgrad_to + wgrad_flush) likewise"""
    from cwf import functional as CF
    op, cin, cout, size, n, want = WGRAD[path]
    plan = _plan(hip, op, n, size, cin, cout)
    _, _, nsplit, tps, slab, _ = plan
    x, dy, sc, sh, slope = _wgrad_inputs(op, cin, cout, size, n, probe)
    dw_ref, db_ref, aw, ab = R.wgrad_ref(op, x, dy, "fp32", sc, sh, slope)
    gamma = R.gamma_fp32(R.wgrad_chain_fp32(tps, TILE_VOXELS[op], nsplit))
    spec = CF.ConvSpec(op, cin, cout).to(torch.device(DEV))
    assert spec.inv_map.numel() == slab
    has_b = spec.has_bias_map                            # (ConvTranspose slabs carry no bias row: its bias gradient is a channel sum)
    assert has_b == (op != pk.CONVT2)
    wn = math.prod(_wshape(op, cin, cout))
    dv = lambda t: None if t is None else t.to(DEV)
    ca = (cout + 3) // 4 * 4                             # dy in rows of ca floats (a 2-channel gradient lives in 4-channel rows)
    xd = x.to(DEV)
    dbuf = torch.zeros((*dy.shape[:4], ca), device=DEV)
    dbuf[..., :cout] = dy.to(DEV)
    dyd = dbuf[..., :cout]

    def check(gw, gb, what):
        gw, gb = gw.reshape(dw_ref.shape).cpu().double(), gb.cpu().double()
        if probe == "impulse":
            assert torch.equal(gw, dw_ref), (path, what, float((gw - dw_ref).abs().max()))
            assert not has_b or torch.equal(gb, db_ref), (path, what, float((gb - db_ref).abs().max()))
            return
        _record("wgrad %s %s %s" % (path, what, probe), R.assert_operand_exact(gw, dw_ref, aw, gamma, "%s %s dW" % (path, what)), gamma)
        if has_b:
            _record("bgrad %s %s %s" % (path, what, probe), R.assert_operand_exact(gb, db_ref, ab, gamma, "%s %s db" % (path, what)), gamma)

    G = 64                                               # guard floats around every buffer
    results = []
    for rep in range(2):
        part_all = torch.full((nsplit * slab + G,), float("nan"), device=DEV)
        a = hip._wgrad_args(op, xd, cin, dv(sc), dv(sh), slope, dyd, ca, cout, part_all, "fp32")
        used = ctypes.c_int(0)
        assert hip.lib.cwf_wgrad(ctypes.addressof(a), ctypes.addressof(used), hip._stream()) == 0
        torch.cuda.synchronize()
        assert used.value == nsplit
        assert bool(torch.isfinite(part_all[:nsplit * slab]).all()), "a slab slot the reduce reads was not written"
        assert bool(part_all[nsplit * slab:].isnan().all()), "written beyond the nsplit slabs"
        outs = []
        for which in ("reduce", "batched"):
            dw_all = torch.full((wn + 2 * G,), float("nan"), device=DEV)
            db_all = torch.full((cout + 2 * G,), float("nan"), device=DEV)
            dw, db = dw_all[G:G + wn], db_all[G:G + cout]
            dbp = db if has_b else None
            if which == "reduce":
                assert hip.lib.cwf_wgrad_reduce(part_all.data_ptr(), nsplit, slab, spec.inv_map.data_ptr(), dw.data_ptr(),
                                                0 if dbp is None else dbp.data_ptr(), hip._stream()) == 0
                torch.cuda.synchronize()
            else:
                _reduce_batched(hip, part_all, spec.inv_map, dw, dbp, slab, nsplit)
            for g_ in (dw_all[:G], dw_all[G + wn:], db_all[:G], db_all[G + cout:]) + (() if has_b else (db,)):
                assert bool(g_.isnan().all()), (which, "wrote outside dW / db")
            if rep == 0:
                check(dw, db, which)
            outs.append((dw.clone(), db.clone()))
        results.append(outs)
    for k in range(2):                                   # each reduce: bitwise the same over two runs
        assert torch.equal(results[0][k][0], results[1][k][0]) and (not has_b or torch.equal(results[0][k][1], results[1][k][1]))
    # the Python paths: hip.wgrad (workspace from the grow-only cache, cwf_wgrad_reduce) and wgrad_to + wgrad_flush (persistent slab
    # buffer, the batched reduce)
    gw, gb = hip.wgrad(op, xd, dv(sc), dv(sh), slope, dyd, cout, spec.inv_map, has_b, wn, prec="fp32")
    torch.cuda.synchronize()
    assert torch.equal(gw, results[0][0][0]) and (gb is None) == (not has_b) and (gb is None or torch.equal(gb, results[0][0][1]))
    gw2, gb2 = torch.full((wn,), float("nan"), device=DEV), torch.full((cout,), float("nan"), device=DEV)
    hip.wgrad_to(("fp32 exact", path), op, xd, dv(sc), dv(sh), slope, dyd, cout, spec.inv_map, gw2, gb2 if has_b else None, prec="fp32")
    hip.wgrad_flush(torch.device(DEV))
    torch.cuda.synchronize()
    assert torch.equal(gw2, results[0][1][0]) and (not has_b or torch.equal(gb2, results[0][1][1]))


def test_weight_gradient_of_strided_views(hip):
    """x from a concatenation buffer (x_ldc > cin) and dy from a channel slice of a wider buffer (dy_ldc > cout, unaligned start)"""
    op, cin, cout, size, n = pk.CONV3_S1, 20, 12, (6, 8, 19), 2
    from cwf import functional as CF
    x, dy, sc, sh, slope = _wgrad_inputs(op, cin, cout, size, n, "random")
    xw = torch.full((n, *size, cin + 12), float("nan"), device=DEV); xw[..., 4:4 + cin] = x.to(DEV)
    dw_ = torch.full((n, *size, cout + 9), float("nan"), device=DEV); dw_[..., 5:5 + cout] = dy.to(DEV)
    spec = CF.ConvSpec(op, cin, cout).to(torch.device(DEV))
    wn = math.prod(_wshape(op, cin, cout))
    gw, gb = hip.wgrad(op, xw[..., 4:4 + cin], sc.to(DEV), sh.to(DEV), slope, dw_[..., 5:5 + cout], cout, spec.inv_map, True, wn, prec="fp32")
    p = _plan(hip, op, n, size, cin, cout)
    gamma = R.gamma_fp32(R.wgrad_chain_fp32(p[3], TILE_VOXELS[op], p[2]))
    dw_ref, db_ref, aw, ab = R.wgrad_ref(op, x, dy, "fp32", sc, sh, slope)
    _record("wgrad strided views", R.assert_operand_exact(gw.view(dw_ref.shape), dw_ref, aw, gamma, "strided dW"), gamma)
    R.assert_operand_exact(gb, db_ref, ab, gamma, "strided db")


# ====================================================================================================== refusals
def _conv_call(hip, op, x_ptr, x_ldc, cin, wpk, y, cout, n, size, **kw):
    do, ho, wo = pk.out_dims(op, *size)
    a = _lib.ConvArgs(op=op, precision=_lib.PRECISION["fp32"], x=x_ptr, x_ldc=x_ldc, wpk=wpk.data_ptr(), y=y.data_ptr(), y_ldc=cout,
                      in_slope=1.0, nb_slope=1.0, N=n, Di=size[0], Hi=size[1], Wi=size[2], Cin=cin, Do=do, Ho=ho, Wo=wo, Cout=cout, **kw)
    return hip.lib.cwf_conv(ctypes.addressof(a), hip._stream())


def test_fp32_refusals(hip):
    """what the fp32 routes cannot honour is an error, never a different computation: the norm-backward sums (nb_x) and dy_scale in
    fp32, Cin % 4 != 0, a misaligned x -- and nothing is written"""
    n, size, cin, cout = 1, (4, 4, 16), 16, 16
    spec = _packed(pk.CONV3_S1, cin, cout, _weights(pk.CONV3_S1, cin, cout, "random", 1))
    buf = torch.zeros(n * 4 * 4 * 16 * cin + 8, device=DEV)
    y = torch.full((n, *size, cout), 3.0, device=DEV)
    st = hip.new_stats(n, cout, DEV)
    sc = torch.ones(n, cout, device=DEV)
    assert _conv_call(hip, pk.CONV3_S1, buf.data_ptr(), cin, cin, spec.wpk_f, y, cout, n, size) == 0
    torch.cuda.synchronize()
    y.fill_(3.0)
    assert _conv_call(hip, pk.CONV3_S1, buf.data_ptr(), cin, cin, spec.wpk_f, y, cout, n, size, stats=st.data_ptr(), nb_x=buf.data_ptr(),
                      nb_ldc=cout, nb_scale=sc.data_ptr(), nb_shift=sc.data_ptr()) == _lib_err("BADARG")
    assert _conv_call(hip, pk.CONV3_S1, buf.data_ptr(), 6, 6, spec.wpk_f, y, cout, n, size) == _lib_err("ALIGN")
    assert _conv_call(hip, pk.CONV3_S1, buf.data_ptr() + 4, cin, cin, spec.wpk_f, y, cout, n, size) == _lib_err("ALIGN")
    torch.cuda.synchronize()
    assert bool((y == 3.0).all()) and bool((st == 0).all())
    with pytest.raises(_lib.CwfError):
        hip.conv(pk.CONV3_S1, buf[:n * 4 * 4 * 16 * cin].view(n, *size, cin), spec.wpk_f, None, cout, out=y, prec="fp32", stats=st,
                 nb=(buf[:n * 4 * 4 * 16 * cin].view(n, *size, cin), sc, sc, 0.01))

    part = torch.full((1 << 16,), float("nan"), device=DEV)
    dy = torch.zeros(n, *size, cout, device=DEV)
    dys = torch.ones(n, cout, device=DEV)

    def wg(x_ptr, x_ldc, c, **kw):
        a = _lib.WgradArgs(op=pk.CONV3_S1, precision=_lib.PRECISION["fp32"], x=x_ptr, x_ldc=x_ldc, in_slope=1.0, dy=dy.data_ptr(),
                           dy_ldc=cout, partial=part.data_ptr(), N=n, Di=4, Hi=4, Wi=16, Cin=c, Do=4, Ho=4, Wo=16, Cout=cout, **kw)
        return hip.lib.cwf_wgrad(ctypes.addressof(a), None, hip._stream())
    assert wg(buf.data_ptr(), cin, cin) == 0
    torch.cuda.synchronize()
    part.fill_(float("nan"))
    assert wg(buf.data_ptr(), cin, cin, dy_scale=dys.data_ptr()) == _lib_err("BADARG")
    assert wg(buf.data_ptr(), 6, 6) == _lib_err("ALIGN")
    assert wg(buf.data_ptr() + 4, cin, cin) == _lib_err("ALIGN")
    torch.cuda.synchronize()
    assert bool(part.isnan().all())


def _lib_err(name):
    return {"BADARG": -1, "TOOLARGE": -2, "ALIGN": -3}[name]
