"""GPU: every bf16 conv path against the operand-exact float64 reference (tests/bf16_operand_ref.py): |got - ref| <= gamma * A
elementwise, with A the same reference on |operands|.  Probes per path and mode:
  random    zero-mean operands with every prologue / epilogue feature the path takes, ragged extents, batch >= 2
  positive  all-positive operands (no cancellation: dropped or duplicated work shows at full size)
  impulse   input (or dy) zero except isolated bf16 values: every output is ONE product -- bit-exact in single-bf16 mode, within
            one fp32 ulp in split mode; zeros outside the support
  constant  x = 0, scale 1, shift != 0: the activated shift reaches only in-bounds taps (padding after activation)
and untouched memory (channels outside an out= slice, other groups) where the path writes into a wider buffer."""
import ctypes
import math

import pytest
import torch

import bf16_operand_ref as R
import wgrad_bf16_cases as WG
from cwf import _lib, packing as pk

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MODES = ["bf16", "bf16x3"]
PROBES = ["random", "positive", "impulse"]
ALL_CFGS = {(4, 4, 1), (2, 4, 2), (2, 4, 4), (4, 2, 4), (4, 1, 4), (1, 4, 4), (1, 2, 4), (1, 2, 2), (1, 1, 4)}


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
    return _u(*shape, seed=seed, lo_=0.5 * s if probe == "positive" else -s, hi_=s)


def _field(shape, probe, seed):
    """an operand tensor [N, D, H, W, C] for the probe (impulse: see _impulses)"""
    if probe == "positive":
        return _u(*shape, seed=seed, lo_=0.5, hi_=1.0)
    if probe == "impulse":
        return _impulses(shape, seed)
    return _u(*shape, seed=seed)


def _impulses(shape, seed, per_channel=False):
    """zero except isolated bf16-representable values, pairwise >= 3 voxels apart: the 8 corners, face centres, voxels inside the last
    (ragged) 4 x 4 x 16 tile of each dimension, in the last sample, in channel 0 and the last channel (per_channel: one impulse per
    channel, for weight gradients)"""
    n, d, h, w, c = shape
    cand = []
    for nn in sorted({0, n - 1}, reverse=True):
        cand += [(nn, a, b, e) for a in (0, d - 1) for b in (0, h - 1) for e in (0, w - 1)]
        cand += [(nn, d // 2, h // 2, 0), (nn, d // 2, h // 2, w - 1), (nn, 0, h // 2, w // 2), (nn, d - 1, h // 2, w // 2),
                 (nn, d // 2, 0, w // 2), (nn, d // 2, h - 1, w // 2)]
        cand += [(nn, ((d - 1) // 4) * 4, h // 2, w // 2), (nn, d // 2, ((h - 1) // 4) * 4, w // 2), (nn, d // 2, h // 2, ((w - 1) // 16) * 16),
                 (nn, d - 2, h - 2, w - 2)]
    keep = []
    for p in cand:
        if all(p[0] != q[0] or max(abs(p[1] - q[1]), abs(p[2] - q[2]), abs(p[3] - q[3])) >= 3 for q in keep):
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


def _packed(op, cin, cout, w, mode):
    from cwf import functional as CF, kernels
    spec = CF.ConvSpec(op, cin, cout)
    packer = CF.WeightPacker()
    packer.add(spec, torch.nn.Parameter(w.to(DEV).contiguous()))
    kernels.set_precision(mode)
    try:
        packer.refresh()
    finally:
        kernels.set_precision("fp32")
    spec._keepalive = packer
    return spec


def _record(path, mode, worst):
    """one line per checked result (visible with -s): the worst err / A, already within gamma"""
    print("\nworst err/A  %-28s %-7s %.3e  (%.2f x 2^-18)" % (path, mode, worst, worst / 2.0 ** -18))


def _check(got, ref, gamma, path, mode, probe, what):
    if probe == "impulse":
        g = ref.pick(got)
        if mode == "bf16":
            assert torch.equal(g, ref.y), (path, what, float((g - ref.y).abs().max()))
        else:
            ulp = (torch.nextafter(ref.y.float().abs(), torch.tensor(math.inf)) - ref.y.float().abs()).double()
            assert bool(((g - ref.y).abs() <= ulp).all()), (path, what, float((g - ref.y).abs().max()))
        return
    _record(path, mode, R.check(got, ref, gamma, "%s %s %s %s" % (path, mode, probe, what)))


# ====================================================================================================== forward
# path: (op, cin, cout, size, n, features).  features: p = InstanceNorm + LeakyReLU prologue, b = bias, r = residual, o = out_scale,
# s = statistics, w = raw weights (w_ref: stem / s2c16), S = into a channel slice of a wider buffer
FWD = {
    "stem": (pk.CONV3_S1, 4, 16, (32, 34, 37), 2, "bosw"),
    "s2c16": (pk.CONV3_S2, 16, 32, (66, 64, 70), 2, "bsw"),
    "conv16s": (pk.CONV3_S1, 16, 16, (32, 33, 34), 2, "pbros"),
    "conv16s_cin8": (pk.CONV3_S1, 8, 16, (34, 30, 38), 2, "pbs"),
    "taptable_s1_114": (pk.CONV3_S1, 48, 16, (9, 10, 20), 2, "pbrosS"),
    "taptable_s1_424": (pk.CONV3_S1, 16, 128, (16, 32, 17), 2, "pbrsS"),
    "taptable_s1_441": (pk.CONV3_S1, 16, 256, (16, 32, 17), 2, "pbsS"),
    "taptable_s2": (pk.CONV3_S2, 32, 64, (10, 12, 35), 2, "pbosS"),
    "taptable_convT_144": (pk.CONVT2, 16, 256, (2, 9, 2), 3, "bsS"),
    "taptable_conv1": (pk.CONV1, 256, 128, (4, 5, 9), 2, "pboS"),
    "pointwise": (pk.CONV1, 32, 16, (8, 8, 32), 2, "brsS"),
    "pointwise_convT": (pk.CONVT2, 16, 16, (4, 6, 16), 2, "bsS"),
    "weight_stationary": (pk.CONV3_S1, 64, 32, (8, 8, 32), 2, "pbrsS"),
}


def _ws_debug(hip, on):
    if on:
        return hip.lib.cwf_debug_ws_min_units(1), hip.lib.cwf_debug_ws_x3(1)
    return None


@pytest.mark.parametrize("probe", PROBES + ["constant"])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("path", list(FWD))
def test_forward_is_operand_exact(hip, path, mode, probe):
    op, cin, cout, size, n, feat = FWD[path]
    if probe == "constant" and "p" not in feat:
        pytest.skip("no prologue on this path")
    x = _field((n, *size, cin), probe, seed=1)
    w = _weights(op, cin, cout, probe, seed=2)
    imp = probe == "impulse"
    pos = probe == "positive"
    b = None if imp or "b" not in feat else _u(cout, seed=3, lo_=0.0 if pos else -0.1, hi_=0.1)
    sc = sh = None
    slope = 1.0
    if "p" in feat and not imp:
        sc, sh, slope = _u(n, cin, seed=4, lo_=0.5, hi_=1.5), _u(n, cin, seed=5, lo_=0.0 if pos else -1.0), 0.01
    if probe == "constant":
        x = torch.zeros_like(x)
        sc = torch.ones(n, cin)
        sh = torch.full((n, cin), -0.75) if path.endswith(("114", "conv16s")) else torch.linspace(0.25, 1.5, cin).repeat(n, 1)
    do, ho, wo = pk.out_dims(op, *size)
    res = _field((n, do, ho, wo, cout), "positive" if pos else "random", seed=6) if ("r" in feat and not imp) else None
    osc = None
    if "o" in feat and not imp:
        osc = _u(n, cout, seed=7, lo_=0.5, hi_=1.5) if pos else (_u(n, cout, seed=7) > -0.5).float() * 1.25
    spec = _packed(op, cin, cout, w, mode)
    st = hip.new_stats(n, cout, DEV) if "s" in feat else None
    old = _ws_debug(hip, path == "weight_stationary")
    try:
        kw = dict(w_ref=w.to(DEV).contiguous()) if "w" in feat else {}
        if "S" in feat:
            wide = torch.full((n, do, ho, wo, cout + 8), 7.0, device=DEV)
            kw["out"] = wide[..., 4:4 + cout]
        dv = lambda t: None if t is None else t.to(DEV)
        y = hip.conv(op, x.to(DEV), spec.wpk16_f, dv(b), cout, dv(sc), dv(sh), slope, dv(res), dv(osc), st, prec=mode, **kw)
        torch.cuda.synchronize()
    finally:
        if old:
            hip.lib.cwf_debug_ws_min_units(old[0]); hip.lib.cwf_debug_ws_x3(old[1])
    ref = R.conv_ref(op, x, w, mode, bias=b, in_scale=sc, in_shift=sh, slope=slope, residual=res, out_scale=osc)
    _check(y, ref, R.GAMMA_CONV, path, mode, probe, "forward")
    if st is not None and not imp:
        R.assert_stats(st, ref, R.GAMMA_CONV, path)
    if "S" in feat:
        assert bool((wide[..., :4] == 7.0).all()) and bool((wide[..., 4 + cout:] == 7.0).all()), "wrote outside its channel slice"


def test_pointwise_bf16_side_output_is_the_rounded_output(hip):
    """conv(..., y16=): the pointwise kernel's bf16 image is bf16_rne of its own fp32 output, which is operand-exact"""
    n, size, cin, cout = 2, (8, 8, 32), 32, 16
    x, w, b = _u(n, *size, cin, seed=11), _weights(pk.CONV1, cin, cout, "random", 12), _u(cout, seed=13, lo_=-0.1, hi_=0.1)
    for mode in MODES:
        spec = _packed(pk.CONV1, cin, cout, w, mode)
        y16 = torch.empty((n, *size, cout), dtype=torch.bfloat16, device=DEV)
        y = hip.conv(pk.CONV1, x.to(DEV), spec.wpk16_f, b.to(DEV), cout, prec=mode, y16=y16)
        _record("pointwise y16", mode, R.check(y, R.conv_ref(pk.CONV1, x, w, mode, bias=b), R.GAMMA_CONV, "pointwise y16"))
        assert torch.equal(y16, y.to(torch.bfloat16))


@pytest.mark.parametrize("probe", PROBES)
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("cin,cout,size,n,G", [(128, 32, (8, 8, 16), 2, 3), (8, 2, (8, 12, 16), 2, 3), (16, 16, (6, 8, 20), 2, 2)])
def test_grouped_conv_is_operand_exact(hip, cin, cout, size, n, G, mode, probe):
    """cwf_conv with groups: forward and data gradient; padding channels and other groups' channels stay as written"""
    ca = (cout + 3) // 4 * 4
    x_all = _field((n, *size, G * cin), probe, seed=21)
    ws = [_weights(pk.CONV3_S1, cin, cout, probe, seed=22 + q) for q in range(G)]
    bs = [None if probe == "impulse" else _u(cout, seed=32 + q, lo_=0.0 if probe == "positive" else -0.1, hi_=0.1) for q in range(G)]
    specs = [_packed(pk.CONV3_S1, cin, cout, w, mode) for w in ws]
    y_all = torch.full((n, *size, G * ca + 4), 5.0, device=DEV)
    hip.conv_grouped(x_all.to(DEV), cin, [s.wpk16_f for s in specs], [None if b is None else b.to(DEV) for b in bs], cout, y_all[..., :G * ca],
                     x_goff=cin, y_goff=ca, prec=mode)
    for q in range(G):
        ref = R.conv_ref(pk.CONV3_S1, x_all[..., q * cin:(q + 1) * cin], ws[q], mode, bias=bs[q])
        _check(y_all[..., q * ca:q * ca + cout], ref, R.GAMMA_CONV, "grouped fwd", mode, probe, "group %d" % q)
        assert bool((y_all[..., q * ca + cout:(q + 1) * ca] == 5.0).all())
    assert bool((y_all[..., G * ca:] == 5.0).all())
    dy_all = torch.zeros(n, *size, G * ca)
    for q in range(G):
        dy_all[..., q * ca:q * ca + cout] = _field((n, *size, cout), probe, seed=41 + q)
    dx_all = torch.full((n, *size, G * cin + 4), 5.0, device=DEV)
    hip.conv_grouped(dy_all.to(DEV), ca, [s.wpk16_d for s in specs], None, cin, dx_all[..., :G * cin], x_goff=ca, y_goff=cin, fwd_op=pk.CONV3_S1, prec=mode)
    for q in range(G):
        ref = R.conv_ref(pk.CONV3_S1, dy_all[..., q * ca:q * ca + cout], ws[q], mode, dgrad=True, out_size=size)
        _check(dx_all[..., q * cin:(q + 1) * cin], ref, R.GAMMA_CONV, "grouped dgrad", mode, probe, "group %d" % q)
    assert bool((dx_all[..., G * cin:] == 5.0).all())


# ====================================================================================================== data gradient
# path: (forward op, cin, cout, forward input size, n, features): r = residual (carried gradient), N = norm-backward sums,
# x = also from the bf16 image of dy (x16=, single-bf16 only)
DGRAD = {
    "conv16s": (pk.CONV3_S1, 16, 16, (32, 33, 34), 2, "rNx"),
    "weight_stationary": (pk.CONV3_S1, 64, 32, (8, 8, 32), 2, "rN"),
    "taptable_s1": (pk.CONV3_S1, 32, 16, (9, 10, 20), 2, "rN"),
    "taptable_s2": (pk.CONV3_S2, 16, 32, (16, 16, 33), 2, "rN"),
    "taptable_convT": (pk.CONVT2, 32, 32, (4, 5, 9), 2, "r"),
    "pointwise": (pk.CONV1, 32, 16, (8, 8, 32), 2, "rN"),
}


@pytest.mark.parametrize("probe", PROBES)
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("path", list(DGRAD))
def test_data_gradient_is_operand_exact(hip, path, mode, probe):
    op, cin, cout, size, n, feat = DGRAD[path]
    w = _weights(op, cin, cout, probe, seed=51)
    do, ho, wo = pk.out_dims(op, *size)
    dy = _field((n, do, ho, wo, cout), probe, seed=52)
    imp = probe == "impulse"
    res = _field((n, *size, cin), "positive" if probe == "positive" else "random", seed=53) if ("r" in feat and not imp) else None
    nbx, nsc, nsh = _u(n, *size, cin, seed=54), _u(n, cin, seed=55, lo_=0.5, hi_=1.5), _u(n, cin, seed=56)
    spec = _packed(op, cin, cout, w, mode)
    dv = lambda t: None if t is None else t.to(DEV)
    ref = R.conv_ref(op, dy, w, mode, residual=res, dgrad=True, out_size=size)
    old = _ws_debug(hip, path == "weight_stationary")
    try:
        sums = hip.new_stats(n, cin, DEV) if "N" in feat else None
        nb = (nbx.to(DEV), nsc.to(DEV), nsh.to(DEV), 0.01) if "N" in feat else None
        dx = hip.conv(pk.dgrad_op(op), dy.to(DEV), spec.wpk16_d, None, cin, residual=dv(res), out=torch.empty((n, *size, cin), device=DEV),
                      prec=mode, stats=sums, nb=nb)
        _check(dx, ref, R.GAMMA_CONV, "dgrad " + path, mode, probe, "dx")
        if nb is not None and not imp:
            R.assert_nb_sums(sums, ref, (nbx, nsc, nsh, 0.01), R.GAMMA_CONV, path)
        if "x" in feat and mode == "bf16":
            sums16 = hip.new_stats(n, cin, DEV)
            dy16 = dy.to(DEV).to(torch.bfloat16)
            dx16 = hip.conv(pk.CONV3_S1, dy.to(DEV), spec.wpk16_d, None, cin, residual=dv(res), out=torch.empty((n, *size, cin), device=DEV),
                            prec="bf16", fwd_op=pk.CONV3_S1, stats=sums16, nb=nb, x16=dy16)
            _check(dx16, ref, R.GAMMA_CONV, "dgrad conv16s x16", mode, probe, "dx (x16)")
            if not imp:
                R.assert_nb_sums(sums16, ref, (nbx, nsc, nsh, 0.01), R.GAMMA_CONV, path + " x16")
        torch.cuda.synchronize()
    finally:
        if old:
            hip.lib.cwf_debug_ws_min_units(old[0]); hip.lib.cwf_debug_ws_x3(old[1])


# ====================================================================================================== tile configurations
def _cfg(hip, op, n, in_dims, out_dims, cout):
    a = (ctypes.c_int * 3)()
    assert hip.lib.cwf_debug_conv_bf16_cfg(op, n, *in_dims, *out_dims, cout, a) == 0
    return tuple(a)


def _s2_dgrad_cfg(hip, n, size, cin):
    """the configuration of the stride-2 data gradient onto a forward input of extent size (cin channels)"""
    return _cfg(hip, pk.CONV3_S2_DGRAD, n, pk.out_dims(pk.CONV3_S2, *size), size, cin)


# stride-2 data gradients (eight parity classes; no other route takes them) that reach each configuration choose_cfg can return:
# (expected cfg, forward cin, forward cout, forward input size, n)
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
    # the forward tap-table shapes of FWD: the configuration each runs
    assert _cfg(hip, pk.CONV3_S1, 2, (16, 32, 17), (16, 32, 17), 128) == (4, 2, 4)
    assert _cfg(hip, pk.CONV3_S1, 2, (9, 10, 20), (9, 10, 20), 16) == (1, 1, 4)
    assert _cfg(hip, pk.CONV3_S1, 2, (16, 32, 17), (16, 32, 17), 256) == (4, 4, 1)
    assert _cfg(hip, pk.CONVT2, 3, (2, 9, 2), (4, 18, 4), 256) == (1, 4, 4)
    assert _cfg(hip, pk.CONV3_S2, 2, (10, 12, 35), pk.out_dims(pk.CONV3_S2, 10, 12, 35), 64) == (1, 1, 4)
    # the stride-2 rule: no configuration with MT * WM > 4 for the stride-2 forward / ConvTranspose data gradient
    for op in (pk.CONV3_S2, pk.CONVT2_DGRAD):
        for dims in ((8, 8, 16), (16, 16, 32), (32, 32, 64)):
            for c in (16, 64, 256):
                m, _, wm = _cfg(hip, op, 2, tuple(2 * v for v in dims), dims, c)
                assert m * wm <= 4


@pytest.mark.parametrize("probe", PROBES)
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("cfg,cin,cout,size,n", CFG_CASES, ids=["%d%d%d" % c[0] for c in CFG_CASES])
def test_every_tile_configuration_is_operand_exact(hip, cfg, cin, cout, size, n, mode, probe):
    """the tap-table kernel at each configuration, as the stride-2 data gradient with a residual and the norm-backward sums"""
    op = pk.CONV3_S2
    assert _s2_dgrad_cfg(hip, n, size, cin) == cfg
    w = _weights(op, cin, cout, probe, seed=61)
    do, ho, wo = pk.out_dims(op, *size)
    dy = _field((n, do, ho, wo, cout), probe, seed=62)
    res = None if probe == "impulse" else _field((n, *size, cin), "positive" if probe == "positive" else "random", seed=63)
    spec = _packed(op, cin, cout, w, mode)
    nbx, nsc, nsh = _u(n, *size, cin, seed=64), _u(n, cin, seed=65, lo_=0.5, hi_=1.5), _u(n, cin, seed=66)
    sums = hip.new_stats(n, cin, DEV)
    dx = hip.conv(pk.CONV3_S2_DGRAD, dy.to(DEV), spec.wpk16_d, None, cin, residual=None if res is None else res.to(DEV),
                  out=torch.empty((n, *size, cin), device=DEV), prec=mode, stats=sums, nb=(nbx.to(DEV), nsc.to(DEV), nsh.to(DEV), 0.01))
    ref = R.conv_ref(op, dy, w, mode, residual=res, dgrad=True, out_size=size)
    _check(dx, ref, R.GAMMA_CONV, "taptable %d%d%d" % cfg, mode, probe, "dx")
    if probe != "impulse":
        R.assert_nb_sums(sums, ref, (nbx, nsc, nsh, 0.01), R.GAMMA_CONV, "cfg %s" % (cfg,))


# ====================================================================================================== weight gradient
# path: (op, cin, cout, size, n, route): "tiled" = hip.wgrad (cwf_wgrad, pw_wgrad_kernel for 1x1x1 / transposed),
# "images" = wgrad_to in the bench's precision setting (bf16 operand images: wgrad16 / wgrad_s1), "dys" = the dy_scale fold
WGRAD = {
    "tiled_s1": (pk.CONV3_S1, 48, 16, (9, 10, 20), 2, "tiled"),
    "tiled_s1_cin4": (pk.CONV3_S1, 4, 16, (8, 12, 33), 2, "tiled"),
    "tiled_s2": (pk.CONV3_S2, 16, 32, (16, 16, 33), 2, "tiled"),
    "pw_conv1": (pk.CONV1, 32, 16, (8, 8, 32), 2, "tiled"),
    "pw_convT": (pk.CONVT2, 16, 16, (4, 6, 8), 2, "tiled"),
    "wgrad16_images": (pk.CONV3_S1, 16, 16, (32, 33, 34), 2, "images"),
    "wgrad_s1_images": (pk.CONV3_S1, 32, 32, (8, 12, 20), 2, "images"),
    "dys": (pk.CONV3_S1, 4, 16, (32, 33, 34), 2, "dys"),
}


@pytest.mark.parametrize("probe", PROBES + ["constant"])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("path", list(WGRAD))
def test_weight_gradient_is_operand_exact(hip, path, mode, probe):
    from cwf import functional as CF, kernels
    op, cin, cout, size, n, route = WGRAD[path]
    if route == "images" and mode != "bf16":
        pytest.skip("the bf16-image kernels are single-bf16 only")
    imp = probe == "impulse"
    do, ho, wo = pk.out_dims(op, *size)
    x = _bf(_u(n, *size, cin, seed=71)) if imp else _field((n, *size, cin), probe, seed=71)
    dy = _impulses((n, do, ho, wo, cout), 0, per_channel=True) if imp else _field((n, do, ho, wo, cout), probe, seed=72)
    sc, sh, slope = None, None, 1.0
    if not imp:
        sc, sh, slope = _u(n, cin, seed=73, lo_=0.5, hi_=1.5), _u(n, cin, seed=74, lo_=0.0 if probe == "positive" else -1.0), 0.01
    if probe == "constant":
        x = torch.zeros_like(x)
        sc, sh = torch.ones(n, cin), torch.linspace(-1.0, 1.0, cin).repeat(n, 1)
    s = None
    if route == "dys":
        s = torch.tensor([1.25, 0.0, -0.7, 3.0, 1.25, 0.5, 0.0, 1.25, -2.0, 1.25, 0.0, 0.25, 1.25, 1.5, 1.25, -0.3])
        s = torch.stack([s.roll(3 * i) for i in range(n)]).contiguous()
        if probe == "positive" or imp:
            s = s.abs() + 0.25 * (s == 0)
        if imp:
            s = _bf(s)                                             # dy * s then has <= 16 significant bits: hi + lo is exact
    # the operand form of the kernel that runs, from the library's own plan (pw_wgrad_kernel: exact fp32 products in both modes)
    ex = WG.operand_form(_lib, hip.lib, op, cin, cout, size, n, mode, {"tiled": "contig", "images": "images", "dys": "dys"}[route])
    assert ex == R.wgrad_operand_mode(op, cin, cout, size, mode)
    dw_ref, db_ref, aw, ab = R.wgrad_ref(op, x, dy, ex, sc, sh, slope, dy_scale=s)
    dv = lambda t: None if t is None else t.to(DEV)
    wn = math.prod(_wshape(op, cin, cout))
    spec = CF.ConvSpec(op, cin, cout).to(torch.device(DEV))
    if route == "tiled":
        gw, gb = hip.wgrad(op, x.to(DEV), dv(sc), dv(sh), slope, dy.to(DEV), cout, spec.inv_map, spec.has_bias_map, wn, prec=mode)
    else:
        kernels.set_precision("bf16x3", wgrad=mode, dgrad="bf16")
        try:
            nv = do * ho * wo
            if route == "images":
                assert hip.bf16_operands_ok(op, cin, cout, nv) == (16 if cin == 16 else 32)
            else:
                assert hip.dy_scale_ok(op, cin, cout, nv)
            gw, gb = torch.zeros(wn, device=DEV), torch.zeros(cout, device=DEV)
            hip.wgrad_to(("exact", path), op, x.to(DEV), dv(sc), dv(sh), slope, dy.to(DEV), cout, spec.inv_map, gw, gb, dy_scale=dv(s))
            hip.wgrad_flush(torch.device(DEV))
        finally:
            kernels.set_precision("fp32")
    torch.cuda.synchronize()
    gw = gw.view(dw_ref.shape)
    if imp:
        assert torch.equal(gw.cpu().double(), dw_ref), (path, float((gw.cpu().double() - dw_ref).abs().max()))
        assert gb is None or torch.equal(gb.cpu().double(), db_ref)
        return
    _record("wgrad " + path, mode, R.assert_operand_exact(gw, dw_ref, aw, R.GAMMA_WGRAD, "%s %s %s dW" % (path, mode, probe)))
    if gb is not None:
        _record("bgrad " + path, mode, R.assert_operand_exact(gb, db_ref, ab, R.GAMMA_WGRAD, "%s %s %s db" % (path, mode, probe)))


@pytest.mark.parametrize("probe", PROBES)
@pytest.mark.parametrize("mode", MODES)
def test_grouped_weight_gradient_is_operand_exact(hip, mode, probe):
    G, cin, cout, size, n = 3, 32, 8, (8, 12, 16), 2
    ca = 8
    imp = probe == "impulse"
    x_all = _bf(_u(n, *size, G * cin, seed=81)) if imp else _field((n, *size, G * cin), probe, seed=81)
    dy_all = torch.zeros(n, *size, G * ca)
    for q in range(G):
        dy_all[..., q * ca:q * ca + cout] = _impulses((n, *size, cout), 0, per_channel=True) if imp else _field((n, *size, cout), probe, seed=82 + q)
    specs = [_packed(pk.CONV3_S1, cin, cout, _weights(pk.CONV3_S1, cin, cout, "random", 90 + q), mode) for q in range(G)]
    xd, dd = x_all.to(DEV), dy_all.to(DEV)
    xs = [xd[..., q * cin:(q + 1) * cin] for q in range(G)]
    dys = [dd[..., q * ca:q * ca + cout] for q in range(G)]
    dws = [torch.full((cout, cin, 3, 3, 3), 3.0, device=DEV) for _ in range(G)]
    dbs = [torch.full((cout,), 3.0, device=DEV) for _ in range(G)]
    hip.wgrad_to_grouped(specs, pk.CONV3_S1, xs, dys, cout, [s_.inv_map for s_ in specs], dws, dbs, prec=mode)
    hip.wgrad_flush(torch.device(DEV))
    torch.cuda.synchronize()
    for q in range(G):
        dw_ref, db_ref, aw, ab = R.wgrad_ref(pk.CONV3_S1, x_all[..., q * cin:(q + 1) * cin], dy_all[..., q * ca:q * ca + cout], mode)
        if imp:
            assert torch.equal(dws[q].cpu().double(), dw_ref) and torch.equal(dbs[q].cpu().double(), db_ref)
            continue
        _record("wgrad grouped", mode, R.assert_operand_exact(dws[q], dw_ref, aw, R.GAMMA_WGRAD, "grouped dW %d" % q))
        _record("bgrad grouped", mode, R.assert_operand_exact(dbs[q], db_ref, ab, R.GAMMA_WGRAD, "grouped db %d" % q))


def test_fp32_statistics_of_the_widest_tile(hip):
    """the fp32 kernel (conv_mfma_kernel) shares the statistics reduction of the tap-table kernel: at {4, 4, 1} (four wave columns x four
    16-channel tiles = 512 (channel, sum) pairs for 256 threads) every channel's sums must arrive"""
    n, size, cin, cout = 2, (16, 32, 17), 16, 256
    x, w = _u(n, *size, cin, seed=91), _weights(pk.CONV3_S1, cin, cout, "random", 92)
    from cwf import functional as CF
    spec = CF.ConvSpec(pk.CONV3_S1, cin, cout)
    packer = CF.WeightPacker()
    packer.add(spec, torch.nn.Parameter(w.to(DEV).contiguous()))
    packer.refresh()
    st = hip.new_stats(n, cout, DEV)
    y = hip.conv(pk.CONV3_S1, x.to(DEV), spec.wpk_f, None, cout, stats=st, prec="fp32")
    yd = y.cpu().double()
    bound = R.REL_SUMS * torch.stack([yd.abs().sum((1, 2, 3)), (yd * yd).sum((1, 2, 3))], -1)
    assert bool(((st.cpu() - R.stats_ref(yd)).abs() <= bound).all())
