"""GPU: the wave-specialised split-bf16 forward of the 32-256-channel 3x3x3 layers (csrc/conv_wsp.hip) against the tap-table
kernel it replaces and against the operand-exact float64 reference (tests/bf16_operand_ref.py).

Its accumulation order per output element is the tap-table kernel's (chunk, tap pair, hi.hi / hi.lo / lo.hi into one fp32
accumulator from zero; then + bias, + residual), so its output must be bit-identical to the tap-table kernel's.  Its InstanceNorm
statistics are built from the tap-table kernel's own fp32 partial sums and differ only in the order of their float64 summation.  cwf_debug_wsp(0) sends a launch to the
tap-table kernel; cwf_debug_wsp(2) sends every eligible launch to the new kernel, whatever its size."""
import ctypes

import pytest
import torch

import bf16_operand_ref as R
from cwf import packing as pk
from test_conv_bf16_exact_gpu import _check, _field, _packed, _u, _weights

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PROBES = ["random", "positive"]

# (cin, cout, (D, H, W), n, wide output buffer, float64 reference, prologue): prologue "norm" = InstanceNorm scale / shift +
# LeakyReLU, "act" = LeakyReLU alone (no norm), "none" = the input as it is
SHAPES = {
    # the 3x3x3 layers of the bench step (tools/layer_table.py's census, batch 2) that the product routes here, and the 256-channel
    # input (16 chunks) the route also takes ...
    "model_128_128_16c": (128, 128, (16, 16, 16), 2, False, False, "norm"),
    "model_128_256_16c": (128, 256, (16, 16, 16), 2, False, False, "norm"),
    "model_256_128_16c": (256, 128, (16, 16, 16), 2, False, False, "norm"),
    # ... an activation without a norm (tools/layer_table.py times the 128-channel layers so) and no prologue at all ...
    "model_act_128_128_16c": (128, 128, (16, 16, 16), 2, False, False, "act"),
    "model_none_128_128_16c": (128, 128, (16, 16, 16), 2, False, False, "none"),
    # ... and the layers it leaves on the tap-table kernel (forced here): compared with the tap-table kernel only (their float64
    # reference is too slow for a test)
    "forced_32_64c": (32, 32, (64, 64, 64), 2, False, False, "norm"),
    "forced_64_32c": (64, 64, (32, 32, 32), 2, False, False, "norm"),
    # three tiles per workgroup (a partial round), sample boundaries inside workgroups' tile ranges
    "rounds_n3": (32, 32, (32, 32, 64), 3, False, True, "norm"),
    # ragged batch, odd multiples of 16 input channels, several output groups, wide output buffer, the other prologues
    "cin48_n1": (48, 32, (8, 8, 32), 1, True, True, "norm"),
    "cin96_n3": (96, 64, (8, 12, 16), 3, False, True, "norm"),
    "cin192_wide": (192, 96, (4, 8, 32), 2, True, True, "norm"),
    "act_cin64": (64, 32, (8, 8, 32), 2, False, True, "act"),
    "none_cin64": (64, 32, (8, 8, 32), 2, True, True, "none"),
}


def _launches(hip):
    f = hip.lib.cwf_debug_wsp_launches
    f.restype = ctypes.c_longlong
    return int(f())


def _run(hip, route, x, spec, b, cout, sc, sh, slope, res, n, out_shape, wide):
    old = hip.lib.cwf_debug_wsp(route)
    try:
        st = hip.new_stats(n, cout, DEV)
        kw = {}
        buf = None
        if wide:
            buf = torch.full(out_shape[:-1] + (cout + 8,), 7.0, device=DEV)
            kw["out"] = buf[..., 4:4 + cout]
        before = _launches(hip)
        y = hip.conv(pk.CONV3_S1, x, spec.wpk16_f, b, cout, sc, sh, slope, res, None, st, prec="bf16x3", **kw)
        torch.cuda.synchronize()
        ran = _launches(hip) - before
    finally:
        hip.lib.cwf_debug_wsp(old)
    # the launch took the route under test: the new kernel exactly once, or (route 0) not at all
    assert ran == (0 if route == 0 else 1), (route, ran)
    if wide:
        assert bool((buf[..., :4] == 7.0).all()) and bool((buf[..., 4 + cout:] == 7.0).all()), "wrote outside its channel slice"
    return y, st


@pytest.mark.parametrize("probe", PROBES)
@pytest.mark.parametrize("name", list(SHAPES))
def test_wsp_forward_equals_tap_table(hip, name, probe):
    cin, cout, size, n, wide, with_ref, pro = SHAPES[name]
    pos = probe == "positive"
    x = _field((n, *size, cin), probe, seed=21)
    w = _weights(pk.CONV3_S1, cin, cout, probe, seed=22)
    b = _u(cout, seed=23, lo_=0.0 if pos else -0.1, hi_=0.1)
    sc = sh = None
    slope = 1.0 if pro == "none" else 0.01
    if pro == "norm":
        sc, sh = _u(n, cin, seed=24, lo_=0.5, hi_=1.5), _u(n, cin, seed=25, lo_=0.0 if pos else -1.0)
    res = _field((n, *size, cout), "positive" if pos else "random", seed=26)
    spec = _packed(pk.CONV3_S1, cin, cout, w, "bf16x3")
    dv = lambda t: None if t is None else t.to(DEV)
    args = (dv(x), spec, dv(b), cout, dv(sc), dv(sh), slope, dv(res), n, (n, *size, cout), wide)
    # route 2 forces the new kernel even below its size threshold; the model shapes must reach it on the product route (1)
    y_new, st_new = _run(hip, 1 if name.startswith("model") else 2, *args)
    y_old, st_old = _run(hip, 0, *args)
    assert torch.equal(y_new, y_old), (name, probe, float((y_new - y_old).abs().max()))
    # statistics: the tap-table kernel's own fp32 partials, summed in float64 in another order
    yd = y_old.double()
    scale = torch.stack([yd.abs().sum((1, 2, 3)), (yd * yd).sum((1, 2, 3))], -1)
    assert bool(((st_new - st_old).abs() <= 1e-12 * scale + 1e-30).all()), (name, probe, float(((st_new - st_old).abs() / scale).max()))
    if with_ref:
        ref = R.conv_ref(pk.CONV3_S1, x, w, "bf16x3", bias=b, in_scale=sc, in_shift=sh, slope=slope, residual=res)
        for tag, y, st in (("wsp", y_new, st_new), ("tap-table", y_old, st_old)):
            _check(y, ref, R.GAMMA_CONV, "%s %s" % (tag, name), "bf16x3", probe, "forward")
            R.assert_stats(st, ref, R.GAMMA_CONV, "%s %s" % (tag, name))


def test_wsp_debug_knob(hip):
    """the knob returns the previous value (1, the product route, by default)"""
    assert hip.lib.cwf_debug_wsp(2) == 1
    assert hip.lib.cwf_debug_wsp(1) == 2
