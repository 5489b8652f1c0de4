"""GPU: the wave-specialised weight-in-LDS single-bf16 kernel of the small deep 3x3x3 layers' data gradients (csrc/conv_wsd.hip)
against the tap-table kernel it replaces and against the operand-exact float64 reference (tests/bf16_operand_ref.py).

Its accumulation order per output element is the tap-table kernel's (chunk, tap pair, one fp32 accumulator from zero; then
+ residual), so its output must be bit-identical to the tap-table kernel's.  Its norm-backward sums are built from the tap-table
kernel's own fp32 partial sums and differ only in the order of their float64 summation.  cwf_debug_wsd(0) sends a launch to the
tap-table kernel (or conv_ws.hip, where that takes it), cwf_debug_wsd(2) sends every eligible launch to the new kernel, whatever its
size, and cwf_debug_wsd(3) does so with 32 output channels per workgroup."""
import ctypes
import functools

import pytest
import torch

import bf16_operand_ref as R
from cwf import packing as pk
from test_conv_bf16_exact_gpu import _check, _field, _packed, _u, _weights

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PROBES = ["random", "positive", "impulse"]
OP = pk.CONV3_S1

# (launch Cin, launch Cout, (D, H, W), N): the launch reads dy with Cin channels and writes dx with Cout channels (the forward layer
# is Cout -> Cin)
SHAPES = {
    "one_tile": (32, 32, (4, 4, 16), 1),           # every face a boundary, two chunks
    "faces": (48, 64, (8, 8, 32), 2),              # interior faces in all directions, odd chunk count, several groups, sample boundary
    "cin128": (128, 128, (4, 8, 16), 1),           # eight chunks
    "cin256": (256, 128, (4, 4, 32), 1),           # sixteen chunks
    "ragged_n3": (96, 96, (8, 12, 16), 3),         # ragged batch
}
# epilogue forms: (residual, norm-backward slope or None)
FORMS = {"plain": (False, None), "res": (True, None), "nb": (False, 0.01), "nb0": (False, 0.0), "res_nb": (True, 0.01)}
# (shape, form, knob): every form on three shapes, the step's form and the plain one on the deep shapes; knob 3 (two output tiles per
# workgroup) on every shape
CASES = [(s, f, 2) for s in ("one_tile", "faces", "ragged_n3") for f in FORMS]
CASES += [(s, f, 2) for s in ("cin128", "cin256") for f in ("plain", "res_nb")]
CASES += [(s, f, 3) for s in SHAPES for f in ("plain", "res_nb")] + [("faces", "nb0", 3), ("ragged_n3", "res", 3)]


def _launches(hip):
    return int(hip.lib.cwf_debug_wsd_launches())


@functools.lru_cache(maxsize=None)
def _operands(name, probe):
    cin, cout, size, n = SHAPES[name]
    dy = _field((n, *size, cin), probe, seed=31)
    w = _weights(OP, cout, cin, probe, seed=32)            # the forward layer's parameter: [cin, cout, 3, 3, 3]
    res = _field((n, *size, cout), "positive" if probe == "positive" else "random", seed=33)
    nbx, nsc, nsh = _u(n, *size, cout, seed=34), _u(n, cout, seed=35, lo_=0.5, hi_=1.5), _u(n, cout, seed=36)
    spec = _packed(OP, cout, cin, w, "bf16")
    return dy, w, res, (nbx, nsc, nsh), spec, dy.to(DEV), res.to(DEV), tuple(t.to(DEV) for t in (nbx, nsc, nsh))


@functools.lru_cache(maxsize=None)
def _ref(name, probe, with_res):
    dy, w, res = _operands(name, probe)[:3]
    return R.conv_ref(OP, dy, w, "bf16", residual=res if with_res else None, dgrad=True, out_size=SHAPES[name][2])


def _run(hip, knob, x, spec, cout, res, nb, n, size, wide=False, expect=None):
    """one single-bf16 data-gradient launch under cwf_debug_wsd(knob); returns (dx, sums)"""
    old = hip.lib.cwf_debug_wsd(knob)
    try:
        sums = hip.new_stats(n, cout, DEV) if nb is not None else None
        buf = torch.full((n, *size, cout + 8), 7.0, device=DEV) if wide else None
        out = buf[..., 4:4 + cout] if wide else torch.empty((n, *size, cout), device=DEV)
        before = _launches(hip)
        dx = hip.conv(OP, x, spec.wpk16_d, None, cout, residual=res, out=out, prec="bf16", fwd_op=OP, stats=sums, nb=nb)
        torch.cuda.synchronize()
        ran = _launches(hip) - before
    finally:
        hip.lib.cwf_debug_wsd(old)
    assert ran == ((0 if knob == 0 else 1) if expect is None else expect), (knob, ran)
    if wide:
        assert bool((buf[..., :4] == 7.0).all()) and bool((buf[..., 4 + cout:] == 7.0).all()), "wrote outside its channel slice"
    return dx, sums


def _sums_equal(new, old, y_old, nb, what):
    """the sums of two routes: the same fp32 partials, summed in float64 in another order"""
    nbx, nsc, nsh, slope = nb
    h = torch.addcmul(nsh[:, None, None, None, :], nbx, nsc[:, None, None, None, :]).double()
    gn = y_old.double() * torch.where(h > 0, 1.0, float(slope))
    scale = torch.stack([gn.abs().sum((1, 2, 3)), (gn * h).abs().sum((1, 2, 3))], -1)
    assert bool(((new - old).abs() <= 1e-12 * scale + 1e-30).all()), (what, float(((new - old).abs() / (scale + 1e-30)).max()))


@pytest.mark.parametrize("probe", PROBES)
@pytest.mark.parametrize("name,form,knob", CASES, ids=["%s-%s-k%d" % c for c in CASES])
def test_wsd_equals_tap_table_and_reference(hip, name, form, knob, probe):
    cin, cout, size, n = SHAPES[name]
    with_res, slope = FORMS[form]
    imp = probe == "impulse"
    dy, w, res, nbh, spec, dy_d, res_d, nb_d = _operands(name, probe)
    with_res = with_res and not imp
    nb = None if slope is None else nb_d + (slope,)
    args = (dy_d, spec, cout, res_d if with_res else None, nb, n, size)
    y_new, s_new = _run(hip, knob, *args)
    y_old, s_old = _run(hip, 0, *args)
    assert torch.equal(y_new, y_old), (name, form, probe, float((y_new - y_old).abs().max()))
    if nb is not None:
        _sums_equal(s_new, s_old, y_old, nb, (name, form, probe))
    ref = _ref(name, probe, with_res)
    _check(y_new, ref, R.GAMMA_CONV, "wsd %s %s" % (name, form), "bf16", probe, "dx")
    if nb is not None and not imp:
        R.assert_nb_sums(s_new, ref, nbh + (slope,), R.GAMMA_CONV, "wsd %s %s" % (name, form))


@pytest.mark.parametrize("knob", [2, 3])
@pytest.mark.parametrize("name", ["faces", "ragged_n3"])
def test_wsd_wide_output_and_channel_slice_input(hip, name, knob):
    """y_ldc > Cout (sentinel-filled buffer: nothing outside the channel slice is written) and x_ldc > Cin (the input is a channel
    slice of a wider tensor)"""
    cin, cout, size, n = SHAPES[name]
    dy, w, res, nbh, spec, dy_d, res_d, nb_d = _operands(name, "random")
    wide_x = torch.full((n, *size, cin + 8), 1e30, device=DEV)
    wide_x[..., 4:4 + cin] = dy_d
    nb = nb_d + (0.01,)
    y_new, s_new = _run(hip, knob, wide_x[..., 4:4 + cin], spec, cout, res_d, nb, n, size, wide=True)
    y_old, s_old = _run(hip, 0, dy_d, spec, cout, res_d, nb, n, size)
    assert torch.equal(y_new, y_old)
    _sums_equal(s_new, s_old, y_old, nb, name)
    ref = _ref(name, "random", True)
    _check(y_new, ref, R.GAMMA_CONV, "wsd wide " + name, "bf16", "random", "dx")
    R.assert_nb_sums(s_new, ref, nbh + (0.01,), R.GAMMA_CONV, "wsd wide " + name)


def _model_operands(cin, cout, n=2, s=16):
    dy = _u(n, s, s, s, cin, seed=41).to(DEV)
    spec = _packed(OP, cout, cin, _weights(OP, cout, cin, "random", seed=42), "bf16")
    res = _u(n, s, s, s, cout, seed=43).to(DEV)
    nb = (_u(n, s, s, s, cout, seed=44).to(DEV), _u(n, cout, seed=45, lo_=0.5, hi_=1.5).to(DEV), _u(n, cout, seed=46).to(DEV), 0.01)
    return dy, spec, res, nb


@pytest.mark.parametrize("cin,cout", [(128, 128), (256, 128), (128, 256)])
def test_wsd_model_shapes_on_the_product_route(hip, cin, cout):
    """the step's launches at 16^3, batch 2, as the step makes them (residual + norm-backward sums), default knobs: one launch of the new
    kernel each, bit-equal to the tap-table kernel and to itself"""
    n, size = 2, (16, 16, 16)
    dy, spec, res, nb = _model_operands(cin, cout)
    y_a, s_a = _run(hip, 1, dy, spec, cout, res, nb, n, size)
    y_b, s_b = _run(hip, 1, dy, spec, cout, res, nb, n, size)
    y_old, s_old = _run(hip, 0, dy, spec, cout, res, nb, n, size)
    assert torch.equal(y_a, y_old), float((y_a - y_old).abs().max())
    assert torch.equal(y_a, y_b)
    _sums_equal(s_a, s_old, y_old, nb, (cin, cout))
    _sums_equal(s_b, s_old, y_old, nb, (cin, cout))


def test_wsd_route(hip):
    """what the product route (default knobs) takes and what it leaves alone"""
    assert hip.lib.cwf_debug_wsd(1) == 1                   # the default, and the knob returns the previous value
    assert hip.lib.cwf_debug_wsd(2) == 1 and hip.lib.cwf_debug_wsd(1) == 2
    # the larger 32- / 64-channel layers keep their kernels
    for c, s in ((32, 64), (64, 32)):
        spec = _packed(OP, c, c, _weights(OP, c, c, "random", seed=42), "bf16")
        _run(hip, 1, torch.rand((2, s, s, s, c), device=DEV), spec, c, None, None, 2, (s, s, s), expect=0)
    dy, spec, res, nb = _model_operands(128, 128)
    n, size, cout = 2, (16, 16, 16), 128
    _run(hip, 1, dy, spec, cout, None, None, n, size, expect=1)
    _run(hip, 0, dy, spec, cout, None, None, n, size, expect=0)
    before = _launches(hip)
    # a per-channel output scale stays off this route
    osc = _u(n, cout, seed=47, lo_=0.5, hi_=1.5).to(DEV)
    hip.conv(OP, dy, spec.wpk16_d, None, cout, out_scale=osc, out=torch.empty((n, *size, cout), device=DEV), prec="bf16", fwd_op=OP)
    # the split-bf16 form and a launch with a prologue stay off it
    spec3 = _packed(OP, cout, 128, _weights(OP, cout, 128, "random", seed=42), "bf16x3")
    hip.conv(OP, dy, spec3.wpk16_d, None, cout, out=torch.empty((n, *size, cout), device=DEV), prec="bf16x3", fwd_op=OP)
    hip.conv(OP, dy, spec.wpk16_d, None, cout, slope=0.01, out=torch.empty((n, *size, cout), device=DEV), prec="bf16", fwd_op=OP)
    # a bf16 input image goes to the image routes: 128 -> 256 @16^3 is one conv_ws.hip takes as an image
    dy2, spec2, res2, nb2 = _model_operands(128, 256)
    assert hip.lib.cwf_conv_x16_ok(OP, n, 16, 16, 16, 128, 256) == 1
    hip.conv(OP, dy2, spec2.wpk16_d, None, 256, out=torch.empty((n, *size, 256), device=DEV), prec="bf16", fwd_op=OP, x16=dy2.to(torch.bfloat16))
    # channel groups (the grouped entry point): three 128 -> 32 convs in one launch
    specs = [_packed(OP, 128, 32, _weights(OP, 128, 32, "random", seed=50 + q), "bf16") for q in range(3)]
    xg = _u(n, 8, 8, 16, 3 * 128, seed=48).to(DEV)
    yg = torch.empty((n, 8, 8, 16, 3 * 32), device=DEV)
    hip.conv_grouped(xg, 128, [s_.wpk16_f for s_ in specs], None, 32, yg, x_goff=128, y_goff=32, prec="bf16")
    torch.cuda.synchronize()
    assert _launches(hip) == before


def test_wsd_argument_errors_launch_nothing(hip):
    """argument errors return the codes they returned before, without a launch"""
    from cwf import _lib
    n, size, cin, cout = 2, (16, 16, 16), 128, 128
    dy, spec, res, nb = _model_operands(cin, cout)
    y = torch.empty((n, *size, cout), device=DEV)

    def call(**kw):
        a = _lib.ConvArgs(op=OP, precision=_lib.PRECISION["bf16"], x=dy.data_ptr(), x_ldc=cin, wpk=spec.wpk16_d.data_ptr(), y=y.data_ptr(),
                          y_ldc=cout, in_slope=1.0, nb_slope=1.0, N=n, Di=16, Hi=16, Wi=16, Cin=cin, Do=16, Ho=16, Wo=16, Cout=cout)
        for k, v in kw.items():
            setattr(a, k, v)
        return hip.lib.cwf_conv(ctypes.addressof(a), None)

    rcs = {}
    for knob in (1, 0):
        old = hip.lib.cwf_debug_wsd(knob)
        before = _launches(hip)
        try:
            rcs[knob] = [call(wpk=None), call(y=None), call(x_ldc=cin - 4), call(y_ldc=cout - 1), call(x=dy.data_ptr() + 4),
                         call(nb_x=nb[0].data_ptr()), call(N=0)]
        finally:
            hip.lib.cwf_debug_wsd(old)
        torch.cuda.synchronize()
        assert _launches(hip) == before
    assert all(rc != 0 for rc in rcs[1]) and rcs[1] == rcs[0], rcs
