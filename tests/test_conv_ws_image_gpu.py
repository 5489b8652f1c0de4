"""GPU: the weight-stationary data gradient reading its incoming gradient as a bf16 image (convws_kernel<false, true>: conv(..., x16=) on the
32- / 64-channel 3x3x3 stride-1 layers; halo and weights by LDS-DMA, loader waves, two A images per group).

The fp32-input launch rounds dy to bf16 (RNE) in its loader; the image holds the same rounded values, so the two launches multiply the same
operands in the same order: dx must be BIT-EQUAL, and the norm-backward sums equal up to the order of their float64 atomics.  Beside that
the image launch is held to the operand-exact float64 reference (tests/bf16_operand_ref.py) like every other bf16 conv path.
cwf_debug_ws_min_units(1) lets the small shapes reach the kernel (the product sends layers of >= 256 (tile, output group) units)."""
import contextlib
import functools
import math

import pytest
import torch

import bf16_operand_ref as R
from cwf import packing as pk
from cwf._lib import CwfError
from test_conv_bf16_exact_gpu import _field, _packed, _u, _weights

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PROBES = ["random", "positive", "impulse"]
# forward (cin -> cout, input size, n): the data gradient is a cout -> cin launch
CASES = {
    "64to32": (64, 32, (8, 8, 32), 2),       # two chunks (weights stay resident), two output groups, every face of the volume a tile edge
    "32to64": (32, 64, (4, 12, 16), 1),      # four chunks (weights reloaded per block), 3 tiles: a group without an item, a short last round
}


@contextlib.contextmanager
def _knob(hip, units):
    old = hip.lib.cwf_debug_ws_min_units(units)
    try:
        yield
    finally:
        hip.lib.cwf_debug_ws_min_units(old)


@functools.lru_cache(maxsize=None)
def _case(case, probe, feat):
    """operands (CPU) and the float64 operand reference of one case: computed once, shared, never modified"""
    cin, cout, size, n = CASES[case]
    w = _weights(pk.CONV3_S1, cin, cout, probe, seed=61)
    dy = _field((n, *size, cout), probe, seed=62)
    res = None
    if "r" in feat and probe != "impulse":
        res = _field((n, *size, cin), "positive" if probe == "positive" else "random", seed=63)
    nb = (_u(n, *size, cin, seed=64), _u(n, cin, seed=65, lo_=0.5, hi_=1.5), _u(n, cin, seed=66), 0.01) if "N" in feat else None
    ref = R.conv_ref(pk.CONV3_S1, dy, w, "bf16", residual=res, dgrad=True, out_size=size)
    return w, dy, res, nb, ref


def _launch(hip, spec, dy, cin, res, nb, image, out=None, **kw):
    """one data-gradient launch: from the fp32 tensor (image None) or from the bf16 image"""
    n = dy.shape[0]
    sums = hip.new_stats(n, cin, dy.device) if nb is not None else None
    out = torch.empty((*dy.shape[:4], cin), device=dy.device) if out is None else out
    dx = hip.conv(pk.CONV3_S1, dy, spec.wpk16_d, None, cin, residual=res, out=out, prec="bf16", fwd_op=pk.CONV3_S1, stats=sums, nb=nb,
                  x16=image, **kw)
    return dx, sums


def _dev(t):
    return None if t is None else t.to(DEV)


def _sums_close(s_img, s_f32, dx, nb, what):
    """both launches form the same fp32 partial sums (same work split, same waves) and add them in float64 in a different order: at most
    2^13 partials per (sample, channel), each addition off by 2^-53 of the running sum <= sum |terms|  ->  2^-40 sum |terms|"""
    x, sc, sh, slope = nb
    h = (x.double() * sc.double()[:, None, None, None, :] + sh.double()[:, None, None, None, :]).float().double()
    gn = dx.double() * torch.where(h > 0, torch.ones_like(h), torch.full_like(h, slope))
    t = torch.stack([gn.abs().sum((1, 2, 3)), (gn * h).abs().sum((1, 2, 3))], -1)
    err = (s_img.double() - s_f32.double()).abs()
    assert bool((err <= 2.0 ** -40 * t + 1e-300).all()), (what, float((err / t.clamp_min(1e-300)).max()))


@pytest.mark.parametrize("feat", ["rN", ""])
@pytest.mark.parametrize("probe", PROBES)
@pytest.mark.parametrize("case", list(CASES))
def test_image_launch_is_operand_exact_and_bit_equal(hip, case, probe, feat):
    cin, cout, size, n = CASES[case]
    w, dy, res, nb, ref = _case(case, probe, feat)
    spec = _packed(pk.CONV3_S1, cin, cout, w, "bf16")
    dyd, resd = dy.to(DEV), _dev(res)
    nbd = None if nb is None else (nb[0].to(DEV), nb[1].to(DEV), nb[2].to(DEV), nb[3])
    with _knob(hip, 1):
        assert hip.lib.cwf_conv_x16_ok(pk.CONV3_S1, n, *size, cout, cin) == 1
        dx32, s32 = _launch(hip, spec, dyd, cin, resd, nbd, None)
        dx16, s16 = _launch(hip, spec, dyd, cin, resd, nbd, dyd.to(torch.bfloat16))
        torch.cuda.synchronize()
    assert torch.equal(dx16, dx32), (case, probe, feat, float((dx16 - dx32).abs().max()))
    if probe == "impulse":
        assert torch.equal(ref.pick(dx16), ref.y), (case, feat, float((ref.pick(dx16) - ref.y).abs().max()))
    else:
        worst = R.check(dx16, ref, R.GAMMA_CONV, "dgrad ws x16 %s %s %s" % (case, probe, feat))
        print("\nworst err/A  dgrad ws x16 %-8s %-8s %-2s %.3e  (%.2f x 2^-18)" % (case, probe, feat, worst, worst / 2.0 ** -18))
        if nb is not None:
            R.assert_nb_sums(s16, ref, nb, R.GAMMA_CONV, "ws x16 " + case)
            R.assert_nb_sums(s32, ref, nb, R.GAMMA_CONV, "ws f32 " + case)
    if nb is not None:
        _sums_close(s16, s32, dx16, nbd, (case, probe))


def test_steady_state_and_a_sample_boundary_inside_a_workgroup(hip):
    """forward 32 -> 32 at 32 x 32 x 80, n = 3: 960 tiles on 256 workgroups, several rounds per workgroup (both A images and both weight
    buffers in turn); tile 320, the first of sample 1, falls inside workgroup 85's range [318, 322) of the kernel's own split
    (slot * tiles / slots), so that workgroup flushes its sums in mid-range"""
    c, size, n = 32, (32, 32, 80), 3
    tiles, slots = n * (size[0] // 4) * (size[1] // 4) * (size[2] // 16), 256
    per_n = tiles // n
    assert (tiles, per_n) == (960, 320)
    assert any((s * tiles) // slots < per_n < ((s + 1) * tiles) // slots for s in range(slots)), "no sample boundary inside a range"
    assert (85 * tiles // slots, 86 * tiles // slots) == (318, 322)
    w = _weights(pk.CONV3_S1, c, c, "random", seed=71)
    spec = _packed(pk.CONV3_S1, c, c, w, "bf16")
    dy, res = _u(n, *size, c, seed=72).to(DEV), _u(n, *size, c, seed=73).to(DEV)
    nb = (_u(n, *size, c, seed=74).to(DEV), _u(n, c, seed=75, lo_=0.5, hi_=1.5).to(DEV), _u(n, c, seed=76).to(DEV), 0.01)
    assert hip.lib.cwf_conv_x16_ok(pk.CONV3_S1, n, *size, c, c) == 1          # (960 units: no knob needed)
    dx32, s32 = _launch(hip, spec, dy, c, res, nb, None)
    dx16, s16 = _launch(hip, spec, dy, c, res, nb, dy.to(torch.bfloat16))
    torch.cuda.synchronize()
    assert torch.equal(dx16, dx32), float((dx16 - dx32).abs().max())
    assert bool((s16[..., 0].abs() > 0).all())
    _sums_close(s16, s32, dx16, nb, "steady state")


def test_the_fp32_tensor_is_not_read(hip):
    cin, cout, size, n = CASES["64to32"]
    w, dy, res, nb, _ = _case("64to32", "random", "rN")
    spec = _packed(pk.CONV3_S1, cin, cout, w, "bf16")
    dyd, resd = dy.to(DEV), res.to(DEV)
    nbd = (nb[0].to(DEV), nb[1].to(DEV), nb[2].to(DEV), nb[3])
    img = dyd.to(torch.bfloat16)
    with _knob(hip, 1):
        dx_a, s_a = _launch(hip, spec, dyd, cin, resd, nbd, img)
        dx_b, s_b = _launch(hip, spec, torch.full_like(dyd, float("nan")), cin, resd, nbd, img)
        torch.cuda.synchronize()
    assert bool(torch.isfinite(dx_b).all()) and bool(torch.isfinite(s_b).all())
    assert torch.equal(dx_a, dx_b)
    _sums_close(s_b, s_a, dx_a, nbd, "NaN fp32 tensor")


def test_writes_stay_in_their_channel_slice(hip):
    cin, cout, size, n = CASES["64to32"]
    w, dy, res, nb, ref = _case("64to32", "random", "rN")
    spec = _packed(pk.CONV3_S1, cin, cout, w, "bf16")
    dyd = dy.to(DEV)
    nbd = (nb[0].to(DEV), nb[1].to(DEV), nb[2].to(DEV), nb[3])
    wide = torch.full((n, *size, cin + 8), 7.0, device=DEV)
    with _knob(hip, 1):
        dx, _ = _launch(hip, spec, dyd, cin, res.to(DEV), nbd, dyd.to(torch.bfloat16), out=wide[..., 4:4 + cin])
        torch.cuda.synchronize()
    assert bool((wide[..., :4] == 7.0).all()) and bool((wide[..., 4 + cin:] == 7.0).all()), "wrote outside its channel slice"
    R.check(wide[..., 4:4 + cin], ref, R.GAMMA_CONV, "ws x16 into a slice")


def test_argument_checks(hip, monkeypatch):
    """every refusal is CWF_E_BADARG (-1) or CWF_E_ALIGN (-3), returned before anything is launched (the output keeps its sentinel)"""
    cin, cout, size, n = CASES["64to32"]
    w = _weights(pk.CONV3_S1, cin, cout, "random", seed=61)
    spec = _packed(pk.CONV3_S1, cin, cout, w, "bf16")
    dy = _u(n, *size, cout, seed=62).to(DEV)
    img = dy.to(torch.bfloat16)
    out = torch.full((n, *size, cin), 7.0, device=DEV)

    def refused(image=img, prec="bf16", **kw):
        with pytest.raises(CwfError, match=r"status -[13]\b"):
            hip.conv(pk.CONV3_S1, dy, spec.wpk16_d, None, cin, out=out, prec=prec, fwd_op=pk.CONV3_S1, x16=image, **kw)
        torch.cuda.synchronize()
        assert bool((out == 7.0).all()), kw

    with _knob(hip, 1):
        refused(in_scale=torch.ones(n, cout, device=DEV), in_shift=torch.zeros(n, cout, device=DEV), slope=0.01)      # a prologue
        refused(out_scale=torch.ones(n, cin, device=DEV))
        refused(prec="bf16x3")
        refused(prec="fp32")
        flat = torch.zeros(img.numel() + 8, dtype=torch.bfloat16, device=DEV)
        off = flat[4:4 + img.numel()].view(img.shape)                     # contiguous, 8 bytes off a 16-byte boundary
        off.copy_(img)
        assert off.is_contiguous() and off.data_ptr() % 16 == 8
        refused(image=off)
        page = torch.zeros(64, dtype=torch.uint8, device=DEV)
        monkeypatch.setattr(hip, "zero16", lambda device: page[8:])
        refused()
        monkeypatch.undo()
        hip.conv(pk.CONV3_S1, dy, spec.wpk16_d, None, cin, out=out, prec="bf16", fwd_op=pk.CONV3_S1, x16=img)      # the same call, accepted
        torch.cuda.synchronize()
        assert not bool((out == 7.0).any())
        out.fill_(7.0)
    # a layer the predicate rejects (16 x 2 units, below the threshold at its default): never a different computation
    assert hip.lib.cwf_conv_x16_ok(pk.CONV3_S1, n, *size, cout, cin) == 0
    refused()


def _stacked_graph(hip, n, size, c):
    """three stacked c -> c convs, the second and third with InstanceNorm + LeakyReLU prologues, in a single-consumer graph under a gradient
    sink: the apply pass of layer 3 hands layer 2 its gradient, the apply pass of layer 2 hands layer 1 its gradient.  Returns the sink
    gradients of (w1, b1, w2, b2, w3, b3)."""
    from cwf import functional as CF
    from cwf.optim import GradSink
    K = CF.backend()
    ws = [_u(c, c, 3, 3, 3, seed=81 + i) / math.sqrt(27 * c) for i in range(3)]
    bs = [_u(c, seed=91 + i) * 0.1 for i in range(3)]
    params = []
    for w, b in zip(ws, bs):
        params += [torch.nn.Parameter(w.to(DEV).contiguous()), torch.nn.Parameter(b.to(DEV).contiguous())]
    specs = [CF.ConvSpec(pk.CONV3_S1, c, c) for _ in range(3)]
    packer = CF.WeightPacker()
    for s, p in zip(specs, params[0::2]):
        packer.add(s, p)
    packer.refresh()
    sink = GradSink(params)
    x, q = _u(n, *size, c, seed=101).to(DEV), _u(n, *size, c, seed=102).to(DEV)
    with CF.single_consumer_graph():
        y1, st1 = CF.conv(x, params[0], params[1], specs[0], want_stats=True)
        y2, st2 = CF.conv(y1, params[2], params[3], specs[1], in_norm=st1, slope=0.01, want_stats=True)
        y3, _ = CF.conv(y2, params[4], params[5], specs[2], in_norm=st2, slope=0.01)
    loss = (y3 * q).sum()
    sink.begin()
    with sink:
        loss.backward()
    K.wgrad_flush()
    torch.cuda.synchronize()
    assert all(p.grad is None for p in params)
    return [sink.view(p).clone() for p in params]


def test_bf16_only_handoff_reaches_the_image_launch(hip, monkeypatch):
    """functional.conv declares a residual-free layer's gradient "bf16 image only" exactly where the library will launch the image kernel:
    with the fp32 carriers poisoned, no NaN reaches a gradient, and the gradients are those of the same graph on fp32 gradients -- with the
    layers eligible (knob 1) and not (default: 16 units)."""
    from cwf import kernels
    n, size, c = 2, (8, 8, 32), 32
    calls, need = [], []
    conv0, apply0 = hip.conv, hip.in_bwd_apply16

    def conv_spy(*a, **kw):
        calls.append(kw.get("x16") is not None)
        return conv0(*a, **kw)

    def apply_spy(*a, **kw):
        need.append(kw.get("need_f32", True))
        return apply0(*a, **kw)
    monkeypatch.setattr(hip, "conv", conv_spy)
    monkeypatch.setattr(hip, "in_bwd_apply16", apply_spy)
    monkeypatch.setattr(kernels, "POISON_UNWRITTEN_CARRIERS", True)
    kernels.set_precision("bf16x3", wgrad="bf16", dgrad="bf16")
    try:
        for units, eligible in ((1, True), (None, False)):
            knob = (lambda: _knob(hip, units)) if units else contextlib.nullcontext
            # the reference: the same graph under the same knob (the knob also moves the fp32-input data gradients between kernels) with
            # every gradient handed on as an fp32 tensor
            calls.clear(); need.clear()
            with monkeypatch.context() as m, knob():
                m.setattr(hip, "bf16_dgrad_ok", lambda *a: False)
                ref = _stacked_graph(hip, n, size, c)
            assert not any(calls) and all(need), (calls, need)
            calls.clear(); need.clear()
            with knob():
                got = _stacked_graph(hip, n, size, c)
            assert any(calls) == eligible and (False in need) == eligible, (units, calls, need)
            for g, r, what in zip(got, ref, ("w1", "b1", "w2", "b2", "w3", "b3")):
                assert bool(torch.isfinite(g).all()), (units, what)
                # same kernels' arithmetic on the same operands in both graphs (the image launch is bit-equal to the fp32-input launch); what
                # may differ is the order of the float64 atomics in the norm-backward sums, i.e. the last fp32 bit of a per-channel
                # coefficient, carried through at most two layers of gradients
                tol = 2e-5 * float(r.abs().max())
                err = float((g - r).abs().max())
                print("\nhand-off units=%s %s: max |diff| %.3e of max |ref| %.3e" % (units, what, err, float(r.abs().max())))
                assert err <= tol, (units, what, err, tol)
    finally:
        kernels.set_precision("fp32")
