"""CPU: the operand-exact float64 reference of tests/bf16_operand_ref.py -- against torch's float64 convs and autograd adjoints in
fp32 mode, self-consistency of its bf16 operand forms, and its power to see the defects the fp32-oracle bound lets through
(planted in the reference's own output, never in a kernel)."""
import math

import pytest
import torch
import torch.nn.functional as F

import bf16_operand_ref as R

OPS = [(R.CONV3_S1, 3), (R.CONV3_S2, 3), (R.CONV1, 1), (R.CONVT2, 2)]


def _u(*shape, seed, lo_=-1.0, hi_=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(*shape, generator=g) * (hi_ - lo_) + lo_


def _w(op, cin, cout, seed, positive=False):
    k = {R.CONV3_S1: 3, R.CONV3_S2: 3, R.CONV1: 1, R.CONVT2: 2}[op]
    shape = (cin, cout, k, k, k) if op == R.CONVT2 else (cout, cin, k, k, k)
    s = 1.0 / math.sqrt(cin * k ** 3)
    return _u(*shape, seed=seed, lo_=0.5 * s if positive else -s, hi_=s)


def _torch_fwd(op, x, w):
    xc = x.permute(0, 4, 1, 2, 3)
    if op == R.CONVT2:
        y = F.conv_transpose3d(xc, w, stride=2)
    else:
        y = F.conv3d(xc, w, stride=2 if op == R.CONV3_S2 else 1, padding=1 if op in (R.CONV3_S1, R.CONV3_S2) else 0)
    return y.permute(0, 2, 3, 4, 1)


@pytest.mark.parametrize("op,k", OPS)
@pytest.mark.parametrize("size", [(5, 6, 7), (4, 4, 16)])
def test_fp32_mode_is_torch_float64(op, k, size):
    """fp32 mode == float64 F.conv3d / conv_transpose3d (forward, with prologue / bias / residual / out_scale), the autograd adjoint
    (data gradient, every parity class) and autograd's weight / bias gradient."""
    n, cin, cout = 2, 4, 8
    x = _u(n, *size, cin, seed=1)
    w = _w(op, cin, cout, seed=2)
    b, sc, sh = _u(cout, seed=3), _u(n, cin, seed=4, lo_=0.5, hi_=1.5), _u(n, cin, seed=5)
    osc = _u(n, cout, seed=6)
    xa = R.prologue(x, sc, sh, 0.01).double()
    y0 = _torch_fwd(op, xa, w.double())
    res = _u(*y0.shape, seed=7)
    ref = R.conv_ref(op, x, w, "fp32", bias=b, in_scale=sc, in_shift=sh, slope=0.01, residual=res, out_scale=osc)
    want = (y0 + b.double() + res.double()) * osc.double()[:, None, None, None, :]
    assert torch.allclose(ref.y, want, rtol=1e-12, atol=1e-12)
    assert bool((ref.A >= ref.y.abs() - 1e-12).all())
    # data gradient: the adjoint w.r.t. the (activated) input
    dy = _u(*y0.shape, seed=8)
    xin = torch.zeros(n, *size, cin, dtype=torch.float64, requires_grad=True)
    (gx,) = torch.autograd.grad(_torch_fwd(op, xin, w.double()), xin, dy.double())
    dref = R.conv_ref(op, dy, w, "fp32", dgrad=True, out_size=size)
    assert torch.allclose(dref.y, gx, rtol=1e-12, atol=1e-12)
    # weight / bias gradient
    wv = w.double().clone().requires_grad_(True)
    bv = torch.zeros(cout, dtype=torch.float64, requires_grad=True)
    y = _torch_fwd(op, xa, wv) + bv
    gw, gb = torch.autograd.grad(y, (wv, bv), dy.double())
    dw, db, aw, ab = R.wgrad_ref(op, x, dy, "fp32", sc, sh, 0.01)
    assert torch.allclose(dw, gw, rtol=1e-12, atol=1e-12) and torch.allclose(db, gb, rtol=1e-12, atol=1e-12)
    assert bool((aw >= dw.abs() - 1e-12).all()) and bool((ab >= db.abs() - 1e-12).all())


@pytest.mark.parametrize("op,k", OPS)
def test_single_bf16_equals_fp32_on_representable_operands(op, k):
    """bf16-representable input and weights, no prologue: the single-bf16 reference is the fp32-mode reference"""
    n, cin, cout, size = 2, 8, 4, (4, 5, 6)
    x = R.hi(_u(n, *size, cin, seed=11)).float()
    w = R.hi(_w(op, cin, cout, seed=12)).float()
    a, b = R.conv_ref(op, x, w, "bf16"), R.conv_ref(op, x, w, "fp32")
    assert torch.equal(a.y, b.y) and torch.equal(a.A, b.A)
    dy = R.hi(_u(*a.y.shape, seed=13)).float()
    assert torch.equal(R.conv_ref(op, dy, w, "bf16", dgrad=True, out_size=size).y, R.conv_ref(op, dy, w, "fp32", dgrad=True, out_size=size).y)
    wa, wb = R.wgrad_ref(op, x, dy, "bf16"), R.wgrad_ref(op, x, dy, "fp32")
    assert torch.equal(wa[0], wb[0]) and torch.equal(wa[1], wb[1])


@pytest.mark.parametrize("op,k", OPS)
def test_split_products_are_within_2_15_of_exact(op, k):
    """per product: lo(a) and lo(b) carry 2^-17 relative rounding each and lo.lo (<= 2^-16) is dropped, so |split - exact| <=
    3 * 2^-17 |a||b| < 2^-15 A; a ConvTranspose output is ONE product per channel, the 3x3x3 sums average below 2^-16"""
    n, cin, cout, size = 1, 16, 8, (4, 6, 8)
    x, w = _u(n, *size, cin, seed=21), _w(op, cin, cout, seed=22)
    sc, sh = _u(n, cin, seed=23, lo_=0.5, hi_=1.5), _u(n, cin, seed=24)
    a = R.conv_ref(op, x, w, "bf16x3", in_scale=sc, in_shift=sh, slope=0.01)
    b = R.conv_ref(op, x, w, "fp32", in_scale=sc, in_shift=sh, slope=0.01)
    assert float(((a.y - b.y).abs() / b.A).max()) <= (2.0 ** -15 if op == R.CONVT2 else 2.0 ** -16)
    single = R.conv_ref(op, x, w, "bf16", in_scale=sc, in_shift=sh, slope=0.01)
    assert float(((single.y - b.y).abs() / b.A).max()) > 2.0 ** -12        # (the single form is visibly coarser)
    dy = _u(*a.y.shape, seed=25)
    wa, wb = R.wgrad_ref(op, x, dy, "bf16x3", sc, sh, 0.01), R.wgrad_ref(op, x, dy, "fp32", sc, sh, 0.01)
    assert float(((wa[0] - wb[0]).abs() / wb[2]).max()) <= 2.0 ** -15


def test_prologue_is_fp32_fma_then_activation_then_padding():
    """h = fp32(x * s + t) (one rounding), max(h, h * slope) in fp32; padded voxels contribute zero even where act(shift) != 0"""
    x = torch.zeros(1, 3, 3, 3, 4)
    sc, sh = torch.ones(1, 4), torch.full((1, 4), -0.75)
    w = torch.ones(2, 4, 3, 3, 3)
    ref = R.conv_ref(R.CONV3_S1, x, w, "fp32", in_scale=sc, in_shift=sh, slope=0.01)
    inb = torch.tensor([2, 3, 2]).view(3, 1, 1) * torch.tensor([2, 3, 2]).view(1, 3, 1) * torch.tensor([2, 3, 2]).view(1, 1, 3)
    act = float(torch.tensor(-0.75, dtype=torch.float32) * torch.tensor(0.01, dtype=torch.float32))
    assert torch.allclose(ref.y[0, ..., 0], 4 * act * inb.double(), rtol=1e-12)


def _simulate_fp32_kernel(op, x, w, mode, **kw):
    """a correct kernel: the exact operand products of `mode` accumulated in fp32, 32 products per step (one MFMA K) -- here the
    reference's own gather with fp32 matmuls over 32-wide K slices"""
    tabs_ref = R.conv_ref(op, x, w, mode, **kw)
    W = R._weight_matrix(op, w, kw.get("dgrad", False))
    T, C, Co = W.shape
    n = x.shape[0]
    dims = tabs_ref.y.shape[1:4]
    xa = R.prologue(x[..., :C], kw.get("in_scale"), kw.get("in_shift"), kw.get("slope", 1.0))
    tabs = [R._dim_table(op, kw.get("dgrad", False), dims[i], x.shape[1 + i]) for i in range(3)]
    vox = R._all_voxels(n, dims)
    acc = torch.zeros(vox[0].numel(), Co, dtype=torch.float32)
    for xp, wp in R.split_terms(xa, W.float(), mode):
        wm = wp.reshape(T * C, Co)
        for sl, p in R._gather(xp, tabs, vox, 1 << 30):
            for s in range(0, T * C, 32):
                acc[sl] += (p[:, s:s + 32] @ wm[s:s + 32]).float()          # exact products, one fp32 rounding per 32-wide step
    return acc.view(n, *dims, Co), tabs_ref


# the issue's setup: 16 -> 16 3x3x3 on 1 x 18 x 20 x 50 (ragged in W against the 16-wide tile)
CASE = dict(n=1, size=(18, 20, 50), c=16)


def _case(positive, seed=0):
    n, (d, h, w_), c = CASE["n"], CASE["size"], CASE["c"]
    x = _u(n, d, h, w_, c, seed=31 + seed, lo_=0.5 if positive else -1.0)
    w = _w(R.CONV3_S1, c, c, seed=32 + seed, positive=positive)
    return x, w


@pytest.mark.parametrize("mode", ["bf16", "bf16x3"])
@pytest.mark.parametrize("positive", [False, True])
def test_correct_fp32_accumulating_kernel_passes(mode, positive):
    x, w = _case(positive)
    got, ref = _simulate_fp32_kernel(R.CONV3_S1, x, w, mode)
    worst = R.check(got, ref, R.GAMMA_CONV, "simulated kernel")
    assert worst < R.GAMMA_CONV / 4


def _fails_by(got, ref: R.Ref, gamma, factor=30):
    r = float(((got.double() - ref.y).abs() / ref.A.clamp_min(1e-300)).max())
    assert r >= factor * gamma, (r, r / gamma)
    with pytest.raises(AssertionError):
        R.check(got, ref, gamma, "planted defect")
    return r


@pytest.mark.parametrize("mode", ["bf16", "bf16x3"])
@pytest.mark.parametrize("positive", [False, True])
def test_planted_conv_defects_fail_by_30x(mode, positive):
    x, w = _case(positive)
    ref = R.conv_ref(R.CONV3_S1, x, w, mode)
    W = ref.y.shape[3]
    last_w0 = ((W - 1) // 16) * 16

    # (1) one (input channel, tap) pair missing on the last ragged W tile
    def drop(vox, t):
        return ~((vox[3] >= last_w0) & (t == 13))
    d1 = R.conv_ref(R.CONV3_S1, x, w, mode, tap_filter=drop)      # (tap 13 = centre, all 16 channels: the channel-chunk of one tap)
    # narrow it to one input channel: remove only channel 5 of the centre tap
    one = ref.y.clone()
    xa = R.prologue(x)
    terms = R.split_terms(xa[..., 5], w[:, 5, 1, 1, 1], mode)
    contrib = sum(xp[..., None] * wp for xp, wp in terms)             # [n, d, h, w, cout]
    one[:, :, :, last_w0:] -= contrib[:, :, :, last_w0:]
    _fails_by(d1.y.float(), ref, R.GAMMA_CONV)
    _fails_by(one.float(), ref, R.GAMMA_CONV)
    # (2) truncating fp32 -> bf16 conversion instead of round-to-nearest-even (single-bf16 products only: in split form the lo
    # part absorbs a truncated hi, and the lo part's own truncation is ~2^-17 relative -- below what gamma can separate)
    if mode == "bf16":
        tr = R.conv_ref(R.CONV3_S1, x, w, mode, hi_fn=R.hi_trunc)
        _fails_by(tr.y.float(), ref, R.GAMMA_CONV)
    # (3) the last input column read as zero
    xz = x.clone(); xz[:, :, :, -1] = 0
    _fails_by(R.conv_ref(R.CONV3_S1, xz, w, mode).y.float(), ref, R.GAMMA_CONV)


@pytest.mark.parametrize("mode", ["bf16", "bf16x3"])
@pytest.mark.parametrize("positive", [False, True])
def test_planted_wgrad_defects_fail_by_30x(mode, positive):
    """a dropped 4x4x16 output tile of a weight gradient, and the truncating conversion, against the bound of 2^-16"""
    n, (d, h, w_), c = 2, (8, 12, 40), 16
    x = _u(n, d, h, w_, c, seed=41, lo_=0.5 if positive else -1.0)
    dy = _u(n, d, h, w_, c, seed=42, lo_=0.5 if positive else -1.0)
    sc, sh = _u(n, c, seed=43, lo_=0.5, hi_=1.5), _u(n, c, seed=44, lo_=0.0 if positive else -1.0)
    dw, db, aw, ab = R.wgrad_ref(R.CONV3_S1, x, dy, mode, sc, sh, 0.01)

    def ratio(a, b, A):
        return float(((a - b).abs() / A.clamp_min(1e-300)).max())
    lastw = ((w_ - 1) // 16) * 16
    tile = lambda v: ~((v[0] == n - 1) & (v[1] >= 4) & (v[1] < 8) & (v[2] >= 8) & (v[3] >= lastw))     # ragged last W tile, last sample
    dw2, db2, _, _ = R.wgrad_ref(R.CONV3_S1, x, dy, mode, sc, sh, 0.01, tile_filter=tile)
    assert ratio(dw2, dw, aw) >= 30 * R.GAMMA_WGRAD and ratio(db2, db, ab) >= 30 * R.GAMMA_WGRAD
    with pytest.raises(AssertionError):
        R.assert_operand_exact(dw2.float(), dw, aw, R.GAMMA_WGRAD, "dropped tile")
    if mode != "bf16":
        return
    dw3, db3, _, _ = R.wgrad_ref(R.CONV3_S1, x, dy, mode, sc, sh, 0.01, hi_fn=R.hi_trunc)
    assert ratio(dw3, dw, aw) >= 30 * R.GAMMA_WGRAD
    with pytest.raises(AssertionError):
        R.assert_operand_exact(dw3.float(), dw, aw, R.GAMMA_WGRAD, "truncation")


def test_fp32_oracle_bound_misses_what_this_one_sees():
    """the motivating gap: a missing channel-tap pair on the ragged tile passes 2 * 3e-2 * max|ref| against the fp32 answer"""
    x, w = _case(False)
    ref = R.conv_ref(R.CONV3_S1, x, w, "bf16")
    fp32 = R.conv_ref(R.CONV3_S1, x, w, "fp32")
    last_w0 = ((ref.y.shape[3] - 1) // 16) * 16
    bad = ref.y.clone()
    xa = R.prologue(x)
    bad[:, :, :, last_w0:] -= (R.hi(xa[..., 5])[..., None] * R.hi(w[:, 5, 1, 1, 1]))[:, :, :, last_w0:]
    assert float((bad - fp32.y).abs().max()) <= 2 * 3e-2 * float(fp32.y.abs().max())        # today's bound lets it through
    _fails_by(bad.float(), ref, R.GAMMA_CONV)


def test_sampled_reference_matches_the_full_one():
    n, size, cin, cout = 2, (9, 10, 37), 8, 16
    x, w = _u(n, *size, cin, seed=51), _w(R.CONV3_S2, cin, cout, seed=52)
    b = _u(cout, seed=53)
    for op in (R.CONV3_S1, R.CONV3_S2):
        full = R.conv_ref(op, x, w, "bf16x3", bias=b)
        vox = R.edge_voxels(n, full.y.shape[1:4], n_random=64)
        part = R.conv_ref(op, x, w, "bf16x3", bias=b, vox=vox)
        assert torch.equal(part.y, full.y[vox]) and torch.equal(part.A, full.A[vox])
        assert torch.equal(part.pick(full.y.float()), full.y.float().double()[vox])
