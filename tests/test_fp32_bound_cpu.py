"""CPU: the bound of the exact-fp32 conv family, gamma_fp32(chain) of tests/bf16_operand_ref.py.  A simulated correct kernel -- exact
products, one fp32 rounding per product (the weaker rounding model), in the kernels' chain order -- stays within gamma / 4 at the
longest chains the GPU tests use; planted defects (in the reference's own output, never in a kernel) fail it by >= 30 gamma; and the
old normwise check close(rtol=2e-5) lets one of them through."""
import math

import pytest
import torch

import bf16_operand_ref as R

C3 = R.CONV3_S1


def _u(*shape, seed, lo_=-1.0, hi_=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(*shape, generator=g) * (hi_ - lo_) + lo_


def _w(op, cin, cout, seed, positive=False):
    k = {R.CONV3_S1: 3, R.CONV3_S2: 3, R.CONV1: 1, R.CONVT2: 2}[op]
    shape = (cin, cout, k, k, k) if op == R.CONVT2 else (cout, cin, k, k, k)
    s = 1.0 / math.sqrt(cin * k ** 3)
    return _u(*shape, seed=seed, lo_=0.5 * s if positive else -s, hi_=s)


def _fails_by(got, ref: R.Ref, gamma, factor=30):
    r = float(((got.double() - ref.y).abs() / ref.A.clamp_min(1e-300)).max())
    assert r >= factor * gamma, (r, r / gamma)
    with pytest.raises(AssertionError):
        R.check(got, ref, gamma, "planted defect")
    return r


def _close_passes(got, ref, rtol=2e-5):
    """tests/test_kernels_gpu.py close(): err <= atol + rtol max|ref| with atol = rtol max|ref|"""
    m = float(ref.abs().max())
    return float((got.double() - ref).abs().max()) <= 2 * rtol * m


# ------------------------------------------------------------------ forward / data gradient chain
def _simulate_conv_mfma(x, w, bias, residual, out_scale, sc, sh, slope):
    """conv_mfma_kernel's fp32 chain for a 3x3x3 stride-1 forward: per output one accumulator, chunk -> tap -> 4 MFMAs (i) -> 4 k
    slots (kq, channel 16 chunk + 4 kq + i), every product exact and added with one fp32 rounding; then + bias, + residual,
    * out_scale in fp32"""
    n, d, h, w_, cin = x.shape
    W = R._weight_matrix(C3, w, False)                                  # [27, cin, cout]
    T, C, Co = W.shape
    xa = R.prologue(x, sc, sh, slope)
    tabs = [R._dim_table(C3, False, (d, h, w_)[i], (d, h, w_)[i]) for i in range(3)]
    vox = R._all_voxels(n, (d, h, w_))
    (_, p), = list(R._gather(xa.double(), tabs, vox, 1 << 30))
    p = p.view(-1, T, C)
    acc = torch.zeros(p.shape[0], Co, dtype=torch.float32)
    for chunk in range(-(-C // 16)):
        for t in range(T):
            for i in range(4):
                for kq in range(4):
                    c = chunk * 16 + 4 * kq + i
                    if c < C:
                        acc = (acc.double() + p[:, t, c, None] * W[t, c][None, :]).float()
    acc = acc.view(n, d, h, w_, Co)
    acc = (acc + bias.float()) + residual.float()
    return acc * out_scale.float()[:, None, None, None, :]


@pytest.mark.parametrize("positive", [False, True])
def test_correct_fp32_chain_kernel_passes(positive):
    """the longest forward chain of the GPU tests: 256 input channels x 27 taps (+ the epilogue), ragged W"""
    n, size, cin, cout = 1, (3, 4, 21), 256, 16
    lo = 0.5 if positive else -1.0
    x, w = _u(n, *size, cin, seed=1, lo_=lo), _w(C3, cin, cout, seed=2, positive=positive)
    b, res = _u(cout, seed=3, lo_=0.0 if positive else -0.1, hi_=0.1), _u(n, *size, cout, seed=4, lo_=lo)
    osc, sc, sh = _u(n, cout, seed=5, lo_=0.5, hi_=1.5), _u(n, cin, seed=6, lo_=0.5, hi_=1.5), _u(n, cin, seed=7, lo_=0.0 if positive else -1.0)
    got = _simulate_conv_mfma(x, w, b, res, osc, sc, sh, 0.01)
    ref = R.conv_ref(C3, x, w, "fp32", bias=b, in_scale=sc, in_shift=sh, slope=0.01, residual=res, out_scale=osc)
    chain = R.conv_chain_fp32(cin, 27)
    assert chain == 6916
    gamma = R.gamma_fp32(chain)
    worst = R.check(got, ref, gamma, "simulated fp32 kernel")
    assert worst < gamma / 4, (worst / gamma, worst / 2.0 ** -18)


# ------------------------------------------------------------------ weight-gradient chain
def _slab_sums(terms):
    """[nsplit, L, outputs] exact float64 products -> [nsplit, outputs] fp32 slabs, one rounding per product in order"""
    acc = torch.zeros(terms.shape[0], terms.shape[2], dtype=torch.float32)
    for k in range(terms.shape[1]):
        acc = (acc.double() + terms[:, k]).float()
    return acc


def _reduce_in_slab_order(slabs):                                      # wgrad_reduce_kernel
    s = torch.zeros(slabs.shape[1], dtype=torch.float32)
    for k in range(slabs.shape[0]):
        s = s + slabs[k]
    return s


def _reduce_batched(slabs):                                            # wgrad_reduce_batched_kernel: lanes k = l, l + 4, ...
    lanes = [_reduce_in_slab_order(slabs[l::4]) if l < slabs.shape[0] else torch.zeros(slabs.shape[1]) for l in range(4)]
    return (lanes[0] + lanes[1]) + (lanes[2] + lanes[3])


@pytest.mark.parametrize("positive", [False, True])
def test_correct_fp32_wgrad_chain_passes(positive):
    """the longest weight-gradient chain of the GPU tests (3x3x3, 64^3, N = 2: 512 slabs of 4 tiles x 256 voxels), both reduces, at 256
    sampled outputs; products x * dy of the probes' operand ranges"""
    nsplit, tps, mv, outs = 512, 4, 256, 256
    lo = 0.5 if positive else -1.0
    terms = _u(nsplit, tps * mv, outs, seed=11, lo_=lo).double() * _u(nsplit, tps * mv, outs, seed=12, lo_=lo).float().double()
    terms = terms.float().double()                                     # (the products of fp32 operands are exact in float64 anyway)
    exact, A = terms.sum((0, 1)), terms.abs().sum((0, 1))
    gamma = R.gamma_fp32(R.wgrad_chain_fp32(tps, mv, nsplit))
    slabs = _slab_sums(terms)
    for red in (_reduce_in_slab_order, _reduce_batched):
        worst = R.assert_operand_exact(red(slabs), exact, A, gamma, red.__name__)
        assert worst < gamma / 4, (red.__name__, worst / gamma)
    if positive:
        # planted: one of the 512 slabs dropped (with zero-mean products a slab's sum is ~ sqrt(1024) |p| of A = 2^19 |p|: only the
        # all-positive probe sees it at this nsplit; test_planted_fp32_wgrad_defects_fail_by_30x drops a split of five in both)
        r = float(((_reduce_in_slab_order(slabs[1:]).double() - exact).abs() / A).max())
        assert r >= 30 * gamma, r / gamma


# ------------------------------------------------------------------ planted forward defects
@pytest.mark.parametrize("positive", [False, True])
def test_planted_fp32_conv_defects_fail_by_30x(positive):
    lo = 0.5 if positive else -1.0
    # <= 64 channels: one missing (channel, tap) product on the ragged last W tile, and the last input column read as zero
    n, size, c = 1, (6, 7, 40), 32
    x, w = _u(n, *size, c, seed=21, lo_=lo), _w(C3, c, c, seed=22, positive=positive)
    ref = R.conv_ref(C3, x, w, "fp32")
    gamma = R.gamma_fp32(R.conv_chain_fp32(c, 27))
    last_w0 = ((size[2] - 1) // 16) * 16
    one = ref.y.clone()
    one[:, :, :, last_w0:] -= (x[..., 5].double()[..., None] * w[:, 5, 1, 1, 1].double())[:, :, :, last_w0:]
    _fails_by(one.float(), ref, gamma)
    xz = x.clone(); xz[:, :, :, -1] = 0
    _fails_by(R.conv_ref(C3, xz, w, "fp32").y.float(), ref, gamma)
    # 256 channels: one 16-channel chunk missing (every tap) on the ragged last W tile
    n, size, c, co = 1, (3, 4, 21), 256, 16
    x, w = _u(n, *size, c, seed=23, lo_=lo), _w(C3, c, co, seed=24, positive=positive)
    ref = R.conv_ref(C3, x, w, "fp32")
    gamma = R.gamma_fp32(R.conv_chain_fp32(c, 27))
    xc = x.clone(); xc[..., 48:64] = 0
    chunk = R.conv_ref(C3, x, w, "fp32").y - R.conv_ref(C3, xc, w, "fp32").y
    bad = ref.y.clone()
    bad[:, :, :, 16:] -= chunk[:, :, :, 16:]
    _fails_by(bad.float(), ref, gamma)


def test_planted_defect_in_a_quiet_region_passes_the_old_normwise_check():
    """the motivating gap: one missing (channel, tap) product on the ragged tile of a low-magnitude region passes close(rtol=2e-5)
    against the float64 answer, and fails the elementwise bound by >= 30 gamma"""
    n, size, c = 1, (6, 7, 40), 32
    x, w = _u(n, *size, c, seed=31), _w(C3, c, c, seed=32)
    x[:, :, :, 30:] *= 2.0 ** -10                                      # a quiet region around the last (ragged) W tile
    ref = R.conv_ref(C3, x, w, "fp32")
    bad = ref.y.clone()
    bad[:, :, :, 32:] -= (x[..., 5].double()[..., None] * w[:, 5, 1, 1, 1].double())[:, :, :, 32:]
    assert _close_passes(bad.float(), ref.y)
    _fails_by(bad.float(), ref, R.gamma_fp32(R.conv_chain_fp32(c, 27)))


# ------------------------------------------------------------------ planted weight-gradient defects
def _tile_split_wave(vox, dims, tps, mtot=16):
    """(split, wave) of every output voxel under make_plan's tiling (TD x TH x 16 tiles over n, d, h, w; M-tile -> wave mt & 3)"""
    td, th = {16: (4, 4), 4: (2, 2)}[mtot]
    tiles = [-(-dims[0] // td), -(-dims[1] // th), -(-dims[2] // 16)]
    vn, vd, vh, vw = vox
    tile = ((vn * tiles[0] + vd // td) * tiles[1] + vh // th) * tiles[2] + vw // 16
    mt = (vd % td) * th + vh % th
    return tile // tps, mt % 4


@pytest.mark.parametrize("positive", [False, True])
def test_planted_fp32_wgrad_defects_fail_by_30x(positive):
    lo = 0.5 if positive else -1.0
    # the 27-tap kernel, 16 -> 8 on 20 x 4 x 13 (5 tiles, one per split): split 2 dropped
    n, size, cin, cout = 1, (20, 4, 13), 16, 8
    x, dy = _u(n, *size, cin, seed=41, lo_=lo), _u(n, *size, cout, seed=42, lo_=lo)
    sc, sh = _u(n, cin, seed=43, lo_=0.5, hi_=1.5), _u(n, cin, seed=44, lo_=0.0 if positive else -1.0)
    dw, db, aw, ab = R.wgrad_ref(C3, x, dy, "fp32", sc, sh, 0.01)
    gamma = R.gamma_fp32(R.wgrad_chain_fp32(1, 256, 5))
    drop = lambda v: _tile_split_wave(v, size, 1)[0] != 2
    dw2, db2, _, _ = R.wgrad_ref(C3, x, dy, "fp32", sc, sh, 0.01, tile_filter=drop)
    for got, ref, A in ((dw2, dw, aw), (db2, db, ab)):
        assert float(((got - ref).abs() / A).max()) >= 30 * gamma
        with pytest.raises(AssertionError):
            R.assert_operand_exact(got.float(), ref, A, gamma, "dropped split")
    # the 1-tap kernel, 32 -> 16 on 2 x 8 x 8 x 32 (16 splits x 4 wave slabs): the slab of wave 1 of split 5 counted twice
    n, size, cin, cout = 2, (8, 8, 32), 32, 16
    x, dy = _u(n, *size, cin, seed=45, lo_=lo), _u(n, *size, cout, seed=46, lo_=lo)
    dw, db, aw, ab = R.wgrad_ref(R.CONV1, x, dy, "fp32")
    gamma = R.gamma_fp32(R.wgrad_chain_fp32(1, 256, 64))

    def one_slab(v):
        s, wv = _tile_split_wave(v, size, 1)
        return (s == 5) & (wv == 1)
    extra_w, extra_b, _, _ = R.wgrad_ref(R.CONV1, x, dy, "fp32", tile_filter=one_slab)
    for got, ref, A in ((dw + extra_w, dw, aw), (db + extra_b, db, ab)):
        assert float(((got - ref).abs() / A).max()) >= 30 * gamma
        with pytest.raises(AssertionError):
            R.assert_operand_exact(got.float(), ref, A, gamma, "slab counted twice")


def test_gamma_fp32_is_tighter_than_the_worst_case_and_within_reach_of_2_18():
    """gamma_fp32 sits between the probabilistic reach of 2^-18 (lambda < 1 at the longest chain) and the worst case chain * u"""
    k = R.conv_chain_fp32(256, 27)
    assert R.gamma_fp32(k) < k * R.U32 / 8
    assert 2.0 ** -18 < R.gamma_fp32(k) < 2.0 ** -14
    assert R.conv_chain_fp32(20, 27) == 32 * 27 + 4 and R.conv_chain_fp32(4, 1) == 20
