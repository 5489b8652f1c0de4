"""Operand-exact float64 references for the bf16 conv kernels (a helper module for the tests, not a test file).

The fp32 oracle (oracle/kernel_emul.py) computes every conv on unrounded fp32 operands, so a single-bf16 kernel can only be held
to a few per cent of max|ref| against it.  This module rebuilds the operands each kernel actually multiplies -- the fp32 prologue
value act(fma(x, scale, shift)), rounded to bf16 hi (and lo) parts -- and sums their exact products in float64.  A correct kernel
then differs from the reference only by its fp32 accumulation, which is bounded elementwise by gamma * A, where A is the same
reference evaluated on |operands| (plus |bias|, |residual|, times |out_scale|): `assert_operand_exact`.

Operand forms ("mode"):
  "fp32"    exact fp32 products (the fp32 family, pw_wgrad_kernel)
  "bf16"    hi(a) * hi(b)                                   hi(v) = bf16_rne(v) of the fp32 value v
  "bf16x3"  hi(a) hi(b) + hi(a) lo(b) + lo(a) hi(b)        lo(v) = bf16_rne(v - hi(v))   (v - hi(v) is exact in fp32)

What each kernel path rounds, read from its source (csrc/):
  conv_bf16_kernel (tap table), conv16s_kernel, pw_conv_kernel, convws_kernel, the grouped launch:
      input operand  = act01(fmaf(x, scale, shift), slope) = max(h, h * slope) in fp32, rounded by v_cvt_pk_bf16_f32 (RNE),
                       split as split_bf16 (common.h); no prologue when scale is NULL and slope == 1 (data gradients);
                       zero padding is applied AFTER the activation (stage_tile_bf16).
      weights        = hi / lo of the fp32 parameter (gather_split_bf16_kernel, the same split rule).
      epilogue       = (acc + bias + residual) * out_scale (the fast epilogue never has residual and out_scale together);
                       statistics S1 = sum y, S2 = sum y^2 of the stored fp32 y; norm-backward sums (nb=) S1 = sum g,
                       S2 = sum g * h with g = y * act'(h), h = fmaf(nb_x, nb_scale, nb_shift).
  conv16s with x16= (cwf_conv with x16): the input is the bf16 image hi(dy) -- the same operand as the single-bf16 launch.
  stem and stride-2 kernels (cwf_conv with w_raw): raw fp32 weights split in the kernel by the same rule; no prologue.
  cwf_wgrad (tiled, both modes), wgrad16d / wgrad_s1d (bf16 images: hi only), the grouped launch:
      x operand as above (recomputed prologue), dy operand hi(dy) (+ lo(dy) in split mode);
      bias slot = ones . dy with the bf16 operand: sum hi(dy) (single), sum hi(dy) + lo(dy) (split).
  cwf_wgrad with dy_scale: dy operand hi(fp32(dy * s)); in split mode the compiler contracts the multiply into the
      lo-part subtraction, lo = bf16(fma(dy, s, -hi)) -- emulated here as bf16(fp32(dy * s - hi)) from an exact float64
      product (one fp32 rounding, as the fma).  The bias slot carries the same operands.
  pw_wgrad_kernel (1x1x1 / ConvTranspose weight gradients): fp32 MFMA on fp32 operands -- exact products in both bf16 modes;
      bias = sum dy.
The fp32 family (csrc/conv_mfma.hip conv_mfma_kernel, csrc/wgrad_mfma.hip wgrad_mfma_kernel + the slab reduces) multiplies the
fp32 operands themselves ("fp32" mode: exact products in float64) and is held to gamma_fp32(chain) below, not to GAMMA_CONV.
Not reproduced bit for bit: the prologue's fma is emulated in float64 and rounded once to fp32 (a double rounding can differ
from fmaf in the last fp32 bit in rare ties; the bf16 rounding after it hides that except at bf16 ties) -- covered by gamma.
"""
from __future__ import annotations

import math

import numpy as np
import torch

CONV3_S1, CONV3_S2, CONV1, CONVT2, CONV3_S2_DGRAD, CONVT2_DGRAD = range(6)
FWD_OF_DGRAD = {CONV3_S2_DGRAD: CONV3_S2, CONVT2_DGRAD: CONVT2}

GAMMA_CONV = 2.0 ** -18         # forward / data gradient: |got - ref| <= gamma * A
GAMMA_WGRAD = 2.0 ** -16        # weight gradients (K up to millions, split-K slabs + reduce)
REL_SUMS = 1e-6                 # statistics / norm-backward sums, relative to the float64 sums of |terms|

# ------------------------------------------------------------------ the fp32 family's bound
# Rounding model.  v_mfma_f32_16x16x4_f32 adds 4 products per step to an fp32 accumulator.  Whether it rounds once per step or once
# per product is not documented here, so the weaker model is assumed: every product is added with a rounding of its own (and the
# product itself may round once).  A result s = sum p_i then carries err = sum_j delta_j s_j, |delta_j| <= u = 2^-24, where the s_j
# are partial sums of the same terms, |s_j| <= A.  "chain" = the number of roundings on the longest path from a product to the
# stored result.  The worst case, chain * u * A (2^-11.2 A at 256 channels x 27 taps), would let a missing channel chunk through;
# round-to-nearest errors are mean-zero and, in the standard probabilistic model (Higham & Mary 2019), independent, so err is a sum
# of `chain` independent terms bounded by u A each and Hoeffding's inequality gives
#     P(|err| > lambda sqrt(chain) u A) <= 2 exp(-lambda^2 / 2)        lambda = 8:  2.5e-14 per result
# i.e. gamma_fp32(chain) = 8 sqrt(chain) 2^-24.  (2^-18 = GAMMA_CONV is lambda ~ 0.77 at chain 6912: at or past its limit -- a CPU
# simulation of that chain with all-positive operands reaches 1.25 x 2^-18.)
# The chains, read from the kernels:
#   forward / data gradient (conv_mfma_kernel): one register accumulator per (output voxel, channel), never split across waves; the
#       channel-chunk loop (ceil(C/16) chunks of 16 input channels) x the tap loop (ntaps of the output's class: 27, 8 (ConvTranspose
#       data gradient), 1..8 (stride-2 data-gradient parity classes), 1) x 4 MFMAs x 4 products -- 16 ceil(C/16) ntaps products --
#       then the epilogue's + bias, + residual, * out_scale (3), plus the product's own rounding (1): conv_chain_fp32.  C is the
#       launch's input channel count (the forward's Cout for a data gradient).  256 channels x 27 taps: chain 6916, gamma 2^-14.6.
#   weight gradient (wgrad_mfma_kernel): one accumulator per (tap, ci, co) and slab over the voxels of `tiles per split` spatial
#       tiles of TD x TH x 16 voxels (the 27-tap kernel: every voxel of a tile through one wave; the 1-tap kernel: a quarter of the
#       M-tiles per wave, each wave its own slab -- shorter), then the reduce of the nsplit slabs: four lanes of
#       stride 4 combined as (l0 + l1) + (l2 + l3) (wgrad_reduce_kernel and wgrad_reduce_batched_kernel alike), at most
#       nsplit + 1 roundings; plus the product's own: wgrad_chain_fp32.
#   statistics: per-thread fp32 sums of at most 16 stored values, shuffles, f64 across waves: REL_SUMS, as for the bf16 kernels.
#       (This describes the sums fused into the conv epilogues only.  in_reduce_kernel of csrc/norm.hip adds up to 256 values per
#       thread at 1024 channels; it is held to norm_ref.sum_rel(L) with L read from its launch rule, not to REL_SUMS.)
U32 = 2.0 ** -24
LAMBDA_FP32 = 8.0


def gamma_fp32(chain):
    """elementwise bound |got - ref| <= gamma * A of an fp32-family result whose longest rounding chain is `chain` (see above)"""
    return LAMBDA_FP32 * math.sqrt(chain) * U32


def conv_chain_fp32(c, ntaps):
    """the chain of conv_mfma_kernel with c input channels (of the launch) and ntaps taps per output"""
    return 16 * (-(-c // 16)) * ntaps + 4


def wgrad_chain_fp32(tiles_per_split, tile_voxels, nsplit):
    """the chain of wgrad_mfma_kernel + either reduce: tiles_per_split tiles of tile_voxels voxels per slab, nsplit slabs"""
    return tiles_per_split * tile_voxels + nsplit + 2


# ------------------------------------------------------------------ operand rounding
def hi(v):
    """bf16 round-to-nearest-even of the fp32 value v (v_cvt_pk_bf16_f32), as float64"""
    return v.float().to(torch.bfloat16).double()


def lo(v):
    """bf16_rne(v - hi(v)) (split_bf16, common.h); v - hi(v) is exact in fp32"""
    v = v.float()
    return (v - v.to(torch.bfloat16).float()).to(torch.bfloat16).double()


def hi_trunc(v):
    """truncating fp32 -> bf16 conversion (a defect the tests must see, not a kernel rule)"""
    b = v.float().contiguous().view(torch.int32) & ~0xFFFF
    return b.view(torch.float32).double()


def prologue(x, scale=None, shift=None, slope=1.0):
    """fp32 act01(fmaf(x, scale, shift), slope) per (sample, channel): the fma in float64, rounded once to fp32, then
    max(h, h * slope) in fp32.  scale None and slope 1: x itself (data gradients)."""
    x = x.float()
    if scale is not None:
        h = (x.double() * scale.double()[:, None, None, None, :] + shift.double()[:, None, None, None, :]).float()
    else:
        h = x
    if scale is not None or slope != 1.0:
        h = torch.maximum(h, h * torch.tensor(slope, dtype=torch.float32))
    return h


def split_terms(a, b, mode, hi_fn=hi):
    """[(a_part, b_part), ...] whose product sum is the kernel's product of a and b in `mode` (a, b fp32 tensors)"""
    if mode == "fp32":
        return [(a.double(), b.double())]
    if mode == "bf16":
        return [(hi_fn(a), hi_fn(b))]
    if mode == "bf16x3":
        ha, hb = hi_fn(a), hi_fn(b)
        la, lb = (a.double() - ha).float().to(torch.bfloat16).double(), (b.double() - hb).float().to(torch.bfloat16).double()
        return [(ha, hb + lb), (la, hb)]                 # ha.hb + ha.lb + la.hb (exact in float64 up to 2^-53 per sum)
    raise ValueError(mode)


# ------------------------------------------------------------------ gather form of every op
def _dim_table(op, dgrad, n_out, n_in):
    """src[o, k]: the input coordinate that output coordinate o reads through kernel tap k along one dimension (n_in = padding)"""
    o = np.arange(n_out)[:, None]
    if op in (CONV3_S1, CONV3_S2):
        k = np.arange(3)[None, :]
        s = 1 if op == CONV3_S1 else 2
        if not dgrad:
            src, ok = s * o + k - 1, np.ones((n_out, 3), bool)
        else:                                            # dx[i] += dy[(i + 1 - k) / s] w[k]
            t = o + 1 - k
            src, ok = t // s, (t % s) == 0
    elif op == CONV1:
        k = np.zeros((1, 1), int)
        src, ok = o + k, np.ones((n_out, 1), bool)
    elif op == CONVT2:
        k = np.arange(2)[None, :]
        if not dgrad:                                    # y[2i + k] = x[i] w[k]
            t = o - k
            src, ok = t // 2, (t % 2) == 0
        else:                                            # dx[i] = sum_k dy[2i + k] w[k]
            src, ok = 2 * o + k, np.ones((n_out, 2), bool)
    else:
        raise ValueError(op)
    ok = ok & (src >= 0) & (src < n_in)
    return torch.from_numpy(np.where(ok, src, n_in).astype(np.int64))


def _weight_matrix(op, w, dgrad):
    """[T, C_in_of_this_launch, C_out_of_this_launch] from the parameter layout"""
    w = w.double()
    if op == CONVT2:                                     # (cin, cout, 2, 2, 2)
        t = w.permute(2, 3, 4, 0, 1)                      # [kd, kh, kw, cin, cout]
    else:                                                # (cout, cin, k, k, k)
        t = w.permute(2, 3, 4, 1, 0)                      # [kd, kh, kw, cin, cout]
    t = t.reshape(-1, t.shape[3], t.shape[4])
    return t.transpose(1, 2).contiguous() if dgrad else t.contiguous()


def _gather(inp, tabs, vox, chunk_rows):
    """yields (row slice, patches [rows, T * C]) of inp [N, D, H, W, C] (f64) for the output voxels vox = (n, od, oh, ow)"""
    n_, d_, h_, w_, c = inp.shape
    pad = torch.zeros((n_, d_ + 1, h_ + 1, w_ + 1, c), dtype=inp.dtype)
    pad[:, :d_, :h_, :w_] = inp
    vn, vd, vh, vw = vox
    for s in range(0, vn.numel(), chunk_rows):
        e = min(vn.numel(), s + chunk_rows)
        td, th, tw = tabs[0][vd[s:e]], tabs[1][vh[s:e]], tabs[2][vw[s:e]]
        p = pad[vn[s:e, None, None, None], td[:, :, None, None], th[:, None, :, None], tw[:, None, None, :]]
        yield slice(s, e), p.reshape(e - s, -1)


def _all_voxels(n, dims):
    g = torch.meshgrid(torch.arange(n), torch.arange(dims[0]), torch.arange(dims[1]), torch.arange(dims[2]), indexing="ij")
    return tuple(t.reshape(-1) for t in g)


def _chunk(tc):
    return max(64, (1 << 22) // max(1, tc))


class Ref:
    """y (reference), A (magnitude companion); both [N, Do, Ho, Wo, Co] float64, or [V, Co] at sampled voxels `vox`"""

    def __init__(self, y, A, vox=None):
        self.y, self.A, self.vox = y, A, vox

    def pick(self, got):
        """the kernel output at the reference's voxels (channels [0, Co))"""
        got = got.detach().cpu().double()[..., :self.y.shape[-1]]
        if self.vox is None:
            return got
        return got[self.vox]


def conv_ref(op, x, w, mode, bias=None, in_scale=None, in_shift=None, slope=1.0, residual=None, out_scale=None,
             dgrad=False, out_size=None, vox=None, hi_fn=hi, tap_filter=None):
    """Forward (dgrad False) or data gradient (dgrad True: x = dy, op = the forward op, out_size = the forward input's extent)
    of op in operand form `mode`, with the kernels' prologue and epilogue.  vox: (n, d, h, w) index tensors of the outputs to
    compute (None = all).  tap_filter(vox, t) -> bool mask [rows] of (voxel, tap) products to keep (defect emulation only)."""
    n, di, hi_, wi, _ = x.shape
    if not dgrad:
        dims = {CONV3_S1: (di, hi_, wi), CONV1: (di, hi_, wi), CONV3_S2: ((di - 1) // 2 + 1, (hi_ - 1) // 2 + 1, (wi - 1) // 2 + 1),
                CONVT2: (2 * di, 2 * hi_, 2 * wi)}[op]
    else:
        dims = tuple(out_size)
    tabs = [_dim_table(op, dgrad, dims[i], (di, hi_, wi)[i]) for i in range(3)]
    W = _weight_matrix(op, w, dgrad)
    T, C, Co = W.shape
    xa = prologue(x[..., :C], in_scale, in_shift, slope)
    full = vox is None
    if full:
        vox = _all_voxels(n, dims)
    rows = vox[0].numel()
    y = torch.zeros(rows, Co, dtype=torch.float64)
    A = torch.zeros(rows, Co, dtype=torch.float64)
    Wf = W.float()
    for xp, wp in split_terms(xa, Wf, mode, hi_fn) + [("abs", None)]:
        src = xa.double().abs() if xp == "abs" else xp
        wm = (Wf.double().abs() if xp == "abs" else wp).reshape(T * C, Co)
        for sl, p in _gather(src, tabs, vox, _chunk(T * C)):
            if tap_filter is not None and xp != "abs":
                keep = torch.stack([tap_filter(tuple(v[sl] for v in vox), t) for t in range(T)], 1)      # [rows, T]
                p = (p.view(-1, T, C) * keep[:, :, None]).reshape(-1, T * C)
            if xp == "abs":
                A[sl] += p @ wm
            else:
                y[sl] += p @ wm

    def at(t):                                           # per-voxel operand [rows, Co] from a [N, D, H, W, Co] tensor
        return t.double()[..., :Co][vox]
    if bias is not None:
        y += bias.double()[None, :Co]
        A += bias.double().abs()[None, :Co]
    if residual is not None:
        y += at(residual)
        A += at(residual).abs()
    if out_scale is not None:
        s = out_scale.double()[vox[0], :Co]
        y *= s
        A *= s.abs()
    if full:
        y, A = y.view(n, *dims, Co), A.view(n, *dims, Co)
        return Ref(y, A)
    return Ref(y, A, vox)


def wgrad_operand_mode(op, cin, cout, size, mode):
    """the operand form of the weight-gradient kernel cwf_wgrad runs for op (cin -> cout) on a forward input of extent
    size (D, H, W) -- a copy of the pointwise conditions of wgrad_tensor_plan, csrc/wgrad_bf16.hip, for the CPU reference tests;
    tests/test_wgrad_bf16_plan_cpu.py holds it to the library's own answer: pw_wgrad_kernel (exact fp32 products in both bf16
    modes) for 1x1x1 layers with D*H*W % 4 == 0 and (16-channel chunks, 16-channel tiles) in {(1, 1), (2, 1), (4, 2), (8, 4)}, and
    for ConvTranspose layers with D*H*W % 4 == 0, W % 4 == 0 and (chunks, tiles) in {(1, 1), (2, 2)}; the bf16 tiled / persistent
    kernels otherwise"""
    d, h, w = size
    shape = (-(-cin // 16), -(-cout // 16))
    if op == CONV1 and (d * h * w) % 4 == 0 and shape in ((1, 1), (2, 1), (4, 2), (8, 4)):
        return "fp32"
    if op == CONVT2 and (d * h * w) % 4 == 0 and w % 4 == 0 and shape in ((1, 1), (2, 2)):
        return "fp32"
    return mode


def wgrad_ref(op, x, dy, mode, in_scale=None, in_shift=None, slope=1.0, dy_scale=None, hi_fn=hi, tile_filter=None):
    """(dW in the parameter layout, db, A_dW, A_db) of op in operand form `mode` with the recomputed prologue and the dy_scale fold.
    tile_filter(vox) -> bool mask [rows] of output voxels whose products count (defect emulation only)."""
    n, di, hi_, wi, cin = x.shape
    _, do, ho, wo, cout = dy.shape
    tabs = [_dim_table(op, False, (do, ho, wo)[i], (di, hi_, wi)[i]) for i in range(3)]
    T = tabs[0].shape[1] * tabs[1].shape[1] * tabs[2].shape[1]
    xa = prologue(x, in_scale, in_shift, slope)
    dyf = dy.float()
    if dy_scale is not None:
        prod = dy.double() * dy_scale.double()[:, None, None, None, :]
        g = prod.float()
    vox = _all_voxels(n, (do, ho, wo))
    keep = None if tile_filter is None else tile_filter(vox).double()[:, None]
    if mode == "fp32":
        terms = [(xa.double(), dyf.double())]
        bias_terms = dyf.double()
    else:
        if dy_scale is None:
            dh = hi_fn(dyf)
            dl = lo(dyf) if hi_fn is hi else (dyf.double() - dh).float().to(torch.bfloat16).double()
        else:
            dh = hi_fn(g)
            dl = (prod - dh).float().to(torch.bfloat16).double()            # bf16(fma(dy, s, -hi)): one fp32 rounding of the exact value
        xh = hi_fn(xa)
        if mode == "bf16":
            terms, bias_terms = [(xh, dh)], dh
        else:
            xl = (xa.double() - xh).float().to(torch.bfloat16).double()
            terms, bias_terms = [(xh, dh + dl), (xl, dh)], dh + dl
    dyabs = (g if dy_scale is not None else dyf).double().abs()
    dW = torch.zeros(T * cin, cout, dtype=torch.float64)
    AW = torch.zeros(T * cin, cout, dtype=torch.float64)
    for src, d in terms + [("abs", None)]:
        s_ = xa.double().abs() if src == "abs" else src
        dd = (dyabs if src == "abs" else d).reshape(-1, cout)
        for sl, p in _gather(s_, tabs, vox, _chunk(T * cin)):
            dv = dd[sl] if keep is None or src == "abs" else dd[sl] * keep[sl]
            if src == "abs":
                AW += p.t() @ dv
            else:
                dW += p.t() @ dv
    bt = bias_terms.reshape(-1, cout)
    db = (bt if keep is None else bt * keep).sum(0)
    Ab = dyabs.reshape(-1, cout).sum(0)

    def layout(m):                                       # [T * cin, cout] -> parameter layout
        m = m.view(tabs[0].shape[1], tabs[1].shape[1], tabs[2].shape[1], cin, cout)
        if op == CONVT2:
            return m.permute(3, 4, 0, 1, 2).contiguous()          # (cin, cout, 2, 2, 2)
        return m.permute(4, 3, 0, 1, 2).contiguous()              # (cout, cin, k, k, k)
    return layout(dW), db, layout(AW), Ab


# ------------------------------------------------------------------ sums
def stats_ref(y):
    """f64 InstanceNorm statistics [N, C, 2] (S1 = sum y, S2 = sum y^2) of y [N, D, H, W, C]"""
    y = y.double()
    return torch.stack([y.sum((1, 2, 3)), (y * y).sum((1, 2, 3))], -1)


def assert_stats(got, ref: Ref, gamma, what):
    """statistics of the kernel's output against those of the reference: the elementwise bound propagated (S1: gamma sum A,
    S2: gamma sum (2|y| + gamma A) A) plus REL_SUMS of the float64 sums of |terms| (fp32 partial sums)"""
    assert ref.vox is None
    y, A = ref.y, ref.A
    got = got.detach().cpu().double()
    st = stats_ref(y)
    b1 = gamma * A.sum((1, 2, 3)) + REL_SUMS * y.abs().sum((1, 2, 3))
    b2 = gamma * ((2 * y.abs() + gamma * A) * A).sum((1, 2, 3)) + REL_SUMS * (y * y).sum((1, 2, 3))
    bound = torch.stack([b1, b2], -1) + 1e-30
    r = (got - st).abs() / bound
    assert float(r.max()) <= 1.0, (what, "stats", float(r.max()), np.unravel_index(int(r.argmax()), r.shape))
    return float(r.max())


def nb_sums_ref(g: Ref, nb_x, nb_scale, nb_shift, nb_slope):
    """the fused norm-backward sums [N, C, 2]: S1 = sum gn, S2 = sum gn * h, gn = y * act'(h), h = fmaf(nb_x, scale, shift); with
    the bound terms (sum A |act'|, sum A |act' h|) for the kernel's error."""
    C = g.y.shape[-1]
    h = prologue(nb_x[..., :C], nb_scale, nb_shift, 1.0).double()
    da = torch.where(h > 0, torch.ones_like(h), torch.full_like(h, float(nb_slope)))
    gn = g.y * da
    s = torch.stack([gn.sum((1, 2, 3)), (gn * h).sum((1, 2, 3))], -1)
    a = torch.stack([(g.A * da.abs()).sum((1, 2, 3)), (g.A * (da * h).abs()).sum((1, 2, 3))], -1)
    t = torch.stack([gn.abs().sum((1, 2, 3)), (gn * h).abs().sum((1, 2, 3))], -1)
    return s, a, t


def assert_nb_sums(got, g: Ref, nb, gamma, what):
    s, a, t = nb_sums_ref(g, *nb)
    bound = gamma * a + REL_SUMS * t + 1e-30
    r = (got.detach().cpu().double() - s).abs() / bound
    assert float(r.max()) <= 1.0, (what, "nb sums", float(r.max()), np.unravel_index(int(r.argmax()), r.shape))
    return float(r.max())


# ------------------------------------------------------------------ the check
def err_over_A(got, ref, A):
    got = got.detach().cpu().double()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert bool(torch.isfinite(got).all()), "non-finite output"
    return (got - ref).abs() / A.clamp_min(1e-300)


def assert_operand_exact(got, ref, A, gamma, what):
    """|got - ref| <= gamma * A elementwise (where A == 0, got must equal ref exactly); returns the worst err / A"""
    got = got.detach().cpu().double()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    err = (got - ref).abs()
    zero = A == 0
    assert bool(torch.isfinite(got).all()), (what, "non-finite output")
    bad_zero = zero & (err > 0)
    assert not bool(bad_zero.any()), (what, "non-zero where every product is zero", tuple(int(i) for i in bad_zero.nonzero()[0]))
    r = torch.where(zero, torch.zeros_like(err), err / A.clamp_min(1e-300))
    worst = float(r.max()) if r.numel() else 0.0
    idx = tuple(int(i) for i in np.unravel_index(int(r.argmax()), r.shape)) if r.numel() else ()
    assert worst <= gamma, (what, "worst err/A = %.3e (%.1f x gamma) at %s: got %r ref %r" %
                            (worst, worst / gamma, idx, float(got[idx]) if idx else None, float(ref[idx]) if idx else None))
    return worst


def check(got, ref: Ref, gamma, what):
    return assert_operand_exact(ref.pick(got), ref.y, ref.A, gamma, what)


# ------------------------------------------------------------------ sampling for large layers
def edge_voxels(n, dims, tile=(4, 4, 16), n_random=2048, seed=0):
    """(n, d, h, w) index tensors: every voxel of the last tile in each dimension, every face voxel, and a seeded random
    interior sample, in every sample n"""
    D, H, W = dims
    d, h, w = torch.meshgrid(torch.arange(D), torch.arange(H), torch.arange(W), indexing="ij")
    last = [((s - 1) // t) * t for s, t in zip(dims, tile)]
    m = (d >= last[0]) | (h >= last[1]) | (w >= last[2]) | (d == 0) | (h == 0) | (w == 0) | (d == D - 1) | (h == H - 1) | (w == W - 1)
    g = torch.Generator().manual_seed(seed)
    flat = m.reshape(-1).clone()
    flat[torch.randint(0, flat.numel(), (n_random,), generator=g)] = True
    idx = flat.nonzero()[:, 0]
    vd, vh, vw = idx // (H * W), (idx // W) % H, idx % W
    vn = torch.arange(n).repeat_interleave(idx.numel())
    return vn, vd.repeat(n), vh.repeat(n), vw.repeat(n)
