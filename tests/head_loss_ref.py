"""Float64 reference for the supervision heads and their losses (a helper module for the tests, not a test file).

The chain: low-resolution logits [N, d, h, w, ldc] (channels 0..C-1 used) -> trilinear upsample by `scale`
(align_corners=False) -> C-class softmax -> per (map, n, c) sums -> Dice + weighted CE -> dLoss/dp -> logit gradient.
Everything here is written from the formulas, in float64, and runs on whatever device its inputs live on.

Formulas
  source index (PyTorch's rule, restated at the top of csrc/heads.hip): src = max((o + 0.5) / s - 0.5, 0),
      i0 = min(floor(src), n - 1), i1 = min(i0 + 1, n - 1), l1 = src - i0; weights (1 - l1, l1).
      Upsampling is three 1-D interpolation matrices applied along D, H, W; its adjoint is their transposes.
  labels: C = 4: class = label; C = 2: class = (posmask >> label) & 1 (utils.tools.REGION_MASKS / EDGE_MASKS).
  sums[n, c] = (I, P, T, S) = (sum p t, sum p, sum t, sum t log clamp(p, lo, 1)), lo = fp32(0.005) = 0.004999999888...:
      the kernels compare fp32 probabilities with the fp32 constant 0.005f, as torch.clamp does on fp32 tensors.
  dice_ce_finalize_kernel: den_c = P_c + T_c + 1e-7 over the batch; loss = 1 - (1/C) sum_c 2 I_c / den_c
      + (1/(N V)) sum_{n,c} -w_c[n] S_c[n], w_c[n] = 1 - T_c[n] / sum_k T_k[n]  (Dice on batch sums, CE weights per sample);
      coef[n, c] = (a = -(2/C)/den_c, b = (2/C) I_c/den_c^2, k = -w_c[n]/(N V), 0).
  dLoss/dp_c = b_c + t_c (a_c + k_c / p_c * [lo <= p_c <= 1])  (torch.clamp passes the gradient on the closed interval);
      the logit gradient is float64 autograd of gscale * sum (a t p + b p + k t log clamp(p)) with the given coefficients,
      which equals autograd of the loss itself when the coefficients are the exact ones (tests/test_head_loss_ref_cpu.py).

Which kernel computes what (csrc/heads.hip, csrc/loss.hip)
  upsample_softmax_kernel (cwf_upsample_softmax): the eight-corner form, wgt = wd * wh * ww, val += wgt * l; expf; 1.f / sum.
  head_loss_sums_kernel, head_loss_bwd_rows_kernel (cwf_head_loss_*): the separable form, a D/H lerp per row into LDS
      (hl_build_rows) then a W lerp per voxel (hl_prob); __expf = v_exp_f32(log2e * x); __frcp_rn. fp32 per-thread partials,
      a 64-lane wave_sum, four waves added in f64, one f64 atomic per block.  The backward evaluates the clamp gate on its
      own fp32 p and finishes the adjoint in two passes (rows: H then W in LDS; planes: D).
  upsample_softmax_bwd_{rows,planes}_kernel: the same adjoint from a stored p and dprob.
  channel_softmax(_bwd)_kernel: the 4-class decoder softmax and its adjoint, pointwise.
  dice_ce_sums_kernel: per-thread fp32 partials over vox_per_block / 256 voxels, then as above; logf.
  dice_ce_finalize_kernel: float64 from the f64 sums, each output rounded once to fp32; total = fp32 sum of the map losses.
  dice_ce_bwd_kernel: g = gs * (b + a + k / p) in fp32, gated on the fp32 p.

Error model: |got - ref| <= gamma * A elementwise, u = 2^-24 (fp32 unit roundoff).  Scales are powers of two, so every source
index, lerp weight and product of weights is exact in fp32; only products with logits and additions round.
  q = 1 + M per high-resolution voxel, M = max_c sum_i w_i |l_ic| (the interpolation of |logit|; max_c |l_c| unfused).
  Probabilities, |dp_c| <= GAMMA_P * p_c * q:
      lerp rounding: at most 8 roundings per product term in either form -> |dv_c| <= 8u M; in x_c = v_c - max_k v_k it
      enters twice (16u M) and the subtraction adds u |x_c| <= 2u M.  v_exp_f32 (documented 1 ulp: 2u relative) on
      fl(log2e) * x (argument relative error 2u -> 2u |x| <= 4u M relative in the result); the expf of the unfused kernels is
      within the same 1 ulp.  rel(e_c) <= 22u M + 2u; the sum of C <= 4 positive terms adds 3u; v_rcp_f32 1 ulp (2u), the
      product u: rel(p_c) <= 2 (22u M + 2u) + 6u = 44u M + 10u <= 48u q.
  Sums (gamma_sums), A = (sum t p q, sum p q, sum t, sum t (q + |log clamp p|)): the probability error GAMMA_P q per term, the
      logarithm's ulp (2u |log|), and the fp32 partials: a thread adds k terms (each addition at most u of the running |sum|),
      the wave tree 6 levels, the f64 tail 1u.  T is a count below 2^24 and is exact.
  Logit gradients (gamma_grad), A = adjoint(q (p_c G_c + p_c sum_k p_k G_k)), G_c = |gs| (|b_c| + t_c (|a_c| + gate |k_c| / p_c))
      the magnitude of dLoss/dp_c's parts: p enters three times (3 GAMMA_P q), g's four fp32 operations 4u, the dot C u,
      g - dot, the product and the row weight 3u, and each of the three adjoint sums over 2 * scale high-resolution
      indices (2 scale + 1)u.  Where the kernel's fp32 p may fall on the other side of lo than the exact one
      (|p_c - lo| <= GAMMA_P q p_c), either branch of the gate is accepted: the bound gains the adjoint of
      p_c |gs k_c / p_c| (1 + p_c) there.  Coefficient errors from upstream sums (the Python route) enter the same way.
  From stored fp32 inputs (the unfused adjoints and dice_ce_bwd) the inputs are exact and only the listed arithmetic remains.
"""
from __future__ import annotations

import math

import numpy as np
import torch
import torch.nn.functional as F

U = 2.0 ** -24
CLAMP_LO = float(np.float32(0.005))
HL_ROWS, HL_GROUPS = 8, 4                # csrc/heads.hip: rows per LDS row table, row groups per block of head_loss_sums_kernel
GAMMA_P = 48 * U
GAMMA_FIN = 2 * U                        # a float64 value rounded once to fp32 (the float64 arithmetic before it: < 2^-40)


def gamma_sums(terms_per_thread, from_logits=True):
    return (GAMMA_P if from_logits else 0.0) + (terms_per_thread + 6 + 1 + 2) * U


def fused_terms_per_thread(Wo):
    """head_loss_sums_kernel: 256 threads stride over HL_ROWS rows of Wo voxels, HL_GROUPS groups per block"""
    return HL_GROUPS * -(-HL_ROWS * Wo // 256)


def unfused_terms_per_thread(N, V):
    """dice_ce_sums_kernel: vox_per_block = clamp(ceil(N V / 2048), 1024, V), 256 threads"""
    vpb = min(max(-(-N * V // 2048), 1024), V)
    return -(-vpb // 256)


def gamma_grad(C, scale, from_logits=True):
    adj = 3 * (2 * scale + 1) if scale > 1 else 0
    return (3 * GAMMA_P if from_logits else 0.0) + (4 + C + 3 + adj) * U


def gamma_softmax_bwd(C, scale):
    """cwf_upsample_softmax_bwd / cwf_channel_softmax_bwd (scale 1) from stored p, dprob: dot, g - dot, two products, the sums"""
    return (C + 3 + (3 * (2 * scale + 1) if scale > 1 else 0)) * U


GAMMA_DPROB = 4 * U                      # dice_ce_bwd_kernel: k / p, two additions, gs *


# ------------------------------------------------------------------ upsampling
def axis_matrix(n_in, scale, device="cpu"):
    """[n_in * scale, n_in] float64: row o holds the two lerp weights of output index o (PyTorch's source-index rule)"""
    o = torch.arange(n_in * scale, dtype=torch.float64, device=device)
    src = ((o + 0.5) / scale - 0.5).clamp_min(0.0)
    i0 = src.floor().clamp_max(n_in - 1)
    l1 = src - i0
    i0 = i0.long()
    i1 = (i0 + 1).clamp_max(n_in - 1)
    M = torch.zeros(n_in * scale, n_in, dtype=torch.float64, device=device)
    M.index_put_((torch.arange(len(o), device=device), i0), 1.0 - l1, accumulate=True)
    M.index_put_((torch.arange(len(o), device=device), i1), l1, accumulate=True)
    return M


def axis_matrices(lo_dims, scale, device="cpu"):
    return tuple(axis_matrix(n, scale, device) for n in lo_dims)


def interp(x, mats):
    """x [N, d, h, w, C] -> [N, D, H, W, C] = sum Md Mh Mw x (mats None: identity, the unfused 4-class softmax)"""
    if mats is None:
        return x
    Md, Mh, Mw = mats
    x = torch.einsum("ai,nijkc->najkc", Md, x)
    x = torch.einsum("bj,najkc->nabkc", Mh, x)
    return torch.einsum("ck,nabkz->nabcz", Mw, x)


def interp_adjoint(y, mats):
    if mats is None:
        return y
    Md, Mh, Mw = mats
    y = torch.einsum("ck,nabcz->nabkz", Mw, y)
    y = torch.einsum("bj,nabkc->najkc", Mh, y)
    return torch.einsum("ai,najkc->nijkc", Md, y)


def probs(logit, C, mats, exp=torch.exp, rcp=torch.reciprocal):
    """float64 p [N, D, H, W, C] and q = 1 + max_c interp(|logit_c|) [N, D, H, W, 1] (exp / rcp: for planted defects only)"""
    lg = logit[..., :C].double()
    v = interp(lg, mats)
    q = 1.0 + interp(lg.abs(), mats).amax(-1, keepdim=True)
    e = exp(v - v.amax(-1, keepdim=True))
    return e * rcp(e.sum(-1, keepdim=True)), q


# ------------------------------------------------------------------ labels, sums, finalize
def target(label, C, posmask=0):
    """one-hot [N, D, H, W, C] float64 of the class each kernel decodes from the label"""
    label = label.long()
    cls = label if C == 4 else torch.bitwise_right_shift(torch.full_like(label, int(posmask)), label) & 1
    return F.one_hot(cls, C).double()


def clamped(p, lo=CLAMP_LO):
    return p.clamp(lo, 1.0)


def sums(p, t, q=None):
    """(S, A) [N, C, 4]: (sum p t, sum p, sum t, sum t log clamp p) and the magnitude companion
    (sum t p q, sum p q, sum t, sum t (q + |log clamp p|)); q None: p is an exact input (unfused sums)"""
    if q is None:
        q = torch.ones_like(p[..., :1])
    r = tuple(range(1, p.dim() - 1))
    lg = torch.log(clamped(p))
    S = torch.stack([(p * t).sum(r), p.sum(r), t.sum(r), (t * lg).sum(r)], -1)
    A = torch.stack([(p * t * q).sum(r), (p * q).sum(r), t.sum(r), (t * (q + lg.abs())).sum(r)], -1)
    return S, A


def finalize(S, V):
    """S [N, C, 4] float64 -> (loss, coef [N, C, 4], A_loss): dice_ce_finalize_kernel's formulas in float64"""
    N, C = S.shape[0], S.shape[1]
    I, P, T = S[..., 0].sum(0), S[..., 1].sum(0), S[..., 2].sum(0)
    den = P + T + 1e-7
    dice = (2.0 * I / den).sum()
    w = 1.0 - S[..., 2] / S[..., 2].sum(1, keepdim=True)
    ce = (-w * S[..., 3]).sum()
    loss = (1.0 - dice / C) + ce / (N * V)
    coef = torch.zeros_like(S)
    coef[..., 0] = (-(2.0 / C) / den).expand(N, C)
    coef[..., 1] = ((2.0 / C) * I / (den * den)).expand(N, C)
    coef[..., 2] = -w / (N * V)
    A_loss = 1.0 + dice / C + ce.abs() / (N * V)
    return loss, coef, A_loss


def coef_error(S, A_S, gamma_s, coef):
    """bound on |coef(kernel sums) - coef(exact sums)| from |dS| <= gamma_s A_S (T exact, so k is exact up to its rounding)"""
    I, P, T = S[..., 0].sum(0), S[..., 1].sum(0), S[..., 2].sum(0)
    dI, dP = gamma_s * A_S[..., 0].sum(0), gamma_s * A_S[..., 1].sum(0)
    den = P + T + 1e-7
    e = torch.zeros_like(coef)
    e[..., 0] = coef[..., 0].abs() * (dP / den + GAMMA_FIN)
    e[..., 1] = (2.0 / S.shape[1]) * (dI + 2 * I * dP / den) / den ** 2 + coef[..., 1].abs() * GAMMA_FIN
    e[..., 2] = coef[..., 2].abs() * GAMMA_FIN
    return e


# ------------------------------------------------------------------ dLoss/dp and the logit gradient
def _per_voxel(coef, n_shape):
    """coef [N, C, 4] -> (a, b, k) broadcastable to [N, D, H, W, C]"""
    c = coef.double().reshape(coef.shape[0], 1, 1, 1, coef.shape[1], coef.shape[2])
    return c[..., 0], c[..., 1], c[..., 2]


def dprob(p, t, coef, gscale, lo=CLAMP_LO):
    """(g, G): dLoss/dp scaled by gscale with the gate on [lo, 1], and |gs| times the sum of |parts|"""
    a, b, k = _per_voxel(coef, p.shape)
    gate = (p >= lo) & (p <= 1.0)
    kp = torch.where(gate, k / torch.where(gate, p, torch.ones_like(p)), torch.zeros_like(p))
    g = gscale * (b + t * (a + kp))
    G = abs(gscale) * (b.abs() + t * (a.abs() + kp.abs()))
    return g, G


def softmax_adjoint(p, g):
    return p * (g - (p * g).sum(-1, keepdim=True))


def softmax_adjoint_mag(p, G):
    return p * G + p * (p * G).sum(-1, keepdim=True)


def logit_grad(logit, C, mats, label_t, coef, gscale, keep=None, p_override=None):
    """float64 autograd of gscale * sum(a t p + b p + k t log clamp p) w.r.t. the logits [N, d, h, w, C]
    (keep: a 0/1 mask on high-resolution voxels, p_override: a defective p function -- planted defects only)"""
    lg = logit[..., :C].detach().double().requires_grad_(True)
    v = interp(lg, mats)
    p = torch.softmax(v, -1) if p_override is None else p_override(v)
    a, b, k = _per_voxel(coef, p.shape)
    surr = a * label_t * p + b * p + k * label_t * torch.log(clamped(p))
    if keep is not None:
        surr = surr * keep
    (gscale * surr.sum()).backward()
    return lg.grad


def logit_grad_bound(logit, C, mats, label_t, coef, gscale, scale, coef_err=None):
    """absolute elementwise bound on the kernel's logit gradient: gamma_grad * A plus the gate-ambiguity and coefficient terms"""
    with torch.no_grad():
        p, q = probs(logit, C, mats)
        g, G = dprob(p, label_t, coef, gscale)
        A = interp_adjoint(q * softmax_adjoint_mag(p, G), mats)
        a, b, k = _per_voxel(coef, p.shape)
        amb = ((p - CLAMP_LO).abs() <= GAMMA_P * q * p).double() * label_t
        extra = amb * abs(gscale) * k.abs() / p                         # |dg| where the gate may flip
        if coef_err is not None:
            ea, eb, ek = _per_voxel(coef_err, p.shape)
            extra = extra + abs(gscale) * (eb + label_t * (ea + ek / clamped(p)))
        E = interp_adjoint(softmax_adjoint_mag(p, extra), mats)
        return gamma_grad(C, scale) * A + E, A


# ------------------------------------------------------------------ the check
def worst(got, ref, bound, what, limit=1.0):
    """max |got - ref| / bound (where the bound is 0, got must equal ref); asserts <= limit and returns it"""
    got = got.detach().cpu().double()
    ref, bound = ref.detach().cpu().double(), bound.detach().cpu().double()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert bool(torch.isfinite(got).all()), (what, "non-finite output")
    err = (got - ref).abs()
    zero = bound == 0
    assert not bool((zero & (err > 0)).any()), (what, "differs where the reference is exact")
    r = torch.where(zero, torch.zeros_like(err), err / bound.clamp_min(1e-300))
    w = float(r.max()) if r.numel() else 0.0
    if w > limit:
        idx = tuple(int(i) for i in np.unravel_index(int(r.argmax()), r.shape))
        raise AssertionError("%s: worst err/bound = %.3g at %s: got %r ref %r bound %r" % (
            what, w, idx, float(got[idx]), float(ref[idx]), float(bound[idx])))
    return w


def old_bound_fails(got, ref, rtol=1e-4):
    """the suite's earlier check: |got - ref| <= rtol * max|ref|"""
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    return float((got - ref).abs().max()) > rtol * float(ref.abs().max())



def loss_error(S, A_S, gamma_s, V):
    """bound on |loss(kernel sums) - loss(exact sums)| from |dS| <= gamma_s A_S, plus the fp32 rounding of the loss"""
    N, C = S.shape[0], S.shape[1]
    I, P, T = S[..., 0].sum(0), S[..., 1].sum(0), S[..., 2].sum(0)
    dI, dP = gamma_s * A_S[..., 0].sum(0), gamma_s * A_S[..., 1].sum(0)
    den = P + T + 1e-7
    w = 1.0 - S[..., 2] / S[..., 2].sum(1, keepdim=True)
    e = (2.0 / C) * (dI / den + I * dP / den ** 2).sum() + (w.abs() * gamma_s * A_S[..., 3]).sum() / (N * V)
    return float(e) + GAMMA_FIN * float(finalize(S, V)[2])


def dprob_bound(p, t, coef, gscale, coef_err):
    """bound on dice_ce_bwd's dprob from exact probabilities when the coefficients carry coef_err (the Python route)"""
    g, G = dprob(p, t, coef, gscale)
    ea, eb, ek = _per_voxel(coef_err, p.shape)
    gate = (p >= CLAMP_LO) & (p <= 1.0)
    ekp = torch.where(gate, ek / torch.where(gate, p, torch.ones_like(p)), torch.zeros_like(p))
    return g, GAMMA_DPROB * G + abs(gscale) * (eb + t * (ea + ekp)) * (1 + GAMMA_DPROB)
