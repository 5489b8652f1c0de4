"""Float64 reference and per-element bounds for the InstanceNorm kernel family (a helper module for the tests, not a test file).

Kernels (csrc/norm.hip; csrc/optim.hip for the channel sum) and the rule each function here restates:
  in_reduce_kernel<0> / <1> (norm.hip:20-65), launched by launch_reduce (norm.hip:168-179):
      vpb = max(256, ceil(N V / 2048)) capped at V voxels per workgroup (norm.hip:173), nvs = 256 / (C / 4) voxel sub-lanes per
      workgroup (norm.hip:26); a thread adds its L = ceil(vpb / nvs) voxels into fp32 registers (norm.hip:39-52), the nvs sub-lanes
      are folded in f64 (norm.hip:58-62) and the workgroups meet in f64 atomics (norm.hip:63).  `launch_L` restates that rule:
      whoever changes norm.hip:173 or :26 changes launch_L too.
      <0>: S1 = sum x, S2 = sum x^2.   <1>: h = x*scale + shift (plain multiply-add, the compiler may contract it),
      g = dy * act'(h), act'(h) = h > 0 ? 1 : slope (common.h:29), S1 = sum g, S2 = sum g*h.
  in_finalize_kernel (norm.hip:7-17): mean = S1/V, var = max(S2/V - mean^2, 0), rstd = 1/sqrt(var + (double)eps) with eps an fp32
      argument, scale = fp32(rstd), shift = fp32(-mean*rstd); all in f64 before the two casts.
  norm_act_add_kernel (norm.hip:68-89): y = act(x*scale + shift) + residual, act(h) = h > 0 ? h : h*slope (common.h:28);
      y16 = bf16_rne(y) (pack_bf16, common.h:34-37).
  in_bwd_apply_kernel<F32, DX16, XA16> (norm.hip:96-132): h = fmaf(x, scale, shift), g = dy*act'(h), invV = 1.0f/(float)V,
      m1 = fp32(S1 * (double)invV), m2 = fp32(S2 * (double)invV), dx = scale*(g - m1 - h*m2) (+ dx_add), dx16 = bf16_rne(dx),
      xa16 = bf16_rne(fmaxf(h, h*slope)).
  to_bf16_kernel (norm.hip:136-152): bf16_rne(fmaxf(h, h*slope)), h = fmaf(x, scale, shift).
  stats_channel_sum_kernel (optim.hip:156-162): out[c] = fp32(sum_n S1[n, c]) in f64.
slope reaches every kernel as an fp32 argument: the reference uses fp32(slope), not the Python double.

Every function takes channels-last [N, D, H, W, C] (or [N, V, C]) tensors and works on [N, V, C] float64; scale / shift are the fp32
[N, C] operands the kernel is given (the reference does not recompute them: what in_finalize makes of the sums has its own check).

Rounding model.  u = 2^-24 (bf16_operand_ref.U32).  All bounds are first order in u; the neglected products of two errors are at
most (L + 1) u <= 2^-14 of a bound each, a few of them: every bound is multiplied by SECOND_ORDER = 1 + 2^-10.

sum_rel(L).  A thread's fp32 sum of L terms: the first addition (to 0) is exact, the other L - 1 round once each, and a term carries
at most two roundings of its own (x*x: one; g*h: the product and dy*slope) -- (L + 1) u relative to T = sum |terms|, deterministic.
For long chains the project's probabilistic model (bf16_operand_ref.gamma_fp32, lambda = 8) is smaller: sum_rel = min of the two.
The f64 fold and the f64 atomics add 2^-53 per operation: nothing at this scale.

The error of h.  e = 2u (|x*scale| + |shift|) bounds |h_kernel - h_ref| for the fused form (u |h|), the unfused one
(u |x*scale| + u |h|) and the float64-then-fp32 double rounding of an emulation.  Where |h_ref| <= e the sign the kernel sees is
not determined by the operands: sign_ambiguous.  (e == 0 only if x*scale and shift are both zero; then every form gives h == 0
exactly and nothing is ambiguous, so the mask also asks for e > 0.)  On such an element either branch of act / act' is accepted.

The norm-backward sums carry, beside sum_rel(L) T, two terms the reference cannot remove (`D` of bwd_sums_ref):
  * sign-ambiguous elements: |dy| (1 - slope) in S1, |dy| (1 - slope) |h| in S2 (the other branch of act');
  * the rounding of h inside g*h: sum |g| e in S2.  It is deterministic on purpose: in a constant channel every voxel has the same x
    and so the same rounding error of h; the errors do not average out.  (T2 = sum |g h| knows nothing of it: there h_ref is ~1e-4
    while x*scale is ~2e3.)

kappa.  var = S2/V - mean^2 cancels: an error rel * T of the sums moves var by rel (T2/V + 2 |mean| T1/V) = rel (var + eps)
(kappa + 2 kappa1), kappa = (S2/V) / (var + eps), kappa1 = |mean| (T1/V) / (var + eps) <= kappa.  A channel whose mean lies 10
standard deviations from zero has kappa ~ 100, the `50 +- 0.5` family 10^4.  finalize_bound evaluates rstd at both ends of that
interval of var (the clamp at 0 included) instead of linearising: the same number wherever the first-order form is valid, and still a
bound in the constant channel, where var + eps = eps is smaller than the interval.

A channel is `degenerate` when its exact variance is 0 (a constant channel, or V == 1): h_ref is then the rounding residue of
x*scale + shift, every element is sign-ambiguous (unless x == 0) and the bf16 images sit on a bound much wider than their ulp.  Such
channels are checked like all others (either branch, the bf16 interval); they are left out only of the two vacuity caps, which are
statements about channels that have a sign and a spread.
"""
from __future__ import annotations

import numpy as np
import torch

from bf16_operand_ref import U32, gamma_fp32, hi, prologue, stats_ref

SECOND_ORDER = 1.0 + 2.0 ** -10
C_APPLY = 7          # roundings of in_bwd_apply_kernel on the longest path of a term of dx, see in_bwd_ref
C_G = 5              # ... on the path of g alone
AMBIGUOUS_CAP = 1e-4
TWO_CANDIDATE_CAP = {True: 1e-3, False: 5e-2}      # keyed by kappa <= KAPPA_SPLIT
KAPPA_SPLIT = 1.25                                  # of the family's nominal mean and spread: (mean^2 + std^2) / std^2


def f32(v):
    """the fp32 value of a Python scalar handed to a kernel as float (slope, eps)"""
    return float(np.float32(v))


def flat(t):
    """[N, ..., C] -> [N, V, C] float64"""
    return t.detach().cpu().double().reshape(t.shape[0], -1, t.shape[-1])


def bc(s):
    """[N, C] per-(sample, channel) operand -> [N, 1, C] float64"""
    return s.detach().cpu().double()[:, None, :]


# ------------------------------------------------------------------ the reduce
def launch_L(N, V, C):
    """(L, vpb, nvs) of launch_reduce + in_reduce_kernel for the public arguments (norm.hip:173 and :26, see the module docstring)"""
    vpb = max(256, -(-(V * N) // 2048))
    vpb = min(vpb, V)
    nvs = 256 // (C // 4)
    return -(-vpb // nvs), vpb, nvs


def sum_rel(L):
    """relative bound (against T = sum |terms|) of the kernel's sum whose threads add L terms in fp32"""
    return min((L + 1) * U32, gamma_fp32(L + 1))


def sums_ref(terms):
    """S = sum terms, T = sum |terms| over the voxels: [N, C] each, from [N, V, C] float64"""
    return terms.sum(1), terms.abs().sum(1)


def fwd_sums_ref(x):
    """(S, T) [N, C, 2] of in_reduce_kernel<0>: S1 = sum x, S2 = sum x^2 (S is bf16_operand_ref.stats_ref)"""
    xf = flat(x)
    S = stats_ref(xf[:, :, None, None, :])
    T = torch.stack([xf.abs().sum(1), (xf * xf).sum(1)], -1)
    return S, T


def degenerate(x):
    """[N, C] bool: the exact variance of the channel is zero (see the module docstring)"""
    xf = flat(x)
    return ((xf - xf.mean(1, keepdim=True)).abs().sum(1) == 0) | (xf.shape[1] == 1)


# ------------------------------------------------------------------ finalize
def _stat(S, V, eps):
    mean = S[..., 0] / V
    m2 = S[..., 1] / V
    var = (m2 - mean * mean).clamp_min(0.0)
    return mean, m2, var, var + f32(eps)


def finalize_ref(S, V, eps=1e-5):
    """f64 (scale, shift) [N, C] of in_finalize_kernel from sums S [N, C, 2] (the clamp var < 0 -> 0 is part of the rule)"""
    mean, _, _, ve = _stat(S.double(), V, eps)
    rstd = 1.0 / torch.sqrt(ve)
    return rstd, -mean * rstd


def kappa_of(S, V, eps=1e-5):
    mean, m2, _, ve = _stat(S.double(), V, eps)
    return m2 / ve


def finalize_bound(S, T, rel, V, eps=1e-5):
    """(B_scale, B_shift) [N, C] for scale / shift computed from sums within rel * T of S (rel = 0: the final casts alone)."""
    S, T = S.double(), T.double()
    mean, m2, var, ve = _stat(S, V, eps)
    rstd = 1.0 / torch.sqrt(ve)
    dmean = rel * T[..., 0] / V
    kappa = m2 / ve                                         # T2 == S2 for the forward sums: T2 / V = kappa (var + eps)
    kappa1 = mean.abs() * (T[..., 0] / V) / ve
    dvar = rel * ve * (kappa + 2 * kappa1) + dmean * dmean
    r_hi = 1.0 / torch.sqrt((var - dvar).clamp_min(0.0) + f32(eps))
    r_lo = 1.0 / torch.sqrt(var + dvar + f32(eps))
    drstd = torch.maximum(r_hi - rstd, rstd - r_lo)
    b_scale = drstd + 2 * U32 * rstd
    b_shift = mean.abs() * drstd + (rstd + drstd) * dmean + 2 * U32 * (mean * rstd).abs()
    return b_scale * SECOND_ORDER, b_shift * SECOND_ORDER


# ------------------------------------------------------------------ h and the forward tail
def h_ref(x, scale, shift):
    """(h, e, sign_ambiguous) [N, V, C]: h = x*scale + shift in float64 from the fp32 operands, its error radius, the mask"""
    xs = flat(x) * bc(scale)
    h = xs + bc(shift)
    e = 2 * U32 * (xs.abs() + bc(shift).abs())
    return h, e, (h.abs() <= e) & (e > 0)


def _act(h, s):
    return torch.where(h > 0, h, h * s)


def norm_act_add_ref(x, scale, shift, slope, residual=None):
    """y = act(h) + residual.  Returns (y, y_alt, B_y, amb): y_alt is the other branch of act on sign-ambiguous elements (== y
    elsewhere).  B_y = e + u (|slope h| + |y|): the error of h (e; slope * e where h is negative beyond doubt), then the roundings of
    h*slope (negative branch only) and of + residual (absent without one)."""
    s = f32(slope)
    h, e, amb = h_ref(x, scale, shift)
    r = flat(residual) if residual is not None else torch.zeros_like(h)
    y = _act(h, s) + r
    y_alt = torch.where(amb, torch.where(h > 0, h * s, h) + r, y)
    eh = torch.where(amb | (h > 0), e, s * e)                # the error of h passes through act: e, or slope * e below zero
    B = eh + U32 * ((s * h).abs() + torch.maximum(y.abs(), y_alt.abs()))
    return y, y_alt, B * SECOND_ORDER, amb


def act_h_ref(x, scale, shift, slope):
    """(lo, hi) float64 ends of act(h) over h_ref +- e: what xa16 / to_bf16 round (act is monotone for slope >= 0)"""
    s = f32(slope)
    h, e, _ = h_ref(x, scale, shift)
    e = e * SECOND_ORDER
    return _act(h - e, s), _act(h + e, s)


# ------------------------------------------------------------------ bf16 side outputs
def bf16_candidates(v, radius):
    """(lo, hi): bf16_rne(v - radius), bf16_rne(v + radius) as float64.  A bf16 output must be one of them; where radius exceeds the
    bf16 spacing (values next to zero) more than two bf16 numbers lie between them and, rounding being monotone, any of those is
    what a correct kernel may store: the check is lo <= got <= hi, which is `one of the two` whenever they are equal or adjacent."""
    return hi(v - radius), hi(v + radius)


def bf16_ratio(got16, lo16, hi16):
    """0.0 if every element of the bf16 tensor lies in [lo16, hi16], else inf; plus the index of the first offender"""
    g = got16.detach().cpu().double().reshape(lo16.shape)
    bad = ~((g >= lo16) & (g <= hi16))
    if bool(bad.any()):
        return float("inf"), tuple(int(i) for i in bad.nonzero()[0])
    return 0.0, None


# ------------------------------------------------------------------ backward
def bwd_sums_ref(dy, x, scale, shift, slope):
    """(S, T, D) [N, C, 2] of in_reduce_kernel<1>: the sums, the sums of |terms|, and the absolute error no summation order can
    avoid (sign-ambiguous elements and the rounding of h, see the module docstring).  Additive over voxel chunks."""
    s = f32(slope)
    h, e, amb = h_ref(x, scale, shift)
    d = flat(dy)
    g = d * torch.where(h > 0, 1.0, s)
    S1, T1 = sums_ref(g)
    S2, T2 = sums_ref(g * h)
    a = torch.where(amb, d.abs() * (1 - s), torch.zeros_like(d))
    D1 = a.sum(1)
    D2 = (a * h.abs()).sum(1) + (torch.maximum(g.abs(), d.abs() * amb) * e).sum(1)
    return torch.stack([S1, S2], -1), torch.stack([T1, T2], -1), torch.stack([D1, D2], -1)


def sums_bound(T, rel, D=None):
    b = rel * T.double()
    if D is not None:
        b = b + D
    return b * SECOND_ORDER


class Bwd:
    pass


def in_bwd_ref(dy, x, scale, shift, slope, S=None, dx_add=None, rel=0.0, V=None, dS=None):
    """dx = scale (g - S1/V - h S2/V) + dx_add with its per-element bound
        B_dx = |scale| (dS1/V + |h| dS2/V + |m2| e) + u (|scale| (5 |g| + 7 |m1| + 7 |h m2|) + |dx_add|)
    (c = C_APPLY = 7 is the longest chain; g, the largest term by far, has the shorter one, and the bound says so):
      |g|:    dy*slope 1, g - m1 1, - h*m2 1, scale* 1, + dx_add 1                                        = 5
      |m1|:   (float)V, 1.0f/ and the f64 -> fp32 cast 3, then the same four                               = 7
      |h m2|: the same 3 for m2, the product 1, the subtraction, scale*, + dx_add 3 (h's own error: |m2| e) = 7
      |dx_add|: its addition                                                                              = 1
    S given (the sums the kernel is fed, exact doubles): dS = 0 unless passed -- the apply kernel alone.  S None: the reference sums
    of the given tensors, dS = rel T + D (bwd_sums_ref) -- the two-pass cwf_in_bwd.  V: voxels per sample when the tensors are a
    chunk of the volume (S must then be given).  On sign-ambiguous elements dx_alt holds the other branch (== dx elsewhere)."""
    s = f32(slope)
    h, e, amb = h_ref(x, scale, shift)
    d = flat(dy)
    V = d.shape[1] if V is None else V
    r = Bwd()
    if S is None:
        S, T, D = bwd_sums_ref(dy, x, scale, shift, slope)
        dS = rel * T + D
        r.T, r.D = T, D
    elif dS is None:
        dS = torch.zeros_like(S, dtype=torch.float64)
    S = S.detach().cpu().double()
    m1, m2 = S[:, None, :, 0] / V, S[:, None, :, 1] / V
    sc = bc(scale)
    add = flat(dx_add) if dx_add is not None else torch.zeros_like(d)
    pos = h > 0
    g = d * torch.where(pos, 1.0, s)
    g_alt = torch.where(amb, d * torch.where(pos, s, 1.0), g)
    dx = sc * (g - m1 - h * m2) + add
    dx_alt = sc * (g_alt - m1 - h * m2) + add
    gm = torch.maximum(g.abs(), g_alt.abs())
    B = sc.abs() * (dS[:, None, :, 0] / V + h.abs() * dS[:, None, :, 1] / V + m2.abs() * e) \
        + U32 * (sc.abs() * (C_G * gm + C_APPLY * (m1.abs() + (h * m2).abs())) + add.abs())
    r.g, r.S, r.dS, r.dx, r.dx_alt, r.B, r.h, r.e, r.amb = g, S, dS, dx, dx_alt, B * SECOND_ORDER, h, e, amb
    return r


# ------------------------------------------------------------------ checks (return the worst err / bound; > 1 is a failure)
def ratios(got, ref, bound, alt=None):
    """|got - ref| / bound per element (alt: a second accepted reference); bound == 0 asks for equality; non-finite -> inf"""
    g = got.detach().cpu().double().reshape(ref.shape)
    err = (g - ref).abs()
    if alt is not None:
        err = torch.minimum(err, (g - alt).abs())
    r = torch.where(err == 0, torch.zeros_like(err), err / bound.clamp_min(1e-300))
    return torch.where(torch.isfinite(g), r, torch.full_like(r, float("inf")))


def ratio(got, ref, bound, alt=None):
    """(worst |got - ref| / bound, its index)"""
    r = ratios(got, ref, bound, alt)
    i = int(r.argmax())
    return float(r.reshape(-1)[i]), tuple(int(k) for k in np.unravel_index(i, r.shape))


def bf16_hull(y, y_alt, B):
    """(lo16, hi16) of a bf16 image of a value within B of y or of y_alt"""
    return hi(torch.minimum(y, y_alt) - B), hi(torch.maximum(y, y_alt) + B)


def vacuity(amb, lo16, hi16, kap, degen):
    """(share of sign-ambiguous elements, share of two-candidate elements in channels with kappa <= KAPPA_SPLIT, share in the
    others), each over the non-degenerate channels; kap (the nominal kappa of the channel's input family), degen: [N, C]."""
    live = (~degen)[:, None, :].expand_as(amb)
    two = lo16 != hi16
    small = (kap <= KAPPA_SPLIT + 1e-12)[:, None, :].expand_as(amb)

    def share(m, within):
        n = int(within.sum())
        return (float((m & within).sum()) / n if n else 0.0), n
    return share(amb, live), share(two, live & small), share(two, live & ~small)


def cap_for(cap, n):
    """the cap on a share observed on n elements: the cap on the rate plus three standard deviations of a count of n draws at
    that rate (a case of 3000 elements holds three two-candidate elements at the rate 1e-3; one more is sampling noise, not
    vacuity).  From 10^6 elements on the allowance is under a tenth of the cap."""
    return cap + 3.0 * (cap * (1 - cap) / max(n, 1)) ** 0.5


def assert_not_vacuous(amb, lo16, hi16, kap, degen, what):
    (a, na), (t_small, ns), (t_large, nl) = vacuity(amb, lo16, hi16, kap, degen)
    assert a <= cap_for(AMBIGUOUS_CAP, na), (what, "vacuous: sign-ambiguous share", a)
    assert t_small <= cap_for(TWO_CANDIDATE_CAP[True], ns), (what, "vacuous: two-candidate share, kappa <= 1.25", t_small, ns)
    assert t_large <= cap_for(TWO_CANDIDATE_CAP[False], nl), (what, "vacuous: two-candidate share, kappa > 1.25", t_large, nl)
    return a, t_small, t_large


def prologue_operand(x, scale, shift, slope):
    """the bf16 x operand the weight-gradient reference builds (bf16_operand_ref.prologue + hi), [N, V, C] float64"""
    return flat(hi(prologue(x, scale, shift, f32(slope))))
