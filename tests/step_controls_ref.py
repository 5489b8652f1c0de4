"""Yardstick for the step controls (gradient accumulation, clipping by global norm, EMA weights): pure torch / numpy on the CPU.

  * the accumulated gradient: an fp32 sum in micro-step order, ((g1 + g2) + ...) + gN;
  * the squared norm: np.sum(g.astype(np.float64) ** 2);
  * the clip coefficient of torch.nn.utils.clip_grad_norm_ in float64;
  * a whole optimisation run -- torch.optim.Adam(amsgrad=True, weight_decay) + torch.nn.utils.clip_grad_norm_ + Tensor.lerp_ --
    in float64 (or float32) from the SAME fp32 inputs.  torch's optimizer is what the reference trains with.
"""
import math

import numpy as np
import torch

SIZES = (1, 7, 300, 4097, 65537)
STEPS = 6
LR, WD = 2e-4, 1e-5
W_RTOL, W_ATOL = 1e-6, 1e-7          # weights / EMA: the bounds test_fused_adam_against_torch_fixture holds the plain kernel to
MOMENT_MARGIN = 8.0                  # moments: relative L2 error <= 8 x fp32 torch's own error against float64
MOMENTS = ("exp_avg", "exp_avg_sq", "max_exp_avg_sq")


def accumulated_sum(grads):
    """fp32 sum of a list of fp32 tensors / arrays in list order"""
    acc = np.array(grads[0], dtype=np.float32, copy=True)
    for g in grads[1:]:
        acc = (acc + np.asarray(g, dtype=np.float32)).astype(np.float32)
    return acc


def sq_norm64(g):
    return float(np.sum(np.asarray(g).astype(np.float64) ** 2))


def clip_coef64(sq_sum, grad_scale, max_norm):
    """(coefficient the optimizer multiplies the raw gradient by, norm of the scaled gradient before clipping), float64"""
    norm = float(grad_scale) * math.sqrt(sq_sum)
    c = float(max_norm) / (norm + 1e-6)
    return float(grad_scale) * (1.0 if c > 1.0 else c), norm


def make_inputs(seed=1000, sizes=SIZES, steps=STEPS):
    """fp32 start weights and per-step gradients whose scale alternates 0.01 / 10 (global norms ~2.6 and ~2600 over the 69,942
    elements): max_norm 1 clips every step, by 0.38 and by 3.8e-4; max_norm 100 leaves the small steps alone and clips the large.
    The seed is the training script's default (--seed 1000).  fp32 torch's own moment error against float64 depends on the draw -- on
    the one-element tensor it is a single rounding history, 4e-7 to 4e-6 over a handful of seeds -- which is why the GPU tests bound
    the kernel's moments RELATIVE to that error, measured on the same inputs, and not by a fixed figure."""
    gen = torch.Generator().manual_seed(seed)
    p0 = [torch.randn(n, generator=gen) for n in sizes]
    grads = [[torch.randn(n, generator=gen) * (0.01 if i % 2 == 0 else 10.0) for n in sizes] for i in range(steps)]
    return p0, grads


def run_torch(p0, grads, dtype, lr=LR, wd=WD, max_norm=None, ema_decay=None, grad_scale=1.0):
    """torch.optim.Adam(amsgrad) [+ clip_grad_norm_] [+ lerp_] in `dtype` from fp32 inputs.  Returns a dict of lists (one entry per
    tensor): 'w', 'ema' (None without ema_decay), the three moments, and 'norms' (per step, the pre-clip norm)."""
    ps = [torch.nn.Parameter(t.detach().clone().to(dtype)) for t in p0]
    ema = [p.detach().clone() for p in ps] if ema_decay is not None else None
    opt = torch.optim.Adam(ps, lr=lr, weight_decay=wd, amsgrad=True)
    norms = []
    for gs in grads:
        for p, g in zip(ps, gs):
            p.grad = g.detach().clone().to(dtype) * grad_scale
        if max_norm is not None:
            norms.append(float(torch.nn.utils.clip_grad_norm_(ps, max_norm)))
        opt.step()
        if ema is not None:
            with torch.no_grad():
                for e, p in zip(ema, ps):
                    e.lerp_(p, 1.0 - ema_decay)
    out = {"w": [p.detach().clone() for p in ps], "ema": ema, "norms": norms}
    for k in MOMENTS:
        out[k] = [opt.state[p][k].detach().clone() for p in ps]
    return out


def rel_l2(x, ref):
    x, ref = x.detach().double().cpu().reshape(-1), ref.detach().double().cpu().reshape(-1)
    return float((x - ref).norm() / ref.norm())


def close(x, ref, rtol=W_RTOL, atol=W_ATOL):
    """|x - ref| <= atol + rtol |ref| elementwise, compared in float64"""
    x, ref = x.detach().double().cpu().reshape(-1), ref.detach().double().cpu().reshape(-1)
    return bool(((x - ref).abs() <= atol + rtol * ref.abs()).all())
