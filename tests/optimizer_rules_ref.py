"""Yardstick for the AdamW and SGD rules of the fused step (csrc/optim_rules.hip, cwf.optim.FusedAdamW / FusedSGD): torch's own
optimizers on the CPU, in float64 and in float32, from the fp32 inputs of step_controls_ref.make_inputs() (sizes 1, 7, 300, 4097,
65537; six steps; gradient scale alternating 0.01 / 10), each with optional clip_grad_norm_ and lerp_ -- and a hand-written numpy
statement of both rules that the float64 runs are checked against (tests/test_optimizer_rules_cpu.py).

The bound every GPU comparison uses, for weights, EMA and every state tensor alike, per tensor:

    rel_l2(kernel, float64) <= MARGIN * max(rel_l2(torch fp32, float64), 2^-24)

MARGIN is the project's MOMENT_MARGIN (8): an equally valid fp32 evaluation (a fused multiply-add where torch rounds twice, a clip
coefficient from a double sum where torch sums in fp32) moves the last bit of an operation, no more.  torch's fp32 error is measured
on the same inputs; the 2^-24 floor (half an fp32 ulp) keeps a tensor on which torch happens to land exactly -- the one-element tensor
does, on some steps -- from demanding exactness.  W_RTOL / W_ATOL of step_controls_ref are NOT used here: they are figures fitted
to Adam's weights at its learning rate, and fp32 torch's own distance from float64 under another rule and rate is not theirs to know."""
import copy

import numpy as np
import torch

import step_controls_ref as sref

MARGIN = sref.MOMENT_MARGIN
FLOOR = 2.0 ** -24
rel_l2 = sref.rel_l2

# rule -> (constructor keywords, state tensor names).  Learning rates and decays are the recipes' own: AdamW 2e-4 / 1e-2 (transformer
# recipes), SGD 1e-2 / 3e-5 (nnU-Net).
ADAMW = dict(lr=2e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2)
SGD = dict(lr=1e-2, weight_decay=3e-5)
CASES = {
    "adamw": ("adamw", dict(ADAMW, amsgrad=False)),
    "adamw_amsgrad": ("adamw", dict(ADAMW, amsgrad=True)),
    "sgd_plain": ("sgd", dict(SGD, momentum=0.0, dampening=0.0, nesterov=False)),
    "sgd_momentum_damp": ("sgd", dict(SGD, momentum=0.9, dampening=0.1, nesterov=False)),
    "sgd_nesterov": ("sgd", dict(SGD, momentum=0.99, dampening=0.0, nesterov=True)),
}


def state_names(rule, kw):
    if rule == "adamw":
        return ("exp_avg", "exp_avg_sq") + (("max_exp_avg_sq",) if kw["amsgrad"] else ())
    return ("momentum_buffer",) if kw["momentum"] > 0 else ()


def torch_optimizer(rule, params, kw, mask=None):
    """torch.optim.AdamW / SGD over `params`; mask (one bool per parameter, True = not decayed) makes two parameter groups."""
    cls = torch.optim.AdamW if rule == "adamw" else torch.optim.SGD
    if mask is None:
        return cls(params, **kw)
    groups = [{"params": [p for p, m in zip(params, mask) if not m]},
              {"params": [p for p, m in zip(params, mask) if m], "weight_decay": 0.0}]
    return cls([g for g in groups if g["params"]], **kw)


def run_torch(rule, kw, p0, grads, dtype, max_norm=None, ema_decay=None, grad_scale=1.0, mask=None, opt_state=None, first_step=0):
    """`rule` with keywords `kw` [+ clip_grad_norm_] [+ lerp_] in `dtype` from fp32 inputs.  Returns a dict of lists (one entry per
    tensor): 'w', 'ema' (None without ema_decay), every state tensor of the rule, 'norms' (per step, the pre-clip norm), and
    'opt' (the torch optimizer, for state_dict()).  opt_state: a state_dict() to continue from."""
    ps = [torch.nn.Parameter(t.detach().clone().to(dtype)) for t in p0]
    ema = [p.detach().clone() for p in ps] if ema_decay is not None else None
    opt = torch_optimizer(rule, ps, kw, mask)
    if opt_state is not None:
        opt.load_state_dict(copy.deepcopy(opt_state))          # (torch keeps the tensors it is handed: the donor goes on using its own)
    norms = []
    for gs in grads[first_step:]:
        for p, g in zip(ps, gs):
            p.grad = g.detach().clone().to(dtype) * grad_scale
        if max_norm is not None:
            norms.append(float(torch.nn.utils.clip_grad_norm_(ps, max_norm)))
        opt.step()
        if ema is not None:
            with torch.no_grad():
                for e, p in zip(ema, ps):
                    e.lerp_(p, 1.0 - ema_decay)
    out = {"w": [p.detach().clone() for p in ps], "ema": ema, "norms": norms, "opt": opt}
    for k in state_names(rule, kw):
        out[k] = [opt.state[p][k].detach().clone() for p in ps]
    return out


def run_numpy(rule, kw, p0, grads, max_norm=None, ema_decay=None, grad_scale=1.0, mask=None):
    """The two rules written out in float64 numpy, operation for operation as the header states them."""
    ps = [t.numpy().astype(np.float64) for t in p0]
    n = len(ps)
    mul = [0.0 if (mask is not None and mask[i]) else 1.0 for i in range(n)]
    ema = [p.copy() for p in ps] if ema_decay is not None else None
    m = [np.zeros_like(p) for p in ps]
    v = [np.zeros_like(p) for p in ps]
    vmax = [np.zeros_like(p) for p in ps]
    lr, wd = kw["lr"], kw["weight_decay"]
    for t, gs in enumerate(grads, 1):
        g = [x.numpy().astype(np.float64) * grad_scale for x in gs]
        if max_norm is not None:
            norm = np.sqrt(sum(float(np.sum(x * x)) for x in g))
            c = min(1.0, max_norm / (norm + 1e-6))
            g = [x * c for x in g]
        for i in range(n):
            if rule == "adamw":
                b1, b2 = kw["betas"]
                ps[i] = ps[i] * (1.0 - lr * wd * mul[i])
                m[i] = m[i] + (1.0 - b1) * (g[i] - m[i])
                v[i] = b2 * v[i] + (1.0 - b2) * g[i] * g[i]
                vv = v[i]
                if kw["amsgrad"]:
                    vmax[i] = np.maximum(vmax[i], v[i])
                    vv = vmax[i]
                denom = np.sqrt(vv) / np.sqrt(1.0 - b2 ** t) + kw["eps"]
                ps[i] = ps[i] - (lr / (1.0 - b1 ** t)) * (m[i] / denom)
            else:
                mu, damp = kw["momentum"], kw["dampening"]
                gi = g[i] + wd * mul[i] * ps[i]
                if mu > 0:
                    m[i] = gi.copy() if t == 1 else mu * m[i] + (1.0 - damp) * gi          # first update: no dampening
                    gi = gi + mu * m[i] if kw["nesterov"] else m[i]
                ps[i] = ps[i] - lr * gi
            if ema is not None:
                ema[i] = ema[i] + (1.0 - ema_decay) * (ps[i] - ema[i])
    out = {"w": ps, "ema": ema, "exp_avg": m, "exp_avg_sq": v, "max_exp_avg_sq": vmax, "momentum_buffer": m}
    return out


def bound(own):
    """the right-hand side of the bound for a tensor on which fp32 torch is `own` away from float64"""
    return MARGIN * max(own, FLOOR)


def compared(rule, kw, ema):
    """names of everything the bound is applied to"""
    return ("w",) + (("ema",) if ema else ()) + state_names(rule, kw)


def own_errors(r32, r64, names):
    return {k: [rel_l2(a, b) for a, b in zip(r32[k], r64[k])] for k in names}
