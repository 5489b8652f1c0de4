"""Fused multi-tensor optimizers -- one HIP launch per optimizer step for all 218 parameters.

``FusedAdam``: semantics and state layout are those of ``torch.optim.Adam(params, lr, weight_decay, amsgrad=True)`` as the reference
uses it (train_no_amp.py:136,239): L2 decay folded into the gradient, bias-corrected first/second moments, running
max of the second moment; ``state_dict()`` has the same keys ('step', 'exp_avg', 'exp_avg_sq', 'max_exp_avg_sq') so
the checkpoint's 'optim_dict' (train_no_amp.py:252) stays interchangeable.  ``poly_lr`` is
train_no_amp.adjust_learning_rate (:270-273).

``FusedAdamW`` (``torch.optim.AdamW``: the decay multiplies the weight, the moments see the undecayed gradient) and ``FusedSGD``
(``torch.optim.SGD``: momentum, dampening, Nesterov; state 'momentum_buffer') are the two further rules, one launch of
csrc/optim_rules.hip each, with torch's state layout as well.  Both take ``no_decay`` (None, "bias_norm" or a callable
``(name, param) -> bool``): the parameters it selects get the weight-decay multiplier 0 in a per-tensor device array the launch reads.

Gradients are gathered into ONE persistent flat fp32 buffer (``flat_grad``, 67 MB): the kernel's descriptor table is
then static (safe for hipGraph capture / replay) and data-parallel training all-reduces that single buffer.

Three optional controls act on that buffer and inside the launch (csrc/grad_step.hip); with all of them off the step is the one
``cwf_adam_amsgrad_scaled`` launch it always was:
  * accumulation over micro-batches: ``accumulate(first)`` keeps the running sum of the flat gradient in a second buffer ``acc``,
    ``fold(lo, hi)`` adds it to (a slice of) the flat buffer before the update -- fp32, in micro-step order;
  * ``max_grad_norm``: clipping by global norm as ``torch.nn.utils.clip_grad_norm_`` does it; norm and coefficient stay on the
    device (``grad_norm``), the Adam launch reads the coefficient there;
  * ``ema_decay``: an exponential moving average of the weights (``ema``), updated by the Adam launch from the new value it holds
    in a register.  The EMA is not optimizer state: ``state_dict()`` keeps torch's layout.
The sink, the descriptor table and these controls live in ``FusedOptimizer``, the base of the three classes; a class adds its state
tensors and its launch."""
import math

import numpy as np
import torch

from .kernels import backend


def poly_lr(init_lr, epoch, max_epoch, power=0.9):
    return round(init_lr * np.power(1 - epoch / max_epoch, power), 8)


def cosine_lr(init_lr, epoch, max_epoch):
    """init_lr * 1/2 (1 + cos(pi epoch / max_epoch)), rounded as poly_lr rounds"""
    return round(init_lr * 0.5 * (1.0 + math.cos(math.pi * epoch / max_epoch)), 8)


SCHEDULES = ("poly", "cosine", "constant")


def schedule_lr(schedule, init_lr, epoch, max_epoch):
    """The learning rate of an epoch under `schedule` ("poly" | "cosine" | "constant"), before warm-up."""
    if schedule == "poly":
        return float(poly_lr(init_lr, epoch, max_epoch))
    if schedule == "cosine":
        return float(cosine_lr(init_lr, epoch, max_epoch))
    if schedule == "constant":
        return float(init_lr)
    raise ValueError("schedule must be one of %s, got %r" % (", ".join(SCHEDULES), schedule))


def warmup_factor(updates_done, warmup_steps):
    """Linear warm-up over weight updates: min(1, (updates_done + 1) / warmup_steps); warmup_steps = 0: 1."""
    return 1.0 if warmup_steps <= 0 else min(1.0, (updates_done + 1) / warmup_steps)


def no_decay_mask(no_decay, params, names=None):
    """One bool per parameter: True = not decayed.  no_decay: None (decay everything), "bias_norm" (every parameter with
    ndim <= 1: biases, norm gains, the couplers' tokens) or a callable (name, param) -> bool, which needs `names`."""
    params = list(params)
    if no_decay is None:
        return [False] * len(params)
    if no_decay == "bias_norm":
        return [p.ndim <= 1 for p in params]
    if callable(no_decay):
        if names is None:
            raise ValueError("a callable no_decay needs parameter names: pass (name, parameter) pairs, e.g. model.named_parameters()")
        return [bool(no_decay(n, p)) for n, p in zip(names, params)]
    raise ValueError("no_decay must be None, 'bias_norm' or a callable (name, param) -> bool, got %r" % (no_decay,))


_ACTIVE_SINK = None


def active_sink():
    """The gradient sink backward kernels may write parameter gradients into (None outside Trainer-driven backward passes)."""
    return _ACTIVE_SINK


class GradSink:
    """ONE flat fp32 buffer holding every parameter gradient, laid out in backward-completion order (`phases`: lists of
    parameters; phase k is final once backward has passed the k-th cut point of the model).  While a sink is active the conv
    weight-gradient reduction (cwf_wgrad_reduce_batched) and the coupler Functions write their parameter gradients straight
    into their slices and return None to autograd: no per-parameter gradient tensors, no AccumulateGrad, no concatenation, and
    the data-parallel all-reduce of a phase's contiguous slice can start while backward is still running (cwf.trainer)."""

    def __init__(self, params, phases=None):
        params = [p for p in params if p.requires_grad]
        if phases is None:
            phases = [params]
        known = {id(p) for p in params}
        order = [p for ph in phases for p in ph if id(p) in known]
        if len(order) != len(params) or len({id(p) for p in order}) != len(params):
            raise ValueError("phases must partition the parameter list")
        dev = params[0].device
        self.flat = torch.zeros(sum(p.numel() for p in order), dtype=torch.float32, device=dev)
        self.params = order
        self.views, self.chunks, off = {}, [], 0
        for ph in phases:
            start = off
            for p in ph:
                if id(p) in known:
                    self.views[p.data_ptr()] = self.flat[off:off + p.numel()].view_as(p)
                    off += p.numel()
            self.chunks.append((start, off))
        self.written = set()

    def view(self, p):
        """the slice of `p` (looked up by storage address: autograd may hand a Function a different Python object)"""
        return self.views.get(p.data_ptr())

    def mark(self, p):
        self.written.add(p.data_ptr())

    def begin(self):
        self.written = set()

    def __enter__(self):
        global _ACTIVE_SINK
        self._prev, _ACTIVE_SINK = _ACTIVE_SINK, self
        return self

    def __exit__(self, *a):
        global _ACTIVE_SINK
        _ACTIVE_SINK = self._prev

    def finish(self):
        """After backward: parameters whose gradient came through autograd (.grad) are copied in, parameters that received no
        gradient at all are zeroed (their slices would otherwise keep the previous step's values)."""
        srcs, dsts = [], []
        for p in self.params:
            if p.data_ptr() in self.written:
                continue
            v = self.views[p.data_ptr()]
            if p.grad is not None:
                srcs.append(p.grad); dsts.append(v)
            else:
                v.zero_()
        if srcs:
            torch._foreach_copy_(dsts, srcs)


def _split_named(params):
    """params, or (name, parameter) pairs as model.named_parameters() yields them -> (parameters, names or None)"""
    params = list(params)
    if params and isinstance(params[0], tuple):
        return [p for _, p in params], [n for n, _ in params]
    return params, None


class FusedOptimizer(torch.optim.Optimizer):
    """What the fused rules share: the gradient sink, the descriptor table {param, grad slice, up to three state tensors, n}, the
    step controls and the three phases of a step.  A rule names its state tensors in STATE (table columns m, v, vmax; a tensor
    missing from a parameter's state is a null column), creates them in _init_state and issues its launch in _update."""
    STATE = ()

    def __init__(self, params, defaults, phases=None, max_grad_norm=None, ema_decay=None, no_decay=None):
        params, names = _split_named(params)
        super().__init__(params, defaults)
        if len(self.param_groups) != 1:
            raise ValueError("%s supports one parameter group (the reference uses one, train_no_amp.py:136)" % type(self).__name__)
        if max_grad_norm is not None and not float(max_grad_norm) > 0.0:
            raise ValueError("max_grad_norm must be > 0 (float('inf'): measure the norm, never clip) or None")
        if ema_decay is not None and not 0.5 <= float(ema_decay) < 1.0:
            raise ValueError("ema_decay must lie in [0.5, 1) or be None")
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        self.ema_decay = None if ema_decay is None else float(ema_decay)
        self.acc = None                 # running sum of the flat gradient over the micro-steps of a window (accumulate / fold)
        self.ema = None                 # fp32 tensors parallel to the parameter list (built with the descriptor table)
        self._ema_table = None
        self._clip = None               # device float32 [2] = {clip coefficient * grad_scale, pre-clip norm}
        self._clip_ws = None
        keep = [i for i, p in enumerate(self.param_groups[0]["params"]) if p.requires_grad]
        self._plist = [self.param_groups[0]["params"][i] for i in keep]
        # per-parameter "not decayed" flags (None: no mask, the launch gets a null wd_mul); a constructor setting like ema_decay
        mask = no_decay_mask(no_decay, self.param_groups[0]["params"], names)
        self._no_decay = None if no_decay is None else [mask[i] for i in keep]
        self._wd_mul = None             # device float32 [len(_plist)]: 0 for a masked tensor, 1 otherwise (built with the table)
        self._phases = phases
        self.sink = None
        self.grad_scale = 1.0
        self.flat_grad = None
        self._table = None
        self._max_n = 0
        self._steps = 0

    # ------------------------------------------------------------------ setup
    def _key(self):
        """Everything the descriptor table points at: parameters AND state tensors (load_state_dict replaces the latter)."""
        k = []
        for p in self._plist:
            st = self.state.get(p) or {}
            k.append((p.data_ptr(),) + tuple(st[n].data_ptr() if n in st else 0 for n in self.STATE))
        return tuple(k)

    def load_state_dict(self, state_dict):
        """torch semantics; additionally the descriptor table is rebuilt (the state tensors are new ones) and the update counter
        continues from the loaded state (_loaded_steps)."""
        super().load_state_dict(state_dict)
        self._table = None
        self._steps = self._loaded_steps()

    def _loaded_steps(self):
        steps = [int(float(self.state[p]["step"])) for p in self._plist if p in self.state and "step" in self.state[p]]
        return max(steps) if steps else 0

    def _init_state(self, p, st, group):
        raise NotImplementedError

    def _ensure(self):
        if self._table is not None and self._table_key == self._key():
            return
        group = self.param_groups[0]
        dev = self._plist[0].device
        total = sum(p.numel() for p in self._plist)
        if self.sink is None or self.sink.flat.numel() != total or self.sink.flat.device != dev or \
                any(self.sink.view(p) is None for p in self._plist):
            self.sink = GradSink(self._plist, self._phases)
            self.flat_grad = self.sink.flat
        rows = []
        for p in self._plist:
            st = self.state[p]
            self._init_state(p, st, group)
            cols = [st[n].data_ptr() if n in st else 0 for n in self.STATE] + [0] * (3 - len(self.STATE))
            rows.append([p.data_ptr(), self.sink.view(p).data_ptr()] + cols + [p.numel()])
        self._table = torch.tensor(rows, dtype=torch.int64).to(dev)
        if self._no_decay is not None and (self._wd_mul is None or self._wd_mul.device != dev):
            self._wd_mul = torch.tensor([0.0 if nd else 1.0 for nd in self._no_decay], dtype=torch.float32).to(dev)
        if self.ema_decay is not None:
            if self.ema is None or any(e.device != p.device or e.shape != p.shape for e, p in zip(self.ema, self._plist)):
                self.ema = [p.detach().clone(memory_format=torch.contiguous_format).float() for p in self._plist]
            self._ema_table = torch.tensor([e.data_ptr() for e in self.ema], dtype=torch.int64).to(dev)
        if self.max_grad_norm is not None and (self._clip is None or self._clip.device != dev):
            from . import _lib
            self._clip = torch.zeros(2, dtype=torch.float32, device=dev)
            self._clip_ws = torch.zeros(_lib.GRADNORM_WS_DOUBLES, dtype=torch.float64, device=dev)
        self._table_key = self._key()
        self._max_n = max(r[5] for r in rows)

    # ------------------------------------------------------------------ step controls
    @property
    def grad_norm(self):
        """0-dim device tensor: L2 norm of the gradient the last update used (averaged over ranks and micro-batches), before
        clipping.  None when clipping is off.  Reading it on the host is the caller's synchronisation, not the step's."""
        if self.max_grad_norm is None:
            return None
        self._ensure()
        return self._clip[1]

    def accumulate(self, first):
        """One micro-step of an accumulation window is done: acc = flat if `first` else acc + flat (one launch, current stream)."""
        self._ensure()
        if self.acc is None or self.acc.numel() != self.flat_grad.numel() or self.acc.device != self.flat_grad.device:
            if not first:
                raise RuntimeError("accumulate(first=False) before any accumulate(first=True)")
            self.acc = torch.empty_like(self.flat_grad)
        backend().grad_add(self.flat_grad, None if first else self.acc, self.acc)

    def fold(self, lo=0, hi=None):
        """flat[lo:hi] += acc[lo:hi]: the last micro-step's gradient joins the window's sum (current stream; per phase slice when the
        slices are all-reduced one by one).  Every element must be folded exactly once before the update reads it."""
        if self.acc is None:
            raise RuntimeError("fold() without a preceding accumulate()")
        hi = self.flat_grad.numel() if hi is None else hi
        if hi > lo:
            backend().grad_add(self.flat_grad[lo:hi], self.acc[lo:hi], self.flat_grad[lo:hi])

    def reset_ema(self):
        """EMA := the current weights (e.g. after loading a checkpoint that carries none)."""
        if self.ema_decay is None:
            raise RuntimeError("this optimizer keeps no EMA (ema_decay=None)")
        self._ensure()
        with torch.no_grad():
            torch._foreach_copy_(self.ema, [p.detach() for p in self._plist])

    # ------------------------------------------------------------------ the three phases of a step
    def gather_grads(self):
        """p.grad -> flat gradient buffer for every parameter the backward kernels did not already write there (all of them
        when no sink was active during backward): one multi-tensor copy; capturable."""
        self._ensure()
        self.sink.finish()
        return self.flat_grad

    def advance_host(self):
        """Host side of a step: the step counter.  Call BEFORE launch()."""
        self._ensure()
        self._steps += 1
        for p in self._plist:
            st = self.state[p]
            if "step" in st:
                st["step"] += 1

    def _controls(self):
        """the step controls as the keyword arguments every rule's extended launch takes"""
        return dict(grad_scale=self.grad_scale,
                    gscale_dev=self._clip if self.max_grad_norm is not None else None,
                    ema_table=self._ema_table if self.ema_decay is not None else None,
                    ema_weight=(1.0 - self.ema_decay) if self.ema_decay is not None else 0.0)

    def launch(self):
        """The single fused kernel.  lr and the step number travel as KERNEL ARGUMENTS (copied at enqueue time; the bias
        corrections are evaluated in double inside the entry point): nothing the host rewrites later is read by the GPU, so
        any number of steps may be in flight.  The launch is issued eagerly after a graph replay (it is not captured)."""
        K = backend()
        if self.max_grad_norm is not None:
            # norm of the averaged gradient and grad_scale * clip coefficient, left on the device for the launch below
            K.grad_norm_clip(self.flat_grad, self.grad_scale, self.max_grad_norm, self._clip_ws, self._clip)
        self._update(K, self.param_groups[0])

    def _update(self, K, group):
        raise NotImplementedError

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        self._ensure()
        self.sink.begin()               # plain optimizer use: every gradient comes from p.grad
        self.gather_grads()
        self.advance_host()
        self.launch()
        return loss


def _init_adam_state(opt, p, st, group):
    if not st:
        st["step"] = torch.tensor(float(opt._steps))
        st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
        st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
        if group["amsgrad"]:
            st["max_exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)


class FusedAdam(FusedOptimizer):
    STATE = ("exp_avg", "exp_avg_sq", "max_exp_avg_sq")

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, amsgrad=False, phases=None,
                 max_grad_norm=None, ema_decay=None, no_decay=None):
        if no_decay is not None:
            raise ValueError("FusedAdam decays every parameter (its launch takes no mask): no_decay must be None; use FusedAdamW or FusedSGD")
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=amsgrad), phases=phases,
                         max_grad_norm=max_grad_norm, ema_decay=ema_decay)

    _init_state = _init_adam_state

    def _update(self, K, group):
        b1, b2 = group["betas"]
        if self.max_grad_norm is None and self.ema_decay is None:
            K.adam(self._table, len(self._plist), self._max_n, float(group["lr"]), b1, b2, group["eps"], group["weight_decay"],
                   self._steps, group["amsgrad"], hyper_dev=None, grad_scale=self.grad_scale)
            return
        K.adam_ex(self._table, len(self._plist), self._max_n, float(group["lr"]), b1, b2, group["eps"], group["weight_decay"],
                  self._steps, group["amsgrad"], hyper_dev=None, **self._controls())


class FusedAdamW(FusedOptimizer):
    """torch.optim.AdamW in one launch: p <- p (1 - lr weight_decay mul), then Adam's update from the undecayed gradient."""
    STATE = ("exp_avg", "exp_avg_sq", "max_exp_avg_sq")

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, amsgrad=False, phases=None,
                 max_grad_norm=None, ema_decay=None, no_decay=None):
        if not 0.0 <= lr:
            raise ValueError("Invalid learning rate: %r" % (lr,))
        if not 0.0 <= eps:
            raise ValueError("Invalid epsilon value: %r" % (eps,))
        if not (0.0 <= betas[0] < 1.0 and 0.0 <= betas[1] < 1.0):
            raise ValueError("Invalid beta parameters: %r" % (betas,))
        if not 0.0 <= weight_decay:
            raise ValueError("Invalid weight_decay value: %r" % (weight_decay,))
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=amsgrad), phases=phases,
                         max_grad_norm=max_grad_norm, ema_decay=ema_decay, no_decay=no_decay)

    _init_state = _init_adam_state

    def _update(self, K, group):
        b1, b2 = group["betas"]
        K.optim_step("adamw", self._table, len(self._plist), self._max_n, float(group["lr"]), group["weight_decay"], wd_mul=self._wd_mul,
                     beta1=b1, beta2=b2, eps=group["eps"], step=self._steps, amsgrad=group["amsgrad"], **self._controls())


class FusedSGD(FusedOptimizer):
    """torch.optim.SGD in one launch.  State: 'momentum_buffer' per parameter (none with momentum = 0), absent from state_dict()
    until the first update has filled it, as in torch -- the first update sets buf = g without dampening.  torch's SGD keeps no
    step count; the number of updates (what a warm-up continues from) travels as the extra param_group entry 'updates'."""
    STATE = ("momentum_buffer",)

    def __init__(self, params, lr=1e-3, momentum=0.0, dampening=0.0, weight_decay=0.0, nesterov=False, phases=None,
                 max_grad_norm=None, ema_decay=None, no_decay=None):
        if not 0.0 <= lr:
            raise ValueError("Invalid learning rate: %r" % (lr,))
        if not 0.0 <= momentum:
            raise ValueError("Invalid momentum value: %r" % (momentum,))
        if not 0.0 <= dampening:
            raise ValueError("Invalid dampening value: %r" % (dampening,))
        if not 0.0 <= weight_decay:
            raise ValueError("Invalid weight_decay value: %r" % (weight_decay,))
        if nesterov and (momentum <= 0 or dampening != 0):
            raise ValueError("Nesterov momentum requires a momentum and zero dampening")
        super().__init__(params, dict(lr=lr, momentum=momentum, dampening=dampening, weight_decay=weight_decay, nesterov=nesterov,
                                      updates=0), phases=phases, max_grad_norm=max_grad_norm, ema_decay=ema_decay, no_decay=no_decay)
        self._first = True              # the next update is the buffers' first one

    def _init_state(self, p, st, group):
        if group["momentum"] > 0 and st.get("momentum_buffer") is None:
            if not self._first:
                raise RuntimeError("FusedSGD: a parameter without a momentum buffer beside parameters that have one")
            st["momentum_buffer"] = torch.zeros_like(p, memory_format=torch.preserve_format)

    def state_dict(self):
        sd = super().state_dict()
        if self._first:                 # allocated but not yet filled: torch has no buffer at this point, and says so by its absence
            sd["state"] = {k: {n: v for n, v in s.items() if n != "momentum_buffer"} for k, s in sd["state"].items()}
            sd["state"] = {k: s for k, s in sd["state"].items() if s}
        return sd

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        have = [self.state.get(p, {}).get("momentum_buffer") is not None for p in self._plist]
        if any(have) and not all(have):
            raise ValueError("FusedSGD: the loaded state has momentum buffers for some parameters only")
        self._first = not any(have)     # loaded buffers: the next update is not a first one

    def _loaded_steps(self):
        return int(self.param_groups[0].setdefault("updates", 0))

    def advance_host(self):
        super().advance_host()
        self.param_groups[0]["updates"] = self._steps

    def _update(self, K, group):
        K.optim_step("sgd", self._table, len(self._plist), self._max_n, float(group["lr"]), group["weight_decay"], wd_mul=self._wd_mul,
                     momentum=group["momentum"], dampening=group["dampening"], nesterov=group["nesterov"],
                     first=self._first, **self._controls())
        if group["momentum"] > 0:
            self._first = False
