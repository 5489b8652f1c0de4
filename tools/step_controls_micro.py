"""Time the step controls (csrc/grad_step.hip) on the real model's 218-tensor descriptor table and 16,824,556-float flat gradient, with
hip events after a warm-up:
  * cwf_grad_add over the whole buffer (accumulate: acc += flat) against the one-thread-per-element cwf_add on the same buffers;
  * cwf_grad_norm_clip;
  * cwf_adam_amsgrad_ex with clip only, EMA only and both, against the plain Adam launch (cwf_adam_amsgrad_scaled);
  * with --trainer: Trainer.step in ms at the bench shape (B = 2 x 128^3, plan mode, bench precision) with all options off, with
    accum_steps=2 (per micro-step) and with clip + EMA.
usage: python tools/step_controls_micro.py [--iters N] [--trainer] [--steps K]"""
import argparse
import gc
import json
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "decouple-and-couple_learning_in_multi-modal_brain_tumor_segmentation_amd"))

from cwf import _lib, kernels  # noqa: E402
from cwf.optim import FusedAdam  # noqa: E402

DEV = "cuda:0"


def timed_us(fn, iters, warmup=5):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters


def model():
    from models.clswiseformer.cls_wise_former import get_cls_wise_former
    torch.manual_seed(1000)
    return get_cls_wise_former(dataset="brats", _conv_repr=True, _pe_type="fixed").to(DEV).train()


def kernel_times(iters):
    K = kernels.backend()
    m = model()
    opt = FusedAdam(m.parameters(), lr=2e-4, weight_decay=1e-5, amsgrad=True, phases=m.grad_phases(), max_grad_norm=1.0, ema_decay=0.999)
    opt._ensure()
    flat = opt.flat_grad
    flat.normal_(0.0, 1e-3)
    acc = torch.randn_like(flat)
    n, nt = flat.numel(), len(opt._plist)
    out = {"floats": n, "tensors": nt, "MB": round(n * 4 / 1e6, 1)}
    out["grad_add_us"] = timed_us(lambda: K.grad_add(flat, acc, acc), iters)
    out["grad_add_copy_us"] = timed_us(lambda: K.grad_add(flat, None, acc), iters)
    s = K._stream()
    out["cwf_add_us"] = timed_us(lambda: K._call("cwf_add", flat.data_ptr(), acc.data_ptr(), acc.data_ptr(), n, s), iters)
    lo, hi = opt.sink.chunks[1]
    out["grad_add_phase1_us"] = timed_us(lambda: K.grad_add(flat[lo:hi], acc[lo:hi], flat[lo:hi]), iters)
    out["phase1_floats"] = hi - lo
    flat.normal_(0.0, 1e-3)
    out["grad_norm_clip_us"] = timed_us(lambda: K.grad_norm_clip(flat, 0.5, 1.0, opt._clip_ws, opt._clip), iters)
    g = opt.param_groups[0]
    args = (opt._table, nt, opt._max_n, 2e-4, 0.9, 0.999, g["eps"], g["weight_decay"], 3, True)
    out["adam_us"] = timed_us(lambda: K.adam(*args, grad_scale=0.5), iters)
    out["adam_ex_clip_us"] = timed_us(lambda: K.adam_ex(*args, grad_scale=0.5, gscale_dev=opt._clip), iters)
    out["adam_ex_ema_us"] = timed_us(lambda: K.adam_ex(*args, grad_scale=0.5, ema_table=opt._ema_table, ema_weight=0.001), iters)
    out["adam_ex_clip_ema_us"] = timed_us(lambda: K.adam_ex(*args, grad_scale=0.5, gscale_dev=opt._clip, ema_table=opt._ema_table,
                                                            ema_weight=0.001), iters)
    gb = lambda nbytes, us: round(nbytes / us / 1e3, 1)
    out["GBps"] = {"grad_add": gb(12 * n, out["grad_add_us"]), "cwf_add": gb(12 * n, out["cwf_add_us"]),
                   "grad_norm_clip": gb(4 * n, out["grad_norm_clip_us"]), "adam": gb(36 * n, out["adam_us"]),
                   "adam_ex_clip_ema": gb(44 * n, out["adam_ex_clip_ema_us"])}
    return {k: (round(v, 1) if isinstance(v, float) else v) for k, v in out.items()}


def trainer_times(steps, warmup=6):
    from cwf.trainer import Trainer
    from utils import synthetic as syn
    kernels.set_precision("bf16x3", "bf16", "bf16")                  # bench precision
    x, target, edge = (t.to(DEV) for t in syn.synthetic_batch([0, 1], (128, 128, 128)))
    out = {}
    for tag, kw in (("off", {}), ("accum2_per_micro_step", dict(accum_steps=2)), ("clip_ema", dict(max_grad_norm=1.0, ema_decay=0.999)),
                    ("accum2_clip_ema_per_micro_step", dict(accum_steps=2, max_grad_norm=1.0, ema_decay=0.999))):
        tr = Trainer(model(), lr=2e-4, weight_decay=1e-5, amsgrad=True, end_epoch=1000, use_graph="plan", **kw)
        for _ in range(warmup):
            tr.step(x, target, edge, epoch=0)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(steps):
            tr.step(x, target, edge, epoch=0)
        e1.record()
        torch.cuda.synchronize()
        out[tag + "_ms"] = round(e0.elapsed_time(e1) / steps, 3)
        out[tag + "_captured"] = tr._plan is not None
        # model and Trainer reference each other (phase_callback): collect them now -- the captured graph's destruction synchronises the
        # device and must not land in the next configuration's timed window
        del tr
        gc.collect()
        torch.cuda.synchronize()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=1000)
    ap.add_argument("--trainer", action="store_true", help="also time Trainer.step at the bench shape")
    ap.add_argument("--steps", type=int, default=60)
    a = ap.parse_args()
    assert _lib.GRADNORM_WS_DOUBLES == 1024
    print(json.dumps({"kernels_us": kernel_times(a.iters)}), flush=True)
    if a.trainer:
        print(json.dumps({"trainer_step_ms": trainer_times(a.steps)}), flush=True)


if __name__ == "__main__":
    main()
