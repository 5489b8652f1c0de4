"""Time the update rules of the fused step (csrc/optim_rules.hip: AdamW, SGD) on the real model's 218-tensor descriptor table and
16,824,556-float parameter set, with hip events: medians of 5 windows of 20 calls, and the spread of the windows ((max - min) /
median).  One run records
  * each rule -- AdamW, AdamW amsgrad, SGD with Nesterov momentum, plain SGD -- without step controls and with clip + EMA (the device
    gradient scale and the EMA blend inside the launch; cwf_grad_norm_clip is tools/step_controls_micro.py's to time);
  * the existing Adam(amsgrad) launch, cwf_adam_amsgrad_scaled and cwf_adam_amsgrad_ex with clip + EMA, in the same run: the yardstick.
    A rule's time per byte moved is compared with the Adam launch's time per byte (per_byte_vs_adam);
  * each rule's own byte count and the time it would take at 6.3 TB/s.  Per element: AdamW 4 reads + 3 writes, with amsgrad 5 + 4 (as
    Adam), SGD with momentum 3 + 2, plain SGD 2 + 1; clip + EMA add one read and one write;
  * the same rule through torch.optim (AdamW / SGD, its default multi-tensor path) on the device, on a copy of the parameters.
With --trainer: Trainer.step in ms at the bench shape (B = 2 x 128^3, plan mode, bench precision) with default arguments, 5 windows of
20 steps; --parent-tree DIR (a checkout of another commit with its library built) measures that tree with this same file, in child
processes alternating with this tree's (this, parent, this, parent), so both figures come from one run.
usage: python tools/optimizer_micro.py [--trainer] [--parent-tree DIR]"""
import argparse
import gc
import json
import os
import statistics
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG_NAME = "decouple-and-couple_learning_in_multi-modal_brain_tumor_segmentation_amd"

DEV = "cuda:0"
WINDOWS, CALLS = 5, 20
HBM_BYTES_PER_S = 6.3e12


def use_tree(tree):
    sys.path.insert(0, os.path.join(tree, PKG_NAME))


def windows_us(fn, warmup=10):
    """[time per call in us] for WINDOWS windows of CALLS calls each, after a warm-up"""
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(WINDOWS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(CALLS):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) * 1e3 / CALLS)
    return out


def summary(ws, digits=1):
    med = statistics.median(ws)
    return {"median": round(med, digits), "min": round(min(ws), digits), "max": round(max(ws), digits),
            "spread": round((max(ws) - min(ws)) / med, 4)}


def model():
    import torch
    from models.clswiseformer.cls_wise_former import get_cls_wise_former
    torch.manual_seed(1000)
    return get_cls_wise_former(dataset="brats", _conv_repr=True, _pe_type="fixed").to(DEV).train()


def kernel_times():
    import torch
    from cwf import kernels
    from cwf.optim import FusedAdam, FusedAdamW, FusedSGD
    K = kernels.backend()
    m = model()
    ctl = dict(phases=m.grad_phases(), max_grad_norm=1.0, ema_decay=0.999)
    adam = FusedAdam(m.parameters(), lr=2e-4, weight_decay=1e-5, amsgrad=True, **ctl)
    adam._ensure()
    adam.flat_grad.normal_(0.0, 1e-3)
    adam._clip.copy_(torch.tensor([0.5, 1.0]))
    n, nt = adam.flat_grad.numel(), len(adam._plist)
    out = {"floats": n, "tensors": nt, "windows": WINDOWS, "calls_per_window": CALLS, "us": {}}
    on = dict(gscale_dev=adam._clip, ema_table=adam._ema_table, ema_weight=0.001)
    g = adam.param_groups[0]
    args = (adam._table, nt, adam._max_n, 2e-6, 0.9, 0.999, g["eps"], g["weight_decay"], 3, True)
    runs = {"adam": (36, lambda: K.adam(*args, grad_scale=0.5)),
            "adam_clip_ema": (44, lambda: K.adam_ex(*args, grad_scale=0.5, **on))}

    def rule(opt, per_elt, **kw):
        """the launch of `opt`'s rule over ITS table (own state tensors; parameters, gradients and EMA shared with the Adam one)"""
        opt.sink, opt.flat_grad = adam.sink, adam.flat_grad
        opt._ensure()
        name = "adamw" if isinstance(opt, FusedAdamW) else "sgd"
        a = (name, opt._table, nt, opt._max_n, 2e-6, 1e-2)
        return {"": (per_elt, lambda: K.optim_step(*a, wd_mul=opt._wd_mul, grad_scale=0.5, **kw)),
                "_clip_ema": (per_elt + 8, lambda: K.optim_step(*a, wd_mul=opt._wd_mul, **kw, **on))}

    named = list(m.named_parameters())
    for tag, opt, per_elt, kw in (
            ("adamw", FusedAdamW(named, no_decay="bias_norm", phases=ctl["phases"]), 28, dict(step=3)),
            ("adamw_amsgrad", FusedAdamW(named, amsgrad=True, no_decay="bias_norm", phases=ctl["phases"]), 36, dict(step=3, amsgrad=True)),
            ("sgd_nesterov", FusedSGD(named, momentum=0.99, nesterov=True, no_decay="bias_norm", phases=ctl["phases"]), 20,
             dict(momentum=0.99, nesterov=True)),
            ("sgd_plain", FusedSGD(named, phases=ctl["phases"]), 12, dict())):
        for suffix, r in rule(opt, per_elt, **kw).items():
            runs[tag + suffix] = r
    # (a learning rate of 2e-6 keeps thousands of timed updates from moving the weights anywhere that matters)
    for tag, (per_elt, fn) in runs.items():
        out["us"][tag] = dict(summary(windows_us(fn)), bytes=per_elt * n, at_6p3_TBps_us=round(per_elt * n / HBM_BYTES_PER_S * 1e6, 1))
    base = {"": out["us"]["adam"], "_clip_ema": out["us"]["adam_clip_ema"]}
    for tag, r in out["us"].items():
        ref = base["_clip_ema" if tag.endswith("_clip_ema") else ""]
        r["GBps"] = round(r["bytes"] / r["median"] / 1e3, 1)
        r["per_byte_vs_adam"] = round((r["median"] / r["bytes"]) / (ref["median"] / ref["bytes"]), 3)
    # the same rules through torch.optim on the device
    ps = [torch.nn.Parameter(p.detach().clone()) for p in adam._plist]
    for p in ps:
        p.grad = torch.randn_like(p) * 1e-3
    out["torch_optim_us"] = {}
    for tag, topt in (("adamw", torch.optim.AdamW(ps, lr=2e-6, weight_decay=1e-2)),
                      ("adamw_amsgrad", torch.optim.AdamW(ps, lr=2e-6, weight_decay=1e-2, amsgrad=True)),
                      ("sgd_nesterov", torch.optim.SGD(ps, lr=2e-6, momentum=0.99, nesterov=True, weight_decay=1e-2)),
                      ("sgd_plain", torch.optim.SGD(ps, lr=2e-6, weight_decay=1e-2))):
        out["torch_optim_us"][tag] = summary(windows_us(topt.step, warmup=3))
        del topt
    return out


def trainer_windows(warmup=8):
    """Trainer.step with default arguments at the bench shape, plan mode: WINDOWS windows of CALLS steps, ms per step"""
    import torch
    from cwf import kernels
    from cwf.trainer import Trainer
    from utils import synthetic as syn
    kernels.set_precision("bf16x3", "bf16", "bf16")                  # bench precision
    x, target, edge = (t.to(DEV) for t in syn.synthetic_batch([0, 1], (128, 128, 128)))
    tr = Trainer(model(), use_graph="plan")
    step = lambda: tr.step(x, target, edge, epoch=0)
    ws = [w / 1e3 for w in windows_us(step, warmup=warmup)]
    res = dict(summary(ws, digits=3), captured=tr._plan is not None, optimizer=type(tr.opt).__name__)
    del tr
    gc.collect()
    torch.cuda.synchronize()
    return res


def trainer_compare(parent_tree):
    """this tree and `parent_tree` alternately, each measurement in a fresh process running THIS file on that tree's package"""
    order = [("this", REPO)] + ([("parent", parent_tree), ("this", REPO), ("parent", parent_tree)] if parent_tree else [])
    runs = {"this": [], "parent": []}
    for tag, tree in order:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--trainer-child", "--tree", tree], capture_output=True, text=True,
                           timeout=600)
        if r.returncode != 0:
            raise RuntimeError("Trainer.step measurement of %s failed (%d):\n%s" % (tree, r.returncode, r.stderr[-2000:]))
        runs[tag].append(json.loads(r.stdout.strip().splitlines()[-1]))
    return {k: v for k, v in runs.items() if v}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--trainer", action="store_true", help="also time Trainer.step with default arguments at the bench shape")
    ap.add_argument("--parent-tree", default=None, help="with --trainer: a checkout of another commit (library built) to time beside this one")
    ap.add_argument("--trainer-child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--tree", default=REPO, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.trainer_child:
        use_tree(a.tree)
        print(json.dumps(trainer_windows()), flush=True)
        return
    use_tree(REPO)
    print(json.dumps({"kernels": kernel_times()}), flush=True)
    if a.trainer:
        print(json.dumps({"trainer_step_ms": trainer_compare(a.parent_tree)}), flush=True)


if __name__ == "__main__":
    main()
