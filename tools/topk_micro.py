"""Time the top-k cross-entropy term (csrc/topk.hip) in one process, hip events, medians of 5 windows of 20 calls after a warm-up, every
section under a time limit of its own (SIGALRM ends the process):
  * kernels: cwf_topk_ce and cwf_topk_ce_bwd at 128^3, B = 2 and B = 8, C = 4, k = 10 %, on the softmax of synthetic-subject logits
    (a one-hot of the subject's label map, blurred by noise), each against (i) the floor of ONE read of prob and label at 6.3 TB/s
    (24 B / voxel) and (ii) the torch statement on the device in the same run: gather, clamp_min, log, topk(sorted=False), mean, and
    its backward;
  * step: Trainer.step at the bench shape (B = 2 x 4 x 128^3, plan mode, bench precision) with the term off and on in the same run;
    --what step_off times the term-off step alone and also runs on a tree without the feature;
  * logf: the largest distance, in float32 units in the last place of the float64 result, of the device's logf from the float64 log
    over 4096 arguments in [1e-7, 1], read through the kernel itself (M = 1, k = 1, w = 1 makes the loss -logf(p)).
usage: python tools/topk_micro.py [--what kernels,step,logf] [--limit SECONDS]"""
import argparse
import gc
import json
import os
import signal
import statistics
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "decouple-and-couple_learning_in_multi-modal_brain_tumor_segmentation_amd"))

from cwf import kernels  # noqa: E402
from utils import synthetic as syn  # noqa: E402

DEV = "cuda:0"
SHAPE = (128, 128, 128)
HBM_BPS = 6.3e12
WINDOWS, CALLS = 5, 20


def windows_ms(fn, warmup=3):
    """median and spread over WINDOWS windows of CALLS calls each, ms per call"""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    per = []
    for _ in range(WINDOWS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(CALLS):
            fn()
        e1.record()
        torch.cuda.synchronize()
        per.append(e0.elapsed_time(e1) / CALLS)
    return {"median_ms": round(statistics.median(per), 4), "min_ms": round(min(per), 4), "max_ms": round(max(per), 4)}


def limited(seconds):
    def on_alarm(signum, frame):
        print(json.dumps({"error": "section ran past its %d s limit" % seconds}), flush=True)
        os._exit(124)
    signal.signal(signal.SIGALRM, on_alarm)
    signal.alarm(seconds)


def subject_probs(nb):
    """(prob [nb, 128, 128, 128, 4] channels-last, label): softmax of 3 x one-hot(label) + noise, a network that is mostly right"""
    lab = torch.cat([syn.synthetic_batch([i], SHAPE)[1] for i in range(nb)]).to(DEV).contiguous()
    gen = torch.Generator(device=DEV).manual_seed(7)
    logit = 3.0 * torch.nn.functional.one_hot(lab, 4).float() + 1.5 * torch.randn(lab.shape + (4,), device=DEV, generator=gen)
    return torch.softmax(logit, dim=-1).contiguous(), lab


def torch_statement(prob, lab, k):
    """the same term written with torch on the device: forward and backward"""
    leaf = prob.detach().requires_grad_(True)
    pt = leaf.gather(-1, lab.unsqueeze(-1)).reshape(-1)
    loss = torch.topk(-torch.log(pt.clamp_min(1e-7)), k, sorted=False).values.mean()
    return loss, leaf


def kernels_section(out):
    from cwf.functional import topk_count
    K = kernels.backend()
    for nb in (2, 8):
        prob, lab = subject_probs(nb)
        m = lab.numel()
        k = topk_count(m, 10.0)
        w = torch.ones(1, device=DEV)
        gs = torch.ones(1, device=DEV)
        loss, coef = K.topk_ce(prob, lab, 0, k, w)
        floor_ms = m * 24 / HBM_BPS * 1e3
        f = windows_ms(lambda: K.topk_ce(prob, lab, 0, k, w))
        f.update(traffic_floor_ms=round(floor_ms, 4), times_floor=round(f["median_ms"] / floor_ms, 2))
        b = windows_ms(lambda: K.topk_ce_bwd(prob, lab, 0, coef, gs))
        # the backward also writes dprob: its own floor is 40 B / voxel; the issue's yardstick is the 24 B read
        b.update(traffic_floor_ms=round(floor_ms, 4), times_floor=round(b["median_ms"] / floor_ms, 2),
                 times_read_write_floor=round(b["median_ms"] / (m * 40 / HBM_BPS * 1e3), 2))
        tl, _ = torch_statement(prob, lab, k)
        f["loss"], f["torch_loss"], f["k"] = float(loss), float(tl), k
        tf = windows_ms(lambda: torch_statement(prob, lab, k))

        def fwd_bwd():
            l, leaf = torch_statement(prob, lab, k)
            l.backward()
        tfb = windows_ms(fwd_bwd)
        out["topk_ce_B%d" % nb], out["topk_ce_bwd_B%d" % nb] = f, b
        out["torch_forward_B%d" % nb], out["torch_forward_backward_B%d" % nb] = tf, tfb
        del prob, lab
        gc.collect()
        torch.cuda.empty_cache()


def logf_section(out):
    K = kernels.backend()
    rng = np.random.default_rng(0)
    args = np.concatenate([np.exp(rng.uniform(np.log(1e-7), 0.0, 3072)), rng.uniform(0.5, 1.0, 1023), [1.0]]).astype(np.float32)
    lab = torch.zeros((1, 1, 1, 1), dtype=torch.int64, device=DEV)
    w = torch.ones(1, device=DEV)
    got = []
    for a in args:
        prob = torch.tensor([[[[[float(a), 0.0, 0.0, 0.0]]]]], device=DEV)
        got.append(K.topk_ce(prob, lab, 0, 1, w)[0])
    got = torch.cat(got).cpu().numpy().astype(np.float64)
    want = -np.log(np.maximum(args, np.float32(1e-7)).astype(np.float64))
    ulp = np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
    d = np.abs(got - want) / ulp
    i = int(d.argmax())
    out["logf"] = {"values": int(args.size), "largest_ulp32": round(float(d[i]), 4), "at": float(args[i])}


def model():
    from models.clswiseformer.cls_wise_former import get_cls_wise_former
    torch.manual_seed(1000)
    return get_cls_wise_former(dataset="brats", _conv_repr=True, _pe_type="fixed").to(DEV).train()


def step(out, configs):
    from cwf.trainer import Trainer
    kernels.set_precision("bf16x3", "bf16", "bf16")                  # bench precision
    x, target, edge = (t.to(DEV) for t in syn.synthetic_batch([0, 1], SHAPE))
    for tag, kw in configs:
        tr = Trainer(model(), lr=2e-4, weight_decay=1e-5, amsgrad=True, end_epoch=1000, use_graph="plan", **kw)
        for _ in range(6):
            tr.step(x, target, edge, epoch=0)
        t = windows_ms(lambda: tr.step(x, target, edge, epoch=0), warmup=2)
        t["captured"] = tr._plan is not None
        out["step_" + tag] = t
        del tr                                                      # (model and Trainer reference each other: collect them now)
        gc.collect()
        torch.cuda.synchronize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", default="kernels,step")
    ap.add_argument("--limit", type=int, default=240, help="seconds each section may take")
    a = ap.parse_args()
    for what in a.what.split(","):
        out = {}
        limited(a.limit)
        if what == "kernels":
            kernels_section(out)
        elif what == "logf":
            logf_section(out)
        elif what == "step":
            step(out, (("off", {}), ("on", dict(topk_weight=1.0)), ("off_again", {})))
        elif what == "step_off":
            step(out, (("off", {}), ("off_again", {})))
        else:
            raise SystemExit("unknown section %r" % what)
        signal.alarm(0)
        print(json.dumps({what: out}), flush=True)


if __name__ == "__main__":
    main()
