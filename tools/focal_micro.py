"""Time the focal Tversky + focal cross-entropy term (csrc/focal.hip) in one process, hip events, medians of 5 windows of 20 calls after a
warm-up, every section under a time limit of its own (SIGALRM ends the process):
  * kernels: cwf_focal_loss and cwf_focal_loss_bwd at 128^3, B = 2 and B = 8, R = 3 (WT, TC, ET), default parameters, on the softmax of
    synthetic-subject logits (a one-hot of the subject's label map, blurred by noise), each against (i) the floor of ONE read of prob
    and label at 6.3 TB/s (24 B / voxel; the backward also against 40 B / voxel, since it writes dprob) and (ii) the same term written
    with torch ops on the device in the same run, forward and forward + backward; also the two halves alone (ce_ratio = 0; no regions);
  * step: Trainer.step at the bench shape (B = 2 x 4 x 128^3, plan mode, bench precision) with the term off, on and off again in the
    same run; --what step_off times the term-off step alone and also runs on a tree without the feature.
usage: python tools/focal_micro.py [--what kernels,step] [--limit SECONDS]"""
import argparse
import gc
import json
import os
import signal
import statistics
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "decouple-and-couple_learning_in_multi-modal_brain_tumor_segmentation_amd"))

from cwf import kernels  # noqa: E402
from utils import synthetic as syn  # noqa: E402

DEV = "cuda:0"
SHAPE = (128, 128, 128)
HBM_BPS = 6.3e12
WINDOWS, CALLS = 5, 20
MASKS = (0b1110, 0b1010, 0b1000)


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


def torch_statement(prob, lab, p):
    """the same term written with torch on the device (channels-last prob): -> (loss, the leaf to differentiate)"""
    leaf = prob.detach().requires_grad_(True)
    total = leaf.new_zeros(())
    for m in MASKS:
        cls = [c for c in range(4) if (m >> c) & 1]
        pr = sum(leaf[..., c] for c in cls)
        t = sum((lab == c) for c in cls).to(leaf.dtype)
        TP, SP, ST = (t * pr).sum(), pr.sum(), t.sum()
        TI = (TP + p["smooth"]) / (TP + p["fn"] * (ST - TP) + p["fp"] * (SP - TP) + p["smooth"])
        total = total + torch.clamp(1.0 - TI, min=0.0) ** p["exponent"] / len(MASKS)
    q = leaf.gather(-1, lab.unsqueeze(-1)).squeeze(-1).clamp(1e-7, 1.0)
    total = total + p["ce_ratio"] * (-(1.0 - q) ** p["gamma"] * torch.log(q)).mean()
    return total, leaf


def kernels_section(out):
    K = kernels.backend()
    P = dict(kernels.FOCAL_DEFAULTS)
    for nb in (2, 8):
        prob, lab = subject_probs(nb)
        m = lab.numel()
        w = torch.ones(1, device=DEV)
        gs = torch.ones(1, device=DEV)
        floor_ms, floor_rw_ms = m * 24 / HBM_BPS * 1e3, m * 40 / HBM_BPS * 1e3
        for tag, masks, p in (("", MASKS, P), ("_tversky_only", MASKS, dict(P, ce_ratio=0.0)), ("_ce_only", (), P)):
            loss, coef = K.focal_loss(prob, lab, masks, p, w)
            f = windows_ms(lambda: K.focal_loss(prob, lab, masks, p, w))
            f.update(traffic_floor_ms=round(floor_ms, 4), times_floor=round(f["median_ms"] / floor_ms, 2), loss=float(loss))
            b = windows_ms(lambda: K.focal_loss_bwd(prob, lab, masks, p, coef, gs))
            b.update(traffic_floor_ms=round(floor_ms, 4), times_floor=round(b["median_ms"] / floor_ms, 2),
                     times_read_write_floor=round(b["median_ms"] / floor_rw_ms, 2))
            out["focal_loss%s_B%d" % (tag, nb)], out["focal_loss_bwd%s_B%d" % (tag, nb)] = f, b
        tl, _ = torch_statement(prob, lab, P)
        out["focal_loss_B%d" % nb]["torch_loss"] = float(tl.detach())
        tf = windows_ms(lambda: torch_statement(prob, lab, P))

        def fwd_bwd():
            l, leaf = torch_statement(prob, lab, P)
            l.backward()
        tfb = windows_ms(fwd_bwd)
        out["torch_forward_B%d" % nb], out["torch_forward_backward_B%d" % nb] = tf, tfb
        del prob, lab
        gc.collect()
        torch.cuda.empty_cache()


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
        elif what == "step":
            step(out, (("off", {}), ("on", dict(focal_weight=1.0)), ("off_again", {})))
        elif what == "step_off":
            step(out, (("off", {}), ("off_again", {})))
        else:
            raise SystemExit("unknown section %r" % what)
        signal.alarm(0)
        print(json.dumps({what: out}), flush=True)


if __name__ == "__main__":
    main()
