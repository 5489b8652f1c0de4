"""Time the boundary loss (csrc/boundary.hip) in one process, hip events, medians of 5 windows of 20 calls after a warm-up, every
section under a time limit of its own (SIGALRM ends the process):
  * distance: cwf_signed_distance at B = 2 and B = 8, R = 3, 128^3 on synthetic-subject labels, against its traffic floor -- one read
    of the int64 labels plus one write of the float32 maps at 6.3 TB/s -- and against scipy's distance_transform_edt on one host
    thread for the same maps (B = 2 only; skipped when scipy is missing);
  * loss: sums + finalize, and the backward, at the same shapes;
  * step: Trainer.step at the bench shape (B = 2 x 4 x 128^3, plan mode, bench precision) with the term off and on in the same run;
    --what step_off times the term-off step alone and also runs on a tree without the feature.
usage: python tools/boundary_micro.py [--what distance,loss,step] [--limit SECONDS]"""
import argparse
import gc
import json
import os
import signal
import statistics
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "decouple-and-couple_learning_in_multi-modal_brain_tumor_segmentation_amd"))

from cwf import kernels  # noqa: E402
from utils import synthetic as syn  # noqa: E402

DEV = "cuda:0"
SHAPE = (128, 128, 128)
MASKS = (0b1110, 0b1010, 0b1000)
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


def labels(nb):
    return torch.cat([syn.synthetic_batch([i], SHAPE)[1] for i in range(nb)]).to(DEV).contiguous()


def distance(out):
    K = kernels.backend()
    for nb in (2, 8):
        lab = labels(nb)
        v = lab[0].numel()
        t = windows_ms(lambda: K.signed_distance(lab, MASKS))
        floor_ms = (nb * v * 8 + nb * len(MASKS) * v * 4) / HBM_BPS * 1e3
        t.update(traffic_floor_ms=round(floor_ms, 4), times_floor=round(t["median_ms"] / floor_ms, 2))
        if nb == 2:
            try:
                from scipy.ndimage import distance_transform_edt as edt
                host = lab.cpu().numpy()
                t0 = time.perf_counter()
                for n in range(nb):
                    for m in MASKS:
                        g = ((m >> np.clip(host[n], 0, 31)) & 1).astype(bool)
                        if g.any() and not g.all():
                            (edt(~g) * ~g - (edt(g) - 1.0) * g).astype(np.float32)
                t["scipy_one_thread_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
            except ImportError:
                pass
        out["signed_distance_B%d" % nb] = t


def loss(out):
    K = kernels.backend()
    for nb in (2, 8):
        lab = labels(nb)
        phi = K.signed_distance(lab, MASKS)
        prob = torch.softmax(torch.randn((nb,) + SHAPE + (4,), device=DEV), dim=-1)
        w = torch.full((1,), 0.01, device=DEV)
        gs = torch.ones(1, device=DEV)
        _, coef = K.boundary_loss(prob, phi, MASKS, w)

        def fwd():
            K.begin_step(prob.device)                 # (hands the float64 accumulator out of the per-step arena, as the step does)
            K.boundary_loss(prob, phi, MASKS, w)
        out["begin_step_B%d" % nb] = windows_ms(lambda: K.begin_step(prob.device))
        out["begin_step_sums_finalize_B%d" % nb] = windows_ms(fwd)
        out["backward_B%d" % nb] = windows_ms(lambda: K.boundary_loss_bwd(prob, phi, MASKS, coef, gs))


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
    ap.add_argument("--what", default="distance,loss,step")
    ap.add_argument("--limit", type=int, default=240, help="seconds each section may take")
    a = ap.parse_args()
    for what in a.what.split(","):
        out = {}
        limited(a.limit)
        if what == "distance":
            distance(out)
        elif what == "loss":
            loss(out)
        elif what == "step":
            step(out, (("off", {}), ("on", dict(boundary_weight=0.01)), ("off_again", {})))
        elif what == "step_off":
            step(out, (("off", {}), ("off_again", {})))
        else:
            raise SystemExit("unknown section %r" % what)
        signal.alarm(0)
        print(json.dumps({what: out}), flush=True)


if __name__ == "__main__":
    main()
