"""Time the nonzero box (csrc/nonzero_box.hip) and what it buys sliding-window inference, in one process, every section under a time
limit of its own (SIGALRM ends the process).  The subject is utils.synthetic.synthetic_masked_volume at 240 x 240 x 155: zero outside
an ellipsoid whose box is 140 x 170 x 140, about a skull-stripped BraTS brain.
  * kernel: cwf_nonzero_box at B = 1 and B = 8, hip events, medians of 5 windows of 20 calls after a warm-up, against (a) the floor of
    ONE read of x at 6.3 TB/s and (b) the same box written with torch ops on the device in the same run ((x != 0).any(1), `any` over
    the axis pairs, nonzero; its result is compared; it synchronises with the host, the kernel does not);
  * inference: predict_overlap.sliding_window_inference with the model (deterministic synthetic weights, stem dropout 0, fp32 kernels)
    on that subject at the default settings (128^3 windows, overlap 0.5, Gaussian blending, chunks of 8), crop_nonzero off and on, with
    the window counts and the largest difference of the two results inside the box; medians of 5 calls.
usage: python tools/nonzero_box_micro.py [--what kernel,inference] [--limit SECONDS]"""
import argparse
import json
import os
import signal
import statistics
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "decouple-and-couple_learning_in_multi-modal_brain_tumor_segmentation_amd"))
sys.path.insert(0, REPO)

import predict_overlap as po  # noqa: E402
from utils import synthetic as syn  # noqa: E402

FULL = (240, 240, 155)
HBM_BPS = 6.3e12
WINDOWS, CALLS = 5, 20
DEV = "cuda:0"


def windows_us(fn, warmup=3, windows=WINDOWS, calls=CALLS):
    """median and spread over `windows` windows of `calls` calls each, microseconds per call"""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    per = []
    for _ in range(windows):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(calls):
            fn()
        e1.record()
        torch.cuda.synchronize()
        per.append(e0.elapsed_time(e1) / calls * 1e3)
    return {"median_us": round(statistics.median(per), 2), "min_us": round(min(per), 2), "max_us": round(max(per), 2)}


def limited(seconds):
    def on_alarm(signum, frame):
        print(json.dumps({"error": "section ran past its %d s limit" % seconds}), flush=True)
        os._exit(124)
    signal.signal(signal.SIGALRM, on_alarm)
    signal.alarm(seconds)


def torch_statement(x):
    """the same boxes with torch ops on the device: int64 [B, 6]; one nonzero (a host synchronisation) per sample and axis"""
    nz = (x != 0).any(1)
    out = torch.empty((x.shape[0], 6), dtype=torch.int64, device=x.device)
    for b in range(x.shape[0]):
        for d, pair in enumerate(((1, 2), (0, 2), (0, 1))):
            where = nz[b].any(pair[1]).any(pair[0]).nonzero().reshape(-1)
            out[b, d], out[b, 3 + d] = (where[0], where[-1] + 1) if where.numel() else (x.shape[2 + d], 0)
    return out


def kernel_section(out):
    from cwf import kernels
    be = kernels.backend()
    one = syn.synthetic_masked_volume(0, FULL)[0].to(DEV)
    for nb in (1, 8):
        x = torch.stack([one.roll(b, dims=1) for b in range(nb)]).contiguous()       # eight boxes, each shifted by one voxel
        box = torch.empty((nb, 6), dtype=torch.int32, device=DEV)
        count = torch.empty(nb, dtype=torch.int64, device=DEV)
        be.nonzero_box(x, out=(box, count))
        floor_us = x.numel() * 4 / HBM_BPS * 1e6
        k = windows_us(lambda: be.nonzero_box(x, out=(box, count)))
        t = windows_us(lambda: torch_statement(x), windows=3, calls=5)
        k.update(one_read_floor_us=round(floor_us, 2), times_floor=round(k["median_us"] / floor_us, 2),
                 times_torch=round(k["median_us"] / t["median_us"], 4))
        out["B=%d" % nb] = {"cwf_nonzero_box": k, "torch_on_device": t, "box": box[0].tolist(), "count": int(count[0]),
                            "equal_to_torch": bool(torch.equal(box.long(), torch_statement(x)))}
        del x


def model():
    from models.clswiseformer.cls_wise_former import get_cls_wise_former
    from oracle import reference_model as rm
    m = get_cls_wise_former(dataset="brats", _conv_repr=True, _pe_type="fixed")
    m.load_state_dict(syn.det_state_dict(rm.param_shapes()), strict=False)
    m.Unet_list.InitConv.dropout = 0.0
    return m.to(DEV).eval()


def inference_section(out):
    m = model()
    x = syn.synthetic_masked_volume(0, FULL)[0][None].to(DEV)
    lo, hi = po.nonzero_box(x)
    ext = tuple(b - a for a, b in zip(lo, hi))
    out["box"], out["box_extent"] = [list(lo), list(hi)], list(ext)
    res = {}
    with torch.no_grad():
        for name, kw, shape in (("crop_nonzero_off", {}, FULL), ("crop_nonzero_on", {"crop_nonzero": True}, ext)):
            res[name] = po.sliding_window_inference(x, None, m, **kw)
            t = windows_us(lambda: po.sliding_window_inference(x, None, m, **kw), warmup=1, windows=5, calls=1)
            out[name] = {"windows": len(po.windows(po.window_grid(shape, (128, 128, 128), 0.5))),
                         "median_ms": round(t["median_us"] / 1e3, 2), "min_ms": round(t["min_us"] / 1e3, 2),
                         "max_ms": round(t["max_us"] / 1e3, 2)}
    out["times_off"] = round(out["crop_nonzero_on"]["median_ms"] / out["crop_nonzero_off"]["median_ms"], 3)
    a, b = (r[:, :, lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]] for r in (res["crop_nonzero_off"], res["crop_nonzero_on"]))
    out["max_abs_difference_inside_box"] = float((a - b).abs().max())
    out["label_agreement_inside_box"] = round(float((a.argmax(1) == b.argmax(1)).float().mean()), 6)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", default="kernel,inference")
    ap.add_argument("--limit", type=int, default=240, help="seconds each section may take")
    a = ap.parse_args()
    sections = {"kernel": kernel_section, "inference": inference_section}
    for what in a.what.split(","):
        if what not in sections:
            raise SystemExit("unknown section %r" % what)
        out = {}
        limited(a.limit)
        sections[what](out)
        signal.alarm(0)
        print(json.dumps({what: out}), flush=True)


if __name__ == "__main__":
    main()
