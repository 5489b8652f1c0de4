"""Time cwf.validation.Validator.run against a plain loop of validate_softmax plus .tolist() per case, on the same model, in one
process: eight synthetic 240 x 240 x 155 subjects (utils.synthetic.synthetic_masked_volume) held on the device, roi 128^3, fp32 kernels,
deterministic synthetic weights.  Settings: the defaults (overlap 0.5), crop_nonzero, overlap 0.25, and 8-flip TTA.  A window is one
pass over the eight subjects; host wall time around a device synchronisation (the loop's cost includes its host round trips, which
device events would not see); medians of 5 windows after one warm-up pass, the two loops' windows interleaved.  The bar: the Validator's
median is not above the loop's median by more than the spread (max - min) of the loop's own windows.
usage: python tools/validation_micro.py [--what default,crop_nonzero,overlap25,tta] [--subjects 8] [--limit SECONDS]"""
import argparse
import json
import os
import signal
import statistics
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "decouple-and-couple_learning_in_multi-modal_brain_tumor_segmentation_amd"))
sys.path.insert(0, REPO)

import predict_overlap as po  # noqa: E402
from cwf.validation import Validator  # noqa: E402
from utils import synthetic as syn  # noqa: E402

DEV = "cuda:0"
WINDOWS = 5
SETTINGS = {"default": ({"roi_size": (128, 128, 128), "overlap": 0.5}, False),
            "crop_nonzero": ({"roi_size": (128, 128, 128), "overlap": 0.5, "crop_nonzero": True}, False),
            "overlap25": ({"roi_size": (128, 128, 128), "overlap": 0.25}, False),
            "tta": ({"roi_size": (128, 128, 128), "overlap": 0.5}, True)}


def limited(seconds):
    def on_alarm(signum, frame):
        print(json.dumps({"error": "section ran past its %d s limit" % seconds}), flush=True)
        os._exit(124)
    signal.signal(signal.SIGALRM, on_alarm)
    signal.alarm(seconds)


def model():
    from models.clswiseformer.cls_wise_former import get_cls_wise_former
    from oracle import reference_model as rm
    m = get_cls_wise_former(dataset="brats", _conv_repr=True, _pe_type="fixed")
    m.load_state_dict(syn.det_state_dict(rm.param_shapes()), strict=False)
    m.Unet_list.InitConv.dropout = 0.0
    return m.to(DEV).eval()


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def summary(per, cases):
    return {"median_ms": round(statistics.median(per), 2), "min_ms": round(min(per), 2), "max_ms": round(max(per), 2),
            "per_case_ms": round(statistics.median(per) / cases, 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", default="default,crop_nonzero,overlap25,tta")
    ap.add_argument("--subjects", type=int, default=8)
    ap.add_argument("--limit", type=int, default=300, help="seconds each setting may take")
    a = ap.parse_args()
    m = model()
    subjects = [(x, t.to(torch.uint8)) for x, t in (syn.synthetic_masked_volume(i) for i in range(a.subjects))]
    for what in a.what.split(","):
        window, tta = SETTINGS[what]
        limited(a.limit)
        v = Validator(subjects, DEV, window=window, use_tta=tta)
        cases = [v.case(i) for i in range(len(v))]              # the loop reads the Validator's own device copies

        def loop():
            out = []
            for x, t in cases:
                res = po.validate_softmax(x, t, m, deterministic=True, use_TTA=tta, with_miou=True, window=window)
                out.append([float(d) for d in torch.stack(res[2] + res[3]).tolist()])
            return out

        want, got = loop(), v.run(m)                            # warm-up pass of each, and the same numbers
        same = [r[:3] for r in want] == got.dice.tolist()
        per_v, per_l = [], []
        for _ in range(WINDOWS):
            per_l.append(wall_ms(loop))
            per_v.append(wall_ms(lambda: v.run(m)))
        signal.alarm(0)
        sv, sl = summary(per_v, len(v)), summary(per_l, len(v))
        ratio = sv["median_ms"] / sl["median_ms"]
        print(json.dumps({what: {"validator": sv, "loop": sl, "ratio": round(ratio, 4), "same_dice": same,
                                 "within_loop_spread": sv["median_ms"] - sl["median_ms"] <= sl["max_ms"] - sl["min_ms"]}}), flush=True)


if __name__ == "__main__":
    main()
