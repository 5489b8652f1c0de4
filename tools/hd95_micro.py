"""Time backend().hausdorff on 240x240x155 BraTS-like label maps (three regions WT / TC / ET, surface mode, unit spacing) for B = 1
and B = 8 after a warm-up, with hip events; prints ms per case, and scipy's CPU time per case (binary_erosion +
distance_transform_edt, medpy's hd95) next to it when scipy is importable.  usage: python tools/hd95_micro.py [--iters N]"""
import argparse
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "decouple-and-couple_learning_in_multi-modal_brain_tumor_segmentation_amd"))
sys.path.insert(0, os.path.join(REPO, "tests"))

import hausdorff_ref as H  # noqa: E402
from cwf.kernels import backend  # noqa: E402

SHAPE = (240, 240, 155)


def scipy_case_ms(seg, tgt):
    from scipy import ndimage as nd
    fp = nd.generate_binary_structure(3, 1)
    t0 = time.perf_counter()
    for o, g in zip(H.regions(seg), H.regions(tgt)):
        bo, bg = o ^ nd.binary_erosion(o, structure=fp), g ^ nd.binary_erosion(g, structure=fp)
        d = np.hstack((nd.distance_transform_edt(~bg)[bo], nd.distance_transform_edt(~bo)[bg]))
        np.percentile(d, 95)
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    args = ap.parse_args()
    be = backend()
    rng = np.random.default_rng(0)
    maps = [(H.nested_labels(SHAPE, rng), H.nested_labels(SHAPE, rng)) for _ in range(8)]
    for nb in (1, 8):
        seg = torch.from_numpy(np.stack([m[0] for m in maps[:nb]])).cuda()
        tgt = torch.from_numpy(np.stack([m[1] for m in maps[:nb]])).cuda()
        a, b = be.region_bits(seg), be.region_bits(tgt)
        for _ in range(2):
            be.hausdorff(a, b, 3)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.iters):
            out = be.hausdorff(a, b, 3)
        e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1) / args.iters / nb
        line = "B=%d: %.3f ms per 240x240x155 case (3 regions, hd + hd95)" % (nb, ms)
        if nb == 1:
            try:
                cpu = scipy_case_ms(maps[0][0], maps[0][1])
                line += "; scipy on the CPU: %.0f ms per case" % cpu
            except ImportError:
                pass
        print(line, "hd95 of case 0:", [round(v, 4) for v in out[1][0].tolist()], flush=True)


if __name__ == "__main__":
    main()
