"""Time backend().surface_metrics (T = 2 tolerances: 0.5 and 1.0) against backend().hausdorff on the same masks in the same process:
240x240x155 BraTS-like label maps (three regions WT / TC / ET, surface mode, unit spacing) for B = 1 and B = 8 after a warm-up, with hip
events; prints ms per case for both and the overhead, and the scipy host path (predict_overlap.surface_regions on CPU tensors) per
case when scipy is importable.  usage: python tools/surface_micro.py [--iters N]"""
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
TAUS = (0.5, 1.0)


def timed(fn, iters):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters, out


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
        hd_ms, hd_out = timed(lambda: be.hausdorff(a, b, 3), args.iters)
        sf_ms, sf_out = timed(lambda: be.surface_metrics(a, b, 3, TAUS), args.iters)
        assert torch.equal(hd_out[1].view(torch.int64), sf_out["hd95"].view(torch.int64))
        line = "B=%d: surface_metrics (T=2) %.3f ms, hausdorff %.3f ms per 240x240x155 case (3 regions), overhead %.3f ms (%.1f%%)" % (
            nb, sf_ms / nb, hd_ms / nb, (sf_ms - hd_ms) / nb, 100.0 * (sf_ms - hd_ms) / hd_ms)
        if nb == 1:
            try:
                import predict_overlap as po
                t0 = time.perf_counter()
                po.surface_regions(seg.cpu(), tgt.cpu(), TAUS)
                line += "; scipy on the CPU: %.0f ms per case" % ((time.perf_counter() - t0) * 1e3)
            except ImportError:
                pass
        print(line, "nsd of case 0:", [[round(v, 4) for v in r] for r in sf_out["nsd"][0].tolist()], "assd:",
              [round(v, 4) for v in sf_out["assd"][0].tolist()], flush=True)


if __name__ == "__main__":
    main()
