"""Time the device batch preparation (HipBackend.prepare_batch, csrc/prep.hip) for 128^3 crops of 240 x 240 x 155 sources at B = 1, 2
and 8, flips off and on (intensity on in both), random origins, hip events around --iters back-to-back launches into the same output
buffers.  Prints us per batch against the floor of 102.8 MB per sample (4 fp32 image channels + uint8 label in, fp32 x + int64
target + int64 edge out) at 6.29 TB/s.  usage: python tools/prep_micro.py [--iters N]"""
import argparse
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "decouple-and-couple_learning_in_multi-modal_brain_tumor_segmentation_amd"))

from cwf.kernels import backend  # noqa: E402
from utils import data  # noqa: E402

SRC, CROP = (240, 240, 155), (128, 128, 128)
COPY_TBS = 6.29e12


def bytes_per_sample():
    v = CROP[0] * CROP[1] * CROP[2]
    return 4 * 4 * v + v + 4 * 4 * v + 8 * v + 8 * v


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    args = ap.parse_args()
    be = backend()
    g = torch.Generator(device="cuda").manual_seed(0)
    imgs = [torch.randn((4,) + SRC, device="cuda", generator=g) for _ in range(8)]
    labs = [torch.randint(0, 5, SRC, device="cuda", generator=g).to(torch.uint8) for _ in range(8)]
    floor_us = bytes_per_sample() / COPY_TBS * 1e6
    for nb in (1, 2, 8):
        out = (torch.empty((nb, 4) + CROP, device="cuda"), torch.empty((nb,) + CROP, dtype=torch.int64, device="cuda"),
               torch.empty((nb,) + CROP, dtype=torch.int64, device="cuda"))
        for flip in (False, True):
            params = [data.draw_params(1000, 0, i, SRC, CROP, flip=flip, intensity=0.1) for i in range(nb)]
            for _ in range(3):
                be.prepare_batch(imgs[:nb], labs[:nb], params, CROP, out=out)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.iters):
                be.prepare_batch(imgs[:nb], labs[:nb], params, CROP, out=out)
            e1.record()
            torch.cuda.synchronize()
            us = e0.elapsed_time(e1) * 1e3 / args.iters
            print("B=%d flip=%-5s %7.1f us per batch (%5.1f us per sample; floor %.1f us per batch = %.1f MB per sample at %.2f TB/s; "
                  "%.2f TB/s achieved)" % (nb, flip, us, us / nb, nb * floor_us, bytes_per_sample() / 1e6, COPY_TBS / 1e12,
                                           nb * bytes_per_sample() / (us * 1e-6) / 1e12), flush=True)


if __name__ == "__main__":
    main()
