"""Time the elastically deformed batch preparation (HipBackend.prepare_batch with a control grid, csrc/prep.hip
cwf_prepare_batch_elastic) for 128^3 crops of 240 x 240 x 155 subjects at B = 1, 2 and 8, beside the plain and the rotated / zoomed
preparation of the same crops.  Parameters: draw_params(flip, intensity 0.1), for affine plus rotate 15 degrees and scale 0.2, for
elastic plus elastic 6 voxels on a 7^3 grid.  The elastic figure includes the pinned upload of the grids (one copy per call).

Each figure is the median over --repeats windows of --iters back-to-back calls between device events (affine_prep_micro's helper);
the variants alternate inside every repeat, and the spread (max - min over the median) is printed with it.  Nothing is asserted.
usage: python tools/elastic_prep_micro.py [--iters N] [--repeats R]"""
import argparse
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "decouple-and-couple_learning_in_multi-modal_brain_tumor_segmentation_amd"))
sys.path.insert(0, os.path.join(REPO, "tools"))

from affine_prep_micro import CROP, SRC, timed  # noqa: E402
from cwf.kernels import backend  # noqa: E402
from utils import data  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--repeats", type=int, default=7)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("elastic_prep_micro: no GPU; nothing is measured without one")
    be = backend()
    gen = torch.Generator(device="cuda").manual_seed(0)
    imgs = [torch.randn((4,) + SRC, device="cuda", generator=gen) for _ in range(8)]
    labs = [torch.randint(0, 5, SRC, device="cuda", generator=gen).to(torch.uint8) for _ in range(8)]
    for nb in (1, 2, 8):
        out = (torch.empty((nb, 4) + CROP, device="cuda"), torch.empty((nb,) + CROP, dtype=torch.int64, device="cuda"),
               torch.empty((nb,) + CROP, dtype=torch.int64, device="cuda"))
        kw = dict(flip=True, intensity=0.1)
        plain = [data.draw_params(1000, 0, i, SRC, CROP, **kw) for i in range(nb)]
        aff = [data.draw_params(1000, 0, i, SRC, CROP, rotate=15.0, scale=0.2, **kw) for i in range(nb)]
        ela = [data.draw_params(1000, 0, i, SRC, CROP, rotate=15.0, scale=0.2, elastic=6.0, elastic_grid=7, **kw) for i in range(nb)]
        variants = {
            "plain": lambda: be.prepare_batch(imgs[:nb], labs[:nb], plain, CROP, out=out),
            "affine": lambda: be.prepare_batch(imgs[:nb], labs[:nb], aff, CROP, out=out),
            "elastic": lambda: be.prepare_batch(imgs[:nb], labs[:nb], ela, CROP, out=out),
        }
        for fn in variants.values():
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        times = {k: [] for k in variants}
        for _ in range(args.repeats):
            for k, fn in variants.items():
                times[k].append(timed(fn, args.iters))
        med = {k: float(np.median(v)) for k, v in times.items()}
        for k in variants:
            print("B=%d %-8s %9.1f us per batch, %8.1f us per sample (median of %d x %d calls; min %.1f max %.1f; spread %.1f %%)"
                  % (nb, k, med[k], med[k] / nb, args.repeats, args.iters, min(times[k]), max(times[k]),
                     100 * (max(times[k]) - min(times[k])) / med[k]), flush=True)
        print("B=%d elastic / affine = %.3f, affine / plain = %.3f" % (nb, med["elastic"] / med["affine"], med["affine"] / med["plain"]),
              flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
