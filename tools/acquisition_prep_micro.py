"""Time the acquisition stage of the batch preparation (HipBackend.prepare_batch with bias / contrast / lowres, csrc/acquire.hip
cwf_augment_acquisition) for 128^3 crops of 240 x 240 x 155 subjects at B = 2 and B = 8: the plain preparation (draw_params(flip,
intensity 0.1)), and the same with the bias field (5^3 control multipliers exp(U(-0.5, 0.5))), with contrast (factor 1.2), with the
low-resolution simulation (zoom 0.7) and with all three, each switched on for all four channels of every sample -- the most the
stage can be asked for (draw_params switches a channel on with probability 1/2).  A variant's time less the plain preparation's is
the stage's cost; it is printed beside
  * the floor of a stage that reads x once and writes it once, 2 * B * 4 * 128^3 * 4 B (134 MB at B = 2) at 6.3 TB/s, the
    achievable HBM rate of MI355X_MICROARCH.md (contrast reads x a second time for its statistics, and with all three on the gather
    reads and writes it once more: the ratio printed is to ONE read and one write in every row), and
  * a torch baseline on the same x in the same run: the field as three einsum contractions of dense per-axis weight matrices with
    the control grid and a multiply; mean / amin / amax per channel and the clamped map; nearest interpolate down to the lattice and
    trilinear interpolate back (torch's own definitions of the sample positions).

Each figure is the median over --repeats windows of --iters back-to-back calls between device events; the variants alternate
inside every repeat, and the spread (max - min over the median) is printed with it.  Beside it stands the host's time to enqueue a
call (a clock around the same loop, read before the synchronise): where the two are about equal the window measured the host, and
the device's share is smaller than the figure.  Nothing is asserted.
usage: python tools/acquisition_prep_micro.py [--iters N] [--repeats R]"""
import argparse
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "decouple-and-couple_learning_in_multi-modal_brain_tumor_segmentation_amd"))
sys.path.insert(0, os.path.join(REPO, "tools"))

from affine_prep_micro import CROP, SRC  # noqa: E402
from cwf.kernels import backend  # noqa: E402
from intensity_prep_micro import HBM, timed  # noqa: E402
from utils import data  # noqa: E402


def torch_baseline(x, grids, factor, lattice):
    """the three transforms on x [B, 4, *CROP] with torch operators"""
    B = x.shape[0]
    w = []
    for d in range(3):
        wd, idx = data._spline_axis(CROP[d], False, grids.shape[2 + d])
        dense = np.zeros((CROP[d], grids.shape[2 + d]), dtype=np.float32)
        for j in range(4):
            np.add.at(dense, (np.arange(CROP[d]), idx[:, j]), wd[:, j])
        w.append(torch.from_numpy(dense).cuda())

    def bias(y=None):
        y = x if y is None else y
        m = torch.einsum("bcijk,zk->bcijz", grids, w[2])
        m = torch.einsum("bcijz,yj->bciyz", m, w[1])
        m = torch.einsum("bciyz,xi->bcxyz", m, w[0])
        return y * m

    def contrast(y=None):
        y = x if y is None else y
        mean = y.mean(dim=(2, 3, 4), keepdim=True, dtype=torch.float64).float()
        mn, mx = y.amin(dim=(2, 3, 4), keepdim=True), y.amax(dim=(2, 3, 4), keepdim=True)
        return torch.minimum(torch.maximum((y - mean) * factor + mean, mn), mx)

    def lowres(y=None):
        y = x if y is None else y
        F = torch.nn.functional
        coarse = F.interpolate(y.reshape(B, 4, *CROP), size=lattice, mode="nearest")
        return F.interpolate(coarse, size=CROP, mode="trilinear", align_corners=False)

    return {"torch bias": bias, "torch contrast": contrast, "torch lowres": lowres, "torch all": lambda: lowres(contrast(bias()))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("acquisition_prep_micro: no GPU; nothing is measured without one")
    be = backend()
    gen = torch.Generator(device="cuda").manual_seed(0)
    imgs = [torch.randn((4,) + SRC, device="cuda", generator=gen) for _ in range(8)]
    labs = [torch.randint(0, 5, SRC, device="cuda", generator=gen).to(torch.uint8) for _ in range(8)]
    factor, zoom, G = 1.2, 0.7, (5, 5, 5)
    rng = np.random.default_rng(0)
    grids = [np.exp(rng.uniform(-0.5, 0.5, (4,) + G)).astype(np.float32) for _ in range(8)]
    for nb in (2, 8):
        out = (torch.empty((nb, 4) + CROP, device="cuda"), torch.empty((nb,) + CROP, dtype=torch.int64, device="cuda"),
               torch.empty((nb,) + CROP, dtype=torch.int64, device="cuda"))
        base = [data.draw_params(1000, 0, i, SRC, CROP, flip=True, intensity=0.1) for i in range(nb)]
        variants = {}
        for name in ("plain", "bias", "contrast", "lowres", "all"):
            ps = []
            for i, p in enumerate(base):
                kw = {}
                if name in ("bias", "all"):
                    kw.update(bias=grids[i], bias_mask=(True,) * 4)
                if name in ("contrast", "all"):
                    kw.update(contrast=(factor,) * 4)
                if name in ("lowres", "all"):
                    kw.update(lowres=(zoom,) * 4)
                ps.append(data.AugParams(p.origin, p.flip, p.scale, p.shift, **kw))
            variants[name] = (lambda ps=ps: be.prepare_batch(imgs[:nb], labs[:nb], ps, CROP, out=out))
        x = be.prepare_batch(imgs[:nb], labs[:nb], base, CROP)[0]
        variants.update(torch_baseline(x, torch.from_numpy(np.stack(grids[:nb])).cuda(), factor, data.lowres_lattice(CROP, zoom)))
        for fn in variants.values():
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        times, host = {k: [] for k in variants}, {k: [] for k in variants}
        for _ in range(args.repeats):
            for k, fn in variants.items():
                dev_us, host_us = timed(fn, args.iters)
                times[k].append(dev_us)
                host[k].append(host_us)
        med = {k: float(np.median(v)) for k, v in times.items()}
        for k in variants:
            print("B=%d %-14s %9.1f us per batch (median of %d x %d calls; min %.1f max %.1f; spread %.1f %%; host enqueue %.1f us)"
                  % (nb, k, med[k], args.repeats, args.iters, min(times[k]), max(times[k]), 100 * (max(times[k]) - min(times[k])) / med[k],
                     float(np.median(host[k]))), flush=True)
        floor = 2 * nb * 4 * CROP[0] * CROP[1] * CROP[2] * 4 / HBM * 1e6
        for k in ("bias", "contrast", "lowres", "all"):
            cost = med[k] - med["plain"]
            print("B=%d stage %-8s %9.1f us over plain = %.2f x the floor of %.1f us (one read and one write of x at 6.3 TB/s) = %.3f x "
                  "torch %s (%.1f us)" % (nb, k, cost, cost / floor, floor, cost / med["torch " + k], k, med["torch " + k]), flush=True)
        del x, variants
    return 0


if __name__ == "__main__":
    sys.exit(main())
