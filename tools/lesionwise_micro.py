"""Time predict_overlap.lesionwise_metrics (region bits -> dilation -> two labellings -> touch / count passes -> HD95 of eight lesions per
call -> aggregate) on 240x240x155 synthetic multi-lesion label maps, for B = 1 and B = 8: wall time around every call after a warm-up
(the call reads lesion counts back, so it ends synchronised), the median over the repeats, printed as ms per case.  Next to it the
same function on host copies of the first case (numpy + scipy, one thread).  The target holds --lesions nested blobs, the prediction the
same blobs shifted, all but one of them, plus one spurious blob and stray voxels.
usage: python tools/lesionwise_micro.py [--iters N] [--lesions N] [--noise N]"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "decouple-and-couple_learning_in_multi-modal_brain_tumor_segmentation_amd"))
sys.path.insert(0, os.path.join(REPO, "tests"))

import hausdorff_ref as H  # noqa: E402
import predict_overlap as po  # noqa: E402

SHAPE = (240, 240, 155)


def pair(rng, lesions, noise):
    centers = [[rng.uniform(0.15, 0.85) * s for s in SHAPE] for _ in range(lesions + 1)]
    tgt = H.nested_labels(SHAPE, rng, centers=centers[:lesions], scale=0.5)
    seg = H.nested_labels(SHAPE, rng, centers=[[c + 2.0 for c in p] for p in centers[1:]], scale=0.5)
    idx = rng.integers(0, seg.size, size=noise)
    seg.ravel()[idx] = rng.integers(1, 4, size=noise)
    return seg, tgt


def wall_ms(fn, iters):
    times = []
    for _ in range(iters):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(times), min(times), max(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--lesions", type=int, default=6)
    ap.add_argument("--noise", type=int, default=200, help="stray predicted voxels sprinkled over each map")
    args = ap.parse_args()
    rng = np.random.default_rng(0)
    pairs = [pair(rng, args.lesions, args.noise) for _ in range(8)]
    for nb in (1, 8):
        seg = torch.from_numpy(np.stack([p[0] for p in pairs[:nb]])).cuda()
        tgt = torch.from_numpy(np.stack([p[1] for p in pairs[:nb]])).cuda()
        for _ in range(2):
            out = po.lesionwise_metrics(seg, tgt)
        med, lo, hi = wall_ms(lambda: po.lesionwise_metrics(seg, tgt), args.iters)
        print("B=%d: lesionwise_metrics %.2f ms per case (median of %d; %.2f .. %.2f); case 0 counts (G, kept, matched, FP, FN, P) per "
              "region: %s; dice %s; hd95 %s"
              % (nb, med / nb, args.iters, lo / nb, hi / nb, out["counts"][0].tolist(), [round(v, 4) for v in out["dice"][0].tolist()],
                 [round(v, 3) for v in out["hd95"][0].tolist()]), flush=True)
    torch.set_num_threads(1)
    seg, tgt = torch.from_numpy(pairs[0][0][None]), torch.from_numpy(pairs[0][1][None])
    times = []
    for _ in range(2):
        t0 = time.perf_counter()
        host = po.lesionwise_metrics(seg, tgt)
        times.append((time.perf_counter() - t0) * 1e3)
    print("host, one thread: numpy + scipy lesionwise_metrics %.0f ms per case; counts %s" % (min(times), host["counts"][0].tolist()), flush=True)


if __name__ == "__main__":
    main()
