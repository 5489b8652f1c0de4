"""Time backend().components (R = 3: WT / TC / ET, connectivity 1) and the full predict_overlap.postprocess (region bits -> components
-> policy) on 240x240x155 BraTS-like label maps with stray voxels, for B = 1 and B = 8: hip events around every call after a warm-up,
the median over the repeats, printed as ms per case.  Next to it the same work on one host thread: scipy.ndimage.label plus the numpy
policy (the CPU path of predict_overlap.postprocess).  usage: python tools/components_micro.py [--iters N] [--noise N]"""
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
from cwf.kernels import backend  # noqa: E402

SHAPE = (240, 240, 155)
POLICY = dict(min_component=100, keep_largest=True, et_min_component=10, et_min_voxels=500, et_replace=1)


def label_map(rng, noise):
    lab = H.nested_labels(SHAPE, rng)
    idx = rng.integers(0, lab.size, size=noise)
    lab.ravel()[idx] = rng.integers(1, 4, size=noise)
    return lab


def median_ms(fn, iters):
    times = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1))
    return statistics.median(times), min(times), max(times)


def host_ms(seg, iters):
    from scipy import ndimage
    torch.set_num_threads(1)
    fp = ndimage.generate_binary_structure(3, 1)
    t_label, t_post = [], []
    for _ in range(iters):
        t0 = time.perf_counter()
        for m in H.regions(seg):
            ndimage.label(m, structure=fp)
        t1 = time.perf_counter()
        po.postprocess(torch.from_numpy(seg[None]), **POLICY)
        t2 = time.perf_counter()
        t_label.append((t1 - t0) * 1e3)
        t_post.append((t2 - t1) * 1e3)
    return statistics.median(t_label), statistics.median(t_post)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--noise", type=int, default=4000, help="stray voxels sprinkled over each map")
    args = ap.parse_args()
    be = backend()
    rng = np.random.default_rng(0)
    maps = [label_map(rng, args.noise) for _ in range(8)]
    for nb in (1, 8):
        seg = torch.from_numpy(np.stack(maps[:nb])).cuda()
        bits = be.region_bits(seg)
        for _ in range(3):
            out = be.components(bits, 3)
            post = po.postprocess(seg, **POLICY)
        torch.cuda.synchronize()
        c_med, c_min, c_max = median_ms(lambda: be.components(bits, 3), args.iters)
        p_med, p_min, p_max = median_ms(lambda: po.postprocess(seg, **POLICY), args.iters)
        print("B=%d: components (R=3) %.3f ms per case (median of %d; %.3f .. %.3f); postprocess %.3f ms per case (%.3f .. %.3f); "
              "components per region of case 0: %s; voxels changed in case 0: %d"
              % (nb, c_med / nb, args.iters, c_min / nb, c_max / nb, p_med / nb, p_min / nb, p_max / nb, out[2][0].tolist(),
                 int((post[0] != seg[0]).sum())), flush=True)
    lab_ms, post_ms = host_ms(maps[0], 3)
    print("host, one thread: scipy.ndimage.label of the three regions %.0f ms per case; numpy + scipy postprocess %.0f ms per case"
          % (lab_ms, post_ms), flush=True)


if __name__ == "__main__":
    main()
