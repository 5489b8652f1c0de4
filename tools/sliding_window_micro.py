"""Time predict_overlap.sliding_window_inference with the model (deterministic synthetic weights, stem dropout 0, fp32 kernels) on
one 240x240x155 volume -- roi 128^3 at overlap 0.5 (18 windows) and 0 (8 windows), roi 160x192x160 at overlap 0.5 -- next to the
reference-parity tailor_and_concat, and the three window kernels (cwf_window_gather / _blend / _finalize) alone against their HBM
byte floors (bytes the kernel must move / 8.0 TB/s peak).  hip events after a warm-up; prints one line per case.
usage: python tools/sliding_window_micro.py [--iters N]"""
import argparse
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "decouple-and-couple_learning_in_multi-modal_brain_tumor_segmentation_amd"))
sys.path.insert(0, REPO)

import predict_overlap as po  # noqa: E402
from cwf.kernels import backend  # noqa: E402

SHAPE = (240, 240, 155)
HBM_PEAK = 8.0e12          # bytes/s (spec)


def timed(fn, iters):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def model():
    from models.clswiseformer.cls_wise_former import get_cls_wise_former
    from oracle import reference_model as rm
    from utils import synthetic as syn
    m = get_cls_wise_former(dataset="brats", _conv_repr=True, _pe_type="fixed")
    m.load_state_dict(syn.det_state_dict(rm.param_shapes()), strict=False)
    m.Unet_list.InitConv.dropout = 0.0
    return m.cuda().eval()


def kernels(x, roi, overlap, sw, iters):
    """per-launch ms of gather / blend / finalize for the first chunk of `sw` windows, with their byte floors"""
    be = backend()
    nb = x.shape[0]
    starts = po.window_grid(SHAPE, roi, overlap)
    grid = be.window_grid(nb, SHAPE, roi, starts)
    w = torch.from_numpy(np.concatenate(po.importance_tables(roi))).cuda()
    cnt = min(sw, len(po.windows(starts)))
    nvw = roi[0] * roi[1] * roi[2]
    nv = SHAPE[0] * SHAPE[1] * SHAPE[2]
    xb = be.window_gather(x, grid, 0, cnt)
    probs = torch.rand_like(xb)
    acc = torch.empty((nb,) + SHAPE + (4,), device=x.device)
    be.window_blend(probs, w, acc, grid, 0, cnt, False)
    # floors: gather reads and writes 16 B per window voxel; blend reads the chunk's probabilities and reads + writes the
    # accumulator; finalize reads the accumulator and writes the NCDHW volume
    cases = [("gather", lambda: be.window_gather(x, grid, 0, cnt), 2 * 16 * cnt * nb * nvw),
             ("blend", lambda: be.window_blend(probs, w, acc, grid, 0, cnt, True), 16 * cnt * nb * nvw + 2 * 16 * nb * nv),
             ("finalize", lambda: be.window_finalize(acc, w, grid), 2 * 16 * nb * nv)]
    for name, fn, nbytes in cases:
        ms = timed(fn, iters)
        print("  %-8s roi %s, %d windows x B=%d: %.3f ms, %.2f GB, floor %.3f ms (%.0f%% of HBM peak)"
              % (name, "x".join(map(str, roi)), cnt, nb, ms, nbytes / 1e9, nbytes / HBM_PEAK * 1e3, 100 * nbytes / HBM_PEAK / (ms * 1e-3)),
              flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    args = ap.parse_args()
    m = model()
    x = torch.randn((1, 4) + SHAPE, generator=torch.Generator().manual_seed(0)).cuda()
    with torch.no_grad():
        ms = timed(lambda: po.tailor_and_concat(x, None, m), args.iters)
        print("tailor_and_concat (8 windows, hard overwrite): %.1f ms per volume" % ms, flush=True)
        for roi, overlap, sw in (((128, 128, 128), 0.5, 8), ((128, 128, 128), 0.0, 8), ((160, 192, 160), 0.5, 4)):
            nw = len(po.windows(po.window_grid(SHAPE, roi, overlap)))
            ms = timed(lambda: po.sliding_window_inference(x, None, m, roi_size=roi, overlap=overlap, sw_batch_size=sw), args.iters)
            print("sliding_window_inference roi %s overlap %.1f (%d windows, sw_batch_size %d): %.1f ms per volume"
                  % ("x".join(map(str, roi)), overlap, nw, sw, ms), flush=True)
    kernels(x, (128, 128, 128), 0.5, 8, 20)
    kernels(x, (160, 192, 160), 0.5, 4, 20)


if __name__ == "__main__":
    main()
