"""Single-bf16 data gradient of the 32- / 64-channel 3x3x3 stride-1 layers in isolation: from the fp32 gradient tensor (convws_kernel<false>)
and from its bf16 image (convws_kernel<false, true>, conv(..., x16=)), as launched in the step (residual + norm-backward sums) and plain.
HIP events around ITERS launches after WARM warm-ups, REPS repetitions; one line per (layer, form, path).  A build without
cwf_conv_x16_ok (the parent) prints the fp32 path only.
    python tools/dgrad_image_micro.py [reps]"""
import math
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "decouple-and-couple_learning_in_multi-modal_brain_tumor_segmentation_amd")); sys.path.insert(0, REPO)
import torch
from cwf import functional as CF, packing as pk, kernels

DEV = "cuda:0"
WARM, ITERS = 5, 40
REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 3
LAYERS = [(32, 32, 64), (64, 64, 32)]          # forward cin -> cout @ size^3, batch 2
hip = kernels.backend()
has_img = hasattr(hip.lib, "cwf_conv_x16_ok")


def timeit(f):
    for _ in range(WARM):
        f()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(ITERS):
        f()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1000.0 / ITERS


for cin, cout, s in LAYERS:
    n = 2
    g = torch.Generator().manual_seed(1)
    w = (torch.rand(cout, cin, 3, 3, 3, generator=g) * 2 - 1) / math.sqrt(27 * cin)
    spec = CF.ConvSpec(pk.CONV3_S1, cin, cout)
    packer = CF.WeightPacker()
    packer.add(spec, torch.nn.Parameter(w.to(DEV).contiguous()))
    kernels.set_precision("bf16")
    packer.refresh()
    kernels.set_precision("fp32")
    dy = (torch.rand(n, s, s, s, cout, generator=g) * 2 - 1).to(DEV)
    res = (torch.rand(n, s, s, s, cin, generator=g) * 2 - 1).to(DEV)
    x = (torch.rand(n, s, s, s, cin, generator=g) * 2 - 1).to(DEV)
    sc, sh = (torch.rand(n, cin, generator=g) + 0.5).to(DEV), (torch.rand(n, cin, generator=g) - 0.5).to(DEV)
    dy16 = dy.to(torch.bfloat16)
    dx = torch.empty(n, s, s, s, cin, device=DEV)
    sums = hip.new_stats(n, cin, DEV)
    forms = {"step ": dict(residual=res, stats=sums, nb=(x, sc, sh, 0.01)), "plain": dict()}
    ok = has_img and bool(hip.lib.cwf_conv_x16_ok(pk.CONV3_S1, n, s, s, s, cout, cin))
    for form, kw in forms.items():
        for path, img in (("fp32 ", None), ("image", dy16)):
            if img is not None and not ok:
                continue
            f = lambda: hip.conv(pk.CONV3_S1, dy, spec.wpk16_d, None, cin, out=dx, prec="bf16", fwd_op=pk.CONV3_S1,
                                 **(dict(x16=img) if img is not None else {}), **kw)
            t = [timeit(f) for _ in range(REPS)]
            print("dgrad %3d->%3d @%d^3  %s  %s  us/launch: %s" % (cin, cout, s, form, path, "  ".join("%.1f" % v for v in t)), flush=True)
