"""Single-bf16 data gradient of the 128- / 256-channel 3x3x3 stride-1 layers at 16^3 in isolation, on both routes: the wave-specialised
weight-in-LDS kernel (convwsd_kernel, cwf_debug_wsd(1)) and what the launch takes without it (cwf_debug_wsd(0): the tap-table kernel, or
convws_kernel<false> for 128 -> 256), as launched in the step (residual + norm-backward sums) and plain.
HIP events around ITERS launches after WARM warm-ups, REPS repetitions; one line per (layer, form, route).  A build without
cwf_debug_wsd (the parent) prints the old route only.  Extra layers: CIN,COUT,SIZE triples after the repetition count.
    python tools/dgrad_wsd_micro.py [reps [knob [cin,cout,size ...]]]"""
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
KNOB = int(sys.argv[2]) if len(sys.argv) > 2 else 1
# launch cin -> cout @ size^3, batch 2 (the forward layer is cout -> cin)
LAYERS = [tuple(int(v) for v in a.split(",")) for a in sys.argv[3:]] or [(128, 128, 16), (256, 128, 16), (128, 256, 16)]
hip = kernels.backend()
has_wsd = hasattr(hip.lib, "cwf_debug_wsd")


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
    w = (torch.rand(cin, cout, 3, 3, 3, generator=g) * 2 - 1) / math.sqrt(27 * cout)
    spec = CF.ConvSpec(pk.CONV3_S1, cout, cin)
    packer = CF.WeightPacker()
    packer.add(spec, torch.nn.Parameter(w.to(DEV).contiguous()))
    kernels.set_precision("bf16")
    packer.refresh()
    kernels.set_precision("fp32")
    dy = (torch.rand(n, s, s, s, cin, generator=g) * 2 - 1).to(DEV)
    res = (torch.rand(n, s, s, s, cout, generator=g) * 2 - 1).to(DEV)
    x = (torch.rand(n, s, s, s, cout, generator=g) * 2 - 1).to(DEV)
    sc, sh = (torch.rand(n, cout, generator=g) + 0.5).to(DEV), (torch.rand(n, cout, generator=g) - 0.5).to(DEV)
    dx = torch.empty(n, s, s, s, cout, device=DEV)
    sums = hip.new_stats(n, cout, DEV)
    forms = {"step ": dict(residual=res, stats=sums, nb=(x, sc, sh, 0.01)), "plain": dict()}
    for form, kw in forms.items():
        for route, knob in (("old", 0), ("wsd", KNOB)):
            if knob and not has_wsd:
                continue
            old = hip.lib.cwf_debug_wsd(knob) if has_wsd else None
            try:
                n0 = hip.lib.cwf_debug_wsd_launches() if has_wsd else 0
                f = lambda: hip.conv(pk.CONV3_S1, dy, spec.wpk16_d, None, cout, out=dx, prec="bf16", fwd_op=pk.CONV3_S1, **kw)
                t = [timeit(f) for _ in range(REPS)]
                took = (hip.lib.cwf_debug_wsd_launches() - n0) if has_wsd else 0
            finally:
                if has_wsd:
                    hip.lib.cwf_debug_wsd(old)
            print("dgrad %3d->%3d @%d^3  %s  %s%s  us/launch: %s" % (cin, cout, s, form, route, "" if bool(took) == bool(knob) else " (NOT TAKEN)",
                                                                   "  ".join("%.1f" % v for v in t)), flush=True)
