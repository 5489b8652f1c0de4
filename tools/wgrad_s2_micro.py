"""The slab launch of the four stride-2 3x3x3 weight gradients of the training step alone (batch 2, single-bf16, fp32 operands,
contiguous x and dy), on both routes of cwf_debug_wgrad_s2: 0 = the tiled kernel wgrad_bf16_kernel<7, NTW, true, false>, 1 =
wgrad_s2_kernel.  Each layer is timed without a prologue (the EnDown convs read a block's output as it is) and with the
InstanceNorm + LeakyReLU(0.01) prologue.  HIP events around 30 launches after 3 warm-ups, two repetitions per route, routes
alternating; the slabs of the routes must be equal bit for bit.  A layer takes the new route in the product only if it is at least
10 % faster in BOTH repetitions.  A build without the switch (the parent) prints route 0 only.
  --route N      time one route only (for a counter run: rocprofv3 --pmc ... -- python tools/wgrad_s2_micro.py --route 0)
  --layer I      one layer of the table only
  --routes A,B   the routes of the table (default 0,1)
The bytes column is what a launch must move once (x and dy, fp32); GB/s is that over the time."""
import argparse, ctypes, os, sys
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "decouple-and-couple_learning_in_multi-modal_brain_tumor_segmentation_amd")); sys.path.insert(0, REPO)
import torch
from cwf import kernels, packing as pk
K = kernels.backend()
dev = "cuda:0"
ap = argparse.ArgumentParser()
ap.add_argument("--route", type=int, default=None)
ap.add_argument("--layer", type=int, default=None)
ap.add_argument("--routes", default="0,1")
ap.add_argument("--launches", type=int, default=30)
opt = ap.parse_args()
has_switch = hasattr(K.lib, "cwf_debug_wgrad_s2")
LAYERS = ((16, 32, 128), (32, 64, 64), (32, 32, 64), (64, 128, 32))              # cin, cout, input extent
N = 2


def timed(run):
    for _ in range(3): run()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(opt.launches): run()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / opt.launches * 1e3


def on_route(route, run):
    if not has_switch:
        return timed(run)
    old = K.lib.cwf_debug_wgrad_s2(route)
    try:
        n0 = K.lib.cwf_debug_wgrad_s2_launches()
        t = timed(run)
        took = K.lib.cwf_debug_wgrad_s2_launches() - n0
        assert took == ((opt.launches + 3) if route else 0), ("route", route, "launches of the new kernel", took)
        return t
    finally:
        K.lib.cwf_debug_wgrad_s2(old)


routes = tuple(int(r) for r in opt.routes.split(",")) if has_switch else (0,)
print("stride-2 weight-gradient slab launches, batch %d; us per launch (x2) and GB/s, then ratio to route 0 (x2)" % N)
for li, (cin, cout, s) in enumerate(LAYERS):
    if opt.layer is not None and li != opt.layer:
        continue
    so = (s - 1) // 2 + 1
    x = torch.randn(N, s, s, s, cin, device=dev)
    dy = torch.randn(N, so, so, so, cout, device=dev)
    nsplit = K.lib.cwf_wgrad_nsplit(pk.CONV3_S2, N, so, so, so, cin, cout)
    slab = K.lib.cwf_wgrad_slab_floats(pk.CONV3_S2, cin, cout)
    part = torch.empty(nsplit * slab, device=dev)
    mb = (x.numel() + dy.numel()) * 4 / 1e6
    for pro in (False, True):
        sc = (torch.rand(N, cin, device=dev) + 0.5) if pro else None
        sh = (torch.rand(N, cin, device=dev) * 2 - 1) if pro else None
        a = K._wgrad_args(pk.CONV3_S2, x, cin, sc, sh, 0.01 if pro else 1.0, dy, cout, cout, part, "bf16")
        used = ctypes.c_int(0)

        def run():
            assert K.lib.cwf_wgrad(ctypes.addressof(a), ctypes.addressof(used), K._stream()) == 0
        name = "%3d ->%4d @%3d^3 %s %4.0f MB" % (cin, cout, s, "norm " if pro else "plain", mb)
        if opt.route is not None:
            t = on_route(opt.route, run)
            print("%s route %d: %7.1f us %6.0f GB/s" % (name, opt.route, t, mb / t * 1e3))
            continue
        t, out = {r: [] for r in routes}, {}
        for rep in range(2):
            for r in routes:
                part.fill_(float("nan"))
                t[r].append(on_route(r, run))
                out[r] = part[:used.value * slab].clone()
        line = name
        for r in routes:
            assert torch.equal(out[r].view(torch.int32), out[routes[0]].view(torch.int32)), (name, r, "the routes' slabs differ")
            line += " | r%d %6.1f %6.1f %5.0f" % (r, t[r][0], t[r][1], mb / min(t[r]) * 1e3)
            if r != routes[0]:
                ratios = [t[r][i] / t[routes[0]][i] for i in range(2)]
                line += "  %4.2f %4.2f %s" % (ratios[0], ratios[1], "win" if max(ratios) <= 0.9 else "no ")
        print(line)
