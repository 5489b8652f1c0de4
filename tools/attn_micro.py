"""The attention core and scatter_bwd alone at the training step's three launches each: attn_fwd, attn_bwd on both routes (the one-launch
attn_bwd_kernel, cwf_debug_attn_split(0), and the two launches of cwf_attn_bwd_ws at 4 / 8 / 16 waves per workgroup of launch A) and
scatter_bwd on every route (cwf_debug_scatter_bwd: 0 = 64 columns per workgroup, 8 / 16 / 32 = the narrow-block kernel).  HIP events
around 30 launches after 3 warm-ups, two repetitions per route, routes alternating.  A route counts as a win only if it is at least
10 % faster than route 0 in BOTH repetitions.  A build without the switches (the parent) prints the old routes only.
  --only attn|scatter    one family
  --route N              time one route only (for a counter run: rocprofv3 --pmc ... -- python tools/attn_micro.py --only attn --route 0)
The shapes are the step's (batch 2): attention Z = 12, 12, 2 at T = 129; scatter_bwd over 6 x 2048, 6 x 1024 (with dscat and dgate_extra)
and 2 x 1024 token rows, k = 128, E = 512."""
import argparse, os, sys
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "decouple-and-couple_learning_in_multi-modal_brain_tumor_segmentation_amd")); sys.path.insert(0, REPO)
import torch
from cwf import kernels
K = kernels.backend()
dev = "cuda:0"
ap = argparse.ArgumentParser()
ap.add_argument("--only", default=None, choices=("attn", "scatter"))
ap.add_argument("--route", type=int, default=None)
ap.add_argument("--launches", type=int, default=30)
opt = ap.parse_args()
has_split = hasattr(K.lib, "cwf_debug_attn_split")
has_wide = hasattr(K.lib, "cwf_debug_scatter_bwd")
HEADS, T, E, KSEL, P = 8, 129, 512, 128, 0.1
ATTN = (("intra-1", 12), ("intra-2", 12), ("fusion", 2))                      # name, Z (cwf/coupler.py: gb * 2, gb * 2, b)
SCATTER = (("edge", 6, 2048, False, False), ("sem", 6, 1024, True, True), ("fusion", 2, 1024, False, False))   # name, B, tokens, dscat, dgate_extra


def timed(run):
    for _ in range(3): run()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(opt.launches): run()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / opt.launches * 1e3


def attn_route(route, run):
    """route 0 = one launch; 4 / 8 / 16 = two launches at that many waves"""
    if not has_split:
        return timed(run)
    old, oldw = K.lib.cwf_debug_attn_split(1 if route else 0), K.lib.cwf_debug_attn_split_waves(route)
    try:
        n0 = K.lib.cwf_debug_attn_split_launches()
        t = timed(run)
        took = K.lib.cwf_debug_attn_split_launches() - n0
        assert took == ((opt.launches + 3) if route else 0), ("route", route, "split launches", took)
        return t
    finally:
        K.lib.cwf_debug_attn_split(old); K.lib.cwf_debug_attn_split_waves(oldw)


def scatter_route(route, run):
    if not has_wide:
        return timed(run)
    old = K.lib.cwf_debug_scatter_bwd(route)
    try:
        return timed(run)
    finally:
        K.lib.cwf_debug_scatter_bwd(old)


def table(name, routes, route_fn, run, result):
    if opt.route is not None:
        print("%-18s route %d: %7.1f us" % (name, opt.route, route_fn(opt.route, run)))
        return
    t, out = {r: [] for r in routes}, {}
    for rep in range(2):
        for r in routes:
            t[r].append(route_fn(r, run))
            out[r] = [x.clone() for x in result()]
    line = "%-18s" % name
    for r in routes:
        assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(out[r], out[routes[0]])), (name, r, "the routes differ")
        line += " | r%-2d %6.1f %6.1f" % (r, t[r][0], t[r][1])
        if r != routes[0]:
            ratios = [t[r][i] / t[routes[0]][i] for i in range(2)]
            line += "  %4.2f %4.2f %s" % (ratios[0], ratios[1], "win" if max(ratios) <= 0.9 else "no ")
    print(line)


if opt.only in (None, "attn"):
    print("attention, T = %d, heads = %d, p = %g; us per call (x2), then ratio to route 0 (x2); bwd route 0 = one launch, 4 / 8 / 16 = two launches at that many waves" % (T, HEADS, P))
    for name, z in ATTN:
        qkv = torch.randn(z * T, 3 * E, device=dev)
        d_o = torch.randn(z * T, E, device=dev)
        res = []
        if opt.route is None:
            print("%-18s | %6.1f" % (name + " Z=%d fwd" % z, timed(lambda: K.attn_fwd(qkv, z, T, HEADS, (17, P)))))
        def run():
            res[:] = [K.attn_bwd(qkv, d_o, z, T, HEADS, (17, P))]
        table(name + " Z=%d bwd" % z, (0, 4, 8, 16) if has_split else (0,), attn_route, run, lambda: res)

if opt.only in (None, "scatter"):
    print("scatter_bwd, k = %d, E = %d; us per call (x2), then ratio to route 0 (x2)" % (KSEL, E))
    for name, b, n, use_s, use_x in SCATTER:
        feats, dgated = torch.randn(b, n, E, device=dev), torch.randn(b, n, E, device=dev)
        dscat = torch.randn(b, n, E, device=dev) if use_s else None
        extra = torch.randn(b, 1, E, device=dev) if use_x else None
        index = torch.stack([torch.randperm(n, device=dev)[:KSEL] for _ in range(b)]).to(torch.int32)
        inv = torch.full((b, n), -1, dtype=torch.int32, device=dev)
        inv.scatter_(1, index.long(), torch.arange(KSEL, dtype=torch.int32, device=dev).expand(b, KSEL))
        R = torch.randn(b, 1 + KSEL, E, device=dev)
        dR = torch.empty_like(R)
        run = lambda: K.scatter_bwd(dgated, dscat, feats, inv, index, R[:, 1:], R[:, 0:1], extra, dR[:, 1:], dR[:, 0:1])
        mb = (2 * b * n * E * 4) / 1e6
        table(name + " %dx%d (%.0f MB)" % (b, n, mb), (0, 8, 16, 32) if has_wide else (0,), scatter_route, run, lambda: [dR])
