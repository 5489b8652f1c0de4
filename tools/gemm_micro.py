"""Plain strided-batched GEMM (cwf_gemm_ex without epilogue features) at the token path's production shapes and operand layouts, on both
routes: the 16-byte-load kernel (cwf_debug_gemm_panel(0)) and the K-panel kernel ((2)).  HIP events around 30 launches after 3
warm-ups, two repetitions per route, routes alternating.  A shape class counts as a win for the panel kernel only if it is at least
10 % faster there in BOTH repetitions.
  --only NAME     one shape (for a counter run: rocprofv3 --pmc ... -- python tools/gemm_micro.py --only fwd-out --route 2)
  --route 0|2     time one route only"""
import argparse, os, sys
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "decouple-and-couple_learning_in_multi-modal_brain_tumor_segmentation_amd")); sys.path.insert(0, REPO)
import torch
from cwf import kernels
K = kernels.backend()
dev = "cuda:0"
# name, M, N, K, ZB, layout: T/F = the unit-stride dimension of A is k / of B is n (forward x W^T: TF, data gradient dy W: TT, weight gradient dy^T x: FT)
SHAPES = (("fwd-out", 516, 512, 512, 3, "TF"), ("fwd-qkv", 516, 1536, 512, 3, "TF"), ("fwd-fusion", 258, 512, 512, 1, "TF"),
          ("dgrad-512", 516, 512, 512, 3, "TT"), ("dgrad-1024", 516, 512, 1024, 3, "TT"),
          ("wgrad-512", 512, 512, 516, 3, "FT"), ("wgrad-qkv", 1536, 512, 516, 3, "FT"), ("wgrad-fusion", 512, 512, 258, 1, "FT"))
ap = argparse.ArgumentParser()
ap.add_argument("--only", default=None)
ap.add_argument("--route", type=int, default=None, choices=(0, 2))
ap.add_argument("--launches", type=int, default=30)
opt = ap.parse_args()


def operands(m, n, k, zb, lay):
    ak, bn = lay[0] == "T", lay[1] == "T"
    a = torch.randn((zb, m, k) if ak else (zb, k, m), device=dev)
    b = torch.randn((zb, k, n) if bn else (zb, n, k), device=dev)
    sa = (k, 1, m * k, 0) if ak else (1, m, k * m, 0)
    sb = (n, 1, k * n, 0) if bn else (1, k, n * k, 0)
    ref = torch.bmm(a if ak else a.transpose(1, 2), b if bn else b.transpose(1, 2))
    return a, sa, b, sb, ref


def timed(run, route):
    old = K.lib.cwf_debug_gemm_panel(route)
    try:
        for _ in range(3): run()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        n0 = K.lib.cwf_debug_gemm_panel_launches()
        e0.record()
        for _ in range(opt.launches): run()
        e1.record(); torch.cuda.synchronize()
        took = K.lib.cwf_debug_gemm_panel_launches() - n0
        assert took == (opt.launches if route == 2 else 0), ("route", route, "panel launches", took)
        return e0.elapsed_time(e1) / opt.launches * 1e3
    finally:
        K.lib.cwf_debug_gemm_panel(old)


print("%-12s %5s %5s %5s %2s %3s | %21s | %21s | %13s | %s" % ("shape", "M", "N", "K", "ZB", "lay", "16-byte-load us (x2)", "K-panel us (x2)", "panel / old", "verdict"))
for name, m, n, k, zb, lay in SHAPES:
    if opt.only and name != opt.only:
        continue
    a, sa, b, sb, ref = operands(m, n, k, zb, lay)
    c = torch.empty((zb, m, n), device=dev)
    run = lambda: K.gemm(a, sa, b, sb, c, (n, m * n, 0), m, n, k, zb=zb)
    if opt.route is not None:
        print("%-12s route %d: %7.1f us" % (name, opt.route, timed(run, opt.route)))
        continue
    t, out = {0: [], 2: []}, {}
    for rep in range(2):
        for route in (0, 2):
            c.fill_(float("nan"))
            t[route].append(timed(run, route))
            out[route] = c.clone()
    assert torch.equal(out[0], out[2]), (name, "the routes differ")
    err = float((out[2] - ref).abs().max() / ref.abs().max())
    ratios = [t[2][i] / t[0][i] for i in range(2)]
    print("%-12s %5d %5d %5d %2d %3s | %9.1f %9.1f   | %9.1f %9.1f   | %5.2f  %5.2f  | %s   (%.1f TFLOP/s, err %.1e)" % (
        name, m, n, k, zb, lay, t[0][0], t[0][1], t[2][0], t[2][1], ratios[0], ratios[1], "win" if max(ratios) <= 0.9 else "no",
        2.0 * m * n * k * zb / min(t[2]) / 1e6, err))
