"""Time the intensity stage of the batch preparation (HipBackend.prepare_batch with blur / noise / gamma, csrc/intensity.hip
cwf_augment_intensity) for 128^3 crops of 240 x 240 x 155 subjects at B = 2 and B = 8: the plain preparation (draw_params(flip,
intensity 0.1)), and the same with noise (sigma 0.1), with blur (sigma 1.0), with gamma (exponent 0.8) and with all three, each
switched on for all four channels of every sample -- the most the stage can be asked for (draw_params switches a channel on with
probability 1/2).  A variant's time less the plain preparation's is the stage's cost; it is printed beside
  * the floor of a stage that reads x once and writes it once, 2 * B * 4 * 128^3 * 4 B (134 MB at B = 2) at 6.3 TB/s, the
    achievable HBM rate of MI355X_MICROARCH.md (gamma reads x a second time and writes it a second time: its floor is twice that), and
  * a torch baseline on the same x in the same run: three depthwise conv3d passes over a replicate-padded x, randn_like times sigma
    added in place, amin / amax per channel and pow on the normalised channel.

Each figure is the median over --repeats windows of --iters back-to-back calls between device events; the variants alternate
inside every repeat, and the spread (max - min over the median) is printed with it.  Beside it stands the host's time to enqueue a
call (a clock around the same loop, read before the synchronise): where the two are about equal the window measured the host, and
the device's share is smaller than the figure.  Nothing is asserted.

--powf instead measures the largest distance, in float32 ulps of the float64 result, of the device's powf from the float64 pow over
u in [0, 1] and gamma in [0.5, 2]: channels that hold 0, 1 and 2^20 - 2 other values of u go through the stage's gamma alone, where
mn = 0 and r = 1 make the result powf(u, gamma) itself.
usage: python tools/intensity_prep_micro.py [--iters N] [--repeats R] [--powf]"""
import argparse
import ctypes
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "decouple-and-couple_learning_in_multi-modal_brain_tumor_segmentation_amd"))
sys.path.insert(0, os.path.join(REPO, "tools"))

from affine_prep_micro import CROP, SRC  # noqa: E402
from cwf import _lib  # noqa: E402
from cwf.kernels import backend  # noqa: E402
from utils import data  # noqa: E402

HBM = 6.3e12        # achievable HBM bytes/s (MI355X_MICROARCH.md)


def timed(fn, iters):
    """(us per call between device events, us per call the host took to enqueue)"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    host = time.perf_counter() - t0
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters, host * 1e6 / iters


def powf_distance(be):
    crop = (64, 128, 128)
    n = crop[0] * crop[1] * crop[2]
    gen = torch.Generator(device="cuda").manual_seed(1)
    gammas = sorted(set(np.linspace(0.5, 2.0, 61, dtype=np.float32).tolist() + [0.5, 1.0, 2.0, float(np.float32(1.0 / 3.0)) + 0.5]))
    gammas += [gammas[-1]] * (-len(gammas) % 4)
    ws = torch.empty(_lib.intensity_ws_floats(1, crop), device="cuda")
    worst = (0.0, None, None)
    for k in range(0, len(gammas), 4):
        x = torch.rand((4, n), device="cuda", generator=gen)
        x[1] = x[1] * x[1] * x[1]                                   # more small u
        x[2] = 1.0 - x[2] * x[2] * 0.01                             # u near 1
        x[3, : n // 2] = torch.exp2(-126.0 * torch.rand(n // 2, device="cuda", generator=gen))     # down to the smallest normal
        x[:, 0], x[:, 1] = 0.0, 1.0
        u = x.clone()
        smp = (_lib.IntensitySample * 1)()
        smp[0].gam = 15
        smp[0].gamma[:] = gammas[k:k + 4]
        be._call("cwf_augment_intensity", ctypes.addressof(smp), 1, crop[0], crop[1], crop[2], x.data_ptr(), 4 * n, x.data_ptr(), 4 * n,
                 ws.data_ptr(), ws.numel(), be._stream())
        g = torch.tensor(gammas[k:k + 4], dtype=torch.float32, device="cuda").double().reshape(4, 1)
        ref = u.double().pow(g)
        ulp = torch.ldexp(torch.ones_like(ref), (torch.frexp(ref)[1] - 24).clamp(min=-149))
        d = (x.double() - ref).abs() / ulp
        for c in range(4):
            i = int(d[c].argmax())
            if float(d[c, i]) > worst[0]:
                worst = (float(d[c, i]), float(u[c, i]), gammas[k + c])
    print("powf: largest |powf(u, g) - pow64(u, g)| = %.4f ulp32 at u = %.9g, g = %.9g (%d exponents in [0.5, 2] x %d values of u "
          "in [0, 1])" % (worst + (len(set(gammas)), n)), flush=True)


def torch_baseline(x, taps, sigma, g):
    """the three transforms on x [B, 4, *CROP] with torch operators (its own definitions of the border and the noise)"""
    F = torch.nn.functional

    def blur():
        y = x
        for axis in (2, 1, 0):
            pad = [0, 0, 0, 0, 0, 0]
            pad[2 * (2 - axis)] = pad[2 * (2 - axis) + 1] = 3
            shape = [4, 1, 1, 1, 1]
            shape[2 + axis] = 7
            y = F.conv3d(F.pad(y, pad, mode="replicate"), taps.reshape(shape), groups=4)
        return y

    def noise(y=None):
        y = x if y is None else y
        return y.add_(torch.randn_like(y), alpha=sigma)

    def gamma(y=None):
        y = x if y is None else y
        mn, mx = y.amin(dim=(2, 3, 4), keepdim=True), y.amax(dim=(2, 3, 4), keepdim=True)
        return ((y - mn) / (mx - mn)).pow_(g).mul_(mx - mn).add_(mn)

    return {"torch blur": blur, "torch noise": noise, "torch gamma": gamma, "torch all": lambda: gamma(noise(blur()))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--powf", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("intensity_prep_micro: no GPU; nothing is measured without one")
    be = backend()
    if args.powf:
        powf_distance(be)
        return 0
    gen = torch.Generator(device="cuda").manual_seed(0)
    imgs = [torch.randn((4,) + SRC, device="cuda", generator=gen) for _ in range(8)]
    labs = [torch.randint(0, 5, SRC, device="cuda", generator=gen).to(torch.uint8) for _ in range(8)]
    sig_b, sig_n, g = 1.0, 0.1, 0.8
    on = {"plain": {}, "noise": dict(noise=(sig_n,) * 4, noise_key=12345), "blur": dict(blur=(sig_b,) * 4), "gamma": dict(gamma=(g,) * 4)}
    on["all"] = dict(on["noise"], **on["blur"], **on["gamma"])
    for nb in (2, 8):
        out = (torch.empty((nb, 4) + CROP, device="cuda"), torch.empty((nb,) + CROP, dtype=torch.int64, device="cuda"),
               torch.empty((nb,) + CROP, dtype=torch.int64, device="cuda"))
        base = [data.draw_params(1000, 0, i, SRC, CROP, flip=True, intensity=0.1) for i in range(nb)]
        variants = {}
        for name, kw in on.items():
            ps = [data.AugParams(p.origin, p.flip, p.scale, p.shift, **kw) for p in base]
            variants[name] = (lambda ps=ps: be.prepare_batch(imgs[:nb], labs[:nb], ps, CROP, out=out))
        x = be.prepare_batch(imgs[:nb], labs[:nb], base, CROP)[0]
        taps = torch.from_numpy(np.tile(data.blur_taps(sig_b), (4, 1))).cuda()
        variants.update(torch_baseline(x, taps, sig_n, g))
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
            print("B=%d %-12s %9.1f us per batch (median of %d x %d calls; min %.1f max %.1f; spread %.1f %%; host enqueue %.1f us)"
                  % (nb, k, med[k], args.repeats, args.iters, min(times[k]), max(times[k]), 100 * (max(times[k]) - min(times[k])) / med[k],
                     float(np.median(host[k]))), flush=True)
        floor = 2 * nb * 4 * CROP[0] * CROP[1] * CROP[2] * 4 / HBM * 1e6
        for k in ("noise", "blur", "gamma", "all"):
            cost, passes = med[k] - med["plain"], 2 if k in ("gamma", "all") else 1
            print("B=%d stage %-6s %9.1f us over plain = %.2f x its floor of %.1f us (%d read and write of x at 6.3 TB/s) = %.3f x torch %s "
                  "(%.1f us)" % (nb, k, cost, cost / (passes * floor), passes * floor, passes, cost / med["torch " + k], k, med["torch " + k]),
                  flush=True)
        del x, variants
    return 0


if __name__ == "__main__":
    sys.exit(main())
