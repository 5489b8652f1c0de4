"""Float64 reference for the sliding-window kernels of csrc/window.hip (a helper module for the tests, not a test file).

What the kernels compute, read from their source:
  cwf_window_gather    windows[j*B + b][l0][l1][l2][c] = x[b][c][s0 + l0][s1 + l1][s2 + l2], 0 outside the volume -- a copy, exact.
  cwf_window_blend     for each voxel v and each window k covering it, in window order:
                           wt_k = fp32(fp32(g0[l0] * g1[l1]) * g2[l2])        (g_a: the fp32 1-D tables, l = v - s_k)
                           acc  = fp32(acc + fp32(wt_k * p_k))                 (acc starts at 0 in the first chunk)
  cwf_window_finalize  wsum = fp32(wsum + wt_k) over the same windows in the same order (from 0), y = fp32(acc / wsum).
  The file is built with -ffp-contract=off (no fused multiply-add) and fp32 division is correctly rounded.

The reference (`blend_loop`, `blend_voxel`) forms w_k = g0 g1 g2 from the same fp32 table values and
    ref = sum_k w_k p_k / sum_k w_k
in float64.  Bound, with u = 2^-24, gamma_n = n u / (1 - n u) (Higham, Accuracy and Stability of Numerical Algorithms, 3.1) and
k = the most windows covering one voxel:
  * wt_k = w_k (1 + a)(1 + b), |a|, |b| <= u (two product roundings).
  * acc: each term wt_k p_k is rounded once more and then takes part in at most k - 1 roundings of additions (0 + t is exact), so
    acc_got = sum_k w_k p_k (1 + t_k), |t_k| <= gamma_{k+2}.  Every term is >= 0 (w > 0, p in [0, 1]), hence
    acc_got = acc (1 + T), |T| <= gamma_{k+2}: the sum of the perturbations is a weighted mean of the t_k.
  * wsum: the same without the probability product: wsum_got = wsum (1 + S), |S| <= gamma_{k+1}.
  * y = acc_got / wsum_got (1 + d), |d| <= u, so y / ref - 1 lies within (1 + gamma_{k+2})(1 + u) / (1 - gamma_{k+1}) - 1 (= `rel(k)`,
    about (2k + 4) u).
  * ref is a weighted mean of values in [0, 1], so ref <= 1 and |y - ref| <= rel(k) =: gamma(k) elementwise.  The reference's own
    float64 roundings (the triple product, k additions, one division: about (2k + 4) 2^-53 relative) add `SLACK`.
A chunk split does not enter: the kernel stores acc in fp32 between chunks, which is the rounding it makes anyway.
The bound holds for any p in [0, 1]; for probabilities of the model (softmax outputs) it is the bound the tests use.
"""
from __future__ import annotations

import itertools

import numpy as np

U = 2.0 ** -24
SLACK = 1e-12


def gamma_n(n):
    return n * U / (1.0 - n * U)


def gamma(k):
    """elementwise bound |kernel - reference| for at most k windows covering a voxel and p in [0, 1]"""
    return (1.0 + gamma_n(k + 2)) * (1.0 + U) / (1.0 - gamma_n(k + 1)) - 1.0 + SLACK


def windows(starts):
    """window start triples in window order (axis 0 slowest)"""
    return list(itertools.product(*starts))


def _clip(s, r, size):
    """the part [lo, hi) of window [s, s + r) inside [0, size), and its offset in the window"""
    lo, hi = max(s, 0), min(s + r, size)
    return lo, hi, lo - s


def coverage(shape, roi, starts):
    """[S0, S1, S2] int: how many windows cover each voxel"""
    cnt = np.zeros(shape, np.int64)
    for s in windows(starts):
        sl = tuple(slice(*_clip(s[a], roi[a], shape[a])[:2]) for a in range(3))
        cnt[sl] += 1
    return cnt


def max_coverage(shape, roi, starts):
    return int(coverage(shape, roi, starts).max())


def weights3(tables):
    """float64 [r0, r1, r2] = g0 g1 g2 of the fp32 table values"""
    g0, g1, g2 = (np.asarray(t, np.float64) for t in tables)
    return g0[:, None, None] * g1[None, :, None] * g2[None, None, :]


def gather(x, starts, roi):
    """x [B, C, S0, S1, S2] -> [nw, B, C, r0, r1, r2] windows in window order, zeros outside the volume (dtype of x)"""
    x = np.asarray(x)
    shape = x.shape[2:]
    out = np.zeros((len(windows(starts)),) + x.shape[:2] + tuple(roi), x.dtype)
    for w, s in enumerate(windows(starts)):
        src, dst = [], []
        for a in range(3):
            lo, hi, off = _clip(s[a], roi[a], shape[a])
            src.append(slice(lo, hi)); dst.append(slice(off, off + hi - lo))
        out[(w, slice(None), slice(None)) + tuple(dst)] = x[(slice(None), slice(None)) + tuple(src)]
    return out


def blend_loop(probs, starts, roi, shape, tables, skip=()):
    """Per-window loop form.  probs [nw, B, C, r0, r1, r2] (window order; an array or a list of per-window arrays) ->
    (acc [B, C, S...], wsum [S...]) in float64.  skip: window indices left out of acc (not of wsum) -- only for planting defects."""
    wt = weights3(tables)
    acc = np.zeros(np.shape(probs[0])[:2] + tuple(shape))
    wsum = np.zeros(tuple(shape))
    for w, s in enumerate(windows(starts)):
        src, dst = [], []
        for a in range(3):
            lo, hi, off = _clip(s[a], roi[a], shape[a])
            dst.append(slice(lo, hi)); src.append(slice(off, off + hi - lo))
        src, dst = tuple(src), tuple(dst)
        wsum[dst] += wt[src]
        if w not in skip:
            acc[(slice(None), slice(None)) + dst] += wt[src] * np.asarray(probs[w], np.float64)[(slice(None), slice(None)) + src]
    return acc, wsum


def finalize(acc, wsum):
    return acc / wsum


def blend(probs, starts, roi, shape, tables):
    """reference probability volume [B, C, S0, S1, S2] (float64)"""
    return finalize(*blend_loop(probs, starts, roi, shape, tables))


def blend_voxel(probs, starts, roi, shape, tables):
    """Per-voxel form (as the kernels walk it: each voxel visits the windows covering it in window order).  Small volumes only."""
    probs = np.asarray(probs, np.float64)
    wt = weights3(tables)
    wins = windows(starts)
    out = np.zeros(probs.shape[1:3] + tuple(shape))
    for v in itertools.product(*(range(n) for n in shape)):
        acc = np.zeros(probs.shape[1:3])
        ws = 0.0
        for w, s in enumerate(wins):
            l = tuple(v[a] - s[a] for a in range(3))
            if all(0 <= l[a] < roi[a] for a in range(3)):
                acc += wt[l] * probs[(w, slice(None), slice(None)) + l]
                ws += wt[l]
        out[(slice(None), slice(None)) + v] = acc / ws
    return out


def excess(got, ref, k):
    """max |got - ref| / gamma(k); inf where either is not finite (a NaN never passes)"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    if not (np.isfinite(got).all() and np.isfinite(ref).all()):
        return float("inf")
    return float(np.abs(got - ref).max() / gamma(k))


def softmax4(x):
    """per-voxel softmax over axis 1 (the pointwise stand-in model), float64"""
    x = np.asarray(x, np.float64)
    e = np.exp(x - x.max(axis=1, keepdims=True))
    return e / e.sum(axis=1, keepdims=True)
