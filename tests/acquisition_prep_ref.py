"""Restatement of the acquisition stage of the batch preparer (include/cwf_hip.h cwf_augment_acquisition: bias field, contrast,
low-resolution simulation), written from the definitions and sharing no code with utils.data.  The per-axis quantities (spline
weights, control indices, lattice taps and fractions) are formed one coordinate at a time on numpy float32 scalars; the per-voxel
formulas are then written out voxel-wise -- the 64 control points of a voxel, its eight lattice taps -- over index arrays of the whole
crop, every operation on float32 arrays, so each product and sum is rounded once, in the order the statement writes it."""
import math

import numpy as np

F = np.float32
U = 2.0 ** -24


def spline_axis(C, G):
    """(w float32 [C, 4], control index int [C, 4]) of the cubic B-spline at the crop indices 0..C-1 of an axis with G control points"""
    k = F(G - 3) / F(C - 1) if C > 1 else F(0.0)
    w, ix = np.zeros((C, 4), dtype=F), np.zeros((C, 4), dtype=np.int64)
    h = F(1.0 / 6.0)
    for p in range(C):
        g = F(F(F(p) * k) + F(1.0))
        i = int(math.floor(float(g)))
        t = F(g - F(i))
        s = F(F(1.0) - t)
        w[p, 0] = F(F(F(s * s) * s) * h)
        w[p, 1] = F(F(F(F(F(F(F(3.0) * t) - F(6.0)) * t) * t) + F(4.0)) * h)
        w[p, 2] = F(F(F(F(F(F(F(F(-3.0) * t) + F(3.0)) * t) + F(3.0)) * t) + F(1.0)) * h)
        w[p, 3] = F(F(F(t * t) * t) * h)
        ix[p] = [min(max(i - 1 + j, 0), G - 1) for j in range(4)]
    return w, ix


def sum4(v):
    return ((v[0] + v[1]) + v[2]) + v[3]


def bias_field(grid, crop):
    """m [*crop] float32: at every voxel sum_j0 w0 * (sum_j1 w1 * (sum_j2 w2 * grid[i0+j0][i1+j1][i2+j2]))"""
    grid = np.asarray(grid, dtype=F)
    (w0, i0), (w1, i1), (w2, i2) = (spline_axis(crop[d], grid.shape[d]) for d in range(3))
    outer = []
    for j0 in range(4):
        mid = []
        for j1 in range(4):
            inner = sum4([w2[None, None, :, j2] * grid[i0[:, j0][:, None, None], i1[:, j1][None, :, None], i2[:, j2][None, None, :]]
                          for j2 in range(4)])
            mid.append(w1[None, :, None, j1] * inner)
        outer.append(w0[:, None, None, j0] * sum4(mid))
    m = sum4(outer)
    assert m.dtype == F
    return m


def weight_sums(crop, G):
    """per axis, the exact (float64) sums of the four float32 weights at every crop index"""
    return [spline_axis(crop[d], G[d])[0].astype(np.float64).sum(axis=1) for d in range(3)]


def contrast_parts(a):
    """(mean float32, mn, mx) of one channel: the float64 sum over V rounded to float32, the NaN-ignoring extremes"""
    flat = np.ascontiguousarray(a, dtype=F).reshape(-1)
    mean = F(flat.astype(np.float64).sum() / flat.size)
    return mean, np.fmin.reduce(flat), np.fmax.reduce(flat)


def contrast(a, f, mean=None):
    m, mn, mx = contrast_parts(a)
    mean = m if mean is None else F(mean)
    if not np.isfinite(mean):
        return a.copy()
    with np.errstate(over="ignore", invalid="ignore"):
        return np.minimum(np.maximum(((a - mean) * F(f)) + mean, mn), mx).astype(F)


def lattice(crop, z):
    z = float(F(z))
    return tuple(min(C, max(1, int(math.floor(float(C) * z + 0.5)))) for C in crop)


def lowres_axis(C, n):
    """(lo, hi) crop indices of the two taps and t float32, at the crop indices 0..C-1"""
    lo, hi, t = np.zeros(C, dtype=np.int64), np.zeros(C, dtype=np.int64), np.zeros(C, dtype=F)
    r = F(n) / F(C)
    for p in range(C):
        u = F(F(F(F(p) + F(0.5)) * r) - F(0.5))
        u = min(max(u, F(0.0)), F(n - 1))
        k = 0 if n == 1 else min(int(math.floor(float(u))), n - 2)
        k1 = min(k + 1, n - 1)
        t[p] = F(u - F(k))
        lo[p], hi[p] = ((2 * k + 1) * C) // (2 * n), ((2 * k1 + 1) * C) // (2 * n)
        assert 0 <= lo[p] < C and 0 <= hi[p] < C
    return lo, hi, t


def lowres(a, n):
    """one channel through the lattice n = (n_0, n_1, n_2): eight taps per voxel, lerp along axis 2, then 1, then 0"""
    C = a.shape
    (l0, h0, t0), (l1, h1, t1), (l2, h2, t2) = (lowres_axis(C[d], n[d]) for d in range(3))
    i0, i1, i2 = ((l0, h0), (l1, h1), (l2, h2))

    def tap(d0, d1, d2):
        return a[i0[d0][:, None, None], i1[d1][None, :, None], i2[d2][None, None, :]]

    def lerp(lo, hi, t):
        return lo + t * (hi - lo)

    with np.errstate(over="ignore", invalid="ignore"):
        r1 = {(d0, d1): lerp(tap(d0, d1, 0), tap(d0, d1, 1), t2[None, None, :]) for d0 in (0, 1) for d1 in (0, 1)}
        r0 = [lerp(r1[d0, 0], r1[d0, 1], t1[None, :, None]) for d0 in (0, 1)]
        y = lerp(r0[0], r0[1], t0[:, None, None])
    assert y.dtype == F
    return y


def stage(x, bias=None, bias_mask=(False,) * 4, factor=None, zoom=None):
    """x [4, *crop] float32 -> the stage's output (a new array): bias field, then contrast, then low resolution, per channel"""
    x = np.array(x, dtype=F, order="C")
    crop = x.shape[1:]
    for c in range(4):
        if bias is not None and bias_mask[c]:
            x[c] = x[c] * bias_field(bias[c], crop)
        if factor is not None and factor[c] > 0.0:
            x[c] = contrast(x[c], factor[c])
        if zoom is not None and zoom[c] > 0.0:
            x[c] = lowres(x[c], lattice(crop, zoom[c]))
    return x


def random_bias(G, rng, b=0.7):
    """control multipliers float32 [4, *G] = exp(U(-b, b))"""
    return np.exp(rng.uniform(-b, b, (4,) + tuple(G))).astype(F)


def ulp32(v):
    """the spacing of float32 at |v| (the smallest normal's for smaller values)"""
    a = np.maximum(np.abs(np.asarray(v, dtype=np.float64)), 2.0 ** -126)
    return 2.0 ** (np.floor(np.log2(a)) - 23)
