"""Restatement of the intensity stage of the batch preparer (include/cwf_hip.h cwf_augment_intensity, utils.data._intensity_stage_cpu)
that shares no code with utils.data: the blur one output voxel at a time on numpy float32 scalars in the order the statement writes
it, the noise on Python integers, and the float64 sides the tests bound against -- the same seven float32 taps applied by
scipy.ndimage.correlate1d(mode="nearest") in float64, and the gamma map with a float64 pow on the statement's float32 u, r, mn."""
import math

import numpy as np
from scipy import ndimage

F = np.float32
RADIUS = 3
M64 = (1 << 64) - 1
NOISE_DIV = math.sqrt((65536.0 ** 2 - 1.0) / 3.0)


def taps(sigma):
    """float32 [7] from the float32 sigma, in float64"""
    sg = float(F(sigma))
    e = [math.exp(-0.5 * ((j - RADIUS) / sg) ** 2) for j in range(2 * RADIUS + 1)]
    return np.array([v / sum(e) for v in e], dtype=np.float64).astype(F)


def blur_pass(a, w, axis):
    """one pass along `axis`, every product and sum rounded to float32, indices clamped"""
    a = np.moveaxis(np.asarray(a, dtype=F), axis, -1)
    n = a.shape[-1]
    y = np.empty_like(a)
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        for i in np.ndindex(a.shape[:-1]):
            row = a[i]
            for p in range(n):
                t = [F(w[j] * row[min(max(p + j - RADIUS, 0), n - 1)]) for j in range(2 * RADIUS + 1)]
                acc = F(t[0] + t[1])
                for j in range(2, 2 * RADIUS + 1):
                    acc = F(acc + t[j])
                y[i + (p,)] = acc
    return np.moveaxis(y, -1, axis)


def blur(a, sigma):
    w = taps(sigma)
    for axis in (2, 1, 0):
        a = blur_pass(a, w, axis)
    return np.ascontiguousarray(a)


def blur64(a, w):
    """the separable filter in float64 with the float32 taps w, axis 2, then 1, then 0"""
    y = np.asarray(a, dtype=np.float64)
    for axis in (2, 1, 0):
        y = ndimage.correlate1d(y, np.asarray(w, dtype=np.float64), axis=axis, mode="nearest")
    return y


def splitmix64(z):
    z = (z + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def noise_int(key, counter):
    h = splitmix64((int(key) + int(counter)) & M64)
    return (h & 0xFFFF) + ((h >> 16) & 0xFFFF) + ((h >> 32) & 0xFFFF) + (h >> 48) - 131070


def noise_amp(sigma):
    return F(float(F(sigma)) / NOISE_DIV)


def add_noise(x, c, sigma, key):
    """channel c of a crop whose channels have x.size voxels each"""
    V, amp = x.size, noise_amp(sigma)
    s = np.array([noise_int(key, c * V + v) for v in range(V)], dtype=np.int64).astype(F).reshape(x.shape)
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        return (np.asarray(x, dtype=F) + (s * amp).astype(F)).astype(F)


def blur_noise(x, blur_sigma, noise_sigma, key):
    """steps 1 and 2 of the stage on x [4, C0, C1, C2]; sigmas are 4 values each or None"""
    x = np.array(x, dtype=F)
    for c in range(4):
        if blur_sigma is not None and blur_sigma[c] > 0:
            x[c] = blur(x[c], blur_sigma[c])
        if noise_sigma is not None and noise_sigma[c] > 0:
            x[c] = add_noise(x[c], c, noise_sigma[c], key)
    return x


def gamma_parts(pre):
    """(mn, r, u) of the statement, float32, from a channel after steps 1 and 2; r is None when the channel stays as it is"""
    pre = np.asarray(pre, dtype=F)
    mn, mx = np.nanmin(pre), np.nanmax(pre)
    r = F(mx - mn)
    if not (np.isfinite(r) and r > 0):
        return mn, None, None
    return mn, r, ((pre - mn) / r).astype(F)


def gamma64(pre, g):
    """(y, ref, r) in float64: y = pow(u, g) and ref = y * r + mn on the statement's float32 u, r, mn and the float32 exponent"""
    mn, r, u = gamma_parts(pre)
    y = np.power(u.astype(np.float64), float(F(g)))
    return y, y * float(r) + float(mn), float(r)


def ulp32(v):
    return np.spacing(np.abs(np.asarray(v, dtype=np.float64)).astype(F)).astype(np.float64)
