"""float64 numpy restatement of medpy.metric.binary's hd / hd95 (0.4) and of the reference's utils/hausdorff.py wrapper rules -- the
contract the device kernels (csrc/metrics.hip) are tested against.  medpy is not installed; this states what it computes:

  border(M)  = M & ~binary_erosion(M, generate_binary_structure(ndim, connectivity), border_value=0)
  sd(A, B)   = distance_transform_edt(~border(B), sampling)[border(A)]  = min over b in border(B) of sqrt(sum_i (s_i (a_i - b_i))^2),
               the terms summed in axis order
  hd         = max(sd(A, B).max(), sd(B, A).max());  hd95 = np.percentile(np.hstack((sd(A, B), sd(B, A))), 95)

Borders come from shifted comparisons (N-D), surface distances from chunked brute force over border voxels (small volumes or sparse
borders) or, optionally, scipy's EDT (large volumes)."""
import itertools
import math

import numpy as np


def footprint(ndim, connectivity):
    """Neighbour offsets of generate_binary_structure(ndim, connectivity): at most `connectivity` non-zero components."""
    return [o for o in itertools.product((-1, 0, 1), repeat=ndim) if 0 < sum(c != 0 for c in o) <= connectivity]


def shifted(m, off):
    """out[x] = m[x + off], False where x + off lies outside the volume."""
    out = np.zeros_like(m)
    src, dst = [], []
    for o, n in zip(off, m.shape):
        if abs(o) >= n:
            return out
        src.append(slice(max(o, 0), n + min(o, 0)))
        dst.append(slice(max(-o, 0), n - max(o, 0)))
    out[tuple(dst)] = m[tuple(src)]
    return out


def border(m, connectivity=1):
    m = np.asarray(m).astype(bool)
    eroded = m.copy()
    for off in footprint(m.ndim, connectivity):
        eroded &= shifted(m, off)
    return m & ~eroded


def _spacing(spacing, ndim):
    if spacing is None:
        return (1.0,) * ndim
    if np.isscalar(spacing):
        return (float(spacing),) * ndim
    sp = tuple(float(s) for s in spacing)
    assert len(sp) == ndim
    return sp


def sq_distances(pa, pb, spacing, chunk=2048):
    """For each point of pa [n, ndim] the squared distance to the nearest point of pb [m, ndim]: sum_i (s_i * d_i)^2 in axis order."""
    out = np.empty(len(pa), dtype=np.float64)
    pb = pb.astype(np.float64)
    chunk = max(1, min(chunk, (1 << 22) // max(len(pb), 1)))            # at most ~32 MB per term
    for i in range(0, len(pa), chunk):
        a = pa[i:i + chunk].astype(np.float64)
        acc = None
        for ax, s in enumerate(spacing):
            t = (a[:, ax:ax + 1] - pb[None, :, ax]) * s
            t = t * t
            acc = t if acc is None else acc + t
        out[i:i + chunk] = acc.min(axis=1)
    return out


def surface_distances(a, b, spacing=None, connectivity=1, use_scipy=False):
    """medpy's __surface_distances(a, b): distances from border(a) to border(b) (float64)."""
    a, b = np.asarray(a).astype(bool), np.asarray(b).astype(bool)
    if not a.any():
        raise RuntimeError("The first supplied array does not contain any binary object.")
    if not b.any():
        raise RuntimeError("The second supplied array does not contain any binary object.")
    sp = _spacing(spacing, a.ndim)
    ba, bb = border(a, connectivity), border(b, connectivity)
    if use_scipy:
        from scipy.ndimage import distance_transform_edt
        return distance_transform_edt(~bb, sampling=sp)[ba]
    return np.sqrt(sq_distances(np.argwhere(ba), np.argwhere(bb), sp))


def hd_hd95(a, b, spacing=None, connectivity=1, use_scipy=False):
    d1 = surface_distances(a, b, spacing, connectivity, use_scipy)
    d2 = surface_distances(b, a, spacing, connectivity, use_scipy)
    return float(max(d1.max(), d2.max())), float(np.percentile(np.hstack((d1, d2)), 95))


def hd(a, b, spacing=None, connectivity=1, use_scipy=False):
    return hd_hd95(a, b, spacing, connectivity, use_scipy)[0]


def hd95(a, b, spacing=None, connectivity=1, use_scipy=False):
    return hd_hd95(a, b, spacing, connectivity, use_scipy)[1]


def wrapped(which, test, reference, nan_for_nonexisting=False, voxel_spacing=None, connectivity=1, use_scipy=False):
    """The reference's hausdorff_distance (which=0) / hausdorff_distance_95 (which=1): 0 or NaN if either mask is empty or full."""
    t, r = np.asarray(test) != 0, np.asarray(reference) != 0
    if not t.any() or t.all() or not r.any() or r.all():
        return math.nan if nan_for_nonexisting else 0
    return hd_hd95(t, r, voxel_spacing, connectivity, use_scipy)[which]


def regions(labels):
    """[WT, TC, ET] masks of tools.softmax_output_dice."""
    labels = np.asarray(labels)
    return [labels > 0, (labels == 1) | (labels == 3), labels == 3]


def blobs(shape, n, rng, rmin=2.0, rmax=6.0):
    """Union of n random balls (seeded)."""
    grid = np.indices(shape).astype(np.float64)
    m = np.zeros(shape, dtype=bool)
    for _ in range(n):
        c = [rng.uniform(0, s - 1) for s in shape]
        r = rng.uniform(rmin, rmax)
        m |= sum((g - ci) ** 2 for g, ci in zip(grid, c)) <= r * r
    return m


def shell(shape, center, r_out, r_in):
    grid = np.indices(shape).astype(np.float64)
    d2 = sum((g - c) ** 2 for g, c in zip(grid, center))
    return (d2 <= r_out * r_out) & (d2 > r_in * r_in)


def nested_labels(shape, rng, centers=None, scale=1.0):
    """A BraTS-like label map: WT (labels 1, 2, 3) containing TC (1, 3) containing ET (3), as nested random blobs."""
    grid = np.indices(shape).astype(np.float64)
    lab = np.zeros(shape, dtype=np.int64)
    for c in centers or [[rng.uniform(0.3, 0.7) * s for s in shape]]:
        d = np.sqrt(sum((g - ci) ** 2 for g, ci in zip(grid, c)))
        wobble = 1.0 + 0.25 * np.sin(grid[0] * 0.31 + rng.uniform(0, 6)) * np.cos(grid[1] * 0.23 + rng.uniform(0, 6))
        r = rng.uniform(18, 30) * scale
        lab[d * wobble <= r] = 2
        lab[d * wobble <= 0.6 * r] = 1
        lab[d * wobble <= 0.3 * r] = 3
    return lab
