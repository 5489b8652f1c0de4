"""Restatement of what csrc/components.hip and predict_overlap.postprocess compute -- the contract the kernels are tested against.

  label(mask, c)       scipy.ndimage.label under generate_binary_structure(3, c): components numbered 1..K in increasing order of their
                       smallest linear (C-order) voxel index
  sizes / largest      voxel counts per component, zero-padded to cap = (V + 1) // 2; (label, size) of the largest, ties to the lowest
  postprocess(seg, ..) the policy, rule by rule, on [B, D0, D1, D2] label maps (classes 0..3, WT = seg > 0, ET = seg == 3):
      1  every WT component of fewer than min_component voxels is set to 0
      2  keep_largest: only the largest surviving WT component is kept (ties: lowest label), everything else set to 0
      3  every ET component of fewer than et_min_component voxels is relabelled et_replace
      4  if fewer than et_min_voxels ET voxels remain after rules 1-3, all of them are relabelled et_replace
    each rule off at 0 / False; stats per sample = WT voxels removed, WT components removed, ET voxels relabelled, ET voxels remaining."""
import numpy as np
from scipy import ndimage


def label(mask, connectivity=1):
    mask = np.asarray(mask).astype(bool)
    lab, k = ndimage.label(mask, structure=ndimage.generate_binary_structure(mask.ndim, connectivity))
    return lab.astype(np.int32), int(k)


def sizes(lab, k, cap=None):
    """Entry j - 1 = voxels of component j; zeros up to cap (default (V + 1) // 2)."""
    cap = (lab.size + 1) // 2 if cap is None else cap
    out = np.zeros(cap, dtype=np.int32)
    out[:k] = np.bincount(lab.ravel(), minlength=k + 1)[1:k + 1]
    return out


def largest(size):
    """(label, size) of the largest component, the lowest label among equals; (0, 0) when there is none."""
    if size.size == 0 or size.max() == 0:
        return (0, 0)
    j = int(np.argmax(size))                  # the first maximum
    return (j + 1, int(size[j]))


def first_indices(lab, k):
    """Smallest linear index of every component 1..K."""
    flat = lab.ravel()
    first = np.full(k + 1, flat.size, dtype=np.int64)
    np.minimum.at(first, flat, np.arange(flat.size))
    return first[1:]


def postprocess(seg, min_component=0, keep_largest=False, et_min_component=0, et_min_voxels=0, et_replace=1, connectivity=1):
    seg = np.asarray(seg)
    out = seg.copy()
    stats = np.zeros((seg.shape[0], 4), dtype=np.int64)
    for b in range(seg.shape[0]):
        s = out[b]
        lab, k = label(s > 0, connectivity)                     # WT components of the input
        size = sizes(lab, k, cap=max(k, 1))
        alive = np.ones(k, dtype=bool)
        if min_component > 0:                                   # rule 1
            alive &= size[:k] >= min_component
        if keep_largest and alive.any():                        # rule 2, among the survivors of rule 1
            best = int(np.argmax(np.where(alive, size[:k], -1)))
            alive = np.zeros(k, dtype=bool)
            alive[best] = True
        gone = (lab > 0) & ~np.concatenate(([True], alive))[lab]
        stats[b, 0], stats[b, 1] = int(gone.sum()), int(k - alive.sum())
        s[gone] = 0
        if et_min_component > 0:                                # rule 3, on what rules 1-2 left
            lab, k = label(s == 3, connectivity)
            size = sizes(lab, k, cap=max(k, 1))
            hit = (lab > 0) & np.concatenate(([False], size[:k] < et_min_component))[lab]
            stats[b, 2] = int(hit.sum())
            s[hit] = et_replace
        left = int((s == 3).sum())                              # rule 4
        if et_min_voxels > 0 and left < et_min_voxels:
            s[s == 3] = et_replace
            stats[b, 2] += left
            left = 0
        stats[b, 3] = left
    return out, stats


# ---------------------------------------------------------------------------------------------------------------------- test masks
def serpentine(shape):
    """A one-voxel-wide path that crosses the whole volume back and forth: full rows along axis 2 on every second (i0, i1) line of
    every second plane, joined at alternating ends, the planes joined by single voxels -- one component under every connectivity."""
    d0, d1, d2 = shape
    m = np.zeros(shape, dtype=bool)
    end = 0                                   # which i2 end the next connector sits at
    rows = list(range(0, d1, 2))
    for k, i0 in enumerate(range(0, d0, 2)):
        order = rows if k % 2 == 0 else rows[::-1]
        for n, i1 in enumerate(order):
            m[i0, i1, :] = True
            if n + 1 < len(order):            # connector to the next row of the plane
                step = 1 if order[n + 1] > i1 else -1
                m[i0, i1 + step, -1 if end else 0] = True
                end ^= 1
        if i0 + 2 < d0:                       # connector to the next plane, at the end the path has reached
            m[i0 + 1, order[-1], -1 if end else 0] = True
            end ^= 1
    return m


def checkerboard(shape):
    return (np.indices(shape).sum(axis=0) % 2) == 0
