"""The float-free statement of the nonzero box (csrc/nonzero_box.hip, utils.data.nonzero_box, predict_overlap.nonzero_box), of the
origin range of utils.data.box_crop_origin, and the crop-and-paste statement of sliding_window_inference(crop_nonzero=True).  Nothing
here imports the code under test; floats are looked at as their 32 bits only."""
import numpy as np

import sliding_window_ref as R


def nonzero_mask(x):
    """bool [S0, S1, S2] of x float32 [4, S0, S1, S2]: some channel has (bits & 0x7fffffff) != 0"""
    bits = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    return ((bits & np.uint32(0x7FFFFFFF)) != 0).any(axis=0)


def box_count(x):
    """(box int32 [6] = lo | hi with hi exclusive, count) of one sample x [4, S0, S1, S2]; lo = S, hi = 0, count = 0 when empty"""
    m = nonzero_mask(x)
    idx = np.nonzero(m)
    if idx[0].size == 0:
        return np.array(list(m.shape) + [0, 0, 0], dtype=np.int32), 0
    return np.array([int(i.min()) for i in idx] + [int(i.max()) + 1 for i in idx], dtype=np.int32), int(idx[0].size)


def boxes_counts(x):
    """(int32 [B, 6], int64 [B]) of a batch x [B, 4, S0, S1, S2]"""
    res = [box_count(s) for s in x]
    return np.stack([r[0] for r in res]), np.array([r[1] for r in res], dtype=np.int64)


def brute_box_count(x):
    """box_count by a loop over the voxels, testing sign-stripped bits with Python integers (tiny volumes only)"""
    bits = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    S = x.shape[1:]
    lo, hi, n = list(S), [0, 0, 0], 0
    for i in range(S[0]):
        for j in range(S[1]):
            for k in range(S[2]):
                if any((int(bits[c, i, j, k]) & 0x7FFFFFFF) != 0 for c in range(4)):
                    n += 1
                    for d, v in enumerate((i, j, k)):
                        lo[d], hi[d] = min(lo[d], v), max(hi[d], v + 1)
    return np.array(lo + hi, dtype=np.int32), n


def union_box(boxes, shape, margin=0):
    """(lo, hi) tuples: the union of the non-empty rows of boxes [B, 6], grown by margin per side and clipped to the volume; None when
    every row is empty"""
    rows = [b for b in np.asarray(boxes) if int(b[3]) > 0]
    if not rows:
        return None
    lo = [max(min(int(b[d]) for b in rows) - margin, 0) for d in range(3)]
    hi = [min(max(int(b[3 + d]) for b in rows) + margin, int(shape[d])) for d in range(3)]
    return tuple(lo), tuple(hi)


def origin_range(s, c, a, b):
    """the inclusive range [first, last] of box_crop_origin along one axis: extent s, crop c, box [a, b)"""
    top = max(s - c, 0)
    lo, hi = (a, b - c) if b - a >= c else (b - c, a)
    return max(lo, 0), min(hi, top)


def overlap(o, c, a, b):
    """|[o, o + c) n [a, b)|"""
    return max(min(o + c, b) - max(o, a), 0)


def paste(inner, full_shape, lo):
    """inner [B, 4, *box extent] pasted at lo into a [B, 4, *full_shape] volume of the background one-hot (1, 0, 0, 0)"""
    out = np.zeros(inner.shape[:2] + tuple(full_shape), dtype=inner.dtype)
    out[:, 0] = 1
    sl = tuple(slice(a, a + n) for a, n in zip(lo, inner.shape[2:]))
    out[(slice(None), slice(None)) + sl] = inner
    return out


def crop_and_paste(x, box, infer):
    """The statement of sliding_window_inference(crop_nonzero=True): x [B, 4, S] (numpy) cropped to box = (lo, hi) as a contiguous
    array, infer(crop) -> [B, 4, box extent] (today's sliding window on the crop), pasted into background."""
    lo, hi = box
    crop = np.ascontiguousarray(x[:, :, lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]])
    return paste(np.asarray(infer(crop)), x.shape[2:], lo)


def gather_box(x, box, starts, roi):
    """cwf_window_gather_box's statement: sliding_window_ref.gather of the contiguous crop of x to box, [nw, B, 4, r0, r1, r2]"""
    lo, hi = box
    return R.gather(np.ascontiguousarray(x[:, :, lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]]), starts, roi)


def window_count(extent, roi, overlap_frac, window_grid):
    """the number of windows window_grid plans over a volume of `extent`"""
    return len(R.windows(window_grid(extent, roi, overlap_frac)))
