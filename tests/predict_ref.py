"""The statement of the prediction and evaluation glue (csrc/predict.hip: cwf_stitch_windows, cwf_argmax_dice, cwf_argmax_metrics;
csrc/components.hip: cwf_label_metrics; csrc/metrics.hip: cwf_region_bits): the argmax over four classes, the exact Dice / IoU count
table, the two float64 quotients, the region bits of a label and the index rule of the eight-window stitch.  Plain numpy and Python
integers; nothing here imports the code under test."""
import numpy as np

REGIONS = ("WT", "TC", "ET", "class 1", "class 2", "class 3")
EPS = 1e-8


def argmax4(p, axis=1):
    """int64 index of the first maximum of p along the class axis (four classes), with torch.argmax's order of the values: NaN ranks
    above everything (+inf included) and the first NaN wins; -0.0 == +0.0; a row of equal values gives 0."""
    p = np.moveaxis(np.asarray(p), axis, 0)
    assert p.shape[0] == 4
    nan = np.isnan(p)
    finite_max = np.where(nan, -np.inf, p).max(axis=0)
    top = np.where(nan.any(axis=0), nan, p == finite_max)           # the entries that hold the maximum: every NaN, or every equal of the max
    best = np.full(p.shape[1:], 4, dtype=np.int64)
    for c in (3, 2, 1, 0):                                          # the first of them
        best = np.where(top[c], c, best)
    assert int(best.max(initial=0)) < 4
    return best


def _region_masks(x):
    """the six masks of utils/tools.py on the full int64 value: WT > 0, TC == 1 or == 3, ET == 3, class k == k"""
    x = np.asarray(x)
    assert x.dtype == np.int64
    return [x > 0, (x == 1) | (x == 3), x == 3, x == 1, x == 2, x == 3]


def counts(seg, target):
    """int64 [6][3]: (|o & t|, |o|, |t|) for WT, TC, ET and the classes 1, 2, 3 of two int64 label maps of one shape"""
    seg, target = np.asarray(seg), np.asarray(target)
    assert seg.shape == target.shape
    table = [[int(np.count_nonzero(o & t)), int(np.count_nonzero(o)), int(np.count_nonzero(t))]
             for o, t in zip(_region_masks(seg), _region_masks(target))]
    return np.array(table, dtype=np.int64)


def dice(c):
    """float64 (2 c0 + 1e-8) / (c1 + c2 + 1e-8) per row of a [..., 3] count table (tools.dice_score)"""
    c = np.asarray(c).astype(np.float64)
    return (2.0 * c[..., 0] + EPS) / (c[..., 1] + c[..., 2] + EPS)


def iou(c):
    """float64 (c0 + 1e-8) / (c1 + c2 - c0 + 1e-8) per row of a [..., 3] count table (tools.mIOU: |o | t| = |o| + |t| - |o & t|)"""
    c = np.asarray(c).astype(np.float64)
    return (c[..., 0] + EPS) / (c[..., 1] + c[..., 2] - c[..., 0] + EPS)


def region_bits(labels):
    """uint8 per int64 label: bit 0 WT, bit 1 TC, bit 2 ET"""
    wt, tc, et = _region_masks(labels)[:3]
    return (wt * 1 + tc * 2 + et * 4).astype(np.uint8)


WINDOW, STARTS = 128, ((0, 112), (0, 112), (0, 27))                  # the eight windows: start[axis][i], i = 0 or 1 per axis


def stitch_source(b, a, bb, c, nb):
    """(window * nb + b, la, lb, lc): the sample of the batch of 8 nb window outputs and the voxel in it that output voxel (b, a, bb, c)
    of the stitched [nb, 4, 240, 240, 155] volume takes (all four channels alike).  Window (ia, ib, ic) starts at (112 ia, 112 ib,
    27 ic) and has the number 4 ic + 2 ia + ib.  Along the first two axes the later window overwrites the earlier from 128 on: a < 128
    comes from window 0 at a, a >= 128 from window 1 at a - 112.  Along the last axis c < 128 comes from window 0 at c, and c >= 128
    from window 1 at 96 + (c - 128), not at c - 27: the reference's `y[..., 128:155] = t[..., 96:123]`.  Works on Python integers and,
    elementwise, on integer arrays or tensors."""
    ia, ib, ic = (a >= 128) * 1, (bb >= 128) * 1, (c >= 128) * 1
    window = 4 * ic + 2 * ia + ib
    return window * nb + b, a - STARTS[0][1] * ia, bb - STARTS[1][1] * ib, c - (128 - 96) * ic


def window_start(window):
    """(start a, start bb, start c) of window number 0..7 in the input volume"""
    ic, ia, ib = window // 4, (window // 2) % 2, window % 2
    return STARTS[0][1] * ia, STARTS[1][1] * ib, STARTS[2][1] * ic


# ------------------------------------------------------------------ test material shared by the CPU and the GPU file
VALUES = np.array([-np.inf, -1.0, -0.0, 0.0, 1e-45, 0.25, 1.0, np.inf, np.nan], dtype=np.float32)     # 1e-45: the smallest denormal
FOREIGN = [-1, 4, 5, 2 ** 32 + 3, -2 ** 63]                                                            # labels outside 0..3


def value_table():
    """float32 [6561, 4]: every row of four values of VALUES (every tie pattern, every NaN position)"""
    idx = np.stack(np.meshgrid(*([np.arange(9)] * 4), indexing="ij"), axis=-1).reshape(-1, 4)
    return VALUES[idx]


def tied_probabilities(rng, shape):
    """float32 [B, 4, *shape[1:]] for shape = (B, D0, D1, D2): random finite values in [0, 1), a third of the rows forced to ties (two,
    three or four equal classes at the maximum, in every position)"""
    b, sp = shape[0], tuple(shape[1:])
    p = rng.random((b, 4) + sp, dtype=np.float32)
    tie = rng.random((b,) + sp) < 1.0 / 3.0
    members = rng.integers(1, 16, size=(b,) + sp)                  # the classes that share the maximum, as a bitmask
    for c in range(4):
        hit = tie & ((members >> c) & 1).astype(bool)
        p[:, c][hit] = np.float32(2.0)
    return p


def target_families(rng, seg):
    """name -> int64 target of seg's shape: random 0..3, all zero, only class 2, equal to seg, and one holding the FOREIGN labels"""
    seg = np.asarray(seg)
    pool = np.array([0, 1, 2, 3, 2 ** 32 + 1] + FOREIGN, dtype=np.int64)
    foreign = pool[rng.integers(0, pool.size, size=seg.shape)]
    if foreign.size >= len(FOREIGN):
        foreign.reshape(-1)[:len(FOREIGN)] = FOREIGN               # each of them at least once
    return {"random": rng.integers(0, 4, size=seg.shape, dtype=np.int64), "zero": np.zeros(seg.shape, dtype=np.int64),
            "class 2": np.full(seg.shape, 2, dtype=np.int64), "seg": seg.astype(np.int64).copy(), "foreign": foreign}
