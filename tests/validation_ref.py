"""The aggregates of cwf.validation.ValidationResult restated in plain numpy float64, case by case and region by region, from a count
table [N, 19] int64: 18 counts ((|o & t|, |o|, |t|) of WT, TC, ET, class 1, 2, 3) and the voxel count.

Per case: Dice (2 |o & t| + 1e-8) / (|o| + |t| + 1e-8), IoU (|o & t| + 1e-8) / (|o| + |t| - |o & t| + 1e-8).  Over the cases: mean,
population standard deviation, median, quartiles (linear interpolation between order statistics).  Global Dice: the Dice formula on the
counts summed over cases.  Sensitivity |o & t| / |t|, precision |o & t| / |o|, specificity (V - |o| - |t| + |o & t|) / (V - |t|) on the
summed counts and summed voxel count V, NaN on a zero denominator.  score: the mean of the three mean Dice values.  No case: all NaN."""
import numpy as np


def _quantile(sorted_vals, q):
    n = len(sorted_vals)
    pos = q * (n - 1)
    lo = int(np.floor(pos))
    hi = min(lo + 1, n - 1)
    return sorted_vals[lo] + (sorted_vals[hi] - sorted_vals[lo]) * (pos - lo)


def spread(values):
    """mean, population std, median, q1, q3 of a 1-D list of float64"""
    v = [np.float64(x) for x in values]
    if not v:
        return dict(mean=np.nan, std=np.nan, median=np.nan, q1=np.nan, q3=np.nan)
    mean = sum(v) / len(v)
    std = np.sqrt(sum((x - mean) ** 2 for x in v) / len(v))
    s = sorted(v)
    return dict(mean=mean, std=std, median=_quantile(s, 0.5), q1=_quantile(s, 0.25), q3=_quantile(s, 0.75))


def _div(a, b):
    return np.float64(a) / np.float64(b) if b != 0 else np.float64(np.nan)


def aggregates(table):
    t = np.asarray(table, dtype=np.int64).reshape(-1, 19)
    n = t.shape[0]
    dice = np.zeros((n, 3))
    iou = np.zeros((n, 3))
    for i in range(n):
        for r in range(3):
            both, o, g = (np.float64(v) for v in t[i, 3 * r:3 * r + 3])
            dice[i, r] = (2 * both + 1e-8) / (o + g + 1e-8)
            both, o, g = (np.float64(v) for v in t[i, 9 + 3 * r:12 + 3 * r])
            iou[i, r] = (both + 1e-8) / (o + g - both + 1e-8)
    out = {"dice": dice, "iou": iou,
           "dice_stats": [spread(dice[:, r]) for r in range(3)], "iou_stats": [spread(iou[:, r]) for r in range(3)]}
    glob, sens, spec, prec = [], [], [], []
    vox = int(t[:, 18].sum())
    for r in range(3):
        both, o, g = (int(t[:, 3 * r + k].sum()) for k in range(3))
        glob.append((2 * np.float64(both) + 1e-8) / (np.float64(o) + np.float64(g) + 1e-8) if n else np.nan)
        sens.append(_div(both, g) if n else np.nan)
        prec.append(_div(both, o) if n else np.nan)
        spec.append(_div(vox - o - g + both, vox - g) if n else np.nan)
    out.update(global_dice=np.array(glob), sensitivity=np.array(sens), specificity=np.array(spec), precision=np.array(prec))
    out["score"] = sum(s["mean"] for s in out["dice_stats"]) / 3
    return out


def label_table_row(seg, target):
    """the 19 integers of one case from two integer label maps (numpy), counted mask by mask"""
    seg, target = np.asarray(seg), np.asarray(target)
    pairs = [(seg > 0, target > 0), ((seg == 1) | (seg == 3), (target == 1) | (target == 3)), (seg == 3, target == 3)]
    pairs += [(seg == c, target == c) for c in (1, 2, 3)]
    row = []
    for o, g in pairs:
        row += [int((o & g).sum()), int(o.sum()), int(g.sum())]
    return row + [int(seg.size)]
