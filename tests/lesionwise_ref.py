"""scipy restatement of the lesion-wise Dice / HD95 definition of predict_overlap.lesionwise_metrics (the BraTS 2023 ranking metrics
with this project's HD95) -- the contract that csrc/lesions.hip and the host path are tested against.  Written step by step from the
definition, one lesion at a time, with ndimage.label, ndimage.binary_dilation and tests/hausdorff_ref.hd95; nothing is shared with the
code under test."""
import numpy as np
from scipy import ndimage

import hausdorff_ref as H

FULL = ndimage.generate_binary_structure(3, 3)       # 26 neighbours
EDGE = ndimage.generate_binary_structure(3, 2)       # 18 neighbours


def dilate(mask, connectivity, iterations):
    """scipy's iterated dilation; 0 iterations leave the mask as it is (scipy itself would iterate to convergence)."""
    mask = np.asarray(mask).astype(bool)
    if iterations == 0:
        return mask.copy()
    return ndimage.binary_dilation(mask, ndimage.generate_binary_structure(3, connectivity), iterations=iterations)


def lesions(gt, dilation=3):
    """(dil_cc, G): the 26-neighbour components of the dilated ground truth; lesion g = gt & (dil_cc == g)."""
    return ndimage.label(dilate(gt, 2, dilation), structure=FULL)


def lesionwise(pred, gt, dilation=3, min_lesion_voxels=50, penalty=374.0, use_scipy=False):
    """One sample and region.  Returns a dict: dice, hd95 (float), counts = (G, kept, matched, FP, FN, P), table [G, 4] int64 =
    gt_vol, pred_vol, inter, touching components, lesion_dice [G], lesion_hd95 [G] float64."""
    pred, gt = np.asarray(pred).astype(bool), np.asarray(gt).astype(bool)
    if not pred.any() and not gt.any():
        return dict(dice=1.0, hd95=0.0, counts=(0, 0, 0, 0, 0, 0), table=np.zeros((0, 4), np.int64), lesion_dice=np.zeros(0),
                    lesion_hd95=np.zeros(0))
    pred_cc, P = ndimage.label(pred, structure=FULL)
    dil_cc, G = lesions(gt, dilation)
    table = np.zeros((G, 4), np.int64)
    ldice, lhd = np.zeros(G), np.zeros(G)
    touched = set()
    for g in range(1, G + 1):
        lesion = gt & (dil_cc == g)
        comps = [p for p in range(1, P + 1) if ((pred_cc == p) & (dil_cc == g)).any()]
        touched.update(comps)
        pred_g = np.isin(pred_cc, comps) if comps else np.zeros_like(pred)
        gt_vol, pred_vol, inter = int(lesion.sum()), int(pred_g.sum()), int((pred_g & lesion).sum())
        table[g - 1] = (gt_vol, pred_vol, inter, len(comps))
        if comps:
            ldice[g - 1] = 2.0 * inter / (pred_vol + gt_vol)
            lhd[g - 1] = H.hd95(pred_g, lesion, use_scipy=use_scipy)
        else:
            ldice[g - 1], lhd[g - 1] = 0.0, penalty
    fp = P - len(touched)
    kept = [g for g in range(G) if table[g, 0] > min_lesion_voxels]
    fn = sum(1 for g in kept if table[g, 3] == 0)
    n = len(kept) + fp
    if n == 0:
        dice, hd95 = 1.0, 0.0
    else:
        sd = sh = 0.0
        for g in kept:
            sd += ldice[g]
            sh += lhd[g]
        dice, hd95 = sd / n, (sh + fp * penalty) / n
    return dict(dice=float(dice), hd95=float(hd95), counts=(G, len(kept), P - fp, fp, fn, P), table=table, lesion_dice=ldice,
                lesion_hd95=lhd)


def scene(shape=(24, 40, 72)):
    """The hand-built scene: two ground-truth parts that the dilation merges, a 125-voxel lesion the prediction misses, a 27-voxel
    lesion it matches, and two spurious predicted components."""
    gt, pred = np.zeros(shape, bool), np.zeros(shape, bool)
    gt[4:10, 4:10, 4:10] = True
    gt[4:10, 4:10, 14:18] = True
    gt[4:9, 20:25, 40:45] = True
    gt[15:18, 30:33, 60:63] = True
    pred[5:11, 4:10, 5:17] = True
    pred[15:18, 30:33, 61:64] = True
    pred[18:22, 5:9, 30:34] = True
    pred[0:2, 36:40, 0:2] = True
    return pred, gt


def labels_from_mask(mask):
    """A label map whose WT, TC and ET regions all equal mask (label 3 throughout)."""
    return np.where(mask, 3, 0).astype(np.int64)
