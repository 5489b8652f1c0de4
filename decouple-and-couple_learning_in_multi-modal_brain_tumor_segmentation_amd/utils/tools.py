"""Drop-in for the hot-path part of the reference ``utils.tools``: the per-sub-region Dice / weighted-CE losses
(tools.py:8-34,112-231) on the fused HIP loss kernels, the collective helper (:37-41), the integer Dice / IoU metrics
(:44-61,89-109) and ``softmax_hd_dice`` (:64-86), whose medpy Hausdorff distances (tools.py:5) run on the device kernels of
``utils.hausdorff``: ``medpy`` is not required.

Label decoding happens inside the kernel: a 4-class map uses the label as class; a binary map uses
``(posmask >> label) & 1`` -- sub-region k -> {target == k}; edge sets E1={1,5,6,7}, E2={2,5,6,8}, E4={4,5,7,8}
(tools.py:174-218).  Per-sample CE weights and batch-global Dice sums, as in the reference."""
import torch
import torch.distributed as dist

from cwf import functional as CF

REGION_MASKS = {"01": 1 << 1, "02": 1 << 2, "04": 1 << 3}
EDGE_MASKS = {"01": sum(1 << c for c in (1, 5, 6, 7)), "02": sum(1 << c for c in (2, 5, 6, 8)),
              "04": sum(1 << c for c in (4, 5, 7, 8))}


def dice_ce(output, target, num_cls=4, posmask=0):
    """dice_loss(output, onehot) + softmax_weighted_loss(output, onehot)  (tools.py:8-34) in one fused pass."""
    if output.shape[1] != num_cls:
        raise ValueError("expected %d channels, got %d" % (num_cls, output.shape[1]))
    return CF.dice_ce_loss(output, target, posmask)


def boundary_loss(output, target, posmasks=CF.REGION_MASKS, weight=1.0, phi=None):
    """Boundary loss (Kervadec et al., MIDL 2019) of the probabilities output [B,C,D,H,W] against the label map target [B,D,H,W]:
    weight * mean of (signed distance to the region's ground-truth boundary) * (probability of the region) over the regions
    `posmasks` (class bitmasks; default WT, TC, ET).  Not in the reference; off unless asked for."""
    return CF.boundary_loss(output, target, posmasks=posmasks, weight=weight, phi=phi)


def topk_ce(output, target, percent=10.0, weight=1.0, posmask=0):
    """Top-k cross-entropy (nnU-Net's TopKLoss, k = 10 %) of the probabilities output [B,C,D,H,W] (C = 4, or 2 with a posmask) against
    the label map target [B,D,H,W]: weight * mean of -log max(p_target, 1e-7) over the hardest `percent` % of the voxels of the whole
    batch, selected exactly on the device.  Not in the reference; off unless asked for."""
    return CF.topk_ce_loss(output, target, percent=percent, weight=weight, posmask=posmask)


def focal_loss(output, target, posmasks=CF.REGION_MASKS, fn=0.7, fp=0.3, exponent=0.75, smooth=1e-5, gamma=2.0, ce_ratio=1.0,
               class_weight=None, weight=1.0):
    """Focal Tversky on the regions `posmasks` (class bitmasks; default WT, TC, ET) + ce_ratio * focal cross-entropy of the probabilities
    output [B,4,D,H,W] against the label map target [B,D,H,W]: weight * (mean_r max(1 - TI_r, 0)^exponent + ce_ratio * mean of
    -k_y (1 - q)^gamma ln q), TI_r = (TP + smooth) / (TP + fn FN + fp FP + smooth) over the whole batch.  Not in the reference; off unless
    asked for."""
    return CF.focal_loss(output, target, posmasks=posmasks, fn=fn, fp=fp, exponent=exponent, smooth=smooth, gamma=gamma, ce_ratio=ce_ratio,
                         class_weight=class_weight, weight=weight)


def focal_tversky(output, target, posmasks=CF.REGION_MASKS, fn=0.7, fp=0.3, exponent=0.75, smooth=1e-5, weight=1.0):
    """focal_loss with ce_ratio = 0: the recall-weighted overlap loss alone (Salehi et al. 2017; Abraham & Khan 2019)."""
    return CF.focal_loss(output, target, posmasks=posmasks, fn=fn, fp=fp, exponent=exponent, smooth=smooth, ce_ratio=0.0, weight=weight)


def focal_ce(output, target, gamma=2.0, class_weight=None, weight=1.0):
    """focal_loss with no regions: weight * mean of -k_y (1 - q)^gamma ln q, q = clamp(p_target, 1e-7, 1) (Lin et al. 2017)."""
    return CF.focal_loss(output, target, posmasks=(), gamma=gamma, ce_ratio=1.0, class_weight=class_weight, weight=weight)


def lovasz_softmax(output, target, posmasks=CF.CLASS_MASKS, only_present=True, weight=1.0):
    """Lovasz-Softmax (Berman et al. 2018) of the probabilities output [B,4,D,H,W] against the label map target [B,D,H,W]: weight * the
    mean over the counted regions `posmasks` (class bitmasks; default the four classes, CF.REGION_MASKS for WT / TC / ET) of the Lovasz
    extension of the Jaccard loss, the errors of the whole batch sorted exactly on the device; only_present counts only the regions the
    target holds.  Not in the reference; off unless asked for."""
    return CF.lovasz_softmax(output, target, posmasks=posmasks, only_present=only_present, weight=weight)


def _separate(output, target, masks):
    maps = [output[r] for r in ("01", "02", "04")]
    if all(isinstance(m, CF.LazyProb) for m in maps) and len({(m.scale, tuple(m.logit.shape)) for m in maps}) == 1:
        # training-mode outputs of this package's heads: Dice / CE straight from the low-resolution logits, one label read for
        # the three sub-regions, no full-resolution map (cwf_head_loss_*)
        return CF.head_group_loss(maps, target, [masks[r] for r in ("01", "02", "04")])
    return sum(dice_ce(torch.as_tensor(output[r]) if not isinstance(output[r], CF.LazyProb) else output[r].materialize(), target, 2, masks[r])
               for r in ("01", "02", "04"))


def get_separate_loss(output, target):
    """tools.get_separate_loss (tools.py:112-162): three binary problems {target == k}, k = 1, 2, 3."""
    return _separate(output, target, REGION_MASKS)


def get_edge_separate_loss(output, target):
    """tools.get_edge_separate_loss (tools.py:165-231) on edge codes in {0,1,2,4,5,6,7,8}."""
    return _separate(output, target, EDGE_MASKS)


def all_reduce_tensor(tensor, op=dist.ReduceOp.SUM, world_size=1):
    """tools.all_reduce_tensor (tools.py:37-41)."""
    tensor = tensor.clone()
    dist.all_reduce(tensor, op)
    tensor.div_(world_size)
    return tensor


def dice_score(o, t, eps=1e-8):
    """tools.dice_score (tools.py:44-47) on boolean / 0-1 arrays or tensors."""
    num = 2 * (o * t).sum() + eps
    den = o.sum() + t.sum() + eps
    return num / den


def mIOU(o, t, eps=1e-8):
    """tools.mIOU (tools.py:50-53) on boolean arrays or tensors."""
    num = (o * t).sum() + eps
    den = (o | t).sum() + eps
    return num / den


def softmax_mIOU_score(output, target):
    """tools.softmax_mIOU_score (tools.py:56-61): IoU of classes 1, 2, 3 of integer label maps (numpy or torch)."""
    return [mIOU(o=(output == 1), t=(target == 1)), mIOU(o=(output == 2), t=(target == 2)), mIOU(o=(output == 3), t=(target == 3))]


def softmax_hd_dice(output, target):
    """tools.softmax_hd_dice (tools.py:64-86): ([WT, TC, ET] Dice, [WT, TC, ET] medpy hd) of integer label maps (numpy or torch, any
    device).  A region that is empty in either map raises medpy's RuntimeError; rank rules as utils.hausdorff."""
    from utils import hausdorff
    return softmax_output_dice(output, target), hausdorff.softmax_hd(output, target)


def softmax_output_dice(output, target):
    """tools.softmax_output_dice (tools.py:89-109): [WT, TC, ET] Dice of integer label maps (numpy or torch)."""
    ret = [dice_score(output > 0, target > 0)]
    ret.append(dice_score((output == 1) | (output == 3), (target == 1) | (target == 3)))
    ret.append(dice_score(output == 3, target == 3))
    return ret
