"""Drop-in for the reference ``models.criterions`` on the hot path: ``softmax_dice`` (criterions.py:49-62), the default
``--criterion`` of every training script (train_no_amp.py:83,138).  One fused HIP pass (cwf_dice_ce_*) replaces
F.one_hot + permute + tools.dice_loss + tools.softmax_weighted_loss; the backward is analytic.

The reference's other criteria (softmax_dice2, sigmoid_dice, Generalized_dice, Dual_focal_loss) are selectable by name
there but never defaulted; they are out of scope and raise here."""
from utils import tools


def softmax_dice(output, target):
    """output: probabilities [B,4,D,H,W]; target: int64 [B,D,H,W] in {0..3}.  Returns a scalar tensor."""
    return tools.dice_ce(output, target, num_cls=4)


def boundary_loss(output, target, **kw):
    """tools.boundary_loss: the distance-weighted term added to softmax_dice when --boundary_weight is set."""
    return tools.boundary_loss(output, target, **kw)


def topk_ce(output, target, **kw):
    """tools.topk_ce: the mean cross-entropy over the hardest k % of the batch's voxels (nnU-Net's TopKLoss)."""
    return tools.topk_ce(output, target, **kw)


def softmax_dice_topk(output, target):
    """softmax_dice + topk_ce at k = 10 %, weight 1 (nnU-Net's DC_and_topk_loss shape): selectable as --criterion softmax_dice_topk."""
    return softmax_dice(output, target) + tools.topk_ce(output, target)


def focal_tversky(output, target, **kw):
    """tools.focal_tversky: the focal Tversky loss of the regions WT / TC / ET, sums over the whole batch."""
    return tools.focal_tversky(output, target, **kw)


def focal_ce(output, target, **kw):
    """tools.focal_ce: the focal cross-entropy, mean over the batch's voxels."""
    return tools.focal_ce(output, target, **kw)


def focal_loss(output, target, **kw):
    """tools.focal_loss: focal Tversky + ce_ratio * focal cross-entropy, the term added when --focal_weight is set."""
    return tools.focal_loss(output, target, **kw)


def softmax_dice_focal(output, target):
    """softmax_dice + focal_loss at its defaults (fn 0.7, fp 0.3, exponent 0.75, gamma 2, ce_ratio 1, weight 1): selectable as
    --criterion softmax_dice_focal."""
    return softmax_dice(output, target) + tools.focal_loss(output, target)


def lovasz_softmax(output, target, **kw):
    """tools.lovasz_softmax: the Lovasz extension of the Jaccard loss, mean over the classes present, sorted over the whole batch."""
    return tools.lovasz_softmax(output, target, **kw)


def softmax_dice_lovasz(output, target):
    """softmax_dice + lovasz_softmax at its defaults (the four classes, only those present, weight 1): selectable as
    --criterion softmax_dice_lovasz."""
    return softmax_dice(output, target) + tools.lovasz_softmax(output, target)


def _not_built(name):
    def f(*a, **k):
        raise NotImplementedError("criterions.%s is an unused alternative in the reference and is not built; "
                                  "use softmax_dice" % name)
    f.__name__ = name
    return f


softmax_dice2 = _not_built("softmax_dice2")
sigmoid_dice = _not_built("sigmoid_dice")
Generalized_dice = _not_built("Generalized_dice")
Dual_focal_loss = _not_built("Dual_focal_loss")
