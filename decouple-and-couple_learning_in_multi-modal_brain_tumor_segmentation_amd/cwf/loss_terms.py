"""The supplementary loss terms of the training step as ONE ordered table: what cwf.trainer (constructor checks, weight tensors,
total_loss) and train_no_amp.py (flag checks, log line) know about a term they read from here.  The order is the order in which the
parts are appended to the reference's five and added to the total."""
from __future__ import annotations

import math
from typing import Callable, NamedTuple


class LossTerm(NamedTuple):
    name: str               # `<name>_weight` is the Trainer keyword, attribute and flag; `<name>_loss` the label in the log line
    title: str              # the term as messages call it
    tool: str               # utils.tools.<tool>(outputs[0], target, weight=<weight tensor>, **kwargs(*options)) computes the part
    options: tuple          # Trainer keywords (and attributes) of the static options, in the order of the value total_loss receives
    normalise: Callable     # (*options as given) -> the options as stored; ValueError for a bad one, with the term off too
    kwargs: Callable        # (*options as stored) -> the keyword arguments of the tools call beside `weight`


def _topk_options(percent=10.0):
    percent = float(percent)
    if not 0.0 < percent <= 100.0:                      # (NaN fails both comparisons)
        raise ValueError("topk_percent must lie in (0, 100], got %r" % (percent,))
    return (percent,)


def _focal_options(params=None):
    """params None or a dict of tools.focal_loss's keyword arguments (posmasks, fn, fp, exponent, smooth, gamma, ce_ratio, class_weight),
    checked by cwf.kernels.check_focal_params -> the keyword arguments with every default filled in"""
    from .kernels import REGION_MASKS, check_focal_params
    params = dict(params or {})
    unknown = set(params) - {"posmasks", "fn", "fp", "exponent", "smooth", "gamma", "ce_ratio", "class_weight"}
    if unknown:
        raise ValueError("focal_params takes posmasks, fn, fp, exponent, smooth, gamma, ce_ratio and class_weight, got %s" % sorted(unknown))
    posmasks = tuple(int(m) for m in params.pop("posmasks", REGION_MASKS))
    return (dict(check_focal_params(posmasks, **params), posmasks=posmasks),)


def _lovasz_options(regions="classes", only_present=True):
    """regions "classes" (the four classes), "regions" (WT / TC / ET) or 1 to 8 class bitmasks in 1..15, checked by
    cwf.kernels.check_lovasz_params -> (the masks as a tuple, only_present)"""
    from .kernels import CLASS_MASKS, REGION_MASKS, check_lovasz_params
    if isinstance(regions, str):
        if regions not in ("classes", "regions"):
            raise ValueError("lovasz_regions must be 'classes', 'regions' or a tuple of class bitmasks, got %r" % (regions,))
        regions = CLASS_MASKS if regions == "classes" else REGION_MASKS
    return check_lovasz_params(regions, only_present)


TERMS = (
    # signed distance maps of the target's WT / TC / ET computed on the device every step
    LossTerm("boundary", "boundary", "boundary_loss", (), lambda: (), lambda: {}),
    # mean of -log p_target over the hardest topk_percent % of the batch's voxels, selected exactly on the device
    LossTerm("topk", "top-k", "topk_ce", ("topk_percent",), _topk_options, lambda percent: {"percent": percent}),
    # focal Tversky on WT / TC / ET + ce_ratio x focal cross-entropy, sums over the whole batch
    LossTerm("focal", "focal", "focal_loss", ("focal_params",), _focal_options, lambda params: params),
    # Lovasz-Softmax, the errors of the whole batch sorted exactly on the device
    LossTerm("lovasz", "Lovasz", "lovasz_softmax", ("lovasz_regions", "lovasz_only_present"), _lovasz_options,
             lambda masks, only_present: {"posmasks": masks, "only_present": only_present}),
)
BY_NAME = {t.name: t for t in TERMS}


def check_weight(name, w):
    """the weight of term `name`: None (term off) or a finite float >= 0"""
    if w is None:
        return None
    w = float(w)
    if not math.isfinite(w) or w < 0.0:
        raise ValueError("%s_weight must be None or a finite number >= 0, got %r" % (name, w))
    return w


def check(name, weight, *options):
    """-> (weight, *the options as stored): the options are checked first, and with the term off too"""
    options = BY_NAME[name].normalise(*options)
    return (check_weight(name, weight),) + tuple(options)


def pack(term, weight_tensor, options):
    """the value total_loss receives for an active term: the weight tensor alone for a term without options, else (tensor, *options)"""
    return (weight_tensor,) + tuple(options) if term.options else weight_tensor


def unpack(term, value):
    """pack's value -> the keyword arguments of the term's tools call"""
    weight_tensor, *options = value if term.options else (value,)
    return dict(term.kwargs(*options), weight=weight_tensor)
