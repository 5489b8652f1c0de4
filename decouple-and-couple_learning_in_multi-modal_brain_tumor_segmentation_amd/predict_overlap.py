"""Sliding-window inference -- counterpart of the hot-path part of the reference ``predict_overlap.py``
(BASELINE.json configs[3]: full 240x240x155 volume on one MI355X).

``tailor_and_concat`` (predict_overlap.py:31-58): eight fixed 128^3 windows over a [B,4,240,240,>=155] volume
(H, W starts {0, 112}, D starts {0, 27}) and hard-overwrite stitching -- INCLUDING the reference's depth-axis quirk
(`y[..., 128:155] = window(27:155)[..., 96:123]`, i.e. voxels 123..149 land at 128..154), reproduced
for parity.  The reference runs the eight windows as eight sequential B=1 forwards; here they are independent samples of
one batch, so they go through the kernels as ONE batch-8 forward.

``validate_softmax`` (predict_overlap.py:103-171) minus file I/O (nibabel / imageio are not hot-path): argmax over
classes and the WT / TC / ET Dice of ``utils.tools.softmax_output_dice``; optionally the per-region surface HD95 (``with_hd95``).

``flip_tta`` (N4; predict_simple.py:333-349, predict_cls.py:184-203): the reference's 8-flip test-time augmentation -- the
mean over all subsets of the three spatial axes of ``softmax(model(flip(x))[0]).flip`` (the reference re-applies softmax to
the model's already-normalised output; kept, ``resoftmax=True``).  The eight flipped copies are independent samples, so
they run as batches instead of eight sequential B=1 forwards.

``sliding_window_inference`` (N5): volumes of any size -- overlapping windows on the grid of ``window_grid``, each window's
probabilities weighted by the separable ``importance_map`` (Gaussian or constant) and normalised by the per-voxel weight sum, in
the manner of nnU-Net / MONAI (the grid and map rules are this project's own, stated below; no bit parity with either is claimed).
Per chunk of windows: one gather launch, one model forward, one blend launch; one finalize launch at the end (csrc/window.hip).
``crop_nonzero=True`` lays the windows over the nonzero box of the volume (``nonzero_box``, csrc/nonzero_box.hip) instead of the
whole of it and writes background outside: 8 window forwards instead of 18 for a BraTS case at the default settings.

``postprocess`` (N6): connected-component post-processing of a predicted label map -- small whole-tumour components removed, only the
largest kept, small enhancing-tumour components and a tiny enhancing-tumour total relabelled (the ``postprocess=True`` switch of the
reference's predictors, whose 500-voxel rule is the preset ``REFERENCE_POSTPROCESS``).  On the device: region bits -> component labelling
-> policy (csrc/components.hip), no host synchronisation; CPU tensors go through numpy and scipy.ndimage.label.

``lesionwise_metrics`` (N7): lesion-wise Dice and HD95, the numbers BraTS has ranked by since 2023 -- every ground-truth lesion scored on
its own, every missed lesion and every spurious predicted component penalised.  On the device: region bits -> dilation -> two
labellings -> touch / count passes -> HD95 of eight lesions per call -> aggregate (csrc/lesions.hip); CPU tensors go through numpy and scipy.

``surface_regions`` (N8): the normalised surface Dice at given tolerances and medpy's average symmetric surface distance per region, on
the borders and exact distances of the HD95 kernels (cwf_surface_metrics); ``lesionwise_metrics(nsd_tolerances=...)`` scores the NSD
per lesion as well.
"""
import itertools
import math

import numpy as np
import torch

from utils import tools
from utils.hausdorff import surface_host as _surface_host

WINDOWS = [(0, 0, 0), (0, 112, 0), (112, 0, 0), (112, 112, 0), (0, 0, 27), (0, 112, 27), (112, 0, 27), (112, 112, 27)]


def tailor_and_concat(x, missing_modal, model, target=None, batched=True):
    """x: [B,4,240,240,D>=155].  Returns the stitched probability volume [B,4,240,240,155]."""
    wins = [x[..., a:a + 128, b:b + 128, c:c + 128] for a, b, c in WINDOWS]
    if batched:
        nb = x.shape[0]
        out = model(torch.cat(wins, dim=0), missing_modal)[0]
        if out.is_cuda and out.dtype == torch.float32 and tuple(out.shape[1:]) == (4, 128, 128, 128) and x.shape[-1] >= 155:
            from cwf.kernels import backend
            return backend().stitch_windows(out, nb)          # one launch (cwf_stitch_windows) instead of clone + 8 slice copies
        t = [out[i * nb:(i + 1) * nb] for i in range(8)]
    else:
        t = [model(w, missing_modal)[0] for w in wins]
    y = x.clone()                       # the reference relies on 4 modalities == 4 classes (predict_overlap.py:43)
    y[..., :128, :128, :128] = t[0]
    y[..., :128, 128:240, :128] = t[1][..., :, 16:128, :]
    y[..., 128:240, :128, :128] = t[2][..., 16:128, :, :]
    y[..., 128:240, 128:240, :128] = t[3][..., 16:128, 16:128, :]
    y[..., :128, :128, 128:155] = t[4][..., 96:123]
    y[..., :128, 128:240, 128:155] = t[5][..., :, 16:128, 96:123]
    y[..., 128:240, :128, 128:155] = t[6][..., 16:128, :, 96:123]
    y[..., 128:240, 128:240, 128:155] = t[7][..., 16:128, 16:128, 96:123]
    return y[..., :155]


FLIPS = [(), (2,), (3,), (4,), (2, 3), (2, 4), (3, 4), (2, 3, 4)]          # order of predict_simple.py:333-347


@torch.no_grad()
def flip_tta(x, missing_modal, forward, resoftmax=True, batch=8):
    """x [B,4,D,H,W]; forward(xb, missing_modal) -> probabilities [b,C,D,H,W].  Returns the 8-flip average [B,C,D,H,W]."""
    nb = x.shape[0]
    acc = None
    for g0 in range(0, 8, max(1, batch // max(nb, 1))):
        group = FLIPS[g0:g0 + max(1, batch // max(nb, 1))]
        xb = torch.cat([x.flip(dims=f) if f else x for f in group], dim=0)
        out = forward(xb, missing_modal)
        for k, f in enumerate(group):
            o = out[k * nb:(k + 1) * nb]
            if resoftmax:
                o = torch.softmax(o, dim=1)
            o = o.flip(dims=f) if f else o
            acc = o.clone() if acc is None else acc.add_(o)
    return acc / 8.0


def window_grid(shape, roi_size, overlap):
    """Per-axis window starts (three lists) for a volume of spatial `shape` and windows of `roi_size`; the windows are the Cartesian
    product, ordered lexicographically with axis 0 slowest.  Along an axis of size S with window r: S <= r gives one window at 0 (the
    volume is zero-padded to r); otherwise n = ceil((S - r) / (r (1 - overlap))) + 1 windows at round(i (S - r) / (n - 1)), the
    first at 0 and the last at S - r.  overlap in [0, 1)."""
    shape, roi = tuple(int(s) for s in shape), tuple(int(r) for r in roi_size)
    if len(shape) != 3 or len(roi) != 3 or min(shape) <= 0 or min(roi) <= 0:
        raise ValueError("window_grid: need three positive extents and three positive window sizes, got %r and %r" % (shape, roi))
    if not 0.0 <= float(overlap) < 1.0:
        raise ValueError("window_grid: overlap must lie in [0, 1), got %r" % (overlap,))
    starts = []
    for s, r in zip(shape, roi):
        if s <= r:
            starts.append([0])
            continue
        n = int(math.ceil((s - r) / (r * (1.0 - float(overlap))))) + 1
        step = (s - r) / (n - 1)
        starts.append([int(np.round(step * i)) for i in range(n)])
    return tuple(starts)


def importance_tables(roi_size, blend="gaussian", sigma_scale=0.125):
    """The three fp32 1-D factors of the importance map: ones ("constant") or g_a(t) = exp(-(t - (r_a - 1) / 2)^2 / (2 sigma_a^2)),
    sigma_a = sigma_scale * r_a, evaluated in float64 and rounded once to fp32 ("gaussian")."""
    roi = tuple(int(r) for r in roi_size)
    if len(roi) != 3 or min(roi) <= 0:
        raise ValueError("importance map: need three positive window sizes, got %r" % (roi_size,))
    if blend == "constant":
        return tuple(np.ones(r, np.float32) for r in roi)
    if blend != "gaussian":
        raise ValueError("importance map: blend must be 'gaussian' or 'constant', got %r" % (blend,))
    if not sigma_scale > 0:
        raise ValueError("importance map: sigma_scale must be positive, got %r" % (sigma_scale,))
    tabs = []
    for r in roi:
        t = np.arange(r, dtype=np.float64) - (r - 1) / 2.0
        sig = float(sigma_scale) * r
        tabs.append(np.exp(-t * t / (2.0 * sig * sig)).astype(np.float32))
    if np.float32(np.float32(tabs[0].min() * tabs[1].min()) * tabs[2].min()) <= 0:   # the smallest weight (fp32 rounding is monotone)
        raise ValueError("importance map: sigma_scale %r makes edge weights underflow to 0 in fp32" % (sigma_scale,))
    return tuple(tabs)


def importance_map(roi_size, blend="gaussian", sigma_scale=0.125):
    """[r0, r1, r2] fp32 weights fp32(fp32(g0 * g1) * g2) of importance_tables -- what cwf_window_blend multiplies each window by."""
    g0, g1, g2 = importance_tables(roi_size, blend, sigma_scale)
    g01 = g0[:, None] * g1[None, :]                     # fp32 x fp32 -> fp32 (rounded once), as the kernel forms it
    return g01[:, :, None] * g2[None, None, :]


MIN_SEMANTIC_TOKENS = 128      # the model's top_num: (r0 / 16) (r1 / 16) (r2 / 8) tokens per window at least


def check_roi(roi_size):
    """Raise ValueError unless the model accepts windows of roi_size: sides multiples of 16 and >= 128 semantic tokens."""
    roi = tuple(int(r) for r in roi_size)
    if len(roi) != 3 or min(roi) <= 0 or any(r % 16 for r in roi):
        raise ValueError("sliding window: roi_size must be three positive multiples of 16 (the model's down-sampling), got %r"
                         % (tuple(roi_size),))
    if (roi[0] // 16) * (roi[1] // 16) * (roi[2] // 8) < MIN_SEMANTIC_TOKENS:
        raise ValueError("sliding window: roi_size %r yields %d semantic tokens, the model needs at least %d ((r0/16)(r1/16)(r2/8))"
                         % (roi, (roi[0] // 16) * (roi[1] // 16) * (roi[2] // 8), MIN_SEMANTIC_TOKENS))
    return roi


_weights_cache = {}


def _device_tables(roi, blend, sigma_scale, device):
    key = (roi, blend, float(sigma_scale), str(device))
    w = _weights_cache.get(key)
    if w is None:
        w = torch.from_numpy(np.concatenate(importance_tables(roi, blend, sigma_scale))).to(device)
        _weights_cache[key] = w
    return w


def nonzero_box(x, margin=0):
    """(lo, hi), two triples of Python ints with hi exclusive: the union over the samples of x [B,4,S0,S1,S2] float32 of the tightest
    box holding every nonzero voxel (a voxel is nonzero iff some channel's bits & 0x7fffffff != 0: +-0 is background, denormals,
    infinities and NaN are not), grown by `margin` >= 0 voxels per side and clipped to the volume; None when every sample is all
    zero.  CUDA tensors: one kernel call (HipBackend.nonzero_box) and one copy of the B x 6 integers to the host; CPU tensors: numpy."""
    if not (torch.is_tensor(x) and x.dtype == torch.float32 and x.dim() == 5 and x.shape[1] == 4 and x.numel() > 0):
        raise ValueError("nonzero_box: x must be a non-empty fp32 [B,4,S0,S1,S2] tensor, got %s %s"
                         % (getattr(x, "dtype", type(x)), tuple(getattr(x, "shape", ()))))
    if int(margin) != margin or int(margin) < 0:
        raise ValueError("nonzero_box: margin must be an integer >= 0, got %r" % (margin,))
    shape = tuple(int(s) for s in x.shape[2:])
    if x.is_cuda:
        from cwf.kernels import backend
        boxes = backend().nonzero_box(x)[0].cpu().numpy()
    else:
        from utils.data import nonzero_boxes_host
        boxes = nonzero_boxes_host(x.numpy())[0]
    lo, hi = boxes[:, :3].min(axis=0), boxes[:, 3:].max(axis=0)           # an empty sample (lo = S, hi = 0) moves neither
    if int(hi[0]) == 0:
        return None
    m = int(margin)
    return tuple(max(int(a) - m, 0) for a in lo), tuple(min(int(b) + m, s) for b, s in zip(hi, shape))


@torch.no_grad()
def sliding_window_inference(x, missing_modal, model, roi_size=(128, 128, 128), overlap=0.5, blend="gaussian", sigma_scale=0.125,
                             sw_batch_size=8, crop_nonzero=False, nonzero_margin=0):
    """x: CUDA fp32 [B,4,S0,S1,S2] of any extent; model(xb, missing_modal) -> (prob [n*B,4,r0,r1,r2], ...).  Returns the blended
    probability volume [B,4,S0,S1,S2]: sum over covering windows of w(v - s) p / sum of w(v - s), with the windows of
    window_grid(roi_size, overlap) (axes shorter than the window zero-padded) and w = importance_map(roi_size, blend, sigma_scale).
    sw_batch_size windows (times B samples) go through the model per forward.  Results do not depend on sw_batch_size.
    crop_nonzero (nnU-Net's crop_to_nonzero, MONAI's CropForeground; off by default, and then nothing new is called): the windows are
    those of window_grid(box extent, roi_size, overlap) laid over box = nonzero_box(x, nonzero_margin), read from x in place, and the
    result is still [B,4,S0,S1,S2].  It is bit-equal to cropping x to the box, running this function on the contiguous crop and
    pasting the result into a volume of the background one-hot (1, 0, 0, 0) (cwf_window_gather_box, cwf_window_finalize_box: no
    crop copy, no fill pass, no paste).  Against crop_nonzero=False this is an approximation, and only outside the box: there the
    input is zero by construction, the uncropped path would still have run the model on it and blended whatever it predicts for
    air, the cropped path writes background; inside the box the two differ only in which windows cover a voxel.  A batch that is
    zero everywhere has no box and takes the whole volume, identical to crop_nonzero=False."""
    roi = check_roi(roi_size)
    if not (torch.is_tensor(x) and x.is_cuda and x.dtype == torch.float32 and x.dim() == 5 and x.shape[1] == 4):
        raise ValueError("sliding window: x must be a CUDA fp32 [B,4,S0,S1,S2] tensor, got %s %s"
                         % (getattr(x, "dtype", type(x)), tuple(getattr(x, "shape", ()))))
    if int(sw_batch_size) < 1:
        raise ValueError("sliding window: sw_batch_size must be >= 1, got %r" % (sw_batch_size,))
    from cwf.kernels import backend
    be = backend()
    nb, shape = int(x.shape[0]), tuple(int(s) for s in x.shape[2:])
    box = nonzero_box(x, nonzero_margin) if crop_nonzero else None
    if box is not None:
        return _sliding_window_box(be, x, missing_modal, model, roi, overlap, blend, sigma_scale, int(sw_batch_size), box)
    starts = window_grid(shape, roi, overlap)
    weights = _device_tables(roi, blend, sigma_scale, x.device)
    grid = be.window_grid(nb, shape, roi, starts)
    x = x.contiguous()
    nw = len(starts[0]) * len(starts[1]) * len(starts[2])
    acc = torch.empty((nb,) + shape + (4,), dtype=torch.float32, device=x.device)
    for w0 in range(0, nw, int(sw_batch_size)):
        cnt = min(int(sw_batch_size), nw - w0)
        prob = model(be.window_gather(x, grid, w0, cnt), missing_modal)[0]
        be.window_blend(prob, weights, acc, grid, w0, cnt, accumulate=w0 > 0)
    return be.window_finalize(acc, weights, grid)


def _sliding_window_box(be, x, missing_modal, model, roi, overlap, blend, sigma_scale, sw_batch_size, box):
    """sliding_window_inference's loop with the grid laid over box = (lo, hi) of x: the accumulator has the box's extent, the gather
    reads x in place and the finalize writes the whole volume"""
    lo, hi = box
    nb, full = int(x.shape[0]), tuple(int(s) for s in x.shape[2:])
    shape = tuple(b - a for a, b in zip(lo, hi))
    starts = window_grid(shape, roi, overlap)
    weights = _device_tables(roi, blend, sigma_scale, x.device)
    grid, wbox = be.window_grid(nb, shape, roi, starts), be.window_box(full, lo)
    x = x.contiguous()
    nw = len(starts[0]) * len(starts[1]) * len(starts[2])
    acc = torch.empty((nb,) + shape + (4,), dtype=torch.float32, device=x.device)
    for w0 in range(0, nw, sw_batch_size):
        cnt = min(sw_batch_size, nw - w0)
        prob = model(be.window_gather_box(x, grid, wbox, w0, cnt), missing_modal)[0]
        be.window_blend(prob, weights, acc, grid, w0, cnt, accumulate=w0 > 0)
    return be.window_finalize_box(acc, weights, grid, wbox)


def windows(starts):
    """The window start triples of a window_grid result, in window order."""
    return list(itertools.product(*starts))


@torch.no_grad()
def validate_softmax(x, target, model, deterministic=True, use_TTA=False, with_miou=False, with_hd95=False, window=None,
                     postprocess=None, lesionwise=None, with_nsd=None, with_counts=False, predict=None):
    """One subject: stitched probabilities -> label map (argmax; class 3 stands for BraTS label 4) -> [WT, TC, ET] Dice.
    ``deterministic`` zeroes the stem dropout that the reference leaves on in eval mode.  ``with_miou`` adds the per-class
    IoU list of tools.softmax_mIOU_score (what predict_simple.py reports next to Dice) as a fourth result.  ``with_hd95`` appends the
    BraTS surface HD95: a [B, 3] float64 tensor of per-sample WT / TC / ET HD95 between ``seg`` and the target, on 3-D surfaces (unit
    spacing, connectivity 1), 0 where either region is empty or full (the rule of utils.hausdorff.hausdorff_distance_95), computed on
    the device (cwf_hausdorff); None without a target.  Result order: (seg, prob, dice[, miou][, hd95]).  predict_simple.py's own numbers
    come from utils.hausdorff on [1, ...] arrays, where every mask voxel counts as a border voxel.
    ``window``: None -- the reference's eight-window stitcher on a [B,4,240,240,>=155] volume, the target cut to depth 155; a dict of
    sliding_window_inference keyword arguments (roi_size, overlap, blend, sigma_scale, sw_batch_size, crop_nonzero, nonzero_margin) --
    blended windows over a volume of any size, the target compared at the volume's own shape; with "crop_nonzero": True the windows
    cover the volume's nonzero box only and ``seg`` is 0 outside it (with use_TTA every flipped volume finds its own box).
    ``postprocess``: None -- the label map is the plain argmax; a dict of `postprocess` keyword arguments (REFERENCE_POSTPROCESS is
    one) -- ``seg`` is the processed map and Dice, IoU and HD95 are all computed from it (Dice as tools.softmax_output_dice gives it).
    ``lesionwise``: None -- the result tuple is as above; True or a dict of `lesionwise_metrics` keyword arguments -- the dict that
    lesionwise_metrics(seg, target) returns for the final ``seg`` is appended as the last element (None without a target).
    ``with_nsd``: None -- nothing more; a tuple of tolerances -- the dict that surface_regions(seg, target, tolerances) returns for the
    final ``seg`` (the post-processed map when ``postprocess`` is given) is appended after everything above (None without a target).
    ``with_counts``: True -- the int64 [6, 3] tensor of (|o & t|, |o|, |t|) for WT, TC, ET, class 1, 2, 3 of the final ``seg`` against the
    target, the counts the Dice and IoU values are ratios of, is appended last of all (None without a target); on the device it is the
    count tensor of the launch that produced them (argmax_dice / label_metrics counts=True), nothing is counted twice.
    ``predict``: None -- the model predicts through the stitcher or the windows, as above; a callable x [B,4,...] -> probabilities
    [B,4,...] of x's own extent -- it stands in for all of that (``model`` and ``window`` are not used and ``model`` may be None, the
    target is compared at the volume's own shape), on CUDA or CPU tensors; everything after the probabilities is unchanged."""
    given = predict
    if given is None:
        model.eval()
        saved = model.Unet_list.InitConv.dropout
        if deterministic:
            model.Unet_list.InitConv.dropout = 0.0
    if given is not None:
        predict, cut = (lambda xb, mm: given(xb)), None
    elif window is None:
        predict, cut = (lambda xb, mm: tailor_and_concat(xb, mm, model)), 155
    else:
        predict, cut = (lambda xb, mm: sliding_window_inference(xb, mm, model, **window)), None
    try:
        if use_TTA:         # each flipped volume goes through the predictor (the 8-window stitcher: one batch-8 forward per flip)
            prob = flip_tta(x, None, predict, batch=1)
        else:
            prob = predict(x, None)
    finally:
        if given is None:
            model.Unet_list.InitConv.dropout = saved
    counts = [] if with_counts and target is not None else None          # _validate / _revalidate append the tensor they counted
    res = _validate(prob, target, with_miou, cut, counts)
    if postprocess is not None:
        res = _revalidate(_apply_postprocess(res[0], postprocess), prob, target, with_miou, cut, counts)
    if with_hd95:
        res = res + ((None if target is None else hd95_regions(res[0], target[..., :cut].long())),)
    if lesionwise is not None and lesionwise is not False:
        kw = {} if lesionwise is True else dict(lesionwise)
        res = res + ((None if target is None else lesionwise_metrics(res[0], target[..., :cut].long().to(res[0].device), **kw)),)
    if with_nsd is not None:
        res = res + ((None if target is None else surface_regions(res[0], target[..., :cut].long().to(res[0].device), tuple(with_nsd))),)
    if with_counts:
        res = res + ((counts[-1] if counts else None),)
    return res


def label_counts(seg, target):
    """int64 [6, 3] tensor on seg's device of (|o & t|, |o|, |t|) for WT, TC, ET (the regions of tools.softmax_output_dice) and class 1, 2, 3
    (tools.softmax_mIOU_score) of two integer label maps of one shape, by torch reductions: what cwf_argmax_metrics and
    cwf_label_metrics count, for tensors that do not pass through them (CPU tensors)."""
    pairs = [(seg > 0, target > 0), ((seg == 1) | (seg == 3), (target == 1) | (target == 3)), (seg == 3, target == 3)]
    pairs += [(seg == c, target == c) for c in (1, 2, 3)]
    return torch.stack([torch.stack([(o & t).sum(), o.sum(), t.sum()]) for o, t in pairs]).to(torch.int64)


def _validate(prob, target, with_miou, cut=155, counts=None):
    """counts: None, or a list that receives the int64 [6, 3] count tensor of the label map against the target"""
    if prob.is_cuda and prob.dtype == torch.float32 and prob.dim() == 5 and prob.shape[1] == 4:
        from cwf.kernels import backend                     # argmax + WT/TC/ET counts in one launch (cwf_argmax_dice)
        tgt = None if target is None else target[..., :cut].long().to(prob.device)
        if counts is not None and tgt is not None:          # the launch of with_miou, its count tensor kept
            seg, d, iou, table = backend().argmax_dice(prob, tgt, miou=True, counts=True)
            counts.append(table)
            res = (seg, prob, [d[0], d[1], d[2]])
            return res + ([iou[0], iou[1], iou[2]],) if with_miou else res
        if with_miou and tgt is not None:
            seg, d, iou = backend().argmax_dice(prob, tgt, miou=True)          # argmax + Dice + IoU counts, still one launch
            return seg, prob, [d[0], d[1], d[2]], [iou[0], iou[1], iou[2]]
        seg, d = backend().argmax_dice(prob, tgt)
        res = (seg, prob, (None if d is None else [d[0], d[1], d[2]]))
        return res + (None,) if with_miou else res
    seg = prob.argmax(1)
    dice = tools.softmax_output_dice(seg, target[..., :cut]) if target is not None else None
    if counts is not None and target is not None:
        counts.append(label_counts(seg, target[..., :cut].to(seg.device)))
    if with_miou:
        return seg, prob, dice, (tools.softmax_mIOU_score(seg, target[..., :cut]) if target is not None else None)
    return seg, prob, dice


def _apply_postprocess(seg, policy):          # validate_softmax's keyword hides the function's name there
    return postprocess(seg, **policy)


def _revalidate(seg, prob, target, with_miou, cut, counts=None):
    """The result tuple of _validate for a label map that is already there (the post-processed one); counts as there."""
    dice = miou = None
    if target is not None:
        tgt = target[..., :cut].long()
        if seg.is_cuda:
            from cwf.kernels import backend
            if counts is not None:
                d, iou, table = backend().label_metrics(seg, tgt.to(seg.device), counts=True)
                counts.append(table)
            else:
                d, iou = backend().label_metrics(seg, tgt.to(seg.device))
            dice, miou = [d[0], d[1], d[2]], [iou[0], iou[1], iou[2]]
        else:
            dice, miou = tools.softmax_output_dice(seg, tgt), tools.softmax_mIOU_score(seg, tgt)
            if counts is not None:
                counts.append(label_counts(seg, tgt))
    return (seg, prob, dice, miou) if with_miou else (seg, prob, dice)


def hd95_regions(seg, target):
    """[B, 3] float64 WT / TC / ET surface HD95 of two [B, D0, D1, D2] int64 label maps on the device, 0 where either region is empty
    or full (utils.hausdorff's rule).  No host synchronisation."""
    from cwf.kernels import backend
    be = backend()
    target = target.to(seg.device)
    _, hd95, counts = be.hausdorff(be.region_bits(seg), be.region_bits(target), 3)
    nvox = seg[0].numel()
    degenerate = (counts[..., 0] == 0) | (counts[..., 1] == 0) | (counts[..., 0] == nvox) | (counts[..., 1] == nvox)
    return hd95.masked_fill(degenerate, 0.0)


def surface_regions(seg, target, tolerances=(1.0,), spacing=None):
    """Per-region (WT, TC, ET) normalised surface Dice and average symmetric surface distance of two [B, D0, D1, D2] int64 label maps:
    a dict of nsd [B, 3, T] (T = len(tolerances) <= 4) and assd [B, 3] float64, on seg's device.  With dA, dB the connectivity-1
    borders of the two regions and d(p) the Euclidean distance (in `spacing` units; None = 1) from a border voxel to the nearest
    voxel of the other border: nsd[t] = (|{p in dA: d(p) <= tol_t}| + |{p in dB: d(p) <= tol_t}|) / (|dA| + |dB|) -- the voxel-border
    form (MONAI's compute_surface_dice without sub-voxel handling), not the area-weighted surface-element form of DeepMind's
    surface-distance; with unit spacing every tolerance < 1 counts coincident border voxels only -- and assd = medpy's assd, the mean
    of the two directed mean distances.  NaN where either region is empty.  CUDA tensors run on the device (cwf_surface_metrics)
    without a host synchronisation; CPU tensors go through numpy and scipy."""
    for name, t in (("seg", seg), ("target", target)):
        if not torch.is_tensor(t) or t.dim() != 4 or t.dtype != torch.int64:
            raise ValueError("surface_regions: %s must be an int64 tensor of shape [B, D0, D1, D2], got %s %s"
                             % (name, getattr(t, "dtype", type(t)), tuple(getattr(t, "shape", ()))))
    if tuple(seg.shape) != tuple(target.shape) or seg.numel() == 0:
        raise ValueError("surface_regions: seg and target must have one non-empty shape, got %r and %r"
                         % (tuple(seg.shape), tuple(target.shape)))
    tol = _tolerances("surface_regions", tolerances)
    if seg.is_cuda:
        from cwf.kernels import backend
        be = backend()
        out = be.surface_metrics(be.region_bits(seg), be.region_bits(target.to(seg.device)), 3, tol, spacing)
        return {"nsd": out["nsd"], "assd": out["assd"]}
    s, t = seg.numpy(), target.cpu().numpy()
    nsd = torch.full((seg.shape[0], 3, len(tol)), math.nan, dtype=torch.float64)
    assd = torch.full((seg.shape[0], 3), math.nan, dtype=torch.float64)
    for b in range(seg.shape[0]):
        for r, (o, g) in enumerate(zip(_regions(s[b]), _regions(t[b]))):
            if o.any() and g.any():
                _, m, _, n, _ = _surface_host(o, g, tol, spacing)
                assd[b, r] = m
                nsd[b, r] = torch.tensor(n, dtype=torch.float64)
    return {"nsd": nsd, "assd": assd}


def _tolerances(name, tolerances):
    tol = tuple(float(t) for t in tolerances)
    if len(tol) > 4 or any(not t >= 0.0 for t in tol):
        raise ValueError("%s: at most 4 tolerances, each >= 0 and not NaN, got %r" % (name, tol))
    return tol


REFERENCE_POSTPROCESS = dict(et_min_voxels=500, et_replace=1)        # the 500-voxel enhancing-tumour rule of the reference's lineage


def postprocess(seg, min_component=0, keep_largest=False, et_min_component=0, et_min_voxels=0, et_replace=1, connectivity=1,
                with_stats=False):
    """Connected-component post-processing of [B, D0, D1, D2] int64 label maps (classes 0..3; WT = seg > 0, ET = seg == 3), components
    under the 6/18/26-neighbour footprint (connectivity 1/2/3).  Applied in this order, each rule off at 0 / False:
      1  every WT component of fewer than min_component voxels is set to 0
      2  keep_largest: only the largest WT component surviving rule 1 is kept (ties: the one met first in C order), the rest set to 0
      3  every ET component of fewer than et_min_component voxels is relabelled et_replace (0, 1 or 2)
      4  if fewer than et_min_voxels ET voxels remain after rules 1-3, all of them are relabelled et_replace
    Returns the processed map (a new tensor), with_stats: and a [B, 4] int64 tensor of WT voxels removed, WT components removed, ET
    voxels relabelled, ET voxels remaining.  CUDA tensors run region_bits -> components -> postprocess_labels on the device without a
    host synchronisation; CPU tensors run numpy + scipy.ndimage.label."""
    if not torch.is_tensor(seg) or seg.dim() != 4 or seg.dtype != torch.int64:
        raise ValueError("postprocess: seg must be an int64 tensor of shape [B, D0, D1, D2], got %s %s"
                         % (getattr(seg, "dtype", type(seg)), tuple(getattr(seg, "shape", ()))))
    if seg.numel() == 0:
        raise ValueError("postprocess: seg is empty, shape %r" % (tuple(seg.shape),))
    thresholds = (int(min_component), int(et_min_component), int(et_min_voxels))
    if min(thresholds) < 0:
        raise ValueError("postprocess: min_component, et_min_component and et_min_voxels must be >= 0, got %r" % (thresholds,))
    if et_replace not in (0, 1, 2):
        raise ValueError("postprocess: et_replace must be 0, 1 or 2, got %r" % (et_replace,))
    if connectivity not in (1, 2, 3):
        raise ValueError("postprocess: connectivity must be 1, 2 or 3, got %r" % (connectivity,))
    if seg.is_cuda:
        from cwf.kernels import backend
        be = backend()
        labels, sizes, _, largest = be.components(be.region_bits(seg), 3, connectivity)
        out, stats = be.postprocess_labels(seg, labels, sizes, largest, 0, 2, thresholds[0], keep_largest, thresholds[1], thresholds[2],
                                           int(et_replace))
    else:
        out, stats = _postprocess_host(seg.numpy(), thresholds[0], bool(keep_largest), thresholds[1], thresholds[2], int(et_replace),
                                       int(connectivity))
        out, stats = torch.from_numpy(out), torch.from_numpy(stats)
    return (out, stats) if with_stats else out


def _postprocess_host(seg, min_component, keep_largest, et_min_component, et_min_voxels, et_replace, connectivity):
    from scipy import ndimage                                   # only the CPU path needs scipy
    footprint = ndimage.generate_binary_structure(3, connectivity)
    out = seg.copy()
    stats = np.zeros((seg.shape[0], 4), dtype=np.int64)
    for b in range(seg.shape[0]):
        s = out[b]
        if min_component > 0 or keep_largest:
            lab, k = ndimage.label(s > 0, structure=footprint)
            size = np.bincount(lab.ravel(), minlength=k + 1)
            drop = np.zeros(k + 1, dtype=bool)
            if min_component > 0:
                drop[1:] = size[1:] < min_component
            if keep_largest and k:
                drop[1:] |= np.arange(1, k + 1) != 1 + int(np.argmax(size[1:]))      # argmax: the first of equal sizes
            gone = drop[lab]
            stats[b, 0], stats[b, 1] = int(gone.sum()), int(drop[1:].sum())
            s[gone] = 0
        if et_min_component > 0:
            lab, k = ndimage.label(s == 3, structure=footprint)
            size = np.bincount(lab.ravel(), minlength=k + 1)
            small = np.zeros(k + 1, dtype=bool)
            small[1:] = size[1:] < et_min_component
            hit = small[lab]
            stats[b, 2] = int(hit.sum())
            s[hit] = et_replace
        left = int((s == 3).sum())
        if et_min_voxels > 0 and left < et_min_voxels:
            s[s == 3] = et_replace
            stats[b, 2] += left
            left = 0
        stats[b, 3] = left
    return out, stats


LESIONWISE_MAX = 64            # CWF_LESIONWISE_MAX: lesions per (sample, region) on the device path


def lesionwise_metrics(seg, target, dilation=3, min_lesion_voxels=50, penalty=374.0, with_table=False, nsd_tolerances=None):
    """Lesion-wise Dice and HD95 (the BraTS 2023 ranking metrics) of [B, D0, D1, D2] int64 label maps, per sample and region
    (WT = label > 0, TC = label in {1, 3}, ET = label == 3).  For the binary masks pred, gt of one sample and region:
      1  pred_cc = components of pred under the 26-neighbour footprint, numbered 1..P as scipy.ndimage.label numbers them
      2  gt_dil = gt dilated `dilation` times with the 18-neighbour footprint (out-of-volume voxels unset; 0 leaves gt as it is)
      3  dil_cc = 26-neighbour components of gt_dil, 1..G; lesion g = gt & (dil_cc == g): ground-truth parts whose dilations touch are
         one lesion
      4  component p touches lesion g if some voxel has pred_cc == p and dil_cc == g; a component may touch several lesions and counts
         for each; pred_g = the union of the components touching g
      5  per lesion gt_vol = |lesion g|, pred_vol = |pred_g|, inter = |pred_g & lesion g|; if nothing touches it, it is a false negative
         with dice_g = 0 and hd95_g = penalty; otherwise dice_g = 2 inter / (pred_vol + gt_vol) and hd95_g = the HD95 of (pred_g,
         lesion g) that this project computes everywhere (medpy's hd95 on 3-D surfaces, connectivity 1, unit spacing)
      6  FP = predicted components touching no lesion (lesions below the volume threshold take part in the touching)
      7  kept = lesions with gt_vol > min_lesion_voxels, n = |kept| + FP; lw_dice = sum over kept of dice_g / n and
         lw_hd95 = (sum over kept of hd95_g + FP penalty) / n, summed in increasing g in float64; (1, 0) if n == 0 (both masks empty
         included)
    This follows the published BraTS 2023 lesion-wise procedure except that HD95 is this project's, not the challenge tool's
    surface-distance library: parity is claimed with this definition only, not with the challenge tool's numbers.
    Returns a dict: dice [B, 3] and hd95 [B, 3] float64, counts [B, 3, 6] int64 = G, kept, matched predicted components (P - FP), FP,
    FN (kept lesions that nothing touches), P; with_table also table [B, 3, L, 4] int64 = gt_vol, pred_vol, inter, touching components
    of lesion g at row g - 1 and lesion_hd95 [B, 3, L] float64 (zeros past G), L = 64 or the largest G if that is more.
    CUDA tensors take the device path (backend().lesionwise): it needs one device-to-host readback of the B x 3 lesion counts, to
    launch only the HD95 calls that hold a lesion, and this function reads the overflow flags back; a (sample, region) with more than 64
    lesions is recomputed by the host path and patched in.  CPU tensors go through numpy and scipy.  Results are on seg's device.
    nsd_tolerances: None -- the dict above; a tuple of up to four tolerances -- also lw_nsd [B, 3, T] float64, the lesion-wise
    normalised surface Dice: nsd_g = the NSD of (pred_g, lesion g) as `surface_regions` defines it (unit spacing), 0 for a lesion that
    nothing touches, and lw_nsd = sum over kept of nsd_g / n, summed in increasing g, 1 if n == 0 (a false-positive component
    contributes 0, as to lw_dice); with_table also lesion_nsd [B, 3, L, T] (zeros past G)."""
    for name, t in (("seg", seg), ("target", target)):
        if not torch.is_tensor(t) or t.dim() != 4 or t.dtype != torch.int64:
            raise ValueError("lesionwise_metrics: %s must be an int64 tensor of shape [B, D0, D1, D2], got %s %s"
                             % (name, getattr(t, "dtype", type(t)), tuple(getattr(t, "shape", ()))))
    if tuple(seg.shape) != tuple(target.shape) or seg.numel() == 0:
        raise ValueError("lesionwise_metrics: seg and target must have one non-empty shape, got %r and %r"
                         % (tuple(seg.shape), tuple(target.shape)))
    dilation, min_lesion_voxels, penalty = int(dilation), int(min_lesion_voxels), float(penalty)
    if not 0 <= dilation <= 8:
        raise ValueError("lesionwise_metrics: dilation must lie in 0..8, got %r" % (dilation,))
    if min_lesion_voxels < 0 or not 0.0 <= penalty < 1e300:
        raise ValueError("lesionwise_metrics: min_lesion_voxels and penalty must be >= 0 (and finite), got %r and %r"
                         % (min_lesion_voxels, penalty))
    nb = int(seg.shape[0])
    tol = () if nsd_tolerances is None else _tolerances("lesionwise_metrics", nsd_tolerances)
    nt = len(tol)
    if seg.is_cuda:
        from cwf.kernels import backend
        be = backend()
        dev_out = be.lesionwise(be.region_bits(seg), be.region_bits(target.to(seg.device)), 3, dilation, min_lesion_voxels, penalty, tol)
        summary, counts, overflow, table, lesion_hd95 = dev_out[:5]
        lesion_nsd, lw_nsd = dev_out[5:] if nt else (torch.zeros((nb, 3, LESIONWISE_MAX, 0), dtype=torch.float64, device=seg.device),
                                                     torch.zeros((nb, 3, 0), dtype=torch.float64, device=seg.device))
        over = overflow.cpu().numpy()
        if over.any():
            width = LESIONWISE_MAX
            patches = []
            for b in np.nonzero(over.any(axis=1))[0]:            # one copy to the host per overflowing sample
                s, t = seg[b].cpu().numpy(), target[b].cpu().numpy()
                for r in np.nonzero(over[b])[0]:
                    masks = [(s > 0, t > 0), ((s == 1) | (s == 3), (t == 1) | (t == 3)), (s == 3, t == 3)][r]
                    patches.append((int(b), int(r), _lesionwise_host(masks[0], masks[1], dilation, min_lesion_voxels, penalty, tol)))
                    width = max(width, patches[-1][2][2].shape[0])
            if width > LESIONWISE_MAX:
                table = torch.nn.functional.pad(table, (0, 0, 0, width - LESIONWISE_MAX))
                lesion_hd95 = torch.nn.functional.pad(lesion_hd95, (0, width - LESIONWISE_MAX))
                lesion_nsd = torch.nn.functional.pad(lesion_nsd, (0, 0, 0, width - LESIONWISE_MAX))
            for b, r, (sm, cn, tb, lh, ln, wn) in patches:
                summary[b, r] = torch.tensor(sm, dtype=torch.float64)
                counts[b, r] = torch.tensor(cn, dtype=torch.int64)
                table[b, r, :tb.shape[0]] = torch.from_numpy(tb).to(table.device)
                lesion_hd95[b, r, :lh.shape[0]] = torch.from_numpy(lh).to(table.device)
                if nt:
                    lesion_nsd[b, r, :ln.shape[0]] = torch.from_numpy(ln).to(table.device)
                    lw_nsd[b, r] = torch.tensor(wn, dtype=torch.float64)
    else:
        s, t = seg.numpy(), target.numpy()
        res = [[_lesionwise_host(o, g, dilation, min_lesion_voxels, penalty, tol) for o, g in zip(_regions(s[b]), _regions(t[b]))]
               for b in range(nb)]
        width = max([LESIONWISE_MAX] + [x[2].shape[0] for row in res for x in row])
        summary = torch.tensor([[x[0] for x in row] for row in res], dtype=torch.float64)
        counts = torch.tensor([[x[1] for x in row] for row in res], dtype=torch.int64)
        table = torch.zeros((nb, 3, width, 4), dtype=torch.int64)
        lesion_hd95 = torch.zeros((nb, 3, width), dtype=torch.float64)
        lesion_nsd = torch.zeros((nb, 3, width, nt), dtype=torch.float64)
        lw_nsd = torch.tensor([[list(x[5]) for x in row] for row in res], dtype=torch.float64).reshape(nb, 3, nt)
        for b, row in enumerate(res):
            for r, x in enumerate(row):
                table[b, r, :x[2].shape[0]] = torch.from_numpy(x[2])
                lesion_hd95[b, r, :x[3].shape[0]] = torch.from_numpy(x[3])
                lesion_nsd[b, r, :x[4].shape[0]] = torch.from_numpy(x[4])
    out = {"dice": summary[..., 0].contiguous(), "hd95": summary[..., 1].contiguous(), "counts": counts}
    if nsd_tolerances is not None:
        out["lw_nsd"] = lw_nsd
    if with_table:
        out["table"], out["lesion_hd95"] = table, lesion_hd95
        if nsd_tolerances is not None:
            out["lesion_nsd"] = lesion_nsd
    return out


def _regions(labels):
    return [labels > 0, (labels == 1) | (labels == 3), labels == 3]


def _hd95_host(a, b):
    """medpy's hd95 (connectivity 1, unit spacing) of two non-empty 3-D masks with scipy, on the bounding box of a | b grown by one
    voxel inside the volume: every border voxel of either mask lies in it, and what lies beyond it is unset in both."""
    from scipy import ndimage
    box = tuple(slice(max(int(i.min()) - 1, 0), int(i.max()) + 2) for i in np.nonzero(a | b))
    a, b = a[box], b[box]
    ba, bb = a & ~ndimage.binary_erosion(a), b & ~ndimage.binary_erosion(b)
    d = np.hstack((ndimage.distance_transform_edt(~bb)[ba], ndimage.distance_transform_edt(~ba)[bb]))
    return float(np.percentile(d, 95))


def _lesionwise_host(pred, gt, dilation, min_lesion_voxels, penalty, tolerances=()):
    """One sample and region on the host: ((lw_dice, lw_hd95), counts [6], table [G, 4] int64, lesion_hd95 [G] float64,
    lesion_nsd [G, T] float64, lw_nsd [T]) for the T tolerances."""
    from scipy import ndimage                                   # only the CPU path needs scipy
    full = ndimage.generate_binary_structure(3, 3)
    pred_cc, npred = ndimage.label(pred, structure=full)
    gt_dil = ndimage.binary_dilation(gt, ndimage.generate_binary_structure(3, 2), iterations=dilation) if dilation > 0 else gt
    dil_cc, ng = ndimage.label(gt_dil, structure=full)
    sizes = np.bincount(pred_cc.ravel(), minlength=npred + 1)
    pairs = np.unique(np.stack([pred_cc[(pred_cc > 0) & (dil_cc > 0)], dil_cc[(pred_cc > 0) & (dil_cc > 0)]]), axis=1)
    gt_vol = np.bincount(dil_cc[gt], minlength=ng + 1)
    inter = np.bincount(dil_cc[gt & pred], minlength=ng + 1)
    table = np.zeros((ng, 4), dtype=np.int64)
    hd = np.zeros(ng, dtype=np.float64)
    nsd = np.zeros((ng, len(tolerances)), dtype=np.float64)
    snsd = [0.0] * len(tolerances)
    sdice = shd = 0.0
    kept = fn = 0
    for g in range(1, ng + 1):
        comps = pairs[0][pairs[1] == g]
        table[g - 1] = (gt_vol[g], sizes[comps].sum(), inter[g], len(comps))
        if len(comps):
            dice = 2.0 * float(inter[g]) / float(table[g - 1, 1] + gt_vol[g])
            hd[g - 1] = _hd95_host(np.isin(pred_cc, comps), gt & (dil_cc == g))
            if tolerances:
                nsd[g - 1] = _surface_host(np.isin(pred_cc, comps), gt & (dil_cc == g), tolerances)[3]
        else:
            dice, hd[g - 1] = 0.0, penalty
        if gt_vol[g] > min_lesion_voxels:
            sdice, shd, kept, fn = sdice + dice, shd + hd[g - 1], kept + 1, fn + (len(comps) == 0)
            snsd = [x + float(y) for x, y in zip(snsd, nsd[g - 1])]
    fp = npred - len(np.unique(pairs[0]))
    n = kept + fp
    summary = (sdice / n, (shd + fp * penalty) / n) if n else (1.0, 0.0)
    return summary, (ng, kept, npred - fp, fp, fn, npred), table, hd, nsd, [(x / n if n else 1.0) for x in snsd]
