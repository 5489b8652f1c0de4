"""float64 restatement of the normalised surface Dice and of medpy's asd / assd as cwf_surface_metrics defines them -- the contract
csrc/metrics.hip (N8), csrc/lesions.hip (cwf_lesionwise_ex) and the host paths are tested against -- on top of
tests/hausdorff_ref.surface_distances.  For masks A, B with borders dA, dB and d(p) the distance from a border voxel to the nearest
voxel of the other border:

  within[t] = (|{p in dA : d(p) <= tau_t}|, |{p in dB : d(p) <= tau_t}|)
  nsd[t]    = (within[t][0] + within[t][1]) / (|dA| + |dB|)           one float64 division of two integers
  asd       = (mean of d over dA, mean of d over dB)                   math.fsum: the correctly rounded sum, then one division
  assd      = (asd[0] + asd[1]) / 2
  either mask empty: NaN floats, zero within.

Lesion-wise: nsd_g of (pred_g, lesion g) of tests/lesionwise_ref.py, 0 for a lesion nothing touches, and
lw_nsd[t] = (sum over kept lesions of nsd_g[t]) / (kept + FP) in increasing g, 1 if kept + FP == 0."""
import math

import numpy as np
from scipy import ndimage

import hausdorff_ref as H
import lesionwise_ref as LW


def distances(a, b, spacing=None, connectivity=1, all_border=False, use_scipy=False):
    """(d over dA, d over dB) of two non-empty 3-D masks; all_border: medpy on [1, D0, D1, D2] arrays (every mask voxel is a border)."""
    a, b = np.asarray(a).astype(bool), np.asarray(b).astype(bool)
    if all_border:
        a, b = a[None], b[None]
        spacing = (1.0,) + H._spacing(spacing, 3)
    return (H.surface_distances(a, b, spacing, connectivity, use_scipy), H.surface_distances(b, a, spacing, connectivity, use_scipy))


def surface(a, b, tolerances=(), spacing=None, connectivity=1, all_border=False, use_scipy=False):
    """dict: within [T][2] ints, nsd [T], asd (2,), assd floats, counts = (|A|, |B|, |dA|, |dB|)."""
    a, b = np.asarray(a).astype(bool), np.asarray(b).astype(bool)
    na, nb = int(a.sum()), int(b.sum())
    nda = na if all_border else int(H.border(a, connectivity).sum())
    ndb = nb if all_border else int(H.border(b, connectivity).sum())
    if na == 0 or nb == 0:
        return dict(within=[[0, 0] for _ in tolerances], nsd=[math.nan] * len(tolerances), asd=(math.nan, math.nan), assd=math.nan,
                    counts=(na, nb, nda, ndb))
    da, db = distances(a, b, spacing, connectivity, all_border, use_scipy)
    assert da.dtype == np.float64 and da.size == nda and db.size == ndb
    within = [[int((da <= t).sum()), int((db <= t).sum())] for t in tolerances]
    nsd = [float(w[0] + w[1]) / float(nda + ndb) for w in within]
    asd = (math.fsum(da.tolist()) / nda, math.fsum(db.tolist()) / ndb)
    return dict(within=within, nsd=nsd, asd=asd, assd=(asd[0] + asd[1]) / 2.0, counts=(na, nb, nda, ndb))


def asd_bound(n, ref):
    """Worst-case error of any-order float64 summation of n non-negative terms plus the final division, against the exact mean."""
    return 2.0 * n * 2.0 ** -53 * ref


def lesionwise_nsd(pred, gt, tolerances, dilation=3, min_lesion_voxels=50, use_scipy=False):
    """(lesion_nsd [G, T], lw_nsd [T]) of one sample and region, the lesions and the matching written out as lesionwise_ref does."""
    pred, gt = np.asarray(pred).astype(bool), np.asarray(gt).astype(bool)
    nt = len(tolerances)
    if not pred.any() and not gt.any():
        return np.zeros((0, nt)), [1.0] * nt
    pred_cc, P = ndimage.label(pred, structure=LW.FULL)
    dil_cc, G = LW.lesions(gt, dilation)
    out = np.zeros((G, nt))
    touched, kept = set(), []
    for g in range(1, G + 1):
        lesion = gt & (dil_cc == g)
        comps = [p for p in range(1, P + 1) if ((pred_cc == p) & (dil_cc == g)).any()]
        touched.update(comps)
        if comps:
            out[g - 1] = surface(np.isin(pred_cc, comps), lesion, tolerances, use_scipy=use_scipy)["nsd"]
        if int(lesion.sum()) > min_lesion_voxels:
            kept.append(g - 1)
    n = len(kept) + P - len(touched)
    lw = []
    for t in range(nt):
        s = 0.0
        for g in kept:
            s += out[g, t]
        lw.append(s / n if n else 1.0)
    return out, lw
