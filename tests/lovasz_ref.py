"""The Lovasz-Softmax term (csrc/lovasz.hip) stated in float64 / numpy, its derived bound and the input families of its tests.

The statement (this project's; Berman, Triggs, Blaschko, CVPR 2018, per_image=False, with tie groups sharing their increment):
  prob float32 [N, 4, *shape] (the device holds it channels-last), label int64 [N, *shape], y = label & 3, M = N V voxels.
  Regions: 1..8 class bitmasks in 1..15; default (1, 2, 4, 8), the four classes; REGION_MASKS = WT / TC / ET.
  Per region r and voxel v:
    fg  = (mask >> y) & 1
    q   = the p_c of the mask's classes added in ascending class order, float32 (one class: q = p_c exactly)
    qc  = (q > 0) ? fminf(q, 1.0f) : 0.0f            NaN, negatives, -0 -> +0; above 1 and +inf -> 1
    e   = fg ? 1.0f - qc : qc                        in [0, 1]; key = bits(e) orders like e
    sgn = (e > 0) ? (fg ? -1 : +1) : 0
  G = #{fg}.  The distinct keys in DESCENDING order; group j has m_j voxels, f_j of them foreground; n_j, F_j the running sums.
  J(n, F) = 0.0 if n = 0 else 1.0 - (double)(G - F) / (double)(G + n - F);  dJ_j = J(n_j, F_j) - J(n_{j-1}, F_{j-1}), float64, each
  operation rounded once.  L_r = sum_j (double)e_j dJ_j.  Counted: G_r > 0 (only_present) or every region; P = the number counted.
  loss = float32((double)w / max(P, 1) * sum_counted L_r); coef = [float32((double)w / P) or +0, (float)P, 0, 0].
  Every voxel of group j carries c = float32(dJ_j / (double)m_j) (0 in a region that is not counted); vcoef = c * (float)sgn.
  Backward: g0 = gscale * coef[0]; dprob[v][c] = 0.0f + (g0 * vcoef[r][v]) over the regions holding c, ascending r, float32, every
  product and sum rounded on its own."""
import math

import numpy as np

U = 2.0 ** -24
CLASS_MASKS = (1, 2, 4, 8)
REGION_MASKS = (0b1110, 0b1010, 0b1000)
F32 = np.float32


def errors(prob, label, masks):
    """-> (fg bool [R, M], e float32 [R, M], sgn float32 [R, M]) with the float32 operations of the statement"""
    prob = np.asarray(prob, dtype=F32)
    p = np.moveaxis(prob, 1, -1).reshape(-1, 4)
    y = (np.asarray(label).reshape(-1) & 3).astype(np.int64)
    fgs, es, sgns = [], [], []
    with np.errstate(invalid="ignore", over="ignore"):
        for mask in masks:
            fg = ((int(mask) >> y) & 1).astype(bool)
            q = None
            for c in range(4):
                if (int(mask) >> c) & 1:
                    q = p[:, c].copy() if q is None else (q + p[:, c]).astype(F32)
            qc = np.where(q > 0, np.minimum(q, F32(1.0)), F32(0.0)).astype(F32)
            e = np.where(fg, (F32(1.0) - qc).astype(F32), qc).astype(F32)
            sgn = np.where(e > 0, np.where(fg, F32(-1.0), F32(1.0)), F32(0.0)).astype(F32)
            fgs.append(fg), es.append(e), sgns.append(sgn)
    return np.stack(fgs), np.stack(es), np.stack(sgns)


def region64(e, fg):
    """one region -> dict: G, keys (descending distinct), m, f, n, F, dJ (float64 per group), L (float64), group (index per voxel)"""
    key = np.ascontiguousarray(e, dtype=F32).view(np.uint32)
    vals, inv, cnt = np.unique(key, return_inverse=True, return_counts=True)
    inv = inv.reshape(-1)
    nf = np.bincount(inv, weights=fg.astype(np.float64), minlength=vals.size).astype(np.int64)
    vals, m, f = vals[::-1], cnt[::-1].astype(np.int64), nf[::-1]
    group = (vals.size - 1) - inv
    n, F = np.cumsum(m), np.cumsum(f)
    G = int(fg.sum())
    J = 1.0 - (G - F).astype(np.float64) / (G + n - F).astype(np.float64)          # n >= 1 in every group: the denominator is >= 1
    dJ = J - np.concatenate([[0.0], J[:-1]])
    ev = vals.view(F32).astype(np.float64)
    return dict(G=G, keys=vals, m=m, f=f, n=n, F=F, dJ=dJ, L=math.fsum(ev * dJ), group=group)


def lovasz64(prob, label, masks=CLASS_MASKS, only_present=True, w=1.0, gscale=1.0):
    """-> dict: loss64 (before the one rounding), loss (float32), coef (float32 [4]), P, G (per region), share64 (float64 [R, M]: dJ / m of
    the voxel's group, 0 where not counted), vcoef (float32 [R, M]), dprob (float32 like prob), dJmin (the smallest increment)"""
    prob = np.asarray(prob, dtype=F32)
    fg, e, sgn = errors(prob, label, masks)
    R, M = e.shape
    share = np.zeros((R, M))
    Ls, Gs, dJmin = [], [], math.inf
    for r in range(R):
        reg = region64(e[r], fg[r])
        Gs.append(reg["G"])
        dJmin = min(dJmin, float(reg["dJ"].min()))
        if reg["G"] > 0 or not only_present:
            share[r] = (reg["dJ"] / reg["m"].astype(np.float64))[reg["group"]]
            Ls.append(reg["L"])
    P = len(Ls)
    wd = float(F32(w))
    loss64 = wd / P * math.fsum(Ls) if P else 0.0
    coef = np.array([wd / P if P else 0.0, P, 0.0, 0.0], dtype=F32)
    vcoef = (share.astype(F32) * sgn).astype(F32)
    g0 = F32(F32(gscale) * coef[0])
    d = np.zeros((M, 4), dtype=F32)
    for r, mask in enumerate(masks):
        t = (g0 * vcoef[r]).astype(F32)
        for c in range(4):
            if (int(mask) >> c) & 1:
                d[:, c] = (d[:, c] + t).astype(F32)
    dprob = np.moveaxis(d.reshape(prob.shape[:1] + prob.shape[2:] + (4,)), -1, 1).copy()
    return dict(loss64=loss64, loss=F32(loss64), coef=coef, P=P, G=Gs, share64=share, vcoef=vcoef, dprob=dprob, dJmin=dJmin, e=e, fg=fg, sgn=sgn)


def forward_bound(ref, m):
    """|kernel loss - ref| <= (2^-24 + (M + 8) 2^-52) |ref|.  The kernel's dJ_j is the statement's float64 bit for bit (integer counts,
    the same operations).  It adds (double)e (dJ_j / m_j) once per voxel where the statement adds e_j dJ_j once per group: the
    division and the product are one rounding each, and a float64 sum of M terms >= 0 in any order is within (M - 1) 2^-53 of the exact
    sum, relative; the sum over the regions and the scale w / P add three roundings, the fsum of the reference one per region.  To
    first order (M + 8) 2^-53; 2^-52 leaves the margin.  The result is rounded once to float32."""
    return (U + (m + 8) * 2.0 ** -52) * abs(float(ref))


# ------------------------------------------------------------------------------------------------------------------ input families
FAMILIES = ("softmax", "lattice", "saturated", "perfect", "lowbits", "exponents", "specials", "absent", "full")
TIE_FREE = ("softmax", "absent", "full")                  # at (5, 6, 7) with one-class masks no two errors of a region are equal


def family(name, shape, nb=2, seed=0):
    """(prob float32 [nb, 4, *shape], label int64 [nb, *shape]).  Each family is there to break one thing:
      softmax    softmax of random logits, all four classes present: the tie-free baseline
      lattice    probabilities on multiples of 1/8: at most 9 distinct keys per region, every group mixes foreground and background
      saturated  exact one-hot rows, a quarter of them wrong: only the keys 0 and 0x3f800000
      perfect    the one-hot rows of the label: loss +0 and an all-zero gradient
      lowbits    errors 0.5 + j 2^-24, j < 256: the keys differ in the lowest digit only
      exponents  errors over every exponent from 2^-149 to 1, denormals included: the keys differ in the highest digits
      specials   softmax with NaN, -0, negatives, values above 1, +inf and denormals sprinkled in: the clamp of q
      absent     softmax, class 2 missing from the label: the region is skipped (P = 3) or, with only_present off, all background
      full       softmax, every voxel of class 1: G = M, no background"""
    rng = np.random.default_rng(seed + sum(shape) + 31 * FAMILIES.index(name))
    full = (nb,) + tuple(shape)
    m = int(np.prod(full))
    label = rng.integers(0, 4, size=full).astype(np.int64)
    z = (2.0 * rng.standard_normal((nb, 4) + tuple(shape))).astype(F32)
    ex = np.exp(z - z.max(axis=1, keepdims=True))
    prob = (ex / ex.sum(axis=1, keepdims=True)).astype(F32)
    onehot = lambda lab: np.moveaxis(np.eye(4, dtype=F32)[lab], -1, 1).copy()
    if name == "softmax":
        label.reshape(-1)[:4] = np.arange(4)
    elif name == "lattice":
        prob = (rng.integers(0, 9, size=prob.shape) / 8.0).astype(F32)
    elif name == "saturated":
        wrong = rng.random(full) < 0.25
        prob = onehot(np.where(wrong, (label + rng.integers(1, 4, size=full)) & 3, label))
    elif name == "perfect":
        prob = onehot(label)
    elif name == "lowbits":
        j = rng.integers(0, 256, size=prob.shape)
        isfg = np.moveaxis(np.eye(4, dtype=bool)[label], -1, 1)
        prob = np.where(isfg, 0.5 - j * 2.0 ** -24, 0.5 + j * 2.0 ** -24).astype(F32)      # 1 - p_y and p_c are both 0.5 + j 2^-24
    elif name == "exponents":
        k = rng.integers(0, 150, size=prob.shape)
        small = (rng.uniform(0.5, 1.0, size=prob.shape) * 2.0 ** -k.astype(np.float64)).astype(F32)
        small.reshape(-1)[:3] = np.array([2.0 ** -149, 1.0, 2.0 ** -126], dtype=F32)
        isfg = np.moveaxis(np.eye(4, dtype=bool)[label], -1, 1)
        prob = np.where(isfg, (F32(1.0) - small).astype(F32), small).astype(F32)
    elif name == "specials":
        odd = np.array([np.nan, -0.0, -0.5, 1.5, np.inf, 1e-40, 0.0, 1.0, -np.inf], dtype=F32)
        where = rng.choice(prob.size, size=max(27, prob.size // 40), replace=False)
        prob.reshape(-1)[where] = odd[np.arange(where.size) % odd.size]
    elif name == "absent":
        label = np.where(label == 2, 3, label)
    elif name == "full":
        label[...] = 1
    else:
        raise ValueError(name)
    assert label.size == m
    return prob, label
