"""The statement of the top-k (hard-voxel) cross-entropy term (csrc/topk.hip restates it in its header), in numpy / float64, the forward
bound, and the input families the tests run.  The definition is this project's.

prob float32 [N, C, D0, D1, D2] with C = 4 or 2; label int64 [N, D0, D1, D2].  Target class t = label for C = 4 (labels 0..3), and
(posmask >> (label & 31)) & 1 for C = 2, as in cwf_dice_ce_*.  M = N D0 D1 D2 voxels; the selection runs over the whole batch.
    pc   = (p_t > 0) ? fminf(p_t, 1.0f) : 0.0f           NaN, negatives and -0 become +0
    key  = bits(pc) as uint32                            pc >= 0: key order is value order, the smallest key is the hardest voxel
    l    = -logf(fmaxf(pc, 1e-7f))
    tau  = the k-th smallest key, 1 <= k <= M;  a = #{key < tau}, n = #{key = tau}, s = k - a, so 1 <= s <= n
    loss = float32( (double)w / k * ( sum_{key < tau} (double)l_v + (double)s * (double)l(tau) ) )
Every voxel with key = tau carries the weight s / n (the symmetric subgradient): the loss does not depend on the choice, and neither
voxel order nor launch geometry enters the gradient.
    coef = (float32((double)w / k), float32((double)s / (double)n), bits tau, +0)
    g0 = gscale * coef[0];  r = -1.0f / fmaxf(pc, 1e-7f);  every product rounded on its own:
    dprob[v][t] = g0 * r for key < tau, (g0 * coef[1]) * r for key = tau, +0 for key > tau and for every other class.
The gradient passes through the 1e-7 floor as -1 / 1e-7: the hardest voxels keep their gradient.

Here l is formed in float64 (numpy's log of the float32 argument); the kernel's logf is allowed LOGF_ULP units in the last place."""
import numpy as np

FLOOR = np.float32(1e-7)
LOGF_ULP = 1.0                  # the documented accuracy of the device logf
U = 2.0 ** -24


def target_class(label, c, posmask=0):
    label = np.asarray(label, dtype=np.int64)
    if c == 4:
        assert label.min() >= 0 and label.max() <= 3, "C = 4 takes labels 0..3"
        return label
    assert c == 2
    return (int(posmask) >> (label & 31)) & 1


def clamp(pt):
    """pc of float32 p_t"""
    pt = np.asarray(pt, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        return np.where(pt > 0, np.minimum(pt, np.float32(1.0)), np.float32(0.0)).astype(np.float32)


def nll64(pc):
    """-log(max(pc, 1e-7f)) in float64 of the float32 argument"""
    return -np.log(np.maximum(np.asarray(pc, dtype=np.float32), FLOOR).astype(np.float64))


def keys_of(prob, label, posmask=0):
    """-> (t [N, ...] int64, pc float32 [N, ...], key uint32 [N, ...])"""
    prob = np.asarray(prob, dtype=np.float32)
    t = target_class(label, prob.shape[1], posmask)
    pt = np.take_along_axis(prob, t[:, None], axis=1)[:, 0]
    pc = clamp(pt)
    return t, pc, pc.view(np.uint32)


def select(key, k):
    """-> (tau, a, n, s) of the k-th smallest key"""
    flat = np.sort(np.asarray(key, dtype=np.uint32).reshape(-1))
    assert 1 <= k <= flat.size
    tau = int(flat[k - 1])
    a = int(np.searchsorted(flat, tau, side="left"))
    n = int(np.searchsorted(flat, tau, side="right")) - a
    s = k - a
    assert 1 <= s <= n
    return tau, a, n, s


def topk_ce64(prob, label, k, w, posmask=0, gscale=1.0):
    """-> dict: tau, a, n, s, loss64 (float64, before the one rounding), loss (float32), sabs (sum of the |terms| of the bracket),
    coef (float32 [4]; [2] carries the bits of tau), weights (float64 per voxel: 1, s / n or 0), dprob (float32 like prob)"""
    prob = np.asarray(prob, dtype=np.float32)
    t, pc, key = keys_of(prob, label, posmask)
    tau, a, n, s = select(key, k)
    l = nll64(pc)
    ltau = float(nll64(np.array([tau], dtype=np.uint32).view(np.float32))[0])
    below, tie = key < tau, key == tau
    bracket = float(l[below].sum()) + float(s) * ltau
    kd = float(np.float32(w)) / float(k)
    coef = np.zeros(4, dtype=np.float32)
    coef[0], coef[1] = np.float32(kd), np.float32(float(s) / float(n))
    coef.view(np.uint32)[2] = tau
    g0 = np.float32(np.float32(gscale) * coef[0])
    g1 = np.float32(g0 * coef[1])
    r = (np.float32(-1.0) / np.maximum(pc, FLOOR)).astype(np.float32)
    g = np.where(below, (g0 * r).astype(np.float32), np.where(tie, (g1 * r).astype(np.float32), np.float32(0.0))).astype(np.float32)
    dprob = np.zeros_like(prob)
    np.put_along_axis(dprob, t[:, None], g[:, None], axis=1)
    weights = np.where(below, 1.0, np.where(tie, float(s) / float(n), 0.0))
    return dict(tau=tau, a=a, n=n, s=s, loss64=kd * bracket, loss=np.float32(kd * bracket), sabs=abs(bracket), coef=coef, weights=weights,
                dprob=dprob)


def forward_bound(ref, sabs, w, k, logf_ulp=LOGF_ULP):
    """|kernel loss - ref| <=  (w / k) (logf_ulp 2^-23 + (k + 2) 2^-52) sabs  +  2^-24 |ref|:
    every l the kernel adds is a float32 within logf_ulp units in the last place of the exact logarithm, at most 2^-23 of its value
    each, and all terms are >= 0, so the bracket moves by at most logf_ulp 2^-23 sabs; a float64 sum of at most k + 1 terms in any
    order, the product s l(tau) and the scale w / k add at most (k + 2) 2^-53 sabs to first order (2^-52 leaves the margin and covers
    numpy's own float64 log); the result is rounded once to float32."""
    return abs(float(w)) / float(k) * (logf_ulp * 2.0 ** -23 + (k + 2) * 2.0 ** -52) * float(sabs) + U * abs(float(ref))


def topk_count(m, percent):
    """nnU-Net's rounding: int(M * percent / 100), kept inside 1..M"""
    return max(1, min(int(m), int(m * percent / 100)))


# ------------------------------------------------------------------------------------------------------------------ input families
FAMILIES = ("softmax", "lattice", "last_digit", "exponents", "constant", "specials")
C2_POSMASK = sum(1 << c for c in (1, 5, 6, 7))            # an edge set of utils.tools


def family(name, shape, c=4, nb=2, seed=0):
    """(prob float32 [nb, c, *shape], label int64 [nb, *shape], posmask): p_t of every voxel follows the family, the other channels hold
    other values (so reading the wrong channel shows).  Each family is there to break one digit pass or one counter:
      softmax     softmax of random logits
      lattice     p_t on the 1/16 lattice: large tie groups at tau
      last_digit  p_t = 0.5 + j 2^-24, j < 1024: the keys differ in their last 10 bits only
      exponents   p_t spread over the exponents 2^-30 .. 1: the first digit decides, and the 1e-7 floor is crossed
      constant    every voxel equal: n = M, one bin holds everything
      specials    softmax with a sprinkle of 0, 1, -0, negative, > 1, NaN and a subnormal"""
    rng = np.random.default_rng(seed + sum(shape) + 17 * FAMILIES.index(name) + c)
    full = (nb,) + tuple(shape)
    m = int(np.prod(full))
    posmask = 0 if c == 4 else C2_POSMASK
    label = rng.integers(0, 4 if c == 4 else 9, size=full).astype(np.int64)
    t = target_class(label, c, posmask)
    z = (2.0 * rng.standard_normal((nb, c) + tuple(shape))).astype(np.float32)
    e = np.exp(z - z.max(axis=1, keepdims=True))
    prob = (e / e.sum(axis=1, keepdims=True)).astype(np.float32)
    if name == "softmax":
        pt = None
    elif name == "lattice":
        pt = (rng.integers(1, 17, size=full) / 16.0).astype(np.float32)
    elif name == "last_digit":
        pt = (0.5 + rng.integers(0, 1024, size=full) * 2.0 ** -24).astype(np.float32)
    elif name == "exponents":
        pt = (rng.uniform(0.5, 1.0, size=full) * 2.0 ** -rng.integers(0, 31, size=full)).astype(np.float32)
    elif name == "constant":
        pt = np.full(full, 0.3, dtype=np.float32)
    elif name == "specials":
        pt = np.take_along_axis(prob, t[:, None], axis=1)[:, 0].copy()
        odd = np.array([0.0, 1.0, -0.0, -0.5, 1.5, np.nan, 1e-40], dtype=np.float32)
        where = rng.choice(m, size=max(14, m // 50), replace=False)
        pt.reshape(-1)[where] = odd[np.arange(where.size) % odd.size]
    else:
        raise ValueError(name)
    if pt is not None:
        np.put_along_axis(prob, t[:, None], pt[:, None], axis=1)
    return prob, label, posmask


def tie_k(key):
    """a k strictly inside the largest tie group of the keys (0 < s < n), or None when no two keys are equal"""
    flat = np.sort(np.asarray(key, dtype=np.uint32).reshape(-1))
    vals, start, cnt = np.unique(flat, return_index=True, return_counts=True)
    j = int(np.argmax(cnt))
    if cnt[j] < 2:
        return None
    return int(start[j]) + int(cnt[j]) // 2


def ks_of(key):
    """the k of every case: 1, M, 10 % of M, and one strictly inside a tie group where the family has one"""
    m = int(np.asarray(key).size)
    ks = [1, m, topk_count(m, 10.0)]
    kt = tie_k(key)
    if kt is not None and kt not in ks:
        ks.append(kt)
    return ks
