"""The statement of the focal Tversky + focal cross-entropy term (csrc/focal.hip restates it in its header; DESIGN.md derives the
bounds), in numpy / float64, its bounds, and the input families and parameter sets the tests run.  The definition is this project's.

prob float32 [N, 4, D0, D1, D2]; label int64 [N, D0, D1, D2], class y = label & 3.  M = N D0 D1 D2; every sum runs over the whole batch.
Regions r < R are class bitmasks m_r over bits 0..3; t_r = (m_r >> y) & 1.
    p_r  = 0.0f + the p_c of the classes of m_r in ascending class order, FLOAT32 as the kernel forms it; everything after is float64
    TP_r = sum t_r p_r, SP_r = sum p_r, ST_r = sum t_r;  FN = ST - TP, FP = SP - TP, num = TP + s, den = ((TP + a FN) + b FP) + s
    x_r  = 1 - num / den;  FT = (1 / R) sum_r (x_r > 0 ? x_r^e : 0), x^e formed as x x^(e-1) with the power K_r uses
    q    = min(max(p_y, 1e-7f), 1);  FCE = (1 / M) sum -k_y (1 - q)^gamma ln q   (gamma, k rounded to float32 once; 1 - q is exact)
    loss = float32( w (FT + rho FCE) )
    coef = float32 of ( w K_r A_r, w K_r B_r )_r, w rho / M;  K_r = -(e / R) x_r^(e-1), A_r = (den - num ((1 - a) - b)) / den^2,
           B_r = -(num b) / den^2; both +0 where x_r <= 0
    dprob[v][c] = g ( sum over the regions holding c of (t_r coef[2 r] + coef[2 r + 1])
                      + [c = y and 1e-7 <= p_y <= 1] coef[2 R] k_y (gamma (1 - q)^(gamma-1) ln q - (1 - q)^gamma / q) )
The kernel forms the gradient in float32, every operation rounded on its own, in the order csrc/focal.hip states; `dprob32` below is
that order in numpy float32 with the logarithm and a non-integer power taken in float64 and rounded once -- what the kernel gives
wherever its logf / powf are correctly rounded, and everywhere on inputs that need neither (the `lattice` family)."""
import itertools

import numpy as np

FLOOR = np.float32(1e-7)
U = 2.0 ** -24
D = 2.0 ** -53
LOGF_ULP = 1.0                  # the documented accuracy of the device logf
POWF_ULP = 1.0                  # ... and of the device powf (used for a gamma that is not 0, 1, 2 or 3)
REGION_MASKS = (0b1110, 0b1010, 0b1000)
DEFAULTS = dict(fn=0.7, fp=0.3, exponent=0.75, smooth=1e-5, gamma=2.0, ce_ratio=1.0, class_weight=(1.0, 1.0, 1.0, 1.0))


def params(**kw):
    p = dict(DEFAULTS)
    p.update(kw)
    p["class_weight"] = tuple(float(k) for k in p["class_weight"])
    return p


# the four parameter sets of the GPU test: (posmasks, parameters)
PARAM_SETS = {
    "defaults": (REGION_MASKS, params()),
    "dice": (REGION_MASKS, params(fn=0.5, fp=0.5, exponent=1.0, ce_ratio=0.0)),
    "ce_only": ((), params(gamma=0.0)),
    "classwise": ((1, 2, 4, 8), params(gamma=1.5, class_weight=(0.1, 1.0, 2.0, 3.0), exponent=1.5)),
}


def region_probs(prob, posmasks):
    """float32 [R, N, ...]: 0.0f + p_c over the classes of each mask, ascending, every addition rounded to float32"""
    prob = np.asarray(prob, dtype=np.float32)
    out = np.zeros((len(posmasks),) + prob.shape[:1] + prob.shape[2:], dtype=np.float32)
    for r, m in enumerate(posmasks):
        for c in range(4):
            if (m >> c) & 1:
                out[r] = out[r] + prob[:, c]
    return out


def region_terms(TP, SP, ST, p, R, dx=0.0):
    """(x^e or 0, K A, K B) of one region in float64, operation by operation as focal_finalize_kernel forms them; dx shifts x (used by
    the bounds alone)"""
    a, b, e, s = p["fn"], p["fp"], p["exponent"], p["smooth"]
    FN, FP = ST - TP, SP - TP
    num = TP + s
    den = ((TP + a * FN) + b * FP) + s
    x = (1.0 - num / den) + dx
    if not x > 0.0:
        return 0.0, 0.0, 0.0
    pw1 = 1.0 if e == 1.0 else x ** (e - 1.0)                                     # one power per region: x^e is formed as x x^(e-1)
    xe = x * pw1
    K = -(e / float(R)) * pw1
    A = (den - num * ((1.0 - a) - b)) / (den * den)
    B = -(num * b) / (den * den)
    return xe, K * A, K * B


def _power64(om, gamma):
    return np.ones_like(om) if gamma == 0.0 else np.power(om, gamma)


def focal64(prob, label, posmasks, p, w=1.0, gscale=1.0, coef=None):
    """-> dict.  loss64 / loss (float32), sums (TP, SP, ST [R]), coef64 / coef (float32 [2 R + 1]), dprob64 (float64, from `coef` if
    given -- the device's own -- else from this statement's float32 coef), dprob_exact (from the unrounded coef64 and gscale),
    dprob32 (the kernel's float32 order, see the module text), and what the bounds need: the sums of absolute terms aTP, aSP, SF,
    and per element sabs, t1, t2."""
    prob = np.asarray(prob, dtype=np.float32)
    label = np.asarray(label, dtype=np.int64)
    posmasks = tuple(int(m) for m in posmasks)
    R, M = len(posmasks), int(label.size)
    y = label & 3
    a, b, e, s, rho = p["fn"], p["fp"], p["exponent"], p["smooth"], float(p["ce_ratio"])
    gamma = float(np.float32(p["gamma"]))
    k32 = np.asarray(p["class_weight"], dtype=np.float32)
    w32 = float(np.float32(w))
    pr = region_probs(prob, posmasks)
    t = np.stack([((m >> y) & 1).astype(bool) for m in posmasks]) if R else np.zeros((0,) + y.shape, dtype=bool)
    pr64 = pr.astype(np.float64)
    TP = np.array([pr64[r][t[r]].sum() for r in range(R)])
    SP = np.array([pr64[r].sum() for r in range(R)])
    ST = np.array([float(t[r].sum()) for r in range(R)])
    aTP = np.array([np.abs(pr64[r][t[r]]).sum() for r in range(R)])
    aSP = np.array([np.abs(pr64[r]).sum() for r in range(R)])
    # focal cross-entropy
    py = np.take_along_axis(prob, y[:, None], axis=1)[:, 0]
    q = np.minimum(np.maximum(py, FLOOR), np.float32(1.0)).astype(np.float32)
    q64 = q.astype(np.float64)
    om64 = 1.0 - q64                                                              # exact
    ky = k32.astype(np.float64)[y]
    SF = float((ky * (_power64(om64, gamma) * -np.log(q64))).sum()) if rho != 0.0 else 0.0
    terms = [region_terms(TP[r], SP[r], ST[r], p, R) for r in range(R)]
    ft = 0.0
    for xe, _, _ in terms:
        ft += xe
    if R:
        ft = ft / float(R)
    total = ft + rho * (SF / float(M)) if rho != 0.0 else ft
    loss64 = w32 * total
    coef64 = np.array([w32 * v for _, ka, kb in terms for v in (ka, kb)] + [w32 * rho / float(M)])
    own = coef64.astype(np.float32)
    use = own if coef is None else np.asarray(coef, dtype=np.float32)
    assert use.shape == (2 * R + 1,)
    g32 = np.float32(gscale)
    passes = (py >= FLOOR) & (py <= np.float32(1.0)) if rho != 0.0 else np.zeros(y.shape, dtype=bool)
    with np.errstate(divide="ignore", invalid="ignore"):
        if gamma == 0.0:
            t1, t2 = np.zeros_like(q64), 1.0 / q64
        else:
            t1, t2 = np.abs(gamma * np.power(om64, gamma - 1.0) * np.log(q64)), _power64(om64, gamma) / q64
    h64 = np.where(passes, -(t1 + t2), 0.0)                                       # ln q <= 0: both parts pull the same way
    t1, t2 = np.where(passes, t1, 0.0), np.where(passes, t2, 0.0)

    def grad64(cf, g):
        d = np.zeros(prob.shape, dtype=np.float64)
        sabs = np.zeros(prob.shape, dtype=np.float64)
        for r, m in enumerate(posmasks):
            u = t[r] * cf[2 * r] + cf[2 * r + 1]
            ua = t[r] * abs(cf[2 * r]) + abs(cf[2 * r + 1])
            for c in range(4):
                if (m >> c) & 1:
                    d[:, c] += u
                    sabs[:, c] += ua
        f = cf[2 * R] * ky * h64
        np.put_along_axis(d, y[:, None], np.take_along_axis(d, y[:, None], axis=1) + f[:, None], axis=1)
        np.put_along_axis(sabs, y[:, None], np.take_along_axis(sabs, y[:, None], axis=1) + np.abs(f)[:, None], axis=1)
        return g * d, sabs
    dprob64, sabs = grad64(use.astype(np.float64), float(g32))
    dprob_exact, _ = grad64(coef64, float(gscale))
    # the kernel's float32 order
    d32 = np.zeros(prob.shape, dtype=np.float32)
    for r, m in enumerate(posmasks):
        u = np.where(t[r], np.float32(use[2 * r] + use[2 * r + 1]), use[2 * r + 1]).astype(np.float32)
        for c in range(4):
            if (m >> c) & 1:
                d32[:, c] = d32[:, c] + u
    if rho != 0.0:
        pq = np.where(passes, py, np.float32(1.0)).astype(np.float32)              # (off the gate the value is not used)
        om = (np.float32(1.0) - pq).astype(np.float32)
        l = np.log(pq.astype(np.float64)).astype(np.float32)
        if gamma == 0.0:
            h = np.float32(-1.0) / pq
        elif gamma == 1.0:
            h = l - om / pq
        elif gamma == 2.0:
            h = (np.float32(2.0) * om) * l - (om * om) / pq
        elif gamma == 3.0:
            h = (np.float32(3.0) * (om * om)) * l - ((om * om) * om) / pq
        else:
            g1 = np.float32(np.float32(gamma) - np.float32(1.0))
            pw1 = np.power(om.astype(np.float64), float(g1)).astype(np.float32)
            pw = np.power(om.astype(np.float64), gamma).astype(np.float32)
            h = (np.float32(gamma) * pw1) * l - pw / pq
        f = (use[2 * R] * (k32[y] * h.astype(np.float32)).astype(np.float32)).astype(np.float32)
        at = np.take_along_axis(d32, y[:, None], axis=1)[:, 0]
        np.put_along_axis(d32, y[:, None], np.where(passes, (at + f).astype(np.float32), at)[:, None], axis=1)
    dprob32 = (g32 * d32).astype(np.float32)
    nreg = np.array([sum((m >> c) & 1 for m in posmasks) for c in range(4)], dtype=np.float64)
    return dict(R=R, M=M, posmasks=posmasks, params=p, w=w32, g=float(g32), gamma=gamma, loss64=loss64, loss=np.float32(loss64),
                TP=TP, SP=SP, ST=ST, aTP=aTP, aSP=aSP, SF=SF, ft=ft, coef64=coef64, coef=own, coef_used=use, dprob64=dprob64,
                dprob_exact=dprob_exact, dprob32=dprob32, sabs=sabs, t1=t1, t2=t2, ky=ky, y=y, nreg=nreg)


def torch_statement(prob, label, posmasks, p, w):
    """the definition written with torch ops on probabilities [N, 4, ...] of any float dtype (autograd gives its gradient; p_r is formed
    in that dtype)"""
    import torch
    total = prob.new_zeros(())
    for m in posmasks:
        cls = [c for c in range(4) if (m >> c) & 1]
        pr = sum(prob[:, c] for c in cls)
        t = sum((label == c).to(prob.dtype) for c in cls)
        TP, SP, ST = (t * pr).sum(), pr.sum(), t.sum()
        TI = (TP + p["smooth"]) / (TP + p["fn"] * (ST - TP) + p["fp"] * (SP - TP) + p["smooth"])
        total = total + torch.clamp(1.0 - TI, min=0.0) ** p["exponent"] / len(posmasks)
    if p["ce_ratio"] != 0.0:
        q = torch.clamp(prob.gather(1, label[:, None])[:, 0], float(FLOOR), 1.0)       # (the gradient passes where 1e-7f <= p_y <= 1)
        k = torch.tensor(np.asarray(p["class_weight"], dtype=np.float32)).to(prob.dtype)[label]
        gamma = float(np.float32(p["gamma"]))
        focal = -k * torch.log(q) if gamma == 0.0 else -k * (1.0 - q) ** gamma * torch.log(q)
        total = total + p["ce_ratio"] * focal.mean()
    return float(np.float32(w)) * total


# ------------------------------------------------------------------------------------------------------------------ bounds
def _eps_terms(gamma):
    """relative error of one focal term's (1 - q)^gamma and of its logarithm, as the kernel forms them: 1 - q rounds once (2^-24, gamma
    times in the power), the multiplications of gamma = 2, 3 round gamma - 1 times, powf and logf carry their documented error read as
    ulp x 2^-23 of the value"""
    pw = POWF_ULP * 2.0 ** -23 if gamma not in (0.0, 1.0, 2.0, 3.0) else 0.0
    return 2.0 * gamma * U + pw, LOGF_ULP * 2.0 ** -23


def _region_spread(res, r):
    """(centre, largest deviation) of (x^e, K A, K B) of region r over the corners of the box the kernel's sums can lie in: every float64
    sum of M terms, in any order, is within (M + 8) 2^-53 sum|terms| of the statement's; x carries the rounding of its own formula,
    8 x 2^-53 x (1 + TI sum|den terms| / |den|)"""
    p, R, M = res["params"], res["R"], res["M"]
    TP, SP, ST = float(res["TP"][r]), float(res["SP"][r]), float(res["ST"][r])
    es = (M + 8) * D
    dTP, dSP = es * float(res["aTP"][r]), es * float(res["aSP"][r])
    a, b, s = p["fn"], p["fp"], p["smooth"]
    num, den = TP + s, ((TP + a * (ST - TP)) + b * (SP - TP)) + s
    denabs = abs(TP) + a * abs(ST - TP) + b * abs(SP - TP) + s
    dx = 8.0 * D * (1.0 + abs(num / den) * denabs / abs(den))
    centre = np.array(region_terms(TP, SP, ST, p, R))
    dev = np.zeros(3)
    for s0, s1, s2 in itertools.product((-1.0, 1.0), repeat=3):
        dev = np.maximum(dev, np.abs(np.array(region_terms(TP + s0 * dTP, SP + s1 * dSP, ST, p, R, dx=s2 * dx)) - centre))
    # K A = (den - num (1 - a - b)) / den^2 forms its numerator by a subtraction: its rounding is magnified by the condition number
    c1 = abs((1.0 - a) - b)
    cond = (abs(den) + abs(num) * c1) / max(abs(den - num * ((1.0 - a) - b)), 1e-300)
    rr = np.array([8.0, 16.0 + 8.0 * cond, 24.0]) * D                                # pow (two units in the last place) and the few products
    return centre, 2.0 * dev + rr * np.abs(centre)


def forward_bound(res):
    """|kernel loss - res['loss']| <= this.  Tversky part: the spread of x^e over the box of the sums (first order, doubled) plus the
    float64 rounding of the formula; focal part: (eps_power + eps_log + (M + 8) 2^-53 + 2^-51) of the sum of its terms, all >= 0;
    the scale, the sum of the two parts and w: 8 x 2^-53 |loss|; one float32 rounding: 2^-24 |loss|."""
    R, M, p, w = res["R"], res["M"], res["params"], abs(res["w"])
    tv = sum(_region_spread(res, r)[1][0] for r in range(R)) / float(R) if R else 0.0
    ep, el = _eps_terms(res["gamma"])
    ce = float(p["ce_ratio"]) / float(M) * (ep + el + (M + 8) * D + 4.0 * D) * abs(res["SF"])
    return w * (tv + ce) * (1.0 + 2.0 ** -20) + (8.0 * D + U) * abs(res["loss64"])


def coef_bound(res):
    """float32 [2 R + 1] of bounds on |kernel coef - res['coef']|: w x the spread of K A and K B as above, one float32 rounding of each
    side (2 x 2^-24 |coef|: the statement's own float32 value is compared), and for w rho / M its two float64 roundings"""
    R, w = res["R"], abs(res["w"])
    out = np.zeros(2 * R + 1)
    for r in range(R):
        _, spread = _region_spread(res, r)
        out[2 * r], out[2 * r + 1] = w * spread[1], w * spread[2]
    out[2 * R] = 4.0 * D * abs(res["coef64"][2 * R])
    return out * (1.0 + 2.0 ** -20) + 2.0 * U * np.abs(res["coef64"]) + 2.0 ** -149


def grad_bound(res):
    """per element, |kernel dprob - res['dprob64']| where dprob64 was formed from the kernel's own coef (operand-exact): the float32
    roundings -- one in t_r coef + coef, one per addition into d_c (n_c regions hold c, then the focal part), three in the focal part
    (its subtraction and two products), one in the product with g: (n_c + 6) 2^-24 of the sum of the absolute terms -- and the error
    of the two halves of h: ((gamma + 1) + ulp_logf + ulp_powf) 2^-23 |gamma (1 - q)^(gamma-1) ln q| and
    ((gamma + 1) + ulp_powf) 2^-23 |(1 - q)^gamma / q| (1 - q rounds once and enters gamma - 1 or gamma times, the products and the
    division round once each)."""
    gamma, R = res["gamma"], res["R"]
    pw = POWF_ULP if gamma not in (0.0, 1.0, 2.0, 3.0) else 0.0
    e1, e2 = ((gamma + 1.0) + LOGF_ULP + pw) * 2.0 ** -23, ((gamma + 1.0) + pw) * 2.0 ** -23
    cfk = abs(float(res["coef_used"][2 * R])) * res["ky"]
    b = (res["nreg"][None, :, None, None, None] + 6.0) * U * res["sabs"]
    focal = cfk * (e1 * res["t1"] + e2 * res["t2"])
    y = res["y"]
    np.put_along_axis(b, y[:, None], np.take_along_axis(b, y[:, None], axis=1) + focal[:, None], axis=1)
    return abs(res["g"]) * b * (1.0 + 2.0 ** -20) + 2.0 ** -149


# ------------------------------------------------------------------------------------------------------------------ input families
FAMILIES = ("softmax", "empty", "one_sided", "full", "specials", "lattice", "saturated")
EXACT = ("lattice", "saturated")                                            # families whose sums are exact in any order
SHAPES = ((5, 6, 7), (33, 34, 65))
SPECIALS = np.array([0.0, 1.0, 1e-9, 1e-7, 1.5], dtype=np.float32)          # at the target class: 0, 1, below the floor, the floor, above 1


def family(name, shape, nb=2, seed=0):
    """(prob float32 [nb, 4, *shape], label int64 [nb, *shape]):
      softmax    softmax of random logits that lean towards the label
      empty      no voxel of class 3 in the whole batch: ST = TP = 0 for ET
      one_sided  sample 0 as softmax, sample 1 all background: every region is present in sample 0 only (the sums are batch-global)
      full       no background voxel: every voxel lies in WT, whose FP is exactly 0
      specials   softmax with 0, 1, 1e-9, 1e-7f and 1.5 sprinkled on the target class
      lattice    every probability on the 1/16 lattice and p_y = 1: all sums are exact in any order, and ln q = 0, 1 - q = 0 need no
                 device function -- the loss must match to its final rounding and coef and the gradient bit for bit.  Tumour channels
                 are large on background voxels (FP) and mostly 0 on tumour voxels, so every region keeps 1 - TI > 0
      saturated  the lattice with every other channel uniform on it: TP > ST in WT and TC, whose Tversky index passes 1 -- they
                 contribute exactly 0 to the loss and to coef"""
    rng = np.random.default_rng(seed + sum(shape) + 31 * FAMILIES.index(name))
    full = (nb,) + tuple(shape)
    label = rng.integers(0, 4, size=full).astype(np.int64)
    if name == "empty":
        label = rng.integers(0, 3, size=full).astype(np.int64)
    elif name == "one_sided":
        label[1:] = 0
    elif name == "full":
        label = rng.integers(1, 4, size=full).astype(np.int64)
    z = (1.5 * rng.standard_normal((nb, 4) + tuple(shape))).astype(np.float32)
    z += 2.0 * np.moveaxis(np.eye(4, dtype=np.float32)[label], -1, 1)
    ez = np.exp(z - z.max(axis=1, keepdims=True))
    prob = (ez / ez.sum(axis=1, keepdims=True)).astype(np.float32)
    if name == "specials":
        pt = np.take_along_axis(prob, label[:, None], axis=1)[:, 0].copy()
        m = label.size
        where = rng.choice(m, size=max(15, m // 40), replace=False)
        pt.reshape(-1)[where] = SPECIALS[np.arange(where.size) % SPECIALS.size]
        np.put_along_axis(prob, label[:, None], pt[:, None], axis=1)
    elif name == "lattice":
        big = (rng.integers(0, 9, size=prob.shape) / 16.0).astype(np.float32)
        small = ((rng.integers(0, 4, size=prob.shape) == 3) / 16.0).astype(np.float32)
        tumour = np.broadcast_to((np.arange(4) > 0)[None, :, None, None, None], prob.shape)
        prob = np.where(tumour & (label[:, None] > 0), small, big).astype(np.float32)
        np.put_along_axis(prob, label[:, None], np.ones(full, dtype=np.float32)[:, None], axis=1)
    elif name == "saturated":
        prob = (rng.integers(0, 17, size=prob.shape) / 16.0).astype(np.float32)
        np.put_along_axis(prob, label[:, None], np.ones(full, dtype=np.float32)[:, None], axis=1)
    elif name not in FAMILIES:
        raise ValueError(name)
    return prob, label
