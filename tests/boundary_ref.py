"""The float statement of the boundary loss (csrc/boundary.hip restates it in its header) and its references.

label int64 [N, D0, D1, D2]; region r = class bitmask posmask_r: voxel v is in G_r iff 0 <= label < 32 and (posmask_r >> label) & 1.
q_r(v): unit spacing; for v outside G_r the exact integer squared Euclidean distance to the nearest voxel of G_r, for v in G_r that to
the nearest voxel of the volume outside G_r.  phi_r(v) = float32(sqrt(float64(q))) outside, float32(1.0 - sqrt(float64(q))) inside,
formed in float64 and rounded once -- (edt(~G) * ~G - (edt(G) - 1) * G).astype(float32) of the common one_hot2dist.  A (sample, region)
whose G_r is empty or fills the volume has phi_r = +0 everywhere (scipy is undefined for the full volume).

prob float32 [N, C, D0, D1, D2].  p_r = float32 sum of p_c over c in r, increasing c.  S = sum_{n,r,v} float64(phi_r) float64(p_r);
loss = float32(float64(w) / (N R V) * S).  k = float32(float64(w) / (N R V)); s_c = float32 sum of phi_r over r holding c, increasing
r; dprob[n, c, v] = (gscale * k) * s_c in float32, each product rounded on its own; +0 for a class in no region."""
import numpy as np

REGION_MASKS = (0b1110, 0b1010, 0b1000)      # WT, TC, ET of the evaluation


def region(label, posmask):
    label = np.asarray(label)
    ok = (label >= 0) & (label < 32)
    return ok & (((int(posmask) >> np.where(ok, label, 0)) & 1) != 0)


def _sq_to_nearest(points, targets, chunk=512):
    """for each integer point [n, 3] the squared distance to the nearest of targets [m, 3] (int64, exact)"""
    out = np.empty(len(points), dtype=np.int64)
    for i in range(0, len(points), chunk):
        d = points[i:i + chunk, None, :] - targets[None, :, :]
        out[i:i + chunk] = (d * d).sum(-1).min(1)
    return out


def _phi_brute(g):
    phi = np.zeros(g.shape, dtype=np.float32)
    if g.all() or not g.any():
        return phi
    pin, pout = np.argwhere(g).astype(np.int64), np.argwhere(~g).astype(np.int64)
    phi[~g] = np.sqrt(_sq_to_nearest(pout, pin).astype(np.float64)).astype(np.float32)
    phi[g] = (1.0 - np.sqrt(_sq_to_nearest(pin, pout).astype(np.float64))).astype(np.float32)
    return phi


def _phi_scipy(g):
    from scipy.ndimage import distance_transform_edt as edt
    if g.all() or not g.any():
        return np.zeros(g.shape, dtype=np.float32)
    return (edt(~g) * ~g - (edt(g) - 1.0) * g).astype(np.float32)


def signed_distance(label, posmasks=REGION_MASKS, use_scipy=False):
    """label [N, D0, D1, D2] -> phi float32 [N, R, D0, D1, D2]; brute force on integers, or scipy's exact EDT"""
    label = np.asarray(label)
    f = _phi_scipy if use_scipy else _phi_brute
    return np.stack([np.stack([f(region(lab, m)) for m in posmasks]) for lab in label])


def boundary_loss64(prob, phi, posmasks, w, gscale=1.0):
    """prob float32 [N, C, D0, D1, D2], phi float32 [N, R, D0, D1, D2] -> (loss float32, sum |terms| float64, dprob float32 [N, C, ...])"""
    prob, phi = np.asarray(prob, dtype=np.float32), np.asarray(phi, dtype=np.float32)
    n, c = prob.shape[:2]
    r = len(posmasks)
    v = int(np.prod(prob.shape[2:]))
    s = sabs = 0.0
    for j, m in enumerate(posmasks):
        pr = np.zeros_like(prob[:, 0])
        for ch in range(c):
            if (int(m) >> ch) & 1:
                pr = (pr + prob[:, ch]).astype(np.float32)
        t = phi[:, j].astype(np.float64) * pr.astype(np.float64)
        s += float(t.sum())
        sabs += float(np.abs(t).sum())
    kd = float(np.float32(w)) / (float(n) * r * v)
    loss = np.float32(kd * s)
    k = np.float32(kd)
    gk = np.float32(np.float32(gscale) * k)
    dprob = np.zeros_like(prob)
    for ch in range(c):
        rs = [j for j, m in enumerate(posmasks) if (int(m) >> ch) & 1]
        if not rs:
            continue
        sc = phi[:, rs[0]]
        for j in rs[1:]:
            sc = (sc + phi[:, j]).astype(np.float32)
        dprob[:, ch] = (gk * sc).astype(np.float32)
    return loss, sabs, dprob


def forward_bound(ref, sabs, w, n, r, v):
    """one float32 rounding of the result plus the any-order float64 summation bound of the V-term sum"""
    return 2.0 ** -24 * abs(float(ref)) + (abs(float(w)) / (n * r * v)) * v * 2.0 ** -52 * sabs


def warmup_weight(a, epoch, warmup):
    """the --boundary_weight A / --boundary_warmup E schedule of train_no_amp.py: A * min(1, epoch / E); E = 0 is constant"""
    return float(a) if warmup <= 0 else float(a) * min(1.0, float(epoch) / float(warmup))


def emulate_passes(label, posmask):
    """The kernel's three integer passes on ONE sample in numpy (the signed single field): -> int64 q with the sign of the side,
    INF where no opposite voxel exists.  For checking the algorithm without a GPU."""
    INF = 1 << 30
    g = region(label, posmask)
    f = np.where(g, -INF, INF).astype(np.int64)
    for ax in (2, 1, 0):
        e = f.shape[ax]
        fm, gm = np.moveaxis(f, ax, 0), np.moveaxis(g, ax, 0)
        out = np.empty_like(fm)
        for t in range(e):
            best = np.abs(fm[t]).copy()
            for u in range(e):
                same = gm[u] == gm[t]
                cand = np.where(same, np.minimum(np.abs(fm[u]) + (t - u) ** 2, INF), (t - u) ** 2)
                if u != t:
                    best = np.minimum(best, cand)
            out[t] = np.where(gm[t], -best, best)
        f = np.moveaxis(out, 0, ax).copy()
    return f
