"""Shared pieces of the resampled-crop tests (utils.data._resample_cpu, csrc/prep.hip cwf_prepare_batch_affine): the matrices the
tests use, seeded sources, and the statement evaluated in float64.  It shares no code with utils.data."""
import numpy as np

# (Euler angles in degrees, zoom, crop) of the float64 cross-check; no matrix entry is a multiple of 1/2 other than 0 and +-1
CASES = [((10.0, -7.0, 15.0), 1.1, (128, 128, 128)),
         ((30.0, 30.0, 30.0), 0.75, (128, 128, 128)),
         ((-15.0, 4.0, 9.0), 1.25, (33, 47, 70))]


def matrix(angles_deg, zoom):
    """float32 [9] of Rz(gamma) . Ry(beta) . Rx(alpha) / zoom, built in float64 (written out, not taken from utils.data)"""
    al, be, ga = np.deg2rad(np.asarray(angles_deg, dtype=np.float64))
    ca, sa, cb, sb, cg, sg = np.cos(al), np.sin(al), np.cos(be), np.sin(be), np.cos(ga), np.sin(ga)
    r = np.array([[cg * cb, cg * sb * sa - sg * ca, cg * sb * ca + sg * sa],
                  [sg * cb, sg * sb * sa + cg * ca, sg * sb * ca - cg * sa],
                  [-sb, cb * sa, cb * ca]], dtype=np.float64)
    return (r / zoom).astype(np.float32).reshape(9)


MATRICES = [matrix(a, z) for a, z, _ in CASES]


def random_image(shape, rng):
    """finite fp32 [4, *shape]: unit normal noise with a different offset and gain per channel"""
    x = rng.standard_normal((4,) + tuple(shape), dtype=np.float32)
    gain = np.array([1.0, 3.5, 0.25, 10.0], dtype=np.float32).reshape(4, 1, 1, 1)
    off = np.array([0.0, -2.0, 5.0, 100.0], dtype=np.float32).reshape(4, 1, 1, 1)
    return (x * gain + off).astype(np.float32)


def blob_labels(shape, rng, n=12):
    """uint8 labels 0..4: overlapping ellipsoids, a later one painting over an earlier one"""
    g = np.meshgrid(*[np.arange(s, dtype=np.float32) for s in shape], indexing="ij", sparse=True)
    lab = np.zeros(shape, np.uint8)
    for k in range(n):
        c = [rng.uniform(0, s) for s in shape]
        r = [rng.uniform(0.08, 0.3) * max(s, 4) for s in shape]
        lab[sum(((gi - ci) / ri) ** 2 for gi, ci, ri in zip(g, c, r)) < 1.0] = 1 + k % 4
    return lab


def coords64(m, flip, crop):
    """q [3][*crop] float64 and the bound e [3][*crop] on |q32 - q64|: 4 * 2^-24 * (sum_j |M_dj| |u_j| + c_d)"""
    m = np.asarray(m, dtype=np.float32).astype(np.float64).reshape(3, 3)
    c = [(n - 1) / 2.0 for n in crop]
    u = []
    for d in range(3):
        p = np.arange(crop[d], dtype=np.float64)
        if flip[d]:
            p = crop[d] - 1 - p
        u.append((p - c[d]).reshape([-1 if k == d else 1 for k in range(3)]))
    q = [m[d, 0] * u[0] + m[d, 1] * u[1] + m[d, 2] * u[2] + c[d] for d in range(3)]
    e = [4.0 * 2.0 ** -24 * (abs(m[d, 0]) * abs(u[0]) + abs(m[d, 1]) * abs(u[1]) + abs(m[d, 2]) * abs(u[2]) + c[d]) for d in range(3)]
    return q, e


def resample64(image, label, m, origin, flip, crop):
    """(x float64 [4, *crop], target int64 [*crop] before 4 -> 3, q, e) of the statement in float64"""
    S = label.shape
    q, e = coords64(m, flip, crop)
    i = [np.floor(qd).astype(np.int64) for qd in q]
    f = [qd - id_ for qd, id_ in zip(q, i)]

    def tap(vol, idx):
        ok = np.ones(tuple(crop), dtype=bool)
        cl = []
        for d in range(3):
            a = idx[d] + origin[d]
            ok = ok & (a >= 0) & (a < S[d])
            cl.append(np.clip(a, 0, S[d] - 1))
        return np.where(ok, vol[cl[0], cl[1], cl[2]], 0)

    x = np.empty((4,) + tuple(crop), dtype=np.float64)
    for c in range(4):
        vol = image[c].astype(np.float64)
        r0 = []
        for d0 in (0, 1):
            r1 = []
            for d1 in (0, 1):
                a, b = tap(vol, (i[0] + d0, i[1] + d1, i[2])), tap(vol, (i[0] + d0, i[1] + d1, i[2] + 1))
                r1.append(a + f[2] * (b - a))
            r0.append(r1[0] + f[1] * (r1[1] - r1[0]))
        x[c] = r0[0] + f[0] * (r0[1] - r0[0])
    t = tap(label.astype(np.int64), [np.floor(qd + 0.5).astype(np.int64) for qd in q])
    return x, t, q, e
