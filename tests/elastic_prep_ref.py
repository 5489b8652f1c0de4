"""Scalar restatement of the elastically deformed crop (include/cwf_hip.h cwf_prepare_batch_elastic, utils.data._resample_cpu): one
loop iteration per output voxel, every operation on numpy float32 scalars in the order the statement writes it.  It shares no code
with utils.data; the edge codes come from tests/batch_prep_ref.py.  Also the same spline evaluated in float64, for the bounds of
tests/test_elastic_prepare_cpu.py."""
import numpy as np

from batch_prep_ref import edge_codes_separable

F = np.float32
Q_MAX = F(2.0 ** 30)
IDENT = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0)


def grid_position(pf, C, G):
    """g_d = p'_d * k_d + 1 in float32, k_d = float32(G_d - 3) / float32(C_d - 1) (0 when C_d == 1)"""
    k = F(G - 3) / F(C - 1) if C > 1 else F(0.0)
    return F(F(pf) * k) + F(1.0)


def axis_spline(pf, C, G):
    """([w0, w1, w2, w3] float32, [four clamped control indices]) at the flipped output index pf"""
    g = grid_position(pf, C, G)
    i = int(np.floor(g))
    t = F(g - F(i))
    s = F(F(1.0) - t)
    h = F(1.0 / 6.0)
    w0 = F(F(F(s * s) * s) * h)
    w1 = F(F(F(F(F(F(3.0) * t) - F(6.0)) * t) * t) + F(4.0))
    w1 = F(w1 * h)
    w2 = F(F(F(F(F(F(F(-3.0) * t) + F(3.0)) * t) + F(3.0)) * t) + F(1.0))
    w2 = F(w2 * h)
    w3 = F(F(F(t * t) * t) * h)
    return [w0, w1, w2, w3], [min(max(i - 1 + j, 0), G - 1) for j in range(4)]


def sum4(v):
    return F(F(F(v[0] + v[1]) + v[2]) + v[3])


def displacement(disp, pf, crop):
    """D [3] float32 at the flipped output index pf = (p'_0, p'_1, p'_2)"""
    G = disp.shape[1:]
    (w0, i0), (w1, i1), (w2, i2) = (axis_spline(pf[d], crop[d], G[d]) for d in range(3))
    D = []
    for c in range(3):
        outer = []
        for j0 in range(4):
            mid = []
            for j1 in range(4):
                inner = sum4([F(w2[j2] * disp[c, i0[j0], i1[j1], i2[j2]]) for j2 in range(4)])
                mid.append(F(w1[j1] * inner))
            outer.append(F(w0[j0] * sum4(mid)))
        D.append(sum4(outer))
    return D


def lerp(a, b, f):
    return F(a + F(f * F(b - a)))


def prepare_one(image, label, origin, flip, scale, shift, matrix, disp, crop):
    """(x float32 [4,*crop], target int64 [*crop], edge int64 [*crop]) of one sample; matrix / disp / scale may be None"""
    image, label = np.asarray(image, dtype=F), np.asarray(label)
    S = label.shape
    m = [F(v) for v in (matrix if matrix is not None else IDENT)]
    cen = [F(F(C - 1) * F(0.5)) for C in crop]
    x = np.zeros((4,) + tuple(crop), dtype=F)
    t = np.zeros(tuple(crop), dtype=np.int64)

    def tap(c, i):
        return image[c, i[0], i[1], i[2]] if all(0 <= i[d] < S[d] for d in range(3)) else F(0.0)

    with np.errstate(over="ignore", invalid="ignore"):
        for p0 in range(crop[0]):
            for p1 in range(crop[1]):
                for p2 in range(crop[2]):
                    p = (p0, p1, p2)
                    pf = [crop[d] - 1 - p[d] if flip[d] else p[d] for d in range(3)]
                    u = [F(F(pf[d]) - cen[d]) for d in range(3)]
                    q = [F(F(F(F(m[3 * d] * u[0]) + F(m[3 * d + 1] * u[1])) + F(m[3 * d + 2] * u[2])) + cen[d]) for d in range(3)]
                    if disp is not None:
                        D = displacement(disp, pf, crop)
                        q = [F(q[d] + D[d]) for d in range(3)]
                    if not all(abs(v) < Q_MAX for v in q):                # (NaN compares false)
                        continue
                    fl = [np.floor(v) for v in q]
                    fr = [F(q[d] - fl[d]) for d in range(3)]
                    i = [int(fl[d]) + origin[d] for d in range(3)]
                    for c in range(4):
                        r0 = []
                        for d0 in (0, 1):
                            r1 = [lerp(tap(c, (i[0] + d0, i[1] + d1, i[2])), tap(c, (i[0] + d0, i[1] + d1, i[2] + 1)), fr[2]) for d1 in (0, 1)]
                            r0.append(lerp(r1[0], r1[1], fr[1]))
                        x[(c,) + p] = lerp(r0[0], r0[1], fr[0])
                    n = [int(np.floor(F(q[d] + F(0.5)))) + origin[d] for d in range(3)]
                    if all(0 <= n[d] < S[d] for d in range(3)):
                        t[p] = int(label[n[0], n[1], n[2]])
    if scale is not None:
        for c in range(4):
            x[c] = (x[c] * F(scale[c])).astype(F)
            x[c] = (x[c] + F(shift[c])).astype(F)
    t[t == 4] = 3
    return x, t, edge_codes_separable(t)


def displacement64(disp, flip, crop):
    """(D [3, *crop], g [3][C_d]) in float64: the spline of the statement evaluated at the statement's float32 grid positions g_d, the
    weights and the sums in float64"""
    d64 = np.asarray(disp, dtype=np.float64)
    G = d64.shape[1:]
    ws, ix, gs = [], [], []
    for d in range(3):
        pf = [crop[d] - 1 - p if flip[d] else p for p in range(crop[d])]
        g = np.array([float(grid_position(v, crop[d], G[d])) for v in pf])
        i = np.floor(g)
        t = g - i
        s = 1.0 - t
        ws.append(np.stack([s ** 3, 3 * t ** 3 - 6 * t ** 2 + 4, -3 * t ** 3 + 3 * t ** 2 + 3 * t + 1, t ** 3], axis=1) / 6.0)
        ix.append(np.clip(i.astype(np.int64)[:, None] - 1 + np.arange(4)[None, :], 0, G[d] - 1))
        gs.append(g)
    a = sum(ws[2][:, j] * d64[:, :, :, ix[2][:, j]] for j in range(4))                          # [3, G0, G1, C2]
    b = sum(ws[1][:, j][:, None] * a[:, :, ix[1][:, j], :] for j in range(4))                   # [3, G0, C1, C2]
    D = sum(ws[0][:, j][:, None, None] * b[:, ix[0][:, j], :, :] for j in range(4))             # [3, C0, C1, C2]
    return D, gs


def random_image(shape, rng):
    """finite fp32 [4, *shape]: unit normal noise with a different offset and gain per channel"""
    gain = np.array([1.0, 3.5, 0.25, 10.0], dtype=F).reshape(4, 1, 1, 1)
    off = np.array([0.0, -2.0, 5.0, 100.0], dtype=F).reshape(4, 1, 1, 1)
    return (rng.standard_normal((4,) + tuple(shape), dtype=F) * gain + off).astype(F)


def blob_labels(shape, rng, n=10):
    """uint8 labels 0..4: overlapping ellipsoids, a later one painting over an earlier one"""
    g = np.meshgrid(*[np.arange(s, dtype=F) for s in shape], indexing="ij", sparse=True)
    lab = np.zeros(shape, np.uint8)
    for k in range(n):
        c = [rng.uniform(0, s) for s in shape]
        r = [rng.uniform(0.1, 0.35) * max(s, 4) for s in shape]
        lab[sum(((gi - ci) / ri) ** 2 for gi, ci, ri in zip(g, c, r)) < 1.0] = 1 + k % 4
    return lab


def random_grid(shape, amplitude, rng):
    """float32 [3, *shape] ~ U(-amplitude, amplitude)"""
    return rng.uniform(-amplitude, amplitude, (3,) + tuple(shape)).astype(F)
