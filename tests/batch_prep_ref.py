"""Independent numpy restatement of the device batch preparation (csrc/prep.hip, utils.data.prepare_batch):

  source coordinate  s_i = o_i + (flip_i ? C_i-1-p_i : p_i); s_i >= S_i -> image 0, label 0
  x                  copied, or float32(float32(v * scale_c) + shift_c) (two roundings)
  target             label with 4 -> 3
  edge               the separable formulation: six bits per voxel (any_k, all_k of label == k, k = 1..3), OR / AND over the 3-box
                     one axis at a time with out-of-crop voxels the identity (0 for OR, 1 for AND), band_k = any_k & ~all_k,
                     membership-coded 1/2/4/6/7/8/5 as utils.synthetic.edge_codes codes it.

It shares no code with utils.data or utils.synthetic, so the tests can hold both the torch statement and the kernel against it."""
import numpy as np

CODE = np.array([0, 1, 2, 6, 4, 7, 8, 5], dtype=np.int64)     # band bits (b1 | b2 << 1 | b4 << 2) -> edge code


def _box(a, axis, op, ident):
    """3-wide OR / AND along `axis`, positions outside the array acting as `ident`"""
    pad = [(0, 0)] * a.ndim
    pad[axis] = (1, 1)
    p = np.pad(a, pad, constant_values=ident)
    n = a.shape[axis]
    sl = lambda k: tuple(slice(k, k + n) if d == axis else slice(None) for d in range(a.ndim))
    return op(op(p[sl(0)], p[sl(1)]), p[sl(2)])


def edge_codes_separable(target):
    """edge codes of an int label volume (values 0..3) by separable any / all passes"""
    t = np.asarray(target)
    band = np.zeros(t.shape, dtype=np.int64)
    for k in (1, 2, 3):
        eq = t == k
        anyk, allk = eq.copy(), eq.copy()
        for ax in range(3):
            anyk = _box(anyk, ax, np.logical_or, False)
            allk = _box(allk, ax, np.logical_and, True)
        band |= (anyk & ~allk).astype(np.int64) << (k - 1)
    return CODE[band]


def crop_source(vol, origin, flip, crop):
    """vol [..., S0, S1, S2] -> [..., C0, C1, C2] read at s_i = o_i + (flip_i ? C_i-1-p_i : p_i), zero outside the volume"""
    vol = np.asarray(vol)
    S = vol.shape[-3:]
    out = np.zeros(vol.shape[:-3] + tuple(crop), dtype=vol.dtype)
    idx, ok = [], []
    for d in range(3):
        p = np.arange(crop[d])
        s = origin[d] + (crop[d] - 1 - p if flip[d] else p)
        idx.append(np.minimum(s, S[d] - 1))
        ok.append(s < S[d])
    g = vol[..., idx[0][:, None, None], idx[1][None, :, None], idx[2][None, None, :]]
    m = ok[0][:, None, None] & ok[1][None, :, None] & ok[2][None, None, :]
    out[..., m] = g[..., m]
    return out


def prepare_one(image, label, origin, flip, scale, shift, crop):
    """(x float32 [4,*crop], target int64 [*crop], edge int64 [*crop]) of one sample"""
    x = crop_source(np.asarray(image, dtype=np.float32), origin, flip, crop)
    if scale is not None:
        sc = np.asarray(scale, dtype=np.float32).reshape(4, 1, 1, 1)
        sh = np.asarray(shift, dtype=np.float32).reshape(4, 1, 1, 1)
        x = (x * sc).astype(np.float32)
        x = (x + sh).astype(np.float32)
    t = crop_source(np.asarray(label).astype(np.int64), origin, flip, crop)
    t[t == 4] = 3
    return x, t, edge_codes_separable(t)


def prepare(images, labels, params, crop):
    xs, ts, es = zip(*(prepare_one(i, l, p.origin, p.flip, p.scale, p.shift, crop) for i, l, p in zip(images, labels, params)))
    return np.stack(xs), np.stack(ts), np.stack(es)


def normalize_ref(image):
    """float64 two-pass z-score of each channel over the voxels whose float32 ((x0 + x1) + x2) + x3 > 0 (a new float32 array)"""
    a = np.array(image, dtype=np.float32, copy=True)
    m = (((a[0] + a[1]) + a[2]) + a[3]) > 0
    if m.any():
        for c in range(4):
            v = a[c][m].astype(np.float64)
            mean = v.mean()
            std = np.sqrt(((v - mean) ** 2).mean())
            if std > 0:
                a[c][m] = ((v - mean) / std).astype(np.float32)
    return a, m


def random_labels(shape, rng, p=(0.4, 0.2, 0.2, 0.1, 0.1)):
    """dense random labels 0..4 (uint8)"""
    return rng.choice(5, size=shape, p=p).astype(np.uint8)


def nested_labels(shape, rng):
    """BraTS-like nested regions: oedema 2 around core 1 around enhancing 4 (uint8)"""
    c = [s * (0.35 + 0.3 * rng.random()) for s in shape]
    r = 0.3 * min(shape)
    g = np.meshgrid(*[np.arange(s) for s in shape], indexing="ij")
    rr = np.sqrt(sum(((gi - ci) / (1.0 + 0.2 * k)) ** 2 for k, (gi, ci) in enumerate(zip(g, c))))
    lab = np.zeros(shape, np.uint8)
    lab[rr < r] = 2
    lab[rr < 0.6 * r] = 1
    lab[rr < 0.3 * r] = 4
    return lab


def random_image(shape, rng):
    """fp32 [4, *shape] with signed zeros, negatives and wide exponents (bit patterns must pass through unchanged)"""
    x = (rng.standard_normal((4,) + tuple(shape)) * np.exp2(rng.integers(-20, 20, (4,) + tuple(shape)))).astype(np.float32)
    flat = x.reshape(-1)
    flat[rng.integers(0, flat.size, max(1, flat.size // 50))] = -0.0
    return x
