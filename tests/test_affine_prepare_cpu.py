"""Rotated / zoomed crops on the CPU: the float32 statement of utils.data (_resample_cpu, through prepare_batch) against the plain
crop, torch.rot90 and a float64 evaluation of the same formulas (tests/affine_prep_ref.py); draw_params, source_box, the staged mode
and the train_no_amp flags.

Bounds of the float64 cross-check, derived and not tuned.  With e_d = 4 * 2^-24 * (sum_j |M_dj| |u_j| + c_d):
  coordinates  |q32_d - q64_d| <= e_d: three products and three sums, each within 2^-24 relative of a partial result that
               sum_j |M_dj| |u_j| + c_d bounds (the float64 side adds nothing at this scale).
  image        trilinear interpolation T(q) is continuous in q, also across cell borders, and linear along an axis inside a cell with
               slope = a difference of two lerped taps, so |slope| <= 2 A with A = max |image| (taps outside the volume are 0).  Hence
               |T(q32) - T(q64)| <= 2 A sum_d e_d.  The float32 evaluation at q32 adds: f_d = q_d - floor(q_d) rounded once, 2^-24 per axis
               -> 3 * 2 A * 2^-24; and three lerp levels of three roundings each on magnitudes <= 2 A, 2 A and 3 A -> 7 A * 2^-24 per
               level, passed on by the next level with weights (1 - f) + f = 1 -> 21 A * 2^-24.  Together, with slack for the
               intermediate magnitudes:  |x32 - x64| <= 2 A sum_d e_d + 30 A * 2^-24.
  labels       floor(q + 0.5) can differ only where q64_d + 0.5 lies within e_d (+ 2^-24 |q_d + 0.5| for the rounded sum) of an integer
               for some d.  Such voxels are at most 0.1 % of a case (a condition on the inputs), and all others agree exactly."""
import numpy as np
import pytest
import torch

import affine_prep_ref as A

IDENT = (1, 0, 0, 0, 1, 0, 0, 0, 1)
FLIPS = [(a, b, c) for a in (False, True) for b in (False, True) for c in (False, True)]


def _src(shape, seed):
    rng = np.random.default_rng(seed)
    return torch.from_numpy(A.random_image(shape, rng)), torch.from_numpy(A.blob_labels(shape, rng))


def test_aug_params_matrix_slot():
    from utils import data
    p = data.AugParams((1, 2, 3), (True, False, True))
    assert p.matrix is None and repr(p) == "AugParams(origin=(1, 2, 3), flip=(True, False, True), scale=None, shift=None)"
    m = A.MATRICES[0]
    q = data.AugParams((1, 2, 3), (True, False, True), matrix=m.reshape(3, 3))
    assert q.matrix == tuple(float(v) for v in m) and q != p and q == data.AugParams((1, 2, 3), (True, False, True), matrix=m)
    assert "matrix=" in repr(q) and q.at_origin((-4, 0, 9)).matrix == q.matrix and q.at_origin((-4, 0, 9)).origin == (-4, 0, 9)
    with pytest.raises(ValueError):
        data.AugParams((0, 0, 0), matrix=[1.0, 0.0, 0.0])
    np.testing.assert_array_equal(data.rotation_zoom_matrix((10.0, -7.0, 15.0), 1.1), m)


@pytest.mark.parametrize("crop,origins", [((12, 16, 20), [(0, 0, 0), (5, 9, 3), (18, 14, 20)]),        # inside the 30 x 30 x 40 volume
                                          ((34, 16, 44), [(0, 3, 0), (0, 14, 0)])])                   # larger than it on two axes
def test_identity_equals_plain_crop(crop, origins):
    from utils import data
    img, lab = _src((30, 30, 40), 1)
    for o in origins:
        for flip in FLIPS:
            sc, sh = ((0.9, 1.1, 1.0, 1.2), (0.1, -0.2, 0.0, 0.3)) if flip[0] else (None, None)
            want = data.prepare_batch([img], [lab], [data.AugParams(o, flip, sc, sh)], crop)
            got = data.prepare_batch([img], [lab], [data.AugParams(o, flip, sc, sh, IDENT)], crop)
            for g, w in zip(got, want):
                assert g.dtype == w.dtype and torch.equal(g, w)


def test_quarter_turn_equals_rot90():
    """M = [[1,0,0],[0,0,-1],[0,1,0]]: out[a, b, c] = crop[a, C-1-c, b] = torch.rot90(crop, -1, (1, 2))"""
    from utils import data
    from utils import synthetic as syn
    img, lab = _src((30, 36, 40), 2)
    crop, o = (16, 16, 16), (7, 11, 20)
    x, t, e = data.prepare_batch([img], [lab], [data.AugParams(o, matrix=(1, 0, 0, 0, 0, -1, 0, 1, 0))], crop)
    px, pt, _ = data.prepare_batch([img], [lab], [data.AugParams(o)], crop)
    assert torch.equal(x, torch.rot90(px, -1, (3, 4)))
    assert torch.equal(t, torch.rot90(pt, -1, (2, 3)))
    assert torch.equal(e[0], syn.edge_codes(t[0]))
    # about axis 2: out[a, b, c] = crop[C-1-b, a, c]
    x, t, _ = data.prepare_batch([img], [lab], [data.AugParams(o, matrix=(0, -1, 0, 1, 0, 0, 0, 0, 1))], crop)
    assert torch.equal(x, torch.rot90(px, -1, (2, 3))) and torch.equal(t, torch.rot90(pt, -1, (1, 2)))


@pytest.mark.parametrize("case", range(len(A.CASES)))
def test_float64_cross_check(case):
    from utils import data
    angles, zoom, crop = A.CASES[case]
    m = A.matrix(angles, zoom)
    S = (150, 160, 140) if crop[0] == 128 else (60, 50, 80)
    img, lab = _src(S, 10 + case)
    origin = tuple((s - c) // 2 for s, c in zip(S, crop))
    flip = (False, True, False) if case == 2 else (False, False, False)
    p = data.AugParams(origin, flip, matrix=m)
    x, t, _ = data.prepare_batch([img], [lab], [p], crop)
    q32, ok = data._affine_coords(p, crop)
    x64, t64, q64, e = A.resample64(img.numpy(), lab.numpy(), m, origin, flip, crop)
    assert ok.all()
    worst = max(float((np.abs(q32[d].astype(np.float64) - q64[d]) / e[d]).max()) for d in range(3))
    print("case %d: worst |q32 - q64| / bound = %.3f" % (case, worst))
    assert worst <= 1.0
    amax = float(img.abs().max())
    bound = 2.0 * amax * (e[0] + e[1] + e[2]) + 30.0 * amax * 2.0 ** -24
    err = np.abs(x[0].numpy().astype(np.float64) - x64)
    print("case %d: worst image error / bound = %.3f" % (case, float((err / bound).max())))
    assert np.all(err <= bound)
    near = np.zeros(crop, dtype=bool)
    for d in range(3):
        h = q64[d] + 0.5
        near |= np.abs(h - np.round(h)) <= e[d] + 2.0 ** -24 * np.abs(h)
    frac = float(near.mean())
    print("case %d: %.4f %% of the voxels within the coordinate bound of a label tie" % (case, 100.0 * frac))
    assert frac <= 1e-3
    t64 = t64.copy()
    t64[t64 == 4] = 3
    assert np.array_equal(t[0].numpy()[~near], t64[~near])
    assert 0 < int((t[0] > 0).sum()) < t[0].numel() and len(np.unique(t[0].numpy())) == 4


def test_non_representable_coordinates_read_nothing():
    """|q| >= 2^30 or NaN (a finite but huge matrix): image 0 (then the intensity map), label 0"""
    from utils import data
    img, lab = _src((12, 12, 12), 3)
    p = data.AugParams((0, 0, 0), scale=(2, 2, 2, 2), shift=(1, 2, 3, 4), matrix=(3e38, 3e38, 0, 0, 1, 0, 0, 0, 1e30))
    x, t, e = data.prepare_batch([img], [lab], [p], (4, 6, 8))
    assert torch.equal(x[0, :, 0, 0, 0], torch.tensor([1.0, 2.0, 3.0, 4.0])) and bool((x[0, 1] == 2.0).all())
    assert int(t.abs().sum()) == 0 and int(e.abs().sum()) == 0


def _todays_draw(seed, epoch, index, full, crop, flip, intensity):
    """draw_params as it was before the matrix: the stream positions are pinned here"""
    rng = np.random.default_rng([seed, epoch, index])
    origin = tuple(int(rng.integers(0, max(f - c, 0) + 1)) for f, c in zip(full, crop))
    fl = tuple(bool(u < 0.5) for u in rng.random(3)) if flip else (False, False, False)
    scale = shift = None
    if intensity > 0.0:
        scale = tuple(float(v) for v in rng.uniform(1.0 - intensity, 1.0 + intensity, 4).astype(np.float32))
        shift = tuple(float(v) for v in rng.uniform(-intensity, intensity, 4).astype(np.float32))
    return origin, fl, scale, shift, rng


def test_draw_params_stability():
    from utils import data
    full, crop = (240, 240, 155), (128, 128, 128)
    for seed in (1000, 3):
        for epoch in (0, 4):
            for index in (0, 17):
                for flip, inten in ((False, 0.0), (True, 0.0), (False, 0.2), (True, 0.1)):
                    o, fl, sc, sh, rng = _todays_draw(seed, epoch, index, full, crop, flip, inten)
                    off = data.draw_params(seed, epoch, index, full, crop, flip, inten)
                    assert (off.origin, off.flip, off.scale, off.shift, off.matrix) == (o, fl, sc, sh, None)
                    assert off == data.draw_params(seed, epoch, index, full, crop, flip, inten, rotate=0.0, scale=0.0)
                    on = data.draw_params(seed, epoch, index, full, crop, flip, inten, rotate=15.0, scale=0.2)
                    assert (on.origin, on.flip, on.scale, on.shift) == (o, fl, sc, sh) and on.matrix is not None
                    assert on == data.draw_params(seed, epoch, index, full, crop, flip, inten, rotate=15.0, scale=0.2)
                    angles = rng.uniform(-15.0, 15.0, 3)                 # drawn after everything else
                    zoom = float(rng.uniform(0.8, 1.2))
                    assert on.matrix == tuple(float(v) for v in A.matrix(angles, zoom))
    rot = data.draw_params(1, 2, 3, full, crop, rotate=20.0)
    m = np.asarray(rot.matrix, dtype=np.float64).reshape(3, 3)
    np.testing.assert_allclose(m @ m.T, np.eye(3), atol=1e-6)            # a pure rotation
    zm = np.asarray(data.draw_params(1, 2, 3, full, crop, scale=0.3).matrix).reshape(3, 3)
    assert zm[0, 0] == zm[1, 1] == zm[2, 2] and 1 / 1.3 <= zm[0, 0] <= 1 / 0.7 and zm[0, 1] == 0.0
    assert data.draw_params(1, 2, 3, full, crop, rotate=20.0) != data.draw_params(1, 2, 4, full, crop, rotate=20.0)


@pytest.mark.parametrize("crop", [(128, 128, 128), (33, 47, 70), (1, 1, 5)])
def test_source_box_contains_every_tap(crop):
    from utils import data
    for m in A.MATRICES + [np.asarray(IDENT, dtype=np.float32)]:
        for flip in ((False, False, False), (True, True, True)):
            p = data.AugParams((0, 0, 0), flip, matrix=m)
            box = p.source_box(crop)
            q, ok = data._affine_coords(p, crop)
            assert ok.all()
            for d in range(3):
                lo, hi = box[d]
                assert isinstance(lo, int) and isinstance(hi, int)
                i = np.floor(q[d]).astype(np.int64)
                n = np.floor(q[d] + np.float32(0.5)).astype(np.int64)
                assert lo <= i.min() and i.max() + 1 < hi and lo <= n.min() and n.max() < hi
    assert data.AugParams((3, 4, 5)).source_box(crop) == tuple((0, c) for c in crop)


def test_staged_equals_cache_cpu():
    from utils import data
    shapes = [(40, 44, 36), (30, 52, 41), (36, 36, 36)]
    subjects = [_src(S, 20 + k) for k, S in enumerate(shapes)]
    crop = (24, 28, 20)
    kw = dict(seed=5, flip=True, intensity=0.2, rotate=15.0, scale=0.2)
    cache = data.DeviceBraTS(subjects, "cpu", crop, **kw)
    staged = data.DeviceBraTS(subjects, "cpu", crop, cache=False, **kw)
    for epoch in (0, 3):
        cache.set_epoch(epoch); staged.set_epoch(epoch)
        assert all(cache.params(i).matrix is not None for i in range(3))
        items = [staged.source[i] for i in range(3)]
        assert len({tuple(it[0].shape) for it in items}) > 1 and all(it[0].is_contiguous() and it[1].is_contiguous() for it in items)
        assert all(it[0].numel() < 4 * np.prod(S) for it, S in zip(items, shapes))
        imgs, labs, idx = data._collate_crops(items, stack=False)
        assert isinstance(imgs, list) and isinstance(labs, list) and idx == [0, 1, 2]
        want = cache.batch([2, 0, 1])
        for got in (staged.batch([2, 0, 1]), next(iter(staged.batches([[2, 0, 1]])))):
            for g, w in zip(got, want):
                assert torch.equal(g, w)
            assert torch.equal(got[0].view(torch.int32), want[0].view(torch.int32))
    # the batch is the CPU statement at draw_params' parameters
    params = [data.draw_params(5, 3, i, shapes[i], crop, True, 0.2, 15.0, 0.2) for i in (2, 0, 1)]
    ref = data.prepare_batch([subjects[i][0] for i in (2, 0, 1)], [subjects[i][1] for i in (2, 0, 1)], params, crop)
    assert all(torch.equal(a, b) for a, b in zip(ref, want))
    # without a matrix the staged items and the collate output stay what they were
    plain = data.DeviceBraTS(subjects, "cpu", crop, seed=5, flip=True, intensity=0.2, cache=False)
    it = plain.source[1]
    assert tuple(it[0].shape) == (4,) + crop and tuple(it[1].shape) == crop
    st = data._collate_crops([plain.source[i] for i in range(3)])
    assert isinstance(st[0], torch.Tensor) and tuple(st[0].shape) == (3, 4) + crop


def test_train_flags():
    import train_no_amp as T
    a = T.build_parser().parse_args([])
    assert a.aug_rotate == 0.0 and a.aug_scale == 0.0
    b = T.build_parser().parse_args(["--device_data", "cache", "--aug_rotate", "15", "--aug_scale", "0.2"])
    assert b.aug_rotate == 15.0 and b.aug_scale == 0.2
    for flags in (["--aug_rotate", "10"], ["--aug_scale", "0.1"]):
        with pytest.raises(SystemExit, match="device_data"):
            T.main(["--synthetic", "1"] + flags)
