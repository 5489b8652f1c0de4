"""The nonzero box on the host: the numpy statement (tests/nonzero_box_ref.py, utils.data.nonzero_boxes_host / nonzero_box,
predict_overlap.nonzero_box) against a brute-force loop, box_crop_origin's invariant and uniformity, draw_params(box=),
NpzCropSource / DeviceBraTS(crop_nonzero=True) on the CPU with DataLoader workers, the empty-subject fallback and refusals."""
import functools
import inspect

import numpy as np
import pytest
import torch

import nonzero_box_ref as ref
import predict_overlap as po
from utils import data
from utils import synthetic as syn


def _volume(shape, seed, lo, hi, special=True):
    """zeros (of both signs) with a dense random block [lo, hi) and, in it, one denormal, one NaN and one inf voxel"""
    rng = np.random.default_rng(seed)
    x = np.zeros((4,) + shape, dtype=np.float32)
    x[:, ::2] = -0.0
    sl = tuple(slice(a, b) for a, b in zip(lo, hi))
    x[(slice(None),) + sl] = rng.standard_normal((4,) + tuple(b - a for a, b in zip(lo, hi))).astype(np.float32)
    if special:
        x[1][lo] = np.float32(1e-45)
        x[2][tuple(b - 1 for b in hi)] = np.nan
        x[3][lo[0], hi[1] - 1, lo[2]] = np.inf
    return x


# ------------------------------------------------------------------ the statement
@pytest.mark.parametrize("shape", [(5, 4, 3), (3, 7, 1), (1, 1, 9)])
def test_statement_against_brute_force(shape):
    rng = np.random.default_rng(sum(shape))
    cases = [np.zeros((4,) + shape, np.float32), -np.zeros((4,) + shape, np.float32)]
    for bits in (0x00000001, 0x80000001, 0x7F800000, 0x7FC00000, 0x3F800000):             # denormals of both signs, inf, NaN, 1.0
        for _ in range(3):
            x = np.zeros((4,) + shape, np.float32)
            x[::2] = -0.0
            x.view(np.uint32)[(int(rng.integers(4)),) + tuple(int(rng.integers(s)) for s in shape)] = bits
            cases.append(x)
    for _ in range(6):
        cases.append((rng.standard_normal((4,) + shape) * (rng.random((1,) + shape) < 0.2)).astype(np.float32))
    for x in cases:
        wb, wc = ref.brute_box_count(x)
        gb, gc = ref.box_count(x)
        assert np.array_equal(gb, wb) and gc == wc
        hb, hc = data.nonzero_boxes_host(x[None])
        assert hb.dtype == np.int32 and hc.dtype == np.int64 and np.array_equal(hb[0], wb) and int(hc[0]) == wc
        got = data.nonzero_box(torch.from_numpy(x))
        assert got == (None if wc == 0 else (tuple(int(v) for v in wb[:3]), tuple(int(v) for v in wb[3:])))


def test_union_margin_and_clip():
    shape = (12, 10, 9)
    x = np.stack([_volume(shape, 1, (2, 3, 4), (6, 5, 7)), np.zeros((4,) + shape, np.float32), _volume(shape, 2, (4, 1, 5), (9, 4, 6))])
    boxes = ref.boxes_counts(x)[0]
    assert ref.union_box(boxes, shape) == ((2, 1, 4), (9, 5, 7))
    for margin in (0, 1, 3, 50):
        want = ref.union_box(boxes, shape, margin)
        assert po.nonzero_box(torch.from_numpy(x), margin) == want
        assert all(isinstance(v, int) for t in want for v in t)
    assert ref.union_box(boxes, shape, 50) == ((0, 0, 0), shape)
    assert po.nonzero_box(torch.from_numpy(x[1:2])) is None and ref.union_box(boxes[1:2], shape) is None
    assert po.nonzero_box(torch.from_numpy(x[:1]), 1) == ((1, 2, 3), (7, 6, 8))


# ------------------------------------------------------------------ box_crop_origin
AXES = {                    # (S, crop, a, b)
    "box >= crop": (40, 8, 10, 30),
    "box == crop": (40, 8, 10, 18),
    "box < crop": (40, 16, 12, 17),
    "box at the low face": (40, 8, 0, 13),
    "box at the high face": (40, 8, 29, 40),
    "small box at the low face": (40, 16, 0, 3),
    "small box at the high face": (40, 16, 37, 40),
    "box is the volume": (40, 8, 0, 40),
    "S < crop": (10, 16, 2, 7),
    "S == crop": (16, 16, 3, 9),
}
DRAWS = 4000


@pytest.mark.parametrize("name", sorted(AXES))
def test_origin_invariant_and_uniformity(name):
    s, c, a, b = AXES[name]
    first, last = ref.origin_range(s, c, a, b)
    assert 0 <= first <= last <= max(s - c, 0), "the range is never empty and lies in random_crop_origin's"
    rng = np.random.default_rng(7)
    # the axis under test in each position, the other two axes in another case
    others = [AXES["box >= crop"], AXES["box < crop"]]
    seen = np.zeros(last - first + 1, dtype=np.int64)
    for n in range(DRAWS):
        pos = n % 3
        axes = others[:pos] + [(s, c, a, b)] + others[pos:]
        full, crop = tuple(t[0] for t in axes), tuple(t[1] for t in axes)
        box = (tuple(t[2] for t in axes), tuple(t[3] for t in axes))
        o = data.box_crop_origin(full, crop, box, rng)
        assert all(isinstance(v, int) for v in o)
        for v, (s_, c_, a_, b_) in zip(o, axes):
            assert 0 <= v <= max(s_ - c_, 0)
            assert ref.overlap(v, c_, a_, b_) == min(c_, b_ - a_)            # the crop lies in the box, or the box in the crop
        seen[o[pos] - first] += 1
    # every origin of the range is drawn, each within 5 standard deviations of DRAWS / k (a binomial count; 5 sigma: 6e-7 a value)
    k = seen.size
    p = 1.0 / k
    assert np.all(np.abs(seen - DRAWS * p) <= 5.0 * np.sqrt(DRAWS * p * (1.0 - p)) + 1e-9), (name, seen)


def test_origin_makes_random_crop_origins_calls():
    """one rng.integers call per axis, as random_crop_origin makes: two generators stay in step when the ranges are equal"""
    full, crop = (40, 30, 20), (8, 8, 8)
    a, b = np.random.default_rng(3), np.random.default_rng(3)
    for _ in range(50):
        assert data.box_crop_origin(full, crop, ((0, 0, 0), full), a) == data.random_crop_origin(full, crop, b)
    assert a.integers(0, 2 ** 62) == b.integers(0, 2 ** 62)
    with pytest.raises(ValueError):
        data.box_crop_origin(full, crop, ((0, 0, 0), (41, 30, 20)), a)
    with pytest.raises(ValueError):
        data.box_crop_origin(full, crop, ((5, 0, 0), (5, 30, 20)), a)


# ------------------------------------------------------------------ draw_params
def _fields(p):
    return [(k, getattr(p, k)) for k in sorted(data.AugParams.__slots__)]


def _same(p, q):
    for (k, a), (k2, b) in zip(_fields(p), _fields(q)):
        assert k == k2
        if isinstance(a, np.ndarray) or isinstance(b, np.ndarray):
            assert a is not None and b is not None and a.dtype == b.dtype and a.tobytes() == b.tobytes(), k
        else:
            assert a == b, k
    return True


def test_draw_params_without_a_box_moves_nothing():
    assert inspect.signature(data.draw_params).parameters["box"].default is None
    full, crop = (40, 36, 31), (16, 20, 24)
    kw = dict(flip=True, intensity=0.1, rotate=10.0, scale=0.1, elastic=2.0, blur=1.0, noise=0.1, gamma=0.3, bias=0.3, contrast=0.2,
              lowres=0.6)
    for index in range(6):
        for k in ({}, kw):
            assert _same(data.draw_params(5, 2, index, full, crop, box=None, **k), data.draw_params(5, 2, index, full, crop, **k))


def test_draw_params_with_a_box():
    full, crop, box = (40, 36, 31), (16, 20, 24), ((10, 4, 8), (30, 15, 29))
    moved = 0
    for index in range(40):
        p = data.draw_params(5, 0, index, full, crop, flip=True, box=box)
        rng = np.random.default_rng([5, 0, index])
        assert p.origin == data.box_crop_origin(full, crop, box, rng)                      # the first draws of the stream
        assert p.flip == tuple(bool(u < 0.5) for u in rng.random(3))
        for d in range(3):
            assert ref.overlap(p.origin[d], crop[d], box[0][d], box[1][d]) == min(crop[d], box[1][d] - box[0][d])
        moved += p.origin != data.draw_params(5, 0, index, full, crop, flip=True).origin
    assert moved >= 30


# ------------------------------------------------------------------ the datasets
FULL, CROP = (40, 36, 31), (16, 20, 24)
BOXES = [((6, 5, 4), (30, 29, 27)), ((12, 0, 10), (20, 36, 18)), None]          # the last subject is zero everywhere


@functools.lru_cache(maxsize=None)
def _subjects():
    out = []
    for i, box in enumerate(BOXES):
        if box is None:
            x, t = syn.synthetic_volume(i, FULL, 4321)
            x, t = x * 0.0, t * 0                                               # zeros of both signs
        else:
            x, t = syn.synthetic_masked_volume(i, FULL, box, 4321)
        out.append((x, t.to(torch.uint8)))
    return out


def test_masked_subject_has_its_box():
    for (x, t), box in zip(_subjects(), BOXES):
        assert data.nonzero_box(x) == box
        b, n = ref.box_count(x.numpy())
        assert (None if n == 0 else (tuple(int(v) for v in b[:3]), tuple(int(v) for v in b[3:]))) == box
    assert bool((_subjects()[2][0] == 0).all()) and bool(torch.signbit(_subjects()[2][0]).any())


def _check_invariant(ds, epochs=(0, 1, 2)):
    for epoch in epochs:
        ds.set_epoch(epoch)
        for i, box in enumerate(BOXES):
            o = ds.params(i).origin
            if box is None:
                assert o == data.draw_params(ds.seed, epoch, i, FULL, CROP).origin     # drawn as if the option were off
                continue
            for d in range(3):
                assert ref.overlap(o[d], CROP[d], box[0][d], box[1][d]) == min(CROP[d], box[1][d] - box[0][d])


@pytest.mark.parametrize("normalize", [False, True])
def test_crop_source_batches_satisfy_the_invariant(normalize):
    src = data.NpzCropSource(_subjects(), CROP, seed=5, normalize=normalize, crop_nonzero=True)
    plain = data.NpzCropSource(_subjects(), CROP, seed=5, normalize=normalize)
    moved = 0
    for epoch in (0, 1, 2):
        src.set_epoch(epoch)
        plain.set_epoch(epoch)
        for i, box in enumerate(BOXES):
            img, lab, idx, b6 = src[i]
            assert idx == i and b6 == (tuple(FULL) + (0, 0, 0) if box is None else box[0] + box[1])
            assert len(plain[i]) == 3
            o = data.draw_params(5, epoch, i, FULL, CROP, **({} if box is None else {"box": box})).origin
            full_img, full_lab = src.load(i)
            assert torch.equal(img, data.crop_pad(full_img, o, CROP)) and torch.equal(lab, data.crop_pad(full_lab, o, CROP))
            if box is None:
                assert torch.equal(img, plain[i][0])
            else:
                moved += o != data.draw_params(5, epoch, i, FULL, CROP).origin
                for d in range(3):
                    assert ref.overlap(o[d], CROP[d], box[0][d], box[1][d]) == min(CROP[d], box[1][d] - box[0][d])
    assert moved >= 4
    assert src.boxes == {i: (tuple(FULL) + (0, 0, 0) if b is None else b[0] + b[1]) for i, b in enumerate(BOXES)}   # from the raw image


@pytest.mark.parametrize("aug", [{}, {"flip": True, "rotate": 10.0, "elastic": 2.0}], ids=["plain", "resampled"])
def test_cached_and_staged_cpu_instances_agree(aug):
    order = [[2, 0], [1]]
    cached = data.DeviceBraTS(_subjects(), "cpu", CROP, seed=5, cache=True, normalize=True, crop_nonzero=True, **aug)
    staged = data.DeviceBraTS(_subjects(), "cpu", CROP, seed=5, cache=False, normalize=True, crop_nonzero=True, **aug)
    off = data.DeviceBraTS(_subjects(), "cpu", CROP, seed=5, cache=True, normalize=True, crop_nonzero=False, **aug)
    plain = data.DeviceBraTS(_subjects(), "cpu", CROP, seed=5, cache=True, normalize=True, **aug)
    _check_invariant(cached)
    for epoch in (0, 1):
        for ds in (cached, staged, off, plain):
            ds.set_epoch(epoch)
        want = list(cached.batches(order))
        for workers in (0, 2):
            fresh = data.DeviceBraTS(_subjects(), "cpu", CROP, seed=5, cache=False, normalize=True, crop_nonzero=True, **aug)
            fresh.set_epoch(epoch)
            for ds in (staged, fresh):                      # `fresh` learns every box from the loader's items
                got = list(ds.batches(order, num_workers=workers))
                for g, w in zip(got, want):
                    for a, b in zip(g, w):
                        assert a.dtype == b.dtype and torch.equal(a, b), (epoch, workers)
                assert all(ds.params(i) == cached.params(i) for i in range(3))
        for g, w in zip(off.batches(order), plain.batches(order)):          # off: the dataset built without the keyword
            assert all(torch.equal(a, b) for a, b in zip(g, w))
    _check_invariant(staged)


def test_oversampled_origins_are_not_moved_by_the_box():
    both = data.DeviceBraTS(_subjects()[:2], "cpu", CROP, seed=5, oversample=1.0, crop_nonzero=True)
    fg = data.DeviceBraTS(_subjects()[:2], "cpu", CROP, seed=5, oversample=1.0)
    for epoch in (0, 1, 2):
        both.set_epoch(epoch)
        fg.set_epoch(epoch)
        for i in range(2):
            if int(fg.foreground[i][0].sum()) > 0:
                assert both.params(i).origin == fg.params(i).origin


# ------------------------------------------------------------------ refusals
def test_refusals():
    x = torch.zeros((4, 5, 4, 3))
    for bad in (x.double(), x[:3], x[None], torch.zeros((4, 0, 4, 3)), x.numpy()):
        with pytest.raises(ValueError):
            data.nonzero_box(bad)
    for bad in (x, x[None].double(), x[None][:, :3], x.numpy()[None]):
        with pytest.raises(ValueError):
            po.nonzero_box(bad)
    for margin in (-1, 0.5):
        with pytest.raises(ValueError):
            po.nonzero_box(x[None], margin)
    from train_no_amp import build_parser, check_foreground
    args = build_parser().parse_args(["--crop_nonzero", "true"])
    assert args.crop_nonzero is True and build_parser().parse_args([]).crop_nonzero is False
    with pytest.raises(SystemExit):
        check_foreground(args)                              # --device_data off
    check_foreground(build_parser().parse_args(["--crop_nonzero", "true", "--device_data", "staged"]))
