"""Foreground-oversampled crops on the host: utils.data.class_locations' CPU statement against tests/foreground_ref.py, the draw
(foreground_origin) and its hook in draw_params, NpzCropSource / DeviceBraTS(device="cpu") in both modes, and the refusals.  No GPU."""
import functools

import numpy as np
import pytest
import torch

import foreground_ref as ref
from cwf import _lib
from utils import data
from utils import synthetic as syn

T = _lib.LOCATIONS_TILE
AUG = dict(flip=True, intensity=0.1, rotate=15.0, scale=0.2, elastic=2.0, elastic_grid=6, blur=1.0, noise=0.1, gamma=0.3, bias=0.3,
           bias_grid=5, contrast=0.3, lowres=0.6)


def _same(got, want):
    counts, table = got
    return (counts.dtype == torch.int64 and table.dtype == torch.int32 and np.array_equal(counts.numpy(), want[0])
            and np.array_equal(table.numpy(), want[1]))


@pytest.mark.parametrize("shape", [(5, 3, 7), (24, 20, 17), (1, 1, T + 1)])
def test_cpu_statement_equals_the_restatement(shape):
    families = ref.label_families(shape, T)
    assert {"background", "one_class", "single_first", "single_last", "foreign", "runs16", "lanes64"} <= set(families)
    assert ("single_tile_start" in families) == (int(np.prod(shape)) > T)
    for name, lab in families.items():
        for masks, K in ((ref.FOREGROUND_CLASSES, 4096), (ref.OVERLAPPING, 64), ((0b1000,), 1), (ref.EIGHT, 7)):
            assert _same(data.class_locations(torch.from_numpy(lab.copy()), masks, K), ref.class_locations(lab, masks, K)), (name, masks, K)
    lab = families["mixed"]
    counts, table = data.class_locations(torch.from_numpy(lab.copy()))          # the defaults: classes 1, 2, 3 and 4096 entries
    assert table.shape == (3, 4096) and _same((counts, table), ref.class_locations(lab, ref.FOREGROUND_CLASSES, 4096))


def test_table_is_every_voxel_or_an_evenly_ranked_sample():
    lab = syn.synthetic_volume(0, (24, 20, 17))[1].to(torch.uint8)
    assert all(int((lab == c).sum()) > 0 for c in (1, 2, 3))
    n2 = int((lab == 2).sum())
    counts, table = data.class_locations(lab, (0b0100,), n2 + 5)               # n <= K: the region itself, then -1
    assert int(counts[0]) == n2 and np.array_equal(table[0, :n2].numpy(), np.flatnonzero(lab.numpy().reshape(-1) == 2))
    assert bool((table[0, n2:] == -1).all())
    counts, table = data.class_locations(lab, (0b0100,), 16)                   # n > K: ranks floor(j n / 16), strictly increasing
    want = np.flatnonzero(lab.numpy().reshape(-1) == 2)[[(j * n2) // 16 for j in range(16)]]
    assert n2 > 16 and np.array_equal(table[0].numpy(), want) and bool((np.diff(table[0].numpy()) > 0).all())


def test_a_voxel_knows_its_entry_from_its_rank():
    """what lets the kernel decide per voxel without a search: the voxel of rank p is entry j = ceil(p m / n) iff j < m and
    floor(j n / m) == p, and is no entry otherwise -- over 3000 random (n, K), and at the ends of the ranges in Python integers"""
    rng = np.random.default_rng(5)
    for _ in range(3000):
        n, K = int(rng.integers(1, 6000)), int(rng.integers(1, 5000))
        m = min(n, K)
        ranks = (np.arange(m, dtype=np.int64) * n) // m                         # the statement: entry j holds rank floor(j n / m)
        p = np.arange(n, dtype=np.int64)
        j = (p * m + n - 1) // n
        is_entry = (j < m) & ((np.minimum(j, m - 1) * n) // m == p)
        assert np.array_equal(p[is_entry], ranks) and np.array_equal(j[is_entry], np.arange(m))
    n, m = 2 ** 31 - 1, 65536
    for j in (0, 1, 2, 12345, m - 2, m - 1):
        p = (j * n) // m
        assert (p * m + n - 1) // n == j and (p + 1) * m < 2 ** 63
        for q in (p - 1, p + 1):                                                # its neighbours in rank are no entries
            jq = (q * m + n - 1) // n
            assert q < 0 or jq >= m or (jq * n) // m != q


# --------------------------------------------------------------------------------------------------------------------- the draw
@functools.lru_cache(maxsize=None)
def _block_label(shape, corner):
    lab = np.zeros(shape, dtype=np.uint8)
    lab[tuple(slice(c, c + 2) for c in corner)] = 2
    lab.setflags(write=False)
    return lab


def test_draw_params_is_unchanged_with_oversampling_off(monkeypatch):
    full, crop = (40, 36, 31), (16, 16, 16)
    fg = ref.class_locations(_block_label(full, (1, 1, 1)), ref.FOREGROUND_CLASSES, 64)
    triples = [(1000 + 7 * k, k % 5, 3 * k + 1) for k in range(50)]
    moved = 0
    for seed, epoch, index in triples:
        today = data.draw_params(seed, epoch, index, full, crop, **AUG)
        rng = np.random.default_rng([seed, epoch, index])
        assert today.origin == data.random_crop_origin(full, crop, rng)        # still the origin NpzBraTS / SyntheticBraTS pick
        on = data.draw_params(seed, epoch, index, full, crop, oversample=1.0, foreground=fg, **AUG)
        assert on.at_origin(today.origin) == today                              # every field but the origin
        moved += on.origin != today.origin
    assert moved >= 45
    monkeypatch.setattr(data, "foreground_origin", None)                        # with it off, nothing new is called
    for seed, epoch, index in triples:
        today = data.draw_params(seed, epoch, index, full, crop, **AUG)
        assert data.draw_params(seed, epoch, index, full, crop, oversample=0.0, foreground=None, **AUG) == today
        assert data.draw_params(seed, epoch, index, full, crop, oversample=0, foreground=fg, **AUG) == today


@pytest.mark.parametrize("full,crop,corner", [((40, 36, 31), (16, 16, 16), (1, 1, 1)),        # clamped at 0
                                              ((40, 36, 31), (16, 16, 16), (38, 34, 29)),     # clamped at S - crop
                                              ((40, 36, 31), (16, 16, 16), (20, 17, 14)),     # not clamped
                                              ((40, 36, 31), (16, 16, 40), (1, 1, 1)),        # S_2 < crop_2
                                              ((40, 36, 31), (16, 16, 40), (38, 34, 29))])
def test_the_chosen_voxel_lies_inside_the_crop(full, crop, corner):
    """a 2 x 2 x 2 block is the only foreground.  For scale: a uniform 16^3 crop of the 40 x 36 x 31 volume has 25 x 21 x 16 = 8400
    origins, and 8 of them hold the block at (1,1,1): under 1e-3."""
    lab = _block_label(full, corner)
    counts, table = data.class_locations(torch.from_numpy(lab.copy()), ref.FOREGROUND_CLASSES, 4096)
    assert counts.tolist() == [0, 8, 0]
    images, labels, params, voxels = [], [], [], []
    img = torch.zeros((4,) + full)
    for index in range(200):
        origin, r, v = data.foreground_origin(5, 2, index, full, crop, counts.numpy(), table.numpy(), 1.0)
        assert (origin, r, v) == ref.foreground_origin(5, 2, index, full, crop, counts.numpy(), table.numpy(), 1.0)
        assert r == 1 and lab[v] == 2
        p = data.draw_params(5, 2, index, full, crop, oversample=1.0, foreground=(counts.numpy(), table.numpy()))
        assert p.origin == origin
        for d in range(3):
            assert 0 <= origin[d] <= max(full[d] - crop[d], 0) and origin[d] <= v[d] < origin[d] + crop[d]
        images.append(img); labels.append(torch.from_numpy(lab.copy())); params.append(p); voxels.append(v)
    assert len(set(voxels)) == 8                                                # every voxel of the block is drawn
    _, target, _ = data.prepare_batch(images, labels, params, crop)
    for b, (p, v) in enumerate(zip(params, voxels)):
        assert int(target[b][tuple(vd - od for vd, od in zip(v, p.origin))]) in ref.region_classes(ref.FOREGROUND_CLASSES[1])


def test_frequencies_of_the_draw():
    full, crop, N, p = (24, 20, 17), (8, 8, 8), 2000, 0.33
    lab = syn.synthetic_volume(1, full)[1].numpy().astype(np.uint8)
    masks = (0b0010, 0b0000, 0b0100, 0b1000)                                    # region 1 holds no class: empty
    counts, table = ref.class_locations(lab, masks, 16)
    assert counts[1] == 0 and all(counts[r] > 16 for r in (0, 2, 3)), counts
    picks = [data.foreground_origin(9, 0, i, full, crop, counts, table, p) for i in range(N)]
    hit = [q for q in picks if q[0] is not None]
    bound = 5.0 * np.sqrt(N * p * (1.0 - p))
    assert abs(len(hit) - N * p) <= bound, (len(hit), N * p, bound)
    bound = 5.0 * np.sqrt(len(hit) * (1.0 / 3.0) * (2.0 / 3.0))
    for r in (0, 2, 3):
        n_r = sum(1 for q in hit if q[1] == r)
        assert abs(n_r - len(hit) / 3.0) <= bound, (r, n_r, len(hit), bound)
    assert not any(q[1] == 1 for q in hit)
    for q in hit:                                                               # the voxel is one of the region's
        assert (int(masks[q[1]]) >> int(lab[q[2]])) & 1
    counts0, table0 = ref.class_locations(np.zeros(full, dtype=np.uint8), masks, 16)
    assert all(data.foreground_origin(9, 0, i, full, crop, counts0, table0, 1.0) == (None, None, None) for i in range(N))
    p0 = data.draw_params(9, 0, 3, full, crop)
    assert data.draw_params(9, 0, 3, full, crop, oversample=1.0, foreground=(counts0, table0)) == p0


# -------------------------------------------------------------------------------------------------------------------- the modes
@functools.lru_cache(maxsize=None)
def _subjects():
    out = []
    for i in range(3):
        x, t = syn.synthetic_volume(i, (40, 36, 31), 1234)
        out.append((x, t.to(torch.uint8)))
    return out


@pytest.mark.parametrize("aug", [{}, {"rotate": 15.0, "elastic": 2.0}])
def test_cached_and_staged_modes_agree_on_the_host(aug):
    crop, order = (16, 20, 24), [[2, 0], [1]]
    cached = data.DeviceBraTS(_subjects(), "cpu", crop, seed=77, cache=True, oversample=0.5, **aug)
    staged = data.DeviceBraTS(_subjects(), "cpu", crop, seed=77, cache=False, oversample=0.5, **aug)
    plain = data.DeviceBraTS(_subjects(), "cpu", crop, seed=77, cache=True, **aug)
    assert plain.foreground is None and len(cached.foreground) == 3
    for i, (x, t) in enumerate(_subjects()):
        want = ref.class_locations(t.numpy(), ref.FOREGROUND_CLASSES, 4096)
        for ds in (cached, staged):
            assert np.array_equal(ds.foreground[i][0], want[0]) and np.array_equal(ds.foreground[i][1], want[1])
    moved = 0
    for epoch in (0, 1):
        for ds in (cached, staged, plain):
            ds.set_epoch(epoch)
        moved += sum(cached.params(i).origin != plain.params(i).origin for i in range(3))
        assert all(cached.params(i) == staged.params(i) for i in range(3))
        want = list(cached.batches(order))
        for workers in (0, 2):
            got = list(staged.batches(order, num_workers=workers))
            assert len(got) == len(want)
            for a, b in zip(got, want):
                assert all(u.dtype == v.dtype and torch.equal(u, v) for u, v in zip(a, b)), (epoch, workers)
    assert moved >= 1                                                           # the oversampled origins are in those batches


# ------------------------------------------------------------------------------------------------------------------- refusals
def test_refusals():
    full, crop = (24, 20, 17), (8, 8, 8)
    lab = syn.synthetic_volume(0, full)[1].to(torch.uint8)
    fg = tuple(t.numpy() for t in data.class_locations(lab))
    for bad in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="oversample"):
            data.draw_params(1, 0, 0, full, crop, oversample=bad, foreground=fg)
        with pytest.raises(ValueError, match="oversample"):
            data.DeviceBraTS([(torch.zeros((4,) + full), lab)], "cpu", crop, oversample=bad)
        with pytest.raises(ValueError, match="oversample"):
            data.NpzCropSource([(torch.zeros((4,) + full), lab)], crop, oversample=bad, foreground=[fg])
    with pytest.raises(ValueError, match="foreground"):
        data.draw_params(1, 0, 0, full, crop, oversample=0.33)
    with pytest.raises(ValueError, match="foreground"):
        data.NpzCropSource([(torch.zeros((4,) + full), lab)], crop, oversample=0.33)
    for K in (0, -1, 65537):
        with pytest.raises(ValueError, match="table length"):
            data.class_locations(lab, samples=K)
        with pytest.raises(ValueError, match="table length"):
            data.DeviceBraTS([(torch.zeros((4,) + full), lab)], "cpu", crop, oversample=0.33, foreground_samples=K)
    for masks in ((), (1,) * 9):
        with pytest.raises(ValueError, match="regions"):
            data.class_locations(lab, masks)
    for masks in ((0b10000,), (0b0010, 0b100000), (-1,)):
        with pytest.raises(ValueError, match="classes 0..3"):
            data.class_locations(lab, masks)
        with pytest.raises(ValueError, match="classes 0..3"):
            data.DeviceBraTS([(torch.zeros((4,) + full), lab)], "cpu", crop, oversample=0.33, foreground_regions=masks)
    with pytest.raises(ValueError, match="uint8"):
        data.class_locations(lab.to(torch.int64))
    assert data.class_locations(lab, (0b1000,), 65536)[1].shape == (1, 65536)   # the ends of both ranges are accepted
    assert data.class_locations(lab, ref.EIGHT, 1)[1].shape == (8, 1)


def test_train_flags():
    import train_no_amp as T
    a = T.build_parser().parse_args([])
    assert (a.oversample_foreground, a.foreground_samples) == (0.0, 4096)
    T.check_foreground(a)
    with pytest.raises(SystemExit, match="device_data"):
        T.main(["--synthetic", "1", "--oversample_foreground", "0.33"])
    with pytest.raises(SystemExit, match="device_data"):
        T.main(["--synthetic", "1", "--device_data", "off", "--oversample_foreground", "0.33"])
    for bad in ("-0.1", "1.5", "nan"):
        with pytest.raises(SystemExit, match="--oversample_foreground takes"):
            T.main(["--synthetic", "1", "--device_data", "cache", "--oversample_foreground", bad])
    for bad in ("0", "65537"):
        with pytest.raises(SystemExit, match="--foreground_samples takes"):
            T.main(["--synthetic", "1", "--device_data", "staged", "--oversample_foreground", "0.33", "--foreground_samples", bad])
    for mode in ("cache", "staged"):
        c = T.build_parser().parse_args(["--synthetic", "2", "--device_data", mode, "--oversample_foreground", "1", "--foreground_samples", "50",
                                         "--input_H", "20", "--input_W", "18", "--output_D", "16", "--crop_H", "8", "--crop_W", "8", "--crop_D", "8"])
        T.check_foreground(c)
        ds = T.make_device_dataset(c, "cpu")
        assert ds.oversample == 1.0 and ds.foreground[0][1].shape == (3, 50)
        x, target, edge, missing = ds.batch([0, 1])
        assert x.shape == (2, 4, 8, 8, 8) and all(bool((target[b] > 0).any()) for b in range(2))
