"""Elastically deformed crops on the CPU: the vectorised float32 statement of utils.data (through prepare_batch) against the scalar
restatement of tests/elastic_prep_ref.py, bit for bit; the zero grid; the float64 and linear-precision bounds on the displacement;
source_box and the staged mode; draw_params, AugParams and the train_no_amp flags.

The bound on the displacement, derived and not tuned: |D32 - D64| <= 64 * 2^-24 * max |disp|.  D is three nested 4-term sums of
products with weights in [0, 1] that sum to 1, so every partial result is bounded by max |disp| (up to the same roundings): a sum of
four products costs at most 4 roundings of such a value (the four products share one rounding's worth, the weights summing to 1, and
three additions), three levels 12, and a weight carries at most 8 roundings of its own (w1 and w2: six operations and the factor 1/6
rounded, on intermediates up to 6 times the result), one weight per level: 24 more.  About 36 * 2^-24 * max |disp|; 64 leaves slack.
The float64 side evaluates the same spline at the same float32 grid positions g_d, which are part of the definition."""
import logging

import numpy as np
import pytest
import torch

import elastic_prep_ref as E

FLIPS = [(a, b, c) for a in (False, True) for b in (False, True) for c in (False, True)]
MATRIX = (0.93, -0.21, 0.08, 0.17, 1.04, -0.12, -0.05, 0.16, 0.88)
BOUND = 64.0 * 2.0 ** -24


def _src(shape, seed):
    rng = np.random.default_rng(seed)
    return torch.from_numpy(E.random_image(shape, rng)), torch.from_numpy(E.blob_labels(shape, rng))


@pytest.mark.parametrize("crop", [(4, 6, 8), (5, 7, 9)])
@pytest.mark.parametrize("grid", [(4, 4, 4), (4, 5, 8)])
def test_equals_the_scalar_restatement(crop, grid):
    """all eight flips; the four combinations of matrix and intensity on / off each meet every flip parity over the two crops and grids"""
    from utils import data
    rng = np.random.default_rng(crop[0] * 10 + grid[2])
    img, lab = _src((9, 10, 12), crop[2])
    seen = set()
    for k, flip in enumerate(FLIPS):
        for combo in (k % 4, (k + 1 + crop[0] + grid[1]) % 4):
            with_m, with_i = bool(combo & 1), bool(combo & 2)
            seen.add((with_m, with_i))
            disp = E.random_grid(grid, 2.5, rng)
            origin = tuple(int(v) for v in rng.integers(-2, 4, 3))
            sc, sh = (rng.uniform(0.5, 1.5, 4), rng.uniform(-2, 2, 4)) if with_i else (None, None)
            p = data.AugParams(origin, flip, sc, sh, MATRIX if with_m else None, disp)
            x, t, e = data.prepare_batch([img], [lab], [p], crop)
            rx, rt, re = E.prepare_one(img.numpy(), lab.numpy(), p.origin, p.flip, p.scale, p.shift, p.matrix, disp, crop)
            assert np.array_equal(x[0].numpy().view(np.int32), rx.view(np.int32)), (flip, with_m, with_i)
            assert np.array_equal(t[0].numpy(), rt) and np.array_equal(e[0].numpy(), re)
            assert t.dtype == torch.int64 and e.dtype == torch.int64 and x.dtype == torch.float32
    assert len(seen) == 4


def test_zero_grid_adds_nothing():
    from utils import data
    img, lab = _src((14, 16, 18), 1)
    crop = (8, 10, 12)
    zero = np.zeros((3, 5, 4, 7), dtype=np.float32)
    for flip in FLIPS:
        sc, sh = ((0.9, 1.1, 1.0, 1.2), (0.1, -0.2, 0.0, 0.3)) if flip[1] else (None, None)
        for m in (None, MATRIX):                           # without a matrix `want` is the plain crop: crop_pad, then torch.flip
            want = data.prepare_batch([img], [lab], [data.AugParams((2, 3, 1), flip, sc, sh, m)], crop)
            got = data.prepare_batch([img], [lab], [data.AugParams((2, 3, 1), flip, sc, sh, m, zero)], crop)
            assert all(np.array_equal(g.numpy(), w.numpy()) for g, w in zip(got, want))


@pytest.mark.parametrize("crop,grid", [((128, 128, 128), (7, 7, 7)), ((33, 47, 70), (4, 5, 8)), ((9, 1, 20), (8, 4, 6))])
def test_displacement_float64_bound(crop, grid):
    from utils import data
    rng = np.random.default_rng(grid[0])
    for flip, amp in (((False, False, False), 6.0), ((True, False, True), 30.0)):
        disp = E.random_grid(grid, amp, rng)
        D32 = data._elastic_disp(data.AugParams((0, 0, 0), flip, disp=disp), crop)
        D64, _ = E.displacement64(disp, flip, crop)
        worst = max(float(np.abs(D32[c].astype(np.float64) - D64[c]).max()) for c in range(3)) / float(np.abs(disp).max())
        print("crop %r grid %r: worst |D32 - D64| / max |disp| = %.2f * 2^-24" % (crop, grid, worst * 2.0 ** 24))
        assert worst <= BOUND
        assert all(D32[c].dtype == np.float32 and D32[c].shape == crop for c in range(3))
        assert max(float(np.abs(D32[c]).max()) for c in range(3)) <= float(np.abs(disp).max()) * (1 + BOUND)   # source_box's premise


def test_linear_precision():
    """control values a + b . (grid index) are reproduced: sum_j w_j (i - 1 + j) = i + t = g"""
    from utils import data
    crop, grid = (40, 33, 52), (6, 8, 5)
    idx = np.meshgrid(*[np.arange(g, dtype=np.float64) for g in grid], indexing="ij")
    coef = [(1.5, (0.75, -0.5, 0.25)), (-3.0, (0.0, 1.25, -2.0)), (0.5, (-1.0, 0.5, 0.125))]
    disp = np.stack([a + sum(b[d] * idx[d] for d in range(3)) for a, b in coef]).astype(np.float32)      # exact in float32
    for flip in ((False, False, False), (True, True, False)):
        D32 = data._elastic_disp(data.AugParams((0, 0, 0), flip, disp=disp), crop)
        _, g = E.displacement64(disp, flip, crop)
        for c, (a, b) in enumerate(coef):
            want = a + b[0] * g[0][:, None, None] + b[1] * g[1][None, :, None] + b[2] * g[2][None, None, :]
            worst = float(np.abs(D32[c].astype(np.float64) - want).max()) / float(np.abs(disp).max())
            print("component %d: worst |D32 - linear| / max |disp| = %.2f * 2^-24" % (c, worst * 2.0 ** 24))
            assert worst <= BOUND


def test_source_box_contains_every_tap():
    from utils import data
    rng = np.random.default_rng(11)
    crop, full = (12, 10, 14), (30, 28, 33)
    widened = 0
    for n in range(300):
        g = int(rng.integers(4, 9))
        p = data.draw_params(7, n // 50, n, full, crop, flip=True, rotate=20.0, scale=0.2, elastic=6.0, elastic_grid=g)
        if n % 3 == 0:
            p = data.AugParams(p.origin, p.flip, matrix=p.matrix if n % 2 else None,
                               disp=E.random_grid(tuple(int(v) for v in rng.integers(4, 9, 3)), 6.0, rng))
        assert p.disp is not None and p.disp.shape[0] == 3
        box = p.source_box(crop)
        q, ok = data._source_coords(p, crop)
        assert ok.all()
        affine_box = data.AugParams(p.origin, p.flip, matrix=p.matrix if p.matrix is not None else (1, 0, 0, 0, 1, 0, 0, 0, 1)).source_box(crop)
        for d in range(3):
            lo, hi = box[d]
            assert isinstance(lo, int) and isinstance(hi, int)
            i = np.floor(q[d]).astype(np.int64)
            nn = np.floor(q[d] + np.float32(0.5)).astype(np.int64)
            assert lo <= i.min() and i.max() + 1 < hi and lo <= nn.min() and nn.max() < hi, (n, d)
            widened += int(i.min() < affine_box[d][0] or i.max() + 1 >= affine_box[d][1])
    assert widened > 0                                     # the displacement does carry taps outside the affine box
    # non-finite and huge control values: the box stays a pair of ints, bounded by what a voxel can still read
    bad = np.zeros((3, 4, 4, 4), dtype=np.float32)
    bad[0, 1, 1, 1], bad[1, 0, 0, 0], bad[2, 3, 3, 3] = np.nan, np.inf, 3e38
    box = data.AugParams((0, 0, 0), disp=bad).source_box(crop)
    assert all(isinstance(v, int) for b in box for v in b) and box[0] == (-2, crop[0] + 3) and box[2][0] < -2 ** 30


def test_staged_equals_cache_cpu():
    from utils import data
    shapes = [(40, 44, 36), (30, 52, 41), (36, 36, 36)]
    subjects = [_src(S, 20 + k) for k, S in enumerate(shapes)]
    crop = (24, 28, 20)
    for kw in (dict(seed=5, flip=True, intensity=0.2, rotate=15.0, scale=0.2, elastic=6.0, elastic_grid=5),
               dict(seed=6, flip=True, elastic=4.0)):
        cache = data.DeviceBraTS(subjects, "cpu", crop, **kw)
        staged = data.DeviceBraTS(subjects, "cpu", crop, cache=False, **kw)
        for epoch in (0, 3):
            cache.set_epoch(epoch); staged.set_epoch(epoch)
            g = kw.get("elastic_grid", 7)
            assert all(cache.params(i).disp.shape == (3, g, g, g) for i in range(3))
            items = [staged.source[i] for i in range(3)]
            assert all(it[0].numel() < 4 * np.prod(S) for it, S in zip(items, shapes))
            want = cache.batch([2, 0, 1])
            for got in (staged.batch([2, 0, 1]), next(iter(staged.batches([[2, 0, 1]])))):
                assert all(torch.equal(a, b) for a, b in zip(got, want))
                assert torch.equal(got[0].view(torch.int32), want[0].view(torch.int32))
        params = [cache.params(i) for i in (2, 0, 1)]
        ref = data.prepare_batch([subjects[i][0] for i in (2, 0, 1)], [subjects[i][1] for i in (2, 0, 1)], params, crop)
        assert all(torch.equal(a, b) for a, b in zip(ref, want))
        assert int((want[1] > 0).sum()) > 0


def test_draw_params_stability():
    from utils import data
    full, crop = (240, 240, 155), (128, 128, 128)
    for seed, epoch, index in ((1000, 0, 0), (1000, 4, 17), (3, 0, 17), (3, 2, 5)):
        for kw in (dict(), dict(flip=True, intensity=0.2), dict(rotate=15.0), dict(flip=True, intensity=0.1, rotate=10.0, scale=0.2)):
            off = data.draw_params(seed, epoch, index, full, crop, **kw)
            assert off.disp is None and off == data.draw_params(seed, epoch, index, full, crop, elastic=0.0, elastic_grid=5, **kw)
            on = data.draw_params(seed, epoch, index, full, crop, elastic=4.0, **kw)
            assert (on.origin, on.flip, on.scale, on.shift, on.matrix) == (off.origin, off.flip, off.scale, off.shift, off.matrix)
            assert on.disp.dtype == np.float32 and on.disp.shape == (3, 7, 7, 7) and on != off
            assert 2.0 < float(np.abs(on.disp).max()) <= 4.0
            again = data.draw_params(seed, epoch, index, full, crop, elastic=4.0, **kw)
            assert again == on and np.array_equal(again.disp, on.disp)
            g5 = data.draw_params(seed, epoch, index, full, crop, elastic=4.0, elastic_grid=5, **kw)
            assert g5.disp.shape == (3, 5, 5, 5) and g5 != on
    assert data.draw_params(1, 2, 3, full, crop, elastic=4.0) != data.draw_params(1, 2, 4, full, crop, elastic=4.0)
    # the stream position: the grid is drawn after the matrix's angles and zoom
    rng = np.random.default_rng([1, 2, 3])
    for f, c in zip(full, crop):
        rng.integers(0, max(f - c, 0) + 1)
    rng.uniform(-15.0, 15.0, 3); rng.uniform(0.8, 1.2)
    want = rng.uniform(-4.0, 4.0, (3, 6, 6, 6)).astype(np.float32)
    assert np.array_equal(data.draw_params(1, 2, 3, full, crop, rotate=15.0, scale=0.2, elastic=4.0, elastic_grid=6).disp, want)
    with pytest.raises(ValueError):
        data.draw_params(1, 2, 3, full, crop, elastic=4.0, elastic_grid=9)


def test_aug_params_disp_slot():
    from utils import data
    p = data.AugParams((1, 2, 3), (True, False, True))
    assert p.disp is None and repr(p) == "AugParams(origin=(1, 2, 3), flip=(True, False, True), scale=None, shift=None)"
    grid = E.random_grid((4, 5, 8), 3.0, np.random.default_rng(0))
    q = data.AugParams((1, 2, 3), (True, False, True), disp=grid.astype(np.float64).tolist())
    assert q.disp.dtype == np.float32 and q.disp.shape == (3, 4, 5, 8) and np.array_equal(q.disp, grid)
    assert q != p and p != q and q == data.AugParams((1, 2, 3), (True, False, True), disp=grid)
    other = grid.copy()
    other[2, 3, 4, 7] += 1.0
    assert q != data.AugParams((1, 2, 3), (True, False, True), disp=other)
    assert q != data.AugParams((1, 2, 3), (True, False, True), disp=grid.transpose(0, 1, 3, 2)[:, :, :5, :5])
    assert "disp=" in repr(q) and "disp=" not in repr(p) and "matrix=" not in repr(q)
    m = data.AugParams((0, 0, 0), matrix=MATRIX, disp=grid)
    assert "matrix=" in repr(m) and "disp=" in repr(m)
    moved = q.at_origin((-4, 0, 9))
    assert moved.origin == (-4, 0, 9) and np.array_equal(moved.disp, grid) and moved.flip == q.flip
    grid[0, 0, 0, 0] = 99.0                                # the parameters keep their own copy
    assert q.disp[0, 0, 0, 0] != 99.0
    with pytest.raises(ValueError):
        q.disp[0, 0, 0, 0] = 1.0
    nan = np.full((3, 4, 4, 4), np.nan, dtype=np.float32)
    assert data.AugParams((0, 0, 0), disp=nan) == data.AugParams((0, 0, 0), disp=nan)
    for shape in ((3, 3, 4, 4), (3, 4, 9, 4), (3, 4, 4), (2, 4, 4, 4), (3, 4, 4, 4, 1), (4, 4, 4)):
        with pytest.raises(ValueError):
            data.AugParams((0, 0, 0), disp=np.zeros(shape, dtype=np.float32))


def test_non_finite_control_values_read_nothing():
    from utils import data
    img, lab = _src((12, 12, 12), 3)
    crop = (8, 8, 8)
    disp = np.zeros((3, 4, 4, 4), dtype=np.float32)
    disp[:, 0, 0, 0] = np.nan, np.inf, -np.inf
    disp[1, 3, 3, 3] = 3e38
    p = data.AugParams((2, 2, 2), scale=(2, 2, 2, 2), shift=(1, 2, 3, 4), disp=disp)
    x, t, e = data.prepare_batch([img], [lab], [p], crop)
    assert not bool(torch.isnan(x).any())
    assert torch.equal(x[0, :, 0, 0, 0], torch.tensor([1.0, 2.0, 3.0, 4.0])) and int(t[0, 0, 0, 0]) == 0
    assert torch.equal(x[0, :, 7, 7, 7], torch.tensor([1.0, 2.0, 3.0, 4.0])) and int(t[0, 7, 7, 7]) == 0
    rx, rt, re = E.prepare_one(img.numpy(), lab.numpy(), p.origin, p.flip, p.scale, p.shift, None, disp, crop)
    assert np.array_equal(x[0].numpy().view(np.int32), rx.view(np.int32)) and np.array_equal(t[0].numpy(), rt)
    assert np.array_equal(e[0].numpy(), re)
    assert int((t[0] > 0).sum()) > 0                       # the voxels no bad control point reaches are the plain crop's


def test_train_flags():
    import train_no_amp as T
    a = T.build_parser().parse_args([])
    assert a.aug_elastic == 0.0 and a.aug_elastic_grid == 7
    b = T.build_parser().parse_args(["--device_data", "cache", "--aug_elastic", "4", "--aug_elastic_grid", "5"])
    assert b.aug_elastic == 4.0 and b.aug_elastic_grid == 5
    with pytest.raises(SystemExit, match="device_data"):
        T.main(["--synthetic", "1", "--aug_elastic", "4"])
    with pytest.raises(SystemExit, match="aug_elastic_grid"):
        T.main(["--synthetic", "1", "--device_data", "cache", "--aug_elastic", "4", "--aug_elastic_grid", "9"])


@pytest.fixture()
def fresh_train_log():
    """train_no_amp attaches its log handlers once per process: drop the ones this test adds, so a later run logs to its own files"""
    log = logging.getLogger("cwf.train")
    before = list(log.handlers)
    yield
    for h in list(log.handlers):
        if h not in before:
            log.removeHandler(h)
            h.close()


def test_train_harness_elastic_cpu(emul_backend, fresh_train_log, tmp_path):
    """--no_cuda --synthetic 2 --device_data cache --aug_elastic 4 --max_iters 2 (on 64^3 crops): runs and writes its checkpoint"""
    import train_no_amp as T
    rc = T.main(["--no_cuda", "true", "--synthetic", "2", "--device_data", "cache", "--aug_elastic", "4", "--max_iters", "2",
                 "--input_H", "72", "--input_W", "70", "--output_D", "66", "--crop_H", "64", "--crop_W", "64", "--crop_D", "64",
                 "--end_epoch", "1", "--project_root", str(tmp_path), "--experiment", "t", "--date", "d"])
    assert rc == 0
    ck = torch.load(tmp_path / "checkpoint" / "td" / "model_epoch_last.pth", weights_only=True)
    assert all(bool(torch.isfinite(v).all()) for v in ck["state_dict"].values() if v.is_floating_point())
