"""Sliding-window inference on the CPU: the window grid and importance map of predict_overlap, the float64 reference of
tests/sliding_window_ref.py (its two forms agree, a pointwise model comes back unchanged) and defects planted in a blend that the
reference's bound catches by a wide margin."""
import itertools

import numpy as np
import pytest

import predict_overlap as po
import sliding_window_ref as R


# ------------------------------------------------------------------ grid
def test_grid_brats_volume_overlap_half():
    starts = po.window_grid((240, 240, 155), (128, 128, 128), 0.5)
    assert starts == ([0, 56, 112], [0, 56, 112], [0, 27])
    assert len(po.windows(starts)) == 18
    assert po.windows(starts)[:3] == [(0, 0, 0), (0, 0, 27), (0, 56, 0)]          # lexicographic, axis 0 slowest


@pytest.mark.parametrize("shape", [(240, 240, 155), (137, 181, 96), (131, 181, 97), (300, 129, 128)])
@pytest.mark.parametrize("roi", [(128, 128, 128), (160, 192, 160), (16, 24, 32)])
@pytest.mark.parametrize("overlap", [0.0, 0.25, 0.5, 0.75])
def test_grid_covers_and_ends_at_the_far_face(shape, roi, overlap):
    starts = po.window_grid(shape, roi, overlap)
    for s, r, st in zip(shape, roi, starts):
        assert st[0] == 0
        assert st == sorted(st)
        if s <= r:
            assert st == [0]
        else:
            assert st[-1] == s - r
            assert max(b - a for a, b in zip(st, st[1:] or [st[0] + r])) <= r
    # coverage along each axis implies coverage of the Cartesian product
    for s, r, st in zip(shape, roi, starts):
        cov = np.zeros(s, int)
        for a in st:
            cov[a:a + r] += 1
        assert cov.min() >= 1


def test_grid_overlap_zero_two_disjoint_windows():
    starts = po.window_grid((64, 96, 256), (32, 96, 128), 0.0)
    assert starts == ([0, 32], [0], [0, 128])


def test_grid_short_axis_one_padded_window():
    starts = po.window_grid((100, 240, 120), (128, 128, 128), 0.5)
    assert starts[0] == [0] and starts[2] == [0] and starts[1] == [0, 56, 112]


@pytest.mark.parametrize("args", [((240, 240, 155), (128, 128), 0.5), ((240, 240, 155), (128, 0, 128), 0.5),
                                  ((240, 240, 155), (128, 128, 128), 1.0), ((240, 240, 155), (128, 128, 128), -0.1),
                                  ((0, 240, 155), (128, 128, 128), 0.5)])
def test_grid_rejects_bad_arguments(args):
    with pytest.raises(ValueError):
        po.window_grid(*args)


@pytest.mark.parametrize("roi", [(120, 128, 128), (48, 64, 64), (128, 128)])
def test_model_roi_limits(roi):
    with pytest.raises(ValueError):
        po.check_roi(roi)
    assert po.check_roi((128, 128, 128)) == (128, 128, 128) and po.check_roi((160, 192, 160)) == (160, 192, 160)
    assert po.check_roi((64, 64, 64)) == (64, 64, 64)          # 4 * 4 * 8 = 128 tokens, the least the model takes


# ------------------------------------------------------------------ importance map
@pytest.mark.parametrize("roi", [(128, 128, 128), (160, 192, 160), (15, 8, 9)])
def test_gaussian_map_symmetric_central_separable(roi):
    m = po.importance_map(roi, "gaussian")
    g = po.importance_tables(roi, "gaussian")
    assert m.dtype == np.float32 and m.shape == roi
    for a in range(3):
        assert np.array_equal(m, np.flip(m, axis=a))
    c = tuple((r - 1) // 2 for r in roi)
    assert m[c] == m.max()
    assert (m > 0).all()
    # separable: fp32(fp32(g0 g1) g2), and within two fp32 roundings of the exact product
    want = ((g[0][:, None] * g[1][None, :])[:, :, None] * g[2][None, None, :]).astype(np.float32)
    assert np.array_equal(m, want)
    assert np.abs(m / R.weights3(g) - 1).max() <= 2 * R.U
    # each table: float64 Gaussian rounded once
    t = np.arange(roi[0]) - (roi[0] - 1) / 2
    assert np.array_equal(g[0], np.exp(-t * t / (2 * (0.125 * roi[0]) ** 2)).astype(np.float32))


def test_constant_map_all_ones_and_bad_modes():
    assert (po.importance_map((16, 32, 48), "constant") == 1).all()
    with pytest.raises(ValueError):
        po.importance_map((16, 16, 16), "triangle")
    with pytest.raises(ValueError):
        po.importance_map((128, 128, 128), "gaussian", sigma_scale=0.0)
    with pytest.raises(ValueError):
        po.importance_map((128, 128, 128), "gaussian", sigma_scale=0.005)         # edge weights underflow in fp32


# ------------------------------------------------------------------ reference
@pytest.mark.parametrize("blend", ["gaussian", "constant"])
@pytest.mark.parametrize("overlap", [0.0, 0.5, 0.75])
def test_reference_loop_and_voxel_forms_agree(blend, overlap):
    shape, roi = (9, 7, 6), (4, 4, 8)
    starts = po.window_grid(shape, roi, overlap)
    rng = np.random.default_rng(1)
    probs = rng.random((len(R.windows(starts)), 2, 4) + roi)
    tabs = po.importance_tables(roi, blend)
    a = R.blend(probs, starts, roi, shape, tabs)
    b = R.blend_voxel(probs, starts, roi, shape, tabs)
    assert np.abs(a - b).max() <= 1e-15


@pytest.mark.parametrize("overlap", [0.0, 0.25, 0.5, 0.75])
def test_reference_reproduces_a_pointwise_model(overlap):
    shape, roi = (37, 29, 13), (16, 12, 16)
    rng = np.random.default_rng(2)
    x = rng.standard_normal((2, 4) + shape)
    starts = po.window_grid(shape, roi, overlap)
    f = R.softmax4(x)
    got = R.blend(R.softmax4(R.gather(x, starts, roi).reshape((-1, 4) + roi)).reshape((-1, 2, 4) + roi), starts, roi, shape,
                  po.importance_tables(roi))
    k = R.max_coverage(shape, roi, starts)
    assert np.abs(got - f).max() <= (2 * k + 4) * 2.0 ** -53      # a weighted mean of equal values: float64 rounding only


def test_gamma_grows_with_coverage():
    assert R.gamma(1) < R.gamma(8) < R.gamma(18) < 1e-5
    assert R.max_coverage((240, 240, 155), (128,) * 3, po.window_grid((240, 240, 155), (128,) * 3, 0.5)) == 18


# ------------------------------------------------------------------ planted defects: each misses the bound by >= 30x
SHAPE, ROI = (40, 36, 30), (16, 16, 16)


def _setup(overlap=0.5):
    rng = np.random.default_rng(7)
    x = rng.standard_normal((1, 4) + SHAPE) * 3
    starts = po.window_grid(SHAPE, ROI, overlap)
    probs = R.softmax4(R.gather(x, starts, ROI).reshape((-1, 4) + ROI)).reshape((-1, 1, 4) + ROI)
    tabs = po.importance_tables(ROI)
    k = R.max_coverage(SHAPE, ROI, starts)
    return x, starts, probs, tabs, k, R.softmax4(x)


def test_correct_blend_passes():
    x, starts, probs, tabs, k, want = _setup()
    assert R.excess(R.blend(probs, starts, ROI, SHAPE, tabs), want, k) <= 1e-3


def test_defect_start_shifted_by_one_voxel():
    x, starts, probs, tabs, k, want = _setup()
    bad = [list(s) for s in starts]
    bad[1][1] += 1                                   # the window is cut at the right place but blended one voxel off
    assert R.excess(R.blend(probs, bad, ROI, SHAPE, tabs), want, k) >= 30


def test_defect_dropped_window():
    x, starts, probs, tabs, k, want = _setup()
    acc, wsum = R.blend_loop(probs, starts, ROI, SHAPE, tabs, skip=(5,))
    assert R.excess(R.finalize(acc, wsum), want, k) >= 30


def test_defect_swapped_axes():
    x, starts, probs, tabs, k, want = _setup()
    assert R.excess(R.blend(np.swapaxes(probs, 3, 4), starts, ROI, SHAPE, tabs), want, k) >= 30


def test_defect_reference_depth_shift():
    """tailor_and_concat's quirk: slices 128..154 carry the predictions for 123..149"""
    rng = np.random.default_rng(9)
    x = rng.standard_normal((1, 4, 8, 8, 155)) * 3
    want = R.softmax4(x)
    got = want.copy()
    got[..., 128:155] = want[..., 123:150]
    k = R.max_coverage((240, 240, 155), (128,) * 3, po.window_grid((240, 240, 155), (128,) * 3, 0.5))
    assert R.excess(got, want, k) >= 30
    assert R.excess(got[..., :128], want[..., :128], k) == 0


def test_excess_fails_on_nan():
    assert R.excess(np.array([np.nan]), np.array([0.5]), 1) == float("inf")


def test_windows_order_matches_itertools():
    starts = ([0, 5], [1], [2, 3, 4])
    assert po.windows(starts) == list(itertools.product(*starts)) == R.windows(starts)
