"""The float64 Hausdorff restatement (tests/hausdorff_ref.py) against scipy, hand-computed cases, and the host-side rules of the
drop-ins (utils/hausdorff.py, tools.softmax_hd_dice) that hold without a GPU."""
import math

import numpy as np
import pytest

import hausdorff_ref as H

SPACINGS = [None, 0.8, (0.9375, 0.9375, 1.5)]


def _scipy_hd_hd95(a, b, spacing, connectivity):
    """medpy's definition in scipy's own terms (binary_erosion + distance_transform_edt)."""
    nd = pytest.importorskip("scipy.ndimage")
    a, b = np.asarray(a, bool), np.asarray(b, bool)
    fp = nd.generate_binary_structure(a.ndim, connectivity)
    sp = None if spacing is None else ([spacing] * a.ndim if np.isscalar(spacing) else list(spacing))

    def sd(x, y):
        bx = x ^ nd.binary_erosion(x, structure=fp, iterations=1)
        by = y ^ nd.binary_erosion(y, structure=fp, iterations=1)
        return nd.distance_transform_edt(~by, sampling=sp)[bx]

    d1, d2 = sd(a, b), sd(b, a)
    return max(d1.max(), d2.max()), np.percentile(np.hstack((d1, d2)), 95)


def _cases():
    rng = np.random.default_rng(7)
    shp = (23, 31, 17)
    yield "blobs", H.blobs(shp, 3, rng), H.blobs(shp, 4, rng)
    face = np.zeros(shp, bool)
    face[0:5, :, 3:9] = True
    yield "face", face, H.blobs(shp, 2, rng, 3, 8)
    yield "shells", H.shell(shp, (11, 15, 8), 7, 5), H.shell(shp, (12, 14, 9), 6, 4.5)
    thin = np.zeros(shp, bool)
    thin[10, 3:28, 2:15] = True
    yield "sheet", thin, H.blobs(shp, 1, rng, 4, 6)


@pytest.mark.parametrize("connectivity", [1, 2, 3])
@pytest.mark.parametrize("spacing", SPACINGS, ids=["unit", "scalar", "aniso"])
def test_restatement_matches_scipy(connectivity, spacing):
    for name, a, b in _cases():
        ref = _scipy_hd_hd95(a, b, spacing, connectivity)
        got = H.hd_hd95(a, b, spacing, connectivity)
        if spacing is None:
            assert got == (ref[0], ref[1]), (name, got, ref)
        else:
            np.testing.assert_allclose(got, ref, rtol=1e-12, err_msg=name)
        assert H.hd_hd95(a, b, spacing, connectivity, use_scipy=True) == pytest.approx(got, rel=1e-12)


def test_borders_match_scipy_erosion():
    nd = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(3)
    m = H.blobs((14, 12, 10), 4, rng)
    m[:, 0, :] |= rng.random((14, 10)) < 0.5
    for c in (1, 2, 3):
        fp = nd.generate_binary_structure(3, c)
        assert np.array_equal(H.border(m, c), m ^ nd.binary_erosion(m, structure=fp, iterations=1))


def test_rank4_singleton_axis_makes_every_voxel_a_border_voxel():
    nd = pytest.importorskip("scipy.ndimage")
    cube = np.zeros((1, 9, 9, 9), bool)
    cube[0, 1:8, 1:8, 1:8] = True
    assert nd.binary_erosion(cube, structure=nd.generate_binary_structure(4, 1)).sum() == 0
    assert np.array_equal(H.border(cube), cube)
    assert H.border(cube[0]).sum() == 7 ** 3 - 5 ** 3
    rng = np.random.default_rng(11)
    a, b = H.blobs((15, 13, 11), 2, rng)[None], H.blobs((15, 13, 11), 2, rng)[None]
    for c in (1, 3):
        for sp in (None, (1.0, 0.9375, 0.9375, 1.5)):
            ref = _scipy_hd_hd95(a, b, sp, c)
            np.testing.assert_allclose(H.hd_hd95(a, b, sp, c), ref, rtol=1e-12)


def test_hand_computed_single_voxels():
    a = np.zeros((8, 8, 8), bool); b = np.zeros((8, 8, 8), bool)
    a[1, 1, 2] = True; b[4, 5, 2] = True
    assert H.hd_hd95(a, b) == (5.0, 5.0)
    a = np.zeros((8, 8, 8), bool); b = np.zeros((8, 8, 8), bool)
    a[2, 2, 1] = True; b[2, 2, 4] = True
    assert H.hd_hd95(a, b, (1, 1, 2)) == (6.0, 6.0)


def test_hd95_interpolation_upper_branch():
    # border(A) = {z=0, z=4}, border(B) = {z=1}: sd(A,B) = [1, 3], sd(B,A) = [1] -> sorted [1, 1, 3]; v = 2 * 0.95 -> g = 0.9 >= 0.5
    a = np.zeros((1, 1, 6), bool); b = np.zeros((1, 1, 6), bool)
    a[0, 0, [0, 4]] = True; b[0, 0, 1] = True
    v = (3 - 1) * 0.95
    g = v - math.floor(v)
    assert g >= 0.5
    expect = 3.0 - (3.0 - 1.0) * (1 - g)
    assert H.hd_hd95(a, b) == (3.0, expect)


def test_dropin_empty_and_full_rules_without_gpu():
    from utils import hausdorff as HD
    z = np.zeros((6, 7, 8), bool)
    m = z.copy(); m[2:4, 2:5, 1:3] = True
    full = np.ones_like(z)
    for f in (HD.hausdorff_distance, HD.hausdorff_distance_95):
        assert f(z, m) == 0 and f(m, z) == 0 and f(full, m) == 0 and f(m, full) == 0
        assert math.isnan(f(z, m, nan_for_nonexisting=True)) and math.isnan(f(m, full, nan_for_nonexisting=True))
        assert f(z[None], m[None]) == 0                                      # rank 4 [1, ...] accepted
        with pytest.raises(ValueError):
            f(np.stack([m, m]), np.stack([m, m]))                            # a real batch axis
        with pytest.raises(ValueError):
            f(m[0], m[0])                                                   # rank 2
    cm = HD.ConfusionMatrix(m, full)
    assert cm.get_existence() == (False, False, False, True)
    assert cm.get_matrix() == (int(m.sum()), 0, 0, int((~m).sum()))
    assert cm.get_size() == m.size
    assert HD.hausdorff_distance_95(confusion_matrix=cm) == 0
    import torch
    assert HD.hausdorff_distance(torch.zeros(4, 5, 6), torch.ones(4, 5, 6)) == 0


def test_softmax_hd_dice_raises_on_empty_region_without_gpu():
    from utils import tools
    lab = np.zeros((10, 10, 10), np.int64)
    lab[2:6, 2:6, 2:6] = 2
    lab[3:5, 3:5, 3:5] = 1                                                  # no label 3: ET empty
    tgt = lab.copy(); tgt[4, 4, 4] = 3
    with pytest.raises(RuntimeError, match="first supplied array"):
        tools.softmax_hd_dice(lab, tgt)
    with pytest.raises(RuntimeError, match="second supplied array"):
        tools.softmax_hd_dice(tgt, lab)
    with pytest.raises(ValueError):
        tools.softmax_hd_dice(np.stack([lab, lab]), np.stack([tgt, tgt]))
