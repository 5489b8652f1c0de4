"""The restatement tests/surface_ref.py against hand-computed cases and scipy's distance transform, and the host paths of the surface
metrics: utils.hausdorff's asd / assd / NSD wrappers, predict_overlap.surface_regions and lesionwise_metrics(nsd_tolerances=...) on
CPU tensors."""
import math

import numpy as np
import pytest
import torch
from scipy import ndimage

import hausdorff_ref as H
import lesionwise_ref as LW
import surface_ref as S


# ------------------------------------------------------------------ hand-computed cases
def test_two_single_voxels():
    a = np.zeros((5, 6, 7), bool); b = np.zeros((5, 6, 7), bool)
    a[1, 1, 1] = True; b[1, 4, 5] = True                            # 3-4-5: d = 5 both ways
    r = S.surface(a, b, (4.999, 5.0, math.inf, 0.0))
    assert r["counts"] == (1, 1, 1, 1) and r["asd"] == (5.0, 5.0) and r["assd"] == 5.0
    assert r["within"] == [[0, 0], [1, 1], [1, 1], [0, 0]] and r["nsd"] == [0.0, 1.0, 1.0, 0.0]
    r = S.surface(a, b, (12.4, 12.5), spacing=(1, 1, 2.5))          # d = sqrt(3^2 + (4 * 2.5)^2) = 10.44...
    assert r["asd"][0] == math.sqrt(9.0 + 100.0) and r["within"] == [[1, 1], [1, 1]]


def test_concentric_cubes_every_distance_known():
    """A = the 7^3 cube [3, 10)^3, B = the 3^3 cube [5, 8)^3 inside a 13^3 volume.  dB is B minus its centre voxel, 26 voxels; dA is the
    7^3 shell, 343 - 125 = 218 voxels.  From dB to dA: every voxel of dB has a coordinate equal to 5 or 7, two steps from the faces 3
    or 9 of A along that axis, and no border voxel of A is nearer: d = 2, 26 times.  From dA to dB: with m the number of coordinates
    of p in dA outside [5, 7] by k_i in {1, 2} each, d^2 = sum k_i^2."""
    a = np.zeros((13, 13, 13), bool); b = np.zeros((13, 13, 13), bool)
    a[3:10, 3:10, 3:10] = True; b[5:8, 5:8, 5:8] = True
    off = np.array([2, 1, 0, 0, 0, 1, 2])                           # distance of coordinate 3..9 to the interval [5, 7]
    want = []
    for i in range(7):
        for j in range(7):
            for k in range(7):
                if 0 in (i, j, k) or 6 in (i, j, k):
                    want.append(math.sqrt(float(off[i] ** 2 + off[j] ** 2 + off[k] ** 2)))
    assert len(want) == 218
    da, db = S.distances(a, b)
    assert sorted(da.tolist()) == sorted(want) and db.tolist() == [2.0] * 26
    r = S.surface(a, b, (1.0, 2.0, math.sqrt(5.0), 3.0))
    assert r["counts"] == (343, 27, 218, 26)
    assert r["asd"] == (math.fsum(want) / 218, 2.0) and r["assd"] == (math.fsum(want) / 218 + 2.0) / 2.0
    for t, tau in enumerate((1.0, 2.0, math.sqrt(5.0), 3.0)):
        w = [sum(1 for d in want if d <= tau), 26 if tau >= 2.0 else 0]
        assert r["within"][t] == w and r["nsd"][t] == (w[0] + w[1]) / 244.0
    assert r["within"][0] == [0, 0] and r["within"][1][0] == 9 * 6         # the face centres 3 x 3, distance 2


def test_identical_masks_and_empty_masks():
    m = H.blobs((12, 13, 14), 3, np.random.default_rng(1))
    r = S.surface(m, m, (0.0, 0.5))
    n = int(H.border(m).sum())
    assert r["nsd"] == [1.0, 1.0] and r["asd"] == (0.0, 0.0) and r["assd"] == 0.0 and r["within"] == [[n, n], [n, n]]
    e = np.zeros_like(m)
    for a, b in ((e, m), (m, e), (e, e)):
        r = S.surface(a, b, (1.0,))
        assert r["within"] == [[0, 0]] and math.isnan(r["nsd"][0]) and math.isnan(r["assd"]) and all(math.isnan(v) for v in r["asd"])
    assert S.surface(m, m, ())["nsd"] == [] and S.asd_bound(4, 2.0) == 16.0 * 2.0 ** -53


# ------------------------------------------------------------------ brute force against scipy's transform
@pytest.mark.parametrize("spacing", [None, (1.0, 1.0, 2.5)], ids=["unit", "1x1x2.5"])
@pytest.mark.parametrize("connectivity", [1, 3])
def test_brute_force_distances_equal_scipy_edt(spacing, connectivity):
    rng = np.random.default_rng(7)
    a, b = H.blobs((14, 15, 16), 3, rng, 1.5, 4.0), H.blobs((14, 15, 16), 3, rng, 1.5, 4.0)
    fp = ndimage.generate_binary_structure(3, connectivity)
    ba, bb = a & ~ndimage.binary_erosion(a, structure=fp), b & ~ndimage.binary_erosion(b, structure=fp)
    sp = spacing or (1.0, 1.0, 1.0)
    da, db = S.distances(a, b, spacing, connectivity)
    assert np.array_equal(da, ndimage.distance_transform_edt(~bb, sampling=sp)[ba])
    assert np.array_equal(db, ndimage.distance_transform_edt(~ba, sampling=sp)[bb])
    sa, sb = S.distances(a, b, spacing, connectivity, use_scipy=True)
    assert np.array_equal(da, sa) and np.array_equal(db, sb)
    da, db = S.distances(a, b, spacing, connectivity, all_border=True)
    assert np.array_equal(da, ndimage.distance_transform_edt(~b, sampling=sp)[a]) and db.size == int(b.sum())


# ------------------------------------------------------------------ host wrappers
def test_host_wrappers_equal_restatement():
    from utils import hausdorff as uh
    rng = np.random.default_rng(11)
    a, b = H.blobs((14, 15, 16), 3, rng, 1.5, 4.0), H.blobs((14, 15, 16), 3, rng, 1.5, 4.0)
    for sp, conn in ((None, 1), ((1.0, 1.0, 2.5), 2)):
        r = S.surface(a, b, (1.0, 2.5), sp, conn)
        assert uh.avg_surface_distance(a, b, voxel_spacing=sp, connectivity=conn) == r["asd"][0]
        assert uh.avg_surface_distance(b, a, voxel_spacing=sp, connectivity=conn) == r["asd"][1]
        assert uh.avg_surface_distance_symmetric(torch.from_numpy(a), torch.from_numpy(b), voxel_spacing=sp, connectivity=conn) == r["assd"]
        assert uh.normalized_surface_dice(a, b, 1.0, voxel_spacing=sp, connectivity=conn) == r["nsd"][0]
        assert uh.normalized_surface_dice(a.astype(np.int64) * 4, b, tolerance=2.5, voxel_spacing=sp, connectivity=conn) == r["nsd"][1]
        assert uh.surface_stats(a, b, (1.0, 2.5), sp, conn) == (r["asd"][0], r["asd"][1], r["assd"], r["nsd"])
    r4 = S.surface(a, b, (1.0,), all_border=True)                   # [1, ...] inputs: every mask voxel is a border voxel
    assert uh.normalized_surface_dice(a[None], b[None], 1.0) == r4["nsd"][0] and r4["counts"][2] == int(a.sum())
    assert uh.avg_surface_distance_symmetric(a[None], b[None], voxel_spacing=(3.0, 1.0, 1.0, 1.0)) == r4["assd"]
    cm = uh.ConfusionMatrix(a, b)
    assert uh.avg_surface_distance_symmetric(confusion_matrix=cm) == S.surface(a, b)["assd"]
    e, f = np.zeros_like(a), np.ones_like(a)
    for fn in (uh.avg_surface_distance, uh.avg_surface_distance_symmetric, uh.normalized_surface_dice):
        for x, y in ((e, b), (a, e), (f, b), (a, f)):
            assert fn(x, y) == 0.0 and math.isnan(fn(x, y, nan_for_nonexisting=True))
    with pytest.raises(RuntimeError, match="first supplied array"):
        uh.surface_stats(e, b)
    with pytest.raises(RuntimeError, match="second supplied array"):
        uh.surface_stats(a, e)
    with pytest.raises(ValueError):
        uh.normalized_surface_dice(a, b, -1.0)
    with pytest.raises(ValueError):
        uh.normalized_surface_dice(a, b, math.nan)
    with pytest.raises(AssertionError, match="Shape mismatch"):      # the ConfusionMatrix's own check, as for the two HD wrappers
        uh.avg_surface_distance(a, b[:-1])
    with pytest.raises(ValueError):
        uh.avg_surface_distance(np.stack([a, a]), np.stack([b, b]))


def test_surface_regions_on_cpu_tensors():
    import predict_overlap as po
    rng = np.random.default_rng(5)
    seg = np.stack([H.nested_labels((20, 22, 24), rng, scale=0.3), H.nested_labels((20, 22, 24), rng, scale=0.3)])
    tgt = np.stack([H.nested_labels((20, 22, 24), rng, scale=0.3), H.nested_labels((20, 22, 24), rng, scale=0.3)])
    tgt[1][tgt[1] == 3] = 1                                          # no ET in the second target
    out = po.surface_regions(torch.from_numpy(seg), torch.from_numpy(tgt), (0.5, 1.0, 2.0), spacing=(1.0, 1.0, 2.5))
    assert set(out) == {"nsd", "assd"} and tuple(out["nsd"].shape) == (2, 3, 3) and tuple(out["assd"].shape) == (2, 3)
    assert out["nsd"].dtype == torch.float64 and out["assd"].dtype == torch.float64
    for b in range(2):
        for r, (o, g) in enumerate(zip(H.regions(seg[b]), H.regions(tgt[b]))):
            ref = S.surface(o, g, (0.5, 1.0, 2.0), (1.0, 1.0, 2.5))
            if (b, r) == (1, 2):
                assert bool(torch.isnan(out["nsd"][b, r]).all()) and math.isnan(float(out["assd"][b, r]))
            else:
                assert out["nsd"][b, r].tolist() == ref["nsd"] and float(out["assd"][b, r]) == ref["assd"]
    assert po.surface_regions(torch.from_numpy(seg), torch.from_numpy(tgt))["nsd"].shape == (2, 3, 1)
    for bad in ((-1.0,), (math.nan,), (1.0,) * 5):
        with pytest.raises(ValueError):
            po.surface_regions(torch.from_numpy(seg), torch.from_numpy(tgt), bad)
    with pytest.raises(ValueError):
        po.surface_regions(torch.from_numpy(seg), torch.from_numpy(tgt[:, :-1]))


# ------------------------------------------------------------------ lesion-wise
def _missed_and_spurious():
    """Three lesions: one matched in part, one matched by a shifted copy, one missed; and one spurious predicted component."""
    gt, pred = np.zeros((24, 40, 48), bool), np.zeros((24, 40, 48), bool)
    gt[4:10, 4:10, 4:10] = True
    gt[4:9, 20:25, 30:35] = True
    gt[15:19, 30:34, 10:14] = True
    pred[5:11, 4:10, 5:12] = True
    pred[4:9, 20:25, 31:36] = True
    pred[18:22, 5:9, 40:44] = True
    return pred, gt


def test_lesionwise_nsd_restatement_by_hand():
    pred, gt = _missed_and_spurious()
    ref = LW.lesionwise(pred, gt, min_lesion_voxels=0)
    assert ref["counts"] == (3, 3, 2, 1, 1, 3)
    nsd, lw = S.lesionwise_nsd(pred, gt, (0.5, 1.0), min_lesion_voxels=0)
    assert nsd.shape == (3, 2) and nsd[2].tolist() == [0.0, 0.0] and (nsd[:2] > 0).all() and (nsd[:2, 0] < nsd[:2, 1]).all()
    g1 = S.surface(pred & (np.arange(48) >= 31)[None, None, :] & (np.arange(40) >= 20)[None, :, None], gt & (np.arange(48) >= 30)[None, None, :], (0.5, 1.0))
    assert nsd[1].tolist() == g1["nsd"]
    assert lw == [(nsd[0, t] + nsd[1, t] + nsd[2, t]) / 4 for t in range(2)]
    e = np.zeros_like(gt)
    assert S.lesionwise_nsd(e, e, (1.0,))[1] == [1.0] and S.lesionwise_nsd(pred, e, (1.0,))[1] == [0.0]


@pytest.mark.parametrize("case", ["scene", "missed and spurious"])
def test_lesionwise_metrics_nsd_on_cpu_tensors(case):
    import predict_overlap as po
    pred, gt = LW.scene() if case == "scene" else _missed_and_spurious()
    seg, tgt = torch.from_numpy(LW.labels_from_mask(pred)[None]), torch.from_numpy(LW.labels_from_mask(gt)[None])
    kw = dict(min_lesion_voxels=0)
    base = po.lesionwise_metrics(seg, tgt, with_table=True, **kw)
    out = po.lesionwise_metrics(seg, tgt, with_table=True, nsd_tolerances=(0.5, 1.0), **kw)
    assert set(out) == set(base) | {"lw_nsd", "lesion_nsd"} and all(torch.equal(out[k], base[k]) for k in base)
    assert tuple(out["lw_nsd"].shape) == (1, 3, 2) and tuple(out["lesion_nsd"].shape) == (1, 3, 64, 2)
    nsd, lw = S.lesionwise_nsd(pred, gt, (0.5, 1.0), **kw)
    for r in range(3):
        assert out["lw_nsd"][0, r].tolist() == lw
        assert out["lesion_nsd"][0, r, :nsd.shape[0]].tolist() == nsd.tolist() and not bool(out["lesion_nsd"][0, r, nsd.shape[0]:].any())
    short = po.lesionwise_metrics(seg, tgt, nsd_tolerances=(1.0,), **kw)
    assert set(short) == {"dice", "hd95", "counts", "lw_nsd"} and short["lw_nsd"][0, 0].tolist() == [lw[1]]
    with pytest.raises(ValueError):
        po.lesionwise_metrics(seg, tgt, nsd_tolerances=(-0.5,))


def test_lesionwise_metrics_without_the_keyword_is_unchanged():
    import predict_overlap as po
    pred, gt = LW.scene()
    seg, tgt = torch.from_numpy(LW.labels_from_mask(pred)[None]), torch.from_numpy(LW.labels_from_mask(gt)[None])
    out = po.lesionwise_metrics(seg, tgt)
    assert set(out) == {"dice", "hd95", "counts"}
    ref = LW.lesionwise(pred, gt)
    for r in range(3):
        assert float(out["dice"][0, r]) == pytest.approx(ref["dice"], rel=1e-12) and float(out["hd95"][0, r]) == pytest.approx(ref["hd95"], rel=1e-12)
        assert tuple(out["counts"][0, r].tolist()) == ref["counts"]
    full = po.lesionwise_metrics(seg, tgt, with_table=True)
    assert set(full) == {"dice", "hd95", "counts", "table", "lesion_hd95"} and tuple(full["table"].shape) == (1, 3, 64, 4)
    assert full["table"][0, 0, :3].tolist() == ref["table"].tolist()
