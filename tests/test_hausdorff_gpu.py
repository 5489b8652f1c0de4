"""Device Hausdorff distance / HD95 (csrc/metrics.hip: cwf_region_bits, cwf_hausdorff) against the float64 restatement of medpy
(tests/hausdorff_ref.py): the kernels on odd shapes for every connectivity and spacing, full-size BraTS label maps, the all-border
mode of [1, ...] inputs, the utils.hausdorff / tools.softmax_hd_dice drop-ins and validate_softmax(with_hd95=True)."""
import math

import numpy as np
import pytest
import torch

import hausdorff_ref as H

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SHAPES = [(23, 31, 17), (1, 40, 40), (64, 48, 40)]


def _cases(shape, rng):
    yield "blobs", H.blobs(shape, 3, rng), H.blobs(shape, 4, rng)
    c = [s / 2 for s in shape]
    rr = min(s for s in shape if s > 1) / 2
    yield "shells", H.shell(shape, c, rr * 0.8, rr * 0.55), H.shell(shape, [x + 0.7 for x in c], rr * 0.7, rr * 0.5)
    a = np.zeros(shape, bool); b = np.zeros(shape, bool)
    a[tuple(int(rng.integers(0, s)) for s in shape)] = True
    b[tuple(int(rng.integers(0, s)) for s in shape)] = True
    yield "single voxels", a, b
    a = np.zeros(shape, bool); b = np.zeros(shape, bool)
    a[0, 0, 0] = True; b[-1, -1, -1] = True
    yield "opposite corners", a, b
    a = np.zeros(shape, bool)
    a[:, : max(1, shape[1] // 3), :] = True
    yield "face-touching", a, H.blobs(shape, 2, rng)
    yield "full volume", np.ones(shape, bool), H.blobs(shape, 2, rng)
    a = np.zeros(shape, bool); b = np.zeros(shape, bool)
    a[tuple(s // 3 for s in shape)] = True; b[tuple(s - 1 - s // 4 for s in shape)] = True
    yield "n = 2", a, b


def _check(got, ref, unit, what):
    if unit:      # exact integers before the sqrt; sqrt and the lerp may differ by one ulp at most
        assert abs(got - ref) <= np.spacing(max(abs(ref), 1.0)), (what, got, ref)
    else:
        assert got == pytest.approx(ref, rel=1e-12, abs=0), (what, got, ref)


def _run(hip, a, b, R=1, **kw):
    ta = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    tb = torch.from_numpy(np.ascontiguousarray(b)).to(DEV)
    if ta.dim() == 3:
        ta, tb = ta[None], tb[None]
    hd, hd95, counts = hip.hausdorff(ta, tb, R, **kw)
    torch.cuda.synchronize()
    return hd.cpu().numpy(), hd95.cpu().numpy(), counts.cpu().numpy()


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("connectivity", [1, 2, 3])
@pytest.mark.parametrize("spacing", [None, (0.9375, 0.9375, 1.5)], ids=["unit", "aniso"])
def test_kernels_match_restatement(hip, shape, connectivity, spacing):
    rng = np.random.default_rng(hash((shape, connectivity)) % 2 ** 32)
    for name, a, b in _cases(shape, rng):
        hd, hd95, counts = _run(hip, a, b, spacing=spacing, connectivity=connectivity)
        ba, bb = H.border(a, connectivity), H.border(b, connectivity)
        assert counts[0, 0].tolist() == [int(a.sum()), int(b.sum()), int(ba.sum()), int(bb.sum())], name
        rh, r95 = H.hd_hd95(a, b, spacing, connectivity)
        _check(float(hd[0, 0]), rh, spacing is None, (name, "hd"))
        _check(float(hd95[0, 0]), r95, spacing is None, (name, "hd95"))


def test_empty_mask_gives_nan_and_counts(hip):
    a = np.zeros((9, 10, 11), bool); b = np.zeros((9, 10, 11), bool)
    b[3:5, 4:6, 5:7] = True
    hd, hd95, counts = _run(hip, a, b)
    assert math.isnan(hd[0, 0]) and math.isnan(hd95[0, 0])
    assert counts[0, 0].tolist() == [0, 8, 0, 8]


def test_hd95_upper_interpolation_branch_on_device(hip):
    a = np.zeros((1, 1, 6), bool); b = np.zeros((1, 1, 6), bool)
    a[0, 0, [0, 4]] = True; b[0, 0, 1] = True
    hd, hd95, _ = _run(hip, a, b)
    assert (float(hd[0, 0]), float(hd95[0, 0])) == H.hd_hd95(a, b)


def _brats_pair(rng, shape=(240, 240, 155)):
    seg = H.nested_labels(shape, rng)
    tgt = H.nested_labels(shape, rng, centers=None)
    return seg, tgt


def test_brats_size_batch_two_against_scipy_restatement(hip):
    pytest.importorskip("scipy")
    rng = np.random.default_rng(2024)
    pairs = [_brats_pair(rng) for _ in range(2)]
    be = hip
    seg = torch.from_numpy(np.stack([p[0] for p in pairs])).to(DEV)
    tgt = torch.from_numpy(np.stack([p[1] for p in pairs])).to(DEV)
    hd, hd95, counts = be.hausdorff(be.region_bits(seg), be.region_bits(tgt), 3)
    hd, hd95, counts = hd.cpu().numpy(), hd95.cpu().numpy(), counts.cpu().numpy()
    for i, (s, t) in enumerate(pairs):
        for r, (o, g) in enumerate(zip(H.regions(s), H.regions(t))):
            assert counts[i, r].tolist() == [int(o.sum()), int(g.sum()), int(H.border(o).sum()), int(H.border(g).sum())]
            rh, r95 = H.hd_hd95(o, g, use_scipy=True)
            _check(float(hd[i, r]), rh, True, (i, r, "hd"))
            _check(float(hd95[i, r]), r95, True, (i, r, "hd95"))


def test_brats_size_sparse_structures_against_brute_force(hip):
    shape = (240, 240, 155)
    rng = np.random.default_rng(99)
    a = np.zeros(shape, bool); b = np.zeros(shape, bool)
    for m in (a, b):
        for _ in range(6):
            c = [int(rng.integers(3, s - 4)) for s in shape]
            m[c[0] - 2:c[0] + 2, c[1] - 2:c[1] + 3, c[2] - 1:c[2] + 2] = True
    a[0, 0, 0] = True; b[239, 239, 154] = True
    for sp in (None, (0.9375, 0.9375, 1.5)):
        hd, hd95, counts = _run(hip, a, b, spacing=sp)
        rh, r95 = H.hd_hd95(a, b, sp)
        _check(float(hd[0, 0]), rh, sp is None, "hd")
        _check(float(hd95[0, 0]), r95, sp is None, "hd95")
        assert counts[0, 0, 2:].tolist() == [int(H.border(a).sum()), int(H.border(b).sum())]


@pytest.mark.parametrize("connectivity", [1, 3])
def test_all_border_mode_matches_rank4_restatement(hip, connectivity):
    from utils import hausdorff as HD
    rng = np.random.default_rng(5)
    shape = (23, 31, 17)
    for sp in (None, (1.0, 0.9375, 0.9375, 1.5)):
        for name, a, b in list(_cases(shape, rng))[:3]:
            a4, b4 = a[None], b[None]
            rh, r95 = H.hd_hd95(a4, b4, sp, connectivity)
            hd, hd95, counts = _run(hip, a, b, spacing=None if sp is None else sp[1:], connectivity=connectivity, all_border=True)
            assert counts[0, 0].tolist() == [int(a.sum()), int(b.sum()), int(a.sum()), int(b.sum())]
            _check(float(hd[0, 0]), rh, sp is None, (name, "hd"))
            _check(float(hd95[0, 0]), r95, sp is None, (name, "hd95"))
            _check(HD.hausdorff_distance_95(a4, b4, voxel_spacing=sp, connectivity=connectivity), r95, sp is None, (name, "drop-in"))


def test_dropins_on_cuda_and_numpy_inputs(hip):
    from utils import hausdorff as HD
    from utils import tools
    rng = np.random.default_rng(17)
    shape = (64, 48, 40)
    seg, tgt = H.nested_labels(shape, rng, scale=0.4), H.nested_labels(shape, rng, scale=0.4)
    for o, t in zip(H.regions(seg), H.regions(tgt)):
        for sp in (None, 1.5, (0.9375, 0.9375, 1.5)):
            rh, r95 = H.wrapped(0, o, t, voxel_spacing=sp), H.wrapped(1, o, t, voxel_spacing=sp)
            for x, y in ((o, t), (torch.from_numpy(o).to(DEV), torch.from_numpy(t).to(DEV)), (torch.from_numpy(o), torch.from_numpy(t))):
                got = HD.hausdorff_distance(x, y, voxel_spacing=sp), HD.hausdorff_distance_95(x, y, voxel_spacing=sp)
                assert all(isinstance(v, float) for v in got)
                _check(got[0], rh, sp is None, "hd")
                _check(got[1], r95, sp is None, "hd95")
    # predict_simple.py's [1, H, W, D] arrays: every mask voxel is a border voxel
    o4, t4 = H.regions(seg)[1][None], H.regions(tgt)[1][None]
    _check(HD.hausdorff_distance_95(o4, t4), H.wrapped(1, o4, t4), True, "rank 4")
    for x, y in ((seg, tgt), (torch.from_numpy(seg).to(DEV), torch.from_numpy(tgt).to(DEV)), (seg[None], tgt[None])):
        dice, hds = tools.softmax_hd_dice(x, y)
        ref_dice = tools.softmax_output_dice(x, y)
        assert [float(d) for d in dice] == [float(d) for d in ref_dice]
        xs, ys = np.asarray(x.cpu() if isinstance(x, torch.Tensor) else x), np.asarray(y.cpu() if isinstance(y, torch.Tensor) else y)
        for r, (o, t) in enumerate(zip(H.regions(xs), H.regions(ys))):
            _check(hds[r], H.hd(o, t), True, ("softmax_hd_dice", r))
    empty = seg.copy(); empty[empty == 3] = 1
    with pytest.raises(RuntimeError, match="first supplied array"):
        tools.softmax_hd_dice(torch.from_numpy(empty).to(DEV), torch.from_numpy(tgt).to(DEV))


def test_validate_softmax_hd95_on_model_output(hip):
    """validate_softmax(with_hd95=True) on the model's 240x240x155 output: the HD95 against the restatement on host copies of seg and
    target (surface mode, 0 for empty or full regions), every other output identical to the call without the flag."""
    import predict_overlap as po
    from models.clswiseformer.cls_wise_former import get_cls_wise_former
    from oracle import reference_model as rm
    from utils import synthetic as syn
    m = get_cls_wise_former(dataset="brats", _conv_repr=True, _pe_type="fixed")
    m.load_state_dict(syn.det_state_dict(rm.param_shapes()), strict=False)
    m = m.to(DEV).eval()
    x = torch.randn(1, 4, 240, 240, 155, generator=torch.Generator().manual_seed(5)).to(DEV)
    rng = np.random.default_rng(3)
    target = torch.from_numpy(H.nested_labels((240, 240, 155), rng)[None]).to(DEV)
    seg0, prob0, dice0, miou0 = po.validate_softmax(x, target, m, with_miou=True)
    seg, prob, dice, miou, hd95 = po.validate_softmax(x, target, m, with_miou=True, with_hd95=True)
    assert torch.equal(seg, seg0) and torch.equal(prob, prob0)
    assert [float(d) for d in dice] == [float(d) for d in dice0] and [float(v) for v in miou] == [float(v) for v in miou0]
    assert hd95.dtype == torch.float64 and tuple(hd95.shape) == (1, 3)
    res = po.validate_softmax(x, target, m, with_hd95=True)
    assert len(res) == 4 and torch.equal(res[3], hd95)
    s, t = seg.cpu().numpy()[0], target.cpu().numpy()[0]
    for r, (o, g) in enumerate(zip(H.regions(s), H.regions(t))):
        ref = H.wrapped(1, o, g, use_scipy=(H.border(o).sum() * H.border(g).sum() > 5e7))
        _check(float(hd95[0, r]), ref, True, ("validate_softmax", r))
