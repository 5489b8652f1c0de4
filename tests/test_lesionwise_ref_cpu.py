"""The scipy restatement of the lesion-wise Dice / HD95 definition (tests/lesionwise_ref.py) and the host path of
predict_overlap.lesionwise_metrics, pinned on a hand-built scene whose numbers can be worked out by hand, and the identity that lets the
device path dilate once per region rather than once per lesion."""
import numpy as np
import pytest
import torch
import hausdorff_ref as H
import lesionwise_ref as LW

# (parameters, (G, kept, FP, P), lw_dice, lw_hd95) on LW.scene(); the merged lesion has dice 480 / 792 = 20 / 33 and hd95 2, the
# 27-voxel lesion dice 2 / 3 and hd95 1, the 125-voxel lesion is missed, two predicted components are spurious
SCENE = [
    (dict(), (3, 2, 2, 4), 5.0 / 33.0, 281.0),
    (dict(min_lesion_voxels=0), (3, 3, 2, 4), 14.0 / 55.0, 225.0),
    (dict(dilation=0), (4, 3, 2, 4), None, 227.6),
]


def _check_scene(res, counts, dice, hd95):
    g, kept, matched, fp, fn, p = (int(v) for v in res["counts"])
    assert (g, kept, fp, p) == counts and matched == p - fp
    if dice is not None:
        assert float(res["dice"]) == pytest.approx(dice, rel=1e-14)
    assert float(res["hd95"]) == pytest.approx(hd95, rel=1e-14)


@pytest.mark.parametrize("kw,counts,dice,hd95", SCENE, ids=["defaults", "min0", "dilation0"])
def test_restatement_on_the_hand_built_scene(kw, counts, dice, hd95):
    pred, gt = LW.scene()
    res = LW.lesionwise(pred, gt, **kw)
    _check_scene(res, counts, dice, hd95)
    if not kw:
        assert res["table"].tolist() == [[360, 432, 240, 1], [125, 0, 0, 0], [27, 27, 18, 1]]
        assert res["lesion_hd95"].tolist() == [2.0, 374.0, 1.0] and res["counts"][4] == 1
    if kw == dict(dilation=0):
        # the two parts are lesions of their own (216 and 144 voxels), both touched by the one component of 432 voxels
        assert res["table"].tolist() == [[216, 432, 150, 1], [144, 432, 90, 1], [125, 0, 0, 0], [27, 27, 18, 1]]
        assert float(res["dice"]) == pytest.approx((300.0 / 648.0 + 180.0 / 576.0) / 5.0, rel=1e-14)
        assert abs(float(res["dice"]) - 0.155093) < 5e-7


def test_restatement_degenerate_inputs():
    pred, gt = LW.scene()
    empty = np.zeros_like(gt)
    r = LW.lesionwise(gt, gt)
    assert (r["dice"], r["hd95"]) == (1.0, 0.0) and r["counts"] == (3, 2, 4, 0, 0, 4)      # the two merged parts are two components
    r = LW.lesionwise(empty, gt)
    assert (r["dice"], r["hd95"]) == (0.0, 374.0) and r["counts"] == (3, 2, 0, 0, 2, 0)
    r = LW.lesionwise(pred, empty)
    assert (r["dice"], r["hd95"]) == (0.0, 374.0) and r["counts"] == (0, 0, 0, 4, 0, 4)
    r = LW.lesionwise(empty, empty)
    assert (r["dice"], r["hd95"]) == (1.0, 0.0) and r["counts"] == (0, 0, 0, 0, 0, 0)


@pytest.mark.parametrize("seed", [0, 1, 2])
@pytest.mark.parametrize("dilation", [1, 3])
def test_dilation_of_a_lesion_is_its_dilated_component(seed, dilation):
    """dilate(gt & (dil_cc == g)) == (dil_cc == g): nothing has to be dilated per lesion."""
    rng = np.random.default_rng(seed)
    gt = H.blobs((30, 36, 33), 9, rng, rmin=1.0, rmax=3.5)
    dil_cc, ng = LW.lesions(gt, dilation)
    assert ng >= 2
    for g in range(1, ng + 1):
        assert np.array_equal(LW.dilate(gt & (dil_cc == g), 2, dilation), dil_cc == g), g


def _host(pred, gt, **kw):
    import predict_overlap as po
    seg = torch.from_numpy(LW.labels_from_mask(pred)[None])
    tgt = torch.from_numpy(LW.labels_from_mask(gt)[None])
    return po.lesionwise_metrics(seg, tgt, with_table=True, **kw)


def _assert_host_equals_restatement(out, b, r, ref):
    assert out["dice"].dtype == torch.float64 and out["hd95"].dtype == torch.float64 and out["counts"].dtype == torch.int64
    assert tuple(int(v) for v in out["counts"][b, r]) == ref["counts"]
    g = ref["counts"][0]
    assert out["table"][b, r, :g].tolist() == ref["table"].tolist() and not bool(out["table"][b, r, g:].any())
    assert np.allclose(out["lesion_hd95"][b, r, :g].numpy(), ref["lesion_hd95"], rtol=1e-14, atol=0)
    assert not bool(out["lesion_hd95"][b, r, g:].any())
    assert float(out["dice"][b, r]) == pytest.approx(ref["dice"], rel=1e-12, abs=0)
    assert float(out["hd95"][b, r]) == pytest.approx(ref["hd95"], rel=1e-12, abs=0)


@pytest.mark.parametrize("kw,counts,dice,hd95", SCENE, ids=["defaults", "min0", "dilation0"])
def test_host_path_on_the_hand_built_scene(kw, counts, dice, hd95):
    pred, gt = LW.scene()
    out = _host(pred, gt, **kw)
    assert tuple(out["dice"].shape) == (1, 3) and tuple(out["counts"].shape) == (1, 3, 6) and tuple(out["table"].shape) == (1, 3, 64, 4)
    ref = LW.lesionwise(pred, gt, **kw)
    for r in range(3):                                   # label 3 throughout: the three regions coincide
        _check_scene({k: v[0, r] for k, v in out.items()}, counts, dice, hd95)
        _assert_host_equals_restatement(out, 0, r, ref)
    assert set(po_keys(pred, gt)) == {"dice", "hd95", "counts"}


def po_keys(pred, gt):
    import predict_overlap as po
    return po.lesionwise_metrics(torch.from_numpy(LW.labels_from_mask(pred)[None]), torch.from_numpy(LW.labels_from_mask(gt)[None]))


def test_host_path_degenerate_inputs_and_nested_labels():
    import predict_overlap as po
    pred, gt = LW.scene()
    empty = np.zeros_like(gt)
    for a, b, want, fp in ((gt, gt, (1.0, 0.0), 0), (empty, gt, (0.0, 374.0), 0), (pred, empty, (0.0, 374.0), 4), (empty, empty, (1.0, 0.0), 0)):
        out = _host(a, b)
        assert (float(out["dice"][0, 0]), float(out["hd95"][0, 0])) == want and int(out["counts"][0, 0, 3]) == fp
    rng = np.random.default_rng(6)
    shape = (32, 48, 40)
    seg = np.stack([H.nested_labels(shape, rng, scale=0.45), H.nested_labels(shape, rng, scale=0.4)])
    tgt = np.stack([H.nested_labels(shape, rng, scale=0.45), H.nested_labels(shape, rng, scale=0.4)])
    out = po.lesionwise_metrics(torch.from_numpy(seg), torch.from_numpy(tgt), min_lesion_voxels=5, with_table=True)
    for b in range(2):
        for r, (o, g) in enumerate(zip(H.regions(seg[b]), H.regions(tgt[b]))):
            _assert_host_equals_restatement(out, b, r, LW.lesionwise(o, g, min_lesion_voxels=5))


def test_host_path_has_no_lesion_cap():
    gt = np.zeros((40, 40, 24), bool)
    gt[2::8, 2::8, 2::8] = True                          # 5 x 5 x 3 single voxels, dilations apart
    pred = np.zeros_like(gt)
    pred[2:4, 2:4, 2:4] = True
    ref = LW.lesionwise(pred, gt, min_lesion_voxels=0)
    assert ref["counts"] == (75, 75, 1, 0, 74, 1)
    out = _host(pred, gt, min_lesion_voxels=0)
    assert tuple(out["table"].shape) == (1, 3, 75, 4)
    _assert_host_equals_restatement(out, 0, 0, ref)


def test_bad_arguments_raise_value_error():
    import predict_overlap as po
    seg = torch.zeros((1, 4, 5, 6), dtype=torch.int64)
    for kw in (dict(dilation=-1), dict(dilation=9), dict(min_lesion_voxels=-1), dict(penalty=-1.0), dict(penalty=float("nan")),
               dict(penalty=float("inf"))):
        with pytest.raises(ValueError):
            po.lesionwise_metrics(seg, seg, **kw)
    for bad in (seg[0], seg.float(), seg.int(), seg.numpy(), torch.zeros((0, 4, 5, 6), dtype=torch.int64),
                torch.zeros((1, 4, 5, 7), dtype=torch.int64)):
        with pytest.raises(ValueError):
            po.lesionwise_metrics(bad, seg)
        with pytest.raises(ValueError):
            po.lesionwise_metrics(seg, bad)


class _Stub(torch.nn.Module):
    """Stands in for the model on the CPU path of validate_softmax: class scores that depend on the input only."""

    class _U:
        class InitConv:
            dropout = 0.0
    Unet_list = _U

    def forward(self, x, missing_modal):
        return (torch.softmax(x * 3.0, dim=1),)


def test_validate_softmax_cpu_lesionwise_none_keeps_the_tuple_and_true_appends_the_dict(monkeypatch):
    """The result plumbing only, so the eight-window stitcher (which needs a 240 x 240 x 155 volume) is replaced by one forward of the
    stub over the hand-built scene's volume."""
    import predict_overlap as po
    monkeypatch.setattr(po, "tailor_and_concat", lambda x, missing_modal, model: model(x, missing_modal)[0])
    pred, gt = LW.scene()
    lab = LW.labels_from_mask(pred)
    lab[pred & (np.indices(pred.shape)[2] % 2 == 0)] = 2                                             # the regions differ
    x = torch.nn.functional.one_hot(torch.from_numpy(lab), 4).permute(3, 0, 1, 2)[None].float()     # argmax gives lab back
    target = torch.from_numpy(LW.labels_from_mask(gt)[None])
    m = _Stub()
    plain = po.validate_softmax(x, target, m)
    a = po.validate_softmax(x, target, m, lesionwise=None)
    assert len(plain) == len(a) == 3 and torch.equal(a[0], plain[0]) and np.array_equal(a[0].numpy()[0], lab)
    assert len(po.validate_softmax(x, target, m, with_miou=True, lesionwise=None)) == 4
    b = po.validate_softmax(x, target, m, lesionwise=True)
    assert len(b) == 4 and set(b[3]) == {"dice", "hd95", "counts"}
    want = po.lesionwise_metrics(b[0], target)
    assert all(torch.equal(b[3][k], want[k]) for k in want)
    assert tuple(int(v) for v in want["counts"][0, 0]) == (3, 2, 2, 2, 1, 4) and float(want["hd95"][0, 0]) == 281.0
    kw = dict(min_lesion_voxels=0, with_table=True)
    c = po.validate_softmax(x, target, m, with_miou=True, lesionwise=kw)
    assert len(c) == 5 and torch.equal(c[0], a[0]) and set(c[4]) == {"dice", "hd95", "counts", "table", "lesion_hd95"}
    want = po.lesionwise_metrics(c[0], target, **kw)
    assert all(torch.equal(c[4][k], want[k]) for k in want)
    assert po.validate_softmax(x, None, m, lesionwise=True)[-1] is None
