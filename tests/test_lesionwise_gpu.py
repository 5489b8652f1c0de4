"""Device lesion-wise Dice / HD95 (csrc/lesions.hip through backend().dilate_bits, backend().lesionwise,
predict_overlap.lesionwise_metrics and validate_softmax(lesionwise=...)) against the scipy restatement of tests/lesionwise_ref.py.
Counts and tables are integers and must be equal; a per-lesion HD95 is held as tests/test_hausdorff_gpu.py holds cwf_hausdorff (unit
spacing: exact integers before the square root, one ulp for the root and the percentile's lerp); the two aggregates are sums of at most
64 float64 terms and a division, held to 1e-12 relative."""
import functools

import numpy as np
import pytest
import torch
from scipy import ndimage

import hausdorff_ref as H
import lesionwise_ref as LW

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


# ------------------------------------------------------------------ dilation
def _planes(shape, seed):
    rng = np.random.default_rng(seed)
    return [rng.random(shape) < p for p in (0.02, 0.1, 0.4)]


def _pack(masks):
    bits = np.zeros(masks[0].shape, dtype=np.uint8)
    for r, m in enumerate(masks):
        bits |= m.astype(np.uint8) << r
    return bits


def _corners():
    m = np.zeros((8, 8, 8), bool)
    m[::7, ::7, ::7] = True
    assert int(m.sum()) == 8
    return [m, np.zeros_like(m), m]


@pytest.mark.parametrize("connectivity", [1, 2, 3])
@pytest.mark.parametrize("name,masks", [("17x33x65", _planes((17, 33, 65), 3)), ("1x1x1 set", [np.ones((1, 1, 1), bool)] * 3),
                                        ("1x1x1 unset", [np.zeros((1, 1, 1), bool)] * 3), ("corners", _corners())],
                         ids=lambda v: v if isinstance(v, str) else "")
def test_dilate_bits_equals_scipy(hip, connectivity, name, masks):
    bits = torch.from_numpy(np.stack([_pack(masks), _pack(masks[::-1])])).to(DEV)          # B = 2, the planes in two orders
    keep = bits.clone()
    for iterations in range(5):
        got = hip.dilate_bits(bits, connectivity, iterations).cpu().numpy()
        assert got.dtype == np.uint8 and torch.equal(bits, keep)
        for b, order in enumerate((masks, masks[::-1])):
            want = _pack([LW.dilate(m, connectivity, iterations) for m in order])
            assert np.array_equal(got[b], want), (name, connectivity, iterations, b)


# ------------------------------------------------------------------ cases shared by the device test and the vacuity check
def _scene(which="scene", **kw):
    pred, gt = LW.scene()
    empty = np.zeros_like(gt)
    pred, gt = {"scene": (pred, gt), "pred = gt": (gt, gt), "empty pred": (empty, gt), "empty gt": (pred, empty),
                "both empty": (empty, empty)}[which]
    return LW.labels_from_mask(pred)[None], LW.labels_from_mask(gt)[None], kw


def _nested(shape, nb, seed, scale=0.3):
    """Per sample: three nested blobs in each map -- one pair overlapping in part, one only in the target, one only in the prediction."""
    rng = np.random.default_rng(seed)
    segs, tgts = [], []
    for _ in range(nb):
        c = [[0.25 * shape[0], 0.25 * shape[1], 0.3 * shape[2]], [0.7 * shape[0], 0.3 * shape[1], 0.75 * shape[2]],
             [0.6 * shape[0], 0.78 * shape[1], 0.3 * shape[2]]]
        far = [0.2 * shape[0], 0.8 * shape[1], 0.8 * shape[2]]
        tgts.append(H.nested_labels(shape, rng, centers=c, scale=scale))
        segs.append(H.nested_labels(shape, rng, centers=[[c[0][0] + 1, c[0][1] + 1, c[0][2]], [c[1][0], c[1][1] - 1, c[1][2] + 1], far],
                                    scale=scale))
    return np.stack(segs), np.stack(tgts), dict(min_lesion_voxels=3)


def _cubes(gap, axis):
    gt = np.zeros((20, 24, 28), bool)
    lo = [6, 6, 6]
    gt[6:9, 6:9, 6:9] = True
    lo[axis] += 3 + gap
    gt[lo[0]:lo[0] + 3, lo[1]:lo[1] + 3, lo[2]:lo[2] + 3] = True
    pred = np.zeros_like(gt)
    pred[7:10, 6:9, 6:9] = True
    return LW.labels_from_mask(pred)[None], LW.labels_from_mask(gt)[None], dict(min_lesion_voxels=0)


def _diagonal():
    """Two voxels (7, 7, 7) apart: three 26-neighbour dilations would join them, three 18-neighbour ones do not."""
    gt = np.zeros((20, 20, 20), bool)
    gt[5, 5, 5] = gt[12, 12, 12] = True
    pred = np.zeros_like(gt)
    pred[5:7, 5, 5] = True
    return LW.labels_from_mask(pred)[None], LW.labels_from_mask(gt)[None], dict(min_lesion_voxels=0)


def _bridge():
    """One predicted bar over two lesions 10 voxels apart, and a second component inside the first lesion's dilation only."""
    gt = np.zeros((16, 20, 40), bool)
    gt[5:9, 5:9, 4:8] = True
    gt[5:9, 5:9, 18:22] = True
    pred = np.zeros_like(gt)
    pred[6:8, 6:8, 6:20] = True
    pred[5:7, 11:13, 4:6] = True
    return LW.labels_from_mask(pred)[None], LW.labels_from_mask(gt)[None], dict(min_lesion_voxels=0)


def _faces():
    shape = (17, 33, 65)
    gt = np.zeros(shape, bool)
    pred = np.zeros(shape, bool)
    gt[0:3, 0:3, 0:3] = True
    gt[14:17, 30:33, 62:65] = True
    gt[0:2, 14:18, 62:65] = True
    gt[7:10, 0:2, 30:34] = True
    pred[0:2, 0:4, 0:3] = True
    pred[15:17, 31:33, 60:65] = True
    pred[7:10, 0:3, 31:36] = True
    pred[16, 0, 0] = True
    return LW.labels_from_mask(pred)[None], LW.labels_from_mask(gt)[None], dict(min_lesion_voxels=0)


CASES = {
    "scene": lambda: _scene(),
    "scene min0": lambda: _scene(min_lesion_voxels=0),
    "scene dilation0": lambda: _scene(dilation=0),
    "scene penalty": lambda: _scene(dilation=1, min_lesion_voxels=26, penalty=100.5),
    "scene pred = gt": lambda: _scene("pred = gt"),
    "scene empty pred": lambda: _scene("empty pred"),
    "scene empty gt": lambda: _scene("empty gt"),
    "scene both empty": lambda: _scene("both empty"),
    "nested 32x48x40 B2": lambda: _nested((32, 48, 40), 2, 5),
    "nested 17x33x65": lambda: _nested((17, 33, 65), 1, 9, 0.22),
    "cubes gap 6 axis 0": lambda: _cubes(6, 0),
    "cubes gap 6 axis 2": lambda: _cubes(6, 2),
    "cubes gap 7 axis 0": lambda: _cubes(7, 0),
    "cubes gap 7 axis 2": lambda: _cubes(7, 2),
    "diagonal": _diagonal,
    "bridge": _bridge,
    "faces": _faces,
}


@functools.lru_cache(maxsize=None)
def _case(name):
    """(seg, tgt, kw, ref[b][r]) -- the restatement is computed once per case and shared."""
    seg, tgt, kw = CASES[name]()
    ref = [[LW.lesionwise(o, g, **kw) for o, g in zip(H.regions(seg[b]), H.regions(tgt[b]))] for b in range(seg.shape[0])]
    return seg, tgt, kw, ref


def _device(seg, tgt, **kw):
    import predict_overlap as po
    out = po.lesionwise_metrics(torch.from_numpy(seg).to(DEV), torch.from_numpy(tgt).to(DEV), with_table=True, **kw)
    assert all(v.is_cuda for v in out.values())
    return {k: v.cpu() for k, v in out.items()}


def _assert_equals_restatement(out, b, r, ref, what):
    assert out["dice"].dtype == torch.float64 and out["hd95"].dtype == torch.float64 and out["counts"].dtype == torch.int64
    assert out["table"].dtype == torch.int64 and out["lesion_hd95"].dtype == torch.float64
    print(what, b, r, "counts", out["counts"][b, r].tolist(), ref["counts"], "dice %.17g %.17g" % (float(out["dice"][b, r]), ref["dice"]),
          "hd95 %.17g %.17g" % (float(out["hd95"][b, r]), ref["hd95"]))
    assert tuple(int(v) for v in out["counts"][b, r]) == ref["counts"], what
    g = ref["counts"][0]
    assert out["table"][b, r, :g].tolist() == ref["table"].tolist() and not bool(out["table"][b, r, g:].any()), what
    for i in range(g):
        got, want = float(out["lesion_hd95"][b, r, i]), float(ref["lesion_hd95"][i])
        assert abs(got - want) <= np.spacing(max(abs(want), 1.0)), (what, i, got, want)
    assert not bool(out["lesion_hd95"][b, r, g:].any()), what
    assert float(out["dice"][b, r]) == pytest.approx(ref["dice"], rel=1e-12, abs=0), what
    assert float(out["hd95"][b, r]) == pytest.approx(ref["hd95"], rel=1e-12, abs=0), what


@pytest.mark.parametrize("name", list(CASES))
def test_device_equals_restatement(hip, name):
    seg, tgt, kw, ref = _case(name)
    out = _device(seg, tgt, **kw)
    assert tuple(out["dice"].shape) == (seg.shape[0], 3) and tuple(out["table"].shape) == (seg.shape[0], 3, 64, 4)
    for b in range(seg.shape[0]):
        for r in range(3):
            _assert_equals_restatement(out, b, r, ref[b][r], (name, b, r))


def test_cases_are_not_vacuous():
    """For every region the cases hold a kept lesion scored strictly between 0 and 1, a false negative and a false positive; and the
    geometric cases decide what their names say."""
    partial, fn, fp = [0, 0, 0], [0, 0, 0], [0, 0, 0]
    for name in CASES:
        _, _, kw, ref = _case(name)
        for row in ref:
            for r, x in enumerate(row):
                kept = x["table"][:, 0] > kw.get("min_lesion_voxels", 50)
                partial[r] += int((kept & (x["lesion_dice"] > 0) & (x["lesion_dice"] < 1)).sum())
                fn[r] += x["counts"][4]
                fp[r] += x["counts"][3]
    assert min(partial) > 0 and min(fn) > 0 and min(fp) > 0, (partial, fn, fp)
    for name in ("nested 32x48x40 B2", "nested 17x33x65"):
        for row in _case(name)[3]:
            for r, x in enumerate(row):
                assert x["counts"][3] > 0 and x["counts"][4] > 0 and ((x["lesion_dice"] > 0) & (x["lesion_dice"] < 1)).any(), (name, r)
    for name, want, counts in (("scene pred = gt", (1.0, 0.0), (3, 2, 4, 0, 0, 4)), ("scene empty pred", (0.0, 374.0), (3, 2, 0, 0, 2, 0)),
                               ("scene empty gt", (0.0, 374.0), (0, 0, 0, 4, 0, 4)), ("scene both empty", (1.0, 0.0), (0, 0, 0, 0, 0, 0))):
        for x in _case(name)[3][0]:
            assert (x["dice"], x["hd95"]) == want and x["counts"] == counts, name
    assert _case("scene")[3][0][0]["counts"][:4] == (3, 2, 2, 2) and _case("scene dilation0")[3][0][0]["counts"][0] == 4
    for axis in (0, 2):
        assert _case("cubes gap 6 axis %d" % axis)[3][0][0]["counts"][0] == 1
        assert _case("cubes gap 7 axis %d" % axis)[3][0][0]["counts"][0] == 2
    seg, tgt, _, ref = _case("diagonal")
    assert ref[0][0]["counts"][0] == 2
    assert ndimage.label(ndimage.binary_dilation(tgt[0] > 0, LW.FULL, iterations=3), structure=LW.FULL)[1] == 1
    x = _case("bridge")[3][0][0]
    assert x["counts"] == (2, 2, 2, 0, 0, 2) and x["table"][:, 3].tolist() == [2, 1] and x["table"][:, 1].tolist() == [64, 56]


# ------------------------------------------------------------------ the cap of 64 lesions
def _lattice(n):
    pts = [(i, j, k) for i in range(2, 40, 8) for j in range(2, 40, 8) for k in range(2, 24, 8)]
    assert len(pts) == 75
    gt = np.zeros((40, 40, 24), bool)
    for p in pts[:n]:
        gt[p] = True
    pred = np.zeros_like(gt)
    pred[2:4, 2:4, 2:12] = True                                    # touches the first two lesions
    pred[34, 34, 18] = True                                        # the last lattice point: a false positive unless n = 75
    return LW.labels_from_mask(pred), LW.labels_from_mask(gt)


def test_cap_64_on_the_device_65_through_the_host_patch(hip):
    import predict_overlap as po
    (s64, t64), (s65, t65) = _lattice(64), _lattice(65)
    seg = torch.from_numpy(np.stack([s65, s64])).to(DEV)
    tgt = torch.from_numpy(np.stack([t65, t64])).to(DEV)
    summary, counts, overflow, table, lesion_hd95 = hip.lesionwise(hip.region_bits(seg), hip.region_bits(tgt), 3, 3, 0, 374.0)
    assert overflow.dtype == torch.int32 and overflow.cpu().tolist() == [[1, 1, 1], [0, 0, 0]]
    for t in (summary, counts, table, lesion_hd95):                # an overflowing entry is left as the wrapper allocated it
        assert not bool(t[0].any())
    ref65 = LW.lesionwise(s65 > 0, t65 > 0, min_lesion_voxels=0)
    ref64 = LW.lesionwise(s64 > 0, t64 > 0, min_lesion_voxels=0)
    assert ref65["counts"][0] == 65 and ref64["counts"][0] == 64 and ref64["counts"][3] == 1
    out = po.lesionwise_metrics(seg, tgt, min_lesion_voxels=0, with_table=True)
    out = {k: v.cpu() for k, v in out.items()}
    assert tuple(out["table"].shape) == (2, 3, 65, 4)
    for r in range(3):
        _assert_equals_restatement(out, 0, r, ref65, ("65 lesions", r))
        _assert_equals_restatement(out, 1, r, ref64, ("64 lesions", r))
    assert torch.equal(out["table"][1, :, :64], table[1].cpu()) and torch.equal(out["counts"][1], counts[1].cpu())


# ------------------------------------------------------------------ batch isolation, determinism
def test_batch_isolation_and_determinism(hip):
    seg, tgt, kw, _ = _case("nested 32x48x40 B2")
    a = _device(seg, tgt, **kw)
    b = _device(seg, tgt, **kw)
    assert all(torch.equal(a[k], b[k]) for k in a)
    seg2, tgt2 = seg.copy(), tgt.copy()
    seg2[1] = np.roll(seg[1], 5, axis=1)
    tgt2[1] = 0
    c = _device(seg2, tgt2, **kw)
    assert all(torch.equal(a[k][0], c[k][0]) for k in a)
    assert not torch.equal(a["counts"][1], c["counts"][1])
    alone = _device(seg[:1], tgt[:1], **kw)
    assert all(torch.equal(a[k][0], alone[k][0]) for k in a)


# ------------------------------------------------------------------ refusals
def test_refusals(hip):
    import predict_overlap as po
    BADARG, TOOLARGE, ALIGN = -1, -2, -3
    shape = (6, 7, 9)
    bits = torch.zeros((1,) + shape, dtype=torch.uint8, device=DEV)
    other = torch.zeros_like(bits)
    nbytes = hip.lib.cwf_lesionwise_workspace(1, 3, *shape)
    assert nbytes > 0 and nbytes % 256 == 0
    ws = torch.empty(nbytes + 256, dtype=torch.uint8, device=DEV)
    summary = torch.zeros((1, 3, 2), dtype=torch.float64, device=DEV)
    counts = torch.zeros((1, 3, 6), dtype=torch.int64, device=DEV)
    overflow = torch.zeros((1, 3), dtype=torch.int32, device=DEV)
    table = torch.zeros((1, 3, 64, 4), dtype=torch.int64, device=DEV)
    lhd = torch.zeros((1, 3, 64), dtype=torch.float64, device=DEV)
    st = hip._stream()
    good = dict(pred=bits.data_ptr(), gt=other.data_ptr(), B=1, R=3, D0=shape[0], D1=shape[1], D2=shape[2], dilation=3, min_lesion=50,
                penalty=374.0, summary=summary.data_ptr(), counts=counts.data_ptr(), overflow=overflow.data_ptr(), table=table.data_ptr(),
                lhd=lhd.data_ptr(), ws=ws.data_ptr(), ws_bytes=nbytes, stream=st)

    def call(**kw):
        return hip.lib.cwf_lesionwise(*{**good, **kw}.values())

    assert call() == 0
    for k in ("pred", "gt", "summary", "counts", "overflow", "table", "lhd", "ws"):
        assert call(**{k: None}) == BADARG, k
    for kw in (dict(R=9), dict(R=0), dict(B=0), dict(D1=0), dict(dilation=-1), dict(dilation=9), dict(min_lesion=-1), dict(penalty=-1.0),
               dict(penalty=float("nan")), dict(penalty=float("inf"))):
        assert call(**kw) == BADARG, kw
    assert call(D0=2048, D1=1024, D2=1024) == TOOLARGE
    assert call(ws_bytes=nbytes - 1) == TOOLARGE
    assert call(ws=ws.data_ptr() + 1) == ALIGN
    assert hip.lib.cwf_lesionwise_workspace(1, 9, *shape) == BADARG
    assert hip.lib.cwf_lesionwise_workspace(1, 3, 2048, 1024, 1024) == TOOLARGE
    torch.cuda.synchronize()
    assert not bool(summary[..., 1].any()) and bool((summary[..., 0] == 1).all())      # only the good call wrote: both masks empty

    def dilate(**kw):
        a = dict(bits=bits.data_ptr(), out=other.data_ptr(), B=1, D0=shape[0], D1=shape[1], D2=shape[2], conn=2, it=3, ws=ws.data_ptr(),
                 ws_bytes=bits.numel(), stream=st)
        return hip.lib.cwf_dilate_bits(*{**a, **kw}.values())

    assert dilate() == 0 and dilate(it=1, ws=None, ws_bytes=0) == 0
    for kw in (dict(bits=None), dict(out=None), dict(out=bits.data_ptr()), dict(conn=0), dict(conn=4), dict(it=-1), dict(it=9), dict(B=0),
               dict(D2=0), dict(ws=None), dict(ws=other.data_ptr())):
        assert dilate(**kw) == BADARG, kw
    assert dilate(ws_bytes=bits.numel() - 1) == TOOLARGE and dilate(D0=2048, D1=1024, D2=1024) == TOOLARGE
    torch.cuda.synchronize()

    for kw in (dict(R=0), dict(R=9), dict(dilation=-1), dict(dilation=9), dict(min_lesion_voxels=-1), dict(penalty=-2.0)):
        with pytest.raises(ValueError):
            hip.lesionwise(bits, other, **{**dict(R=3), **kw})
    for bad in (bits[0], bits.cpu(), bits.int(), torch.zeros((1, 6, 7, 8), dtype=torch.uint8, device=DEV)):
        with pytest.raises(ValueError):
            hip.lesionwise(bad, bits, 3)
        with pytest.raises(ValueError):
            hip.lesionwise(bits, bad, 3)
    for kw in (dict(connectivity=0), dict(connectivity=4), dict(iterations=-1), dict(iterations=9)):
        with pytest.raises(ValueError):
            hip.dilate_bits(bits, **kw)
    with pytest.raises(ValueError):
        hip.dilate_bits(bits.cpu())
    seg = torch.zeros((1,) + shape, dtype=torch.int64, device=DEV)
    for kw in (dict(dilation=9), dict(min_lesion_voxels=-1), dict(penalty=-1.0)):
        with pytest.raises(ValueError):
            po.lesionwise_metrics(seg, seg, **kw)


# ------------------------------------------------------------------ end to end
def test_validate_softmax_lesionwise_end_to_end(hip):
    import predict_overlap as po
    from models.clswiseformer.cls_wise_former import get_cls_wise_former
    from oracle import reference_model as rm
    from utils import synthetic as syn
    m = get_cls_wise_former(dataset="brats", _conv_repr=True, _pe_type="fixed")
    m.load_state_dict(syn.det_state_dict(rm.param_shapes()), strict=False)
    m.Unet_list.InitConv.dropout = 0.0
    m = m.to(DEV).eval()
    shape = (144, 160, 120)
    x = torch.randn((1, 4) + shape, generator=torch.Generator().manual_seed(8)).to(DEV)
    target = torch.from_numpy(H.nested_labels(shape, np.random.default_rng(4))[None]).to(DEV)
    win = {"roi_size": (128, 128, 128), "overlap": 0.5}
    pol = dict(min_component=20, keep_largest=True)
    res = po.validate_softmax(x, target, m, window=win, with_hd95=True, postprocess=pol, lesionwise=True)
    assert len(res) == 5 and isinstance(res[4], dict) and set(res[4]) == {"dice", "hd95", "counts"}
    want = po.lesionwise_metrics(res[0], target)
    assert all(torch.equal(res[4][k], want[k]) for k in want)
    assert tuple(res[4]["dice"].shape) == (1, 3) and res[4]["dice"].dtype == torch.float64 and res[4]["dice"].is_cuda
    kw = dict(dilation=1, min_lesion_voxels=0, with_table=True)
    res2 = po.validate_softmax(x, target, m, window=win, postprocess=pol, lesionwise=kw)
    assert len(res2) == 4 and torch.equal(res2[0], res[0])
    want2 = po.lesionwise_metrics(res2[0], target, **kw)
    assert set(res2[3]) == set(want2) and all(torch.equal(res2[3][k], want2[k]) for k in want2)
