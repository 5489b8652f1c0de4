"""Device normalised surface Dice and average surface distance (csrc/metrics.hip: cwf_surface_metrics; csrc/lesions.hip:
cwf_lesionwise_ex) through backend().surface_metrics, backend().lesionwise(nsd_tolerances=...), predict_overlap.surface_regions /
lesionwise_metrics / validate_softmax(with_nsd=...) and the utils.hausdorff drop-ins, against the float64 restatement of
tests/surface_ref.py.  within, counts and nsd are integers and one division: bit-equal.  hd and hd95 are bit-equal to
backend().hausdorff on the same input.  asd and assd lie within 2 n 2^-53 relative of the correctly rounded mean (n = border voxels of
that direction): the worst case of any-order float64 summation of n non-negative terms plus the final division."""
import functools
import math

import numpy as np
import pytest
import torch

import hausdorff_ref as H
import lesionwise_ref as LW
import surface_ref as S

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SHAPES = [(1, 1, 1), (5, 6, 7), (17, 9, 70), (33, 34, 65)]
MODES = {"conn1": dict(connectivity=1), "conn2": dict(connectivity=2), "conn3": dict(connectivity=3), "all_border": dict(all_border=True)}
TAUS = (0.5, 1.0, 1.5, 3.0)
FLOATS = ("hd", "hd95", "asd", "assd", "nsd")


# ------------------------------------------------------------------ inputs and the shared reference
def _labels(shape, seed):
    """Two different BraTS-like label maps (prediction, target) of one shape: nested blobs around two jittered centres along axis 2
    (the second beyond lane 64 where the axis is that long) plus a few loose WT blobs; noise for the tiny shapes."""
    rng = np.random.default_rng(seed)
    if min(shape) < 9:
        return [rng.choice(4, size=shape, p=[0.5, 0.15, 0.2, 0.15]).astype(np.int64) for _ in range(2)]
    out = []
    for _ in range(2):
        centers = [[shape[0] * 0.5 + rng.uniform(-1.5, 1.5), shape[1] * 0.5 + rng.uniform(-1.5, 1.5), shape[2] * f + rng.uniform(-1.5, 1.5)]
                   for f in (0.25, 0.85)]
        lab = H.nested_labels(shape, rng, centers=centers, scale=min(shape[:2]) / 45.0)
        lab[H.blobs(shape, 2, rng, 1.5, 3.0) & (lab == 0)] = 2
        out.append(lab)
    return out


def _bits(labels):
    return sum(m.astype(np.uint8) << r for r, m in enumerate(H.regions(labels)))


@functools.lru_cache(maxsize=None)
def _batch(shape):
    """(a_bits, b_bits [2, ...] uint8, [(seg, tgt)] * 2): B = 2 with different samples; (1, 1, 1): the second target has no ET."""
    if shape == (1, 1, 1):
        pairs = [(np.full(shape, 3, np.int64), np.full(shape, 3, np.int64)), (np.full(shape, 3, np.int64), np.full(shape, 1, np.int64))]
    else:
        pairs = [tuple(_labels(shape, 100 + i)) for i in range(2)]
    return np.stack([_bits(p[0]) for p in pairs]), np.stack([_bits(p[1]) for p in pairs]), pairs


@functools.lru_cache(maxsize=None)
def _reference(shape, mode, taus=TAUS, spacing=None):
    """ref[b][r] of S.surface for the batch of `shape`: computed once and shared.  Brute force over the border voxels for the small
    shapes, scipy's transform for (33, 34, 65) (tests/test_surface_ref_cpu.py holds the two bit-equal)."""
    _, _, pairs = _batch(shape)
    big = shape[0] * shape[1] * shape[2] > 20000
    return [[S.surface(o, g, taus, spacing, use_scipy=big, **MODES[mode]) for o, g in zip(H.regions(s), H.regions(t))] for s, t in pairs]


def _run(hip, a, b, R=3, taus=TAUS, **kw):
    out = hip.surface_metrics(torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV), R, taus, **kw)
    torch.cuda.synchronize()
    assert set(out) == {"hd", "hd95", "asd", "assd", "nsd", "within", "counts"}
    assert all(out[k].dtype == torch.float64 for k in FLOATS) and out["within"].dtype == torch.int64 and out["counts"].dtype == torch.int64
    return {k: v.cpu() for k, v in out.items()}


def _same_bits(x, y):
    """Bit-equality of float64 tensors (NaN equals NaN)."""
    return torch.equal(x.contiguous().view(torch.int64), y.contiguous().view(torch.int64))


def _assert_equals_reference(out, b, r, ref, what):
    nt = len(ref["nsd"])
    print(what, "counts", out["counts"][b, r].tolist(), "within", out["within"][b, r].tolist(), "nsd", out["nsd"][b, r].tolist(), ref["nsd"],
          "asd", out["asd"][b, r].tolist(), ref["asd"], "assd %.17g %.17g" % (float(out["assd"][b, r]), ref["assd"]))
    assert tuple(out["counts"][b, r].tolist()) == ref["counts"], what
    assert out["within"][b, r].tolist() == ref["within"], what
    if ref["counts"][0] == 0 or ref["counts"][1] == 0:
        assert all(bool(torch.isnan(out[k][b, r]).all()) for k in FLOATS), what
        assert not bool(out["within"][b, r].any()), what
        return
    assert out["nsd"][b, r].tolist() == ref["nsd"] and tuple(out["nsd"][b, r].shape) == (nt,), what
    for d in range(2):
        got, want = float(out["asd"][b, r, d]), ref["asd"][d]
        assert abs(got - want) <= S.asd_bound(ref["counts"][2 + d], want), (what, d, got, want)
    n = max(ref["counts"][2], ref["counts"][3])
    assert abs(float(out["assd"][b, r]) - ref["assd"]) <= S.asd_bound(n, ref["assd"]), what


# ------------------------------------------------------------------ blob masks, every connectivity and all-border
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_blobs_equal_restatement(hip, shape, mode):
    a, b, _ = _batch(shape)
    out = _run(hip, a, b, **MODES[mode])
    ref = _reference(shape, mode)
    assert tuple(out["nsd"].shape) == (2, 3, 4) and tuple(out["within"].shape) == (2, 3, 4, 2) and tuple(out["asd"].shape) == (2, 3, 2)
    for s in range(2):
        for r in range(3):
            _assert_equals_reference(out, s, r, ref[s][r], (shape, mode, s, r))
    hd, hd95, counts = hip.hausdorff(torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV), 3, **MODES[mode])
    assert _same_bits(out["hd"], hd.cpu()) and _same_bits(out["hd95"], hd95.cpu()) and torch.equal(out["counts"], counts.cpu())


def test_blob_cases_are_not_vacuous():
    """The shapes above hold what they are there for: borders beyond lane 64 of axis 2, partial NSD values, an empty region."""
    for shape in SHAPES[2:]:
        _, _, pairs = _batch(shape)
        for s, t in pairs:
            assert H.border(s > 0)[:, :, 64:].any() and H.border(t > 0)[:, :, 64:].any(), shape
        ref = _reference(shape, "conn1")
        vals = [v for row in ref for x in row for v in x["nsd"] if not math.isnan(v)]
        assert any(0.0 < v < 1.0 for v in vals) and len(set(vals)) > 4, shape
        assert all(x["counts"][0] > 0 and x["counts"][1] > 0 for row in ref for x in row), shape
    ref = _reference((1, 1, 1), "conn1")
    assert ref[0][2]["nsd"] == [1.0] * 4 and ref[1][2]["counts"] == (1, 0, 1, 0) and math.isnan(ref[1][2]["assd"])


# ------------------------------------------------------------------ tolerances that border voxels sit exactly on
UNIT_TAUS = (0.0, 0.5, 1.0, math.sqrt(2.0), 2.0, math.inf)


@pytest.mark.parametrize("spacing,taus", [(None, UNIT_TAUS[:3]), (None, UNIT_TAUS[3:]), ((1.0, 1.0, 2.5), (2.5,))],
                         ids=["unit 0 0.5 1", "unit sqrt2 2 inf", "1x1x2.5 2.5"])
def test_tolerance_ties(hip, spacing, taus):
    shape = (17, 9, 70)
    a, b, pairs = _batch(shape)
    for tau in taus:                                  # on the reference alone: border voxels lie at exactly tau, so <= is exercised
        if tau in (0.0, math.inf):
            continue
        at = _reference(shape, "conn1", (tau,), spacing)
        below = _reference(shape, "conn1", (math.nextafter(tau, 0.0),), spacing)
        tied = [x["within"][0] != y["within"][0] for rx, ry in zip(at, below) for x, y in zip(rx, ry)]
        if tau == 0.5:                                # unit spacing: d is 0 or >= 1, no voxel can sit at 0.5; it counts what 0 counts
            zero = _reference(shape, "conn1", (0.0,), spacing)
            assert not any(tied) and all(x["within"] == y["within"] for rx, ry in zip(at, zero) for x, y in zip(rx, ry))
        else:
            assert any(tied), tau
    out = _run(hip, a, b, taus=taus, spacing=spacing)
    ref = _reference(shape, "conn1", taus, spacing)
    for s in range(2):
        for r in range(3):
            _assert_equals_reference(out, s, r, ref[s][r], (spacing, taus, s, r))
            if math.inf in taus:
                assert out["within"][s, r, taus.index(math.inf)].tolist() == list(ref[s][r]["counts"][2:])
                assert float(out["nsd"][s, r, taus.index(math.inf)]) == 1.0


# ------------------------------------------------------------------ empty masks
def test_empty_masks_give_nan_for_that_entry_only(hip):
    shape = (17, 9, 70)
    a, b, pairs = _batch(shape)
    a, b = a.copy(), b.copy()
    a[0] &= ~np.uint8(4)                              # sample 0: ET empty in A
    b[0] &= ~np.uint8(2)                              #           TC empty in B
    a[1] &= ~np.uint8(4); b[1] &= ~np.uint8(4)        # sample 1: ET empty in both
    out = _run(hip, a, b, taus=(1.0, math.inf))
    full = _reference(shape, "conn1", (1.0, math.inf))
    for s, r in ((0, 2), (0, 1), (1, 2)):
        assert all(bool(torch.isnan(out[k][s, r]).all()) for k in FLOATS), (s, r)
        assert not bool(out["within"][s, r].any()), (s, r)
    assert out["counts"][0, 2, 0] == 0 and out["counts"][0, 1, 1] == 0 and out["counts"][1, 2].tolist() == [0, 0, 0, 0]
    assert out["counts"][0, 2, 1] > 0 and out["counts"][0, 1, 0] > 0
    for s, r in ((0, 0), (1, 0), (1, 1)):
        _assert_equals_reference(out, s, r, full[s][r], ("untouched", s, r))


# ------------------------------------------------------------------ determinism
def test_two_calls_and_two_batch_positions_are_bit_identical(hip):
    a, b, _ = _batch((33, 34, 65))
    x, y = _run(hip, a, b), _run(hip, a, b)
    for k in x:
        assert _same_bits(x[k], y[k]) if k in FLOATS else torch.equal(x[k], y[k]), k
    alone = _run(hip, a[:1], b[:1])
    second = _run(hip, np.stack([a[1], a[0]]), np.stack([b[1], b[0]]))
    for k in x:
        eq = _same_bits if k in FLOATS else torch.equal
        assert eq(alone[k][0], x[k][0]) and eq(second[k][1], x[k][0]) and eq(second[k][0], x[k][1]), k
    one = _run(hip, a & 1, b & 1, R=1)              # and on its own as the only region of a call
    for k in x:
        eq = _same_bits if k in FLOATS else torch.equal
        assert eq(one[k][:, 0], x[k][:, 0]), k


# ------------------------------------------------------------------ graph capture
def test_call_captures_into_a_graph(hip):
    a, b, _ = _batch((17, 9, 70))
    ta, tb = torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV)
    eager = {k: v.clone() for k, v in hip.surface_metrics(ta, tb, 3, TAUS).items()}
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        hip.surface_metrics(ta, tb, 3, TAUS)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = hip.surface_metrics(ta, tb, 3, TAUS)
    for _ in range(2):
        for v in out.values():
            v.fill_(-1)
        g.replay()
        torch.cuda.synchronize()
        for k in out:
            assert _same_bits(out[k], eager[k]) if k in FLOATS else torch.equal(out[k], eager[k]), k


# ------------------------------------------------------------------ refusals
def test_refusals(hip):
    BADARG, TOOLARGE, ALIGN = -1, -2, -3
    shape = (6, 7, 9)
    a = torch.full((1,) + shape, 7, dtype=torch.uint8, device=DEV)     # all three regions full
    b = a.clone()
    nbytes = hip.lib.cwf_surface_metrics_workspace(1, 3, *shape)
    assert nbytes > hip.lib.cwf_hausdorff_workspace(1, 3, *shape) > 0 and nbytes % 256 == 0
    ws = torch.empty(nbytes + 256, dtype=torch.uint8, device=DEV)
    f = {k: torch.zeros(n, dtype=torch.float64, device=DEV) for k, n in (("hd", 3), ("hd95", 3), ("asd", 6), ("assd", 3), ("nsd", 12))}
    within = torch.zeros(24, dtype=torch.int64, device=DEV)
    counts = torch.zeros(12, dtype=torch.int64, device=DEV)
    import ctypes
    tau = (ctypes.c_double * 4)(0.0, 1.0, 2.0, math.inf)
    good = dict(a=a.data_ptr(), b=b.data_ptr(), B=1, R=3, D0=shape[0], D1=shape[1], D2=shape[2], s0=1.0, s1=1.0, s2=1.0, conn=1, ab=0, tau=tau,
                T=4, hd=f["hd"].data_ptr(), hd95=f["hd95"].data_ptr(), asd=f["asd"].data_ptr(), assd=f["assd"].data_ptr(),
                within=within.data_ptr(), nsd=f["nsd"].data_ptr(), counts=counts.data_ptr(), ws=ws.data_ptr(), ws_bytes=nbytes,
                stream=hip._stream())

    def call(**kw):
        return hip.lib.cwf_surface_metrics(*{**good, **kw}.values())

    assert call() == 0
    for kw in (dict(T=5), dict(T=-1), dict(tau=(ctypes.c_double * 4)(0.0, -1.0, 2.0, 3.0)), dict(tau=(ctypes.c_double * 4)(0.0, 1.0, math.nan, 3.0)),
               dict(tau=(ctypes.c_double * 4)(-math.inf, 1.0, 2.0, 3.0)), dict(R=0), dict(R=9), dict(B=0), dict(D2=0), dict(conn=0), dict(conn=4),
               dict(s1=0.0), dict(s2=math.nan)):
        assert call(**kw) == BADARG, kw
    for k in ("a", "b", "tau", "hd", "hd95", "asd", "assd", "within", "nsd", "counts", "ws"):
        assert call(**{k: None}) == BADARG, k
    assert call(T=0, tau=None, within=None, nsd=None) == 0
    assert call(D2=4097) == TOOLARGE and call(ws_bytes=nbytes - 1) == TOOLARGE and call(ws=ws.data_ptr() + 1) == ALIGN
    assert call(ws_bytes=hip.lib.cwf_hausdorff_workspace(1, 3, *shape)) == TOOLARGE
    assert hip.lib.cwf_surface_metrics_workspace(1, 9, *shape) == BADARG and hip.lib.cwf_surface_metrics_workspace(1, 3, 6, 7, 4097) == TOOLARGE
    torch.cuda.synchronize()
    assert f["nsd"].tolist() == [1.0] * 12 and f["assd"].tolist() == [0.0] * 3        # what the good calls wrote: identical full masks

    for kw in (dict(tolerances=(1.0,) * 5), dict(tolerances=(-1.0,)), dict(tolerances=(math.nan,)), dict(R=0), dict(R=9), dict(connectivity=0),
               dict(connectivity=4), dict(spacing=(1.0, 1.0))):
        with pytest.raises(ValueError):
            hip.surface_metrics(a, b, **{**dict(R=3), **kw})
    for bad in (a[0], a.cpu(), a.int(), torch.ones((1, 6, 7, 8), dtype=torch.uint8, device=DEV)):
        with pytest.raises(ValueError):
            hip.surface_metrics(bad, b, 3)
        with pytest.raises(ValueError):
            hip.surface_metrics(a, bad, 3)
    with pytest.raises(ValueError):
        hip.lesionwise(a, b, 3, nsd_tolerances=(1.0,) * 5)
    with pytest.raises(ValueError):
        hip.lesionwise(a, b, 3, nsd_tolerances=(-1.0,))
    lw_bytes = hip.lib.cwf_lesionwise_ex_workspace(1, 3, *shape)
    assert lw_bytes > hip.lib.cwf_lesionwise_workspace(1, 3, *shape) > 0 and hip.lib.cwf_lesionwise_ex_workspace(1, 9, *shape) == BADARG


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


@pytest.mark.parametrize("case", ["scene", "missed and spurious"])
def test_lesionwise_nsd_equals_restatement(hip, case):
    import predict_overlap as po
    pred, gt = LW.scene() if case == "scene" else _missed_and_spurious()
    kw = dict(min_lesion_voxels=0) if case != "scene" else {}
    ref = LW.lesionwise(pred, gt, **kw)
    assert ref["counts"][3] > 0 and ref["counts"][4] > 0                  # a false positive and a missed lesion
    nsd, lw = S.lesionwise_nsd(pred, gt, (0.5, 1.0), **kw)
    assert ((nsd > 0) & (nsd < 1)).any()
    seg = torch.from_numpy(np.stack([LW.labels_from_mask(pred), LW.labels_from_mask(gt)])).to(DEV)
    tgt = torch.from_numpy(np.stack([LW.labels_from_mask(gt), LW.labels_from_mask(gt)])).to(DEV)
    base = po.lesionwise_metrics(seg, tgt, with_table=True, **kw)
    out = po.lesionwise_metrics(seg, tgt, with_table=True, nsd_tolerances=(0.5, 1.0), **kw)
    assert set(out) == set(base) | {"lw_nsd", "lesion_nsd"} and all(v.is_cuda for v in out.values())
    for k in base:                                    # everything cwf_lesionwise returned is bit-equal with and without the keyword
        assert _same_bits(out[k], base[k]) if out[k].dtype == torch.float64 else torch.equal(out[k], base[k]), k
    assert tuple(out["lw_nsd"].shape) == (2, 3, 2) and tuple(out["lesion_nsd"].shape) == (2, 3, 64, 2)
    g = nsd.shape[0]
    print(case, "lw_nsd", out["lw_nsd"][0].tolist(), lw, "lesion_nsd", out["lesion_nsd"][0, 0, :g].tolist(), nsd.tolist())
    for r in range(3):
        assert out["lw_nsd"][0, r].tolist() == lw and out["lesion_nsd"][0, r, :g].tolist() == nsd.tolist()
        assert not bool(out["lesion_nsd"][0, r, g:].any())
        assert out["lw_nsd"][1, r].tolist() == [1.0, 1.0]                 # sample 1: prediction = target
        assert bool((out["lesion_nsd"][1, r, :g] == 1).all()) and not bool(out["lesion_nsd"][1, r, g:].any())
    short = po.lesionwise_metrics(seg, tgt, nsd_tolerances=(1.0,), **kw)
    assert set(short) == {"dice", "hd95", "counts", "lw_nsd"} and short["lw_nsd"][0, 0].tolist() == [lw[1]]
    raw = hip.lesionwise(hip.region_bits(seg), hip.region_bits(tgt), 3, 3, kw.get("min_lesion_voxels", 50), 374.0)
    assert len(raw) == 5                              # the backend's return shape without tolerances


def test_lesionwise_nsd_65_lesions_through_the_host(hip):
    import predict_overlap as po
    pts = [(i, j, k) for i in range(2, 40, 8) for j in range(2, 40, 8) for k in range(2, 24, 8)]
    gt = np.zeros((40, 40, 24), bool)
    for p in pts[:65]:
        gt[p] = True
    pred = np.zeros_like(gt)
    pred[2:4, 2:4, 2:12] = True
    pred[34, 34, 18] = True
    seg = torch.from_numpy(LW.labels_from_mask(pred)[None]).to(DEV)
    tgt = torch.from_numpy(LW.labels_from_mask(gt)[None]).to(DEV)
    raw = hip.lesionwise(hip.region_bits(seg), hip.region_bits(tgt), 3, 3, 0, 374.0, nsd_tolerances=(0.5, 1.0))
    assert len(raw) == 7 and raw[2].cpu().tolist() == [[1, 1, 1]] and not bool(raw[5].any()) and not bool(raw[6].any())
    out = po.lesionwise_metrics(seg, tgt, min_lesion_voxels=0, with_table=True, nsd_tolerances=(0.5, 1.0))
    nsd, lw = S.lesionwise_nsd(pred, gt, (0.5, 1.0), min_lesion_voxels=0)
    assert nsd.shape == (65, 2) and tuple(out["lesion_nsd"].shape) == (1, 3, 65, 2) and out["lesion_nsd"].is_cuda
    for r in range(3):
        assert out["lw_nsd"][0, r].tolist() == lw and out["lesion_nsd"][0, r].tolist() == nsd.tolist()
    assert tuple(out["counts"][0, 0].tolist()) == LW.lesionwise(pred, gt, min_lesion_voxels=0)["counts"]


# ------------------------------------------------------------------ drop-ins and end to end
def test_drop_in_wrappers_on_device_tensors(hip):
    from utils import hausdorff as uh
    _, _, pairs = _batch((17, 9, 70))
    a, b = pairs[0][0] > 0, pairs[0][1] > 0
    ta, tb = torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV)
    for sp in (None, (1.0, 1.0, 2.5)):
        ref = S.surface(a, b, (1.0,), sp)
        assert uh.normalized_surface_dice(ta, tb, 1.0, voxel_spacing=sp) == ref["nsd"][0]
        got = uh.avg_surface_distance(ta, tb, voxel_spacing=sp), uh.avg_surface_distance(tb, ta, voxel_spacing=sp)
        for d in range(2):
            assert abs(got[d] - ref["asd"][d]) <= S.asd_bound(ref["counts"][2 + d], ref["asd"][d])
        assert abs(uh.avg_surface_distance_symmetric(ta, tb, voxel_spacing=sp) - ref["assd"]) <= S.asd_bound(max(ref["counts"][2:]), ref["assd"])
    ref4 = S.surface(a, b, (2.0,), all_border=True)
    assert uh.normalized_surface_dice(ta[None], tb[None], 2.0) == ref4["nsd"][0]
    e = torch.zeros_like(ta)
    assert uh.normalized_surface_dice(e, tb, 1.0) == 0.0 and math.isnan(uh.avg_surface_distance_symmetric(ta, e, nan_for_nonexisting=True))


def test_validate_softmax_with_nsd_end_to_end(hip):
    import predict_overlap as po
    from models.clswiseformer.cls_wise_former import get_cls_wise_former
    from oracle import reference_model as rm
    from utils import synthetic as syn
    m = get_cls_wise_former(dataset="brats", _conv_repr=True, _pe_type="fixed")
    m.load_state_dict(syn.det_state_dict(rm.param_shapes()), strict=False)
    m.Unet_list.InitConv.dropout = 0.0
    m = m.to(DEV).eval()
    shape = (128, 128, 128)
    x = torch.randn((1, 4) + shape, generator=torch.Generator().manual_seed(8)).to(DEV)
    target = torch.from_numpy(H.nested_labels(shape, np.random.default_rng(4))[None]).to(DEV)
    win = {"roi_size": (128, 128, 128), "overlap": 0.5}
    pol = dict(min_component=20, keep_largest=True)
    base = po.validate_softmax(x, target, m, window=win, with_hd95=True, postprocess=pol, with_nsd=None)
    plain = po.validate_softmax(x, target, m, window=win, with_hd95=True, postprocess=pol)
    assert len(base) == len(plain) == 4 and torch.equal(base[0], plain[0]) and _same_bits(base[3], plain[3])
    res = po.validate_softmax(x, target, m, window=win, with_hd95=True, postprocess=pol, with_nsd=(1.0,))
    assert len(res) == 5 and torch.equal(res[0], base[0]) and _same_bits(res[3], base[3])
    want = po.surface_regions(res[0], target, (1.0,))
    assert set(res[4]) == {"nsd", "assd"} and tuple(res[4]["nsd"].shape) == (1, 3, 1) and res[4]["nsd"].is_cuda
    assert _same_bits(res[4]["nsd"], want["nsd"]) and _same_bits(res[4]["assd"], want["assd"])
    seg, tgt = res[0][0].cpu().numpy(), target[0].cpu().numpy()
    for r, (o, g) in enumerate(zip(H.regions(seg), H.regions(tgt))):
        if o.any() and g.any():
            ref = S.surface(o, g, (1.0,), use_scipy=True)
            assert float(res[4]["nsd"][0, r, 0]) == ref["nsd"][0]
        else:
            assert math.isnan(float(res[4]["nsd"][0, r, 0]))
    assert po.validate_softmax(x, None, m, window=win, with_nsd=(1.0,))[-1] is None


# ------------------------------------------------------------------ full size
def test_full_size_case_against_scipy(hip):
    rng = np.random.default_rng(2025)                 # two differently wobbled tumours around nearby centres: their borders cross
    seg = H.nested_labels((240, 240, 155), rng, centers=[[120.0, 115.0, 80.0]])
    tgt = H.nested_labels((240, 240, 155), rng, centers=[[123.0, 117.0, 78.0]])
    taus = (0.5, 1.0, 2.0, 5.0)
    refs = [S.surface(o, g, taus, use_scipy=True) for o, g in zip(H.regions(seg), H.regions(tgt))]
    assert all(0.0 < ref["nsd"][1] < ref["nsd"][3] < 1.0 for ref in refs)         # on the reference alone: the counts are partial
    out = _run(hip, _bits(seg)[None], _bits(tgt)[None], taus=taus)
    for r, ref in enumerate(refs):
        _assert_equals_reference(out, 0, r, ref, ("240x240x155", r))
