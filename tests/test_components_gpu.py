"""Device connected-component labelling and label-map post-processing (csrc/components.hip through backend().components,
backend().postprocess_labels and predict_overlap.postprocess) against the restatement of tests/components_ref.py (scipy.ndimage.label and
the numpy policy).  Everything is integer: all comparisons are bit equality."""
import numpy as np
import pytest
import torch

import components_ref as C
import hausdorff_ref as H

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TILE = (16, 16, 32)                                           # CC_T0, CC_T1, CC_T2 of csrc/components.hip
SHAPES = [(23, 31, 17), (1, 40, 40), (40, 1, 1), (64, 48, 40), (TILE[0] + 1, 2 * TILE[1] - 1, TILE[2] + 1)]
FULL = (240, 240, 155)


def _diagonal_blobs(shape, corner):
    """Two 3 x 3 x 3 (the third side clipped to the volume) blobs that touch along an edge (corner=False) or at a corner only (corner=True); None where the
    volume has no room for them."""
    need = [8, 8, 8 if corner else 1]
    axes = sorted(range(3), key=lambda a: -shape[a])          # the two (three) longest axes carry the diagonal
    if any(shape[a] < n for a, n in zip(axes, need)):
        return None
    m = np.zeros(shape, bool)
    lo = [0, 0, 0]
    for a, n in zip(axes, need):
        lo[a] = 2 if n == 8 else 0
    a_sl = [slice(lo[a], lo[a] + 3) for a in range(3)]
    b_sl = list(a_sl)
    for a in axes[:3 if corner else 2]:
        b_sl[a] = slice(lo[a] + 3, lo[a] + 6)
    m[tuple(a_sl)] = True
    m[tuple(b_sl)] = True
    return m


def _masks(shape, rng):
    yield "empty", np.zeros(shape, bool)
    yield "full", np.ones(shape, bool)
    m = np.zeros(shape, bool); m[tuple(int(rng.integers(0, s)) for s in shape)] = True
    yield "single voxel", m
    m = np.zeros(shape, bool); m[0, 0, 0] = m[-1, -1, -1] = True
    yield "opposite corners", m
    for p in (0.05, 0.31, 0.6):
        yield "random %.2f" % p, rng.random(shape) < p
    yield "blobs", H.blobs(shape, 5, rng, rmin=1.5, rmax=5.0)
    yield "serpentine", C.serpentine(shape)
    yield "checkerboard", C.checkerboard(shape)
    for corner in (False, True):
        m = _diagonal_blobs(shape, corner)
        if m is not None:
            yield "diagonal blobs, %s" % ("corner" if corner else "edge"), m


def _pack(masks):
    bits = np.zeros(masks[0].shape, dtype=np.uint8)
    for r, m in enumerate(masks):
        bits |= m.astype(np.uint8) << r
    return bits


def _components(hip, bits, R, connectivity):
    """bits [B, D0, D1, D2] uint8 (numpy) -> numpy labels, sizes, count, largest"""
    out = hip.components(torch.from_numpy(np.ascontiguousarray(bits)).to(DEV), R, connectivity)
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in out]


def _assert_equal_to_restatement(got, b, r, mask, connectivity, what):
    labels, sizes, count, largest = got
    lab, k = C.label(mask, connectivity)
    size = C.sizes(lab, k)
    assert labels.dtype == np.int32 and sizes.dtype == np.int32 and count.dtype == np.int32 and largest.dtype == np.int32
    assert int(count[b, r]) == k, (what, int(count[b, r]), k)
    assert np.array_equal(labels[b, r], lab), what
    assert sizes.shape[-1] == (mask.size + 1) // 2 and np.array_equal(sizes[b, r], size), what      # the tail beyond K is zero too
    assert tuple(int(v) for v in largest[b, r]) == C.largest(size), what
    return k


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("connectivity", [1, 2, 3])
def test_components_bit_equal_to_restatement(hip, shape, connectivity):
    rng = np.random.default_rng(1000 * connectivity + sum(shape))
    cases = list(_masks(shape, rng))
    ks = {}
    for g0 in range(0, len(cases), 8):                        # up to eight masks share one call as the bits of a byte
        group = cases[g0:g0 + 8]
        got = _components(hip, _pack([m for _, m in group])[None], len(group), connectivity)
        for r, (name, m) in enumerate(group):
            ks[name] = _assert_equal_to_restatement(got, 0, r, m, connectivity, (name, shape, connectivity))
    v = int(np.prod(shape))
    assert ks["empty"] == 0 and ks["full"] == 1 and ks["single voxel"] == 1 and ks["serpentine"] == 1
    assert ks["opposite corners"] == 2
    if connectivity == 1 or sum(s > 1 for s in shape) >= 2:   # along a single line the checkerboard's voxels never touch
        assert ks["checkerboard"] == ((v + 1) // 2 if connectivity == 1 else 1)
    if "diagonal blobs, edge" in ks:
        assert ks["diagonal blobs, edge"] == (2 if connectivity == 1 else 1)
    if "diagonal blobs, corner" in ks:
        assert ks["diagonal blobs, corner"] == (1 if connectivity == 3 else 2)


def test_batch_and_region_isolation(hip):
    shape = (19, 18, 37)
    rng = np.random.default_rng(77)
    masks = [[np.zeros(shape, bool), rng.random(shape) < 0.31, rng.random(shape) < 0.5],
             [H.blobs(shape, 4, rng), C.serpentine(shape), rng.random(shape) < 0.1]]
    # the end of one row and the start of the next are neighbours in the linear index only
    masks[0][0][3, 4, -1] = True; masks[0][0][3, 5, 0] = True
    # the last voxel of sample 0 and the first of sample 1, of region r and of region r + 1
    for b in range(2):
        for r in range(3):
            masks[b][r][0, 0, 0] = True; masks[b][r][-1, -1, -1] = True
    bits = np.stack([_pack(masks[b]) for b in range(2)])
    for connectivity in (1, 2, 3):
        got = _components(hip, bits, 3, connectivity)
        for b in range(2):
            for r in range(3):
                _assert_equal_to_restatement(got, b, r, masks[b][r], connectivity, (b, r, connectivity))
                single = _components(hip, masks[b][r].astype(np.uint8)[None], 1, connectivity)
                for full, one in zip(got, single):
                    assert np.array_equal(full[b, r], one[0, 0]), (b, r, connectivity)
        lab = got[0][0, 0]
        assert lab[3, 4, -1] != lab[3, 5, 0] and lab[3, 4, -1] > 0 and lab[3, 5, 0] > 0


def _noisy_full(rng, n_noise=4000):
    lab = H.nested_labels(FULL, rng)
    idx = rng.integers(0, lab.size, size=n_noise)
    lab.ravel()[idx] = rng.integers(1, 4, size=n_noise)
    return lab


def test_full_size_label_map_all_connectivities(hip):
    rng = np.random.default_rng(31)
    seg = _noisy_full(rng)
    bits = hip.region_bits(torch.from_numpy(seg[None]).to(DEV))
    for connectivity in (1, 2, 3):
        out = hip.components(bits, 3, connectivity)
        torch.cuda.synchronize()
        got = [t.cpu().numpy() for t in out]
        for r, m in enumerate(H.regions(seg)):
            k = _assert_equal_to_restatement(got, 0, r, m, connectivity, (r, connectivity))
            assert k > 1


def test_two_runs_are_bit_identical(hip):
    rng = np.random.default_rng(8)
    shape = (70, 50, 67)
    bits = torch.from_numpy(_pack([rng.random(shape) < 0.31, rng.random(shape) < 0.6, C.serpentine(shape)])[None].repeat(2, axis=0)).to(DEV)
    a = hip.components(bits, 3, 2)
    b = hip.components(bits, 3, 2)
    torch.cuda.synchronize()
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    for x in a:                                               # and the two samples hold the same masks
        assert torch.equal(x[0], x[1])


def _policies(po, small):
    s = 1 if small else 8
    return [dict(min_component=3 * s), dict(keep_largest=True), dict(et_min_component=2 * s, et_replace=2), dict(et_min_voxels=500),
            dict(et_min_voxels=10 ** 9, et_replace=0), dict(min_component=2 * s, keep_largest=True, et_min_component=2, et_min_voxels=60 * s),
            po.REFERENCE_POSTPROCESS, dict()]


@pytest.mark.parametrize("size", ["odd", "full"])
def test_postprocess_on_cuda_equals_restatement(hip, size):
    import predict_overlap as po
    rng = np.random.default_rng(5 if size == "odd" else 6)
    if size == "odd":
        shape = (23, 31, 37)
        seg = np.stack([H.nested_labels(shape, rng, scale=0.35) for _ in range(2)])
        idx = rng.integers(0, seg.size, size=300)
        seg.ravel()[idx] = rng.integers(1, 4, size=300)
    else:
        seg = _noisy_full(rng)[None]
    t = torch.from_numpy(seg).to(DEV)
    for connectivity in ((1, 2, 3) if size == "odd" else (1,)):
        for pol in _policies(po, size == "odd"):
            want, wstats = C.postprocess(seg, connectivity=connectivity, **pol)
            got, stats = po.postprocess(t, connectivity=connectivity, with_stats=True, **pol)
            assert got.dtype == torch.int64 and got.is_cuda and stats.dtype == torch.int64 and tuple(stats.shape) == (seg.shape[0], 4)
            assert np.array_equal(stats.cpu().numpy(), wstats), (pol, connectivity, stats.cpu().numpy().tolist(), wstats.tolist())
            assert np.array_equal(got.cpu().numpy(), want), (pol, connectivity)
    assert np.array_equal(t.cpu().numpy(), seg)               # the input is left alone


def test_postprocess_does_not_synchronise_with_the_host(hip):
    import predict_overlap as po
    rng = np.random.default_rng(12)
    seg = torch.from_numpy(H.nested_labels((40, 48, 56), rng, scale=0.5)[None]).to(DEV)
    pol = dict(min_component=10, keep_largest=True, et_min_component=3, et_min_voxels=500)
    want = po.postprocess(seg, **pol)                         # code objects loaded, allocator warm
    torch.cuda.synchronize()
    old = torch.cuda.get_sync_debug_mode()
    try:
        torch.cuda.set_sync_debug_mode("error")
        try:
            torch.ones(1, device=DEV).item()                  # a synchronising call: the mode must object
            implemented = False
        except RuntimeError:
            implemented = True
        if implemented:
            got, stats = po.postprocess(seg, with_stats=True, **pol)
    finally:
        torch.cuda.set_sync_debug_mode(old)
    if not implemented:
        pytest.skip("this torch build does not raise on synchronising calls under set_sync_debug_mode('error') on ROCm")
    assert torch.equal(got, want)


def test_validate_softmax_postprocess_end_to_end(hip):
    import predict_overlap as po
    from models.clswiseformer.cls_wise_former import get_cls_wise_former
    from oracle import reference_model as rm
    from utils import synthetic as syn
    from utils import tools
    m = get_cls_wise_former(dataset="brats", _conv_repr=True, _pe_type="fixed")
    m.load_state_dict(syn.det_state_dict(rm.param_shapes()), strict=False)
    m.Unet_list.InitConv.dropout = 0.0
    m = m.to(DEV).eval()
    shape = (144, 160, 120)
    x = torch.randn((1, 4) + shape, generator=torch.Generator().manual_seed(8)).to(DEV)
    target = torch.from_numpy(H.nested_labels(shape, np.random.default_rng(4))[None]).to(DEV)
    win = {"roi_size": (128, 128, 128), "overlap": 0.5}
    plain = po.validate_softmax(x, target, m, window=win, with_miou=True, with_hd95=True)
    none = po.validate_softmax(x, target, m, window=win, with_miou=True, with_hd95=True, postprocess=None)
    assert len(plain) == len(none) == 5
    assert torch.equal(plain[0], none[0]) and torch.equal(plain[1], none[1]) and torch.equal(plain[4], none[4])
    assert [float(v) for v in plain[2]] == [float(v) for v in none[2]] and [float(v) for v in plain[3]] == [float(v) for v in none[3]]
    pol = dict(min_component=20, keep_largest=True, et_min_component=4, et_min_voxels=500, et_replace=1)
    seg, prob, dice, miou, hd95 = po.validate_softmax(x, target, m, window=win, with_miou=True, with_hd95=True, postprocess=pol)
    assert torch.equal(prob, plain[1])
    want, _ = C.postprocess(plain[0].cpu().numpy(), **pol)
    assert np.array_equal(seg.cpu().numpy(), want)
    s, t = seg.cpu().numpy(), target.cpu().numpy()
    assert [float(v) for v in dice] == [float(v) for v in tools.softmax_output_dice(s, t)]
    assert [float(v) for v in miou] == [float(v) for v in tools.softmax_mIOU_score(s, t)]
    assert torch.equal(hd95, po.hd95_regions(seg, target))
    res = po.validate_softmax(x, target, m, window=win, postprocess=pol)
    assert len(res) == 3 and torch.equal(res[0], seg) and [float(v) for v in res[2]] == [float(v) for v in dice]
