"""The restatement of tests/components_ref.py against an independent flood fill, its numbering property, the post-processing policy on
hand-built cases, and the CPU path and argument checks of predict_overlap.postprocess / validate_softmax(postprocess=...)."""
import collections
import itertools

import numpy as np
import pytest
import torch

import components_ref as C
import hausdorff_ref as H

SMALL_SHAPES = [(5, 6, 7), (1, 9, 8), (12, 1, 1), (1, 1, 1), (12, 12, 12), (4, 1, 11)]


def _flood_fill(mask, connectivity):
    """Breadth-first labelling in C order of the first voxel of every component."""
    offs = [o for o in itertools.product((-1, 0, 1), repeat=3) if 0 < sum(c != 0 for c in o) <= connectivity]
    lab = np.zeros(mask.shape, dtype=np.int32)
    k = 0
    for start in zip(*np.nonzero(mask)):                      # np.nonzero walks in C order
        if lab[start]:
            continue
        k += 1
        lab[start] = k
        queue = collections.deque([start])
        while queue:
            v = queue.popleft()
            for o in offs:
                n = tuple(a + b for a, b in zip(v, o))
                if all(0 <= c < s for c, s in zip(n, mask.shape)) and mask[n] and not lab[n]:
                    lab[n] = k
                    queue.append(n)
    return lab, k


@pytest.mark.parametrize("shape", SMALL_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("connectivity", [1, 2, 3])
def test_label_matches_flood_fill_and_numbers_by_first_voxel(shape, connectivity):
    rng = np.random.default_rng(sum(shape) * 10 + connectivity)
    masks = [rng.random(shape) < p for p in (0.1, 0.31, 0.6)] + [np.zeros(shape, bool), np.ones(shape, bool), C.checkerboard(shape),
                                                                 C.serpentine(shape)]
    for m in masks:
        lab, k = C.label(m, connectivity)
        ref, kr = _flood_fill(m, connectivity)
        assert k == kr and np.array_equal(lab, ref)
        first = C.first_indices(lab, k)
        assert np.all(np.diff(first) > 0)
        size = C.sizes(lab, k)
        assert size.shape == ((m.size + 1) // 2,) and size[:k].sum() == m.sum() and not size[k:].any()
        if k:
            assert C.largest(size) == (int(np.argmax(size)) + 1, int(size.max()))
        else:
            assert C.largest(size) == (0, 0)


def test_special_masks_of_the_restatement():
    shape = (6, 5, 7)
    cb = C.checkerboard(shape)
    assert C.label(cb, 1)[1] == (cb.size + 1) // 2 and C.label(cb, 2)[1] == 1 and C.label(cb, 3)[1] == 1
    for shp in [(9, 10, 11), (1, 8, 8), (7, 1, 1), (8, 8, 1)]:
        s = C.serpentine(shp)
        assert s.any() and all(C.label(s, c)[1] == 1 for c in (1, 2, 3)), shp
    m = np.zeros((4, 4, 4), bool)
    m[0, 0, 0] = m[1, 1, 0] = True                            # share an edge
    assert [C.label(m, c)[1] for c in (1, 2, 3)] == [2, 1, 1]
    m = np.zeros((4, 4, 4), bool)
    m[0, 0, 0] = m[1, 1, 1] = True                            # share a corner only
    assert [C.label(m, c)[1] for c in (1, 2, 3)] == [2, 2, 1]


def _seg(shape=(1, 12, 20, 20)):
    return np.zeros(shape, dtype=np.int64)


def test_rule4_threshold_499_and_500():
    for n, kept in ((499, False), (500, True)):
        s = _seg()
        s[0, 1:11, 1:11, 1:11] = 2                            # 1000-voxel WT
        et = np.zeros(1000, bool); et[:n] = True
        s[0, 1:11, 1:11, 1:11][et.reshape(10, 10, 10)] = 3
        out, stats = C.postprocess(s, et_min_voxels=500, et_replace=1)
        assert int((out == 3).sum()) == (n if kept else 0)
        assert int((out == 1).sum()) == (0 if kept else n) and int((out > 0).sum()) == 1000
        assert stats[0].tolist() == [0, 0, 0 if kept else n, n if kept else 0]


def test_rule2_tie_goes_to_lowest_label():
    s = _seg()
    s[0, 2:4, 2:4, 2:4] = 1
    s[0, 8:10, 8:10, 8:10] = 2                                # the same size, later in C order
    s[0, 6, 15, 15] = 2
    out, stats = C.postprocess(s, keep_largest=True)
    assert int((out == 1).sum()) == 8 and not (out == 2).any()
    assert stats[0].tolist() == [9, 2, 0, 0]


def test_rule4_counts_et_after_rules_1_to_3():
    s = _seg()
    s[0, 1:9, 1:9, 1:9] = 2
    s[0, 2:4, 2:4, 2:4] = 3                                   # 8 ET voxels inside the big component
    s[0, 10, 15:19, 15:19] = 3                                # 16 ET voxels forming a small WT component of their own
    out, stats = C.postprocess(s, min_component=20, et_min_voxels=10)
    assert not out[0, 10].any()                               # rule 1 removed the small component, its ET does not count
    assert not (out == 3).any() and int((out == 1).sum()) == 8
    assert stats[0].tolist() == [16, 1, 8, 0]
    out, _ = C.postprocess(s, et_min_voxels=10)               # without rule 1 the 24 ET voxels stay
    assert int((out == 3).sum()) == 24


def test_rule3_relabels_small_et_components_only():
    s = _seg()
    s[0, 1:9, 1:9, 1:9] = 1
    s[0, 2:5, 2:5, 2:5] = 3
    s[0, 7, 7, 7] = 3
    out, stats = C.postprocess(s, et_min_component=2, et_replace=2)
    assert out[0, 7, 7, 7] == 2 and int((out == 3).sum()) == 27
    assert stats[0].tolist() == [0, 0, 1, 27]


def test_rule_order_1_before_2():
    """Rule 2 keeps the largest of the components that SURVIVED rule 1: when rule 1 removes everything nothing is kept, and the count
    of removed components covers both rules."""
    s = _seg()
    s[0, 1:4, 1:4, 1:4] = 2                                   # 27
    s[0, 6:8, 6:8, 6:8] = 2                                   # 8
    s[0, 10, 10, 10] = 1                                      # 1
    out, stats = C.postprocess(s, min_component=5, keep_largest=True)
    assert int((out > 0).sum()) == 27 and stats[0].tolist() == [9, 2, 0, 0]
    out, stats = C.postprocess(s, min_component=30, keep_largest=True)
    assert not out.any() and stats[0].tolist() == [36, 3, 0, 0]
    out, stats = C.postprocess(s, min_component=5)
    assert int((out > 0).sum()) == 35 and stats[0].tolist() == [1, 1, 0, 0]


POLICIES = [dict(), dict(min_component=30), dict(keep_largest=True), dict(et_min_component=6, et_replace=2), dict(et_min_voxels=40),
            dict(et_min_voxels=100000, et_replace=0), dict(min_component=12, keep_largest=True, et_min_component=4, et_min_voxels=30)]


def noisy_labels(shape, rng, n_noise, scale=0.4):
    """A nested BraTS-like map plus stray voxels of every class."""
    lab = H.nested_labels(shape, rng, scale=scale)
    idx = rng.integers(0, lab.size, size=n_noise)
    lab.ravel()[idx] = rng.integers(1, 4, size=n_noise)
    return lab


@pytest.mark.parametrize("connectivity", [1, 2, 3])
def test_cpu_path_of_postprocess_equals_restatement(connectivity):
    import predict_overlap as po
    rng = np.random.default_rng(11 + connectivity)
    seg = np.stack([noisy_labels((24, 30, 21), rng, 150), noisy_labels((24, 30, 21), rng, 40)])
    for pol in POLICIES + [po.REFERENCE_POSTPROCESS]:
        want, wstats = C.postprocess(seg, connectivity=connectivity, **pol)
        got, stats = po.postprocess(torch.from_numpy(seg), connectivity=connectivity, with_stats=True, **pol)
        assert got.dtype == torch.int64 and np.array_equal(got.numpy(), want), pol
        assert stats.dtype == torch.int64 and np.array_equal(stats.numpy(), wstats), pol
        assert torch.equal(po.postprocess(torch.from_numpy(seg), connectivity=connectivity, **pol), got)
    assert po.REFERENCE_POSTPROCESS == dict(et_min_voxels=500, et_replace=1)


class _Stub(torch.nn.Module):
    """Stands in for the model on the CPU path of validate_softmax: class scores that depend on the input only."""

    class _U:
        class InitConv:
            dropout = 0.0
    Unet_list = _U

    def forward(self, x, missing_modal):
        return (torch.softmax(x * 3.0, dim=1),)


def test_validate_softmax_cpu_postprocess_none_changes_nothing_and_a_policy_applies():
    import predict_overlap as po
    from utils import tools
    g = torch.Generator().manual_seed(2)
    x = torch.randn(1, 4, 240, 240, 155, generator=g)
    x[:, 0] += 1.5                                            # mostly background, scattered foreground
    target = torch.from_numpy(H.nested_labels((240, 240, 155), np.random.default_rng(1))[None])
    m = _Stub()
    a = po.validate_softmax(x, target, m, with_miou=True)
    b = po.validate_softmax(x, target, m, with_miou=True, postprocess=None)
    assert len(a) == len(b) == 4 and torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert [float(v) for v in a[2]] == [float(v) for v in b[2]] and [float(v) for v in a[3]] == [float(v) for v in b[3]]
    pol = dict(min_component=3, et_min_component=2)
    seg, prob, dice, miou = po.validate_softmax(x, target, m, with_miou=True, postprocess=pol)
    want, _ = C.postprocess(a[0].numpy(), **pol)
    assert np.array_equal(seg.numpy(), want) and not np.array_equal(want, a[0].numpy())
    assert torch.equal(prob, a[1])
    assert [float(v) for v in dice] == [float(v) for v in tools.softmax_output_dice(seg, target)]
    assert [float(v) for v in miou] == [float(v) for v in tools.softmax_mIOU_score(seg, target)]


def test_bad_arguments_raise_value_error():
    import predict_overlap as po
    seg = torch.zeros((1, 4, 5, 6), dtype=torch.int64)
    for kw in (dict(et_replace=3), dict(et_replace=-1), dict(min_component=-1), dict(et_min_component=-2), dict(et_min_voxels=-500),
               dict(connectivity=0), dict(connectivity=4)):
        with pytest.raises(ValueError):
            po.postprocess(seg, **kw)
    for bad in (seg[0], seg.float(), seg.int(), seg.numpy(), torch.zeros((0, 4, 5, 6), dtype=torch.int64)):
        with pytest.raises(ValueError):
            po.postprocess(bad)
    assert torch.equal(po.postprocess(seg), seg)
