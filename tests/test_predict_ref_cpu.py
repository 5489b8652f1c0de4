"""The statement of tests/predict_ref.py is right: argmax4 against torch.argmax on every row of the nine special values, the count
table and its two quotients against utils.tools and the oracle on label maps with absent classes, empty regions and labels outside
0..3, the stitch's index rule against predict_overlap.tailor_and_concat's slice assignments, and predict_overlap.flip_tta against the
eight terms written out, for every grouping `batch // nb` takes."""
import numpy as np
import pytest
import torch

import predict_overlap as po
import predict_ref as ref
from oracle import reference_model as rm
from utils import tools


# ------------------------------------------------------------------ argmax
def test_argmax4_is_torch_argmax_on_every_row_of_the_value_table():
    rows = ref.value_table()
    assert rows.shape == (6561, 4) and rows.dtype == np.float32
    assert np.signbit(ref.VALUES[2]) and ref.VALUES[2] == 0 and 0 < ref.VALUES[4] < np.float32(1.2e-38)     # -0.0 and a denormal
    got = ref.argmax4(rows, axis=1)
    want = torch.argmax(torch.from_numpy(rows), dim=1).numpy()
    assert got.dtype == np.int64 and np.array_equal(got, want)
    # the properties by name: a NaN beats +inf and the first NaN wins; the zeros tie; equal rows give 0
    assert ref.argmax4(np.array([[0.1, 0.2, np.nan, 0.9]], np.float32)).tolist() == [2]
    assert ref.argmax4(np.array([[np.inf, np.nan, np.nan, np.inf]], np.float32)).tolist() == [1]
    assert ref.argmax4(np.array([[-1.0, -0.0, 0.0, -0.0], [-1.0, 0.0, -0.0, 1e-45]], np.float32)).tolist() == [1, 3]
    assert ref.argmax4(np.array([[v] * 4 for v in ref.VALUES], np.float32)).tolist() == [0] * 9
    # the class axis in the middle, three differently permuted copies: the layout the kernels get
    rng = np.random.default_rng(0)
    vol = np.stack([rows[rng.permutation(6561)].T.reshape(4, 27, 27, 9) for _ in range(3)])
    assert np.array_equal(ref.argmax4(vol), torch.argmax(torch.from_numpy(vol), dim=1).numpy())


def test_tied_probabilities_hold_every_tie_pattern():
    p = ref.tied_probabilities(np.random.default_rng(1), (3, 10, 10, 10))
    top = p == p.max(axis=1, keepdims=True)
    patterns = set((top * np.array([1, 2, 4, 8]).reshape(1, 4, 1, 1, 1)).sum(axis=1).reshape(-1).tolist())
    assert patterns == set(range(1, 16)) and np.isfinite(p).all()
    assert np.array_equal(ref.argmax4(p), torch.argmax(torch.from_numpy(p), dim=1).numpy())


# ------------------------------------------------------------------ counts, Dice, IoU
def _label_cases():
    rng = np.random.default_rng(2)
    shape = (2, 5, 6, 7)
    cases = {"random": (rng.integers(0, 4, shape), rng.integers(0, 4, shape)),
             "class 3 absent": (rng.integers(0, 3, shape), rng.integers(0, 3, shape)),
             "class 1 absent in seg": (rng.integers(2, 4, shape), rng.integers(0, 4, shape)),
             "all background": (np.zeros(shape, np.int64), np.zeros(shape, np.int64)),
             "empty target": (rng.integers(0, 4, shape), np.zeros(shape, np.int64))}
    seg = rng.integers(0, 4, shape)
    cases["foreign"] = (seg, ref.target_families(rng, seg)["foreign"])
    cases["foreign on both sides"] = (ref.target_families(rng, seg)["foreign"], ref.target_families(rng, seg)["foreign"])
    return {k: (np.asarray(a, np.int64), np.asarray(b, np.int64)) for k, (a, b) in cases.items()}


@pytest.mark.parametrize("name", sorted(_label_cases()))
def test_counts_dice_and_iou_against_tools_and_the_oracle(name):
    seg, tgt = _label_cases()[name]
    c = ref.counts(seg, tgt)
    assert c.shape == (6, 3) and c.dtype == np.int64
    brute = np.zeros((6, 3), dtype=np.int64)                       # the table once more, one voxel at a time with Python integers
    for o, t in zip(seg.reshape(-1).tolist(), tgt.reshape(-1).tolist()):
        ro = [o > 0, o == 1 or o == 3, o == 3, o == 1, o == 2, o == 3]
        rt = [t > 0, t == 1 or t == 3, t == 3, t == 1, t == 2, t == 3]
        for k in range(6):
            brute[k] += (ro[k] and rt[k], ro[k], rt[k])
    assert np.array_equal(c, brute)
    d, i = ref.dice(c[:3]), ref.iou(c[3:])
    assert d.dtype == np.float64 and i.dtype == np.float64
    # the same IEEE operations on the same integers: equal, not close
    assert [float(v) for v in tools.softmax_output_dice(seg, tgt)] == d.tolist()
    assert [float(v) for v in tools.softmax_mIOU_score(seg, tgt)] == i.tolist()
    assert rm.softmax_output_dice(torch.from_numpy(seg), torch.from_numpy(tgt)) == d.tolist()
    assert rm.softmax_miou_score(torch.from_numpy(seg), torch.from_numpy(tgt)) == i.tolist()
    if name == "all background":
        assert d.tolist() == [1.0] * 3 and i.tolist() == [1.0] * 3          # eps / eps
    if name == "class 3 absent":
        assert c[2].tolist() == [0, 0, 0] and d[2] == 1.0 and i[2] == 1.0
    if name == "empty target":
        assert c[:, 2].tolist() == [0] * 6 and bool((d < 1e-9).all())


def test_the_foreign_labels_fall_where_the_host_rules_put_them():
    labels = np.array(list(range(-3, 7)) + [2 ** 32 + 1, 2 ** 32 + 3, -2 ** 63, 2 ** 63 - 1], dtype=np.int64)
    bits = ref.region_bits(labels)
    assert bits.dtype == np.uint8
    assert bits.tolist() == [0, 0, 0, 0, 3, 1, 7, 1, 1, 1, 1, 1, 0, 1]          # 2^32 + 3 is whole tumour only, not ET
    one = np.zeros(len(labels), dtype=np.int64)
    for k, lab in enumerate(labels):
        c = ref.counts(np.array([lab]), np.array([lab]))
        assert c[:3, 0].tolist() == [(int(bits[k]) >> r) & 1 for r in range(3)]
        one[k] = c[0, 0]
    assert one.tolist() == (labels > 0).astype(np.int64).tolist()


# ------------------------------------------------------------------ the stitch
def _position_codes(nb):
    """[nb, 4, 240, 240, 155] fp32 with integer values below 2^24: (a, bb) / c / b / the voxel's linear index, one code per channel"""
    a, bb, c = torch.arange(240).view(240, 1, 1), torch.arange(240).view(1, 240, 1), torch.arange(155).view(1, 1, 155)
    x = torch.empty((nb, 4, 240, 240, 155), dtype=torch.float32)
    x[:, 0] = (a * 240 + bb).float()
    x[:, 1] = c.float().expand(240, 240, 155)
    x[:, 2] = torch.arange(nb, dtype=torch.float32).view(nb, 1, 1, 1)
    x[:, 3] = ((a * 240 + bb) * 155 + c).float()
    assert float(x.max()) == 240 * 240 * 155 - 1 < 2 ** 24
    return x


def test_stitch_source_is_the_slice_assignments_of_tailor_and_concat():
    nb = 2
    x = _position_codes(nb)
    seen = []

    def identity(w, mm):
        seen.append(tuple(w.shape))
        return (w,)

    y = po.tailor_and_concat(x, None, identity, batched=False).numpy()
    assert seen == [(nb, 4, 128, 128, 128)] * 8 and y.shape == (nb, 4, 240, 240, 155)
    b, a, bb, c = np.ogrid[:nb, :240, :240, :155]
    wb, la, lb, lc = ref.stitch_source(b, a, bb, c, nb)
    for loc in (la, lb, lc):
        assert int(loc.min()) == 0 and int(loc.max()) == 127
    assert int(wb.min()) == 0 and int(wb.max()) == 8 * nb - 1
    window, sample = wb // nb, wb % nb
    assert np.array_equal(np.unique(window), np.arange(8)) and np.array_equal(sample, np.broadcast_to(b, sample.shape))
    sa, sb, sc = ref.window_start(window)
    assert [ref.window_start(w) for w in range(8)] == po.WINDOWS
    xn = x.numpy()
    for ch in range(4):
        want = xn[sample, ch, sa + la, sb + lb, sc + lc]
        assert np.array_equal(y[:, ch], want), ch
    # the rule on plain integers, at the seams and at the quirk
    assert ref.stitch_source(1, 127, 128, 127, 2) == (1 * 2 + 1, 127, 16, 127)
    assert ref.stitch_source(0, 128, 0, 128, 2) == (6 * 2 + 0, 16, 0, 96) and ref.stitch_source(0, 239, 239, 154, 1) == (7, 127, 127, 122)
    assert y[0, 1, 0, 0, 128] == 27 + 96 and y[0, 1, 0, 0, 154] == 27 + 122 and y[0, 1, 0, 0, 127] == 127     # voxels 123..149 land at 128..154


# ------------------------------------------------------------------ flip_tta
SP = (3, 4, 5)


def _codes():
    g = torch.Generator().manual_seed(3)
    return torch.randn((4,) + SP, generator=g, dtype=torch.float64) * 3.0


def _forward(calls):
    code = _codes()

    def forward(xb, mm):
        calls.append(int(xb.shape[0]))
        return code[None] + xb                                     # not flip-equivariant: the code stays where it is
    return forward


@pytest.mark.parametrize("resoftmax", [True, False])
@pytest.mark.parametrize("batch", [1, 8])
@pytest.mark.parametrize("nb", [1, 2, 3, 8, 9])
def test_flip_tta_is_the_eight_terms(nb, batch, resoftmax):
    x = torch.randn((nb, 4) + SP, generator=torch.Generator().manual_seed(nb), dtype=torch.float64)
    calls = []
    got = po.flip_tta(x, None, _forward(calls), resoftmax=resoftmax, batch=batch)
    per = max(1, batch // nb)                                      # flips per forward
    assert calls == [min(per, 8 - g0) * nb for g0 in range(0, 8, per)] and sum(calls) == 8 * nb
    assert per == {(1, 8): 8, (2, 8): 4, (3, 8): 2, (8, 8): 1}.get((nb, batch), 1)
    code = _codes()[None]
    want = None
    for dims in [(), (2,), (3,), (4,), (2, 3), (2, 4), (3, 4), (2, 3, 4)]:
        o = code + (x.flip(dims=dims) if dims else x)
        if resoftmax:
            o = torch.softmax(o, dim=1)
        o = o.flip(dims=dims) if dims else o
        want = o if want is None else want + o
    want = want / 8.0
    assert got.shape == x.shape and torch.equal(got, want)
    equivariant = code + x                                         # what a wrong un-flip or a wrong slice of the batch would leave
    assert not torch.allclose(got, torch.softmax(equivariant, 1) if resoftmax else equivariant)
    if resoftmax:                                                  # the oracle softmaxes after flipping back: the same values
        theirs = rm.flip_tta(x, lambda xb: code + xb)
        assert float((got - theirs).abs().max()) <= 4 * np.finfo(np.float64).eps
