"""The boundary loss statement (tests/boundary_ref.py) against scipy, its pinned rounding case, and the host-side logic of the feature:
Trainer's weight check, total_loss's optional sixth part, the --boundary_weight / --boundary_warmup schedule."""
import numpy as np
import pytest
import torch

import boundary_ref as ref

SHAPES = ((1, 1, 1), (1, 1, 7), (5, 6, 7), (3, 70, 2), (9, 10, 11))


@pytest.mark.parametrize("shape", SHAPES)
def test_brute_force_equals_scipy_bit_for_bit(shape):
    rng = np.random.default_rng(sum(shape))
    label = rng.choice(4, size=(2,) + shape, p=[.5, .15, .2, .15]).astype(np.int64)
    a = ref.signed_distance(label, use_scipy=False)
    b = ref.signed_distance(label, use_scipy=True)
    assert a.dtype == np.float32 and a.shape == (2, 3) + shape
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize("shape", SHAPES)
def test_single_signed_field_passes_give_the_statement(shape):
    """the three integer axis passes the kernel runs (boundary_ref.emulate_passes) reach the brute-force q at every voxel"""
    rng = np.random.default_rng(7 + sum(shape))
    label = rng.choice(4, size=(1,) + shape, p=[.5, .15, .2, .15]).astype(np.int64)
    want = ref.signed_distance(label)
    for r, m in enumerate(ref.REGION_MASKS):
        f = ref.emulate_passes(label[0], m)
        q = np.abs(f).astype(np.float64)
        phi = np.where(np.abs(f) >= (1 << 30), 0.0, np.where(f < 0, 1.0 - np.sqrt(q), np.sqrt(q))).astype(np.float32)
        assert np.array_equal(phi.view(np.uint32), want[0, r].view(np.uint32)), (shape, r)


def test_empty_and_full_regions_give_positive_zeros():
    label = np.zeros((2, 4, 5, 6), dtype=np.int64)
    label[1] = 3
    for use_scipy in (False, True):
        phi = ref.signed_distance(label, use_scipy=use_scipy)
        assert np.array_equal(phi.view(np.uint32), np.zeros(phi.shape, dtype=np.uint32))
    # labels outside 0..31 and classes of no region are outside every region
    odd = np.array([[[[7, -1, 40, 3]]]], dtype=np.int64)
    assert ref.region(odd, 0b1000).tolist() == [[[[False, False, False, True]]]]
    assert ref.region(odd, 0xFFFFFFFF).tolist() == [[[[True, False, False, True]]]]


def test_one_minus_distance_is_rounded_once_from_float64():
    """q = 2 inside (the centre of a plus: its nearest outside voxels are the corners): float32(1 - sqrt(2.0)) is 0xBED413CD, while
    1.0f - sqrtf(2.0f) in float32 gives 0xBED413CC.  Over q <= 3 * 1023^2 the two differ at 1,847 values."""
    label = np.zeros((1, 1, 3, 3), dtype=np.int64)
    label[0, 0, 1, :] = 3
    label[0, 0, :, 1] = 3
    phi = ref.signed_distance(label, posmasks=(0b1000,))
    want = np.float32(1.0 - np.sqrt(2.0))
    two_roundings = np.float32(np.float32(1.0) - np.sqrt(np.float32(2.0)))
    assert phi[0, 0, 0, 1, 1].view(np.uint32) == want.view(np.uint32) == 0xBED413CD
    assert two_roundings.view(np.uint32) == 0xBED413CC
    q = np.arange(1, 3 * 1023 ** 2 + 1, dtype=np.int64)
    d = np.sqrt(q.astype(np.float64))
    once = (1.0 - d).astype(np.float32)
    twice = np.float32(1.0) - np.sqrt(q.astype(np.float32))
    assert int((once.view(np.uint32) != twice.view(np.uint32)).sum()) == 1847
    # the outside branch: a correctly rounded float32 sqrt of the integer is the float64 route
    assert np.array_equal(np.sqrt(q.astype(np.float32)).view(np.uint32), d.astype(np.float32).view(np.uint32))


def test_loss_statement_on_a_hand_case():
    """N = 1, one region {1}, V = 2: label (1, 0) -> phi = (0, 1); prob of class 1 = (0.25, 0.5): S = 0.5, loss = w / 2 * 0.5"""
    label = np.array([[[[1, 0]]]], dtype=np.int64)
    phi = ref.signed_distance(label, posmasks=(0b10,))
    assert phi.reshape(-1).tolist() == [0.0, 1.0]
    prob = np.zeros((1, 2, 1, 1, 2), dtype=np.float32)
    prob[0, 1, 0, 0] = (0.25, 0.5)
    prob[0, 0] = 1.0 - prob[0, 1]
    loss, sabs, dprob = ref.boundary_loss64(prob, phi, (0b10,), 0.5, gscale=2.0)
    assert float(loss) == 0.125 and sabs == 0.5
    assert dprob[0, 1].reshape(-1).tolist() == [0.0, 0.5] and not dprob[0, 0].any()


@pytest.mark.parametrize("bad", [-1, -1e-9, float("nan"), float("inf"), float("-inf")])
def test_trainer_rejects_a_bad_boundary_weight_before_touching_anything(bad):
    from cwf.trainer import Trainer
    with pytest.raises(ValueError, match="boundary_weight"):
        Trainer(None, boundary_weight=bad)          # (no model, no backend: the check comes first)


def _stub_losses(monkeypatch):
    from models import criterions
    from utils import tools
    calls = []
    monkeypatch.setattr(criterions, "softmax_dice", lambda o, t: torch.tensor(1.0))
    monkeypatch.setattr(tools, "get_separate_loss", lambda o, t: torch.tensor(2.0))
    monkeypatch.setattr(tools, "get_edge_separate_loss", lambda o, t: torch.tensor(4.0))

    def boundary(output, target, **kw):
        calls.append((output, target, kw))
        return torch.tensor(0.5)
    monkeypatch.setattr(tools, "boundary_loss", boundary)
    return calls


def test_total_loss_has_five_parts_without_a_boundary_weight(monkeypatch):
    from cwf.trainer import total_loss
    calls = _stub_losses(monkeypatch)
    outs = ["o0", "o1", "o2", "o3", "o4"]
    total, parts = total_loss(outs, "t", "e")
    assert len(parts) == 5 and float(total) == 13.0 and calls == []
    total, parts = total_loss(outs, "t", "e", boundary=None)
    assert len(parts) == 5 and float(total) == 13.0 and calls == []
    w = torch.tensor([0.25])
    total, parts = total_loss(outs, "t", "e", boundary=w)
    assert len(parts) == 6 and float(total) == 13.5 and float(parts[5]) == 0.5
    assert len(calls) == 1 and calls[0][0] == "o0" and calls[0][1] == "t" and calls[0][2]["weight"] is w


def test_boundary_flags_and_schedule():
    import train_no_amp as tn
    a = tn.build_parser().parse_args([])
    assert a.boundary_weight is None and a.boundary_warmup == 0
    tn.check_boundary(a)
    assert tn.boundary_weight_at(a, 0) is None and tn.boundary_weight_at(a, 500) is None      # off by default
    a = tn.build_parser().parse_args(["--boundary_weight", "0.01"])
    tn.check_boundary(a)
    assert [tn.boundary_weight_at(a, e) for e in (0, 1, 999)] == [0.01, 0.01, 0.01]          # E = 0: constant
    a = tn.build_parser().parse_args(["--boundary_weight", "0.01", "--boundary_warmup", "10"])
    tn.check_boundary(a)
    got = [tn.boundary_weight_at(a, e) for e in (0, 1, 5, 10, 11, 400)]
    assert got == [0.0, 0.01 * 0.1, 0.01 * 0.5, 0.01, 0.01, 0.01]
    assert got == [ref.warmup_weight(0.01, e, 10) for e in (0, 1, 5, 10, 11, 400)]
    for argv in (["--boundary_weight", "-0.5"], ["--boundary_weight", "nan"], ["--boundary_weight", "inf"],
                 ["--boundary_weight", "0.1", "--boundary_warmup", "-1"], ["--boundary_warmup", "5"],
                 ["--boundary_weight", "0.1", "--no_cuda", "true"]):
        with pytest.raises(SystemExit):
            tn.check_boundary(tn.build_parser().parse_args(argv))


def test_set_boundary_weight_needs_the_term_switched_on():
    from cwf.trainer import Trainer
    tr = Trainer.__new__(Trainer)
    tr.boundary_weight, tr._boundary, tr._plan = None, None, None
    with pytest.raises(ValueError):
        tr.set_boundary_weight(0.1)
    tr.boundary_weight, tr._boundary = 0.1, torch.tensor([0.1])
    tr.set_boundary_weight(0.25)
    assert tr.boundary_weight == 0.25 and float(tr._boundary) == 0.25
    with pytest.raises(ValueError):
        tr.set_boundary_weight(float("nan"))
    assert float(tr._boundary) == 0.25
