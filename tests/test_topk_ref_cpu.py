"""The top-k cross-entropy statement (tests/topk_ref.py) against torch.topk, its tie rule, the input families of the GPU tests, and
the host-side logic of the feature: topk_count, Trainer's argument checks, total_loss's optional part, the --topk_* flags."""
import numpy as np
import pytest
import torch

import topk_ref as ref

SHAPES = ((5, 6, 7), (33, 34, 65))


@pytest.mark.parametrize("c", [4, 2])
def test_without_ties_the_statement_is_the_mean_of_the_topk_losses(c):
    prob, label, posmask = ref.family("softmax", (9, 10, 11), c=c)
    t, pc, key = ref.keys_of(prob, label, posmask)
    assert np.unique(key).size == key.size and float(pc.min()) > 1e-7            # no ties, nothing at the floor
    nll = -torch.log(torch.from_numpy(pc.astype(np.float64)).reshape(-1))
    for k in (1, 7, ref.topk_count(key.size, 10.0), key.size):
        got = ref.topk_ce64(prob, label, k, 1.0, posmask)
        want = float(torch.topk(nll, k, sorted=False).values.mean())
        assert got["n"] == 1 and got["s"] == 1 and got["a"] == k - 1
        assert abs(got["loss64"] - want) <= 1e-13 * abs(want)
        assert got["loss"] == np.float32(got["loss64"])
        # the gradient of that mean: -1 / (k p) on the selected voxels' target class, nothing elsewhere
        sel = got["weights"] == 1.0
        assert int(sel.sum()) == k
        g = np.take_along_axis(got["dprob"], t[:, None], axis=1)[:, 0]
        assert np.allclose(g[sel], -1.0 / (k * pc[sel].astype(np.float64)), rtol=3e-7, atol=0) and not g[~sel].any()
        assert np.count_nonzero(got["dprob"]) == k


def test_ties_share_the_remaining_weight_and_the_gradient_ignores_voxel_order():
    prob, label, posmask = ref.family("lattice", (5, 6, 7))
    t, pc, key = ref.keys_of(prob, label, posmask)
    k = ref.tie_k(key)
    got = ref.topk_ce64(prob, label, k, 0.7, gscale=-0.5)
    assert 0 < got["s"] < got["n"] and got["a"] + got["s"] == k
    assert abs(got["weights"].sum() - k) <= 1e-9 * k                             # the weights sum to k
    assert set(np.unique(got["weights"])) <= {0.0, 1.0, got["s"] / got["n"]}
    perm = np.random.default_rng(3).permutation(key.size)
    shape = prob.shape

    def shuffle(x, channels):
        flat = np.moveaxis(x, 1, -1).reshape(-1, x.shape[1]) if channels else x.reshape(-1)
        flat = flat[perm]
        return np.moveaxis(flat.reshape((shape[0],) + shape[2:] + (x.shape[1],)), -1, 1).copy() if channels else flat.reshape(x.shape)
    again = ref.topk_ce64(shuffle(prob, True), shuffle(label, False), k, 0.7, gscale=-0.5)
    assert (again["tau"], again["a"], again["n"], again["s"]) == (got["tau"], got["a"], got["n"], got["s"])
    assert again["loss"] == got["loss"]
    assert np.array_equal(again["dprob"].view(np.uint32), shuffle(got["dprob"], True).view(np.uint32))
    assert np.array_equal(again["coef"].view(np.uint32), got["coef"].view(np.uint32))


def test_clamp_and_keys_of_special_values():
    pt = np.array([0.0, -0.0, -0.5, np.nan, 1.0, 1.5, np.inf, 0.25, 1e-40], dtype=np.float32)
    pc = ref.clamp(pt)
    assert pc.view(np.uint32).tolist()[:7] == [0, 0, 0, 0, 0x3F800000, 0x3F800000, 0x3F800000]
    assert pc[7] == np.float32(0.25) and pc[8] == np.float32(1e-40) and pc.view(np.uint32)[8] > 0
    l = ref.nll64(pc)
    assert l[0] == l[8] == -np.log(float(np.float32(1e-7))) and l[4] == 0.0
    # key order is value order on the clamped values
    v = np.sort(np.random.default_rng(0).uniform(0, 1, 1000).astype(np.float32))
    assert np.all(np.diff(v.view(np.uint32).astype(np.int64)) >= 0)
    # the gradient passes through the floor: a voxel at p = 0 gets -(w / k) / 1e-7
    prob = np.zeros((1, 4, 1, 1, 2), dtype=np.float32)
    prob[0, :, 0, 0, 1] = 0.25
    got = ref.topk_ce64(prob, np.zeros((1, 1, 1, 2), dtype=np.int64), 1, 1.0)
    assert got["tau"] == 0 and got["dprob"][0, 0, 0, 0, 0] == np.float32(-1.0) / np.float32(1e-7) and not got["dprob"][..., 1].any()


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("name", ref.FAMILIES)
def test_the_input_families_do_what_they_are_there_for(name, shape):
    for c in (4, 2):
        prob, label, posmask = ref.family(name, shape, c=c)
        t, pc, key = ref.keys_of(prob, label, posmask)
        m = key.size
        assert m == 2 * int(np.prod(shape)) and (c == 4 or (0 < t.sum() < m))
        ks = ref.ks_of(key)
        assert ks[:3] == [1, m, ref.topk_count(m, 10.0)]
        if name == "lattice":
            s = ref.select(key, ks[3])
            assert 0 < s[3] < s[2] and s[2] > m // 32                            # strictly inside a large tie group
        elif name == "last_digit":
            assert np.unique(key >> 10).size == 1 and np.unique(key & 1023).size > 300
        elif name == "exponents":
            assert np.unique(key >> 23).size == 31 and float(pc.min()) < 1e-7 < float(pc.max())
            assert ref.select(key, ks[2])[0] >> 21 != ref.select(key, m // 2)[0] >> 21
        elif name == "constant":
            assert ref.select(key, ks[2])[1:] == (0, m, ks[2]) and len(ks) == 4
            if m > 65535 * 2:
                assert ref.select(key, ks[2])[2] > 65535                         # more than a 16-bit bin would hold
        elif name == "specials":
            raw = np.take_along_axis(prob, t[:, None], axis=1)[:, 0]
            assert np.isnan(raw).any() and (raw < 0).any() and (raw > 1).any() and np.signbit(raw[raw == 0]).any()
            assert (key == 0).sum() >= 8 and (key == 0x3F800000).sum() >= 4 and ((key > 0) & (key < 0x00800000)).any()


def test_topk_count_edge_cases():
    from cwf.functional import topk_count
    assert topk_count(420, 10.0) == 42 and topk_count(145860, 10.0) == 14586
    assert topk_count(5, 10.0) == 1                                              # int(0.5) = 0 -> at least one voxel
    assert topk_count(1, 100.0) == 1 and topk_count(7, 100.0) == 7 and topk_count(7, 99.999) == 6
    assert topk_count(19, 10.0) == 1 and topk_count(20, 10.0) == 2 and topk_count(29, 10.0) == 2     # nnU-Net rounds down
    assert topk_count(10, 1e-9) == 1
    assert topk_count(2 * 4 * 128 ** 3, 10.0) == 1677721
    for m in (1, 5, 420, 145860):
        for pct in (0.001, 1.0, 10.0, 33.3, 100.0):
            assert topk_count(m, pct) == ref.topk_count(m, pct) and 1 <= topk_count(m, pct) <= m


def test_forward_bound_is_a_few_float32_roundings_of_the_value():
    prob, label, _ = ref.family("softmax", (5, 6, 7))
    got = ref.topk_ce64(prob, label, 42, 0.5)
    b = ref.forward_bound(got["loss"], got["sabs"], 0.5, 42)
    assert 2.0 ** -24 * abs(got["loss64"]) < b < 4 * 2.0 ** -24 * abs(got["loss64"])


# ------------------------------------------------------------------------------------------------------------------ host logic
@pytest.mark.parametrize("bad", [-1, -1e-9, float("nan"), float("inf"), float("-inf")])
def test_trainer_rejects_a_bad_topk_weight_before_touching_anything(bad):
    from cwf.trainer import Trainer
    with pytest.raises(ValueError, match="topk_weight"):
        Trainer(None, topk_weight=bad)              # (no model, no backend: the check comes first)


@pytest.mark.parametrize("bad", [0, 0.0, -5, 100.0001, 1000, float("nan"), float("inf")])
def test_trainer_rejects_a_bad_topk_percent_before_touching_anything(bad):
    from cwf.trainer import Trainer
    with pytest.raises(ValueError, match="topk_percent"):
        Trainer(None, topk_weight=0.5, topk_percent=bad)
    with pytest.raises(ValueError, match="topk_percent"):
        Trainer(None, topk_percent=bad)             # the percentage is checked with the term off too


def test_topk_ce_loss_rejects_a_bad_percent_before_touching_the_backend():
    from cwf import functional as CF
    p, t = torch.zeros((1, 4, 2, 2, 2)), torch.zeros((1, 2, 2, 2), dtype=torch.int64)
    for bad in (0.0, -1.0, 100.5, float("nan")):
        with pytest.raises(ValueError, match="percent"):
            CF.topk_ce_loss(p, t, percent=bad)
    with pytest.raises(ValueError, match="topk weight"):
        CF.loss_weight_tensor(torch.zeros(2), "cpu", "topk")
    w = torch.tensor([0.25])
    assert CF.loss_weight_tensor(w, "cpu", "topk") is w and CF.boundary_weight_tensor(w, "cpu") is w
    assert CF.loss_weight_tensor(0.5, "cpu", "topk").tolist() == [0.5]


def _stub_losses(monkeypatch):
    from models import criterions
    from utils import tools
    calls = []
    monkeypatch.setattr(criterions, "softmax_dice", lambda o, t: torch.tensor(1.0))
    monkeypatch.setattr(tools, "get_separate_loss", lambda o, t: torch.tensor(2.0))
    monkeypatch.setattr(tools, "get_edge_separate_loss", lambda o, t: torch.tensor(4.0))
    monkeypatch.setattr(tools, "boundary_loss", lambda o, t, **kw: calls.append(("boundary", o, t, kw)) or torch.tensor(0.5))
    monkeypatch.setattr(tools, "topk_ce", lambda o, t, **kw: calls.append(("topk", o, t, kw)) or torch.tensor(0.25))
    return calls


def test_total_loss_appends_the_topk_part_after_the_boundary_part(monkeypatch):
    from cwf.trainer import total_loss
    calls = _stub_losses(monkeypatch)
    outs = ["o0", "o1", "o2", "o3", "o4"]
    total, parts = total_loss(outs, "t", "e")
    assert len(parts) == 5 and float(total) == 13.0 and calls == []
    total, parts = total_loss(outs, "t", "e", None, topk=None)
    assert len(parts) == 5 and float(total) == 13.0 and calls == []
    w = torch.tensor([0.3])
    total, parts = total_loss(outs, "t", "e", topk=(w, 12.5))
    assert len(parts) == 6 and float(total) == 13.25 and float(parts[5]) == 0.25
    assert calls == [("topk", "o0", "t", {"percent": 12.5, "weight": w})] and calls[0][3]["weight"] is w
    del calls[:]
    b = torch.tensor([0.1])
    total, parts = total_loss(outs, "t", "e", b, topk=(w, 10.0))
    assert len(parts) == 7 and float(total) == 13.75 and [float(p) for p in parts[5:]] == [0.5, 0.25]
    assert [c[0] for c in calls] == ["boundary", "topk"] and calls[0][3]["weight"] is b


def test_topk_flags():
    import train_no_amp as tn
    a = tn.build_parser().parse_args([])
    assert a.topk_weight is None and a.topk_percent == 10.0                      # off by default
    tn.check_topk(a)
    a = tn.build_parser().parse_args(["--topk_weight", "0.5", "--topk_percent", "25"])
    tn.check_topk(a)
    assert a.topk_weight == 0.5 and a.topk_percent == 25.0
    tn.check_topk(tn.build_parser().parse_args(["--topk_weight", "0", "--topk_percent", "100"]))
    for argv in (["--topk_weight", "-0.5"], ["--topk_weight", "nan"], ["--topk_weight", "inf"], ["--topk_percent", "0"],
                 ["--topk_weight", "1", "--topk_percent", "100.5"], ["--topk_percent", "nan"], ["--topk_percent", "-3"],
                 ["--topk_weight", "0.1", "--no_cuda", "true"]):
        with pytest.raises(SystemExit):
            tn.check_topk(tn.build_parser().parse_args(argv))


def test_set_topk_weight_needs_the_term_switched_on():
    from cwf.trainer import Trainer
    tr = Trainer.__new__(Trainer)
    tr.topk_weight, tr.topk_percent, tr._topk, tr._plan = None, 10.0, None, None
    with pytest.raises(ValueError):
        tr.set_topk_weight(0.1)
    tr.topk_weight, tr._topk = 0.1, torch.tensor([0.1])
    tr.set_topk_weight(0.25)
    assert tr.topk_weight == 0.25 and float(tr._topk) == 0.25 and tr.topk_percent == 10.0
    for bad in (float("nan"), -1.0, None):
        with pytest.raises(ValueError):
            tr.set_topk_weight(bad)
    assert float(tr._topk) == 0.25


def test_drop_in_names_exist():
    from models import criterions
    from utils import tools
    assert callable(tools.topk_ce) and callable(criterions.topk_ce) and callable(criterions.softmax_dice_topk)
