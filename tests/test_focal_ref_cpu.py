"""The focal Tversky + focal cross-entropy statement (tests/focal_ref.py) against torch float64 autograd of the plain formula, its
identities, the condition its bounds put on the GPU test's inputs, and the host-side logic of the feature: the parameter ranges,
Trainer's argument checks, total_loss's optional part, the --focal_* / --tversky_* flags."""
import numpy as np
import pytest
import torch

import focal_ref as ref


CASES = [("softmax", "classwise"), ("lattice", "defaults"), ("lattice", "dice"), ("softmax", "ce_only"), ("specials", "classwise"),
         ("one_sided", "classwise")]


@pytest.mark.parametrize("name,pset", CASES)
def test_gradient_of_the_statement_against_float64_autograd(name, pset):
    """on inputs whose float32 p_r is exact (one class per region, or the lattice), so that the float64 formula sees the same p_r"""
    prob, label = ref.family(name, (5, 6, 7))
    posmasks, p = ref.PARAM_SETS[pset]
    for gamma in ((p["gamma"],) if pset != "ce_only" else (0.0, 1.0, 2.0, 3.0, 2.5)):
        p = dict(p, gamma=gamma)
        res = ref.focal64(prob, label, posmasks, p, w=0.37, gscale=-0.75)
        leaf = torch.from_numpy(prob.astype(np.float64)).requires_grad_(True)
        loss = ref.torch_statement(leaf, torch.from_numpy(label), posmasks, p, 0.37)
        (-0.75 * loss).backward()
        want = leaf.grad.numpy()
        assert abs(res["loss64"] - float(loss.detach())) <= 1e-12 * abs(float(loss.detach()))
        assert np.abs(res["dprob_exact"] - want).max() <= 1e-12 * np.abs(want).max(), (name, pset, gamma)
        assert np.abs(want).max() > 0
        # the float32 coefficient table carries the same gradient to float32 accuracy, and the float32 order follows it
        assert np.abs(res["dprob64"] - want).max() <= 4 * ref.U * np.abs(res["sabs"]).max() * 0.75 + 1e-30
        assert np.all(np.abs(res["dprob32"].astype(np.float64) - res["dprob64"]) <= ref.grad_bound(res))


def test_dice_identity():
    """a = b = 0.5, e = 1, rho = 0: 1 - mean_r (2 TP + 2 s) / (SP + ST + 2 s), the soft Dice loss of the regions"""
    posmasks, p = ref.PARAM_SETS["dice"]
    for name in ref.FAMILIES:
        prob, label = ref.family(name, (5, 6, 7))
        res = ref.focal64(prob, label, posmasks, p)
        s = p["smooth"]
        dice = np.mean(np.maximum(1.0 - (2 * res["TP"] + 2 * s) / (res["SP"] + res["ST"] + 2 * s), 0.0))
        assert name == "saturated" or np.all((2 * res["TP"] + 2 * s) < (res["SP"] + res["ST"] + 2 * s))     # (no region is clamped)
        assert abs(res["loss64"] - dice) <= 1e-13 * max(abs(dice), 1e-3), (name, res["loss64"], dice)


def test_gamma_zero_is_the_mean_negative_log_likelihood():
    posmasks, p = ref.PARAM_SETS["ce_only"]
    for name in ("softmax", "specials", "full"):
        prob, label = ref.family(name, (5, 6, 7))
        res = ref.focal64(prob, label, posmasks, p)
        py = np.take_along_axis(prob, label[:, None], axis=1)[:, 0]
        want = float(np.mean(-np.log(np.minimum(np.maximum(py, ref.FLOOR), np.float32(1.0)).astype(np.float64))))
        assert abs(res["loss64"] - want) <= 1e-13 * want
        assert res["coef"].shape == (1,) and res["coef"][0] == np.float32(1.0 / label.size)


def test_sums_are_taken_over_the_whole_batch():
    prob, label = ref.family("one_sided", (5, 6, 7))
    posmasks, p = ref.PARAM_SETS["dice"]
    both = ref.focal64(prob, label, posmasks, p)["loss64"]
    per = np.mean([ref.focal64(prob[i:i + 1], label[i:i + 1], posmasks, p)["loss64"] for i in range(2)])
    assert not label[1].any() and label[0].max() == 3
    assert abs(both - per) > 1e-2                                              # the second sample alone has Tversky index ~ 0


def test_a_region_at_or_past_a_perfect_index_contributes_nothing():
    p = ref.params(ce_ratio=0.0)
    assert ref.region_terms(10.0, 10.0, 10.0, p, 3) == (0.0, 0.0, 0.0)         # TI = 1
    assert ref.region_terms(12.0, 12.0, 10.0, p, 3) == (0.0, 0.0, 0.0)         # TI > 1 (probabilities above 1)
    xe, ka, kb = ref.region_terms(5.0, 9.0, 10.0, p, 3)
    assert xe > 0 and ka < 0 < kb                                              # more TP lowers the loss, more FP raises it


@pytest.mark.parametrize("shape", ref.SHAPES)
@pytest.mark.parametrize("name", ref.FAMILIES)
def test_the_gpu_test_inputs_keep_the_loss_far_above_its_bound(name, shape):
    prob, label = ref.family(name, shape)
    assert prob.shape == (2, 4) + shape and label.shape == (2,) + shape
    if name == "empty":
        assert label.max() == 2
    elif name == "full":
        assert label.min() == 1
    elif name == "specials":
        py = np.take_along_axis(prob, label[:, None], axis=1)[:, 0]
        assert (py == 0).sum() >= 3 and (py == 1).sum() >= 3 and (py > 1).sum() >= 3 and ((py > 0) & (py < ref.FLOOR)).sum() >= 3
        assert (py == ref.FLOOR).sum() >= 3
    elif name in ref.EXACT:
        assert np.unique(prob).size <= 17 and np.all(np.take_along_axis(prob, label[:, None], axis=1) == 1.0)
    for pset, (posmasks, p) in ref.PARAM_SETS.items():
        res = ref.focal64(prob, label, posmasks, p, w=0.37)
        b = ref.forward_bound(res)
        assert res["loss64"] == 0.0 or abs(res["loss64"]) > 1e3 * b, (name, shape, pset, res["loss64"], b)
        assert res["loss64"] != 0.0 or (name in ref.EXACT and pset == "ce_only")
        terms = [ref.region_terms(res["TP"][r], res["SP"][r], res["ST"][r], p, res["R"]) for r in range(res["R"])]
        if name == "saturated" and pset == "defaults":
            assert any(t == (0.0, 0.0, 0.0) for t in terms) and terms[2][0] > 0   # a region is clamped, ET is not
        elif name != "saturated":
            assert all(t[0] > 0 for t in terms)
        assert b < 8 * ref.U * abs(res["loss64"]) + 1e-300                      # a few float32 roundings of the value
        cb = ref.coef_bound(res)
        assert np.all(cb <= 8 * ref.U * np.abs(res["coef64"]) + 1e-40)
        if name == "empty" and pset == "defaults":
            assert res["ST"][2] == 0 and res["TP"][2] == 0
        if name == "full" and pset == "defaults":
            assert res["TP"][0] == res["SP"][0]


# ------------------------------------------------------------------------------------------------------------------ host logic
BAD = [dict(fn=-0.1), dict(fn=float("nan")), dict(fp=float("inf")), dict(fn=0.0, fp=0.0), dict(exponent=0.0), dict(exponent=4.5),
       dict(exponent=float("nan")), dict(smooth=0.0), dict(smooth=-1e-5), dict(smooth=float("inf")), dict(gamma=0.5), dict(gamma=-1.0),
       dict(gamma=5.5), dict(gamma=float("nan")), dict(ce_ratio=-1.0), dict(ce_ratio=float("inf")), dict(class_weight=(1, 1, 1)),
       dict(class_weight=(1, -1, 1, 1)), dict(class_weight=(1, 1, float("nan"), 1)), dict(posmasks=(), ce_ratio=0.0), dict(posmasks=(0,)),
       dict(posmasks=(16,)), dict(posmasks=(1,) * 9), dict(weight=torch.zeros(2))]


@pytest.mark.parametrize("bad", BAD, ids=[",".join("%s=%s" % kv for kv in b.items()).replace(" ", "") for b in BAD])
def test_focal_loss_rejects_a_value_outside_its_range_before_touching_the_backend(bad, monkeypatch):
    from cwf import functional as CF

    def boom():
        raise AssertionError("the backend was touched")
    monkeypatch.setattr(CF, "backend", boom)
    p, t = torch.full((1, 4, 2, 2, 2), 0.25), torch.zeros((1, 2, 2, 2), dtype=torch.int64)
    with pytest.raises(ValueError):
        CF.focal_loss(p, t, **bad)


def test_accepted_edge_values():
    from cwf.kernels import check_focal_params
    for ok in (dict(fn=0.0), dict(fp=0.0), dict(exponent=4.0), dict(gamma=0.0), dict(gamma=1.0), dict(gamma=5.0), dict(ce_ratio=0.0),
               dict(class_weight=(0, 0, 0, 0))):
        check_focal_params((14, 10, 8), **ok)
    got = check_focal_params((), gamma=3)
    assert got["gamma"] == 3.0 and got["class_weight"] == (1.0, 1.0, 1.0, 1.0) and got["fn"] == 0.7 and got["exponent"] == 0.75


@pytest.mark.parametrize("bad", [-1, -1e-9, float("nan"), float("inf")])
def test_trainer_rejects_a_bad_focal_weight_before_touching_anything(bad):
    from cwf.trainer import Trainer
    with pytest.raises(ValueError, match="focal_weight"):
        Trainer(None, focal_weight=bad)
    with pytest.raises(ValueError):
        Trainer(None, focal_weight=0.5, focal_params=dict(gamma=0.5))
    with pytest.raises(ValueError):
        Trainer(None, focal_params=dict(gamma=0.5))                             # the parameters are checked with the term off too
    with pytest.raises(ValueError, match="focal_params"):
        Trainer(None, focal_weight=0.5, focal_params=dict(percent=3))


def test_total_loss_appends_the_focal_part_last(monkeypatch):
    from cwf.trainer import total_loss
    from models import criterions
    from utils import tools
    calls = []
    monkeypatch.setattr(criterions, "softmax_dice", lambda o, t: torch.tensor(1.0))
    monkeypatch.setattr(tools, "get_separate_loss", lambda o, t: torch.tensor(2.0))
    monkeypatch.setattr(tools, "get_edge_separate_loss", lambda o, t: torch.tensor(4.0))
    monkeypatch.setattr(tools, "boundary_loss", lambda o, t, **kw: calls.append(("boundary", o, t, kw)) or torch.tensor(0.5))
    monkeypatch.setattr(tools, "topk_ce", lambda o, t, **kw: calls.append(("topk", o, t, kw)) or torch.tensor(0.25))
    monkeypatch.setattr(tools, "focal_loss", lambda o, t, **kw: calls.append(("focal", o, t, kw)) or torch.tensor(0.125))
    outs = ["o0", "o1", "o2", "o3", "o4"]
    total, parts = total_loss(outs, "t", "e")
    assert len(parts) == 5 and float(total) == 13.0 and calls == []
    total, parts = total_loss(outs, "t", "e", None, topk=None, focal=None)
    assert len(parts) == 5 and calls == []
    w = torch.tensor([0.3])
    total, parts = total_loss(outs, "t", "e", focal=(w, dict(gamma=3.0)))
    assert len(parts) == 6 and float(total) == 13.125 and calls == [("focal", "o0", "t", {"weight": w, "gamma": 3.0})]
    assert calls[0][3]["weight"] is w
    del calls[:]
    total, parts = total_loss(outs, "t", "e", torch.tensor([0.1]), topk=(w, 10.0), focal=(w, {}))
    assert len(parts) == 8 and float(total) == 13.875 and [c[0] for c in calls] == ["boundary", "topk", "focal"]
    assert [float(q) for q in parts[5:]] == [0.5, 0.25, 0.125]


def test_set_focal_weight_needs_the_term_switched_on():
    from cwf.trainer import Trainer, check_focal
    tr = Trainer.__new__(Trainer)
    tr.focal_weight, tr.focal_params, tr._focal, tr._plan = None, check_focal(None, None)[1], None, None
    with pytest.raises(ValueError):
        tr.set_focal_weight(0.1)
    tr.focal_weight, tr._focal = 0.1, torch.tensor([0.1])
    tr.set_focal_weight(0.25)
    assert tr.focal_weight == 0.25 and float(tr._focal) == 0.25
    for bad in (float("nan"), -1.0, None):
        with pytest.raises(ValueError):
            tr.set_focal_weight(bad)
    assert float(tr._focal) == 0.25 and tr.focal_params["posmasks"] == (14, 10, 8)


def test_focal_flags():
    import train_no_amp as tn
    a = tn.build_parser().parse_args([])
    assert a.focal_weight is None                                                # off by default
    assert (a.tversky_fn, a.tversky_fp, a.tversky_exponent, a.focal_gamma, a.focal_ce_ratio) == (0.7, 0.3, 0.75, 2.0, 1.0)
    tn.check_focal(a)
    a = tn.build_parser().parse_args(["--focal_weight", "0.5", "--tversky_fn", "0.6", "--tversky_fp", "0.4", "--tversky_exponent", "1",
                                      "--focal_gamma", "3", "--focal_ce_ratio", "0"])
    tn.check_focal(a)
    assert tn.focal_params_of(a) == dict(fn=0.6, fp=0.4, exponent=1.0, gamma=3.0, ce_ratio=0.0) and a.focal_weight == 0.5
    for argv in (["--focal_weight", "-0.5"], ["--focal_weight", "nan"], ["--focal_gamma", "0.5"], ["--tversky_exponent", "0"],
                 ["--tversky_fn", "0", "--tversky_fp", "0"], ["--focal_ce_ratio", "-1"], ["--focal_weight", "0.1", "--no_cuda", "true"]):
        with pytest.raises(SystemExit):
            tn.check_focal(tn.build_parser().parse_args(argv))


def test_drop_in_names_exist():
    from models import criterions
    from utils import tools
    for mod in (tools, criterions):
        assert callable(mod.focal_tversky) and callable(mod.focal_ce) and callable(mod.focal_loss)
    assert callable(criterions.softmax_dice_focal)


def test_binding_covers_the_new_entries():
    from cwf import _lib
    for name in ("cwf_focal_workspace", "cwf_focal_loss", "cwf_focal_loss_bwd"):
        assert name in _lib.SIGNATURES
    assert "cwf_focal_workspace" in _lib.RESTYPE_INT64
    assert [f[0] for f in _lib.FocalParams._fields_] == ["fn", "fp", "exponent", "smooth", "gamma", "ce_ratio", "class_weight"]
