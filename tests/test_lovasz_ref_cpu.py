"""tests/lovasz_ref.py (the yardstick of the GPU tests) against a sort-based float64 torch formulation of the Lovasz-Softmax loss, and
the host-side logic of the feature: check_lovasz_params, Trainer's argument checks, total_loss's optional part, the --lovasz_* flags."""
import numpy as np
import pytest
import torch

import lovasz_ref as ref

SMALL = (5, 6, 7)
MASKSETS = {"classes": ref.CLASS_MASKS, "regions": ref.REGION_MASKS}


def _sorted_formulation(e, fg):
    """Berman's lovasz_softmax_flat for one region on the errors e (float64 leaf): sort descending, cumulative sums, Jaccard
    differences, dot -> (loss, gradient with respect to e by autograd)"""
    x = torch.tensor(e.astype(np.float64), requires_grad=True)
    t = torch.tensor(fg.astype(np.float64))
    es, perm = torch.sort(x.abs(), descending=True, stable=True)
    ts = t[perm]
    gts = ts.sum()
    inter = gts - ts.cumsum(0)
    union = gts + (1.0 - ts).cumsum(0)
    jac = 1.0 - inter / union
    jac = torch.cat([jac[:1], jac[1:] - jac[:-1]])
    loss = torch.dot(es, jac.detach())
    loss.backward()
    return float(loss.detach()), x.grad.numpy()


CASES = [(name, "classes", op) for name in ref.FAMILIES for op in (True,)] + \
        [("softmax", "regions", True), ("lattice", "regions", True), ("absent", "classes", False), ("full", "classes", False)]


@pytest.mark.parametrize("name,maskset,only_present", CASES)
def test_the_statement_against_the_sort_based_formulation(name, maskset, only_present):
    masks = MASKSETS[maskset]
    prob, label = ref.family(name, SMALL)
    want = ref.lovasz64(prob, label, masks, only_present, w=1.0)
    fg, e = want["fg"], want["e"]
    total, counted = 0.0, 0
    for r in range(len(masks)):
        if want["G"][r] == 0 and only_present:
            assert not want["share64"][r].any()
            continue
        counted += 1
        loss, grad = _sorted_formulation(e[r], fg[r])
        total += loss
        share = want["share64"][r]
        key = e[r].view(np.uint32)
        _, inv, cnt = np.unique(key, return_inverse=True, return_counts=True)
        inv = inv.reshape(-1)
        live = e[r] > 0                                   # abs has no gradient at 0: the statement gives those voxels none
        if maskset == "classes":
            assert (cnt.max() == 1) == (name in ref.TIE_FREE), (name, r, cnt.max())
        if cnt.max() == 1:
            assert np.allclose(grad[live], share[live], rtol=1e-12, atol=0.0)
        # per tie group: the statement's share is the mean of the sorted formulation's gradient over the group
        mean = np.bincount(inv, weights=grad, minlength=cnt.size) / cnt
        assert np.allclose(share[live], mean[inv][live], rtol=1e-12, atol=1e-300)
        assert np.all(np.sign(want["vcoef"][r][live]) == np.where(fg[r][live], -1.0, 1.0)) or not share[live].all()
        assert not want["vcoef"][r][~live].any()
    assert counted == want["P"]
    if counted:
        assert abs(want["loss64"] - total / counted) <= 1e-12 * abs(total / counted)
    else:
        assert want["loss64"] == 0.0


@pytest.mark.parametrize("name", ref.FAMILIES)
@pytest.mark.parametrize("shape", [SMALL, (33, 34, 65)])
def test_jaccard_increments_are_never_negative_and_the_families_do_their_job(name, shape):
    prob, label = ref.family(name, shape)
    for masks in (ref.CLASS_MASKS, ref.REGION_MASKS):
        want = ref.lovasz64(prob, label, masks, only_present=False)
        assert want["dJmin"] >= 0.0
        assert float(want["loss"]) == 0.0 or abs(float(want["loss"])) > 1e3 * ref.forward_bound(want["loss"], label.size)
    want = ref.lovasz64(prob, label)
    keys = want["e"].view(np.uint32)
    if name == "softmax":
        assert all(g > 0 for g in want["G"]) and want["P"] == 4
    if name == "lattice":
        assert all(np.unique(k).size <= 9 for k in keys)
        if shape != SMALL:
            assert max(np.bincount(k & 255).max() for k in keys) > 65535          # one digit bucket beyond 16 bits
        for r in range(4):
            for v in np.unique(keys[r]):
                sel = keys[r] == v
                assert want["fg"][r][sel].any() and not want["fg"][r][sel].all()  # every group mixes foreground and background
    if name == "saturated":
        assert all(set(np.unique(k)) == {0, 0x3F800000} for k in keys)
    if name == "perfect":
        assert not keys.any() and float(want["loss"]) == 0.0 and not want["dprob"].any() and not want["vcoef"].any()
        assert not np.signbit(want["loss"])
    if name == "lowbits":
        assert all(np.unique(k >> 8).size == 1 and np.unique(k).size > 100 for k in keys)
    if name == "exponents":
        assert all(np.unique(k >> 23).size >= 100 for k in keys) and keys.min() <= 1 and (keys == 1).any()
    if name == "specials":
        e = want["e"]
        assert np.isnan(prob).any() and np.isinf(prob).any() and np.isfinite(e).all() and e.min() >= 0 and e.max() <= 1
        assert not np.signbit(e).any() and np.isfinite(want["dprob"]).all()
    if name == "absent":
        assert want["G"][2] == 0 and want["P"] == 3 and not want["vcoef"][2].any()
        off = ref.lovasz64(prob, label, only_present=False)
        assert off["P"] == 4
        reg = ref.region64(off["e"][2], off["fg"][2])
        assert reg["L"] == float(off["e"][2].max())                              # all background: the largest error
    if name == "full":
        assert want["G"][1] == label.size and want["P"] == 1


def test_loss_and_gradient_ignore_the_order_of_the_voxels():
    for name in ("softmax", "lattice", "specials"):
        prob, label = ref.family(name, SMALL)
        flat = np.moveaxis(prob, 1, -1).reshape(-1, 4)
        perm = np.random.default_rng(5).permutation(flat.shape[0])
        p2 = np.moveaxis(flat[perm].reshape(prob.shape[:1] + prob.shape[2:] + (4,)), -1, 1)
        l2 = label.reshape(-1)[perm].reshape(label.shape)
        for masks in (ref.CLASS_MASKS, ref.REGION_MASKS):
            a = ref.lovasz64(prob, label, masks, w=0.7, gscale=-1.5)
            b = ref.lovasz64(p2, l2, masks, w=0.7, gscale=-1.5)
            assert np.float32(a["loss"]).view(np.uint32) == np.float32(b["loss"]).view(np.uint32)
            da = np.moveaxis(a["dprob"], 1, -1).reshape(-1, 4)
            db = np.moveaxis(b["dprob"], 1, -1).reshape(-1, 4)
            assert np.array_equal(da[perm].view(np.uint32), db.view(np.uint32))
            assert np.array_equal(a["vcoef"][:, perm].view(np.uint32), b["vcoef"].view(np.uint32))


def test_only_present_counting_and_coef():
    prob, label = ref.family("absent", SMALL)
    on = ref.lovasz64(prob, label, w=0.6)
    off = ref.lovasz64(prob, label, only_present=False, w=0.6)
    w = float(np.float32(0.6))
    assert on["coef"].tolist() == [np.float32(w / 3), 3.0, 0.0, 0.0] and off["coef"].tolist() == [np.float32(w / 4), 4.0, 0.0, 0.0]
    assert off["loss64"] != on["loss64"]
    # nothing counted: every voxel of class 1, the region of class 0 alone
    prob, label = ref.family("full", SMALL)
    none = ref.lovasz64(prob, label, masks=(1,), w=0.6)
    assert none["P"] == 0 and none["loss64"] == 0.0 and none["coef"].tolist() == [0.0, 0.0, 0.0, 0.0] and not none["dprob"].any()


def test_a_class_in_several_regions_adds_their_gradients_in_region_order():
    prob, label = ref.family("softmax", SMALL)
    want = ref.lovasz64(prob, label, ref.REGION_MASKS, w=1.0, gscale=2.0)
    g0 = np.float32(np.float32(2.0) * want["coef"][0])
    d = np.moveaxis(want["dprob"], 1, -1).reshape(-1, 4)
    t = [(g0 * want["vcoef"][r]).astype(np.float32) for r in range(3)]
    assert not d[:, 0].any()                                                     # class 0 is in no region: +0
    assert np.array_equal(d[:, 2], t[0]) and np.array_equal(d[:, 1], (t[0] + t[1]).astype(np.float32))
    assert np.array_equal(d[:, 3], ((t[0] + t[1]).astype(np.float32) + t[2]).astype(np.float32))


# ------------------------------------------------------------------------------------------------------------------ host-side logic
def test_check_lovasz_params():
    from cwf.kernels import CLASS_MASKS, REGION_MASKS, check_lovasz_params
    assert CLASS_MASKS == ref.CLASS_MASKS and REGION_MASKS == ref.REGION_MASKS
    assert check_lovasz_params([1, 2, 4, 8]) == ((1, 2, 4, 8), True)
    assert check_lovasz_params(REGION_MASKS, False) == (REGION_MASKS, False)
    assert check_lovasz_params((15,) * 8) == ((15,) * 8, True)
    for bad in ((), (1,) * 9, (0,), (16,), (1, -2), (1.5,), 3):
        with pytest.raises(ValueError):
            check_lovasz_params(bad)
    for bad in (None, 1, "yes"):
        with pytest.raises(ValueError):
            check_lovasz_params((1, 2), bad)


@pytest.mark.parametrize("bad", [float("nan"), float("inf"), -0.5])
def test_trainer_rejects_a_bad_lovasz_weight_before_touching_anything(bad):
    from cwf.trainer import Trainer
    with pytest.raises(ValueError):
        Trainer(None, lovasz_weight=bad)                # (no model, no backend: the check comes first)


@pytest.mark.parametrize("bad", ["all", (), (0, 1), (16,), (1,) * 9])
def test_trainer_rejects_bad_lovasz_regions_before_touching_anything(bad):
    from cwf.trainer import Trainer
    with pytest.raises(ValueError):
        Trainer(None, lovasz_weight=0.5, lovasz_regions=bad)
    with pytest.raises(ValueError):
        Trainer(None, lovasz_regions=bad)               # checked with the term off too
    with pytest.raises(ValueError):
        Trainer(None, lovasz_weight=0.5, lovasz_only_present=None)


def test_check_lovasz_names_the_region_sets():
    from cwf.trainer import check_lovasz
    assert check_lovasz(None) == (None, ref.CLASS_MASKS, True)
    assert check_lovasz(0.5, "regions", False) == (0.5, ref.REGION_MASKS, False)
    assert check_lovasz(0, (3, 12)) == (0.0, (3, 12), True)


def test_lovasz_softmax_rejects_bad_arguments_before_touching_the_backend():
    from cwf import functional as CF
    p, l = torch.zeros((1, 4, 2, 2, 2)), torch.zeros((1, 2, 2, 2), dtype=torch.int64)
    for kw in (dict(posmasks=()), dict(posmasks=(16,)), dict(only_present=1), dict(weight=torch.ones(2))):
        with pytest.raises(ValueError):
            CF.lovasz_softmax(p, l, **kw)
    with pytest.raises(ValueError):
        CF.lovasz_softmax(torch.zeros((1, 3, 2, 2, 2)), l)


def test_total_loss_appends_the_lovasz_part_last(monkeypatch):
    from cwf.trainer import total_loss
    from models import criterions
    from utils import tools
    calls = []
    monkeypatch.setattr(criterions, "softmax_dice", lambda o, t: torch.tensor(1.0))
    monkeypatch.setattr(tools, "get_separate_loss", lambda o, t: torch.tensor(2.0))
    monkeypatch.setattr(tools, "get_edge_separate_loss", lambda o, t: torch.tensor(4.0))
    monkeypatch.setattr(tools, "focal_loss", lambda o, t, **kw: calls.append(("focal", o, t, kw)) or torch.tensor(0.5))
    monkeypatch.setattr(tools, "lovasz_softmax", lambda o, t, **kw: calls.append(("lovasz", o, t, kw)) or torch.tensor(0.125))
    outs = ["o0", "o1", "o2", "o3", "o4"]
    total, parts = total_loss(outs, "t", "e")
    assert len(parts) == 5 and float(total) == 13.0 and calls == []
    total, parts = total_loss(outs, "t", "e", None, lovasz=None)
    assert len(parts) == 5 and calls == []
    w = torch.tensor([0.3])
    total, parts = total_loss(outs, "t", "e", lovasz=(w, (1, 2, 4, 8), True))
    assert len(parts) == 6 and float(total) == 13.125
    assert calls == [("lovasz", "o0", "t", {"posmasks": (1, 2, 4, 8), "only_present": True, "weight": w})] and calls[0][3]["weight"] is w
    del calls[:]
    total, parts = total_loss(outs, "t", "e", focal=(w, {}), lovasz=(w, ref.REGION_MASKS, False))
    assert len(parts) == 7 and [float(p) for p in parts[5:]] == [0.5, 0.125] and [c[0] for c in calls] == ["focal", "lovasz"]


def test_lovasz_flags():
    import train_no_amp as tn
    a = tn.build_parser().parse_args([])
    assert a.lovasz_weight is None and a.lovasz_regions == "classes"              # off by default
    tn.check_lovasz(a)
    a = tn.build_parser().parse_args(["--lovasz_weight", "0.5", "--lovasz_regions", "regions"])
    tn.check_lovasz(a)
    assert a.lovasz_weight == 0.5 and a.lovasz_regions == "regions"
    tn.check_lovasz(tn.build_parser().parse_args(["--lovasz_weight", "0"]))
    for argv in (["--lovasz_weight", "-0.5"], ["--lovasz_weight", "nan"], ["--lovasz_weight", "inf"],
                 ["--lovasz_weight", "0.1", "--no_cuda", "true"]):
        with pytest.raises(SystemExit):
            tn.check_lovasz(tn.build_parser().parse_args(argv))
    with pytest.raises(SystemExit):
        tn.build_parser().parse_args(["--lovasz_regions", "voxels"])


def test_set_lovasz_weight_needs_the_term_switched_on():
    from cwf.trainer import Trainer
    tr = Trainer.__new__(Trainer)
    tr.lovasz_weight, tr.lovasz_regions, tr.lovasz_only_present, tr._lovasz, tr._plan = None, ref.CLASS_MASKS, True, None, None
    with pytest.raises(ValueError):
        tr.set_lovasz_weight(0.1)
    tr.lovasz_weight, tr._lovasz = 0.1, torch.tensor([0.1])
    tr.set_lovasz_weight(0.25)
    assert tr.lovasz_weight == 0.25 and float(tr._lovasz) == 0.25 and tr.lovasz_regions == ref.CLASS_MASKS
    for bad in (float("nan"), -1.0, None):
        with pytest.raises(ValueError):
            tr.set_lovasz_weight(bad)
    assert float(tr._lovasz) == 0.25


def test_drop_in_names_exist():
    from models import criterions
    from utils import tools
    assert callable(tools.lovasz_softmax) and callable(criterions.lovasz_softmax) and callable(criterions.softmax_dice_lovasz)
