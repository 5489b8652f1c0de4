"""The top-k cross-entropy term on the GPU (csrc/topk.hip and its way up through cwf.kernels, cwf.functional, utils.tools,
models.criterions and cwf.trainer.Trainer): tau, s / n and the gradient bit-equal to the statement, the loss within its derived
bound and bit-identical from call to call, and the Trainer with the term off and on.  Yardstick: tests/topk_ref.py."""
import functools

import numpy as np
import pytest
import torch

import boundary_ref
import topk_ref as ref
from test_boundary_gpu import _batch, _no_dropout_model          # the 64^3 teacher-forced recipe and its cached batch, shared

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# M = 420: less than one workgroup's worth per launch, ragged; M = 145,860: many workgroups, odd extents, more than 65,535 in a bin
SHAPES = ((5, 6, 7), (33, 34, 65))
CASES = [(name, shape, 4) for name in ref.FAMILIES for shape in SHAPES] + \
        [(name, shape, 2) for name in ("softmax", "lattice", "specials") for shape in SHAPES]


@functools.lru_cache(maxsize=None)
def _case(name, shape, c):
    """(prob on the host [N, C, ...], label, posmask, the k of the case), made once and left unchanged"""
    prob, label, posmask = ref.family(name, shape, c=c)
    ks = tuple(ref.ks_of(ref.keys_of(prob, label, posmask)[2]))
    prob.setflags(write=False)
    label.setflags(write=False)
    return prob, label, posmask, ks


def _bits(t):
    return t.detach().cpu().contiguous().numpy().view(np.uint32)


def _device(prob, label):
    """channels-last probabilities [N, D0, D1, D2, C] and the labels on the device"""
    return torch.from_numpy(np.moveaxis(prob, 1, -1).copy()).to(DEV), torch.from_numpy(label.copy()).to(DEV)


def _forward_on_garbage(hip, prob_cl, lab, posmask, k, wt):
    """cwf_topk_ce through the C interface with a workspace filled with 0xFF bytes"""
    n, c = int(prob_cl.shape[0]), int(prob_cl.shape[-1])
    v = int(lab[0].numel())
    nbytes = hip.lib.cwf_topk_ce_workspace(n, v)
    assert nbytes >= 4 * n * v and nbytes % 256 == 0
    ws = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device=DEV)
    loss = torch.full((1,), float("nan"), device=DEV)
    coef = torch.full((4,), float("nan"), device=DEV)
    rc = hip.lib.cwf_topk_ce(prob_cl.data_ptr(), lab.data_ptr(), posmask, k, wt.data_ptr(), loss.data_ptr(), coef.data_ptr(), n, v, c,
                             ws.data_ptr(), hip._stream())
    assert rc == 0
    return loss, coef


@pytest.mark.parametrize("name,shape,c", CASES)
def test_selection_loss_and_gradient_against_the_statement(hip, name, shape, c):
    prob, label, posmask, ks = _case(name, shape, c)
    prob_cl, lab = _device(prob, label)
    assert len(ks) == 4 or name in ("softmax", "exponents", "specials")
    for k, w, gs in zip(ks, (1.0, 0.37, 2.5, 0.01), (1.0, -0.75, 1e-3, 3.0)):
        want = ref.topk_ce64(prob, label, k, w, posmask, gscale=gs)
        bound = ref.forward_bound(want["loss"], want["sabs"], w, k)
        wt = torch.full((1,), w, device=DEV)
        loss, coef = _forward_on_garbage(hip, prob_cl, lab, posmask, k, wt)
        loss2, coef2 = hip.topk_ce(prob_cl, lab, posmask, k, wt)                  # the backend route, workspace from the allocator
        got, cb = float(loss), _bits(coef)
        print("%s %s C=%d k=%d: tau %#x a %d n %d s %d loss %.9g ref %.9g |diff| %.3g bound %.3g"
              % (name, shape, c, k, want["tau"], want["a"], want["n"], want["s"], got, float(want["loss"]), abs(got - float(want["loss"])), bound))
        assert int(cb[2]) == want["tau"], (hex(int(cb[2])), hex(want["tau"]))
        assert np.array_equal(cb, want["coef"].view(np.uint32))                  # w / k, s / n, tau, +0: exactly
        assert abs(got - float(want["loss"])) <= bound
        assert float(want["loss"]) == 0.0 or abs(float(want["loss"])) > 1e3 * bound
        assert np.array_equal(_bits(loss2), _bits(loss)) and np.array_equal(_bits(coef2), cb)      # bit-identical between two calls
        d = hip.topk_ce_bwd(prob_cl, lab, posmask, coef, torch.full((1,), gs, device=DEV))
        assert np.array_equal(_bits(d.permute(0, 4, 1, 2, 3)), want["dprob"].view(np.uint32)), (name, shape, c, k)
    # no cross-sample leakage the other way round: the selection runs over the WHOLE batch, one sample alone selects differently
    if name == "softmax":
        k = ks[2]
        one = ref.topk_ce64(prob[:1], label[:1], k, 1.0, posmask)
        both = ref.topk_ce64(prob, label, k, 1.0, posmask)
        assert one["tau"] != both["tau"]
        _, coef = hip.topk_ce(prob_cl[:1].contiguous(), lab[:1].contiguous(), posmask, k, torch.ones(1, device=DEV))
        assert int(_bits(coef)[2]) == one["tau"]


def test_rejects_bad_arguments_without_a_launch(hip):
    L, s = hip.lib, hip._stream()
    assert L.cwf_topk_ce_workspace(0, 64) == -1 and L.cwf_topk_ce_workspace(1, 0) == -1 and L.cwf_topk_ce_workspace(-2, 64) == -1
    assert L.cwf_topk_ce_workspace(2, 1 << 40) == -2
    assert L.cwf_topk_ce_workspace(2, 210) == 49408 + 1792                       # histograms, state, slab + 4 B / voxel, 256-B aligned
    prob = torch.full((1, 4, 4, 4, 4), 0.25, device=DEV)
    lab = torch.zeros((1, 4, 4, 4), dtype=torch.int64, device=DEV)
    one = torch.ones(1, device=DEV)
    loss = torch.full((1,), -5.0, device=DEV)
    coef = torch.full((4,), -5.0, device=DEV)
    d = torch.full((1, 4, 4, 4, 4), -5.0, device=DEV)
    ws = torch.full((L.cwf_topk_ce_workspace(1, 64) + 256,), 0xFF, dtype=torch.uint8, device=DEV)
    ws = ws[(-ws.data_ptr()) % 256:]
    assert ws.data_ptr() % 256 == 0
    fw, bw = L.cwf_topk_ce, L.cwf_topk_ce_bwd
    p, l, o, ls, cf, w = prob.data_ptr(), lab.data_ptr(), one.data_ptr(), loss.data_ptr(), coef.data_ptr(), ws.data_ptr()
    assert fw(0, l, 0, 6, o, ls, cf, 1, 64, 4, w, s) == -1 and fw(p, 0, 0, 6, o, ls, cf, 1, 64, 4, w, s) == -1
    assert fw(p, l, 0, 6, 0, ls, cf, 1, 64, 4, w, s) == -1 and fw(p, l, 0, 6, o, 0, cf, 1, 64, 4, w, s) == -1
    assert fw(p, l, 0, 6, o, ls, 0, 1, 64, 4, w, s) == -1 and fw(p, l, 0, 6, o, ls, cf, 1, 64, 4, 0, s) == -1
    assert fw(p, l, 0, 6, o, ls, cf, 1, 64, 3, w, s) == -1 and fw(p, l, 0, 6, o, ls, cf, 1, 64, 1, w, s) == -1       # C
    assert fw(p, l, 0, 0, o, ls, cf, 1, 64, 4, w, s) == -1 and fw(p, l, 0, 65, o, ls, cf, 1, 64, 4, w, s) == -1      # k
    assert fw(p, l, 0, -3, o, ls, cf, 1, 64, 4, w, s) == -1
    assert fw(p, l, 0, 6, o, ls, cf, 0, 64, 4, w, s) == -1 and fw(p, l, 0, 6, o, ls, cf, 1, 0, 4, w, s) == -1        # N, V
    assert fw(p, l, 0, 6, o, ls, cf, 1, 64, 4, w + 8, s) == -3                                                       # alignment
    g = one.data_ptr()
    assert bw(0, l, 0, cf, g, d.data_ptr(), 1, 64, 4, s) == -1 and bw(p, 0, 0, cf, g, d.data_ptr(), 1, 64, 4, s) == -1
    assert bw(p, l, 0, 0, g, d.data_ptr(), 1, 64, 4, s) == -1 and bw(p, l, 0, cf, 0, d.data_ptr(), 1, 64, 4, s) == -1
    assert bw(p, l, 0, cf, g, 0, 1, 64, 4, s) == -1 and bw(p, l, 0, cf, g, d.data_ptr(), 1, 64, 5, s) == -1
    assert bw(p, l, 0, cf, g, d.data_ptr(), 0, 64, 4, s) == -1 and bw(p, l, 0, cf, g, d.data_ptr(), 1, 0, 4, s) == -1
    torch.cuda.synchronize()
    assert bool((loss == -5.0).all()) and bool((coef == -5.0).all()) and bool((d == -5.0).all())     # nothing was launched
    assert bool((ws == 0xFF).all())
    # the backend makes the same checks boundary_loss makes, before any call
    with pytest.raises(ValueError):
        hip.topk_ce(prob, lab, 0, 0, one)
    with pytest.raises(ValueError):
        hip.topk_ce(prob, lab, 0, 65, one)
    with pytest.raises(ValueError):
        hip.topk_ce(prob, lab, 0, 6, torch.ones(2, device=DEV))
    with pytest.raises(ValueError):
        hip.topk_ce(prob, lab, 0, 6, torch.ones(1, dtype=torch.float64, device=DEV))
    with pytest.raises(ValueError):
        hip.topk_ce(prob, lab, 0, 6, torch.ones(1))
    with pytest.raises(ValueError):
        hip.topk_ce(prob, lab.int(), 0, 6, one)
    with pytest.raises(ValueError):
        hip.topk_ce(torch.zeros((1, 4, 4, 4, 3), device=DEV), lab, 0, 6, one)
    with pytest.raises(ValueError):
        hip.topk_ce(prob, lab[:, :2], 0, 6, one)


def test_autograd_gradient_alone_and_summed_with_dice_ce(hip):
    """(5, 6, 7): one workgroup per sample in the Dice / CE sums, so that term's gradient is the same bits on every run"""
    from cwf import functional as CF
    from utils import tools
    prob, label, posmask, ks = _case("lattice", (5, 6, 7), 4)
    prob_cl, lab = _device(prob, label)
    m = label.size
    want = ref.topk_ce64(prob, label, ref.topk_count(m, 10.0), 0.2)
    want25 = ref.topk_ce64(prob, label, ref.topk_count(m, 25.0), 1.0)

    def grad(f):
        leaf = prob_cl.clone().requires_grad_(True)
        out = f(leaf.permute(0, 4, 1, 2, 3))
        out.backward()
        return out.detach(), leaf.grad

    loss, gt = grad(lambda p: tools.topk_ce(p, lab, weight=0.2))
    assert abs(float(loss) - float(want["loss"])) <= ref.forward_bound(want["loss"], want["sabs"], 0.2, ref.topk_count(m, 10.0))
    assert np.array_equal(_bits(gt.permute(0, 4, 1, 2, 3)), want["dprob"].view(np.uint32))
    loss, g25 = grad(lambda p: tools.topk_ce(p, lab, percent=25.0, weight=torch.ones(1, device=DEV)))
    assert np.array_equal(_bits(g25.permute(0, 4, 1, 2, 3)), want25["dprob"].view(np.uint32))
    _, gd = grad(lambda p: CF.dice_ce_loss(p, lab))
    _, both = grad(lambda p: tools.dice_ce(p, lab) + tools.topk_ce(p, lab, weight=0.2))
    assert torch.equal(both, gd + gt) and float(gd.abs().max()) > 0
    # C = 2 with a posmask through the public name
    prob2, label2, posmask2, _ = _case("lattice", (5, 6, 7), 2)
    p2, l2 = _device(prob2, label2)
    leaf = p2.clone().requires_grad_(True)
    tools.topk_ce(leaf.permute(0, 4, 1, 2, 3), l2, weight=0.2, posmask=posmask2).backward()
    want2 = ref.topk_ce64(prob2, label2, ref.topk_count(m, 10.0), 0.2, posmask2)
    assert np.array_equal(_bits(leaf.grad.permute(0, 4, 1, 2, 3)), want2["dprob"].view(np.uint32))


def test_drop_in_names(hip):
    from models import criterions
    from utils import tools
    prob, label, posmask, ks = _case("softmax", (5, 6, 7), 4)
    prob_cl, lab = _device(prob, label)
    p = prob_cl.permute(0, 4, 1, 2, 3)
    k = ref.topk_count(label.size, 10.0)
    want = ref.topk_ce64(prob, label, k, 1.0)
    bound = ref.forward_bound(want["loss"], want["sabs"], 1.0, k)
    assert abs(float(tools.topk_ce(p, lab)) - float(want["loss"])) <= bound
    assert abs(float(criterions.topk_ce(p, lab)) - float(want["loss"])) <= bound
    a, b = float(criterions.softmax_dice(p, lab)), float(criterions.topk_ce(p, lab))
    both = float(criterions.softmax_dice_topk(p, lab))
    assert abs(both - (a + b)) <= 1e-6 * abs(a + b) and b > 0
    with pytest.raises(ValueError):
        tools.topk_ce(p, lab, percent=0.0)


# ------------------------------------------------------------------------------------------------------------------ Trainer
def _record_main_output(monkeypatch):
    """total_loss as it is, remembering the main output it was given (in a captured step that tensor is the step's static buffer)"""
    from cwf import trainer
    seen = {}
    orig = trainer.total_loss

    def wrapped(outputs, target, edge, boundary=None, **kw):
        seen["out"] = outputs[0].detach()
        seen["kw"] = dict(kw)
        return orig(outputs, target, edge, boundary, **kw)
    monkeypatch.setattr(trainer, "total_loss", wrapped)
    return seen


def _topk_part_reference(out, target, w, percent=10.0):
    p = out.detach().cpu().contiguous().numpy()
    t = target.cpu().numpy()
    k = ref.topk_count(t.size, percent)
    want = ref.topk_ce64(p, t, k, w)
    return float(want["loss"]), ref.forward_bound(want["loss"], want["sabs"], w, k)


def test_trainer_without_the_term_makes_no_new_call(hip, monkeypatch):
    from cwf import kernels, trainer
    from cwf.trainer import Trainer
    forced, batch = _batch()

    def boom(*a, **k):
        raise AssertionError("the top-k kernels were called with the term off")
    for name in ("topk_ce", "topk_ce_bwd"):
        monkeypatch.setattr(hip, name, boom)
    orig = trainer.total_loss
    calls = []

    def old_signature(outputs, target, edge, boundary=None):                     # what wrappers written before this term look like
        calls.append(boundary)
        return orig(outputs, target, edge, boundary)
    monkeypatch.setattr(trainer, "total_loss", old_signature)
    kernels.set_precision("bf16x3")
    try:
        tr = Trainer(_no_dropout_model(forced))
        loss, parts = tr.step(*batch, 0)
        torch.cuda.synchronize()
        assert len(parts) == 5 and tr._topk is None and tr._boundary is None and bool(torch.isfinite(loss)) and calls == [None]
        with pytest.raises(ValueError):
            tr.set_topk_weight(0.1)
    finally:
        kernels.set_precision("fp32")


def test_trainer_with_the_term_eager_and_plan(hip, monkeypatch):
    """64^3, B = 1, top-k token indices teacher-forced, dropout off, learning rate 0 (the weights stay where they are, so every step
    sees the same problem).  The new part against the statement on the step's own main output within the forward bound; the flat
    gradient moved by more than 100 x the eager-against-eager spread; the plan step's flat gradient against the eager step's within
    max(5e-5, 10 x that spread), the bound of the existing replay tests; set_topk_weight after capture changes the part on the next
    plan step with the plan left as it is."""
    from cwf import kernels
    from cwf.trainer import Trainer
    from utils import tools
    forced, batch = _batch()
    seen = _record_main_output(monkeypatch)
    kernels.set_precision("bf16x3")
    try:
        eager = []
        for rep in range(2):
            tr = Trainer(_no_dropout_model(forced), lr=0.0, weight_decay=0.0, topk_weight=0.5)
            loss, parts = tr._fwd_bwd(*batch)
            torch.cuda.synchronize()
            eager.append(tr.opt.flat_grad.clone())
            assert len(parts) == 6 and set(seen["kw"]) == {"topk"} and seen["kw"]["topk"][1] == 10.0
            want, bound = _topk_part_reference(seen["out"], batch[1], 0.5)
            again = float(tools.topk_ce(seen["out"], batch[1], weight=0.5))
            print("eager top-k part %.9g tools %.9g ref %.9g bound %.3g" % (float(parts[5]), again, want, bound))
            assert abs(float(parts[5]) - want) <= bound and again == float(parts[5]) and abs(want) > 1e3 * bound
            total = sum(float(p) for p in parts)
            assert abs(float(loss) - total) <= 1e-6 * abs(total)
        noise = float((eager[0] - eager[1]).norm() / eager[0].norm())
        # the term reaches the gradient: without it the flat gradient is another one
        tr0 = Trainer(_no_dropout_model(forced), lr=0.0, weight_decay=0.0)
        tr0._fwd_bwd(*batch)
        torch.cuda.synchronize()
        assert seen["kw"] == {}
        moved = float((tr0.opt.flat_grad - eager[0]).norm() / eager[0].norm())
        print("flat gradient moved by %.3g, eager vs eager %.3g" % (moved, noise))
        assert moved > 100 * max(noise, 1e-7), (moved, noise)

        tr = Trainer(_no_dropout_model(forced), lr=0.0, weight_decay=0.0, use_graph="plan", topk_weight=0.5)
        tr._fwd_bwd(*batch)                                                      # eager warm-up (allocations, weight-pack tables)
        tr._finish_comm()
        torch.cuda.synchronize()
        tr._capture(*batch)
        assert tr._plan is not None, tr.plan_info
        plan = tr._plan.value
        loss, parts = tr.step(*batch, 0)
        torch.cuda.synchronize()
        assert len(parts) == 6
        diff = float((tr.opt.flat_grad - eager[0]).norm() / eager[0].norm())
        print("plan vs eager flat gradient %.3g, eager vs eager %.3g" % (diff, noise))
        assert diff < max(5e-5, 10 * noise), (diff, noise)
        want, bound = _topk_part_reference(seen["out"], batch[1], 0.5)
        p6 = float(parts[5])
        assert abs(p6 - want) <= bound

        tr.set_topk_weight(1.0)
        loss, parts = tr.step(*batch, 0)
        torch.cuda.synchronize()
        assert tr._plan.value == plan and len(parts) == 6
        want2, bound2 = _topk_part_reference(seen["out"], batch[1], 1.0)
        print("plan top-k part: %.9g at 0.5, %.9g at 1.0 (ref %.9g, bound %.3g)" % (p6, float(parts[5]), want2, bound2))
        assert abs(float(parts[5]) - want2) <= bound2
        assert abs(float(parts[5]) - 2.0 * p6) <= 1e-4 * abs(2.0 * p6)           # doubled (same weights: lr = 0)
    finally:
        kernels.set_precision("fp32")


def test_trainer_with_boundary_and_topk_has_seven_parts_in_order(hip, monkeypatch):
    from cwf import kernels
    from cwf.trainer import Trainer
    forced, batch = _batch()
    seen = _record_main_output(monkeypatch)
    kernels.set_precision("bf16x3")
    try:
        tr = Trainer(_no_dropout_model(forced), lr=0.0, weight_decay=0.0, boundary_weight=0.01, topk_weight=0.5, topk_percent=5.0)
        loss, parts = tr._fwd_bwd(*batch)
        torch.cuda.synchronize()
        assert len(parts) == 7
        want, bound = _topk_part_reference(seen["out"], batch[1], 0.5, percent=5.0)
        assert abs(float(parts[6]) - want) <= bound
        phi = boundary_ref.signed_distance(batch[1].cpu().numpy(), use_scipy=True)
        p = seen["out"].detach().cpu().contiguous().numpy()
        bw, sabs, _ = boundary_ref.boundary_loss64(p, phi, boundary_ref.REGION_MASKS, 0.01)
        assert abs(float(parts[5]) - float(bw)) <= boundary_ref.forward_bound(bw, sabs, 0.01, 1, 3, int(np.prod(p.shape[2:])))
        assert abs(float(parts[5]) - float(parts[6])) > 10 * bound              # (the two parts are not the same number)
        total = sum(float(q) for q in parts)
        assert abs(float(loss) - total) <= 1e-6 * abs(total)
    finally:
        kernels.set_precision("fp32")
