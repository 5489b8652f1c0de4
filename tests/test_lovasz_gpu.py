"""The Lovasz-Softmax term on the GPU (csrc/lovasz.hip and its way up through cwf.kernels, cwf.functional, utils.tools,
models.criterions and cwf.trainer.Trainer): coef, the per-voxel coefficients and the gradient bit-equal to the statement, the loss
within its derived bound and bit-identical from call to call, and the Trainer with the term off and on.
Yardstick: tests/lovasz_ref.py."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import lovasz_ref as ref
from test_boundary_gpu import _batch, _no_dropout_model          # the 64^3 teacher-forced recipe and its cached batch, shared

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# M = 420: less than one workgroup, ragged; M = 145,860: many workgroups, odd extents, digit buckets beyond 16 bits
SHAPES = ((5, 6, 7), (33, 34, 65))
MASKSETS = {"classes": ref.CLASS_MASKS, "regions": ref.REGION_MASKS}
CASES = [(name, shape, "classes", True) for name in ref.FAMILIES for shape in SHAPES] + \
        [(name, shape, "regions", True) for name in ("softmax", "lattice") for shape in SHAPES] + \
        [("absent", shape, "classes", False) for shape in SHAPES]
GSCALES = (1.0, -0.75, 3e-3)


@functools.lru_cache(maxsize=None)
def _case(name, shape):
    """(prob on the host [N, 4, ...], label), made once and left unchanged"""
    prob, label = ref.family(name, shape)
    prob.setflags(write=False)
    label.setflags(write=False)
    return prob, label


@functools.lru_cache(maxsize=None)
def _want(name, shape, maskset, only_present, w, gs):
    prob, label = _case(name, shape)
    return ref.lovasz64(prob, label, MASKSETS[maskset], only_present, w=w, gscale=gs)


def _bits(t):
    return t.detach().cpu().contiguous().numpy().view(np.uint32)


def _device(prob, label):
    """channels-last probabilities [N, D0, D1, D2, 4] and the labels on the device"""
    return torch.from_numpy(np.moveaxis(prob, 1, -1).copy()).to(DEV), torch.from_numpy(label.copy()).to(DEV)


def _cmasks(masks):
    return (ctypes.c_uint32 * len(masks))(*masks)


def _forward_on_garbage(hip, prob_cl, lab, masks, only_present, wt):
    """cwf_lovasz through the C interface with a workspace filled with 0xFF bytes"""
    n, v, r = int(prob_cl.shape[0]), int(lab[0].numel()), len(masks)
    nbytes = hip.lib.cwf_lovasz_workspace(n, v, r)
    assert nbytes >= 8 * r * n * v and nbytes % 256 == 0
    ws = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device=DEV)
    loss = torch.full((1,), float("nan"), device=DEV)
    coef = torch.full((4,), float("nan"), device=DEV)
    vcoef = torch.full((r, n * v), float("nan"), device=DEV)
    cm = _cmasks(masks)
    rc = hip.lib.cwf_lovasz(prob_cl.data_ptr(), lab.data_ptr(), ctypes.addressof(cm), r, int(only_present), wt.data_ptr(), loss.data_ptr(),
                            coef.data_ptr(), vcoef.data_ptr(), n, v, ws.data_ptr(), hip._stream())
    assert rc == 0
    return loss, coef, vcoef


@pytest.mark.parametrize("name,shape,maskset,only_present", CASES)
def test_coefficients_loss_and_gradient_against_the_statement(hip, name, shape, maskset, only_present):
    prob, label = _case(name, shape)
    masks = MASKSETS[maskset]
    prob_cl, lab = _device(prob, label)
    w = 0.37 if name == "lattice" else 1.0
    want = _want(name, shape, maskset, only_present, w, GSCALES[0])
    bound = ref.forward_bound(want["loss"], label.size)
    wt = torch.full((1,), w, device=DEV)
    loss, coef, vcoef = _forward_on_garbage(hip, prob_cl, lab, masks, only_present, wt)
    loss2, coef2, vcoef2 = hip.lovasz(prob_cl, lab, masks, only_present, wt)          # the backend route, workspace from the allocator
    got = float(loss)
    print("%s %s %s only_present=%s: P %d G %s loss %.9g ref %.9g |diff| %.3g bound %.3g"
          % (name, shape, maskset, only_present, want["P"], want["G"], got, float(want["loss"]), abs(got - float(want["loss"])), bound))
    assert np.array_equal(_bits(coef), want["coef"].view(np.uint32))                   # w / P, P, +0, +0: exactly
    bad = np.flatnonzero(_bits(vcoef).reshape(-1) != want["vcoef"].view(np.uint32).reshape(-1))
    assert bad.size == 0, (bad.size, bad[:8], vcoef.reshape(-1)[torch.from_numpy(bad[:8]).to(DEV)], want["vcoef"].reshape(-1)[bad[:8]])
    assert abs(got - float(want["loss"])) <= bound
    assert float(want["loss"]) == 0.0 or abs(float(want["loss"])) > 1e3 * bound
    if name == "perfect":
        assert _bits(loss)[0] == 0 and not _bits(vcoef).any()                         # +0, and no gradient anywhere
    assert np.array_equal(_bits(loss2), _bits(loss)) and np.array_equal(_bits(coef2), _bits(coef))      # bit-identical between two calls
    assert torch.equal(vcoef2.view(torch.int32), vcoef.view(torch.int32))
    for gs in GSCALES:
        wantg = _want(name, shape, maskset, only_present, w, gs)
        d = hip.lovasz_bwd(vcoef, masks, coef, torch.full((1,), gs, device=DEV), tuple(prob_cl.shape))
        assert np.array_equal(_bits(d.permute(0, 4, 1, 2, 3)), wantg["dprob"].view(np.uint32)), (name, shape, gs)
        if name == "perfect":
            assert not bool(d.any())


def test_the_sort_runs_over_the_whole_batch(hip):
    prob, label = _case("softmax", (5, 6, 7))
    prob_cl, lab = _device(prob, label)
    one = ref.lovasz64(prob[:1], label[:1])
    both = ref.lovasz64(prob, label)
    m1 = label[0].size
    assert not np.array_equal(one["vcoef"], both["vcoef"][:, :m1])
    wt = torch.ones(1, device=DEV)
    _, coef, vcoef = hip.lovasz(prob_cl[:1].contiguous(), lab[:1].contiguous(), ref.CLASS_MASKS, True, wt)
    assert np.array_equal(_bits(vcoef), one["vcoef"].view(np.uint32)) and np.array_equal(_bits(coef), one["coef"].view(np.uint32))
    _, coef, vcoef = hip.lovasz(prob_cl, lab, ref.CLASS_MASKS, True, wt)
    assert np.array_equal(_bits(vcoef), both["vcoef"].view(np.uint32))


def test_rejects_bad_arguments_without_a_launch(hip):
    L, s = hip.lib, hip._stream()
    W = L.cwf_lovasz_workspace
    assert W(0, 64, 4) == -1 and W(1, 0, 4) == -1 and W(-2, 64, 4) == -1 and W(1, 64, 0) == -1 and W(1, 64, 9) == -1
    assert W(2, 1 << 30, 4) == -2 and W(1, 1 << 31, 1) == -2 and W(1, (1 << 31) - 1, 1) > 0
    # two key arrays (4 regions x (432 + 16) keys), the digit counts of one tile (4 x 256 x 4 B), totals (8 KiB), partials (64 KiB), the
    # search tree (4 regions x two padded levels of 48 + 32 keys)
    assert W(2, 210, 4) == 2 * 7168 + 4096 + 8192 + 65536 + 1280
    prob = torch.full((1, 4, 4, 4, 4), 0.25, device=DEV)
    lab = torch.zeros((1, 4, 4, 4), dtype=torch.int64, device=DEV)
    one = torch.ones(1, device=DEV)
    loss = torch.full((1,), -5.0, device=DEV)
    coef = torch.full((4,), -5.0, device=DEV)
    vc = torch.full((4, 64), -5.0, device=DEV)
    d = torch.full((1, 4, 4, 4, 4), -5.0, device=DEV)
    ws = torch.full((W(1, 64, 4) + 256,), 0xFF, dtype=torch.uint8, device=DEV)
    ws = ws[(-ws.data_ptr()) % 256:]
    assert ws.data_ptr() % 256 == 0
    fw, bw = L.cwf_lovasz, L.cwf_lovasz_bwd
    good, zero, big = _cmasks((1, 2, 4, 8)), _cmasks((1, 0, 4, 8)), _cmasks((1, 2, 4, 16))
    m, z, b = ctypes.addressof(good), ctypes.addressof(zero), ctypes.addressof(big)
    p, l, o, ls, cf, v, w = prob.data_ptr(), lab.data_ptr(), one.data_ptr(), loss.data_ptr(), coef.data_ptr(), vc.data_ptr(), ws.data_ptr()
    for args in ((0, l, m, 4, 1, o, ls, cf, v, 1, 64, w), (p, 0, m, 4, 1, o, ls, cf, v, 1, 64, w), (p, l, 0, 4, 1, o, ls, cf, v, 1, 64, w),
                 (p, l, m, 4, 1, 0, ls, cf, v, 1, 64, w), (p, l, m, 4, 1, o, 0, cf, v, 1, 64, w), (p, l, m, 4, 1, o, ls, 0, v, 1, 64, w),
                 (p, l, m, 4, 1, o, ls, cf, 0, 1, 64, w), (p, l, m, 4, 1, o, ls, cf, v, 1, 64, 0),                      # null pointers
                 (p, l, m, 0, 1, o, ls, cf, v, 1, 64, w), (p, l, m, 9, 1, o, ls, cf, v, 1, 64, w),                      # R
                 (p, l, z, 4, 1, o, ls, cf, v, 1, 64, w), (p, l, b, 4, 1, o, ls, cf, v, 1, 64, w),                      # a mask outside 1..15
                 (p, l, m, 4, 1, o, ls, cf, v, 0, 64, w), (p, l, m, 4, 1, o, ls, cf, v, 1, 0, w)):                      # N, V
        assert fw(*args, s) == -1, args
    assert fw(p, l, m, 4, 1, o, ls, cf, v, 1, 1 << 31, w, s) == -2                                                       # 32-bit positions
    assert fw(p, l, m, 4, 1, o, ls, cf, v, 1, 64, w + 8, s) == -3                                                        # alignment
    g, dp = one.data_ptr(), d.data_ptr()
    for args in ((0, m, 4, cf, g, dp, 1, 64), (v, 0, 4, cf, g, dp, 1, 64), (v, m, 4, 0, g, dp, 1, 64), (v, m, 4, cf, 0, dp, 1, 64),
                 (v, m, 4, cf, g, 0, 1, 64), (v, m, 0, cf, g, dp, 1, 64), (v, m, 9, cf, g, dp, 1, 64), (v, z, 4, cf, g, dp, 1, 64),
                 (v, b, 4, cf, g, dp, 1, 64), (v, m, 4, cf, g, dp, 0, 64), (v, m, 4, cf, g, dp, 1, 0)):
        assert bw(*args, s) == -1, args
    assert bw(v, m, 4, cf, g, dp, 1, 1 << 31, s) == -2 and bw(v, m, 4, cf, g, dp + 4, 1, 64, s) == -3
    torch.cuda.synchronize()
    assert bool((loss == -5.0).all()) and bool((coef == -5.0).all()) and bool((vc == -5.0).all()) and bool((d == -5.0).all())
    assert bool((ws == 0xFF).all())                                               # nothing was launched
    # the backend makes the same checks, before any call
    for bad in (lambda: hip.lovasz(prob, lab, (), True, one), lambda: hip.lovasz(prob, lab, (1, 16), True, one),
                lambda: hip.lovasz(prob, lab, (1,) * 9, True, one), lambda: hip.lovasz(prob, lab, (1, 2), 1, one),
                lambda: hip.lovasz(prob, lab, (1, 2), True, torch.ones(2, device=DEV)),
                lambda: hip.lovasz(prob, lab, (1, 2), True, torch.ones(1, dtype=torch.float64, device=DEV)),
                lambda: hip.lovasz(prob, lab, (1, 2), True, torch.ones(1)), lambda: hip.lovasz(prob, lab.int(), (1, 2), True, one),
                lambda: hip.lovasz(torch.zeros((1, 4, 4, 4, 3), device=DEV), lab, (1, 2), True, one),
                lambda: hip.lovasz(prob, lab[:, :2], (1, 2), True, one),
                lambda: hip.lovasz_bwd(vc, (1, 2), coef, one, (1, 4, 4, 4, 4)),
                lambda: hip.lovasz_bwd(vc, (1, 2, 4, 8), coef[:2], one, (1, 4, 4, 4, 4)),
                lambda: hip.lovasz_bwd(vc, (1, 2, 4, 8), coef, one, (1, 4, 4, 4, 3))):
        with pytest.raises(ValueError):
            bad()


def test_autograd_gradient_alone_and_summed_with_dice_ce(hip):
    """(5, 6, 7): one workgroup per sample in the Dice / CE sums, so that term's gradient is the same bits on every run"""
    from cwf import functional as CF
    from utils import tools
    prob, label = _case("lattice", (5, 6, 7))
    prob_cl, lab = _device(prob, label)
    want = ref.lovasz64(prob, label, w=0.2)
    wantr = ref.lovasz64(prob, label, ref.REGION_MASKS, only_present=False, w=1.0)

    def grad(f):
        leaf = prob_cl.clone().requires_grad_(True)
        out = f(leaf.permute(0, 4, 1, 2, 3))
        out.backward()
        return out.detach(), leaf.grad

    loss, gt = grad(lambda p: tools.lovasz_softmax(p, lab, weight=0.2))
    assert abs(float(loss) - float(want["loss"])) <= ref.forward_bound(want["loss"], label.size)
    assert np.array_equal(_bits(gt.permute(0, 4, 1, 2, 3)), want["dprob"].view(np.uint32)) and float(gt.abs().max()) > 0
    loss, gr = grad(lambda p: tools.lovasz_softmax(p, lab, posmasks=CF.REGION_MASKS, only_present=False, weight=torch.ones(1, device=DEV)))
    assert np.array_equal(_bits(gr.permute(0, 4, 1, 2, 3)), wantr["dprob"].view(np.uint32))
    _, gd = grad(lambda p: CF.dice_ce_loss(p, lab))
    _, both = grad(lambda p: tools.dice_ce(p, lab) + tools.lovasz_softmax(p, lab, weight=0.2))
    assert torch.equal(both, gd + gt) and float(gd.abs().max()) > 0


def test_drop_in_names(hip):
    from models import criterions
    from utils import tools
    prob, label = _case("softmax", (5, 6, 7))
    prob_cl, lab = _device(prob, label)
    p = prob_cl.permute(0, 4, 1, 2, 3)
    want = ref.lovasz64(prob, label)
    bound = ref.forward_bound(want["loss"], label.size)
    assert abs(float(tools.lovasz_softmax(p, lab)) - float(want["loss"])) <= bound
    assert abs(float(criterions.lovasz_softmax(p, lab)) - float(want["loss"])) <= bound
    a, b = float(criterions.softmax_dice(p, lab)), float(criterions.lovasz_softmax(p, lab))
    both = float(criterions.softmax_dice_lovasz(p, lab))
    assert abs(both - (a + b)) <= 1e-6 * abs(a + b) and b > 0
    with pytest.raises(ValueError):
        tools.lovasz_softmax(p, lab, posmasks=(0,))


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


def _part_reference(out, target, w, masks=ref.CLASS_MASKS):
    want = ref.lovasz64(out.detach().cpu().contiguous().numpy(), target.cpu().numpy(), masks, w=w)
    return float(want["loss"]), ref.forward_bound(want["loss"], int(target.numel()))


def test_trainer_without_the_term_makes_no_new_call(hip, monkeypatch):
    from cwf import kernels, trainer
    from cwf.trainer import Trainer
    forced, batch = _batch()

    def boom(*a, **k):
        raise AssertionError("the Lovasz kernels were called with the term off")
    for name in ("lovasz", "lovasz_bwd"):
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
        assert len(parts) == 5 and tr._lovasz is None and bool(torch.isfinite(loss)) and calls == [None]
        with pytest.raises(ValueError):
            tr.set_lovasz_weight(0.1)
    finally:
        kernels.set_precision("fp32")


def test_trainer_with_the_term_eager_and_plan(hip, monkeypatch):
    """64^3, B = 1, top-k token indices teacher-forced, dropout off, learning rate 0 (the weights stay where they are, so every step
    sees the same problem).  The new part, appended last, against the statement on the step's own main output within the forward
    bound; the flat gradient moved by more than 100 x the eager-against-eager spread; the plan step's flat gradient against the eager
    step's within max(5e-5, 10 x that spread), the bound of the existing replay tests; set_lovasz_weight after capture changes the part
    on the next plan step with the plan left as it is."""
    from cwf import kernels
    from cwf.trainer import Trainer
    from utils import tools
    forced, batch = _batch()
    seen = _record_main_output(monkeypatch)
    kernels.set_precision("bf16x3")
    try:
        eager = []
        for rep in range(2):
            tr = Trainer(_no_dropout_model(forced), lr=0.0, weight_decay=0.0, lovasz_weight=0.5)
            loss, parts = tr._fwd_bwd(*batch)
            torch.cuda.synchronize()
            eager.append(tr.opt.flat_grad.clone())
            assert len(parts) == 6 and set(seen["kw"]) == {"lovasz"} and seen["kw"]["lovasz"][1:] == (ref.CLASS_MASKS, True)
            want, bound = _part_reference(seen["out"], batch[1], 0.5)
            again = float(tools.lovasz_softmax(seen["out"], batch[1], weight=0.5))
            print("eager Lovasz part %.9g tools %.9g ref %.9g bound %.3g" % (float(parts[5]), again, want, bound))
            assert abs(float(parts[5]) - want) <= bound and again == float(parts[5]) and abs(want) > 1e3 * bound
            total = sum(float(p) for p in parts)
            assert abs(float(loss) - total) <= 1e-6 * abs(total)
        noise = float((eager[0] - eager[1]).norm() / eager[0].norm())
        # the term reaches the gradient: without it the flat gradient is another one
        tr0 = Trainer(_no_dropout_model(forced), lr=0.0, weight_decay=0.0)
        _, parts0 = tr0._fwd_bwd(*batch)
        torch.cuda.synchronize()
        assert seen["kw"] == {} and len(parts0) == 5
        moved = float((tr0.opt.flat_grad - eager[0]).norm() / eager[0].norm())
        print("flat gradient moved by %.3g, eager vs eager %.3g" % (moved, noise))
        assert moved > 100 * max(noise, 1e-7), (moved, noise)

        tr = Trainer(_no_dropout_model(forced), lr=0.0, weight_decay=0.0, use_graph="plan", lovasz_weight=0.5)
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
        want, bound = _part_reference(seen["out"], batch[1], 0.5)
        p6 = float(parts[5])
        assert abs(p6 - want) <= bound

        tr.set_lovasz_weight(1.0)
        loss, parts = tr.step(*batch, 0)
        torch.cuda.synchronize()
        assert tr._plan.value == plan and len(parts) == 6
        want2, bound2 = _part_reference(seen["out"], batch[1], 1.0)
        print("plan Lovasz part: %.9g at 0.5, %.9g at 1.0 (ref %.9g, bound %.3g)" % (p6, float(parts[5]), want2, bound2))
        assert abs(float(parts[5]) - want2) <= bound2
        assert abs(float(parts[5]) - 2.0 * p6) <= 1e-4 * abs(2.0 * p6)           # doubled (same weights: lr = 0)
    finally:
        kernels.set_precision("fp32")


def test_trainer_with_focal_and_lovasz_on_the_regions_has_seven_parts_in_order(hip, monkeypatch):
    from cwf import kernels
    from cwf.trainer import Trainer
    forced, batch = _batch()
    seen = _record_main_output(monkeypatch)
    kernels.set_precision("bf16x3")
    try:
        tr = Trainer(_no_dropout_model(forced), lr=0.0, weight_decay=0.0, focal_weight=0.3, lovasz_weight=0.5, lovasz_regions="regions")
        loss, parts = tr._fwd_bwd(*batch)
        torch.cuda.synchronize()
        assert len(parts) == 7 and list(seen["kw"]) == ["focal", "lovasz"]
        want, bound = _part_reference(seen["out"], batch[1], 0.5, ref.REGION_MASKS)
        assert abs(float(parts[6]) - want) <= bound and abs(float(parts[5]) - float(parts[6])) > 10 * bound
        total = sum(float(q) for q in parts)
        assert abs(float(loss) - total) <= 1e-6 * abs(total)
    finally:
        kernels.set_precision("fp32")


def test_trainer_with_all_four_supplementary_terms_has_nine_parts_in_order(hip, monkeypatch):
    """64^3, B = 1, top-k token indices teacher-forced, dropout off, learning rate 0, one eager forward and backward with the boundary,
    top-k, focal and Lovasz terms on together: each of the four appended parts is bit-equal to its utils.tools call on the step's own
    main output with the same options (the forwards are deterministic; the boundary sum's float64 atomics differ by their order only
    in bits that the one rounding to float32 drops), the four are different numbers, and the total is the sum of the nine."""
    from cwf import kernels
    from cwf.trainer import Trainer
    from utils import tools
    forced, batch = _batch()
    seen = _record_main_output(monkeypatch)
    kernels.set_precision("bf16x3")
    try:
        tr = Trainer(_no_dropout_model(forced), lr=0.0, weight_decay=0.0, boundary_weight=0.01, topk_weight=0.5, topk_percent=5.0,
                     focal_weight=0.25, focal_params=dict(gamma=3.0), lovasz_weight=0.5, lovasz_regions="regions")
        loss, parts = tr._fwd_bwd(*batch)
        torch.cuda.synchronize()
        assert len(parts) == 9 and list(seen["kw"]) == ["topk", "focal", "lovasz"]
        out, target = seen["out"], batch[1]
        again = [float(tools.boundary_loss(out, target, weight=0.01)), float(tools.topk_ce(out, target, percent=5.0, weight=0.5)),
                 float(tools.focal_loss(out, target, gamma=3.0, weight=0.25)),
                 float(tools.lovasz_softmax(out, target, posmasks=ref.REGION_MASKS, weight=0.5))]
        got = [float(p) for p in parts[5:]]
        print("parts 6-9 %s, tools %s" % (["%.9g" % g for g in got], ["%.9g" % a for a in again]))
        assert got == again
        assert len(set(got)) == 4                                                # four different numbers
        total = sum(float(p) for p in parts)
        assert abs(float(loss) - total) <= 1e-6 * abs(total)
    finally:
        kernels.set_precision("fp32")
