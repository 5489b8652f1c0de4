"""The focal Tversky + focal cross-entropy term on the GPU (csrc/focal.hip and its way up through cwf.kernels, cwf.functional,
utils.tools, models.criterions and cwf.trainer.Trainer): the loss and the coefficient table within their derived bounds and
bit-identical from call to call, the gradient per element within its bound of the float64 gradient formed from the device's own
coefficients, everything bit-equal to the statement where no device function enters, and the Trainer with the term off and on.
Yardstick: tests/focal_ref.py."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import boundary_ref
import focal_ref as ref
import topk_ref
from test_boundary_gpu import _batch, _no_dropout_model          # the 64^3 teacher-forced recipe and its cached batch, shared

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
# M = 420: less than one workgroup's tile, ragged; M = 145,860: 143 workgroups, odd extents, a ragged last one
CASES = [(name, shape) for name in ref.FAMILIES for shape in ref.SHAPES]
WEIGHT = 0.37
GSCALES = (1.0, -0.75, 1e-3)


@functools.lru_cache(maxsize=None)
def _case(name, shape):
    prob, label = ref.family(name, shape)
    prob.setflags(write=False)
    label.setflags(write=False)
    return prob, label


@functools.lru_cache(maxsize=None)
def _statement(name, shape, pset):
    """the statement of one (family, shape, parameter set) at WEIGHT, made once and shared"""
    prob, label = _case(name, shape)
    posmasks, p = ref.PARAM_SETS[pset]
    return ref.focal64(prob, label, posmasks, p, w=WEIGHT)


def _bits(t):
    return t.detach().cpu().contiguous().numpy().view(np.uint32)


def _device(prob, label):
    """channels-last probabilities [N, D0, D1, D2, 4] and the labels on the device"""
    return torch.from_numpy(np.moveaxis(prob, 1, -1).copy()).to(DEV), torch.from_numpy(label.copy()).to(DEV)


def _c_params(p):
    from cwf import _lib
    return _lib.FocalParams(p["fn"], p["fp"], p["exponent"], p["smooth"], p["gamma"], p["ce_ratio"], (ctypes.c_double * 4)(*p["class_weight"]))


def _c_masks(posmasks):
    return (ctypes.c_uint32 * max(len(posmasks), 1))(*posmasks)


def _forward_on_garbage(hip, prob_cl, lab, posmasks, p, wt):
    """cwf_focal_loss through the C interface with a workspace filled with 0xFF bytes"""
    n, v, r = int(prob_cl.shape[0]), int(lab[0].numel()), len(posmasks)
    nbytes = hip.lib.cwf_focal_workspace(n, v, r)
    assert nbytes >= 8 * (3 * r + 1) and nbytes % 256 == 0
    ws = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device=DEV)
    loss = torch.full((1,), float("nan"), device=DEV)
    coef = torch.full((2 * r + 1,), float("nan"), device=DEV)
    cm, cp = _c_masks(posmasks), _c_params(p)
    rc = hip.lib.cwf_focal_loss(prob_cl.data_ptr(), lab.data_ptr(), ctypes.addressof(cm), r, ctypes.addressof(cp), wt.data_ptr(),
                                loss.data_ptr(), coef.data_ptr(), n, v, 4, ws.data_ptr(), hip._stream())
    assert rc == 0
    return loss, coef


@pytest.mark.parametrize("name,shape", CASES)
def test_loss_coef_and_gradient_against_the_statement(hip, name, shape):
    prob, label = _case(name, shape)
    prob_cl, lab = _device(prob, label)
    wt = torch.full((1,), WEIGHT, device=DEV)
    for pset, (posmasks, p) in ref.PARAM_SETS.items():
        want = _statement(name, shape, pset)
        fb, cb = ref.forward_bound(want), ref.coef_bound(want)
        loss, coef = _forward_on_garbage(hip, prob_cl, lab, posmasks, p, wt)
        loss2, coef2 = hip.focal_loss(prob_cl, lab, posmasks, p, wt)                   # the backend route, workspace from the allocator
        got, gc = float(loss), coef.cpu().numpy()
        cerr = np.abs(gc.astype(np.float64) - want["coef"].astype(np.float64))
        print("%s %s %s: loss %.9g ref %.9g |diff| %.3g bound %.3g; coef worst |diff| / bound %.3g"
              % (name, shape, pset, got, float(want["loss"]), abs(got - float(want["loss"])), fb, float((cerr / cb).max())))
        assert abs(got - float(want["loss"])) <= fb
        assert np.all(cerr <= cb), (cerr, cb)
        assert np.array_equal(_bits(loss2), _bits(loss)) and np.array_equal(_bits(coef2), _bits(coef))      # bit-identical between two calls
        exact = name in ref.EXACT
        if exact:                                                                      # exact sums, no device function: the final rounding alone
            assert np.array_equal(_bits(loss), np.array([want["loss"]]).view(np.uint32)), (got, float(want["loss"]))
            assert np.array_equal(_bits(coef), want["coef"].view(np.uint32))
        for gs in GSCALES:
            d = hip.focal_loss_bwd(prob_cl, lab, posmasks, p, coef, torch.full((1,), gs, device=DEV)).permute(0, 4, 1, 2, 3)
            g = ref.focal64(prob, label, posmasks, p, w=WEIGHT, gscale=gs, coef=gc)     # operand-exact: from the device's own coef
            err = np.abs(d.cpu().numpy().astype(np.float64) - g["dprob64"])
            gb = ref.grad_bound(g)
            print("    gscale %g: gradient worst |diff| / bound %.3g, largest |gradient| %.3g" % (gs, float((err / gb).max()), float(np.abs(g["dprob64"]).max())))
            assert np.all(err <= gb), (name, shape, pset, gs, float((err / gb).max()))
            assert float(np.abs(g["dprob64"]).max()) > 0
            if exact:
                assert np.array_equal(_bits(d), g["dprob32"].view(np.uint32)), (name, shape, pset, gs)


def test_focal_ce_alone_against_the_topk_term_at_100_percent(hip):
    """R = 0, gamma = 0 is the mean of -ln max(p_y, 1e-7): what tools.topk_ce(percent=100) computes by another kernel"""
    from utils import tools
    for shape in ref.SHAPES:
        prob, label = _case("softmax", shape)
        prob_cl, lab = _device(prob, label)
        p = prob_cl.permute(0, 4, 1, 2, 3)
        a, b = float(tools.focal_ce(p, lab, gamma=0.0, weight=WEIGHT)), float(tools.topk_ce(p, lab, percent=100.0, weight=WEIGHT))
        want = _statement("softmax", shape, "ce_only")
        tk = topk_ref.topk_ce64(prob, label, label.size, WEIGHT)
        bound = ref.forward_bound(want) + topk_ref.forward_bound(tk["loss"], tk["sabs"], WEIGHT, label.size)
        print("%s: focal_ce %.9g topk_ce(100 %%) %.9g |diff| %.3g bound %.3g" % (shape, a, b, abs(a - b), bound))
        assert abs(a - b) <= bound and a > 0


def test_rejects_bad_arguments_without_a_launch(hip):
    L, s = hip.lib, hip._stream()
    assert L.cwf_focal_workspace(0, 64, 3) == -1 and L.cwf_focal_workspace(1, 0, 3) == -1 and L.cwf_focal_workspace(-2, 64, 3) == -1
    assert L.cwf_focal_workspace(1, 64, -1) == -1 and L.cwf_focal_workspace(1, 64, 9) == -1
    assert L.cwf_focal_workspace(2, 1 << 40, 3) == -2
    assert L.cwf_focal_workspace(2, 210, 3) == 1024 * 10 * 8 and L.cwf_focal_workspace(2, 210, 0) == 1024 * 8
    prob = torch.full((1, 4, 4, 4, 4), 0.25, device=DEV)
    lab = torch.zeros((1, 4, 4, 4), dtype=torch.int64, device=DEV)
    one = torch.ones(1, device=DEV)
    loss = torch.full((1,), -5.0, device=DEV)
    coef = torch.full((7,), -5.0, device=DEV)
    d = torch.full((1, 4, 4, 4, 4), -5.0, device=DEV)
    ws = torch.full((L.cwf_focal_workspace(1, 64, 3) + 256,), 0xFF, dtype=torch.uint8, device=DEV)
    ws = ws[(-ws.data_ptr()) % 256:]
    assert ws.data_ptr() % 256 == 0
    good_m, good_p = _c_masks(ref.REGION_MASKS), _c_params(ref.params())
    m, pp = ctypes.addressof(good_m), ctypes.addressof(good_p)
    p, l, o, ls, cf, w, dp = prob.data_ptr(), lab.data_ptr(), one.data_ptr(), loss.data_ptr(), coef.data_ptr(), ws.data_ptr(), d.data_ptr()

    def fw(prob=p, label=l, masks=m, r=3, params=pp, weight=o, loss=ls, coef=cf, n=1, v=64, c=4, ws=w):
        return L.cwf_focal_loss(prob, label, masks, r, params, weight, loss, coef, n, v, c, ws, s)

    def bw(prob=p, label=l, masks=m, r=3, params=pp, coef=cf, g=o, dprob=dp, n=1, v=64, c=4):
        return L.cwf_focal_loss_bwd(prob, label, masks, r, params, coef, g, dprob, n, v, c, s)
    for kw in (dict(prob=0), dict(label=0), dict(masks=0), dict(params=0), dict(weight=0), dict(loss=0), dict(coef=0), dict(ws=0),
               dict(c=2), dict(c=3), dict(n=0), dict(v=0), dict(n=-1), dict(r=-1), dict(r=9)):
        assert fw(**kw) == -1, kw
    for kw in (dict(prob=0), dict(label=0), dict(masks=0), dict(params=0), dict(coef=0), dict(g=0), dict(dprob=0), dict(c=2), dict(n=0),
               dict(v=0), dict(r=-1), dict(r=9)):
        assert bw(**kw) == -1, kw
    assert fw(ws=w + 8) == -3 and fw(prob=p + 4) == -3 and bw(dprob=dp + 4) == -3                                  # alignment
    for masks in ((14, 0, 8), (14, 16, 8), (14, 10, 0x80000008)):
        cm = _c_masks(masks)
        assert fw(masks=ctypes.addressof(cm)) == -1 and bw(masks=ctypes.addressof(cm)) == -1, masks
    nan, inf = float("nan"), float("inf")
    for bad in (dict(fn=-0.1), dict(fn=nan), dict(fp=inf), dict(fn=0.0, fp=0.0), dict(exponent=0.0), dict(exponent=4.5), dict(exponent=nan),
                dict(smooth=0.0), dict(smooth=inf), dict(smooth=nan), dict(gamma=0.5), dict(gamma=-1.0), dict(gamma=5.5), dict(gamma=nan),
                dict(ce_ratio=-1.0), dict(ce_ratio=inf), dict(ce_ratio=nan), dict(class_weight=(1, -1, 1, 1)), dict(class_weight=(1, 1, nan, 1))):
        cp = _c_params(ref.params(**bad))
        assert fw(params=ctypes.addressof(cp)) == -1 and bw(params=ctypes.addressof(cp)) == -1, bad
    cp = _c_params(ref.params(ce_ratio=0.0))
    assert fw(r=0, params=ctypes.addressof(cp)) == -1 and bw(r=0, params=ctypes.addressof(cp)) == -1              # both parts off
    torch.cuda.synchronize()
    assert bool((loss == -5.0).all()) and bool((coef == -5.0).all()) and bool((d == -5.0).all())     # nothing was launched
    assert bool((ws == 0xFF).all())
    assert fw(r=0, masks=0) == 0 and bw(r=0, masks=0) == 0                                          # no regions: no mask array needed
    torch.cuda.synchronize()
    assert float(loss) > 0 and bool((coef[1:] == -5.0).all()) and bool((d != -5.0).all())
    # the backend makes the same checks, before any call
    P = ref.params()
    for args in ((prob, lab, ref.REGION_MASKS, P, torch.ones(2, device=DEV)), (prob, lab, ref.REGION_MASKS, P, torch.ones(1)),
                 (prob, lab, ref.REGION_MASKS, P, torch.ones(1, dtype=torch.float64, device=DEV)), (prob, lab.int(), ref.REGION_MASKS, P, one),
                 (torch.zeros((1, 4, 4, 4, 2), device=DEV), lab, ref.REGION_MASKS, P, one), (prob, lab[:, :2], ref.REGION_MASKS, P, one),
                 (prob, lab, (14, 0), P, one), (prob, lab, (14, 16), P, one), (prob, lab, (), ref.params(ce_ratio=0.0), one),
                 (prob, lab, ref.REGION_MASKS, ref.params(gamma=0.5), one)):
        with pytest.raises(ValueError):
            hip.focal_loss(*args)
    with pytest.raises(ValueError):
        hip.focal_loss_bwd(prob, lab, ref.REGION_MASKS, P, torch.ones(5, device=DEV), one)


def _grad(prob_cl, f):
    leaf = prob_cl.clone().requires_grad_(True)
    out = f(leaf.permute(0, 4, 1, 2, 3))
    out.backward()
    return out.detach(), leaf.grad


def test_autograd_gradient_alone_and_summed_with_dice_ce(hip):
    """(5, 6, 7): one workgroup per sample in the Dice / CE sums, so that term's gradient is the same bits on every run"""
    from cwf import functional as CF
    from utils import tools
    prob, label = _case("softmax", (5, 6, 7))
    prob_cl, lab = _device(prob, label)
    loss, gf = _grad(prob_cl, lambda p: tools.focal_loss(p, lab, weight=WEIGHT))
    want = _statement("softmax", (5, 6, 7), "defaults")
    assert abs(float(loss) - float(want["loss"])) <= ref.forward_bound(want)
    _, coef = hip.focal_loss(prob_cl, lab, ref.REGION_MASKS, ref.params(), torch.full((1,), WEIGHT, device=DEV))
    g = ref.focal64(prob, label, ref.REGION_MASKS, ref.params(), w=WEIGHT, coef=coef.cpu().numpy())
    assert np.all(np.abs(gf.permute(0, 4, 1, 2, 3).cpu().numpy().astype(np.float64) - g["dprob64"]) <= ref.grad_bound(g))
    _, gf2 = _grad(prob_cl, lambda p: tools.focal_loss(p, lab, weight=torch.full((1,), WEIGHT, device=DEV)))
    assert torch.equal(gf2, gf)                                                          # a device-resident weight: the same call
    _, gd = _grad(prob_cl, lambda p: CF.dice_ce_loss(p, lab))
    _, both = _grad(prob_cl, lambda p: tools.dice_ce(p, lab) + tools.focal_loss(p, lab, weight=WEIGHT))
    assert torch.equal(both, gd + gf) and float(gd.abs().max()) > 0 and float(gf.abs().max()) > 0
    # an NCDHW-contiguous input (the Function sees a channels-last copy) gives the same gradient
    nc = prob_cl.permute(0, 4, 1, 2, 3).contiguous().requires_grad_(True)
    tools.focal_loss(nc, lab, weight=WEIGHT).backward()
    assert torch.equal(nc.grad, gf.permute(0, 4, 1, 2, 3))


@pytest.mark.parametrize("shape", ref.SHAPES)
@pytest.mark.parametrize("pset", ["defaults", "classwise"])
def test_end_to_end_gradient_against_float64_autograd(hip, shape, pset):
    """the project's rule for hand-written glue: relative L2 and largest error within 16 x those of a float32 torch run of the same
    float64 autograd statement"""
    from utils import tools
    prob, label = _case("softmax", shape)
    posmasks, p = ref.PARAM_SETS[pset]
    lt = torch.from_numpy(label.copy())

    def torch_grad(dtype):
        leaf = torch.from_numpy(prob.copy()).to(dtype).requires_grad_(True)
        loss = ref.torch_statement(leaf, lt, posmasks, p, WEIGHT)
        loss.backward()
        return float(loss.detach()), leaf.grad.double().numpy()
    l64, g64 = torch_grad(torch.float64)
    l32, g32 = torch_grad(torch.float32)
    prob_cl, lab = _device(prob, label)
    kw = {k: p[k] for k in ("fn", "fp", "exponent", "smooth", "gamma", "ce_ratio", "class_weight")}
    loss, gk = _grad(prob_cl, lambda q: tools.focal_loss(q, lab, posmasks=posmasks, weight=WEIGHT, **kw))
    gk = gk.permute(0, 4, 1, 2, 3).cpu().numpy().astype(np.float64)
    nrm = float(np.linalg.norm(g64))
    e32, m32 = float(np.linalg.norm(g32 - g64)) / nrm, float(np.abs(g32 - g64).max())
    ek, mk = float(np.linalg.norm(gk - g64)) / nrm, float(np.abs(gk - g64).max())
    print("%s %s: rel L2 %.3g (float32 torch %.3g), max |err| %.3g (float32 torch %.3g); loss %.9g / %.9g / %.9g"
          % (shape, pset, ek, e32, mk, m32, float(loss), l32, l64))
    assert e32 > 0 and ek <= 16 * e32 and mk <= 16 * m32
    assert abs(float(loss) - l64) <= 16 * max(abs(l32 - l64), 2.0 ** -24 * abs(l64))


def test_drop_in_names(hip):
    from models import criterions
    from utils import tools
    prob, label = _case("softmax", (5, 6, 7))
    prob_cl, lab = _device(prob, label)
    p = prob_cl.permute(0, 4, 1, 2, 3)
    full = ref.focal64(prob, label, ref.REGION_MASKS, ref.params())
    tv = ref.focal64(prob, label, ref.REGION_MASKS, ref.params(ce_ratio=0.0))
    ce = ref.focal64(prob, label, (), ref.params())
    for mod in (tools, criterions):
        assert abs(float(mod.focal_loss(p, lab)) - float(full["loss"])) <= ref.forward_bound(full)
        assert abs(float(mod.focal_tversky(p, lab)) - float(tv["loss"])) <= ref.forward_bound(tv)
        assert abs(float(mod.focal_ce(p, lab)) - float(ce["loss"])) <= ref.forward_bound(ce)
    assert abs(float(full["loss64"]) - (float(tv["loss64"]) + float(ce["loss64"]))) <= 1e-12      # (the two halves add up)
    a, b = float(criterions.softmax_dice(p, lab)), float(criterions.focal_loss(p, lab))
    both = float(criterions.softmax_dice_focal(p, lab))
    assert abs(both - (a + b)) <= 1e-6 * abs(a + b) and b > 0
    with pytest.raises(ValueError):
        tools.focal_loss(p, lab, gamma=0.5)
    with pytest.raises(ValueError):
        tools.focal_tversky(p, lab, posmasks=())


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


def _focal_part_reference(out, target, w):
    res = ref.focal64(out.detach().cpu().contiguous().numpy(), target.cpu().numpy(), ref.REGION_MASKS, ref.params(), w=w)
    return float(res["loss"]), ref.forward_bound(res)


def test_trainer_without_the_term_makes_no_new_call(hip, monkeypatch):
    from cwf import kernels, trainer
    from cwf.trainer import Trainer
    forced, batch = _batch()

    def boom(*a, **k):
        raise AssertionError("the focal kernels were called with the term off")
    for name in ("focal_loss", "focal_loss_bwd"):
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
        assert len(parts) == 5 and tr._focal is None and tr._topk is None and tr._boundary is None and bool(torch.isfinite(loss))
        assert calls == [None]
        with pytest.raises(ValueError):
            tr.set_focal_weight(0.1)
    finally:
        kernels.set_precision("fp32")


def test_trainer_with_the_term_eager_and_plan(hip, monkeypatch):
    """64^3, B = 1, top-k token indices teacher-forced, dropout off, learning rate 0 (the weights stay where they are, so every step
    sees the same problem).  The new part against the statement on the step's own main output within the forward bound; the flat
    gradient moved by more than 100 x the eager-against-eager spread; the plan step's flat gradient against the eager step's within
    max(5e-5, 10 x that spread), the bound of the existing replay tests; set_focal_weight after capture doubles the part on the next
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
            tr = Trainer(_no_dropout_model(forced), lr=0.0, weight_decay=0.0, focal_weight=0.5)
            loss, parts = tr._fwd_bwd(*batch)
            torch.cuda.synchronize()
            eager.append(tr.opt.flat_grad.clone())
            assert len(parts) == 6 and set(seen["kw"]) == {"focal"} and seen["kw"]["focal"][1]["gamma"] == 2.0
            want, bound = _focal_part_reference(seen["out"], batch[1], 0.5)
            again = float(tools.focal_loss(seen["out"], batch[1], weight=0.5))
            print("eager focal part %.9g tools %.9g ref %.9g bound %.3g" % (float(parts[5]), again, want, bound))
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

        tr = Trainer(_no_dropout_model(forced), lr=0.0, weight_decay=0.0, use_graph="plan", focal_weight=0.5)
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
        want, bound = _focal_part_reference(seen["out"], batch[1], 0.5)
        p6 = float(parts[5])
        assert abs(p6 - want) <= bound

        tr.set_focal_weight(1.0)
        loss, parts = tr.step(*batch, 0)
        torch.cuda.synchronize()
        assert tr._plan.value == plan and len(parts) == 6
        want2, bound2 = _focal_part_reference(seen["out"], batch[1], 1.0)
        print("plan focal part: %.9g at 0.5, %.9g at 1.0 (ref %.9g, bound %.3g)" % (p6, float(parts[5]), want2, bound2))
        assert abs(float(parts[5]) - want2) <= bound2
        assert abs(float(parts[5]) - 2.0 * p6) <= 1e-4 * abs(2.0 * p6)           # doubled (same weights: lr = 0)
    finally:
        kernels.set_precision("fp32")


def test_trainer_with_boundary_topk_and_focal_has_eight_parts_in_order(hip, monkeypatch):
    from cwf import kernels
    from cwf.trainer import Trainer
    forced, batch = _batch()
    seen = _record_main_output(monkeypatch)
    kernels.set_precision("bf16x3")
    try:
        tr = Trainer(_no_dropout_model(forced), lr=0.0, weight_decay=0.0, boundary_weight=0.01, topk_weight=0.5, topk_percent=5.0,
                     focal_weight=0.25)
        loss, parts = tr._fwd_bwd(*batch)
        torch.cuda.synchronize()
        assert len(parts) == 8 and set(seen["kw"]) == {"topk", "focal"}
        p = seen["out"].detach().cpu().contiguous().numpy()
        t = batch[1].cpu().numpy()
        want, bound = _focal_part_reference(seen["out"], batch[1], 0.25)
        assert abs(float(parts[7]) - want) <= bound
        k = topk_ref.topk_count(t.size, 5.0)
        tk = topk_ref.topk_ce64(p, t, k, 0.5)
        assert abs(float(parts[6]) - float(tk["loss"])) <= topk_ref.forward_bound(tk["loss"], tk["sabs"], 0.5, k)
        phi = boundary_ref.signed_distance(t, use_scipy=True)
        bw, sabs, _ = boundary_ref.boundary_loss64(p, phi, boundary_ref.REGION_MASKS, 0.01)
        assert abs(float(parts[5]) - float(bw)) <= boundary_ref.forward_bound(bw, sabs, 0.01, 1, 3, int(np.prod(p.shape[2:])))
        assert min(abs(float(parts[i]) - float(parts[j])) for i in (5, 6, 7) for j in (5, 6, 7) if i < j) > 10 * bound    # three different numbers
        total = sum(float(q) for q in parts)
        assert abs(float(loss) - total) <= 1e-6 * abs(total)
    finally:
        kernels.set_precision("fp32")
