"""The boundary loss on the GPU (csrc/boundary.hip and its way up through cwf.kernels, cwf.functional, utils.tools and
cwf.trainer.Trainer): dense signed distance maps bit-equal to the statement, the fused loss forward within its derived bound, the
backward bit-equal, and the Trainer with the term off and on.  Yardstick: tests/boundary_ref.py."""
import functools

import numpy as np
import pytest
import torch

import boundary_ref as ref
import hausdorff_ref as H
from oracle import reference_model as rm
from utils import synthetic as syn

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# extent 1, odd extents, lines past one wave (130) and past one 256-thread workgroup (300) on each axis, several 64-voxel chunks per
# slab (33 x 34 x 65)
SHAPES = ((1, 1, 1), (1, 1, 7), (5, 6, 7), (3, 70, 2), (2, 3, 130), (2, 3, 300), (2, 300, 3), (300, 2, 3), (33, 34, 65))
BRUTE_BELOW = 2000


def _labels(shape, seed, nb=2):
    rng = np.random.default_rng(seed)
    if int(np.prod(shape)) < BRUTE_BELOW:
        return rng.choice(4, size=(nb,) + shape, p=[.5, .15, .2, .15]).astype(np.int64)
    return np.stack([H.nested_labels(shape, rng) for _ in range(nb)]).astype(np.int64)


def _special(shape, seed):
    """five samples: a general one holding a label 7 and a label -1; one whose ET is empty; one that is all label 3 (every region
    full); one whose WT is a shell on every face of the volume; one that is all background (every region empty)"""
    base = _labels(shape, seed, 2)
    a = base[0].copy()
    a.reshape(-1)[0] = 7
    a.reshape(-1)[a.size // 2] = -1
    b = base[1].copy()
    b[b == 3] = 1
    c = np.full(shape, 3, dtype=np.int64)
    d = np.full(shape, 2, dtype=np.int64)
    d[1:-1, 1:-1, 1:-1] = 0
    e = np.zeros(shape, dtype=np.int64)
    return np.stack([a, b, c, d, e])


@functools.lru_cache(maxsize=None)
def _case(shape, kind="plain", posmasks=ref.REGION_MASKS):
    """(label on the host, reference phi), computed once and left unchanged"""
    label = _special(shape, 11 + sum(shape)) if kind == "special" else _labels(shape, 3 + sum(shape))
    want = ref.signed_distance(label, posmasks, use_scipy=int(np.prod(shape)) >= BRUTE_BELOW)
    label.setflags(write=False)
    want.setflags(write=False)
    return label, want


def _bits(t):
    return t.detach().cpu().contiguous().numpy().view(np.uint32)


# ------------------------------------------------------------------------------------------------------------------ distance maps
@pytest.mark.parametrize("shape", SHAPES)
def test_signed_distance_is_bit_equal_to_the_statement(hip, shape):
    label, want = _case(shape)
    assert not np.array_equal(label[0], label[1])
    lab = torch.from_numpy(label.copy()).to(DEV)
    phi = hip.signed_distance(lab)
    assert phi.shape == (2, 3) + shape and phi.dtype == torch.float32
    assert np.array_equal(_bits(phi), want.view(np.uint32)), shape
    # no cross-sample leakage: each sample alone gives its own maps; and the same call twice gives the same bits
    one = hip.signed_distance(lab[1:2])
    assert np.array_equal(_bits(one), want[1:2].view(np.uint32))
    assert np.array_equal(_bits(hip.signed_distance(lab)), _bits(phi))


@pytest.mark.parametrize("shape", [(5, 6, 7), (33, 34, 65)])
def test_signed_distance_degenerate_regions_faces_and_foreign_labels(hip, shape):
    label, want = _case(shape, "special")
    assert (label[0] == 7).any() and (label[0] == -1).any() and not (label[1] == 3).any()
    phi = hip.signed_distance(torch.from_numpy(label.copy()).to(DEV))
    got = _bits(phi)
    assert np.array_equal(got, want.view(np.uint32))
    assert not got[1, 2].any() and not got[2].any() and not got[4].any()          # empty ET, full regions, empty regions: +0
    assert got[3, 0].any() and not got[3, 2].any()


@pytest.mark.parametrize("posmasks", [(2, 4, 8), (8,), (0b0110, 0xFFFFFFFF)])
def test_signed_distance_custom_regions(hip, posmasks):
    for shape in ((5, 6, 7), (33, 34, 65)):
        label, want = _case(shape, "special", posmasks)
        phi = hip.signed_distance(torch.from_numpy(label.copy()).to(DEV), posmasks)
        assert phi.shape == (5, len(posmasks)) + shape
        assert np.array_equal(_bits(phi), want.view(np.uint32)), (shape, posmasks)


def test_signed_distance_rejects_bad_arguments_without_a_launch(hip):
    from cwf import _lib
    L, s = hip.lib, hip._stream()
    assert L.cwf_signed_distance_workspace(1, 3, 513, 4, 4) == -1 and L.cwf_signed_distance_workspace(1, 3, 4, 513, 4) == -1
    assert L.cwf_signed_distance_workspace(1, 3, 4, 4, 513) == -1 and L.cwf_signed_distance_workspace(1, 9, 4, 4, 4) == -1
    assert L.cwf_signed_distance_workspace(1, 0, 4, 4, 4) == -1 and L.cwf_signed_distance_workspace(0, 3, 4, 4, 4) == -1
    assert L.cwf_signed_distance_workspace(1, 3, 0, 4, 4) == -1
    assert L.cwf_signed_distance_workspace(2, 3, 512, 1, 1) == 2 * 3 * 512 * 6
    lab = torch.zeros((1, 4, 4, 4), dtype=torch.int64, device=DEV)
    phi = torch.full((1, 3, 4, 4, 4), -5.0, device=DEV)
    ws = torch.zeros(4096, dtype=torch.uint8, device=DEV)
    import ctypes
    m3, m9 = (ctypes.c_uint32 * 3)(14, 10, 8), (ctypes.c_uint32 * 9)(*range(9))
    a3, a9 = ctypes.addressof(m3), ctypes.addressof(m9)
    sd = L.cwf_signed_distance
    assert sd(lab.data_ptr(), a3, phi.data_ptr(), 1, 3, 513, 4, 4, ws.data_ptr(), s) == -1
    assert sd(lab.data_ptr(), a9, phi.data_ptr(), 1, 9, 4, 4, 4, ws.data_ptr(), s) == -1
    assert sd(0, a3, phi.data_ptr(), 1, 3, 4, 4, 4, ws.data_ptr(), s) == -1
    assert sd(lab.data_ptr(), 0, phi.data_ptr(), 1, 3, 4, 4, 4, ws.data_ptr(), s) == -1
    assert sd(lab.data_ptr(), a3, 0, 1, 3, 4, 4, 4, ws.data_ptr(), s) == -1
    assert sd(lab.data_ptr(), a3, phi.data_ptr(), 1, 3, 4, 4, 4, 0, s) == -1
    assert sd(lab.data_ptr(), a3, phi.data_ptr(), 1, 3, 4, 4, 4, ws.data_ptr() + 8, s) == -3
    torch.cuda.synchronize()
    assert bool((phi == -5.0).all())                                             # nothing was launched
    big = torch.zeros((1, 513, 1, 1), dtype=torch.int64, device=DEV)
    with pytest.raises(_lib.CwfError):
        hip.signed_distance(big)
    with pytest.raises(_lib.CwfError):
        hip.signed_distance(lab, tuple(range(1, 10)))
    one = torch.ones(1, device=DEV)
    d = torch.zeros(1, dtype=torch.float64, device=DEV)
    assert L.cwf_boundary_sums(phi.data_ptr(), phi.data_ptr(), a9, d.data_ptr(), 1, 9, 64, 4, s) == -1
    assert L.cwf_boundary_sums(phi.data_ptr(), phi.data_ptr(), a3, d.data_ptr(), 1, 3, 64, 33, s) == -1
    assert L.cwf_boundary_sums(0, phi.data_ptr(), a3, d.data_ptr(), 1, 3, 64, 4, s) == -1
    assert L.cwf_boundary_finalize(d.data_ptr(), 0, one.data_ptr(), one.data_ptr(), 1, 3, 64, s) == -1
    assert L.cwf_boundary_finalize(d.data_ptr(), one.data_ptr(), one.data_ptr(), one.data_ptr(), 1, 9, 64, s) == -1
    assert L.cwf_boundary_bwd(phi.data_ptr(), a3, one.data_ptr(), one.data_ptr(), 0, 1, 3, 64, 4, s) == -1
    assert L.cwf_boundary_bwd(phi.data_ptr(), a9, one.data_ptr(), one.data_ptr(), phi.data_ptr(), 1, 9, 64, 4, s) == -1
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------------------ loss
def _prob(shape, seed, c=4, nb=2):
    """random softmax probabilities: (channels-last leaf [N, D0, D1, D2, C] on the device, host copy as [N, C, D0, D1, D2])"""
    gen = torch.Generator().manual_seed(seed)
    p = torch.softmax(2.0 * torch.randn((nb,) + shape + (c,), generator=gen), dim=-1)
    return p.to(DEV), p.permute(0, 4, 1, 2, 3).contiguous().numpy()


@pytest.mark.parametrize("shape", [(5, 6, 7), (33, 34, 65)])
def test_loss_forward_within_one_rounding_plus_the_summation_bound(hip, monkeypatch, shape):
    """|loss - ref| <= 2^-24 |ref| + (w / (N R V)) V 2^-52 sum|terms|: every product of two float32 is exact in float64, a float64 sum of
    V terms in any order is off by at most V 2^-53 sum|terms| (first order; 2^-52 leaves the margin), and the result is rounded once."""
    from cwf import functional as CF
    label, phi_ref = _case(shape)
    n, r, v = 2, 3, int(np.prod(shape))
    prob_cl, prob_host = _prob(shape, 5)
    prob = prob_cl.permute(0, 4, 1, 2, 3)
    lab = torch.from_numpy(label.copy()).to(DEV)
    phi = torch.from_numpy(phi_ref.copy()).to(DEV)
    wt = torch.full((1,), 0.37, device=DEV)
    got = {}
    for w in (0.37, 2.5):
        wt.fill_(w)
        want, sabs, _ = ref.boundary_loss64(prob_host, phi_ref, ref.REGION_MASKS, w)
        bound = ref.forward_bound(want, sabs, w, n, r, v)
        a = float(CF.boundary_loss(prob, lab, weight=wt))                        # maps computed from the label
        b = float(CF.boundary_loss(prob, None, weight=wt, phi=phi))              # precomputed maps
        c = float(CF.boundary_loss(prob, lab, weight=w))                         # weight as a float
        print("shape %s w %g: loss %.9g ref %.9g |diff| %.3g %.3g %.3g bound %.3g" % (shape, w, a, float(want), abs(a - float(want)),
                                                                                      abs(b - float(want)), abs(c - float(want)), bound))
        assert abs(a - float(want)) <= bound and abs(b - float(want)) <= bound and abs(c - float(want)) <= bound
        assert abs(float(want)) > 1e3 * bound                                    # (the bound is far below the value: it tests something)
        got[w] = b
    assert got[0.37] != got[2.5]
    # the weight lives on the device: changing it recomputes no map and allocates none
    monkeypatch.setattr(hip, "signed_distance", lambda *a, **k: (_ for _ in ()).throw(AssertionError("maps recomputed")))
    wt.fill_(0.0)
    assert float(CF.boundary_loss(prob, None, weight=wt, phi=phi)) == 0.0       # w = 0: exactly zero
    wt.fill_(0.37)
    want, sabs, _ = ref.boundary_loss64(prob_host, phi_ref, ref.REGION_MASKS, 0.37)
    assert abs(float(CF.boundary_loss(prob, None, weight=wt, phi=phi)) - float(want)) <= ref.forward_bound(want, sabs, 0.37, n, r, v)


@pytest.mark.parametrize("shape,posmasks,c", [((5, 6, 7), ref.REGION_MASKS, 4), ((33, 34, 65), ref.REGION_MASKS, 4),
                                              ((5, 6, 7), (0b0110, 0b1000, 0b0100), 4), ((5, 6, 7), (0b10, 0b110), 3)])
def test_backward_is_bit_equal_to_the_statement(hip, shape, posmasks, c):
    label, phi_ref = _case(shape, "plain", posmasks)
    prob_cl, prob_host = _prob(shape, 9, c)
    phi = torch.from_numpy(phi_ref.copy()).to(DEV)
    for w, gs in ((0.37, 1.0), (0.01, -0.75), (3.0, 1e-3)):
        wt = torch.full((1,), w, device=DEV)
        loss, coef = hip.boundary_loss(prob_cl, phi, posmasks, wt)
        d = hip.boundary_loss_bwd(prob_cl, phi, posmasks, coef, torch.full((1,), gs, device=DEV))
        _, _, want = ref.boundary_loss64(prob_host, phi_ref, posmasks, w, gscale=gs)
        assert np.array_equal(_bits(d.permute(0, 4, 1, 2, 3)), want.view(np.uint32)), (shape, posmasks, w, gs)
    if c == 4 and posmasks == ref.REGION_MASKS:
        assert not _bits(d)[..., 0].any()                                        # class 0 is in no region: +0


def test_autograd_gradient_and_its_sum_with_dice_ce(hip):
    """(5, 6, 7): one workgroup per sample in the Dice / CE sums, so that term's gradient is the same bits on every run"""
    from cwf import functional as CF
    shape = (5, 6, 7)
    label, phi_ref = _case(shape)
    lab = torch.from_numpy(label.copy()).to(DEV)
    prob_cl, prob_host = _prob(shape, 13)
    _, _, want = ref.boundary_loss64(prob_host, phi_ref, ref.REGION_MASKS, 0.2)

    def grad(f):
        leaf = prob_cl.clone().requires_grad_(True)
        f(leaf.permute(0, 4, 1, 2, 3)).backward()
        return leaf.grad

    gb = grad(lambda p: CF.boundary_loss(p, lab, weight=0.2))
    assert np.array_equal(_bits(gb.permute(0, 4, 1, 2, 3)), want.view(np.uint32))
    gd = grad(lambda p: CF.dice_ce_loss(p, lab))
    both = grad(lambda p: CF.dice_ce_loss(p, lab) + CF.boundary_loss(p, lab, weight=0.2))
    assert torch.equal(both, gd + gb) and float(gd.abs().max()) > 0


def test_drop_in_names(hip):
    from models import criterions
    from utils import tools
    shape = (5, 6, 7)
    label, phi_ref = _case(shape)
    lab = torch.from_numpy(label.copy()).to(DEV)
    prob_cl, prob_host = _prob(shape, 5)
    prob = prob_cl.permute(0, 4, 1, 2, 3)
    want, sabs, _ = ref.boundary_loss64(prob_host, phi_ref, ref.REGION_MASKS, 1.0)
    bound = ref.forward_bound(want, sabs, 1.0, 2, 3, int(np.prod(shape)))
    assert abs(float(tools.boundary_loss(prob, lab)) - float(want)) <= bound
    assert abs(float(criterions.boundary_loss(prob, lab)) - float(want)) <= bound
    for name in ("softmax_dice2", "sigmoid_dice", "Generalized_dice", "Dual_focal_loss"):
        with pytest.raises(NotImplementedError):
            getattr(criterions, name)()


# ------------------------------------------------------------------------------------------------------------------ Trainer
def _no_dropout_model(forced):
    from models.clswiseformer.cls_wise_former import get_cls_wise_former
    m = get_cls_wise_former(dataset="brats", _conv_repr=True, _pe_type="fixed")
    m.load_state_dict(syn.det_state_dict(rm.param_shapes()), strict=False)
    m.Unet_list.InitConv.dropout = 0.0
    m = m.to(DEV).train()
    m.forced_index = forced
    for mod in m.modules():
        if hasattr(mod, "dropout_rate"):
            mod.dropout_rate = 0.0
        if isinstance(mod, torch.nn.Dropout):
            mod.p = 0.0
    return m


@functools.lru_cache(maxsize=None)
def _batch():
    x, t, e = syn.synthetic_batch([0], (64, 64, 64))
    with torch.no_grad():
        _, aux = rm.forward(syn.det_state_dict(rm.param_shapes()), x, return_aux=True)
    forced = {k: v.to(DEV) for k, v in aux.items() if v.dtype == torch.int64}
    return forced, (x.to(DEV), t.to(DEV), e.to(DEV))


def _record_main_output(monkeypatch):
    """total_loss as it is, remembering the main output it was given (in a captured step that tensor is the step's static buffer)"""
    from cwf import trainer
    seen = {}
    orig = trainer.total_loss

    def wrapped(outputs, target, edge, boundary=None):
        seen["out"] = outputs[0].detach()
        return orig(outputs, target, edge, boundary)
    monkeypatch.setattr(trainer, "total_loss", wrapped)
    return seen


def _part6_reference(out, target, w):
    t = target.cpu().numpy()
    phi = ref.signed_distance(t, use_scipy=True)
    p = out.detach().cpu().contiguous().numpy()
    want, sabs, _ = ref.boundary_loss64(p, phi, ref.REGION_MASKS, w)
    return float(want), ref.forward_bound(want, sabs, w, p.shape[0], 3, int(np.prod(p.shape[2:])))


def test_trainer_without_the_term_makes_no_new_call(hip, monkeypatch):
    from cwf import kernels
    from cwf.trainer import Trainer
    forced, batch = _batch()

    def boom(*a, **k):
        raise AssertionError("the boundary kernels were called with the term off")
    for name in ("signed_distance", "boundary_loss", "boundary_loss_bwd"):
        monkeypatch.setattr(hip, name, boom)
    kernels.set_precision("bf16x3")
    try:
        tr = Trainer(_no_dropout_model(forced))
        loss, parts = tr.step(*batch, 0)
        torch.cuda.synchronize()
        assert len(parts) == 5 and tr._boundary is None and bool(torch.isfinite(loss))
        with pytest.raises(ValueError):
            tr.set_boundary_weight(0.1)
    finally:
        kernels.set_precision("fp32")


def test_trainer_with_the_term_eager_and_plan(hip, monkeypatch):
    """64^3, B = 1, top-k teacher-forced, dropout off, learning rate 0 (the weights stay where they are, so every step sees the same
    problem).  Part 6 against the float64 statement on the step's own main output within the forward bound; the plan step's flat
    gradient against the eager step's within max(5e-5, 10 x the eager-against-eager spread measured here), the bound of the existing
    replay tests; set_boundary_weight after capture changes part 6 on the next plan step with the plan left as it is."""
    from cwf import kernels
    from cwf.trainer import Trainer
    from utils import tools
    forced, batch = _batch()
    seen = _record_main_output(monkeypatch)
    kernels.set_precision("bf16x3")
    try:
        eager = []
        for rep in range(2):
            tr = Trainer(_no_dropout_model(forced), lr=0.0, weight_decay=0.0, boundary_weight=0.01)
            loss, parts = tr._fwd_bwd(*batch)
            torch.cuda.synchronize()
            eager.append(tr.opt.flat_grad.clone())
            assert len(parts) == 6
            want, bound = _part6_reference(seen["out"], batch[1], 0.01)
            again = float(tools.boundary_loss(seen["out"], batch[1], weight=0.01))
            print("eager part 6 %.9g tools %.9g ref %.9g bound %.3g" % (float(parts[5]), again, want, bound))
            assert abs(float(parts[5]) - want) <= bound and abs(again - want) <= bound and abs(want) > 1e3 * bound
            total = sum(float(p) for p in parts)
            assert abs(float(loss) - total) <= 1e-6 * abs(total)
        noise = float((eager[0] - eager[1]).norm() / eager[0].norm())
        # the term reaches the gradient: without it the flat gradient is another one
        tr0 = Trainer(_no_dropout_model(forced), lr=0.0, weight_decay=0.0)
        tr0._fwd_bwd(*batch)
        torch.cuda.synchronize()
        moved = float((tr0.opt.flat_grad - eager[0]).norm() / eager[0].norm())
        assert moved > 100 * max(noise, 1e-7), (moved, noise)

        tr = Trainer(_no_dropout_model(forced), lr=0.0, weight_decay=0.0, use_graph="plan", boundary_weight=0.01)
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
        want, bound = _part6_reference(seen["out"], batch[1], 0.01)
        p6 = float(parts[5])
        assert abs(p6 - want) <= bound

        tr.set_boundary_weight(0.02)
        loss, parts = tr.step(*batch, 0)
        torch.cuda.synchronize()
        assert tr._plan.value == plan and len(parts) == 6
        want2, bound2 = _part6_reference(seen["out"], batch[1], 0.02)
        print("plan part 6: %.9g at 0.01, %.9g at 0.02 (ref %.9g, bound %.3g)" % (p6, float(parts[5]), want2, bound2))
        assert abs(float(parts[5]) - want2) <= bound2
        assert abs(float(parts[5]) - 2.0 * p6) <= 1e-4 * abs(2.0 * p6)           # doubled (same weights: lr = 0)
    finally:
        kernels.set_precision("fp32")
