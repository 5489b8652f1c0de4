"""CPU: the float64 head -> loss reference of tests/head_loss_ref.py -- against torch's float64 F.interpolate + softmax + autograd
and the Dice / CE restatements of oracle/reference_model.py (pinned to the reference by tests/golden/losses.npz), and its power
to see defects by >= 30x, beside the earlier 1e-4 * max|ref| bound (planted in the reference's own output, never in a kernel)."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import head_loss_ref as H
from conftest import GOLDEN
from oracle import reference_model as rm
from utils import tools


def _u(*shape, seed, s=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(*shape, generator=g, dtype=torch.float64) * 2 - 1) * s


def _labels(codes, shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.tensor(codes)[torch.randint(0, len(codes), shape, generator=g)]


@pytest.mark.parametrize("scale,lo", [(4, (3, 5, 8)), (8, (2, 3, 2)), (4, (2, 2, 1))])
@pytest.mark.parametrize("C", [2, 4])
def test_upsample_softmax_is_torch_float64(scale, lo, C):
    lg = _u(2, *lo, C, seed=1, s=6)
    mats = H.axis_matrices(lo, scale)
    p, q = H.probs(lg, C, mats)
    up = F.interpolate(lg.permute(0, 4, 1, 2, 3), scale_factor=scale, mode="trilinear", align_corners=False)
    ref = up.softmax(1).permute(0, 2, 3, 4, 1)
    assert float((p - ref).abs().max()) < 1e-14
    absup = F.interpolate(lg.abs().permute(0, 4, 1, 2, 3), scale_factor=scale, mode="trilinear", align_corners=False)
    assert float((q[..., 0] - 1 - absup.amax(1)).abs().max()) < 1e-13
    y = _u(*p.shape, seed=2)
    assert float((H.interp_adjoint(y, mats) * lg).sum() - (y * H.interp(lg, mats)).sum()) < 1e-10          # the adjoint


def _rm_loss(p_ncdhw, cls, C):
    return rm._dice_ce(p_ncdhw, cls, C)


@pytest.mark.parametrize("C,codes,posmask", [(4, (0, 1, 2, 3), 0), (2, (0, 1, 2, 3), tools.REGION_MASKS["02"]),
                                             (2, (0, 1, 2, 4, 5, 6, 7, 8), tools.EDGE_MASKS["04"])])
def test_loss_coefficients_and_gradient_agree_with_autograd_and_oracle(C, codes, posmask):
    """sums -> finalize == the reference model's Dice + weighted CE in float64; the surrogate's gradient with the exact
    coefficients == autograd of that loss, through upsample and softmax, at gscale != 1 and with probabilities below 0.005"""
    scale, lo, n = 4, (3, 4, 5), 2
    lg = _u(n, *lo, C, seed=3, s=7)
    label = _labels(codes, (n,) + tuple(v * scale for v in lo), seed=4)
    mats = H.axis_matrices(lo, scale)
    t = H.target(label, C, posmask)
    p, q = H.probs(lg, C, mats)
    S, A = H.sums(p, t, q)
    V = p[0, ..., 0].numel()
    loss, coef, _ = H.finalize(S, V)
    leaf = lg.clone().requires_grad_(True)
    up = F.interpolate(leaf.permute(0, 4, 1, 2, 3), scale_factor=scale, mode="trilinear", align_corners=False).softmax(1)
    cls = t.argmax(-1)
    ref_loss = _rm_loss(up, cls, C)
    # two differences of float64 noise size, both of the restatement: its CE weight w = 1 - T_c / T is an fp32 quotient
    # (onehot.float(), as in the reference), the finalize kernel's a float64 one (relative 2^-24); and in float64 torch.clamp's
    # bound is 0.005 itself, 2.2e-8 relative above the kernels' fp32 0.005f, so a clamped voxel's log differs by 2.2e-8
    assert abs(float(loss) - float(ref_loss.detach())) < 2.3e-8 + 2 * H.U * abs(float(ref_loss.detach()))
    (0.37 * ref_loss).backward()
    g = H.logit_grad(lg, C, mats, t, coef, 0.37)
    assert float((g - leaf.grad).abs().max()) <= 2 * H.U * float(leaf.grad.abs().max())
    # with the restatement's fp32 weights as coefficients, autograd of the surrogate is autograd of the loss to float64 noise
    w32 = (1.0 - t.sum((1, 2, 3)).float() / t.sum((1, 2, 3, 4)).float()[:, None]).double()
    coef32 = coef.clone()
    coef32[..., 2] = -w32 / (n * V)
    g32 = H.logit_grad(lg, C, mats, t, coef32, 0.37)
    assert float((g32 - leaf.grad).abs().max()) <= 1e-12 * float(leaf.grad.abs().max())
    assert bool((p < H.CLAMP_LO).any()) and bool((p > H.CLAMP_LO).any())
    assert bool((A >= S.abs() - 1e-9).all())
    bound, Ag = H.logit_grad_bound(lg, C, mats, t, coef, 0.37, scale)
    assert bool((Ag >= g.abs() * (1 - 1e-12)).all())          # the companion dominates the value it bounds


def test_label_decoding_matches_the_reference_remaps():
    edge = _labels((0, 1, 2, 4, 5, 6, 7, 8), (2, 6, 6, 6), seed=5)
    for key in rm.REGIONS:
        m = torch.zeros_like(edge, dtype=torch.bool)
        for c in rm.EDGE_SETS[key]:
            m |= edge == c
        assert torch.equal(H.target(edge, 2, tools.EDGE_MASKS[key]).argmax(-1), m.long())
    region = _labels((0, 1, 2, 3), (2, 6, 6, 6), seed=6)
    for key, k in zip(rm.REGIONS, (1, 2, 3)):
        assert torch.equal(H.target(region, 2, tools.REGION_MASKS[key]).argmax(-1), (region == k).long())


def test_losses_fixture_in_float64():
    """tests/golden/losses.npz (the reference's own losses and gradients) from the sums / finalize / dprob of this module"""
    g = np.load(os.path.join(GOLDEN, "losses.npz"))
    target, edge = torch.from_numpy(g["target"]), torch.from_numpy(g["edge"])
    p4 = torch.from_numpy(g["p4"]).double().permute(0, 2, 3, 4, 1)
    V = p4[0, ..., 0].numel()

    def loss_grad(p, t):
        S, _ = H.sums(p, t)
        loss, coef, _ = H.finalize(S, V)
        return loss, H.dprob(p, t, coef, 1.0)[0]
    l4, g4 = loss_grad(p4, H.target(target, 4))
    assert abs(float(l4) - float(g["softmax_dice"])) < 1e-6
    assert np.allclose(g4.permute(0, 4, 1, 2, 3).numpy(), g["softmax_dice_grad"], rtol=1e-5, atol=1e-9)
    for lab, masks, lname, gname in ((target, tools.REGION_MASKS, "separate_loss", "sep_grad_"), (edge, tools.EDGE_MASKS, "edge_separate_loss", "edge_grad_")):
        tot = 0.0
        for r in rm.REGIONS:
            p = torch.from_numpy(g["p2_" + r]).double().permute(0, 2, 3, 4, 1)
            l, gr = loss_grad(p, H.target(lab, 2, masks[r]))
            tot += float(l)
            assert np.allclose(gr.permute(0, 4, 1, 2, 3).numpy(), g[gname + r], rtol=1e-5, atol=1e-9)
        assert abs(tot - float(g[lname])) < 1e-6


# ------------------------------------------------------------------ planted defects
def _trunc12(x):
    """x rounded toward zero to 12 fraction bits: a 2^-12-accurate result"""
    m, e = torch.frexp(x)
    return torch.ldexp(torch.trunc(m * 8192) / 8192, e)


def _defect_case():
    """N = 2, 2 x (4, 5, 6) -> (16, 20, 24) at scale 4: Ho = 20 leaves a ragged last group of 4 rows.  The interior is uncertain
    (|logit| <= 1.5), the outer shell confident background (logit difference 12), where dLoss/dlogit is small -- as at the
    borders of a real volume."""
    n, lo, scale = 2, (4, 5, 6), 4
    lg = _u(n, *lo, 2, seed=7, s=1.5)
    shell = torch.ones(lo, dtype=torch.bool)
    shell[1:-1, 1:-1, 1:-1] = False
    lg[:, shell, 0] = 6.0
    lg[:, shell, 1] = -6.0
    hi = tuple(v * scale for v in lo)
    label = _labels((0, 1, 2, 3), (n,) + hi, seed=8)
    inner = torch.zeros(hi, dtype=torch.bool)
    inner[scale:-scale, scale:-scale, scale:-scale] = True
    label[:, ~inner] = 0                                        # the shell's label agrees with its logits
    return lg, label, scale, tools.REGION_MASKS["01"]


def _grad_check(defect_grad, what):
    lg, label, scale, pm = _defect_case()
    mats = H.axis_matrices(lg.shape[1:4], scale)
    t = H.target(label, 2, pm)
    p, q = H.probs(lg, 2, mats)
    S, _ = H.sums(p, t, q)
    _, coef, _ = H.finalize(S, p[0, ..., 0].numel())
    ref = H.logit_grad(lg, 2, mats, t, coef, 1.0)
    bound, A = H.logit_grad_bound(lg, 2, mats, t, coef, 1.0, scale)
    bad = defect_grad(lg, mats, t, coef, label, p)
    r = float(((bad - ref).abs() / bound).max())
    old = H.old_bound_fails(bad, ref)
    print("%-40s worst err/(gamma A) = %10.1f   1e-4 max|ref| bound %s" % (what, r, "FAILS" if old else "passes"))
    return r, old


def test_planted_defects_fail_the_elementwise_bound():
    """Each defect, planted in the reference, fails |got - ref| <= gamma A by >= 30x; whether the earlier bound 1e-4 max|ref|
    also fails it is printed and pinned below."""
    results = {}

    def far_edge(lg, mats, t, coef, label, p):                  # the last output column reads column W-2 instead of W-1
        Md, Mh, Mw = mats
        Mw = Mw.clone()
        Mw[-1] = 0.0
        Mw[-1, -2] = 1.0
        return H.logit_grad(lg, 2, (Md, Mh, Mw), t, coef, 1.0)
    results["source index off by one at the far edge"] = _grad_check(far_edge, "far-edge source index")

    def drop_rows(rows):
        def f(lg, mats, t, coef, label, p):
            keep = torch.ones_like(p[..., :1])
            keep[:, :, rows] = 0.0
            return H.logit_grad(lg, 2, mats, t, coef, 1.0, keep=keep)
        return f
    Ho = 20
    results["dropped last ragged row"] = _grad_check(drop_rows(slice(Ho - 1, Ho)), "dropped last ragged row")
    results["dropped last row group"] = _grad_check(drop_rows(slice(16, 20)), "dropped last row group (rows 16..19)")

    def fast_math(v):
        e = _trunc12(torch.exp(v - v.amax(-1, keepdim=True)))
        return e * _trunc12(1.0 / e.sum(-1, keepdim=True))
    results["2^-12 exp and rcp"] = _grad_check(lambda lg, mats, t, coef, label, p: H.logit_grad(lg, 2, mats, t, coef, 1.0, p_override=fast_math),
                                               "2^-12-accurate exp and rcp (gradient)")
    # the same defect in the forward map: probabilities against GAMMA_P q p
    lg, label, scale, pm = _defect_case()
    mats = H.axis_matrices(lg.shape[1:4], scale)
    p, q = H.probs(lg, 2, mats)
    pb, _ = H.probs(lg, 2, mats, exp=lambda x: _trunc12(torch.exp(x)), rcp=lambda x: _trunc12(1.0 / x))
    r = float(((pb - p).abs() / (H.GAMMA_P * q * p)).max())
    print("%-40s worst err/(gamma A) = %10.1f   1e-4 max|ref| bound %s" % ("2^-12-accurate exp and rcp (probability)", r,
                                                                       "FAILS" if H.old_bound_fails(pb, p) else "passes"))
    results["2^-12 exp and rcp, probabilities"] = (r, H.old_bound_fails(pb, p))

    # clamp gate one ulp off, on probabilities placed at 0.005f (dice_ce_bwd: dprob from a stored map)
    n, V = 2, 4096
    p = torch.rand(n, 16, 16, 16, 2, generator=torch.Generator().manual_seed(9), dtype=torch.float64).float().double()
    p[..., 1] = 1 - p[..., 0]
    p[0, 3, 5, :7, 1] = H.CLAMP_LO
    p[0, 3, 5, :7, 0] = float(np.float32(1 - H.CLAMP_LO))
    t = H.target(_labels((0, 1, 2, 3), (n, 16, 16, 16), seed=10), 2, tools.REGION_MASKS["01"])
    t[0, 3, 5, :7] = torch.tensor([0.0, 1.0], dtype=torch.float64)
    S, _ = H.sums(p, t)
    _, coef, _ = H.finalize(S, V)
    g, G = H.dprob(p, t, coef, 1.0)
    gb, _ = H.dprob(p, t, coef, 1.0, lo=float(np.nextafter(np.float32(H.CLAMP_LO), np.float32(1))))
    r = float(((gb - g).abs() / (H.GAMMA_DPROB * G)).max())
    old = H.old_bound_fails(gb, g)
    print("%-40s worst err/(gamma A) = %10.1f   1e-4 max|ref| bound %s" % ("clamp boundary one ulp up (dprob)", r, "FAILS" if old else "passes"))
    results["clamp boundary one ulp"] = (r, old)

    def flipped_bit(lg, mats, t, coef, label, p):               # code 5 dropped from E1 = {1, 5, 6, 7}
        return H.logit_grad(lg, 2, mats, H.target(label, 2, tools.EDGE_MASKS["01"] ^ (1 << 5)), coef, 1.0)
    lg, label, scale, _ = _defect_case()
    edge = _labels((0, 1, 2, 4, 5, 6, 7, 8), label.shape, seed=11)
    mats = H.axis_matrices(lg.shape[1:4], scale)
    t = H.target(edge, 2, tools.EDGE_MASKS["01"])
    p, q = H.probs(lg, 2, mats)
    S, A = H.sums(p, t, q)
    _, coef, _ = H.finalize(S, p[0, ..., 0].numel())
    ref = H.logit_grad(lg, 2, mats, t, coef, 1.0)
    bound, _ = H.logit_grad_bound(lg, 2, mats, t, coef, 1.0, scale)
    bad = flipped_bit(lg, mats, t, coef, edge, p)
    r = float(((bad - ref).abs() / bound).max())
    old = H.old_bound_fails(bad, ref)
    print("%-40s worst err/(gamma A) = %10.1f   1e-4 max|ref| bound %s" % ("posmask bit flipped for code 5", r, "FAILS" if old else "passes"))
    results["posmask bit flipped"] = (r, old)

    # one sample's sums credited to the other: against the sums bound of the fused kernel
    Sb = S.clone()
    Sb[1] += Sb[0]
    Sb[0] = 0.0
    gs = H.gamma_sums(H.fused_terms_per_thread(p.shape[3]))
    bnd = gs * A
    r = float(((Sb - S).abs() / torch.where(bnd > 0, bnd, torch.full_like(bnd, 1e-300))).max())
    old = H.old_bound_fails(Sb, S)
    print("%-40s worst err/(gamma A) = %10.1f   1e-4 max|ref| bound %s" % ("sample 0's sums credited to sample 1", r, "FAILS" if old else "passes"))
    results["sums credited to the other sample"] = (r, old)

    for k, (r, _) in results.items():
        assert r >= 30, (k, r)
    # Only the dropped ragged row -- one high-resolution row of confident background -- passes the earlier 1e-4 max|ref| bound.
    # The others move a large part of max|ref| as planted here (the far-edge index and the dropped row group reach interior
    # voxels through the interpolation window); the elementwise bound sees each by >= 30x either way.
    old_catches = {k for k, (_, o) in results.items() if o}
    assert old_catches == set(results) - {"dropped last ragged row"}, old_catches
