"""GPU: every entry point of the head -> loss family against the float64 reference of tests/head_loss_ref.py, elementwise:
|got - ref| <= gamma * A (+ the gate-ambiguity / coefficient terms of the gradient bound).  Production shapes at batch 2, the
edges of the launch geometry (ragged last row, Ho % 32 != 0, W in {1, 63, 64}, the W = 65 and odd-scale refusals, nmaps 1..3),
value edges (absent / single classes, logit differences of +-12 around the 0.005 clamp, gscale != 1), strided and grouped
layouts, and the Python route the model takes.  Run with -s to see the worst err/bound of every check.

Which test covers what: W = 32 at scale 4 and the 2 x 4 x 128^3 decoder -- test_production_shapes[edge-32^3x4] and
test_decoder_softmax_dice_128; the non-cubic patches -- test_production_shapes[*-64x96x80 / *-160x192x160]; a ragged last row
and Ho % 32 != 0 -- test_launch_geometry_edges[ragged-rows / ho-40]; the W = 64 limit and its refusal --
test_launch_geometry_edges[w64] and test_refusals; the clamp gate -- test_value_edges and test_unfused_dprob_clamp_gate;
the grouped output layout -- test_strided_logits_and_grouped_output and test_python_route_grouped_heads."""
import ctypes

import numpy as np
import pytest
import torch

import head_loss_ref as H
from utils import tools

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MAPS = ("01", "02", "04")
REGION = (0, 1, 2, 3)
EDGE = (0, 1, 2, 4, 5, 6, 7, 8)
_REF = {}                                    # float64 reference per (case, map), computed once per module


def _u(*shape, seed, s=1.0):
    g = torch.Generator().manual_seed(seed)
    return ((torch.rand(*shape, generator=g) * 2 - 1) * s).float()


def _labels(codes, shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.tensor(codes)[torch.randint(0, len(codes), shape, generator=g)]


def _report(what, r):
    print("  %-60s worst err/bound = %.3f" % (what, r))


def _worst(got, ref, bound, what):
    """H.worst, printed per check"""
    r = H.worst(got, ref, bound, what)
    print("    %-70s %.2e" % (what, r))
    return r


def _masks(codes):
    m = tools.EDGE_MASKS if codes == EDGE else tools.REGION_MASKS
    return [m[k] for k in MAPS]


def _ref(key, logit, C, scale, label, posmask):
    """(mats, t, p, q, S, A) of one map, cached"""
    if key not in _REF:
        mats = H.axis_matrices(logit.shape[1:4], scale) if scale > 1 else None
        t = H.target(label, C, posmask)
        p, q = H.probs(logit.double(), C, mats)
        S, A = H.sums(p, t, q)
        _REF[key] = (mats, t, p, q, S, A)
    return _REF[key]


def _fused_sums(hip, logits, label, pm, scale):
    """cwf_head_loss_sums alone (the wrapper hip.head_loss goes on to finalize): sums [nm, N, 2, 4] float64"""
    nm = len(logits)
    n, d, h, w, _ = logits[0].shape
    sums = torch.zeros((nm, n, 2, 4), dtype=torch.float64, device=DEV)
    ptrs = (ctypes.c_void_p * nm)(*[t.data_ptr() for t in logits])
    masks = (ctypes.c_uint32 * nm)(*[int(m) for m in pm])
    hip._call("cwf_head_loss_sums", ctypes.addressof(ptrs), nm, logits[0].stride(3), ctypes.addressof(masks), label.data_ptr(),
              sums.data_ptr(), n, d, h, w, scale, hip._stream())
    return sums


def _check_sums(got, S, A, gamma, what):
    got = got.detach().cpu().double()
    assert torch.equal(got[..., 2], S[..., 2]), (what, "T is a count and must be exact")
    return _worst(got, S, gamma * A, what)


def _check_finalize(loss, coef, sums, V, what, total=None):
    """cwf_dice_ce_finalize(_multi) against the float64 finalize of the kernel's own sums"""
    sums = sums.detach().cpu().double().reshape(-1, *sums.shape[-3:])
    r, losses = 0.0, []
    for m in range(sums.shape[0]):
        l_ref, c_ref, A_l = H.finalize(sums[m], V)
        losses.append(l_ref)
        r = max(r, _worst(loss.reshape(-1)[m:m + 1], l_ref.reshape(1), (H.GAMMA_FIN * A_l).reshape(1), what + " loss"))
        r = max(r, _worst(coef.reshape(sums.shape)[m], c_ref, H.GAMMA_FIN * c_ref.abs(), what + " coef"))
    if total is not None:
        nm = sums.shape[0]
        ref = sum(losses)
        A = sum(abs(float(v)) for v in losses)
        r = max(r, _worst(total.reshape(1), ref.reshape(1), torch.tensor([(nm + 1) * H.U * A + H.GAMMA_FIN * A]), what + " total"))
    return r


def fused(hip, name, logits, label, codes, scale, gscale=0.37, pm=None):
    """cwf_head_loss_sums -> cwf_dice_ce_finalize_multi -> cwf_head_loss_bwd on up to three maps; returns the kernel's sums
    and gradients for the layout checks"""
    pm = pm if pm is not None else _masks(codes)[:len(logits)]
    n = label.shape[0]
    Wo = logits[0].shape[3] * scale
    V = label[0].numel()
    ld, lab = [t.to(DEV) for t in logits], label.to(DEV)
    sums = _fused_sums(hip, ld, lab, pm, scale)
    gsum = H.gamma_sums(H.fused_terms_per_thread(Wo))
    r = 0.0
    for m in range(len(logits)):
        mats, t, p, q, S, A = _ref((name, m), logits[m], 2, scale, label, pm[m])
        r = max(r, _check_sums(sums[m], S, A, gsum, "%s map %d sums" % (name, m)))
    loss = torch.empty(len(logits), dtype=torch.float32, device=DEV)
    coef = torch.empty((len(logits), n, 2, 4), dtype=torch.float32, device=DEV)
    total = torch.empty(1, dtype=torch.float32, device=DEV)
    hip._call("cwf_dice_ce_finalize_multi", sums.data_ptr(), loss.data_ptr(), coef.data_ptr(), total.data_ptr(), len(logits), n, V, 2,
              hip._stream())
    r = max(r, _check_finalize(loss, coef, sums, V, name, total))
    gs = torch.tensor([gscale], device=DEV)
    dls = hip.head_loss_bwd(ld, lab, pm, scale, coef, gs)
    for m in range(len(logits)):
        mats, t, p, q, S, A = _ref((name, m), logits[m], 2, scale, label, pm[m])
        c = coef[m].cpu().double()
        ref = H.logit_grad(logits[m], 2, mats, t, c, gscale)
        bound, _ = H.logit_grad_bound(logits[m], 2, mats, t, c, gscale, scale)
        r = max(r, _worst(dls[m][..., :2], ref, bound, "%s map %d dlogit" % (name, m)))
        assert bool((dls[m][..., 2:] == 0).all()), (name, "pad channels")
    _report(name + " fused (sums, finalize_multi, bwd)", r)
    return sums, coef, dls


def unfused(hip, name, logit, label, posmask, scale, gscale=0.37, m=0):
    """cwf_upsample_softmax -> cwf_dice_ce_sums -> cwf_dice_ce_finalize -> cwf_dice_ce_bwd -> cwf_upsample_softmax_bwd (C = 2)"""
    mats, t, p, q, S, A = _ref((name, m), logit, 2, scale, label, posmask)
    n = label.shape[0]
    V = label[0].numel()
    ld, lab = logit.to(DEV), label.to(DEV)
    prob = hip.upsample_softmax(ld, 2, scale)
    r = _worst(prob, p, H.GAMMA_P * q * p, name + " upsample_softmax")
    pk = prob.cpu().double()
    r = max(r, _dice_ce_chain(hip, name, prob, pk, lab, t, posmask, gscale, n, V))
    return r, prob, pk


def _dice_ce_chain(hip, name, prob, pk, lab, t, posmask, gscale, n, V):
    C = prob.shape[-1]
    sums = torch.zeros((n, C, 4), dtype=torch.float64, device=DEV)
    hip._call("cwf_dice_ce_sums", prob.data_ptr(), lab.data_ptr(), int(posmask), sums.data_ptr(), n, V, C, hip._stream())
    S, A = H.sums(pk, t)
    r = _check_sums(sums, S, A, H.gamma_sums(H.unfused_terms_per_thread(n, V), from_logits=False), name + " dice_ce_sums")
    loss = torch.empty(1, dtype=torch.float32, device=DEV)
    coef = torch.empty((n, C, 4), dtype=torch.float32, device=DEV)
    hip._call("cwf_dice_ce_finalize", sums.data_ptr(), loss.data_ptr(), coef.data_ptr(), n, V, C, hip._stream())
    r = max(r, _check_finalize(loss, coef, sums, V, name + " dice_ce_finalize"))
    dprob = hip.dice_ce_bwd(prob, lab, int(posmask), coef, torch.tensor([gscale], device=DEV))
    g, G = H.dprob(pk, t, coef.cpu().double(), gscale)
    r = max(r, _worst(dprob, g, H.GAMMA_DPROB * G, name + " dice_ce_bwd"))
    _unfused_dprob[name] = dprob
    return r


_unfused_dprob = {}


def unfused_bwd(hip, name, prob, pk, lo_shape, scale, ldc_out=4):
    dprob = _unfused_dprob.pop(name)
    mats = H.axis_matrices(lo_shape[1:], scale)
    gk = dprob.cpu().double()
    dl = hip.upsample_softmax_bwd(dprob, prob, lo_shape, 2, scale, ldc_out)
    ref = H.interp_adjoint(H.softmax_adjoint(pk, gk), mats)
    A = H.interp_adjoint(H.softmax_adjoint_mag(pk, gk.abs()), mats)
    r = _worst(dl[..., :2], ref, H.gamma_softmax_bwd(2, scale) * A, name + " upsample_softmax_bwd")
    assert bool((dl[..., 2:] == 0).all())
    return r


def _logits(n, lo, nm, seed, s, ldc=4):
    out = []
    for m in range(nm):
        lg = torch.zeros(n, *lo, ldc)
        lg[..., :2] = _u(n, *lo, 2, seed=seed + m, s=s)
        out.append(lg)
    return out


PRODUCTION = [("region-16^3x8", (16, 16, 16), 8, REGION), ("edge-32^3x4", (32, 32, 32), 4, EDGE),
              ("region-64x96x80", (8, 12, 10), 8, REGION), ("edge-64x96x80", (16, 24, 20), 4, EDGE),
              ("region-160x192x160", (20, 24, 20), 8, REGION), ("edge-160x192x160", (40, 48, 40), 4, EDGE)]


@pytest.mark.parametrize("name,lo,scale,codes", PRODUCTION, ids=[c[0] for c in PRODUCTION])
def test_production_shapes(hip, name, lo, scale, codes):
    """batch 2, three maps, the fused family and (map 0) the unfused chain, at the heads' production shapes"""
    n = 2
    hi = tuple(v * scale for v in lo)
    logits = _logits(n, lo, 3, seed=11, s=4)
    label = _labels(codes, (n,) + hi, seed=12)
    fused(hip, name, logits, label, codes, scale)
    r, prob, pk = unfused(hip, name, logits[0], label, _masks(codes)[0], scale)
    r = max(r, unfused_bwd(hip, name, prob, pk, (n,) + lo, scale))
    _report(name + " unfused chain, map 0", r)
    for m in range(3):
        _REF.pop((name, m), None)


def test_decoder_softmax_dice_128(hip):
    """the decoder's 4-class softmax and Dice + CE at 2 x 4 x 128^3, logits read with a channel stride of 8"""
    n, s = 2, (128, 128, 128)
    buf = torch.zeros(n, *s, 8)
    buf[..., :4] = _u(n, *s, 4, seed=21, s=6)
    lg = buf[..., :4]
    label = _labels(REGION, (n,) + s, seed=22)
    ld = buf.to(DEV)[..., :4]
    prob = hip.channel_softmax(ld, 4)
    p, q = H.probs(lg.double(), 4, None)
    r = _worst(prob, p, H.GAMMA_P * q * p, "decoder channel_softmax")
    pk = prob.cpu().double()
    t = H.target(label, 4)
    lab = label.to(DEV)
    r = max(r, _dice_ce_chain(hip, "decoder", prob, pk, lab, t, 0, 1.3, n, label[0].numel()))
    dprob = _unfused_dprob.pop("decoder")
    gk = dprob.cpu().double()
    dl = hip.channel_softmax_bwd(dprob, prob)
    r = max(r, _worst(dl, H.softmax_adjoint(pk, gk), H.gamma_softmax_bwd(4, 1) * H.softmax_adjoint_mag(pk, gk.abs()),
                       "decoder channel_softmax_bwd"))
    _report("decoder 2 x 4 x 128^3 (softmax, sums, finalize, dprob, softmax_bwd)", r)


GEOMETRY = [("ragged-rows", 2, (4, 3, 8), 4, 3, REGION),       # Ho = 12: one group of 8 rows and a last one of 4
            ("ho-40", 1, (3, 10, 6), 4, 2, EDGE),              # Ho = 40: two row-group blocks, the second with one group
            ("w1", 2, (3, 4, 1), 4, 1, REGION),
            ("w63", 2, (2, 3, 63), 4, 2, EDGE),
            ("w64", 2, (2, 3, 64), 4, 3, REGION),              # the largest row table the LDS holds
            ("scale8-odd-dims", 2, (3, 5, 3), 8, 3, EDGE)]


@pytest.mark.parametrize("name,n,lo,scale,nm,codes", GEOMETRY, ids=[c[0] for c in GEOMETRY])
def test_launch_geometry_edges(hip, name, n, lo, scale, nm, codes):
    hi = tuple(v * scale for v in lo)
    logits = _logits(n, lo, nm, seed=31, s=5)
    label = _labels(codes, (n,) + hi, seed=32)
    fused(hip, name, logits, label, codes, scale, gscale=1.0)
    r, prob, pk = unfused(hip, name, logits[0], label, _masks(codes)[0], scale, gscale=1.0)
    r = max(r, unfused_bwd(hip, name, prob, pk, (n,) + lo, scale))
    _report(name + " unfused chain, map 0", r)
    _REF.clear()


def test_refusals(hip):
    """W = 65 exceeds the sums kernel's LDS row table (CWF_E_TOOLARGE); an odd scale is refused by both backwards (CWF_E_BADARG)"""
    from cwf import _lib
    n, lo = 1, (2, 2, 65)
    ld = [t.to(DEV) for t in _logits(n, lo, 3, seed=41, s=1)]
    label = torch.zeros((n,) + tuple(v * 4 for v in lo), dtype=torch.int64, device=DEV)
    with pytest.raises(_lib.CwfError, match="cwf_head_loss_sums failed with status -2"):
        hip.head_loss(ld, label, _masks(REGION), 4)
    lo3 = (2, 2, 3)
    ld3 = [t.to(DEV) for t in _logits(n, lo3, 2, seed=42, s=1)]
    label3 = torch.zeros((n,) + tuple(v * 3 for v in lo3), dtype=torch.int64, device=DEV)
    coef = torch.zeros((2, n, 2, 4), device=DEV)
    with pytest.raises(_lib.CwfError, match="cwf_head_loss_bwd_ex failed with status -1"):
        hip.head_loss_bwd(ld3, label3, _masks(REGION)[:2], 3, coef, torch.ones(1, device=DEV))
    prob = hip.upsample_softmax(ld3[0], 2, 3)
    with pytest.raises(_lib.CwfError, match="cwf_upsample_softmax_bwd failed with status -1"):
        hip.upsample_softmax_bwd(torch.zeros_like(prob), prob, (n,) + lo3, 2, 3, 4)
    torch.cuda.synchronize()


def test_value_edges(hip):
    """a class absent from sample 1 (no code 3: map "04" has no positive there), sample 0 a single class (all background),
    logit differences of +-12 (probabilities from 6e-6 to 1, both sides of the 0.005 clamp) and gscale = 2.5"""
    n, lo, scale = 2, (6, 5, 8), 4
    hi = tuple(v * scale for v in lo)
    logits = _logits(n, lo, 3, seed=51, s=6)
    label = _labels(REGION, (n,) + hi, seed=52)
    label[0] = 0
    label[1][label[1] == 3] = 2
    for m in range(3):
        _, _, p, _, _, _ = _ref(("values", m), logits[m], 2, scale, label, _masks(REGION)[m])
        assert bool((p < H.CLAMP_LO).any()) and bool((p > 0.5).any())
    sums, coef, _ = fused(hip, "values", logits, label, REGION, scale, gscale=2.5)
    assert float(sums[2, 1, 1, 2]) == 0.0 and float(sums[0, 0, 1, 2]) == 0.0
    r, prob, pk = unfused(hip, "values", logits[2], label, _masks(REGION)[2], scale, gscale=2.5, m=2)
    r = max(r, unfused_bwd(hip, "values", prob, pk, (n,) + lo, scale))
    _report("values unfused chain, map 2", r)
    _REF.clear()


def test_unfused_dprob_clamp_gate(hip):
    """dice_ce_bwd on probabilities placed exactly at 0.005f, one ulp either side, and at 1: the gate is closed below 0.005f only"""
    n, s = 2, (8, 8, 16)
    p = torch.rand(n, *s, generator=torch.Generator().manual_seed(61))
    lo32 = np.float32(0.005)
    vals = [lo32, np.nextafter(lo32, np.float32(0)), np.nextafter(lo32, np.float32(1)), np.float32(1.0), np.float32(0.0)]
    for i, v in enumerate(vals):
        p[0, i, :, :] = float(v)
    prob = torch.stack([1 - p, p], -1).float()
    label = torch.ones((n,) + s, dtype=torch.int64)
    label[1, ::2] = 0
    t = H.target(label, 2, tools.REGION_MASKS["01"])
    pk = prob.double()
    lab, pd = label.to(DEV), prob.to(DEV)
    r = _dice_ce_chain(hip, "clamp", pd, pk, lab, t, tools.REGION_MASKS["01"], 0.8, n, label[0].numel())
    _unfused_dprob.pop("clamp")
    _report("clamp gate: dice_ce sums, finalize, dprob", r)


def test_strided_logits_and_grouped_output(hip):
    """logits as channel slices of one [N,d,h,w,12] buffer (l_ldc = 12); gradients as 4-channel groups of a [N,d,h,w,14] buffer
    (dl_ldc = 14 > dl_ca = 4): pad channels exactly zero, the two channels past the groups untouched; and batch 2 equal, per
    sample, to two batch-1 runs within the bound"""
    n, lo, scale = 2, (4, 6, 8), 4
    hi = tuple(v * scale for v in lo)
    l_all = _u(n, *lo, 12, seed=71, s=4)
    slices = [l_all[..., 4 * q:4 * q + 4] for q in range(3)]
    label = _labels(EDGE, (n,) + hi, seed=72)
    pm = _masks(EDGE)
    sums, coef, dls = fused(hip, "strided", slices, label, EDGE, scale)
    la = l_all.to(DEV)
    d_all = torch.full((n, *lo, 14), 7.5, device=DEV)
    gs = torch.tensor([0.37], device=DEV)
    outs = hip.head_loss_bwd([la[..., 4 * q:4 * q + 4] for q in range(3)], label.to(DEV), pm, scale, coef, gs, grouped_out=(d_all, 4))
    r = 0.0
    for q in range(3):
        mats, t, p, _, _, _ = _ref(("strided", q), slices[q], 2, scale, label, pm[q])
        c = coef[q].cpu().double()
        ref = H.logit_grad(slices[q], 2, mats, t, c, 0.37)
        bound, _ = H.logit_grad_bound(slices[q], 2, mats, t, c, 0.37, scale)
        r = max(r, _worst(d_all[..., 4 * q:4 * q + 2], ref, bound, "grouped dlogit %d" % q))
        assert bool((d_all[..., 4 * q + 2:4 * q + 4] == 0).all())
        assert outs[q].data_ptr() == d_all[..., 4 * q:].data_ptr()
    assert bool((d_all[..., 12:] == 7.5).all()), "channels past the written groups"
    # batch 2 == two batch-1 runs, per sample
    gsum = H.gamma_sums(H.fused_terms_per_thread(lo[2] * scale))
    for i in range(n):
        one = [t[i:i + 1].contiguous().to(DEV) for t in slices]
        s1 = _fused_sums(hip, one, label[i:i + 1].to(DEV), pm, scale)
        d1 = hip.head_loss_bwd(one, label[i:i + 1].to(DEV), pm, scale, coef[:, i:i + 1].contiguous(), gs)
        for q in range(3):
            _, t, p, _, S, A = _ref(("strided", q), slices[q], 2, scale, label, pm[q])
            r = max(r, _worst(s1[q, 0], sums[q, i].cpu().double(), 2 * gsum * A[i], "batch-1 sums, sample %d map %d" % (i, q)))
            mats = H.axis_matrices(lo, scale)
            bound, _ = H.logit_grad_bound(slices[q][i:i + 1], 2, mats, t[i:i + 1], coef[q, i:i + 1].cpu().double(), 0.37, scale)
            r = max(r, _worst(d1[q][..., :2], dls[q][i:i + 1, ..., :2].cpu().double(), 2 * bound, "batch-1 dlogit, sample %d map %d" % (i, q)))
    _report("strided logits, grouped output, batch 2 vs 2 x batch 1", r)
    _REF.clear()


@pytest.mark.parametrize("name,lo,scale,codes", PRODUCTION[:2], ids=[c[0] for c in PRODUCTION[:2]])
def test_python_route_grouped_heads(hip, name, lo, scale, codes):
    """tools.get_separate_loss / get_edge_separate_loss on LazyProb maps whose logits are the 4-channel groups of one buffer (the
    grouped heads of the model): loss and logit gradient against the exact float64 chain, the coefficients' error propagated"""
    from cwf import functional as CF
    n = 2
    hi = tuple(v * scale for v in lo)
    l_all = _u(n, *lo, 12, seed=81, s=4)
    label = _labels(codes, (n,) + hi, seed=82)
    pm = _masks(codes)
    leaf = l_all.to(DEV).requires_grad_(True)
    lz = {k: CF.LazyProb(leaf[..., 4 * q:4 * q + 4], 2, scale, parent=(leaf, q, 3, 4)) for q, k in enumerate(MAPS)}
    loss = (tools.get_separate_loss if codes == REGION else tools.get_edge_separate_loss)(lz, label.to(DEV))
    assert all(z._t is None for z in lz.values())
    (loss * 0.37).backward()
    V = label[0].numel()
    gsum = H.gamma_sums(H.fused_terms_per_thread(lo[2] * scale))
    ref_loss, bound_loss, r = 0.0, 0.0, 0.0
    grad = leaf.grad
    for q in range(3):
        sl = l_all[..., 4 * q:4 * q + 4]
        mats, t, p, _, S, A = _ref((name + "-py", q), sl, 2, scale, label, pm[q])
        l_ref, c_ref, _ = H.finalize(S, V)
        ref_loss += float(l_ref)
        bound_loss += H.loss_error(S, A, gsum, V)
        ref = H.logit_grad(sl, 2, mats, t, c_ref, 0.37)
        bound, _ = H.logit_grad_bound(sl, 2, mats, t, c_ref, 0.37, scale, coef_err=H.coef_error(S, A, gsum, c_ref))
        r = max(r, _worst(grad[..., 4 * q:4 * q + 2], ref, bound, "%s python route dlogit %d" % (name, q)))
        assert bool((grad[..., 4 * q + 2:4 * q + 4] == 0).all())
    bound_loss += 4 * H.U * abs(ref_loss)
    r = max(r, _worst(loss.detach().reshape(1), torch.tensor([ref_loss], dtype=torch.float64), torch.tensor([bound_loss]), name + " python route loss"))
    _report(name + " python route (LazyProb, grouped)", r)
    _REF.clear()
