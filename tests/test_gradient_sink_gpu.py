"""GPU: the bf16-only gradient hand-off under a gradient sink.  An InstanceNorm-backward apply pass may leave the fp32 gradient of its
input unwritten and hand on only its bf16 image (in_bwd_apply16(..., need_f32=False)) -- correct only where that tensor has ONE gradient
consumer, which a model declares for its own forward pass (functional.single_consumer_graph; ClsWiseFormer does).  Graphs built
elsewhere in the same process, after such a model has run, must keep their fp32 gradients."""
import math

import pytest
import torch
import torch.nn.functional as F

from oracle import reference_model as rm
from test_kernels_gpu import PREC_TOL, close, rnd
from utils import synthetic as syn

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _clswiseformer():
    from models.clswiseformer.cls_wise_former import get_cls_wise_former
    m = get_cls_wise_former(dataset="brats", _conv_repr=True, _pe_type="fixed")
    m.load_state_dict(syn.det_state_dict(rm.param_shapes()), strict=False)
    m.Unet_list.InitConv.dropout = 0.0
    return m.to(DEV)


def _two_consumer_graph(site, n, size):
    """y = conv_A(x) (16 -> 16, no residual: the conv marks it for the bf16-only hand-off) with TWO gradient consumers:
       "conv":          conv_B(act(IN(y)))                            (the IN backward is conv_B's apply pass)
       "norm_act_add":  conv_B(norm_act_add(y))                       (the IN backward is the block tail's apply pass)
    and (y * r).sum(), r scaled so that both consumers' gradients of y are of one size.  Returns the sink gradients of
    (w_A, b_A, w_B, b_B) and the float64 torch reference of the same graph (NCDHW)."""
    from cwf import functional as CF, packing as pk
    from cwf.optim import GradSink
    K = CF.backend()
    d, h, w_ = size
    x = rnd(n, d, h, w_, 16, seed=51)
    q = rnd(n, d, h, w_, 16, seed=52)
    r0 = rnd(n, d, h, w_, 16, seed=53)
    wa, wb = (rnd(16, 16, 3, 3, 3, seed=s, scale=1.0 / math.sqrt(16 * 27)) for s in (54, 55))
    ba, bb = rnd(16, seed=56, scale=0.1), rnd(16, seed=57, scale=0.1)

    # ---- float64 reference; r matched to the first consumer's gradient of y
    ncd = lambda t: t.permute(0, 4, 1, 2, 3).double()
    par = [t.double().clone().requires_grad_(True) for t in (wa, ba, wb, bb)]
    y64 = F.conv3d(ncd(x), par[0], par[1], padding=1)
    a64 = F.leaky_relu(F.instance_norm(y64, eps=1e-5), 0.01)
    z64 = F.conv3d(a64, par[2], par[3], padding=1)
    g1 = torch.autograd.grad((z64 * ncd(q)).sum(), y64, retain_graph=True)[0]
    r = r0 * float(g1.norm() / r0.norm())
    ((z64 * ncd(q)).sum() + (y64 * ncd(r)).sum()).backward()
    ref = [p.grad for p in par]

    # ---- the HIP graph under a gradient sink
    params = [torch.nn.Parameter(t.to(DEV).contiguous()) for t in (wa, ba, wb, bb)]
    spec_a, spec_b = CF.ConvSpec(pk.CONV3_S1, 16, 16), CF.ConvSpec(pk.CONV3_S1, 16, 16)
    packer = CF.WeightPacker()
    packer.add(spec_a, params[0])
    packer.add(spec_b, params[2])
    packer.refresh()
    sink = GradSink(params)
    xd, qd, rd = x.to(DEV), q.to(DEV), r.float().to(DEV)
    y, st = CF.conv(xd, params[0], params[1], spec_a, want_stats=True)
    if site == "conv":
        z, _ = CF.conv(y, params[2], params[3], spec_b, in_norm=st, slope=0.01)
    else:
        z, _ = CF.conv(CF.norm_act_add(y, st, 0.01), params[2], params[3], spec_b)
    loss = (z * qd).sum() + (y * rd).sum()
    sink.begin()
    with sink:
        loss.backward()
    K.wgrad_flush()
    torch.cuda.synchronize()
    assert all(p.grad is None for p in params)                 # every gradient went through the sink
    return [sink.view(p) for p in params], ref


def test_bf16_only_gradient_handoff_is_confined_to_the_declaring_model(hip, monkeypatch):
    """After a ClsWiseFormer forward has run in the process, a standalone graph whose 16 -> 16 conv output has a second consumer gets
    the fp32 gradient of that output written (need_f32=True) and correct gradients, at both apply-pass sites; the model's own
    Trainer step still takes the bf16-only hand-off."""
    from cwf import kernels
    from cwf.trainer import Trainer
    seen = []
    apply16 = hip.in_bwd_apply16

    def spy(*a, **kw):
        seen.append(kw.get("need_f32", True))
        return apply16(*a, **kw)
    monkeypatch.setattr(hip, "in_bwd_apply16", spy)
    kernels.set_precision("bf16x3", wgrad="bf16", dgrad="bf16")
    try:
        x, target, edge = syn.synthetic_batch([0], (64, 64, 64))
        x, target, edge = x.to(DEV), target.to(DEV), edge.to(DEV)
        with torch.no_grad():
            _clswiseformer().eval()(x, None)                    # the model declares single-consumer tensors for ITS forward pass
        for site in ("conv", "norm_act_add"):
            seen.clear()
            got, ref = _two_consumer_graph(site, 2, (34, 38, 50))
            assert seen and all(seen), (site, seen)
            for g, r, what in zip(got, ref, ("w_A", "b_A", "w_B", "b_B")):
                assert bool(torch.isfinite(g).all()), (site, what)
                close(g, r, rtol=PREC_TOL["bf16"], what="%s %s" % (site, what))
        # the declaring model keeps the hand-off (a fix that turned it off would cost the benchmark an fp32 write per element)
        seen.clear()
        tr = Trainer(_clswiseformer().train())
        tr._fwd_bwd(x, target, edge)
        torch.cuda.synchronize()
        assert False in seen, seen
        assert bool(torch.isfinite(tr.opt.flat_grad).all())
    finally:
        kernels.set_precision("fp32")
