"""GPU: EVERY element of EVERY parameter gradient of the assembled model against the imported reference's float64 run, on each path
that produces gradients -- plain autograd in three precisions, the Trainer's gradient sink (twice: the second step runs on cached
descriptor tables and slabs) and the planned step -- at 64^3, at 64x96x80 and at batch 2 (tests/golden/grads_{64,noncubic,64_b2}.npz).

The fixtures hold a count-sketch of each of the 218 gradients (tests/grad_sketch.py: 256 signed bucket sums, tensors of at most 256
elements whole); the sketch is taken on the device and only 256 numbers per tensor cross to the host.  Top-k selections are
teacher-forced from the fixture.  The bound on the sketch distance d of a live tensor (reference norm above 1e-7) is

    d <= 1.25 * max(10 * noise_sketch, 1e-2)        fp32, bf16x3
    d <= 1.25 * max(10 * noise_sketch, 2e-2)        single-bf16 gradient operands (the bench precision)

1e-2 / 2e-2 are the elementwise figures test_model_gpu.py holds the ten full gradients to, noise_sketch is the reference's own fp32 run
measured against its float64 run in this metric, 1.25 is the estimator's four sigma (test_grad_sketch_cpu.py): nothing in the bound
comes from the code under test.  A tensor at or below 1e-7 (a bias in front of an InstanceNorm, two LayerNorm vectors the fusion
coupler's output never reaches: true gradient zero) must stay at or below 1e-5 in norm.

Worst d / bound per path (MI355X, `pytest -s`): DESIGN.md section 3."""
import functools
import os

import numpy as np
import pytest
import torch

import grad_sketch as gs
from conftest import GOLDEN
from test_model_gpu import DEV, _flat_by_name, _losses, _model, _no_dropout_model
from utils import synthetic as syn

pytestmark = pytest.mark.gpu

TAGS = ("64", "noncubic", "64_b2")
BENCH = "bf16x3+bf16grad"
FLOOR = {"fp32": 1e-2, "bf16x3": 1e-2, BENCH: 2e-2}

# The one finding.  A conv bias in front of an InstanceNorm has the true gradient zero: the norm's backward returns a dy whose sum over
# a channel's voxels is 0.  The weight-gradient kernels compute the bias gradient as the row "ones . dy" of the same MFMA product, so
# with wgrad="bf16" dy enters it as ONE bf16 operand and what is left is the sum of its rounding residues, 2^-9 relative each with
# random sign: these eleven come out between 1.0e-5 and 3.7e-5 in norm (below), above the 1e-5 they keep in fp32 and bf16x3 (hi + lo
# operands).  No cause but operand rounding; the bias has no effect behind an InstanceNorm.  In the bench precision _hold() leaves these
# names to test_true_zero_bias_gradients_in_the_bench_precision, a strict expected failure, and holds every other tensor.
BF16_BIAS_ROW = tuple("%s.bias" % n for n in (
    "conv_semantic_1", "conv_semantic_2", "conv_semantic_4", "Unet_list.EnBlock1.conv1", "Unet_list.EnBlock1_1.conv1",
    "Unet_list.EnBlock2_1.conv1", "Unet_list.EnBlock2_2.conv1", "Unet_list.EnBlock3_1.conv1", "Unet_list.EnBlock3_2.conv1",
    "Unet_list.EnBlock4_1.conv1", "Unet_list.EnBlock4_2.conv1"))


@functools.lru_cache(maxsize=None)
def _case(tag):
    """the fixture, its inputs on the device and its top-k sets as forced_index"""
    fx = np.load(os.path.join(GOLDEN, "grads_%s.npz" % tag))
    fx = {k: fx[k] for k in fx.files}
    x, target, edge = syn.synthetic_batch([int(s) for s in fx["samples"]], tuple(int(v) for v in fx["size"]))
    forced = {k[5:]: torch.from_numpy(v).long().to(DEV) for k, v in fx.items() if k.startswith("topk_")}
    return fx, (x.to(DEV), target.to(DEV), edge.to(DEV)), forced


def _set_precision(mode):
    from cwf import kernels
    if mode == BENCH:
        kernels.set_precision("bf16x3", wgrad="bf16", dgrad="bf16")
    else:
        kernels.set_precision(mode)


def _hold(fx, got, parts, mode, what):
    """the assertions every run makes: loss parts, finiteness (in gs.check), every live tensor within its bound, every other one
    small, and the number of tensors not held to a bound equal to the fixture's own"""
    parts = [float(v.detach()) for v in parts]
    assert np.allclose(parts, fx["loss_parts"], rtol=1e-4), (what, parts, fx["loss_parts"])
    over, dead, worst = gs.check(fx, got, FLOOR[mode], dead_excused=BF16_BIAS_ROW if mode == BENCH else ())
    print("%s: worst d / bound %.3f (%s); %d tensors not live, largest norm %.2e (%s)" % (
        (what, worst[0], worst[1], len(dead)) + max((v, n) for n, v in dead.items() if mode != BENCH or n not in BF16_BIAS_ROW)))
    assert len(dead) == int(fx["n_not_live"]), (what, len(dead))
    assert not over, (what, over[:10])
    return worst


@pytest.mark.parametrize("mode", ["fp32", "bf16x3", BENCH])
@pytest.mark.parametrize("tag", TAGS)
def test_autograd_gradients_vs_reference_sketch(hip, tag, mode):
    """sum(losses).backward() on the model, per-parameter .grad"""
    fx, (x, target, edge), forced = _case(tag)
    _set_precision(mode)
    try:
        m = _model().eval()
        m.forced_index = forced
        parts = _losses(m(x, None), target, edge)
        sum(parts).backward()
        got = {n: p.grad for n, p in m.named_parameters()}
        assert all(g is not None for g in got.values())
        _hold(fx, got, parts, mode, "autograd %s %s" % (tag, mode))
    finally:
        _set_precision("fp32")


@pytest.mark.parametrize("tag", TAGS)
def test_sink_gradients_vs_reference_sketch(hip, tag):
    """Trainer._fwd_bwd in the bench precision: the backward kernels write the flat buffer (grouped launches, slab reduces, side-stream
    weight gradients, coupler Functions writing in place); twice."""
    from cwf.trainer import Trainer
    fx, (x, target, edge), forced = _case(tag)
    _set_precision(BENCH)
    try:
        m = _no_dropout_model(forced)
        tr = Trainer(m)
        assert tr.wgrad_async
        for rep in range(2):
            loss, parts = tr._fwd_bwd(x, target, edge)
            torch.cuda.synchronize()
            assert all(p.grad is None for p in m.parameters())
            assert abs(float(loss) - float(fx["loss"])) <= 1e-4 * abs(float(fx["loss"]))
            _hold(fx, _flat_by_name(m, tr), parts, BENCH, "sink %s step %d" % (tag, rep))
    finally:
        _set_precision("fp32")


@pytest.mark.parametrize("tag", TAGS)
def test_planned_step_gradients_vs_reference_sketch(hip, tag):
    """Trainer(use_graph="plan") as bench.py runs it: one eager warm-up step, the capture, one replay of the launch list; learning rate
    and weight decay 0, so that the replay sees the fixture's weights."""
    from cwf.trainer import Trainer
    fx, (x, target, edge), forced = _case(tag)
    _set_precision(BENCH)
    try:
        m = _no_dropout_model(forced)
        w0 = torch.cat([p.detach().reshape(-1) for p in m.parameters()]).clone()
        tr = Trainer(m, use_graph="plan", graph_warmup=1, lr=0.0, weight_decay=0.0)
        tr.step(x, target, edge, 0)
        assert tr._plan is None
        loss, parts = tr.step(x, target, edge, 0)
        torch.cuda.synchronize()
        assert tr._plan is not None and "error" not in tr.plan_info, tr.plan_info
        assert torch.equal(torch.cat([p.detach().reshape(-1) for p in m.parameters()]), w0)
        _hold(fx, _flat_by_name(m, tr), parts, BENCH, "plan %s" % tag)
    finally:
        _set_precision("fp32")


@pytest.mark.xfail(strict=True, reason="single-bf16 dy operand in the weight-gradient kernels' bias row: the true-zero gradients of %d conv "
                   "biases in front of an InstanceNorm reach 1.0e-5 .. 3.7e-5 in norm (operand rounding; DESIGN.md section 3)" % len(BF16_BIAS_ROW))
@pytest.mark.parametrize("tag", TAGS)
def test_true_zero_bias_gradients_in_the_bench_precision(hip, tag):
    """Every tensor whose reference gradient is zero (norm <= 1e-7) stays at or below 1e-5 in norm -- in the bench precision, on the
    path bench.py times.  Expected to fail, strictly, for the tensors named in BF16_BIAS_ROW and for the reason given there; the bound is
    the one fp32 and bf16x3 are held to and is not raised.  Measured, MI355X (the same on the autograd, sink and planned paths):
      64^3      Unet_list.EnBlock1_1.conv1.bias 3.66e-5, EnBlock2_1 3.48e-5, EnBlock1 2.72e-5, conv_semantic_2.bias 2.66e-5, EnBlock3_1
                2.32e-5, EnBlock2_2 2.19e-5, EnBlock4_1 1.53e-5, conv_semantic_4 1.49e-5, EnBlock3_2 1.49e-5, conv_semantic_1 1.44e-5,
                EnBlock4_2 1.12e-5
      64x96x80  EnBlock1 2.53e-5, EnBlock2_1 1.93e-5, EnBlock1_1 1.52e-5, EnBlock3_1 1.45e-5, conv_semantic_2 1.38e-5, EnBlock2_2
                1.09e-5, EnBlock4_1 1.04e-5
      64^3 B=2  EnBlock1 2.60e-5, EnBlock2_1 2.28e-5, conv_semantic_2 2.15e-5, EnBlock1_1 2.07e-5, EnBlock3_1 1.51e-5, EnBlock2_2
                1.27e-5, EnBlock4_1 1.27e-5, EnBlock3_2 1.23e-5, conv_semantic_1 1.13e-5"""
    from cwf.trainer import Trainer
    fx, (x, target, edge), forced = _case(tag)
    _set_precision(BENCH)
    try:
        m = _no_dropout_model(forced)
        tr = Trainer(m)
        tr._fwd_bwd(x, target, edge)
        torch.cuda.synchronize()
        _, dead, _ = gs.check(fx, _flat_by_name(m, tr), FLOOR[BENCH])
        big = sorted(((v, n) for n, v in dead.items() if v > gs.DEAD_L2_MAX), reverse=True)
        print("true-zero gradients above %.0e, %s: %s" % (gs.DEAD_L2_MAX, tag, ["%s %.2e" % (n, v) for v, n in big]))
    finally:
        _set_precision("fp32")
    assert not big


def test_check_reports_exactly_the_edited_tensors(hip):
    """The check bites on device data: the fp32 gradients of the 64^3 run pass; copies with the five edits a per-tensor norm cannot
    see (each keeps every norm to under 1 %) are reported, for the edited tensors and no others."""
    fx, (x, target, edge), forced = _case("64")
    m = _model().eval()
    m.forced_index = forced
    parts = _losses(m(x, None), target, edge)
    sum(parts).backward()
    got = {n: p.grad.detach() for n, p in m.named_parameters()}
    conv, qkv, end = "Unet_list.EnBlock2_1.conv1.weight", "transformer_04.cross_attention_list.0.fn.fn.qkv.weight", "decoder.endconv.weight"
    pa, pb = ["transformer_0%d.cross_attention_list.0.fn.fn.out_proj.weight" % k for k in (1, 2)]
    assert tuple(got[conv].shape) == (32, 32, 3, 3, 3) and tuple(got[qkv].shape) == (1536, 512) and got[pa].shape == got[pb].shape
    rolled = got[conv].clone()
    rolled[:, -16:] = torch.roll(got[conv][:, -16:], 4, dims=1)
    less = gs.remove_orthogonal_component(got[end].double().cpu().numpy(), 0.14, np.random.default_rng(0))
    edits = {
        "taps mirrored": {conv: got[conv].flip(3)},
        "q and k rows exchanged": {qkv: torch.cat([got[qkv][512:1024], got[qkv][:512], got[qkv][1024:]])},
        "two tensors exchanged": {pa: got[pb] * (got[pa].norm() / got[pb].norm()), pb: got[pa] * (got[pb].norm() / got[pa].norm())},
        "input channels rolled": {conv: rolled},
        "orthogonal 14 % removed": {end: torch.from_numpy(less).to(got[end])},
    }
    assert gs.check(fx, got, 1e-2)[0] == []
    for edit in edits.values():
        for n, v in edit.items():
            assert v.shape == got[n].shape and abs(float(v.norm() / got[n].norm()) - 1.0) < 1e-2, n
    # two rounds, each a check of all 218 tensors: the edits that touch different tensors together, the second edit of the conv weight alone
    for rnd in (("taps mirrored", "q and k rows exchanged", "two tensors exchanged", "orthogonal 14 % removed"), ("input channels rolled",)):
        edited = {n: v for what in rnd for n, v in edits[what].items()}
        assert len(edited) == sum(len(edits[what]) for what in rnd)
        over, _, _ = gs.check(fx, {**got, **edited}, 1e-2)
        print("%s: %s" % (", ".join(rnd), ["%s d %.3f bound %.3f" % o for o in over]))
        assert sorted(n for n, _, _ in over) == sorted(edited), (rnd, over)
