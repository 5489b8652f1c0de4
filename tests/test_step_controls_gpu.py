"""Step controls on the GPU (csrc/grad_step.hip and their way up through cwf.optim.FusedAdam and cwf.trainer.Trainer): gradient
accumulation over micro-batches, clipping by global norm, EMA weights.  Yardstick: tests/step_controls_ref.py."""
import functools
import math
import os

import numpy as np
import pytest
import torch

import step_controls_ref as ref
from oracle import reference_model as rm
from utils import synthetic as syn

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# The grid of cwf_grad_add is capped at 1024 workgroups x 256 threads, each moving two 16-byte groups per trip of its grid-stride
# loop: one pass covers 2^21 floats, so 2^20 + 5 still fits in one and 2^22 + 3 is the size that takes a second trip.
SIZES = (1, 3, 4, 255, 1027, (1 << 20) + 5, (1 << 22) + 3)
OFFSETS = (0, 1, 2, 3)


def _buf(n, off, gen, scale=1.0):
    """a float32 [n] view `off` floats past a 16-byte aligned address, with one sentinel element on either side"""
    base = torch.empty(n + 12, dtype=torch.float32, device=DEV)
    assert base.data_ptr() % 16 == 0
    base.fill_(-777.0)
    v = base[4 + off:4 + off + n]
    v.copy_((torch.randn(n, generator=gen) * scale).to(DEV))
    return base, v


def _sentinels_intact(base, off, n):
    return float(base[4 + off - 1]) == -777.0 and float(base[4 + off + n]) == -777.0


# ------------------------------------------------------------------------------------------------------------------ cwf_grad_add
@pytest.mark.parametrize("n", SIZES)
def test_grad_add_is_one_rounded_addition_at_every_offset(hip, n):
    gen = torch.Generator().manual_seed(n)
    for off in OFFSETS:
        (ba, a), (bb, b), (by, y) = _buf(n, off, gen), _buf(n, off, gen, 1e-3), _buf(n, off, gen)
        want = a + b
        hip.grad_add(a, b, y)
        assert torch.equal(y, want) and _sentinels_intact(by, off, n), (n, off)
        hip.grad_add(a, None, y)                                   # b = NULL: a copy
        assert torch.equal(y, a) and _sentinels_intact(by, off, n), (n, off)
        a0 = a.clone()
        hip.grad_add(a, b, a)                                      # in place on a
        assert torch.equal(a, want) and _sentinels_intact(ba, off, n), (n, off)
        hip.grad_add(a0, b, b)                                     # in place on b
        assert torch.equal(b, want) and _sentinels_intact(bb, off, n), (n, off)
    # pointers that are not congruent mod 16 take the scalar path
    (ba, a), (bb, b), (by, y) = _buf(n, 1, gen), _buf(n, 2, gen), _buf(n, 3, gen)
    hip.grad_add(a, b, y)
    assert torch.equal(y, a + b) and _sentinels_intact(by, 3, n)


def test_grad_entry_points_check_their_arguments(hip):
    from cwf import _lib
    a = torch.zeros(8, device=DEV)
    ws = torch.zeros(_lib.GRADNORM_WS_DOUBLES, dtype=torch.float64, device=DEV)
    out2 = torch.zeros(2, device=DEV)
    L, s = hip.lib, hip._stream()
    assert L.cwf_grad_add(0, a.data_ptr(), a.data_ptr(), 8, s) == -1 and L.cwf_grad_add(a.data_ptr(), 0, 0, 8, s) == -1
    assert L.cwf_grad_add(a.data_ptr(), 0, a.data_ptr(), 0, s) == -1
    for g, n, mx, w, o in ((0, 8, 1.0, ws.data_ptr(), out2.data_ptr()), (a.data_ptr(), 0, 1.0, ws.data_ptr(), out2.data_ptr()),
                           (a.data_ptr(), 8, -1.0, ws.data_ptr(), out2.data_ptr()), (a.data_ptr(), 8, float("nan"), ws.data_ptr(), out2.data_ptr()),
                           (a.data_ptr(), 8, 1.0, 0, out2.data_ptr()), (a.data_ptr(), 8, 1.0, ws.data_ptr(), 0)):
        assert L.cwf_grad_norm_clip(g, n, 1.0, mx, w, o, s) == -1
    t = torch.zeros(6, dtype=torch.int64, device=DEV)
    adam = lambda table, step, ema, w: L.cwf_adam_amsgrad_ex(table, 1, 8, 2e-4, 0.9, 0.999, 1e-8, 0.0, step, 1, 0, 1.0, 0, ema, w, s)
    assert adam(0, 1, 0, 0.0) == -1 and adam(t.data_ptr(), 0, 0, 0.0) == -1
    for w in (0.0, -0.1, 0.6, float("nan")):
        assert adam(t.data_ptr(), 1, t.data_ptr(), w) == -1
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------------------ cwf_grad_norm_clip
def _norm_clip(hip, g, grad_scale, max_norm):
    from cwf import _lib
    ws = torch.full((_lib.GRADNORM_WS_DOUBLES,), float("nan"), dtype=torch.float64, device=DEV)
    out2 = torch.full((2,), float("nan"), device=DEV)
    hip.grad_norm_clip(g, grad_scale, max_norm, ws, out2)
    return out2.cpu().numpy().copy(), ws.cpu().numpy().copy()


def _check_norm(out2, g_host, grad_scale, max_norm, what):
    coef, norm = ref.clip_coef64(ref.sq_norm64(g_host), grad_scale, max_norm)
    want_norm = np.float32(norm)
    assert np.isfinite(out2).all(), (what, out2)
    assert abs(float(out2[1]) - float(want_norm)) <= 2.0 ** -23 * float(want_norm), (what, out2[1], want_norm)
    assert abs(float(out2[0]) - coef) <= 2.0 ** -22 * coef, (what, out2[0], coef)
    return coef, norm


@pytest.mark.parametrize("n", SIZES)
def test_grad_norm_clip_against_the_float64_formula(hip, n):
    """out2[1] against float32(grad_scale sqrt(S64)) within 2^-23 relative -- every square is exact in double, the double sum is off
    by less than n 2^-53 ~ 5e-10 relative at n = 2^22, what is left is the fp32 rounding of the result -- and out2[0] against the
    float64 coefficient within 2^-22; bit-equal results and partials from two runs."""
    gen = torch.Generator().manual_seed(100 + n)
    for off in OFFSETS:
        base, g = _buf(n, off, gen, 0.37)
        gh = g.cpu().numpy()
        l2 = math.sqrt(ref.sq_norm64(gh))
        for grad_scale, max_norm in ((1.0, 0.5 * l2), (1.0 / 3.0, 0.1 * l2), (0.5, 2.0 * l2), (0.125, float("inf"))):
            out2, ws = _norm_clip(hip, g, grad_scale, max_norm)
            coef, _ = _check_norm(out2, gh, grad_scale, max_norm, (n, off, grad_scale, max_norm))
            assert not np.isnan(ws).any()                          # every workgroup stored its partial
            if max_norm >= grad_scale * l2 + 1e-3:                 # a norm below max_norm, and max_norm = +inf: exactly grad_scale
                assert out2[0] == np.float32(grad_scale)
            out2b, wsb = _norm_clip(hip, g, grad_scale, max_norm)
            assert out2.tobytes() == out2b.tobytes() and ws.tobytes() == wsb.tobytes()
        assert _sentinels_intact(base, off, n)


def test_grad_norm_clip_zero_and_huge_inputs(hip):
    n = 1027
    z = torch.zeros(n, device=DEV)
    out2, _ = _norm_clip(hip, z, 0.25, 1.0)
    assert out2[1] == 0.0 and out2[0] == np.float32(0.25)
    # one element 1e30: its fp32 square overflows; the double one does not
    z[700] = 1e30
    out2, _ = _norm_clip(hip, z, 0.5, 1.0)
    _check_norm(out2, z.cpu().numpy(), 0.5, 1.0, "1e30")
    assert abs(float(out2[1]) - 0.5e30) <= 2.0 ** -22 * 0.5e30
    # a non-finite sum propagates as in torch: inf -> coefficient 0 (g * 0 = NaN for the inf element), NaN -> NaN
    z[3] = float("inf")
    out2, _ = _norm_clip(hip, z, 0.5, 1.0)
    assert np.isinf(out2[1]) and out2[0] == 0.0
    z[3] = float("nan")
    out2, _ = _norm_clip(hip, z, 0.5, 1.0)
    assert np.isnan(out2).all()


# ------------------------------------------------------------------------------------------------------------------ cwf_adam_amsgrad_ex
@functools.lru_cache(maxsize=None)
def _inputs():
    return ref.make_inputs()


@functools.lru_cache(maxsize=None)
def _yardstick(max_norm, ema_decay, grad_scale=1.0):
    p0, grads = _inputs()
    r64 = ref.run_torch(p0, grads, torch.float64, max_norm=max_norm, ema_decay=ema_decay, grad_scale=grad_scale)
    r32 = ref.run_torch(p0, grads, torch.float32, max_norm=max_norm, ema_decay=ema_decay, grad_scale=grad_scale)
    own = {k: [ref.rel_l2(a, b) for a, b in zip(r32[k], r64[k])] for k in ref.MOMENTS}
    return r64, own


def _run_fused(max_grad_norm, ema_decay, grad_scale=1.0):
    from cwf.optim import FusedAdam
    p0, grads = _inputs()
    ps = [torch.nn.Parameter(t.clone().to(DEV)) for t in p0]
    opt = FusedAdam(ps, lr=ref.LR, weight_decay=ref.WD, amsgrad=True, max_grad_norm=max_grad_norm, ema_decay=ema_decay)
    opt.grad_scale = grad_scale
    norms = []
    for gs in grads:
        for p, g in zip(ps, gs):
            p.grad = g.to(DEV)
        opt.step()
        if max_grad_norm is not None:
            norms.append(opt.grad_norm.clone())
    torch.cuda.synchronize()
    return ps, opt, norms


@pytest.mark.parametrize("max_norm,decay", [(1.0, 0.9), (1.0, 0.999), (100.0, 0.9)])
def test_adam_ex_clip_and_ema_against_float64_torch(hip, max_norm, decay):
    """Five tensors of 1 .. 65,537 elements, six steps, gradient scale alternating 0.01 / 10: weights and EMA within rtol 1e-6 /
    atol 1e-7 of the float64 run of torch's Adam + clip_grad_norm_ + lerp_; each moment within 8 x the relative L2 error fp32 torch
    itself has against that run on the same inputs (the margin covers an equally valid fp32 evaluation: fma contraction, a
    coefficient from a double sum where torch sums in fp32 -- each moves the last bit of an operation, no more; an absolute bound
    would be vacuous: the second moments are ~1e-11 under clipping).  (100, 0.9) adds steps on which the clip is idle."""
    r64, own = _yardstick(max_norm, decay)
    ps, opt, norms = _run_fused(max_norm, decay)
    for i, p in enumerate(ps):
        assert ref.close(p, r64["w"][i]), ("w", i)
        assert ref.close(opt.ema[i], r64["ema"][i]), ("ema", i)
        for k in ref.MOMENTS:
            err = ref.rel_l2(opt.state[p][k], r64[k][i])
            print("%s[%d]: %.3g (fp32 torch %.3g)" % (k, i, err, own[k][i]))
            assert err <= ref.MOMENT_MARGIN * own[k][i], (k, i, err, own[k][i])
    for got, want in zip(norms, r64["norms"]):
        assert abs(float(got) - want) <= 2.0 ** -22 * want
    sd = opt.state_dict()                                         # torch's layout: loads into torch.optim.Adam
    topt = torch.optim.Adam([torch.nn.Parameter(t.clone().to(DEV)) for t in _inputs()[0]], lr=ref.LR, weight_decay=ref.WD, amsgrad=True)
    topt.load_state_dict(sd)
    tp = topt.param_groups[0]["params"]
    assert all(torch.equal(topt.state[tp[i]]["max_exp_avg_sq"], opt.state[ps[i]]["max_exp_avg_sq"]) for i in range(len(ps)))
    assert all(set(s.keys()) == {"step", "exp_avg", "exp_avg_sq", "max_exp_avg_sq"} for s in sd["state"].values())


def test_adam_ex_device_scale_equals_the_scaled_entry_point(hip):
    """gscale_dev = {v}, no EMA, against cwf_adam_amsgrad_scaled(grad_scale = v): weights and moments within the bounds above of each
    other (they run the same operations), and an EMA table that is not passed stays untouched."""
    v = 0.3
    r64, own = _yardstick(None, None, v)
    ps_a, opt_a, _ = _run_fused(None, None, grad_scale=v)        # cwf_adam_amsgrad_scaled
    p0, grads = _inputs()
    from cwf.optim import FusedAdam
    ps = [torch.nn.Parameter(t.clone().to(DEV)) for t in p0]
    opt = FusedAdam(ps, lr=ref.LR, weight_decay=ref.WD, amsgrad=True)
    opt._ensure()
    gdev = torch.tensor([v, 123.0], device=DEV)
    ema = [torch.full_like(p, 5.0) for p in ps]
    for gs in grads:
        for p, g in zip(ps, gs):
            p.grad = g.to(DEV)
        opt.sink.begin(); opt.gather_grads(); opt.advance_host()
        hip.adam_ex(opt._table, len(ps), opt._max_n, ref.LR, 0.9, 0.999, 1e-8, ref.WD, opt._steps, True, grad_scale=77.0, gscale_dev=gdev)
    torch.cuda.synchronize()
    for i in range(len(ps)):
        assert ref.close(ps[i], ps_a[i]) and ref.close(ps[i], r64["w"][i]), i
        for k in ref.MOMENTS:
            assert ref.rel_l2(opt.state[ps[i]][k], opt_a.state[ps_a[i]][k]) <= ref.MOMENT_MARGIN * own[k][i], (k, i)
        assert bool((ema[i] == 5.0).all())


# ------------------------------------------------------------------------------------------------------------------ Trainer, 64^3
def _model():
    from models.clswiseformer.cls_wise_former import get_cls_wise_former
    m = get_cls_wise_former(dataset="brats", _conv_repr=True, _pe_type="fixed")
    m.load_state_dict(syn.det_state_dict(rm.param_shapes()), strict=False)
    m.Unet_list.InitConv.dropout = 0.0
    return m.to(DEV)


def _no_dropout_model(forced):
    m = _model().train()
    m.forced_index = forced
    for mod in m.modules():
        if hasattr(mod, "dropout_rate"):
            mod.dropout_rate = 0.0
        if isinstance(mod, torch.nn.Dropout):
            mod.p = 0.0
    return m


def _weights(tr):
    return torch.cat([p.detach().reshape(-1) for p in tr.model.parameters()])


@functools.lru_cache(maxsize=None)
def _window_reference():
    """Computed once, outside any process group: the teacher-forced top-k indices, the batches (samples 0 and 5), g(0) and g(5) from
    _fwd_bwd runs of a plain Trainer on the start weights, the eager-against-eager noise, and the weights a plain FusedAdam step on
    g(0) + g(5) with grad_scale 1/2 leaves."""
    from cwf import kernels
    from cwf.optim import FusedAdam
    from cwf.trainer import Trainer
    kernels.set_precision("bf16x3")
    try:
        xs, ts, es = zip(*[syn.synthetic_batch([i], (64, 64, 64)) for i in (0, 5)])
        with torch.no_grad():
            _, aux = rm.forward(syn.det_state_dict(rm.param_shapes()), xs[0], return_aux=True)
        forced = {k: v.to(DEV) for k, v in aux.items() if v.dtype == torch.int64}
        batches = [(xs[i].to(DEV), ts[i].to(DEV), es[i].to(DEV)) for i in (0, 1)]
        eager = []
        for rep in range(2):
            tr = Trainer(_no_dropout_model(forced))
            assert not tr.comm
            per = []
            for i in (0, 1):
                tr._fwd_bwd(*batches[i])
                torch.cuda.synchronize()
                per.append(tr.opt.flat_grad.clone())
            eager.append(per)
        noise = max(float((eager[0][i] - eager[1][i]).norm() / eager[0][i].norm()) for i in (0, 1))
        gsum = eager[0][0] + eager[0][1]
        w_start = _weights(tr).clone()

        def plain_step(scale):
            m = _no_dropout_model(forced)
            opt = FusedAdam(m.parameters(), lr=2e-4, weight_decay=1e-5, amsgrad=True, phases=m.grad_phases())
            opt._ensure()
            opt.flat_grad.copy_(gsum)
            opt.grad_scale = scale
            opt.advance_host(); opt.launch()
            torch.cuda.synchronize()
            return torch.cat([p.detach().reshape(-1) for p in m.parameters()])

        return dict(forced=forced, batches=batches, noise=noise, gsum=gsum, w_start=w_start, plain_step=plain_step,
                    w_half=plain_step(0.5), norm=0.5 * float(gsum.double().norm()))
    finally:
        kernels.set_precision("fp32")


def _window(R, use_graph, **kw):
    """One accumulation window (samples 0 then 5) on the start weights; graph modes capture first, as
    test_graph_replay_matches_eager_step does.  Returns the Trainer after the asserted micro-step 1 and the finished micro-step 2."""
    from cwf.trainer import Trainer
    tr = Trainer(_no_dropout_model(R["forced"]), use_graph=use_graph, accum_steps=2, **kw)
    assert tr.opt.grad_scale == 0.5
    if use_graph:
        tr._fwd_bwd(*R["batches"][0])                                # eager warm-up (allocations, weight-pack tables)
        tr._finish_comm()
        torch.cuda.synchronize()
        assert tr._works == []
        tr._capture(*R["batches"][0])
        assert (tr._plan is not None) == (use_graph == "plan"), tr.plan_info
    tr.step(*R["batches"][0], 0)
    assert tr._works == []
    torch.cuda.synchronize()
    assert torch.equal(_weights(tr), R["w_start"]) and tr.opt._steps == 0          # micro-step 1: nothing updated, nothing counted
    assert all(float(tr.opt.state[p]["step"]) == 0 for p in tr.opt._plist)
    tr.step(*R["batches"][1], 0)
    assert tr._works == []
    torch.cuda.synchronize()
    assert tr.opt._steps == 1 and tr._micro == 0
    return tr


def _check_window(tr, R, w_want):
    g = tr.opt.flat_grad
    assert bool(torch.isfinite(g).all())
    diff = float((g - R["gsum"]).norm() / R["gsum"].norm())
    assert diff < max(5e-5, 10 * R["noise"]), (diff, R["noise"])
    wd = float((_weights(tr) - w_want).norm() / w_want.norm())
    assert wd < 1e-5, wd
    assert float((_weights(tr) - R["w_start"]).abs().max()) > 1e-5                 # and they did move


@pytest.mark.parametrize("use_graph", [False, "plan", "hipgraph"])
def test_trainer_accumulates_two_micro_batches(hip, use_graph):
    """accum_steps = 2 at 64^3, B = 1, samples 0 and 5 (top-k teacher-forced, dropout off): micro-step 1 leaves weights and step
    count alone; after micro-step 2 the flat gradient is g(0) + g(5) (bound of the replay test: max(5e-5, 10 x eager noise)) and the
    weights are those of a plain FusedAdam step on that sum with grad_scale 1/2 (1e-5 relative norm)."""
    from cwf import kernels
    R = _window_reference()
    kernels.set_precision("bf16x3")
    try:
        tr = _window(R, use_graph)
        assert not tr.comm and tr.opt.ema is None and tr.opt.grad_norm is None
        _check_window(tr, R, R["w_half"])
    finally:
        kernels.set_precision("fp32")


def test_trainer_clips_the_window_without_a_host_sync(hip):
    """max_grad_norm at 40 % of the window's norm: grad_norm = 1/2 |g(0) + g(5)| within 10 x noise, the weights those of a plain step
    with the clipped scale, an EMA that moved towards them -- and a second window taken with torch's sync debug mode on 'error':
    no call of the step waits for the device."""
    from cwf import kernels
    R = _window_reference()
    kernels.set_precision("bf16x3")
    try:
        max_norm = 0.4 * R["norm"]
        tr = _window(R, False, max_grad_norm=max_norm, ema_decay=0.9)
        got = float(tr.opt.grad_norm)
        assert abs(got - R["norm"]) <= max(10 * R["noise"], 2.0 ** -22) * R["norm"], (got, R["norm"])
        coef, _ = ref.clip_coef64(float(R["gsum"].double().pow(2).sum()), 0.5, max_norm)
        assert 0.19 < coef < 0.21
        w_want = R["plain_step"](coef)
        _check_window(tr, R, w_want)
        ema_of = dict(zip(map(id, tr.opt._plist), tr.opt.ema))
        ema = torch.cat([ema_of[id(p)].reshape(-1) for p in tr.model.parameters()])
        want_ema = R["w_start"] + 0.1 * (w_want - R["w_start"])
        assert float((ema - want_ema).norm() / want_ema.norm()) < 1e-5
        sd = tr.ema_state_dict()
        assert list(sd.keys()) == list(tr.model.state_dict().keys())
        name, p = next(iter(tr.model.named_parameters()))
        assert torch.equal(sd[name], ema_of[id(p)]) and not torch.equal(sd[name], p)
        tr.opt.reset_ema()                                            # EMA := weights, then back from the checkpoint form of the state
        assert torch.equal(ema_of[id(p)], p)
        tr.load_ema_state_dict({"module." + k: v for k, v in sd.items()})
        assert all(torch.equal(tr.ema_state_dict()[k], v) for k, v in sd.items())
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            tr.step(*R["batches"][0], 0)
            tr.step(*R["batches"][1], 0)
            norm_dev = tr.opt.grad_norm
        finally:
            torch.cuda.set_sync_debug_mode("default")
        torch.cuda.synchronize()
        assert tr.opt._steps == 2 and math.isfinite(float(norm_dev))
    finally:
        kernels.set_precision("fp32")


@pytest.mark.parametrize("use_graph", [False, "plan"])
def test_trainer_window_under_communication_one_rank(hip, monkeypatch, use_graph):
    """The same window in a one-rank RCCL group with CWF_FORCE_COMM=1: the per-slice folds and the real RCCL all-reduces of the
    communication path run (eager: from the backward cut points; plan: at the three captured markers) and leave the gradient and the
    weights of the window without communication, within the same bounds; no work object is left behind by any call.  A one-rank
    all-reduce is the identity, so this cannot tell a fold in front of its collective from one behind it, nor a slice reduced once
    from one reduced twice or never: that order, the tiling and what each collective reads are checked at world size 2 with a
    simulated peer in tests/test_two_rank_step_gpu.py."""
    import torch.distributed as dist
    from cwf import kernels
    R = _window_reference()                                            # (before the group exists: its Trainers are single-process)
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", str(29600 + os.getpid() % 200))
    monkeypatch.setenv("CWF_FORCE_COMM", "1")
    kernels.set_precision("bf16x3")
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device(DEV))
    try:
        tr = _window(R, use_graph)
        assert tr.comm and tr.overlap_comm and tr._comm_stream is not None and len(tr.opt.sink.chunks) == 3
        if use_graph:
            assert tr._plan is not None and tr.plan_info["markers"] == 3, tr.plan_info
            # the plan with its three markers honours every edge of the captured graph and keeps stream 1 to the weight-gradient chain
            # (tests/plan_ref.py; read from the built plan, nothing is launched)
            import plan_ref
            from cwf import _lib
            desc = _lib.plan_describe(hip.lib, tr._plan)
            plan_ref.check_described(desc)
            assert [k for k in desc["marker_id"] if k >= 0] == [0, 1, 2] and desc["stream"].count(-1) == 3
            assert desc["stream"].count(1) == tr.plan_info["on_stream1"] >= 20
        _check_window(tr, R, R["w_half"])
    finally:
        dist.destroy_process_group()
        kernels.set_precision("fp32")


def test_trainer_defaults_allocate_nothing(hip):
    from cwf.trainer import Trainer
    tr = Trainer(_model().train())
    tr.opt._ensure()
    assert tr.accum_steps == 1 and tr.opt.acc is None and tr.opt.ema is None and tr.opt.grad_norm is None
    assert tr.opt._ema_table is None and tr.opt._clip is None and tr.opt.grad_scale == 1.0
