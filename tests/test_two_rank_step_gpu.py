"""Data-parallel semantics of Trainer.step at world size 2 on the GPU, with the second rank simulated inside the process
(tests/two_rank_ref.py): no process group, no collective, no second process.

A one-rank group makes all_reduce the identity, and then a fold issued after its collective, a phase slice reduced twice or never, a
collective that reads its slice before the slab reduce has landed and a grad_scale without the world size all pass.  Here every case
makes a RECORD pass as rank 1 on rank 1's samples and a REPLAY pass as rank 0 on rank 0's samples, in which each all-reduce adds what
rank 1 contributed at the same program point; the replay's first weight update is the object under test.  The yardsticks are the
solo flat gradients g(s) of the four samples (plain _fwd_bwd runs on the start weights, no communication) and the fused update rule
applied outside any Trainer to their sum.  Setup (64^3, B = 1, dropout off, top-k teacher-forced, bf16x3) and bounds are those of the
window tests in tests/test_step_controls_gpu.py; the noise term is measured here, from solo runs."""
import functools

import pytest
import torch

import step_controls_ref as ref
from test_step_controls_gpu import DEV, _no_dropout_model, _weights, _window_reference
from two_rank_ref import SimulatedPeer, tiling_error
from utils import synthetic as syn

pytestmark = pytest.mark.gpu

SAMPLES = ((0, 5), (3, 7))               # rank -> its samples, in micro-step order; accum_steps = 1 takes the first of each
LR, WD = 2e-4, 1e-5                      # the Trainer's defaults
RULES = {"adam": {}, "adamw": dict(optimizer="adamw", no_decay="bias_norm"), "sgd": dict(optimizer="sgd", momentum=0.99, nesterov=True)}


@functools.lru_cache(maxsize=None)
def _reference():
    """Once per module, outside the harness: g(s) for the four samples from two repetitions of solo _fwd_bwd runs on the start weights
    (their difference is the eager-against-eager noise, measured as _window_reference measures it)."""
    from cwf import kernels
    from cwf.trainer import Trainer
    R = _window_reference()              # the teacher-forced indices, samples 0 and 5 on the device, the start weights
    kernels.set_precision("bf16x3")
    try:
        batches = {0: R["batches"][0], 5: R["batches"][1]}
        for s in (3, 7):
            batches[s] = tuple(t.to(DEV) for t in syn.synthetic_batch([s], (64, 64, 64)))
        order = [s for r in SAMPLES for s in r]
        runs = []
        for rep in range(2):
            tr = Trainer(_no_dropout_model(R["forced"]))
            assert not tr.comm and tr.world == 1
            per = {}
            for s in order:
                tr._fwd_bwd(*batches[s])
                torch.cuda.synchronize()
                per[s] = tr.opt.flat_grad.clone()
            runs.append(per)
        assert torch.equal(_weights(tr), R["w_start"])
        noise = max(float((runs[0][s] - runs[1][s]).norm() / runs[0][s].norm()) for s in order)
        return dict(forced=R["forced"], batches=batches, g=runs[0], noise=noise, w_start=R["w_start"], bound=max(5e-5, 10 * noise), want={})
    finally:
        kernels.set_precision("fp32")


def _local_sum(R, rank, accum):
    """what rank `rank` hands to the collectives: g(last) + g(first), the order accumulate / fold add in"""
    s = SAMPLES[rank][:accum]
    return R["g"][s[-1]] + R["g"][s[0]] if accum == 2 else R["g"][s[0]]


def _plain_step(R, rule, gsum, scale):
    """the weights the fused rule leaves when applied, outside any Trainer, to `gsum` with grad_scale `scale` on the start weights"""
    from cwf.optim import FusedAdam, FusedAdamW, FusedSGD
    m = _no_dropout_model(R["forced"])
    if rule == "adam":
        opt = FusedAdam(m.parameters(), lr=LR, weight_decay=WD, amsgrad=True, phases=m.grad_phases())
    elif rule == "adamw":
        opt = FusedAdamW(m.named_parameters(), lr=LR, weight_decay=WD, amsgrad=True, no_decay="bias_norm", phases=m.grad_phases())
    else:
        opt = FusedSGD(m.named_parameters(), lr=LR, momentum=0.99, weight_decay=WD, nesterov=True, phases=m.grad_phases())
    opt._ensure()
    opt.flat_grad.copy_(gsum)
    opt.grad_scale = scale
    opt.advance_host(); opt.launch()
    torch.cuda.synchronize()
    return torch.cat([p.detach().reshape(-1) for p in m.parameters()])


def _one_pass(R, rank, peer, use_graph, accum, kw):
    """One rank's run up to and including its first weight update; graph modes warm up and capture first, as _window does.
    Returns (Trainer, harness)."""
    from cwf.trainer import Trainer
    mine = [R["batches"][s] for s in SAMPLES[rank][:accum]]
    with SimulatedPeer(rank, peer) as sim:
        tr = sim.attach(Trainer(_no_dropout_model(R["forced"]), use_graph=use_graph, accum_steps=accum, **kw))
        assert tr.world == 2 and tr.comm and tr.opt.grad_scale == 1.0 / (2 * accum) and sim.broadcasts > 0
        assert tr.overlap_comm == (use_graph != "hipgraph") and (tr._comm_stream is not None) == tr.overlap_comm
        if use_graph:
            sim.update = "warmup"
            tr._fwd_bwd(*mine[0])                                        # eager warm-up (allocations, weight-pack tables)
            tr._finish_comm()
            torch.cuda.synchronize()
            assert tr._works == []
            tr._capture(*mine[0])
            assert (tr._plan is not None) == (use_graph == "plan"), tr.plan_info
        sim.update = 0
        if accum == 2:
            tr.step(*mine[0], 0)
            torch.cuda.synchronize()
            assert sim.calls(0) == [] and tr._works == []                # no collective inside a window
            assert torch.equal(_weights(tr), R["w_start"]) and tr.opt._steps == 0
            assert all(float(st["step"]) == 0 for st in (tr.opt.state[p] for p in tr.opt._plist) if "step" in st)
        tr.step(*mine[-1], 0)
        torch.cuda.synchronize()
        assert tr._works == [] and tr.opt._steps == 1 and tr._micro == 0
    return tr, sim


def _check_collectives(R, tr, sim, rank, use_graph, accum, worst):
    """tiling, stream and what each collective read, for the calls of update 0"""
    calls = sim.calls(0)
    n = tr.opt.flat_grad.numel()
    got = [(e["lo"], e["hi"]) for e in calls]
    assert tiling_error(got, n) is None, (tiling_error(got, n), got)
    if use_graph == "hipgraph":
        size = -(-n // 4)
        assert got == [(i * size, min(n, (i + 1) * size)) for i in range(4)], got
        assert tr._comm_stream is None and all(e["stream"] == torch.cuda.current_stream() for e in calls)
    else:
        assert len(tr.opt.sink.chunks) == 3 and got == [tuple(c) for c in tr.opt.sink.chunks], (got, tr.opt.sink.chunks)
        assert all(e["stream"] == tr._comm_stream for e in calls) and tr._comm_stream != torch.cuda.current_stream()
    assert all(e["async_op"] and e["work"].waited for e in calls)        # every work object was waited for before the update
    local = _local_sum(R, rank, accum)
    for e in calls:
        want = local[e["lo"]:e["hi"]]
        err = float((e["snapshot"] - want).norm() / want.norm())
        worst["snapshot"] = max(worst.get("snapshot", 0.0), err / R["bound"])
        assert err < R["bound"], ("rank %d: the collective over [%d, %d) read a slice %g away from the local sum" % (rank, e["lo"], e["hi"], err),
                                  R["noise"])


CASES = [(False, 1, "adam", False), (False, 2, "adam", False), ("plan", 1, "adam", False), ("plan", 2, "adam", False),
         ("hipgraph", 1, "adam", False), ("hipgraph", 2, "adam", False), (False, 2, "adam", True), ("plan", 2, "adam", True),
         ("plan", 2, "adamw", False), (False, 1, "sgd", False)]


@pytest.mark.parametrize("use_graph,accum,rule,controls", CASES,
                         ids=["%s-accum%d-%s%s" % (g or "eager", a, r, "-clip-ema" if c else "") for g, a, r, c in CASES])
def test_first_update_at_world_size_two(hip, use_graph, accum, rule, controls):
    """Record as rank 1, replay as rank 0.  In both passes the all-reduces of the update tile the flat buffer exactly once (the three
    phase slices on the communication stream; under hipGraph replay the four chunk(4) pieces on the main stream), every one reads
    the local sum of its slice (relative norm max(5e-5, 10 x noise)), none is issued inside an accumulation window, every work
    object is waited for.  After the replay's update the flat gradient is the sum over ranks and micro-steps (same bound), the
    weights are those of the plain fused rule on that sum with grad_scale 1 / (2 accum_steps) -- times the float64 clip coefficient
    where clipping is on -- to 1e-5 relative norm, and with clipping the device norm is 1 / (2 accum_steps) |sum g| within
    max(10 x noise, 2^-22) and the EMA is w_start + 0.1 (w_want - w_start) to 1e-5.
    Measured on the MI355X over the ten cases ("Step semantics at world size 2"): noise 0, snapshots, gradient and
    weights bit-equal to their yardsticks, grad_norm 5e-9 relative, EMA 2e-8; run with -s for the figures of a run."""
    from cwf import kernels
    R = _reference()
    kernels.set_precision("bf16x3")
    try:
        scale = 1.0 / (2 * accum)
        total = _local_sum(R, 0, accum) + _local_sum(R, 1, accum)
        sq = float(total.double().pow(2).sum())
        norm = scale * sq ** 0.5                                          # norm of the averaged gradient
        kw = dict(RULES[rule])
        if controls:
            kw.update(max_grad_norm=0.4 * norm, ema_decay=0.9)
        worst = {}
        tr1, rec = _one_pass(R, 1, None, use_graph, accum, kw)
        _check_collectives(R, tr1, rec, 1, use_graph, accum, worst)
        tr, rep = _one_pass(R, 0, rec.contributions(), use_graph, accum, kw)
        _check_collectives(R, tr, rep, 0, use_graph, accum, worst)
        assert [(e["lo"], e["hi"]) for e in rep.calls(0)] == [(e["lo"], e["hi"]) for e in rec.calls(0)]
        if use_graph == "plan":
            import plan_ref
            from cwf import _lib
            assert tr.plan_info["markers"] == 3, tr.plan_info
            plan_ref.check_described(_lib.plan_describe(hip.lib, tr._plan))
        # the reduced gradient
        g = tr.opt.flat_grad
        assert bool(torch.isfinite(g).all())
        err = float((g - total).norm() / total.norm())
        worst["gradient"] = err / R["bound"]
        assert err < R["bound"], (err, R["noise"])
        # the update
        coef = scale
        if controls:
            coef, _ = ref.clip_coef64(sq, scale, 0.4 * norm)
            assert 0.39 * scale < coef < 0.41 * scale
        key = (rule, accum, controls)
        if key not in R["want"]:
            R["want"][key] = _plain_step(R, rule, total, coef)
        w_want = R["want"][key]
        w = _weights(tr)
        wd = float((w - w_want).norm() / w_want.norm())
        worst["weights"] = wd / 1e-5
        assert wd < 1e-5, wd
        moved = float((w - R["w_start"]).abs().max())
        assert moved > 1e-5, moved
        if controls:
            got = float(tr.opt.grad_norm)
            nb = max(10 * R["noise"], 2.0 ** -22)
            worst["grad_norm"] = abs(got - norm) / (nb * norm)
            assert abs(got - norm) <= nb * norm, (got, norm)
            ema_of = dict(zip(map(id, tr.opt._plist), tr.opt.ema))
            ema = torch.cat([ema_of[id(p)].reshape(-1) for p in tr.model.parameters()])
            want_ema = R["w_start"] + 0.1 * (w_want - R["w_start"])
            ed = float((ema - want_ema).norm() / want_ema.norm())
            worst["ema"] = ed / 1e-5
            assert ed < 1e-5, ed
        else:
            assert tr.opt.ema is None and tr.opt.grad_norm is None
        print("\n%s accum %d %s%s: noise %.3g, moved %.3g, observed / bound: %s"
              % (use_graph or "eager", accum, rule, " clip+ema" if controls else "", R["noise"], moved,
                 ", ".join("%s %.3g" % kv for kv in sorted(worst.items()))))
    finally:
        kernels.set_precision("fp32")


def test_harness_refuses_what_it_does_not_model(hip):
    """A collective other than all_reduce(SUM) / broadcast, an all_reduce outside the flat buffer and a slice the peer never
    contributed all raise; torch.distributed is restored on exit."""
    import torch.distributed as dist
    from two_rank_ref import Unmodelled
    before = (dist.all_reduce, dist.is_initialized, dist.barrier)

    class _Opt:
        flat_grad = torch.zeros(16, device=DEV)

    class _Tr:
        opt = _Opt()

    with SimulatedPeer(0, peer={}) as sim:
        assert dist.is_initialized() and dist.get_world_size() == 2 and dist.get_rank() == 0
        sim.attach(_Tr())
        for call in (lambda: dist.barrier(), lambda: dist.all_gather([], _Opt.flat_grad), lambda: dist.reduce(_Opt.flat_grad, 0),
                     lambda: dist.all_reduce(_Opt.flat_grad, op=dist.ReduceOp.MAX), lambda: dist.all_reduce(torch.zeros(4, device=DEV)),
                     lambda: dist.all_reduce(_Opt.flat_grad[::2]), lambda: dist.all_reduce(_Opt.flat_grad[4:8])):
            with pytest.raises(Unmodelled):
                call()
        assert sim.log == []
    assert (dist.all_reduce, dist.is_initialized, dist.barrier) == before
    with SimulatedPeer(1) as sim:
        sim.attach(_Tr())
        sim.update = 0
        _Opt.flat_grad.fill_(2.0)
        w = dist.all_reduce(_Opt.flat_grad[4:8], async_op=True)
        _Opt.flat_grad.fill_(3.0)                                        # after the call: not part of the contribution
        w.wait()
        torch.cuda.synchronize()
        assert [(e["lo"], e["hi"]) for e in sim.calls(0)] == [(4, 8)] and bool((sim.contributions()[(0, 4, 8)] == 2.0).all())
    with SimulatedPeer(0, peer=sim.contributions()) as rep:
        rep.attach(_Tr())
        rep.update = 0
        dist.all_reduce(_Opt.flat_grad[4:8])
        torch.cuda.synchronize()
        assert _Opt.flat_grad.tolist() == [3.0] * 4 + [5.0] * 4 + [3.0] * 8
