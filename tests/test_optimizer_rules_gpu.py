"""AdamW and SGD rules of the fused step on the GPU (csrc/optim_rules.hip, cwf_optim_step) and their way up through
cwf.optim.FusedAdamW / FusedSGD and cwf.trainer.Trainer.  Yardstick and bound: tests/optimizer_rules_ref.py --

    per tensor, rel_l2(kernel, float64 torch) <= 8 * max(rel_l2(fp32 torch, float64 torch), 2^-24)

for weights, EMA and every state tensor alike."""
import functools

import pytest
import torch

import optimizer_rules_ref as ref
import step_controls_ref as sref
from test_step_controls_gpu import _buf, _no_dropout_model, _sentinels_intact, _weights, _window_reference

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CONTROLS = dict(max_norm=1.0, ema_decay=0.9)          # as the step-control tests use them
EVERY_OTHER = [False, True, False, True, False]


@functools.lru_cache(maxsize=None)
def _inputs():
    return sref.make_inputs()


@functools.lru_cache(maxsize=None)
def _yardstick(case, controls, masked=False):
    """(float64 run, fp32 torch's own relative L2 error against it per compared tensor); computed once per configuration"""
    rule, kw = ref.CASES[case]
    p0, grads = _inputs()
    ctl = dict(CONTROLS) if controls else {}
    mask = EVERY_OTHER if masked else None
    r64 = ref.run_torch(rule, kw, p0, grads, torch.float64, mask=mask, **ctl)
    r32 = ref.run_torch(rule, kw, p0, grads, torch.float32, mask=mask, **ctl)
    return r64, ref.own_errors(r32, r64, ref.compared(rule, kw, controls))


def _fused(case, p0, controls=False, mask=None, **extra):
    from cwf.optim import FusedAdamW, FusedSGD
    rule, kw = ref.CASES[case]
    ps = [torch.nn.Parameter(t.detach().clone().float().to(DEV)) for t in p0]
    if controls:
        extra.update(max_grad_norm=CONTROLS["max_norm"], ema_decay=CONTROLS["ema_decay"])
    if mask is not None:
        extra["no_decay"] = lambda name, p: mask[int(name)]
    return ps, (FusedAdamW if rule == "adamw" else FusedSGD)([(str(i), p) for i, p in enumerate(ps)], **kw, **extra)


def _feed(ps, opt, grads):
    for gs in grads:
        for p, g in zip(ps, gs):
            p.grad = g.to(DEV)
        opt.step()
    torch.cuda.synchronize()


def _got(case, ps, opt, controls):
    rule, kw = ref.CASES[case]
    out = {"w": list(ps)}
    if controls:
        out["ema"] = opt.ema
    for k in ref.state_names(rule, kw):
        out[k] = [opt.state[p][k] for p in ps]
    return out


def _assert_within_bound(got, r64, own, what):
    worst = 0.0
    for k, errs in own.items():
        for i, o in enumerate(errs):
            err = ref.rel_l2(got[k][i], r64[k][i])
            worst = max(worst, err / ref.bound(o))
            print("%s %s[%d]: %.3g (fp32 torch %.3g, bound %.3g)" % (what, k, i, err, o, ref.bound(o)))
            assert err <= ref.bound(o), (what, k, i, err, o)
    print("%s: worst error / bound = %.3f" % (what, worst))


# ------------------------------------------------------------------------------------------------------------------ rules
@pytest.mark.parametrize("controls", [False, True])
@pytest.mark.parametrize("case", sorted(ref.CASES))
def test_rule_against_float64_torch(hip, case, controls):
    """Five tensors of 1 .. 65,537 elements (the odd sizes put every later gradient slice at an unaligned offset of the flat buffer;
    65,537 is more than one sweep of the capped grid), six steps, gradient scale alternating 0.01 / 10, with and without
    max_norm 1 + EMA decay 0.9: weights, EMA and every state tensor within the bound of the module docstring."""
    r64, own = _yardstick(case, controls)
    ps, opt = _fused(case, _inputs()[0], controls)
    _feed(ps, opt, _inputs()[1])
    _assert_within_bound(_got(case, ps, opt, controls), r64, own, "%s%s" % (case, " + clip + EMA" if controls else ""))
    rule, kw = ref.CASES[case]
    assert all(set(opt.state[p].keys()) == set(ref.state_names(rule, kw)) | ({"step"} if rule == "adamw" else set()) for p in ps)


# ------------------------------------------------------------------------------------------------------------------ wd_mul
@pytest.mark.parametrize("case", ["adamw_amsgrad", "sgd_nesterov"])
def test_wd_mul_masks_every_other_tensor(hip, case):
    """tensors 1 and 3 not decayed, against torch with two parameter groups (weight_decay 0 in the second); same bound"""
    r64, own = _yardstick(case, False, True)
    ps, opt = _fused(case, _inputs()[0], mask=EVERY_OTHER)
    _feed(ps, opt, _inputs()[1])
    assert opt._wd_mul.tolist() == [1.0, 0.0, 1.0, 0.0, 1.0]
    _assert_within_bound(_got(case, ps, opt, False), r64, own, case + " masked")
    # and the mask matters on these inputs: the unmasked float64 run is outside the bound for a masked tensor
    plain64, _ = _yardstick(case, False)
    assert ref.rel_l2(ps[3], plain64["w"][3]) > ref.bound(own["w"][3])


@pytest.mark.parametrize("case", ["adamw", "sgd_momentum_damp"])
def test_wd_mul_of_ones_is_bit_equal_to_a_null_mask(hip, case):
    runs = []
    for mask in (None, [False] * 5):
        ps, opt = _fused(case, _inputs()[0], controls=True, mask=mask)
        _feed(ps, opt, _inputs()[1])
        assert (opt._wd_mul is None) == (mask is None) and (mask is None or opt._wd_mul.tolist() == [1.0] * 5)
        runs.append(_got(case, ps, opt, True))
    for k in runs[0]:
        assert all(torch.equal(a, b) for a, b in zip(runs[0][k], runs[1][k])), k


# ------------------------------------------------------------------------------------------------------------------ gscale_dev
@pytest.mark.parametrize("case", ["adamw_amsgrad", "sgd_momentum_damp"])
def test_device_scale_is_bit_equal_to_the_host_scale(hip, case):
    """gscale_dev = {s} (grad_scale then ignored) against grad_scale = s: the same bits in weights and state"""
    s = 0.3
    rule, kw = ref.CASES[case]
    gdev = torch.tensor([s, 123.0], device=DEV)
    runs = []
    for dev_scale in (False, True):
        ps, opt = _fused(case, _inputs()[0])
        opt._ensure()
        for t, gs in enumerate(_inputs()[1], 1):
            for p, g in zip(ps, gs):
                p.grad = g.to(DEV)
            opt.sink.begin(); opt.gather_grads(); opt.advance_host()
            common = dict(grad_scale=77.0, gscale_dev=gdev) if dev_scale else dict(grad_scale=s)
            if rule == "adamw":
                b1, b2 = kw["betas"]
                hip.optim_step("adamw", opt._table, len(ps), opt._max_n, kw["lr"], kw["weight_decay"], beta1=b1, beta2=b2, eps=kw["eps"],
                               step=t, amsgrad=kw["amsgrad"], **common)
            else:
                hip.optim_step("sgd", opt._table, len(ps), opt._max_n, kw["lr"], kw["weight_decay"], momentum=kw["momentum"],
                               dampening=kw["dampening"], nesterov=kw["nesterov"], first=t == 1, **common)
        torch.cuda.synchronize()
        runs.append(_got(case, ps, opt, False))
    for k in runs[0]:
        assert all(torch.equal(a, b) for a, b in zip(runs[0][k], runs[1][k])), k
    r64 = ref.run_torch(rule, kw, *_inputs(), torch.float64, grad_scale=s)          # (and both are the rule, not merely each other)
    assert all(ref.rel_l2(a, b) < 1e-5 for a, b in zip(runs[1]["w"], r64["w"]))


def test_adamw_hyper_dev_replaces_the_host_side_corrections(hip):
    """hyper_dev = {lr / (1 - beta1^t), sqrt(1 - beta2^t)} with step = 0 against the same launches given step = t: the two float32
    values are formed here by Python's pow and there by C's, so the runs are held to 1e-6 relative L2 of each other, not to bits"""
    import math
    rule, kw = ref.CASES["adamw_amsgrad"]
    b1, b2 = kw["betas"]
    runs = []
    for from_device in (False, True):
        ps, opt = _fused("adamw_amsgrad", _inputs()[0])
        opt._ensure()
        for t, gs in enumerate(_inputs()[1][:3], 1):
            for p, g in zip(ps, gs):
                p.grad = g.to(DEV)
            opt.sink.begin(); opt.gather_grads(); opt.advance_host()
            hyper = torch.tensor([kw["lr"] / (1.0 - b1 ** t), math.sqrt(1.0 - b2 ** t)], dtype=torch.float32).to(DEV)
            hip.optim_step("adamw", opt._table, len(ps), opt._max_n, kw["lr"], kw["weight_decay"], beta1=b1, beta2=b2, eps=kw["eps"],
                           amsgrad=True, step=0 if from_device else t, hyper_dev=hyper if from_device else None)
        torch.cuda.synchronize()
        runs.append(_got("adamw_amsgrad", ps, opt, False))
    for k in runs[0]:
        assert all(ref.rel_l2(a, b) <= 1e-6 for a, b in zip(runs[0][k], runs[1][k])), k
    assert not torch.equal(runs[0]["w"][4], _inputs()[0][4].to(DEV))


# ------------------------------------------------------------------------------------------------------------------ memory safety
@pytest.mark.parametrize("rule,kw,cols", [
    ("adamw", dict(beta1=0.9, beta2=0.999, eps=1e-8, step=2, amsgrad=True), 3),
    ("adamw", dict(beta1=0.9, beta2=0.999, eps=1e-8, step=2, amsgrad=False), 2),
    ("sgd", dict(momentum=0.9, dampening=0.1, first=False), 1),
    ("sgd", dict(momentum=0.99, nesterov=True, first=True), 1),
    ("sgd", dict(), 0),
])
@pytest.mark.parametrize("ema", [False, True])
def test_every_tensor_stays_inside_its_bounds(hip, rule, kw, cols, ema):
    """Every parameter, gradient, state and EMA tensor lies inside a larger buffer with a sentinel on either side, gradients at the
    float offsets 1, 2, 3 a slice of the flat buffer can have: the sentinels survive, every parameter moved, and columns the rule
    does not use are null pointers."""
    gen = torch.Generator().manual_seed(7)
    bufs, rows, emas = [], [], []
    for t, n in enumerate(sref.SIZES):
        offs = [t % 4, (t + 1) % 4 or 1] + [(t + 2 + c) % 4 for c in range(cols)]
        made = [_buf(n, off, gen) for off in offs]
        for (base, view), off in zip(made, offs):
            bufs.append((base, off, n))
        made[0][1].add_(3.0)                                        # parameters away from 0: the decay has something to act on
        if cols >= 2:
            made[3][1].abs_()                                       # second moments are not negative
            if cols == 3:
                made[4][1].abs_()
        rows.append([made[0][1].data_ptr(), made[1][1].data_ptr()] + [made[2 + c][1].data_ptr() for c in range(cols)] + [0] * (3 - cols) + [n])
        if ema:
            base, view = _buf(n, (t + 3) % 4, gen)
            bufs.append((base, (t + 3) % 4, n)); emas.append(view)
    before = [torch.cat([b[4 + off:4 + off + n] for b, off, n in bufs]).clone()]
    table = torch.tensor(rows, dtype=torch.int64).to(DEV)
    ema_table = torch.tensor([e.data_ptr() for e in emas], dtype=torch.int64).to(DEV) if ema else None
    wd_mul = torch.tensor([1.0, 0.0, 1.0, 0.0, 1.0], device=DEV)
    hip.optim_step(rule, table, len(rows), max(sref.SIZES), 1e-2, 1e-2, wd_mul=wd_mul, grad_scale=0.5, ema_table=ema_table,
                   ema_weight=0.1 if ema else 0.0, **kw)
    torch.cuda.synchronize()
    assert all(_sentinels_intact(b, off, n) for b, off, n in bufs)
    after = torch.cat([b[4 + off:4 + off + n] for b, off, n in bufs])
    assert bool(torch.isfinite(after).all())
    per = (2 + cols + (1 if ema else 0))
    i = 0
    for t, n in enumerate(sref.SIZES):                               # the parameter moved throughout (an element whose gradient is
        moved = before[0][i:i + n] != after[i:i + n]                 # below 1e-5 may keep its bits), the gradient is untouched
        assert bool(moved.any()) and (n < 300 or float(moved.float().mean()) > 0.99), (t, n)
        assert n < 65537 or float(moved[16384:].float().mean()) > 0.99          # beyond the first sweep of 64 x 256 threads
        assert torch.equal(before[0][i + n:i + 2 * n], after[i + n:i + 2 * n])
        i += per * n


# ------------------------------------------------------------------------------------------------------------------ checkpoints
@pytest.mark.parametrize("case", ["sgd_momentum_damp", "adamw_amsgrad"])
def test_checkpoint_round_trip_with_torch(hip, case):
    """Three fused steps, state_dict() into torch.optim.SGD / AdamW (fp32, CPU), three torch steps -- and the reverse -- end within
    the bound of the uninterrupted float64 run.  SGD has dampening 0.1: were the update after the load taken for a first one
    (buf = g), the buffer would be off by about 10 %."""
    rule, kw = ref.CASES[case]
    p0, grads = _inputs()
    r64, own = _yardstick(case, False)
    ps, opt = _fused(case, p0)
    _feed(ps, opt, grads[:3])
    sd = opt.state_dict()
    want_keys = set(ref.state_names(rule, kw)) | ({"step"} if rule == "adamw" else set())
    assert len(sd["state"]) == len(ps) and all(set(s.keys()) == want_keys for s in sd["state"].values())
    t = ref.run_torch(rule, kw, [p.detach().cpu() for p in ps], grads, torch.float32, opt_state=sd, first_step=3)
    _assert_within_bound(t, r64, own, case + " fused -> torch")
    # the reverse
    t3 = ref.run_torch(rule, kw, p0, grads[:3], torch.float32)
    ps2, opt2 = _fused(case, t3["w"])
    opt2.load_state_dict(t3["opt"].state_dict())
    assert opt2._steps == (3 if rule == "adamw" else 0)               # (torch's SGD state carries no count)
    if rule == "sgd":
        assert not opt2._first
    _feed(ps2, opt2, grads[3:])
    _assert_within_bound(_got(case, ps2, opt2, False), r64, own, case + " torch -> fused")
    if rule == "sgd":                                                 # fused -> fused carries the count as well
        ps3, opt3 = _fused(case, [p.detach() for p in ps])
        opt3.load_state_dict(sd)
        assert opt3._steps == 3 and not opt3._first


# ------------------------------------------------------------------------------------------------------------------ argument checks
def test_optim_step_checks_its_arguments(hip):
    """every documented CWF_E_BADARG case returns -1 and launches nothing (the parameter keeps its bits); the good call moves it"""
    L, s = hip.lib, hip._stream()
    p, g, m, v = (torch.ones(8, device=DEV) for _ in range(4))
    table = torch.tensor([[p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), 0, 8]], dtype=torch.int64).to(DEV)
    ema = torch.ones(8, device=DEV)
    ema_table = torch.tensor([ema.data_ptr()], dtype=torch.int64).to(DEV)
    good = dict(rule=2, table=table.data_ptr(), nt=1, max_n=8, lr=1e-2, wd=0.0, wd_mul=0, b1=0.9, b2=0.999, eps=1e-8, step=1, ams=0,
                hyper=0, mu=0.0, damp=0.0, nest=0, first=0, gs=1.0, gdev=0, ema=0, emaw=0.0)

    def call(**kw):
        a = dict(good, **kw)
        return L.cwf_optim_step(a["rule"], a["table"], a["nt"], a["max_n"], a["lr"], a["wd"], a["wd_mul"], a["b1"], a["b2"], a["eps"],
                                a["step"], a["ams"], a["hyper"], a["mu"], a["damp"], a["nest"], a["first"], a["gs"], a["gdev"], a["ema"],
                                a["emaw"], s)

    nan = float("nan")
    bad = [dict(table=0), dict(nt=0), dict(nt=-1), dict(max_n=0), dict(rule=0), dict(rule=3), dict(rule=1, step=0), dict(rule=1, step=-2),
           dict(lr=nan), dict(lr=-1e-3), dict(mu=nan), dict(mu=-0.5), dict(damp=nan), dict(damp=-0.1), dict(wd=-1.0), dict(wd=nan),
           dict(nest=1), dict(nest=1, mu=0.9, damp=0.1), dict(rule=1, b1=1.0), dict(rule=1, b2=-0.1), dict(rule=1, eps=-1.0)]
    bad += [dict(rule=r, ema=ema_table.data_ptr(), emaw=w) for r in (1, 2) for w in (0.0, -0.1, 0.6, nan)]
    for kw in bad:
        assert call(**kw) == -1, kw
    torch.cuda.synchronize()
    assert bool((p == 1.0).all()) and bool((m == 1.0).all()) and bool((ema == 1.0).all())
    hyper = torch.tensor([1e-2, 1.0], device=DEV)
    assert call(rule=1, step=0, hyper=hyper.data_ptr()) == 0          # step <= 0 is fine WITH hyper_dev
    assert call(nest=1, mu=0.9) == 0 and call(ema=ema_table.data_ptr(), emaw=0.5) == 0
    torch.cuda.synchronize()
    assert bool((p != 1.0).all()) and bool((ema != 1.0).all())
    with pytest.raises(ValueError):
        hip.optim_step("lamb", table, 1, 8, 1e-2, 0.0)
    with pytest.raises(ValueError):
        hip.optim_step("sgd", table, 1, 8, 1e-2, 0.0, wd_mul=torch.ones(2, device=DEV))


# ------------------------------------------------------------------------------------------------------------------ Trainer, 64^3
def _replay_optimizer(R, kind, kw):
    """the same rule on a second copy of the start weights, outside any Trainer: fed the flat gradient a Trainer step used"""
    from cwf.optim import FusedAdamW, FusedSGD
    m = _no_dropout_model(R["forced"])
    opt = (FusedAdamW if kind == "adamw" else FusedSGD)(m.named_parameters(), phases=m.grad_phases(), **kw)
    opt._ensure()
    return m, opt


def _replay(opt, tr):
    opt.flat_grad.copy_(tr.opt.flat_grad)
    opt.param_groups[0]["lr"] = tr.opt.param_groups[0]["lr"]
    opt.grad_scale = tr.opt.grad_scale
    opt.advance_host(); opt.launch()


TRAINER_RULES = {
    "adamw": (dict(optimizer="adamw", no_decay="bias_norm", weight_decay=1e-2), dict(lr=2e-4, weight_decay=1e-2, amsgrad=True, no_decay="bias_norm")),
    "sgd": (dict(optimizer="sgd", momentum=0.99, nesterov=True, lr=1e-2, weight_decay=3e-5),
            dict(lr=1e-2, momentum=0.99, nesterov=True, weight_decay=3e-5)),
}


@functools.lru_cache(maxsize=None)
def _three_steps(kind, use_graph):
    """Three Trainer steps of rule `kind` (64^3, B = 1, samples 0, 5, 0, dropout off, top-k teacher-forced, warmup_steps=3), eager or
    from the captured plan; beside them the same rule outside any Trainer, fed the flat gradient each step used.  Run once per
    (rule, mode) and shared by the tests below."""
    from cwf import kernels
    from cwf.trainer import Trainer
    R = _window_reference()
    tkw, okw = TRAINER_RULES[kind]
    kernels.set_precision("bf16x3")
    try:
        tr = Trainer(_no_dropout_model(R["forced"]), use_graph=use_graph, warmup_steps=3, **tkw)
        if use_graph:
            tr._fwd_bwd(*R["batches"][0])                             # eager warm-up, then the capture, as _window does it
            tr._finish_comm()
            torch.cuda.synchronize()
            tr._capture(*R["batches"][0])
        m2, opt2 = _replay_optimizer(R, kind, okw)
        same_start = torch.equal(_weights(tr), torch.cat([p.detach().reshape(-1) for p in m2.parameters()]))
        lrs = []
        for i in range(3):
            tr.step(*R["batches"][i % 2], 0)
            torch.cuda.synchronize()
            lrs.append(tr.opt.param_groups[0]["lr"])
            _replay(opt2, tr)
        torch.cuda.synchronize()
        return dict(w=_weights(tr).clone(), w_replay=torch.cat([p.detach().reshape(-1) for p in m2.parameters()]), lrs=lrs,
                    same_start=same_start, planned=tr._plan is not None, graphed=tr._graph is not None, plan_info=tr.plan_info,
                    cls=type(tr.opt).__name__,
                    optimizer=tr.optimizer, updates=(tr.updates_done, tr.opt._steps),
                    wd_mul=None if tr.opt._wd_mul is None else tr.opt._wd_mul.tolist(), ndims=[p.ndim for p in tr.opt._plist])
    finally:
        kernels.set_precision("fp32")


@pytest.mark.parametrize("use_graph", [False, "plan", "hipgraph"])
@pytest.mark.parametrize("kind", ["adamw", "sgd"])
def test_trainer_steps_with_each_rule(hip, kind, use_graph):
    """Trainer(optimizer="adamw", no_decay="bias_norm") and Trainer(optimizer="sgd", momentum=0.99, nesterov=True) in every step mode:
    after three steps the weights are bit-equal to the rule applied, outside any Trainer, to the three flat gradients those steps used -- the launch
    follows the replay and nothing of it is captured -- with the learning rates poly_lr(0) x 1/3, 2/3, 1 of warmup_steps=3, and the
    mask has a 0 for every parameter with at most one dimension."""
    from cwf.optim import poly_lr
    r = _three_steps(kind, use_graph)
    tkw, _ = TRAINER_RULES[kind]
    assert r["optimizer"] == kind and r["cls"] == {"adamw": "FusedAdamW", "sgd": "FusedSGD"}[kind] and r["same_start"]
    assert r["planned"] == (use_graph == "plan") and r["graphed"] == bool(use_graph), r["plan_info"]
    base = float(poly_lr(tkw.get("lr", 2e-4), 0, 1000))
    assert r["lrs"] == [base * (1 / 3), base * (2 / 3), base] and all(type(x) is float for x in r["lrs"])
    assert r["updates"] == (3, 3)
    w = r["w"]
    assert bool(torch.isfinite(w).all()) and float((w - _window_reference()["w_start"]).abs().max()) > 1e-5
    assert torch.equal(w, r["w_replay"]), float((w - r["w_replay"]).abs().max())
    if "no_decay" in tkw:
        want_mask = [0.0 if d <= 1 else 1.0 for d in r["ndims"]]
        assert r["wd_mul"] == want_mask and 0.0 in want_mask and 1.0 in want_mask
    else:
        assert r["wd_mul"] is None


@pytest.mark.parametrize("kind", ["adamw", "sgd"])
def test_trainer_eager_and_plan_reach_bit_equal_weights(hip, kind):
    """the three eager steps and the three steps from the captured plan end in the same bits (printed before the assertion: the
    largest difference and the number of elements that differ)"""
    e, p = _three_steps(kind, False)["w"], _three_steps(kind, "plan")["w"]
    print("%s eager vs plan: max |d| %.3g, %d of %d elements differ" % (kind, float((e - p).abs().max()), int((e != p).sum()), e.numel()))
    assert torch.equal(e, p)


def test_trainer_accumulates_two_micro_batches_with_sgd(hip):
    """accum_steps = 2 with optimizer="sgd": micro-step 1 updates and counts nothing; after micro-step 2 the flat gradient is
    g(0) + g(5) (bound of the Adam window test) and the weights are bit-equal to one SGD update on that buffer at grad_scale 1/2."""
    from cwf import kernels
    from cwf.trainer import Trainer
    R = _window_reference()
    tkw, okw = TRAINER_RULES["sgd"]
    kernels.set_precision("bf16x3")
    try:
        tr = Trainer(_no_dropout_model(R["forced"]), accum_steps=2, **tkw)
        assert tr.opt.grad_scale == 0.5
        tr.step(*R["batches"][0], 0)
        torch.cuda.synchronize()
        assert torch.equal(_weights(tr), R["w_start"]) and tr.opt._steps == 0 and tr.opt._first
        tr.step(*R["batches"][1], 0)
        torch.cuda.synchronize()
        assert tr.opt._steps == 1 and tr._micro == 0 and not tr.opt._first
        diff = float((tr.opt.flat_grad - R["gsum"]).norm() / R["gsum"].norm())
        assert diff < max(5e-5, 10 * R["noise"]), (diff, R["noise"])
        m2, opt2 = _replay_optimizer(R, "sgd", okw)
        _replay(opt2, tr)
        torch.cuda.synchronize()
        w = _weights(tr)
        assert torch.equal(w, torch.cat([p.detach().reshape(-1) for p in m2.parameters()]))
        assert float((w - R["w_start"]).abs().max()) > 1e-5
    finally:
        kernels.set_precision("fp32")


# ------------------------------------------------------------------------------------------------------------------ defaults
def test_defaults_make_the_call_they_always_made(hip, monkeypatch):
    """A default FusedAdam step and a default Trainer step: one cwf_adam_amsgrad_scaled call with the arguments of the plain launch,
    no cwf_optim_step, no cwf_adam_amsgrad_ex, no wd_mul."""
    from cwf.optim import FusedAdam, poly_lr
    from cwf.trainer import Trainer
    calls = []
    real = hip._call
    monkeypatch.setattr(hip, "_call", lambda name, *a: (calls.append((name,) + a), real(name, *a))[1])
    ps = [torch.nn.Parameter(torch.randn(n, device=DEV)) for n in (5, 12, 3)]
    opt = FusedAdam(ps, lr=2e-4, weight_decay=1e-5, amsgrad=True)
    for p in ps:
        p.grad = torch.ones_like(p)
    opt.step()
    assert [c[0] for c in calls] == ["cwf_adam_amsgrad_scaled"]
    assert calls[0][1:] == (opt._table.data_ptr(), 3, 12, 2e-4, 0.9, 0.999, 1e-8, 1e-5, 1, 1, 0, 1.0, hip._stream())
    assert opt._wd_mul is None and opt._no_decay is None
    R = _window_reference()
    tr = Trainer(_no_dropout_model(R["forced"]))
    calls.clear()
    tr.step(*R["batches"][0], 37)
    torch.cuda.synchronize()
    names = [c[0] for c in calls]
    assert names.count("cwf_adam_amsgrad_scaled") == 1 and names[-1] == "cwf_adam_amsgrad_scaled"
    assert "cwf_optim_step" not in names and "cwf_adam_amsgrad_ex" not in names and "cwf_grad_norm_clip" not in names
    last = calls[-1]
    assert last[1:4] == (tr.opt._table.data_ptr(), len(tr.opt._plist), tr.opt._max_n)
    assert last[4:] == (float(poly_lr(2e-4, 37, 1000)), 0.9, 0.999, 1e-8, 1e-5, 1, 1, 0, 1.0, hip._stream())
    assert tr.opt._wd_mul is None and tr.opt.acc is None and tr.opt.ema is None and tr.opt._clip is None
    assert tr.optimizer == "adam" and tr.schedule == "poly" and tr.warmup_steps == 0
