"""AdamW and SGD rules of the fused step -- everything that needs no GPU: the yardstick (tests/optimizer_rules_ref.py) against a
hand-written numpy statement of both rules, the no-decay mask, the schedule and warm-up arithmetic, the constructors' checks, and the
host logic of cwf.optim.FusedAdamW / FusedSGD (first-update flag, checkpoint layout) through a torch-op emulation of the launch."""
import ctypes
import math

import numpy as np
import pytest
import torch

import optimizer_rules_ref as ref
import step_controls_ref as sref
from test_step_controls_cpu import StepEmul


class RulesEmul(StepEmul):
    """StepEmul plus HipBackend.optim_step in fp32 torch ops on host memory, statement by statement as csrc/optim_rules.hip."""

    def optim_step(self, rule, table, ntensors, max_n, lr, wd, wd_mul=None, beta1=0.9, beta2=0.999, eps=1e-8, step=0, amsgrad=False,
                   hyper_dev=None, momentum=0.0, dampening=0.0, nesterov=False, first=False, grad_scale=1.0, gscale_dev=None,
                   ema_table=None, ema_weight=0.0):
        self.calls.append(("optim_step", rule, lr, step, grad_scale, wd_mul is not None, bool(first)))
        view = lambda ptr, n: torch.from_numpy(np.ctypeslib.as_array((ctypes.c_float * n).from_address(int(ptr))))
        scale = float(gscale_dev[0]) if gscale_dev is not None else grad_scale
        for t, (pp, gp, mp, vp, xp, n) in enumerate(table.tolist()[:ntensors]):
            mul = float(wd_mul[t]) if wd_mul is not None else 1.0
            p, g = view(pp, n), view(gp, n) * scale
            if rule == "adamw":
                assert step > 0
                m, v = view(mp, n), view(vp, n)
                p.mul_(1.0 - lr * wd * mul)
                m.lerp_(g, 1.0 - beta1)
                v.mul_(beta2).addcmul_(g, g, value=1.0 - beta2)
                vv = v
                if amsgrad:
                    vv = view(xp, n)
                    torch.maximum(vv, v, out=vv)
                p.addcdiv_(m, vv.sqrt() / math.sqrt(1.0 - beta2 ** step) + eps, value=-lr / (1.0 - beta1 ** step))
            else:
                assert rule == "sgd" and vp == 0 and xp == 0
                g = g.add(p, alpha=wd * mul)
                if momentum > 0:
                    b = view(mp, n)
                    if first:
                        b.copy_(g)
                    else:
                        b.mul_(momentum).add_(g, alpha=1.0 - dampening)
                    g = g.add(b, alpha=momentum) if nesterov else b
                else:
                    assert mp == 0
                p.add_(g, alpha=-lr)
            if ema_table is not None:
                view(ema_table.tolist()[t], n).lerp_(p, ema_weight)


@pytest.fixture()
def rules_emul():
    from cwf import kernels
    old = kernels._backend
    K = RulesEmul()
    kernels._set_backend_for_testing(K)
    yield K
    kernels._set_backend_for_testing(old)


SMALL = dict(sizes=(1, 7, 300), steps=4)
MASK = [False, True, False]


# ------------------------------------------------------------------------------------------------------------------ the yardstick
@pytest.mark.parametrize("case", sorted(ref.CASES))
@pytest.mark.parametrize("controls", [False, True])
def test_yardstick_float64_equals_the_numpy_statement(case, controls):
    """torch.optim.AdamW / SGD in float64 against the rules written out in numpy (SGD's first update sets buf = g, dampening not
    applied; sgd_momentum_damp has dampening 0.1, so the two readings differ): 1e-12 relative L2 on weights, EMA and every state
    tensor, with and without clip + EMA, with and without a no-decay mask."""
    rule, kw = ref.CASES[case]
    p0, grads = sref.make_inputs(**SMALL)
    ctl = dict(max_norm=1.0, ema_decay=0.9) if controls else {}
    for mask in (None, MASK):
        r64 = ref.run_torch(rule, kw, p0, grads, torch.float64, mask=mask, **ctl)
        rnp = ref.run_numpy(rule, kw, p0, grads, mask=mask, **ctl)
        for k in ref.compared(rule, kw, controls):
            for i in range(len(p0)):
                assert ref.rel_l2(torch.from_numpy(rnp[k][i]), r64[k][i]) <= 1e-12, (k, i, mask)
    if case == "sgd_momentum_damp":           # and the other reading of the first update is visibly different
        wrong = dict(kw, dampening=0.0)
        assert ref.rel_l2(torch.from_numpy(ref.run_numpy(rule, wrong, p0, grads[:1])["momentum_buffer"][2]),
                          ref.run_torch(rule, kw, p0, grads[:1], torch.float64)["momentum_buffer"][2]) <= 1e-12
        two = ref.run_torch(rule, kw, p0, grads[:2], torch.float64)["momentum_buffer"][2]
        assert ref.rel_l2(torch.from_numpy(ref.run_numpy(rule, wrong, p0, grads[:2])["momentum_buffer"][2]), two) > 1e-3


def test_yardstick_fp32_torch_against_float64_on_the_gpu_inputs():
    """The right-hand side of the GPU bound on the GPU tests' inputs: fp32 torch is within 1e-6 relative L2 of its float64 run on
    every compared tensor of every case, so the bound is never looser than 8e-6, and never tighter than 8 x 2^-24."""
    p0, grads = sref.make_inputs()
    for case, (rule, kw) in sorted(ref.CASES.items()):
        for ctl in ({}, dict(max_norm=1.0, ema_decay=0.9)):
            r64, r32 = (ref.run_torch(rule, kw, p0, grads, dt, **ctl) for dt in (torch.float64, torch.float32))
            for k, own in ref.own_errors(r32, r64, ref.compared(rule, kw, bool(ctl))).items():
                print(case, bool(ctl), k, ["%.2g" % e for e in own])
                assert all(e < 1e-6 for e in own) and all(8 * ref.FLOOR <= ref.bound(e) < 8e-6 for e in own), (case, k, own)


# ------------------------------------------------------------------------------------------------------------------ the mask
class Toy(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.conv = torch.nn.Conv1d(2, 3, 3)
        self.norm = torch.nn.LayerNorm(3)
        self.token = torch.nn.Parameter(torch.zeros(1, 1, 3))
        self.head = torch.nn.Linear(3, 2, bias=False)


def test_no_decay_mask_from_bias_norm_and_from_a_callable(rules_emul):
    from cwf.optim import FusedAdam, FusedAdamW, FusedSGD, no_decay_mask
    m = Toy()
    names = [n for n, _ in m.named_parameters()]
    assert names == ["token", "conv.weight", "conv.bias", "norm.weight", "norm.bias", "head.weight"]
    assert no_decay_mask("bias_norm", m.parameters()) == [False, False, True, True, True, False]
    assert no_decay_mask(None, m.parameters()) == [False] * 6
    by_name = lambda n, p: n == "token" or n.endswith(".bias")
    assert no_decay_mask(by_name, m.parameters(), names) == [True, False, True, False, True, False]
    with pytest.raises(ValueError, match="names"):
        no_decay_mask(by_name, m.parameters())
    with pytest.raises(ValueError):
        no_decay_mask("biases", m.parameters())
    # built into wd_mul alongside the descriptor table, in the table's order, frozen parameters left out
    m.conv.bias.requires_grad_(False)
    for cls in (FusedAdamW, FusedSGD):
        opt = cls(m.named_parameters(), lr=0.1, weight_decay=0.1, no_decay=by_name)
        assert opt._wd_mul is None
        opt._ensure()
        assert opt._wd_mul.dtype == torch.float32 and opt._wd_mul.tolist() == [0.0, 1.0, 1.0, 0.0, 1.0]
        assert "no_decay" not in opt.state_dict()["param_groups"][0]
        opt = cls(m.parameters(), lr=0.1, weight_decay=0.1, no_decay="bias_norm")
        opt._ensure()
        assert opt._wd_mul.tolist() == [1.0, 1.0, 0.0, 0.0, 1.0]
        opt = cls(m.parameters(), lr=0.1)
        opt._ensure()
        assert opt._wd_mul is None
    assert FusedAdam(m.parameters(), no_decay=None)._no_decay is None
    for nd in ("bias_norm", by_name):
        with pytest.raises(ValueError, match="no_decay"):
            FusedAdam(m.named_parameters(), no_decay=nd)


def test_masked_tensors_are_not_decayed(rules_emul):
    """zero gradients, plain SGD: a decayed tensor shrinks by (1 - lr wd), a masked one stays bit-equal"""
    from cwf.optim import FusedSGD
    ps = [torch.nn.Parameter(torch.ones(4)), torch.nn.Parameter(torch.ones(3))]
    opt = FusedSGD([("w", ps[0]), ("b", ps[1])], lr=0.5, weight_decay=0.5, no_decay=lambda name, p: name == "b")
    for p in ps:
        p.grad = torch.zeros_like(p)
    opt.step()
    assert torch.equal(ps[0].detach(), torch.full((4,), 0.75)) and torch.equal(ps[1].detach(), torch.ones(3))
    assert rules_emul.calls[-1][:2] == ("optim_step", "sgd") and rules_emul.calls[-1][5] is True


# ------------------------------------------------------------------------------------------------------------------ schedule, warm-up
def test_schedule_and_warmup_arithmetic_including_a_resumed_count(rules_emul):
    from cwf.optim import cosine_lr, poly_lr, schedule_lr, warmup_factor
    from cwf.trainer import Trainer
    assert cosine_lr(2e-4, 0, 1000) == 2e-4 and cosine_lr(2e-4, 1000, 1000) == 0.0
    assert cosine_lr(2e-4, 250, 1000) == round(2e-4 * 0.5 * (1 + math.cos(math.pi / 4)), 8)
    assert cosine_lr(0.123456789, 500, 1000) == 0.06172839           # rounded to 8 places, as poly_lr rounds
    assert schedule_lr("poly", 2e-4, 37, 1000) == float(poly_lr(2e-4, 37, 1000)) and schedule_lr("constant", 2e-4, 37, 1000) == 2e-4
    with pytest.raises(ValueError):
        schedule_lr("linear", 2e-4, 0, 10)
    assert [warmup_factor(u, 3) for u in range(5)] == [1 / 3, 2 / 3, 1.0, 1.0, 1.0] and warmup_factor(0, 0) == 1.0

    def grads(tr):
        for p in tr.model.parameters():
            p.grad = torch.ones_like(p)

    tr = Trainer(torch.nn.Linear(3, 2))                                # defaults: exactly the poly rate, a plain float
    assert tr.optimizer == "adam" and tr.learning_rate(37) == float(poly_lr(2e-4, 37, 1000)) and type(tr.learning_rate(37)) is float
    tr = Trainer(torch.nn.Linear(3, 2), lr=0.1, end_epoch=10, optimizer="sgd", momentum=0.9, schedule="cosine", warmup_steps=4)
    assert tr.updates_done == 0 and tr.learning_rate(0) == pytest.approx(0.1 / 4, rel=1e-15)
    for _ in range(2):
        grads(tr); tr.opt.step()
    assert tr.updates_done == 2 and tr.learning_rate(5) == pytest.approx(cosine_lr(0.1, 5, 10) * 3 / 4, rel=1e-15)
    sd = tr.opt.state_dict()
    assert isinstance(sd["param_groups"][0]["lr"], float) and sd["param_groups"][0]["updates"] == 2
    tr2 = Trainer(torch.nn.Linear(3, 2), lr=0.1, end_epoch=10, optimizer="sgd", momentum=0.9, schedule="cosine", warmup_steps=4)
    tr2.opt.load_state_dict(sd)
    assert tr2.updates_done == 2 and tr2.learning_rate(5) == tr.learning_rate(5)
    for _ in range(2):
        grads(tr2); tr2.opt.step()
    assert tr2.updates_done == 4 and tr2.learning_rate(5) == cosine_lr(0.1, 5, 10)
    # AdamW resumes from torch's 'step'
    tr = Trainer(torch.nn.Linear(3, 2), optimizer="adamw", schedule="constant", warmup_steps=10)
    for _ in range(3):
        grads(tr); tr.opt.step()
    tr2 = Trainer(torch.nn.Linear(3, 2), optimizer="adamw", schedule="constant", warmup_steps=10)
    tr2.opt.load_state_dict(tr.opt.state_dict())
    assert tr2.updates_done == 3 and tr2.learning_rate(0) == pytest.approx(2e-4 * 4 / 10, rel=1e-15)
    for bad in (dict(schedule="linear"), dict(warmup_steps=-1), dict(warmup_steps=1.5), dict(optimizer="lamb"),
                dict(optimizer="adam", no_decay="bias_norm"), dict(optimizer="sgd", nesterov=True)):
        with pytest.raises(ValueError):
            Trainer(torch.nn.Linear(3, 2), **bad)


# ------------------------------------------------------------------------------------------------------------------ constructors
def test_constructors_reject_what_torch_rejects():
    from cwf.optim import FusedAdamW, FusedSGD
    ps = lambda: [torch.nn.Parameter(torch.zeros(3))]
    for kw in (dict(nesterov=True), dict(nesterov=True, momentum=0.9, dampening=0.1), dict(momentum=-0.1), dict(lr=-1.0),
               dict(weight_decay=-1.0), dict(dampening=-0.5), dict(lr=float("nan")), dict(ema_decay=0.3), dict(max_grad_norm=0.0),
               dict(no_decay="all")):
        with pytest.raises(ValueError):
            FusedSGD(ps(), **kw)
    for kw in (dict(betas=(1.0, 0.999)), dict(betas=(0.9, -0.1)), dict(eps=-1e-8), dict(lr=-1.0), dict(weight_decay=-1.0),
               dict(ema_decay=1.0), dict(no_decay=3)):
        with pytest.raises(ValueError):
            FusedAdamW(ps(), **kw)
    with pytest.raises(ValueError, match="one parameter group"):
        FusedSGD([{"params": ps()}, {"params": ps()}])
    FusedSGD(ps(), momentum=0.99, nesterov=True)
    FusedAdamW(ps(), amsgrad=True, no_decay="bias_norm")


# ------------------------------------------------------------------------------------------------------------------ host logic
def _fused(rule, kw, p0, mask=None, **extra):
    from cwf.optim import FusedAdamW, FusedSGD
    ps = [torch.nn.Parameter(t.clone()) for t in p0]
    if mask is not None:
        extra["no_decay"] = lambda name, p: mask[int(name)]
    return ps, (FusedAdamW if rule == "adamw" else FusedSGD)([(str(i), p) for i, p in enumerate(ps)], **kw, **extra)


def _feed(ps, opt, grads):
    for gs in grads:
        for p, g in zip(ps, gs):
            p.grad = g.clone()
        opt.step()


@pytest.mark.parametrize("case", sorted(ref.CASES))
def test_fused_classes_through_the_emulation_match_the_yardstick(rules_emul, case):
    """FusedAdamW / FusedSGD with clip + EMA and a mask, the launch emulated in fp32 torch ops: the host side -- table columns, the
    first-update flag, wd_mul, the step count -- is right when weights, EMA and state agree with the float64 run (1e-5 relative L2:
    this is fp32 against float64 under clipping, not the GPU bound)."""
    rule, kw = ref.CASES[case]
    p0, grads = sref.make_inputs(**SMALL)
    r64 = ref.run_torch(rule, kw, p0, grads, torch.float64, max_norm=1.0, ema_decay=0.9, mask=MASK)
    ps, opt = _fused(rule, kw, p0, mask=MASK, max_grad_norm=1.0, ema_decay=0.9)
    _feed(ps, opt, grads)
    steps = [c for c in rules_emul.calls if c[0] == "optim_step"]
    assert [c[0] for c in rules_emul.calls] == ["grad_norm_clip", "optim_step"] * len(grads)
    has_buf = rule == "sgd" and kw["momentum"] > 0
    assert [c[6] for c in steps] == ([True] + [False] * (len(grads) - 1) if has_buf else [rule == "sgd"] * len(grads))
    if rule == "adamw":
        assert [c[3] for c in steps] == list(range(1, len(grads) + 1))
    for i, p in enumerate(ps):
        assert ref.rel_l2(p, r64["w"][i]) < 1e-5 and ref.rel_l2(opt.ema[i], r64["ema"][i]) < 1e-5
        for k in ref.state_names(rule, kw):
            assert ref.rel_l2(opt.state[p][k], r64[k][i]) < 1e-5, (k, i)
        assert set(opt.state[p].keys()) == set(ref.state_names(rule, kw)) | ({"step"} if rule == "adamw" else set())


def test_state_dict_has_torchs_layout_and_loads_both_ways(rules_emul):
    from cwf.optim import FusedSGD
    p0, grads = sref.make_inputs(**SMALL)
    rule, kw = ref.CASES["sgd_momentum_damp"]
    ps, opt = _fused(rule, kw, p0)
    opt._ensure()                                                     # buffers allocated, not filled: torch has none yet
    assert opt.state_dict()["state"] == {} and opt._first
    _feed(ps, opt, grads[:2])
    sd = opt.state_dict()
    assert all(set(s.keys()) == {"momentum_buffer"} for s in sd["state"].values()) and len(sd["state"]) == 3
    t = ref.run_torch(rule, kw, [p.detach() for p in ps], grads, torch.float32, opt_state=sd, first_step=2)
    _feed(ps, opt, grads[2:])
    assert all(ref.rel_l2(a, b) < 1e-6 for a, b in zip(ps, t["w"]))
    # torch -> fused: after the load the update is not a first one
    t2 = ref.run_torch(rule, kw, p0, grads[:2], torch.float32)
    ps2, opt2 = _fused(rule, kw, [w.detach() for w in t2["w"]])
    opt2.load_state_dict(t2["opt"].state_dict())
    assert not opt2._first
    rules_emul.calls.clear()
    _feed(ps2, opt2, grads[2:])
    assert [c[6] for c in rules_emul.calls if c[0] == "optim_step"] == [False] * (len(grads) - 2)
    assert all(ref.rel_l2(a, b) < 1e-6 for a, b in zip(ps2, ps))
    # a torch state without buffers (saved before its first step) leaves the first update a first one
    fresh = torch.optim.SGD([torch.nn.Parameter(t.clone()) for t in p0], **kw).state_dict()
    ps3, opt3 = _fused(rule, kw, p0)
    opt3.load_state_dict(fresh)
    assert opt3._first and opt3._steps == 0
    # AdamW: torch's keys, interchangeable with torch.optim.AdamW
    rule, kw = ref.CASES["adamw_amsgrad"]
    ps, opt = _fused(rule, kw, p0)
    _feed(ps, opt, grads[:2])
    sd = opt.state_dict()
    assert all(set(s.keys()) == {"step", "exp_avg", "exp_avg_sq", "max_exp_avg_sq"} for s in sd["state"].values())
    t = ref.run_torch(rule, kw, [p.detach() for p in ps], grads, torch.float32, opt_state=sd, first_step=2)
    _feed(ps, opt, grads[2:])
    assert all(ref.rel_l2(a, b) < 1e-6 for a, b in zip(ps, t["w"]))
    assert isinstance(FusedSGD([torch.nn.Parameter(torch.zeros(2))]).state_dict()["param_groups"][0]["updates"], int)


def test_fused_adam_defaults_still_issue_the_plain_adam_launch(rules_emul):
    from cwf.optim import FusedAdam, FusedOptimizer
    ps = [torch.nn.Parameter(torch.randn(n)) for n in (5, 12, 3)]
    opt = FusedAdam(ps, lr=2e-4, weight_decay=1e-5, amsgrad=True)
    assert isinstance(opt, FusedOptimizer)
    for p in ps:
        p.grad = torch.ones_like(p)
    opt.step()
    assert rules_emul.calls == [("adam", 2e-4, 1, 1.0)]
    assert opt._wd_mul is None and opt._no_decay is None and opt.acc is None and opt.ema is None and opt._clip is None


# ------------------------------------------------------------------------------------------------------------------ CLI
def test_cli_flags_default_to_todays_run_and_are_validated():
    import train_no_amp as T
    p = T.build_parser()
    a = p.parse_args([])
    assert (a.optimizer, a.momentum, a.nesterov, a.beta1, a.beta2, a.no_decay, a.lr_schedule, a.warmup_steps) == \
        ("adam", 0.0, False, 0.9, 0.999, None, "poly", 0)
    T.check_optimizer(a)
    a = p.parse_args(["--optimizer", "sgd", "--momentum", "0.99", "--nesterov", "true", "--no_decay", "bias_norm", "--lr_schedule",
                      "cosine", "--warmup_steps", "500"])
    T.check_optimizer(a)
    assert (a.optimizer, a.momentum, a.nesterov, a.no_decay, a.lr_schedule, a.warmup_steps) == ("sgd", 0.99, True, "bias_norm", "cosine", 500)
    T.check_optimizer(p.parse_args(["--optimizer", "adamw", "--beta2", "0.95", "--no_decay", "bias_norm"]))
    for bad in (["--nesterov", "true"], ["--optimizer", "sgd", "--nesterov", "true"], ["--momentum", "0.9"], ["--beta1", "1.0"],
                ["--no_decay", "bias_norm"], ["--warmup_steps", "-1"], ["--optimizer", "sgd", "--momentum", "-1"]):
        with pytest.raises(SystemExit) as e:
            T.check_optimizer(p.parse_args(bad))
        assert "--" in str(e.value)
        with pytest.raises(SystemExit):               # and main() runs the check before it touches a device
            T.main(bad)
