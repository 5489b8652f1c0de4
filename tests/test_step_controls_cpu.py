"""Step controls (gradient accumulation, clipping by global norm, EMA weights) -- everything that needs no GPU: the yardstick's
self-check, the host logic of cwf.optim.FusedAdam / cwf.trainer.Trainer through the kernel emulation, checkpoints and the CLI."""
import ctypes
import math

import numpy as np
import pytest
import torch

import step_controls_ref as ref
from oracle.kernel_emul import EmulBackend


class StepEmul(EmulBackend):
    """oracle.kernel_emul.EmulBackend plus the three step-control methods of HipBackend in torch ops (host memory); records which
    optimizer entry points were used, with the learning rate and step they were given."""

    def __init__(self):
        super().__init__()
        self.calls = []

    def adam(self, table, ntensors, max_n, lr, beta1, beta2, eps, wd, step, amsgrad, hyper_dev=None, grad_scale=1.0, _rec=True):
        if _rec:
            self.calls.append(("adam", lr, step, grad_scale))
        super().adam(table, ntensors, max_n, lr, beta1, beta2, eps, wd, step, amsgrad, hyper_dev=hyper_dev, grad_scale=grad_scale)

    def grad_add(self, a, b, y):
        self.calls.append(("grad_add", b is not None, y.numel()))
        if b is None:
            y.copy_(a)
        else:
            torch.add(a, b, out=y)
        return y

    def grad_norm_clip(self, g, grad_scale, max_norm, ws, out2):
        self.calls.append(("grad_norm_clip", grad_scale, max_norm))
        coef, norm = ref.clip_coef64(ref.sq_norm64(g.numpy()), grad_scale, max_norm)
        out2[0], out2[1] = coef, norm
        return out2

    def adam_ex(self, table, ntensors, max_n, lr, beta1, beta2, eps, wd, step, amsgrad, hyper_dev=None, grad_scale=1.0,
                gscale_dev=None, ema_table=None, ema_weight=0.0):
        self.calls.append(("adam_ex", lr, step, grad_scale, gscale_dev is not None, ema_table is not None))
        if gscale_dev is not None:
            grad_scale = float(gscale_dev[0])
        self.adam(table, ntensors, max_n, lr, beta1, beta2, eps, wd, step, amsgrad, hyper_dev=hyper_dev, grad_scale=grad_scale, _rec=False)
        if ema_table is not None:
            assert 0.0 < ema_weight <= 0.5
            for row, ep in zip(table.tolist()[:ntensors], ema_table.tolist()):
                n = row[5]
                view = lambda ptr: torch.from_numpy(np.ctypeslib.as_array((ctypes.c_float * n).from_address(int(ptr))))
                view(ep).lerp_(view(row[0]), ema_weight)


@pytest.fixture()
def step_emul():
    from cwf import kernels
    old = kernels._backend
    K = StepEmul()
    kernels._set_backend_for_testing(K)
    yield K
    kernels._set_backend_for_testing(old)


# ------------------------------------------------------------------------------------------------------------------ the yardstick
def test_yardstick_fp32_torch_stays_inside_the_bounds_used_on_the_gpu():
    """fp32 torch (Adam amsgrad + clip_grad_norm_ + lerp_) against the float64 run from the same fp32 inputs: weights and EMA inside
    rtol 1e-6 / atol 1e-7, moments within 6e-7 relative L2 -- the bounds the GPU tests hold the fused kernel to are ones an honest
    fp32 implementation meets."""
    p0, grads = ref.make_inputs()
    for decay in (0.9, 0.999):
        r64 = ref.run_torch(p0, grads, torch.float64, max_norm=1.0, ema_decay=decay)
        r32 = ref.run_torch(p0, grads, torch.float32, max_norm=1.0, ema_decay=decay)
        for i in range(len(p0)):
            assert ref.close(r32["w"][i], r64["w"][i]), i
            assert ref.close(r32["ema"][i], r64["ema"][i]), i
            for k in ref.MOMENTS:
                assert ref.rel_l2(r32[k][i], r64[k][i]) <= 6e-7, (k, i)
        # the coefficient formula: torch's own total norm against the float64 restatement
        for step, gs in enumerate(grads):
            coef, norm = ref.clip_coef64(sum(ref.sq_norm64(g.numpy()) for g in gs), 1.0, 1.0)
            assert abs(norm - r64["norms"][step]) <= 1e-12 * norm
            assert coef == pytest.approx(1.0 / (norm + 1e-6), rel=1e-15)


def test_yardstick_accumulated_sum_is_fp32_in_order():
    a, b, c = (np.float32(x) for x in (1.0, 2.0 ** -24, 2.0 ** -24))
    assert ref.accumulated_sum([np.array([a]), np.array([b]), np.array([c])])[0] == np.float32(1.0)        # (1 + e) + e: both lost
    assert ref.accumulated_sum([np.array([b]), np.array([c]), np.array([a])])[0] == np.float32(1.0 + 2.0 ** -23)
    assert ref.clip_coef64(0.0, 0.5, 1.0) == (0.5, 0.0)
    assert ref.clip_coef64(1e60, 0.5, float("inf"))[0] == 0.5


# ------------------------------------------------------------------------------------------------------------------ FusedAdam
def _params(sizes=(5, 12, 3)):
    gen = torch.Generator().manual_seed(3)
    return [torch.nn.Parameter(torch.randn(n, generator=gen)) for n in sizes]


def test_defaults_issue_the_plain_adam_launch_and_allocate_nothing(step_emul):
    from cwf.optim import FusedAdam
    ps = _params()
    opt = FusedAdam(ps, lr=2e-4, weight_decay=1e-5, amsgrad=True)
    for p in ps:
        p.grad = torch.ones_like(p)
    opt.step()
    assert [c[0] for c in step_emul.calls] == ["adam"]
    assert opt.acc is None and opt.ema is None and opt.grad_norm is None and opt._ema_table is None and opt._clip is None


def test_accumulate_fold_window_protocol(step_emul):
    """acc = flat | acc += flat | flat += acc: the window's sum in fp32, micro-step order; fold by slices touches only the slice; the
    step counter, state['step'] and the learning rate belong to the update call alone."""
    from cwf.optim import FusedAdam
    ps = _params()
    opt = FusedAdam(ps, lr=1.0, weight_decay=0.0, amsgrad=True)
    opt._ensure()
    n = opt.flat_grad.numel()
    gen = torch.Generator().manual_seed(4)
    gs = [torch.randn(n, generator=gen) * s for s in (1.0, 1e-4, 1e4)]
    with pytest.raises(RuntimeError):
        opt.fold()
    with pytest.raises(RuntimeError):
        opt.accumulate(first=False)
    opt.flat_grad.copy_(gs[0]); opt.accumulate(first=True)
    assert torch.equal(opt.acc, gs[0]) and opt.acc.data_ptr() != opt.flat_grad.data_ptr()
    opt.flat_grad.copy_(gs[1]); opt.accumulate(first=False)
    assert opt._steps == 0 and all(float(opt.state[p]["step"]) == 0 for p in ps)
    opt.flat_grad.copy_(gs[2])
    want = torch.from_numpy(ref.accumulated_sum([g.numpy() for g in gs]))
    opt.fold(2, 9)
    assert torch.equal(opt.flat_grad[2:9], want[2:9]) and torch.equal(opt.flat_grad[:2], gs[2][:2]) and torch.equal(opt.flat_grad[9:], gs[2][9:])
    opt.fold(0, 2); opt.fold(9); opt.fold(4, 4)
    assert torch.equal(opt.flat_grad, want)
    # a new window starts over
    opt.flat_grad.copy_(gs[1]); opt.accumulate(first=True)
    assert torch.equal(opt.acc, gs[1])
    # the update: lr read at the launch, one count per window
    opt.param_groups[0]["lr"] = 0.125
    opt.grad_scale = 1.0 / 3
    step_emul.calls.clear()
    opt.advance_host(); opt.launch()
    assert step_emul.calls == [("adam", 0.125, 1, 1.0 / 3)]
    assert opt._steps == 1 and all(float(opt.state[p]["step"]) == 1 for p in ps)


def test_clip_and_ema_through_the_emulation_match_the_yardstick(step_emul):
    """FusedAdam(max_grad_norm, ema_decay).step() == torch Adam + clip_grad_norm_ + lerp_; grad_norm is the pre-clip norm; the EMA
    starts from the weights and reset_ema() returns it there; state_dict() keeps torch's layout and loads into torch.optim.Adam."""
    from cwf.optim import FusedAdam
    p0, grads = ref.make_inputs(sizes=(1, 7, 300), steps=4)
    r64 = ref.run_torch(p0, grads, torch.float64, max_norm=1.0, ema_decay=0.9)
    ps = [torch.nn.Parameter(t.clone()) for t in p0]
    opt = FusedAdam(ps, lr=ref.LR, weight_decay=ref.WD, amsgrad=True, max_grad_norm=1.0, ema_decay=0.9)
    opt._ensure()
    assert all(torch.equal(e, p) and e.data_ptr() != p.data_ptr() for e, p in zip(opt.ema, ps))
    for i, gs in enumerate(grads):
        for p, g in zip(ps, gs):
            p.grad = g.clone()
        opt.step()
        assert float(opt.grad_norm) == pytest.approx(r64["norms"][i], rel=1e-6)
    assert [c[0] for c in step_emul.calls] == ["grad_norm_clip", "adam_ex"] * len(grads)
    for i in range(len(ps)):
        assert ref.close(ps[i], r64["w"][i], rtol=1e-5, atol=1e-6) and ref.close(opt.ema[i], r64["ema"][i], rtol=1e-5, atol=1e-6)
    sd = opt.state_dict()
    assert set(sd.keys()) == {"state", "param_groups"}
    assert all(set(s.keys()) == {"step", "exp_avg", "exp_avg_sq", "max_exp_avg_sq"} for s in sd["state"].values())
    plain = FusedAdam([torch.nn.Parameter(t.clone()) for t in p0], lr=ref.LR, weight_decay=ref.WD, amsgrad=True)
    assert set(sd["param_groups"][0].keys()) == set(plain.state_dict()["param_groups"][0].keys())
    topt = torch.optim.Adam([torch.nn.Parameter(t.clone()) for t in p0], lr=ref.LR, weight_decay=ref.WD, amsgrad=True)
    topt.load_state_dict(sd)
    assert torch.equal(topt.state[topt.param_groups[0]["params"][2]]["exp_avg"], opt.state[ps[2]]["exp_avg"])
    # load_state_dict rebuilds the descriptor table and with it the EMA pointer table; the EMA values survive
    before = [e.clone() for e in opt.ema]
    opt.load_state_dict(sd)
    opt._ensure()
    assert opt._ema_table.tolist() == [e.data_ptr() for e in opt.ema] and all(torch.equal(a, b) for a, b in zip(before, opt.ema))
    opt.reset_ema()
    assert all(torch.equal(e, p) for e, p in zip(opt.ema, ps))
    with pytest.raises(ValueError):
        FusedAdam(_params(), ema_decay=0.3)
    with pytest.raises(ValueError):
        FusedAdam(_params(), max_grad_norm=-1.0)


# ------------------------------------------------------------------------------------------------------------------ checkpoints, CLI
def test_ema_checkpoint_round_trip(tmp_path):
    from cwf.trainer import save_checkpoint, load_checkpoint
    m = torch.nn.Sequential(torch.nn.Linear(3, 4), torch.nn.BatchNorm1d(4))
    opt = torch.optim.Adam(m.parameters(), lr=2e-4, amsgrad=True)
    ema = {k: (v + 1 if v.is_floating_point() else v.clone()) for k, v in m.state_dict().items()}
    with_ema, without = str(tmp_path / "a.pth"), str(tmp_path / "b.pth")
    save_checkpoint(with_ema, m, opt, 7, ema=ema)
    save_checkpoint(without, m, opt, 7)
    ck = torch.load(with_ema, map_location="cpu", weights_only=True)
    assert set(ck.keys()) == {"epoch", "state_dict", "optim_dict", "ema_state_dict"}
    assert list(ck["ema_state_dict"].keys()) == list(ck["state_dict"].keys()) and all(k.startswith("module.") for k in ck["ema_state_dict"])
    assert set(torch.load(without, map_location="cpu", weights_only=True).keys()) == {"epoch", "state_dict", "optim_dict"}
    m2 = torch.nn.Sequential(torch.nn.Linear(3, 4), torch.nn.BatchNorm1d(4))
    assert load_checkpoint(with_ema, m2, use_ema=True) == 7
    assert all(torch.equal(m2.state_dict()[k], ema[k]) for k in ema)
    assert load_checkpoint(with_ema, m2) == 7
    assert all(torch.equal(m2.state_dict()[k], v) for k, v in m.state_dict().items())
    with pytest.raises(KeyError, match="ema_state_dict"):
        load_checkpoint(without, m2, use_ema=True)


def test_cli_flags_and_their_validation():
    import train_no_amp as T
    p = T.build_parser()
    a = p.parse_args([])
    assert a.accum_steps == 1 and a.clip_grad_norm is None and a.ema_decay is None
    T.check_step_controls(a)
    a = p.parse_args(["--accum_steps", "8", "--clip_grad_norm", "1.5", "--ema_decay", "0.999"])
    assert (a.accum_steps, a.clip_grad_norm, a.ema_decay) == (8, 1.5, 0.999)
    T.check_step_controls(a)
    T.check_step_controls(p.parse_args(["--ema_decay", "0.5"]))
    for bad in (["--accum_steps", "0"], ["--clip_grad_norm", "0"], ["--clip_grad_norm", "-1"], ["--clip_grad_norm", "nan"],
                ["--ema_decay", "1.0"], ["--ema_decay", "0.49"], ["--ema_decay", "nan"]):
        with pytest.raises(SystemExit) as e:
            T.check_step_controls(p.parse_args(bad))
        assert bad[0] in str(e.value)
        with pytest.raises(SystemExit) as e:          # and main() runs the check before it touches a device
            T.main(bad)
        assert bad[0] in str(e.value)
    helps = {act.dest: act.help for act in p._actions}
    assert "epoch boundary" in helps["accum_steps"] and "dropped" in helps["accum_steps"] and "dropped" in helps["ema_decay"]


# ------------------------------------------------------------------------------------------------------------------ Trainer, real model
def _no_dropout_model():
    from oracle import reference_model as rm
    from utils import synthetic as syn
    from models.clswiseformer.cls_wise_former import get_cls_wise_former
    m = get_cls_wise_former(dataset="brats", _conv_repr=True, _pe_type="fixed")
    m.load_state_dict(syn.det_state_dict(rm.param_shapes()), strict=False)
    m.Unet_list.InitConv.dropout = 0.0
    for mod in m.modules():
        if hasattr(mod, "dropout_rate"):
            mod.dropout_rate = 0.0
        if isinstance(mod, torch.nn.Dropout):
            mod.p = 0.0
    return m.train()


def test_real_trainer_accumulates_two_micro_batches(step_emul):
    """The ACTUAL Trainer on the ACTUAL model (kernels through the emulation, 64^3, samples 0 and 1, dropout off), accum_steps=2:
    micro-step 1 leaves the weights bit-unchanged and the optimizer uncounted; after micro-step 2 the flat gradient is the sum of the
    two plain-autograd gradients (2e-6 relative norm: the bound test_real_trainer_world2_gloo_overlapped_allreduce holds the same sum
    over ranks to) and ONE update has been made, with grad_scale 1/2 and the learning rate of the second call's epoch."""
    from cwf.optim import poly_lr
    from cwf.trainer import Trainer, total_loss
    from utils import synthetic as syn
    torch.set_num_threads(max(torch.get_num_threads(), 4))
    model = _no_dropout_model()
    tr = Trainer(model, accum_steps=2)
    assert tr.opt.grad_scale == 0.5 and tr.opt.acc is None and tr.opt.ema is None and tr.opt.grad_norm is None
    batches = [syn.synthetic_batch([i], (64, 64, 64)) for i in (0, 1)]
    w_start = [p.detach().clone() for p in model.parameters()]
    tr.step(*batches[0], epoch=0)
    assert all(torch.equal(a, b) for a, b in zip(w_start, model.parameters()))
    assert tr.opt._steps == 0 and not any(c[0] in ("adam", "adam_ex") for c in step_emul.calls)
    assert [c for c in step_emul.calls if c[0] == "grad_add"] == [("grad_add", False, tr.opt.flat_grad.numel())]
    tr.step(*batches[1], epoch=500)
    refm = _no_dropout_model()
    pair = dict(zip(map(id, model.parameters()), refm.parameters()))
    want = torch.zeros_like(tr.opt.flat_grad)
    for xb, tb, eb in batches:
        refm.zero_grad(set_to_none=True)
        loss, _ = total_loss(refm(xb, None), tb, eb)
        loss.backward()
        want += torch.cat([pair[id(p)].grad.reshape(-1) for p in tr.opt.sink.params])
    err = float((tr.opt.flat_grad - want).norm() / want.norm())
    assert err < 2e-6, "flat gradient != sum of the two micro-batch gradients: %g" % err
    updates = [c for c in step_emul.calls if c[0] in ("adam", "adam_ex")]
    assert updates == [("adam", float(poly_lr(2e-4, 500, 1000)), 1, 0.5)]
    assert tr.opt._steps == 1 and tr._micro == 0
    assert any(not torch.equal(a, b) for a, b in zip(w_start, model.parameters()))
    with pytest.raises(RuntimeError):
        tr.ema_state_dict()
    with pytest.raises(ValueError):
        Trainer(model, accum_steps=0)
