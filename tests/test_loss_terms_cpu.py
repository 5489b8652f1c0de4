"""The supplementary loss terms as the Trainer handles them (cwf.loss_terms.TERMS through cwf.trainer.Trainer), term by term and
without a GPU: the weight rule, the setters, the lazily made weight tensor and its capture guard, and how total_loss is called.
A stub model and the kernel emulation stand in for the network; total_loss is replaced by a recorder."""
import pytest
import torch

from cwf.loss_terms import TERMS
from oracle.kernel_emul import EmulBackend

NAMES = [t.name for t in TERMS]
# constructor options that differ from the defaults, and what total_loss must then receive behind the weight tensor
OPTIONS = {"boundary": {}, "topk": {"topk_percent": 12.5}, "focal": {"focal_params": {"gamma": 3.0}},
           "lovasz": {"lovasz_regions": "regions", "lovasz_only_present": False}}


def _packed_options(name):
    from cwf.trainer import check_focal
    return {"boundary": (), "topk": (12.5,), "focal": (check_focal(None, {"gamma": 3.0})[1],), "lovasz": ((14, 10, 8), False)}[name]


class _Stub(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.w = torch.nn.Parameter(torch.ones(3))

    def forward(self, x, _):
        return [self.w * x.sum() for _ in range(5)]


BATCH = (torch.ones(2), torch.zeros(2, dtype=torch.int64), torch.zeros(2, dtype=torch.int64))


@pytest.fixture()
def emul():
    from cwf import kernels
    old = kernels._backend
    kernels._set_backend_for_testing(EmulBackend())
    yield
    kernels._set_backend_for_testing(old)


def _trainer(*names, **kw):
    from cwf.trainer import Trainer
    for n in names:
        kw.setdefault(n + "_weight", 0.5)
        kw.update(OPTIONS[n])
    return Trainer(_Stub(), **kw)


def _record(monkeypatch, old_signature):
    """cwf.trainer.total_loss replaced by a recorder of how it was called; old_signature: as wrappers written before the keyword terms"""
    from cwf import trainer
    calls = []

    def result(outputs, boundary, kw):
        calls.append((boundary, dict(kw)))
        loss = sum(o.sum() for o in outputs)
        return loss, [loss] * (5 + (boundary is not None) + len(kw))

    def old(outputs, target, edge, boundary=None):
        return result(outputs, boundary, {})

    def new(outputs, target, edge, boundary=None, **kw):
        return result(outputs, boundary, kw)
    monkeypatch.setattr(trainer, "total_loss", old if old_signature else new)
    return calls


def _tensor_of(call, name):
    """the weight tensor of term `name` in a recorded call"""
    boundary, kw = call
    return boundary if name == "boundary" else kw[name][0]


def test_the_table_is_the_four_terms_in_their_order():
    assert NAMES == ["boundary", "topk", "focal", "lovasz"]
    assert [t.tool for t in TERMS] == ["boundary_loss", "topk_ce", "focal_loss", "lovasz_softmax"]


@pytest.mark.parametrize("name", NAMES)
def test_weight_rule_at_construction_and_in_the_setter(name):
    from cwf.trainer import Trainer
    for bad in (-1, float("nan"), float("inf")):
        with pytest.raises(ValueError, match=name + "_weight"):
            Trainer(None, **{name + "_weight": bad})            # (no model, no backend: the check comes first)
    tr = _trainer(name)
    setter = getattr(tr, "set_%s_weight" % name)
    for bad in (-1, float("nan"), float("inf"), None):
        with pytest.raises(ValueError):
            setter(bad)
        with pytest.raises(ValueError):
            tr.set_loss_weight(name, bad)
    assert getattr(tr, name + "_weight") == 0.5 and getattr(tr, "_" + name) is None
    setter(0)
    assert getattr(tr, name + "_weight") == 0.0


@pytest.mark.parametrize("name", NAMES)
def test_setter_needs_the_term_switched_on_at_construction(name):
    tr = _trainer(*[n for n in NAMES if n != name])
    with pytest.raises(ValueError):
        getattr(tr, "set_%s_weight" % name)(0.1)
    assert getattr(tr, name + "_weight") is None and getattr(tr, "_" + name) is None


@pytest.mark.parametrize("name", NAMES)
def test_weight_set_before_the_first_step_fills_the_tensor_and_later_ones_change_it_in_place(name, emul, monkeypatch):
    calls = _record(monkeypatch, old_signature=False)
    tr = _trainer(name)
    getattr(tr, "set_%s_weight" % name)(0.25)
    assert getattr(tr, "_" + name) is None                      # no tensor before a step needs it
    tr._fwd_bwd(*BATCH)
    made = _tensor_of(calls[-1], name)
    assert made is getattr(tr, "_" + name) and made.dtype == torch.float32 and made.tolist() == [0.25]
    getattr(tr, "set_%s_weight" % name)(0.75)
    assert getattr(tr, "_" + name) is made and made.tolist() == [0.75] and getattr(tr, name + "_weight") == 0.75
    tr._fwd_bwd(*BATCH)
    assert _tensor_of(calls[-1], name) is made


@pytest.mark.parametrize("name", NAMES)
def test_weight_tensor_must_exist_before_the_step_is_captured(name, emul, monkeypatch):
    from cwf import trainer
    _record(monkeypatch, old_signature=False)
    tr = _trainer(name)
    with monkeypatch.context() as m:
        m.setattr(trainer, "_capturing", lambda: True)
        with pytest.raises(RuntimeError, match="must exist before the step is captured"):
            tr._fwd_bwd(*BATCH)
        assert getattr(tr, "_" + name) is None
    tr._fwd_bwd(*BATCH)                                         # made outside the capture ...
    made = getattr(tr, "_" + name)
    with monkeypatch.context() as m:
        m.setattr(trainer, "_capturing", lambda: True)
        tr._fwd_bwd(*BATCH)                                     # ... it is what a capturing step uses
    assert getattr(tr, "_" + name) is made


@pytest.mark.parametrize("name", [None] + NAMES)
def test_total_loss_is_called_with_the_active_term_alone(name, emul, monkeypatch):
    """nothing or the boundary term alone: a wrapper with the signature from before the keyword terms still serves"""
    calls = _record(monkeypatch, old_signature=name in (None, "boundary"))
    tr = _trainer(*([name] if name else []))
    loss, parts = tr._fwd_bwd(*BATCH)
    assert len(parts) == 5 + (name is not None) and len(calls) == 1
    boundary, kw = calls[0]
    if name in (None, "boundary"):
        assert kw == {} and (boundary is None) == (name is None)
    else:
        assert boundary is None and list(kw) == [name] and tuple(kw[name][1:]) == _packed_options(name)
    for n in NAMES:
        assert (getattr(tr, "_" + n) is None) == (n != name)      # a term that is off gets no device tensor


def test_total_loss_is_called_with_all_four_terms_in_the_table_order(emul, monkeypatch):
    calls = _record(monkeypatch, old_signature=False)
    tr = _trainer(*NAMES)
    loss, parts = tr._fwd_bwd(*BATCH)
    boundary, kw = calls[0]
    assert len(parts) == 9 and boundary is tr._boundary and list(kw) == NAMES[1:]
    assert kw["topk"] == (tr._topk, 12.5) and kw["lovasz"] == (tr._lovasz, (14, 10, 8), False)
    assert kw["focal"][0] is tr._focal and (kw["focal"][1],) == _packed_options("focal") and len(kw["focal"]) == 2
    assert len({id(t) for t in (tr._boundary, tr._topk, tr._focal, tr._lovasz)}) == 4
