"""CPU: the coupler Functions of cwf/coupler.py over the kernel emulation against the float64 autograd reference of
tests/coupler_ref.py, per route.  The emulation states each kernel in torch ops, so what this file pins without a GPU is the host
code itself: the hand-derived chain rule, which counter offset goes with which backward launch, which GEMM writes a shared weight set
and which one accumulates, the class-token sums and the destinations in the gradient sink.  test_coupler_graph_gpu.py runs the same
cases on the HIP kernels.

Routes (coupler_ref.ROUTES): C0 dropout off; C1 all four rates 0.1; C1a p_attn = p_select = 0 (the (p_pre, 0.0) branch of _ca_fwd, no
selection or attention site); C1b p_pre = p_ffn = 0; C2 = C1 inside a GradSink over all parameters, the flat buffer NaN-filled before
backward; C3 = C2 with one weight of one set frozen (autograd fall-back, finish() copies in); C4 selections of group 1
teacher-forced (the torch.cat assembly of _select); C5 one weight set applied more than once under a sink must come out as the sum.
Bound per tensor: 16 x the float32 statement's own error (relative L2 and max abs); measured figures: DESIGN.md section 5 (-s prints
them)."""
import pytest
import torch

import coupler_ref as CR
from oracle.kernel_emul import EmulBackend


@pytest.fixture()
def env(emul_backend):
    from cwf import kernels
    K = kernels.backend()

    def begin():
        K.begin_step(None)
        return K
    return CR.Env(K, "cpu", begin)


def _log(s):
    print("\n" + s, end="")


def test_site_bookkeeping_rejects_what_it_should():
    """the reference's own guards: overlapping counter ranges, a site of another extent, a site left over, a site too few"""
    CR.check_disjoint([(0, 10), (20, 5), (30, 1)])
    with pytest.raises(AssertionError):
        CR.check_disjoint([(0, 10), (19, 5)])                    # [0, 20) and [19, 29)
    K = EmulBackend()
    like = torch.zeros(1)
    s = CR.Sites([(0, 12), (24, 6)], K)
    assert s.take((3, 4), 0.1, 0.0, like).shape == (3, 4)
    with pytest.raises(AssertionError):
        s.done()                                                 # one site left over
    with pytest.raises(AssertionError):
        s.take((7,), 0.1, 0.0, like)                             # extent 6 recorded
    with pytest.raises(AssertionError):
        s.take((6,), 0.1, 0.0, like)                             # nothing left
    m = CR.Sites([(5, 8)], K).take((8,), 0.1, 0.2, torch.zeros(1, dtype=torch.float64))
    assert m.dtype == torch.float64 and torch.equal(m.float(), K.keep(5, 8, 0.1, 0.2))


def test_written_out_graph_equals_composition():
    """dropout off, float64: the graph with explicit keep factors (all 1, every multiplication site taken) equals the composition of
    reference_model's select_tokens / intra_region_coupler / cross_region_coupler / scatter_rows, outputs and autograd gradients"""
    for case, k in ((CR.region_case(3, 2, 80, 48, 16), 16), (CR.fusion_case(2, 48, 16), 16), (CR.intra_block_case(2, 17), 0),
                    (CR.fusion_block_case(2, 17), 0)):
        L = {n: t.double() for n, t in case.leaves.items()}
        if case.name == "region":
            q = [(L["E"], "e_tok"), (L["S"], "e_tok"), (L["S"], "s_tok"), (L["E"], "s_tok")]
            sel = [torch.cat([torch.einsum("e,bne->bn", L["%s%d" % (tk, g)][0, 0], f[g]).topk(k, dim=1).indices for g in range(3)], 0)
                   for f, tk in q]
        elif case.name == "fusion":
            sel = [torch.einsum("be,bne->bn", L["tok"][:, 0], L["feats"]).topk(k, dim=1).indices]
        else:
            sel = []
        a = CR.run_reference(case, torch.float64, sel, CR.Rates(), None)
        b = CR.run_reference(case, torch.float64, sel, CR.Rates(0.1, 0.1, 0.1, 0.1), CR.Sites(ones=True))
        assert set(a) == set(b)
        for n in a:
            assert float((a[n] - b[n]).norm()) <= 1e-12 * float(a[n].norm()) and float(a[n].norm()) > 0, (case.name, n)


@pytest.mark.parametrize("route", CR.FN_ROUTES)
@pytest.mark.parametrize("shape", list(CR.REGION_SHAPES))
def test_region_coupler(env, monkeypatch, shape, route):
    CR.run_case(CR.region_case(3, *CR.REGION_SHAPES[shape]), env, monkeypatch, route, _log, shape)


@pytest.mark.parametrize("route", CR.FN_ROUTES)
@pytest.mark.parametrize("only", CR.SUBSETS)
def test_region_coupler_unused_outputs(env, monkeypatch, only, route):
    """one output used, the Function sees None for the rest: where nothing flows the gradient is a true zero, not uninitialised
    memory (coupler_ref.compare holds every element that is exactly zero in both references to exactly zero)"""
    CR.run_case(CR.region_case(3, *CR.REGION_SHAPES["1-t17"], used=(only,)), env, monkeypatch, route, _log, "only " + only)


@pytest.mark.parametrize("route", CR.FN_ROUTES)
@pytest.mark.parametrize("shape", list(CR.FUSION_SHAPES))
def test_fusion_coupler(env, monkeypatch, shape, route):
    CR.run_case(CR.fusion_case(*CR.FUSION_SHAPES[shape]), env, monkeypatch, route, _log, shape)


@pytest.mark.parametrize("route", CR.BLOCK_ROUTES)
@pytest.mark.parametrize("t", CR.INTRA_T)
def test_intra_coupler_block(env, monkeypatch, t, route):
    CR.run_case(CR.intra_block_case(2, t), env, monkeypatch, route, _log, "t%d" % t)


@pytest.mark.parametrize("route", CR.BLOCK_ROUTES)
@pytest.mark.parametrize("t", CR.FUSION_BLOCK_T)
def test_fusion_block(env, monkeypatch, t, route):
    CR.run_case(CR.fusion_block_case(2, t), env, monkeypatch, route, _log, "t%d" % t)


@pytest.mark.parametrize("route", CR.ENCODE_ROUTES)
def test_encode_coupler_section(env, monkeypatch, route):
    CR.run_case(CR.encode_case(), env, monkeypatch, route, _log)


@pytest.mark.parametrize("kind", CR.C5_KINDS)
def test_shared_weight_set_under_sink_is_the_sum(env, monkeypatch, kind):
    """C5: a weight set applied more than once inside an active GradSink (within one Function type and across the coupler
    Functions) comes out as plain autograd's sum.  Before _grad_buffers guarded the case, the second backward overwrote the slices
    the first had written (relative error 0.49 - 0.78 per weight tensor)."""
    CR.run_case(CR.c5_case(kind), env, monkeypatch, "C5", _log, kind, rates=CR.C5_RATES, sink=True)


def test_small_adjoints(env):
    CR.small_adjoints("cpu")
