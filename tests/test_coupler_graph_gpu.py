"""GPU: the coupler Functions of cwf/coupler.py on the HIP kernels against the float64 autograd reference of tests/coupler_ref.py,
per route: the cases, routes and bound of test_coupler_ref_cpu.py (which runs them over the kernel emulation), here with the
kernels that train.  The reference evaluates the counter generator at the device's {seed, step} (as _emul_synced of
test_coupler_gpu.py does) at the site offsets recorded from hip.rng_site during the run under test.  Measured figures: DESIGN.md
section 5 (-s prints them)."""
import pytest

import coupler_ref as CR
from oracle.kernel_emul import EmulBackend

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture()
def env(hip):
    from cwf import kernels
    prec = kernels.precision()
    kernels._set_backend_for_testing(hip)
    kernels.set_precision("fp32")

    def begin():
        hip.begin_step(DEV)
        E = EmulBackend()
        seed, step = hip.rng(DEV).cpu().tolist()
        E.set_rng(seed, step)
        return E
    try:
        yield CR.Env(hip, DEV, begin)
    finally:
        kernels.set_precision(prec)
        kernels._set_backend_for_testing(hip)


def _log(s):
    print("\n" + s, end="")


@pytest.mark.parametrize("route", CR.FN_ROUTES)
@pytest.mark.parametrize("shape", list(CR.REGION_SHAPES))
def test_region_coupler(env, monkeypatch, shape, route):
    CR.run_case(CR.region_case(3, *CR.REGION_SHAPES[shape]), env, monkeypatch, route, _log, shape)


@pytest.mark.parametrize("route", CR.FN_ROUTES)
@pytest.mark.parametrize("only", CR.SUBSETS)
def test_region_coupler_unused_outputs(env, monkeypatch, only, route):
    """one output used, the Function sees None for the rest: where nothing flows the gradient is a true zero, not uninitialised
    memory"""
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
    """C5: a weight set applied more than once inside an active GradSink comes out as plain autograd's sum"""
    CR.run_case(CR.c5_case(kind), env, monkeypatch, "C5", _log, kind, rates=CR.C5_RATES, sink=True)


def test_small_adjoints(env):
    CR.small_adjoints(DEV)
