"""GPU: the conv autograd glue (cwf/functional.py) on block graphs, per route, against float64.

Every graph of tests/block_graph_ref.py runs at each of its shapes under five routes:
  R0  precision fp32, plain .grad
  R1  bench precision (bf16x3, wgrad bf16, dgrad bf16), plain .grad, outside single_consumer_graph
  R2  bench precision, GradSink, outside single_consumer_graph
  R3  bench precision, GradSink, inside single_consumer_graph, unwritten fp32 carriers poisoned
  R4  R3 with the weight gradients (and to_bf16_side) on the side stream, as Trainer._fwd_bwd sets them up
and is held to
  * a route census: the multiset of backend calls with their distinguishing arguments equals the table written out below (a test that
    stops reaching its branch fails, and so does an optimisation that silently switches off), plus the facts that must hold whatever the
    table says (_check_route_facts);
  * finite results under the poison flag;
  * the float64 reference per tensor: relative L2 <= 16 e32 + ek (R0) or 3 e16 + 16 e32 + ek (R1-R4), all measured on the references
    alone (block_graph_ref.Reference); true-zero bias gradients against sum |dy_ref| of their layer.  Two amendments to the issue's
    yardsticks, both found by this test failing and both made in the references, not in the factors (DESIGN.md section 5 has the figures):
      - the derivative of a (Leaky)ReLU net jumps where a pre-activation changes sign, an fp32 realisation flips a Poisson number of
        such elements (about 1.7 per pass in U1 at 65536 voxels, one flip = 1e-3 of a layer's gradient), and a plain float32 run is one
        draw of that number -- U1 at 34 x 38 x 50 drew none, the fp32 kernels drew two.  So e32 is the float32 run on the truth's
        activation pattern (summation error alone, times 16), and ek, the error of the flips to allow for, is added once;
      - the rounded reference sums hi(dy) for the bias gradient where the weight gradient takes bf16 operands: that is the kernels'
        documented bias slot (tests/bf16_operand_ref.py), an exact sum left every such bias 50 to 800 times over its bound;
  * route equivalence: R2, R3, R4 against R1 by the rule of tests/test_model_gpu.py (relative L2 < max(5e-5, 10 x noise), noise = two
    runs of R1), and the same comparison with one consumer's weight doubled (a link that drops a contribution);
  * no state left behind: NaaLink.sums None, CarryLink.grads empty, K._wg_pending empty, and R3 -> R1 -> R3 on the same modules
    reproduces R3 within the same noise rule.
Measured yardsticks and worst ratios: DESIGN.md section 5 (print them with -s)."""
import collections
import contextlib
import inspect

import pytest
import torch

import block_graph_ref as B

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BENCH = dict(mode="bf16x3", wgrad="bf16", dgrad="bf16")
ROUTES = ("R0", "R1", "R2", "R3", "R4")
CASES = [(name, n, size) for name in B.GRAPHS for n, size in B.GPU_SHAPES[name]]
SPIED = ("conv", "wgrad_to", "wgrad", "in_bwd", "in_bwd_apply", "in_bwd_apply16", "add", "channel_scale", "to_bf16", "norm_act_add")


def _case_id(c):
    return "%s-%dx%dx%dx%d" % (c[0], c[1], *c[2])


# ====================================================================================================================
# the route census
# ====================================================================================================================
def _call_key(name, args):
    """one census entry: the call and its distinguishing arguments"""
    has = lambda k: args.get(k) is not None
    if name == "conv":
        f = ["op%d" % args["op"], "dgrad" if has("fwd_op") else "fwd"] + [k for k in ("residual", "out_scale", "stats", "nb", "x16", "y16") if has(k)]
    elif name == "wgrad_to":
        f = ["op%d" % args["op"]] + [k for k in ("x16", "dy16", "dy_scale") if has(k)] + (["private"] if args.get("allow_async") else [])
    elif name == "wgrad":
        f = ["op%d" % args["op"]] + (["private"] if args.get("allow_async") else [])
    elif name in ("in_bwd", "in_bwd_apply"):
        f = ["dx_add"] if has("dx_add") else []
    elif name == "in_bwd_apply16":
        f = [k for k in ("dx_add",) if has(k)] + [k for k in ("want_dx16", "want_xa16") if args.get(k)] + ["f32" if args.get("need_f32", True) else "no_f32"]
    elif name == "to_bf16":
        f = ["prologue"] if has("scale") else []
    elif name == "norm_act_add":
        f = [k for k in ("residual",) if has(k)] + (["want16"] if args.get("want16") else [])
    else:
        f = []
    return " ".join([name] + f)


@contextlib.contextmanager
def _spy(hip, monkeypatch):
    census = collections.Counter()
    with monkeypatch.context() as m:
        for name in SPIED:
            orig = getattr(hip, name)
            sig = inspect.signature(orig)

            def wrap(*a, _orig=orig, _sig=sig, _name=name, **kw):
                census[_call_key(_name, _sig.bind(*a, **kw).arguments)] += 1
                return _orig(*a, **kw)
            m.setattr(hip, name, wrap)
        yield census


def _count(census, *words):
    """calls whose key starts with words[0] and contains every further word"""
    return sum(v for k, v in census.items() if k.split()[0] == words[0] and all(w in k.split()[1:] for w in words[1:]))


def _check_route_facts(name, n, size, route, c):
    """what must hold whatever the tables say (reasoned from cwf/functional.py and HipBackend's predicates, not observed)"""
    big16 = size[0] * size[1] * size[2] >= 32768            # bf16_operands_ok / dy_scale_ok of the 16-channel full-resolution layers
    what = (name, n, size, route)
    if route == "R0":
        # fp32: no fused norm-backward sums, no bf16 images, no sink
        assert not _count(c, "in_bwd_apply") and not _count(c, "in_bwd_apply16") and not _count(c, "to_bf16") and not _count(c, "wgrad_to"), what
        assert not _count(c, "conv", "nb") and not _count(c, "conv", "x16") and not _count(c, "conv", "y16") and not _count(c, "norm_act_add", "want16"), what
    if route in ("R0", "R1"):
        assert not _count(c, "wgrad_to"), what              # no sink is active
        assert _count(c, "wgrad") > 0, what
    else:
        # under a sink only a weight applied twice (S6) and a layer with a frozen weight but a trained bias (S7) return through autograd
        assert _count(c, "wgrad") == {"S6": 2, "S7": 1}.get(name, 0), what
        assert _count(c, "wgrad", "private") == {"S7": 1}.get(name, 0), what      # (a weight applied twice never goes to the side stream)
    if route in ("R0", "R1", "R2") or (not big16 and name != "U2"):
        assert not _count(c, "in_bwd_apply16", "no_f32"), what          # the bf16-only hand-off needs the declaration AND an eligible layer
    # "private" = allow_async: dy is referenced by the glue alone, so a side stream may read it.  Every sink layer but one whose dy also
    # returns to autograd as the gradient of a PLAIN residual (S5's c2; a carried residual goes through its CarryLink and stays private)
    if route in ("R2", "R3", "R4"):
        assert _count(c, "wgrad_to") - _count(c, "wgrad_to", "private") == (1 if name == "S5" else 0), what
    if not big16 and name not in ("U2",):
        if name != "U1":
            assert not _count(c, "wgrad_to", "x16") and not _count(c, "wgrad_to", "dy16") and not _count(c, "conv", "x16"), what
        assert not _count(c, "conv", "y16") and not _count(c, "norm_act_add", "want16"), what
    # the dy_scale fold: the stem of U1 (input without gradient, under a sink, at or above the threshold) and nothing else
    fold = name == "U1" and big16 and route in ("R2", "R3", "R4")
    assert _count(c, "wgrad_to", "dy_scale") == (1 if fold else 0), what
    assert _count(c, "channel_scale") == (1 if (name in ("U1", "S8") and not fold) else 0), what
    # K.add joins a carried gradient from a link with one from autograd: S3 only
    assert _count(c, "add") == (1 if name == "S3" else 0), what
    if name == "S4":
        assert _count(c, "conv", "dgrad") == 2 and _count(c, "wgrad") + _count(c, "wgrad_to") == 2, what      # c1 has no backward work at all


# (graph, n, size) -> route -> {call key: count}; a route name in place of a table: the same table as that route; a case in place of a
# case's tables: the same tables as that case.  The tables were recorded from a run and then read against cwf/functional.py branch by
# branch; what they cannot be trusted for on that ground is restated independently in _check_route_facts.  A
# multiset does not see the ORDER of calls: wgrad_first / early shows only as R4's wgrad_to of that layer arriving with its x16 image.
# Call keys (_call_key): conv "op<code> fwd|dgrad" + the optional operands present (op codes of cwf.packing: 0 3x3x3, 1 3x3x3 stride 2,
# 2 1x1x1, 3 ConvTranspose, 4 / 5 the data gradients of 1 / 3); wgrad_to / wgrad "op<code>" + bf16 images, dy_scale, "private"
# (allow_async: nothing but the glue references dy); in_bwd_apply16 + dx_add, the images asked for, f32 | no_f32 (need_f32).
CENSUS = {
    ('U1', 2, (32, 32, 32)): {
        "R0": {"channel_scale": 1, "conv op0 dgrad": 8, "conv op0 dgrad residual": 2, "conv op0 fwd out_scale stats": 1, "conv op0 fwd residual": 2,
               "conv op0 fwd residual stats": 1, "conv op0 fwd stats": 7, "conv op1 fwd stats": 1, "conv op2 dgrad": 3, "conv op2 fwd": 3,
               "conv op3 fwd": 1, "conv op4 dgrad residual": 1, "conv op5 dgrad": 1, "in_bwd": 7, "in_bwd dx_add": 3, "norm_act_add residual": 2,
               "wgrad op0 private": 11, "wgrad op1 private": 1, "wgrad op2 private": 3, "wgrad op3 private": 1},
        "R1": {"channel_scale": 1, "conv op0 dgrad residual stats nb x16": 1, "conv op0 dgrad residual x16": 1, "conv op0 dgrad stats nb": 3,
               "conv op0 dgrad stats nb x16": 5, "conv op0 fwd out_scale stats": 1, "conv op0 fwd residual": 2, "conv op0 fwd residual stats": 1,
               "conv op0 fwd stats": 7, "conv op1 fwd stats": 1, "conv op2 dgrad": 2, "conv op2 dgrad stats nb": 1, "conv op2 fwd": 2,
               "conv op2 fwd y16": 1, "conv op3 fwd": 1, "conv op4 dgrad residual": 1, "conv op5 dgrad": 1, "in_bwd_apply dx_add": 2,
               "in_bwd_apply16 dx_add want_dx16 f32": 1, "in_bwd_apply16 want_dx16 f32": 7, "norm_act_add residual": 1,
               "norm_act_add residual want16": 1, "wgrad op0 private": 11, "wgrad op1 private": 1, "wgrad op2 private": 3, "wgrad op3 private": 1},
        "R2": {"conv op0 dgrad residual stats nb x16": 1, "conv op0 dgrad residual x16": 1, "conv op0 dgrad stats nb": 3,
               "conv op0 dgrad stats nb x16": 5, "conv op0 fwd out_scale stats": 1, "conv op0 fwd residual": 2, "conv op0 fwd residual stats": 1,
               "conv op0 fwd stats": 7, "conv op1 fwd stats": 1, "conv op2 dgrad": 2, "conv op2 dgrad stats nb": 1, "conv op2 fwd": 2,
               "conv op2 fwd y16": 1, "conv op3 fwd": 1, "conv op4 dgrad residual": 1, "conv op5 dgrad": 1, "in_bwd_apply dx_add": 1,
               "in_bwd_apply16 dx_add want_dx16 want_xa16 f32": 1, "in_bwd_apply16 dx_add want_xa16 f32": 1, "in_bwd_apply16 want_dx16 f32": 2,
               "in_bwd_apply16 want_dx16 want_xa16 f32": 5, "norm_act_add residual": 1, "norm_act_add residual want16": 1, "to_bf16": 2,
               "to_bf16 prologue": 1, "wgrad_to op0 dy16 private": 1, "wgrad_to op0 dy_scale private": 1, "wgrad_to op0 x16 dy16 private": 7,
               "wgrad_to op0 x16 private": 2, "wgrad_to op1 private": 1, "wgrad_to op2 private": 3, "wgrad_to op3 private": 1},
        "R3": {"conv op0 dgrad residual stats nb x16": 1, "conv op0 dgrad residual x16": 1, "conv op0 dgrad stats nb": 3,
               "conv op0 dgrad stats nb x16": 5, "conv op0 fwd out_scale stats": 1, "conv op0 fwd residual": 2, "conv op0 fwd residual stats": 1,
               "conv op0 fwd stats": 7, "conv op1 fwd stats": 1, "conv op2 dgrad": 2, "conv op2 dgrad stats nb": 1, "conv op2 fwd": 2,
               "conv op2 fwd y16": 1, "conv op3 fwd": 1, "conv op4 dgrad residual": 1, "conv op5 dgrad": 1, "in_bwd_apply dx_add": 1,
               "in_bwd_apply16 dx_add want_dx16 want_xa16 f32": 1, "in_bwd_apply16 dx_add want_xa16 f32": 1, "in_bwd_apply16 want_dx16 no_f32": 2,
               "in_bwd_apply16 want_dx16 want_xa16 f32": 1, "in_bwd_apply16 want_dx16 want_xa16 no_f32": 4, "norm_act_add residual": 1,
               "norm_act_add residual want16": 1, "to_bf16": 2, "to_bf16 prologue": 1, "wgrad_to op0 dy16 private": 1,
               "wgrad_to op0 dy_scale private": 1, "wgrad_to op0 x16 dy16 private": 7, "wgrad_to op0 x16 private": 2, "wgrad_to op1 private": 1,
               "wgrad_to op2 private": 3, "wgrad_to op3 private": 1},
        "R4": {"conv op0 dgrad residual stats nb x16": 1, "conv op0 dgrad residual x16": 1, "conv op0 dgrad stats nb": 3,
               "conv op0 dgrad stats nb x16": 5, "conv op0 fwd out_scale stats": 1, "conv op0 fwd residual": 2, "conv op0 fwd residual stats": 1,
               "conv op0 fwd stats": 7, "conv op1 fwd stats": 1, "conv op2 dgrad": 2, "conv op2 dgrad stats nb": 1, "conv op2 fwd": 2,
               "conv op2 fwd y16": 1, "conv op3 fwd": 1, "conv op4 dgrad residual": 1, "conv op5 dgrad": 1, "in_bwd_apply dx_add": 1,
               "in_bwd_apply16 dx_add want_dx16 want_xa16 f32": 1, "in_bwd_apply16 dx_add want_xa16 f32": 1, "in_bwd_apply16 want_dx16 no_f32": 2,
               "in_bwd_apply16 want_dx16 want_xa16 f32": 1, "in_bwd_apply16 want_dx16 want_xa16 no_f32": 4, "norm_act_add residual": 1,
               "norm_act_add residual want16": 1, "to_bf16": 2, "to_bf16 prologue": 1, "wgrad_to op0 dy_scale private": 1,
               "wgrad_to op0 x16 dy16 private": 8, "wgrad_to op0 x16 private": 2, "wgrad_to op1 private": 1, "wgrad_to op2 private": 3,
               "wgrad_to op3 private": 1},
    },
    ("U1", 1, (34, 38, 50)): ("U1", 2, (32, 32, 32)),
    ('U1', 2, (16, 16, 32)): {
        "R0": {"channel_scale": 1, "conv op0 dgrad": 8, "conv op0 dgrad residual": 2, "conv op0 fwd out_scale stats": 1, "conv op0 fwd residual": 2,
               "conv op0 fwd residual stats": 1, "conv op0 fwd stats": 7, "conv op1 fwd stats": 1, "conv op2 dgrad": 3, "conv op2 fwd": 3,
               "conv op3 fwd": 1, "conv op4 dgrad residual": 1, "conv op5 dgrad": 1, "in_bwd": 7, "in_bwd dx_add": 3, "norm_act_add residual": 2,
               "wgrad op0 private": 11, "wgrad op1 private": 1, "wgrad op2 private": 3, "wgrad op3 private": 1},
        "R1": {"channel_scale": 1, "conv op0 dgrad residual": 1, "conv op0 dgrad residual stats nb": 1, "conv op0 dgrad stats nb": 8,
               "conv op0 fwd out_scale stats": 1, "conv op0 fwd residual": 2, "conv op0 fwd residual stats": 1, "conv op0 fwd stats": 7,
               "conv op1 fwd stats": 1, "conv op2 dgrad": 2, "conv op2 dgrad stats nb": 1, "conv op2 fwd": 3, "conv op3 fwd": 1,
               "conv op4 dgrad residual": 1, "conv op5 dgrad": 1, "in_bwd_apply": 6, "in_bwd_apply dx_add": 3, "in_bwd_apply16 want_dx16 f32": 1,
               "norm_act_add residual": 2, "wgrad op0 private": 11, "wgrad op1 private": 1, "wgrad op2 private": 3, "wgrad op3 private": 1},
        "R2": {"channel_scale": 1, "conv op0 dgrad residual": 1, "conv op0 dgrad residual stats nb": 1, "conv op0 dgrad stats nb": 8,
               "conv op0 fwd out_scale stats": 1, "conv op0 fwd residual": 2, "conv op0 fwd residual stats": 1, "conv op0 fwd stats": 7,
               "conv op1 fwd stats": 1, "conv op2 dgrad": 2, "conv op2 dgrad stats nb": 1, "conv op2 fwd": 3, "conv op3 fwd": 1,
               "conv op4 dgrad residual": 1, "conv op5 dgrad": 1, "in_bwd_apply": 6, "in_bwd_apply dx_add": 2,
               "in_bwd_apply16 dx_add want_xa16 f32": 1, "in_bwd_apply16 want_dx16 want_xa16 f32": 1, "norm_act_add residual": 2, "to_bf16": 1,
               "wgrad_to op0 private": 9, "wgrad_to op0 x16 dy16 private": 1, "wgrad_to op0 x16 private": 1, "wgrad_to op1 private": 1,
               "wgrad_to op2 private": 3, "wgrad_to op3 private": 1},
        "R3": "R2",
        "R4": "R2",
    },
    ('U2', 2, (8, 8, 32)): {
        "R0": {"conv op0 dgrad": 8, "conv op0 dgrad residual": 2, "conv op0 fwd residual": 2, "conv op0 fwd residual stats": 1,
               "conv op0 fwd stats": 7, "conv op1 fwd stats": 1, "conv op2 dgrad": 2, "conv op2 fwd": 2, "conv op3 fwd": 1,
               "conv op4 dgrad residual": 1, "conv op5 dgrad": 1, "in_bwd": 7, "in_bwd dx_add": 3, "norm_act_add residual": 2,
               "wgrad op0 private": 10, "wgrad op1 private": 1, "wgrad op2 private": 2, "wgrad op3 private": 1},
        "R1": {"conv op0 dgrad residual stats nb x16": 1, "conv op0 dgrad residual x16": 1, "conv op0 dgrad stats nb": 3,
               "conv op0 dgrad stats nb x16": 5, "conv op0 fwd residual": 2, "conv op0 fwd residual stats": 1, "conv op0 fwd stats": 7,
               "conv op1 fwd stats": 1, "conv op2 dgrad": 2, "conv op2 fwd": 1, "conv op2 fwd y16": 1, "conv op3 fwd": 1,
               "conv op4 dgrad residual": 1, "conv op5 dgrad": 1, "in_bwd": 1, "in_bwd_apply dx_add": 2, "in_bwd_apply16 dx_add want_dx16 f32": 1,
               "in_bwd_apply16 want_dx16 f32": 6, "norm_act_add residual": 1, "norm_act_add residual want16": 1, "wgrad op0 private": 10,
               "wgrad op1 private": 1, "wgrad op2 private": 2, "wgrad op3 private": 1},
        "R2": {"conv op0 dgrad residual stats nb x16": 1, "conv op0 dgrad residual x16": 1, "conv op0 dgrad stats nb": 3,
               "conv op0 dgrad stats nb x16": 5, "conv op0 fwd residual": 2, "conv op0 fwd residual stats": 1, "conv op0 fwd stats": 7,
               "conv op1 fwd stats": 1, "conv op2 dgrad": 2, "conv op2 fwd": 1, "conv op2 fwd y16": 1, "conv op3 fwd": 1,
               "conv op4 dgrad residual": 1, "conv op5 dgrad": 1, "in_bwd": 1, "in_bwd_apply16 dx_add want_dx16 want_xa16 f32": 1,
               "in_bwd_apply16 dx_add want_xa16 f32": 2, "in_bwd_apply16 want_dx16 f32": 1, "in_bwd_apply16 want_dx16 want_xa16 f32": 5,
               "norm_act_add residual": 1, "norm_act_add residual want16": 1, "to_bf16": 3, "wgrad_to op0 x16 dy16 private": 7,
               "wgrad_to op0 x16 private": 3, "wgrad_to op1 private": 1, "wgrad_to op2 private": 2, "wgrad_to op3 private": 1},
        "R3": {"conv op0 dgrad residual stats nb x16": 1, "conv op0 dgrad residual x16": 1, "conv op0 dgrad stats nb": 3,
               "conv op0 dgrad stats nb x16": 5, "conv op0 fwd residual": 2, "conv op0 fwd residual stats": 1, "conv op0 fwd stats": 7,
               "conv op1 fwd stats": 1, "conv op2 dgrad": 2, "conv op2 fwd": 1, "conv op2 fwd y16": 1, "conv op3 fwd": 1,
               "conv op4 dgrad residual": 1, "conv op5 dgrad": 1, "in_bwd": 1, "in_bwd_apply16 dx_add want_dx16 want_xa16 f32": 1,
               "in_bwd_apply16 dx_add want_xa16 f32": 2, "in_bwd_apply16 want_dx16 no_f32": 1, "in_bwd_apply16 want_dx16 want_xa16 no_f32": 5,
               "norm_act_add residual": 1, "norm_act_add residual want16": 1, "to_bf16": 3, "wgrad_to op0 x16 dy16 private": 7,
               "wgrad_to op0 x16 private": 3, "wgrad_to op1 private": 1, "wgrad_to op2 private": 2, "wgrad_to op3 private": 1},
        "R4": "R3",
    },
    ('U2', 1, (4, 12, 16)): {
        "R0": {"conv op0 dgrad": 8, "conv op0 dgrad residual": 2, "conv op0 fwd residual": 2, "conv op0 fwd residual stats": 1,
               "conv op0 fwd stats": 7, "conv op1 fwd stats": 1, "conv op2 dgrad": 2, "conv op2 fwd": 2, "conv op3 fwd": 1,
               "conv op4 dgrad residual": 1, "conv op5 dgrad": 1, "in_bwd": 7, "in_bwd dx_add": 3, "norm_act_add residual": 2,
               "wgrad op0 private": 10, "wgrad op1 private": 1, "wgrad op2 private": 2, "wgrad op3 private": 1},
        "R1": {"conv op0 dgrad residual stats nb x16": 1, "conv op0 dgrad residual x16": 1, "conv op0 dgrad stats nb": 6,
               "conv op0 dgrad stats nb x16": 2, "conv op0 fwd residual": 2, "conv op0 fwd residual stats": 1, "conv op0 fwd stats": 7,
               "conv op1 fwd stats": 1, "conv op2 dgrad": 2, "conv op2 fwd": 1, "conv op2 fwd y16": 1, "conv op3 fwd": 1,
               "conv op4 dgrad residual": 1, "conv op5 dgrad": 1, "in_bwd": 1, "in_bwd_apply dx_add": 2, "in_bwd_apply16 dx_add want_dx16 f32": 1,
               "in_bwd_apply16 want_dx16 f32": 6, "norm_act_add residual": 1, "norm_act_add residual want16": 1, "wgrad op0 private": 10,
               "wgrad op1 private": 1, "wgrad op2 private": 2, "wgrad op3 private": 1},
        "R2": {"conv op0 dgrad residual stats nb x16": 1, "conv op0 dgrad residual x16": 1, "conv op0 dgrad stats nb": 6,
               "conv op0 dgrad stats nb x16": 2, "conv op0 fwd residual": 2, "conv op0 fwd residual stats": 1, "conv op0 fwd stats": 7,
               "conv op1 fwd stats": 1, "conv op2 dgrad": 2, "conv op2 fwd": 1, "conv op2 fwd y16": 1, "conv op3 fwd": 1,
               "conv op4 dgrad residual": 1, "conv op5 dgrad": 1, "in_bwd": 1, "in_bwd_apply16 dx_add want_dx16 want_xa16 f32": 1,
               "in_bwd_apply16 dx_add want_xa16 f32": 2, "in_bwd_apply16 want_dx16 f32": 1, "in_bwd_apply16 want_dx16 want_xa16 f32": 5,
               "norm_act_add residual": 1, "norm_act_add residual want16": 1, "to_bf16": 3, "wgrad_to op0 x16 dy16 private": 7,
               "wgrad_to op0 x16 private": 3, "wgrad_to op1 private": 1, "wgrad_to op2 private": 2, "wgrad_to op3 private": 1},
        "R3": {"conv op0 dgrad residual stats nb x16": 1, "conv op0 dgrad residual x16": 1, "conv op0 dgrad stats nb": 6,
               "conv op0 dgrad stats nb x16": 2, "conv op0 fwd residual": 2, "conv op0 fwd residual stats": 1, "conv op0 fwd stats": 7,
               "conv op1 fwd stats": 1, "conv op2 dgrad": 2, "conv op2 fwd": 1, "conv op2 fwd y16": 1, "conv op3 fwd": 1,
               "conv op4 dgrad residual": 1, "conv op5 dgrad": 1, "in_bwd": 1, "in_bwd_apply16 dx_add want_dx16 want_xa16 f32": 1,
               "in_bwd_apply16 dx_add want_xa16 f32": 2, "in_bwd_apply16 want_dx16 no_f32": 1, "in_bwd_apply16 want_dx16 want_xa16 f32": 2,
               "in_bwd_apply16 want_dx16 want_xa16 no_f32": 3, "norm_act_add residual": 1, "norm_act_add residual want16": 1, "to_bf16": 3,
               "wgrad_to op0 x16 dy16 private": 7, "wgrad_to op0 x16 private": 3, "wgrad_to op1 private": 1, "wgrad_to op2 private": 2,
               "wgrad_to op3 private": 1},
        "R4": "R3",
    },
    ('S1', 1, (34, 38, 50)): {
        "R0": {"conv op0 dgrad": 3, "conv op0 fwd": 2, "conv op0 fwd stats": 1, "in_bwd": 1, "norm_act_add residual": 1, "wgrad op0 private": 3},
        "R1": "R0",
        "R2": {"conv op0 dgrad": 3, "conv op0 fwd": 2, "conv op0 fwd stats": 1, "in_bwd": 1, "norm_act_add residual": 1, "to_bf16": 6,
               "wgrad_to op0 private": 3},
        "R3": "R2",
        "R4": "R2",
    },
    ('S1', 2, (8, 8, 16)): {
        "R0": {"conv op0 dgrad": 3, "conv op0 fwd": 2, "conv op0 fwd stats": 1, "in_bwd": 1, "norm_act_add residual": 1, "wgrad op0 private": 3},
        "R1": "R0",
        "R2": {"conv op0 dgrad": 3, "conv op0 fwd": 2, "conv op0 fwd stats": 1, "in_bwd": 1, "norm_act_add residual": 1, "wgrad_to op0 private": 3},
        "R3": "R2",
        "R4": "R2",
    },
    ('S2', 1, (34, 38, 50)): {
        "R0": {"conv op0 dgrad": 2, "conv op0 fwd": 1, "conv op0 fwd stats": 1, "in_bwd": 2, "norm_act_add": 1, "wgrad op0 private": 2},
        "R1": {"conv op0 dgrad": 1, "conv op0 dgrad stats nb": 1, "conv op0 fwd": 1, "conv op0 fwd stats": 1, "in_bwd": 1, "in_bwd_apply": 1,
               "norm_act_add": 1, "wgrad op0 private": 2},
        "R2": {"conv op0 dgrad": 1, "conv op0 dgrad stats nb": 1, "conv op0 fwd": 1, "conv op0 fwd stats": 1, "in_bwd": 1,
               "in_bwd_apply16 want_xa16 f32": 1, "norm_act_add": 1, "to_bf16": 3, "wgrad_to op0 private": 1, "wgrad_to op0 x16 private": 1},
        "R3": "R2",
        "R4": "R2",
    },
    ('S2', 2, (8, 8, 16)): {
        "R0": {"conv op0 dgrad": 2, "conv op0 fwd": 1, "conv op0 fwd stats": 1, "in_bwd": 2, "norm_act_add": 1, "wgrad op0 private": 2},
        "R1": {"conv op0 dgrad": 1, "conv op0 dgrad stats nb": 1, "conv op0 fwd": 1, "conv op0 fwd stats": 1, "in_bwd": 1, "in_bwd_apply": 1,
               "norm_act_add": 1, "wgrad op0 private": 2},
        "R2": {"conv op0 dgrad": 1, "conv op0 dgrad stats nb": 1, "conv op0 fwd": 1, "conv op0 fwd stats": 1, "in_bwd": 1, "in_bwd_apply": 1,
               "norm_act_add": 1, "wgrad_to op0 private": 2},
        "R3": "R2",
        "R4": "R2",
    },
    ('S3', 1, (34, 38, 50)): {
        "R0": {"add": 1, "conv op0 dgrad": 2, "conv op0 dgrad residual": 1, "conv op0 fwd": 1, "conv op0 fwd residual": 1, "conv op0 fwd stats": 1,
               "in_bwd": 1, "wgrad op0 private": 3},
        "R1": {"add": 1, "conv op0 dgrad": 1, "conv op0 dgrad residual x16": 1, "conv op0 dgrad stats nb": 1, "conv op0 fwd": 1,
               "conv op0 fwd residual": 1, "conv op0 fwd stats": 1, "in_bwd_apply16 want_dx16 f32": 1, "wgrad op0 private": 3},
        "R2": {"add": 1, "conv op0 dgrad": 1, "conv op0 dgrad residual x16": 1, "conv op0 dgrad stats nb": 1, "conv op0 fwd": 1,
               "conv op0 fwd residual": 1, "conv op0 fwd stats": 1, "in_bwd_apply16 want_dx16 want_xa16 f32": 1, "to_bf16": 4,
               "wgrad_to op0 dy16 private": 1, "wgrad_to op0 private": 1, "wgrad_to op0 x16 private": 1},
        "R3": {"add": 1, "conv op0 dgrad": 1, "conv op0 dgrad residual x16": 1, "conv op0 dgrad stats nb": 1, "conv op0 fwd": 1,
               "conv op0 fwd residual": 1, "conv op0 fwd stats": 1, "in_bwd_apply16 want_dx16 want_xa16 no_f32": 1, "to_bf16": 4,
               "wgrad_to op0 dy16 private": 1, "wgrad_to op0 private": 1, "wgrad_to op0 x16 private": 1},
        "R4": "R3",
    },
    ('S3', 2, (8, 8, 16)): {
        "R0": {"add": 1, "conv op0 dgrad": 2, "conv op0 dgrad residual": 1, "conv op0 fwd": 1, "conv op0 fwd residual": 1, "conv op0 fwd stats": 1,
               "in_bwd": 1, "wgrad op0 private": 3},
        "R1": {"add": 1, "conv op0 dgrad": 1, "conv op0 dgrad residual": 1, "conv op0 dgrad stats nb": 1, "conv op0 fwd": 1,
               "conv op0 fwd residual": 1, "conv op0 fwd stats": 1, "in_bwd_apply": 1, "wgrad op0 private": 3},
        "R2": {"add": 1, "conv op0 dgrad": 1, "conv op0 dgrad residual": 1, "conv op0 dgrad stats nb": 1, "conv op0 fwd": 1,
               "conv op0 fwd residual": 1, "conv op0 fwd stats": 1, "in_bwd_apply": 1, "wgrad_to op0 private": 3},
        "R3": "R2",
        "R4": "R2",
    },
    ('S4', 1, (34, 38, 50)): {
        "R0": {"conv op0 dgrad": 2, "conv op0 fwd": 3, "wgrad op0 private": 2},
        "R1": "R0",
        "R2": {"conv op0 dgrad": 2, "conv op0 fwd": 3, "to_bf16": 4, "wgrad_to op0 private": 2},
        "R3": "R2",
        "R4": "R2",
    },
    ('S4', 2, (8, 8, 16)): {
        "R0": {"conv op0 dgrad": 2, "conv op0 fwd": 3, "wgrad op0 private": 2},
        "R1": "R0",
        "R2": {"conv op0 dgrad": 2, "conv op0 fwd": 3, "wgrad_to op0 private": 2},
        "R3": "R2",
        "R4": "R2",
    },
    ('S5', 1, (34, 38, 50)): {
        "R0": {"conv op0 dgrad": 3, "conv op0 fwd": 1, "conv op0 fwd residual": 1, "conv op0 fwd stats": 1, "in_bwd": 1, "wgrad op0": 1,
               "wgrad op0 private": 2},
        "R1": {"conv op0 dgrad": 1, "conv op0 dgrad stats nb": 1, "conv op0 dgrad x16": 1, "conv op0 fwd": 1, "conv op0 fwd residual": 1,
               "conv op0 fwd stats": 1, "in_bwd_apply16 want_dx16 f32": 1, "wgrad op0": 1, "wgrad op0 private": 2},
        "R2": {"conv op0 dgrad": 1, "conv op0 dgrad stats nb": 1, "conv op0 dgrad x16": 1, "conv op0 fwd": 1, "conv op0 fwd residual": 1,
               "conv op0 fwd stats": 1, "in_bwd_apply16 want_dx16 want_xa16 f32": 1, "to_bf16": 4, "wgrad_to op0 dy16 private": 1,
               "wgrad_to op0 private": 1, "wgrad_to op0 x16": 1},
        "R3": {"conv op0 dgrad": 1, "conv op0 dgrad stats nb": 1, "conv op0 dgrad x16": 1, "conv op0 fwd": 1, "conv op0 fwd residual": 1,
               "conv op0 fwd stats": 1, "in_bwd_apply16 want_dx16 want_xa16 no_f32": 1, "to_bf16": 4, "wgrad_to op0 dy16 private": 1,
               "wgrad_to op0 private": 1, "wgrad_to op0 x16": 1},
        "R4": "R3",
    },
    ('S5', 2, (8, 8, 16)): {
        "R0": {"conv op0 dgrad": 3, "conv op0 fwd": 1, "conv op0 fwd residual": 1, "conv op0 fwd stats": 1, "in_bwd": 1, "wgrad op0": 1,
               "wgrad op0 private": 2},
        "R1": {"conv op0 dgrad": 2, "conv op0 dgrad stats nb": 1, "conv op0 fwd": 1, "conv op0 fwd residual": 1, "conv op0 fwd stats": 1,
               "in_bwd_apply": 1, "wgrad op0": 1, "wgrad op0 private": 2},
        "R2": {"conv op0 dgrad": 2, "conv op0 dgrad stats nb": 1, "conv op0 fwd": 1, "conv op0 fwd residual": 1, "conv op0 fwd stats": 1,
               "in_bwd_apply": 1, "wgrad_to op0": 1, "wgrad_to op0 private": 2},
        "R3": "R2",
        "R4": "R2",
    },
    ('S6', 1, (34, 38, 50)): {
        "R0": {"conv op0 dgrad": 2, "conv op0 fwd": 1, "conv op0 fwd stats": 1, "in_bwd": 1, "wgrad op0": 2},
        "R1": {"conv op0 dgrad stats nb": 1, "conv op0 dgrad x16": 1, "conv op0 fwd": 1, "conv op0 fwd stats": 1, "in_bwd_apply16 want_dx16 f32": 1,
               "wgrad op0": 2},
        "R2": "R1",
        "R3": "R1",
        "R4": "R1",
    },
    ('S6', 2, (8, 8, 16)): {
        "R0": {"conv op0 dgrad": 2, "conv op0 fwd": 1, "conv op0 fwd stats": 1, "in_bwd": 1, "wgrad op0": 2},
        "R1": {"conv op0 dgrad": 1, "conv op0 dgrad stats nb": 1, "conv op0 fwd": 1, "conv op0 fwd stats": 1, "in_bwd_apply": 1, "wgrad op0": 2},
        "R2": "R1",
        "R3": "R1",
        "R4": "R1",
    },
    ('S7', 1, (34, 38, 50)): {
        "R0": {"conv op0 dgrad": 3, "conv op0 fwd": 1, "conv op0 fwd stats": 3, "in_bwd": 3, "wgrad op0 private": 3},
        "R1": {"conv op0 dgrad stats nb": 1, "conv op0 dgrad stats nb x16": 2, "conv op0 fwd": 1, "conv op0 fwd stats": 3,
               "in_bwd_apply16 want_dx16 f32": 3, "wgrad op0 private": 3},
        "R2": {"conv op0 dgrad stats nb": 1, "conv op0 dgrad stats nb x16": 2, "conv op0 fwd": 1, "conv op0 fwd stats": 3,
               "in_bwd_apply16 want_dx16 f32": 2, "in_bwd_apply16 want_dx16 want_xa16 f32": 1, "to_bf16": 2, "wgrad op0 private": 1,
               "wgrad_to op0 dy16 private": 1, "wgrad_to op0 x16 private": 1},
        "R3": {"conv op0 dgrad stats nb": 1, "conv op0 dgrad stats nb x16": 2, "conv op0 fwd": 1, "conv op0 fwd stats": 3,
               "in_bwd_apply16 want_dx16 f32": 2, "in_bwd_apply16 want_dx16 want_xa16 no_f32": 1, "to_bf16": 2, "wgrad op0 private": 1,
               "wgrad_to op0 dy16 private": 1, "wgrad_to op0 x16 private": 1},
        "R4": "R3",
    },
    ('S7', 2, (8, 8, 16)): {
        "R0": {"conv op0 dgrad": 3, "conv op0 fwd": 1, "conv op0 fwd stats": 3, "in_bwd": 3, "wgrad op0 private": 3},
        "R1": {"conv op0 dgrad stats nb": 3, "conv op0 fwd": 1, "conv op0 fwd stats": 3, "in_bwd_apply": 3, "wgrad op0 private": 3},
        "R2": {"conv op0 dgrad stats nb": 3, "conv op0 fwd": 1, "conv op0 fwd stats": 3, "in_bwd_apply": 3, "wgrad op0 private": 1,
               "wgrad_to op0 private": 2},
        "R3": "R2",
        "R4": "R2",
    },
    ('S8', 1, (34, 38, 50)): {
        "R0": {"channel_scale": 1, "conv op0 dgrad": 3, "conv op0 fwd": 1, "conv op0 fwd out_scale stats": 1, "conv op0 fwd stats": 1, "in_bwd": 2,
               "wgrad op0 private": 3},
        "R1": {"channel_scale": 1, "conv op0 dgrad stats nb": 2, "conv op0 dgrad x16": 1, "conv op0 fwd": 1, "conv op0 fwd out_scale stats": 1,
               "conv op0 fwd stats": 1, "in_bwd_apply": 1, "in_bwd_apply16 want_dx16 f32": 1, "wgrad op0 private": 3},
        "R2": {"channel_scale": 1, "conv op0 dgrad stats nb": 2, "conv op0 dgrad x16": 1, "conv op0 fwd": 1, "conv op0 fwd out_scale stats": 1,
               "conv op0 fwd stats": 1, "in_bwd_apply16 want_dx16 f32": 1, "in_bwd_apply16 want_xa16 f32": 1, "to_bf16": 3, "to_bf16 prologue": 1,
               "wgrad_to op0 dy16 private": 1, "wgrad_to op0 private": 1, "wgrad_to op0 x16 private": 1},
        "R3": {"channel_scale": 1, "conv op0 dgrad stats nb": 2, "conv op0 dgrad x16": 1, "conv op0 fwd": 1, "conv op0 fwd out_scale stats": 1,
               "conv op0 fwd stats": 1, "in_bwd_apply16 want_dx16 no_f32": 1, "in_bwd_apply16 want_xa16 f32": 1, "to_bf16": 3,
               "to_bf16 prologue": 1, "wgrad_to op0 dy16 private": 1, "wgrad_to op0 private": 1, "wgrad_to op0 x16 private": 1},
        "R4": "R3",
    },
    ('S8', 2, (8, 8, 16)): {
        "R0": {"channel_scale": 1, "conv op0 dgrad": 3, "conv op0 fwd": 1, "conv op0 fwd out_scale stats": 1, "conv op0 fwd stats": 1, "in_bwd": 2,
               "wgrad op0 private": 3},
        "R1": {"channel_scale": 1, "conv op0 dgrad": 1, "conv op0 dgrad stats nb": 2, "conv op0 fwd": 1, "conv op0 fwd out_scale stats": 1,
               "conv op0 fwd stats": 1, "in_bwd_apply": 2, "wgrad op0 private": 3},
        "R2": {"channel_scale": 1, "conv op0 dgrad": 1, "conv op0 dgrad stats nb": 2, "conv op0 fwd": 1, "conv op0 fwd out_scale stats": 1,
               "conv op0 fwd stats": 1, "in_bwd_apply": 2, "wgrad_to op0 private": 3},
        "R3": "R2",
        "R4": "R2",
    },
    ('S9', 1, (34, 38, 50)): {
        "R0": {"conv op0 dgrad": 4, "conv op0 fwd": 1, "conv op0 fwd stats": 3, "in_bwd": 3, "wgrad op0 private": 4},
        "R1": {"conv op0 dgrad stats nb": 2, "conv op0 dgrad stats nb x16": 1, "conv op0 dgrad x16": 1, "conv op0 fwd": 1, "conv op0 fwd stats": 3,
               "in_bwd_apply16 want_dx16 f32": 3, "wgrad op0 private": 4},
        "R2": {"conv op0 dgrad stats nb": 2, "conv op0 dgrad stats nb x16": 1, "conv op0 dgrad x16": 1, "conv op0 fwd": 1, "conv op0 fwd stats": 3,
               "in_bwd_apply16 want_dx16 want_xa16 f32": 3, "to_bf16": 3, "wgrad_to op0 dy16 private": 1, "wgrad_to op0 x16 dy16 private": 1,
               "wgrad_to op0 x16 private": 2},
        "R3": {"conv op0 dgrad stats nb": 2, "conv op0 dgrad stats nb x16": 1, "conv op0 dgrad x16": 1, "conv op0 fwd": 1, "conv op0 fwd stats": 3,
               "in_bwd_apply16 want_dx16 want_xa16 f32": 2, "in_bwd_apply16 want_dx16 want_xa16 no_f32": 1, "to_bf16": 3,
               "wgrad_to op0 dy16 private": 1, "wgrad_to op0 x16 dy16 private": 1, "wgrad_to op0 x16 private": 2},
        "R4": "R3",
    },
    ('S9', 2, (8, 8, 16)): {
        "R0": {"conv op0 dgrad": 4, "conv op0 fwd": 1, "conv op0 fwd stats": 3, "in_bwd": 3, "wgrad op0 private": 4},
        "R1": {"conv op0 dgrad": 1, "conv op0 dgrad stats nb": 3, "conv op0 fwd": 1, "conv op0 fwd stats": 3, "in_bwd_apply": 3,
               "wgrad op0 private": 4},
        "R2": {"conv op0 dgrad": 1, "conv op0 dgrad stats nb": 3, "conv op0 fwd": 1, "conv op0 fwd stats": 3, "in_bwd_apply": 3,
               "wgrad_to op0 private": 4},
        "R3": "R2",
        "R4": "R2",
    },
    ('S10', 1, (34, 38, 50)): {
        "R0": {"conv op0 dgrad": 2, "conv op0 fwd": 1, "conv op0 fwd stats": 1, "in_bwd": 1, "norm_act_add residual": 1, "wgrad op0 private": 2},
        "R1": {"conv op0 dgrad": 1, "conv op0 dgrad stats nb": 1, "conv op0 fwd": 1, "conv op0 fwd stats": 1, "in_bwd": 1,
               "norm_act_add residual": 1, "wgrad op0 private": 2},
        "R2": {"conv op0 dgrad": 1, "conv op0 dgrad stats nb": 1, "conv op0 fwd": 1, "conv op0 fwd stats": 1, "in_bwd": 1,
               "norm_act_add residual": 1, "to_bf16": 4, "wgrad_to op0 private": 2},
        "R3": "R2",
        "R4": "R2",
    },
    ('S10', 2, (8, 8, 16)): {
        "R0": {"conv op0 dgrad": 2, "conv op0 fwd": 1, "conv op0 fwd stats": 1, "in_bwd": 1, "norm_act_add residual": 1, "wgrad op0 private": 2},
        "R1": {"conv op0 dgrad": 1, "conv op0 dgrad stats nb": 1, "conv op0 fwd": 1, "conv op0 fwd stats": 1, "in_bwd": 1,
               "norm_act_add residual": 1, "wgrad op0 private": 2},
        "R2": {"conv op0 dgrad": 1, "conv op0 dgrad stats nb": 1, "conv op0 fwd": 1, "conv op0 fwd stats": 1, "in_bwd": 1,
               "norm_act_add residual": 1, "wgrad_to op0 private": 2},
        "R3": "R2",
        "R4": "R2",
    },
}
CENSUS = {k: (CENSUS[v] if isinstance(v, tuple) else v) for k, v in CENSUS.items()}
CENSUS = {k: {r: (v[t] if isinstance(t, str) else t) for r, t in v.items()} for k, v in CENSUS.items()}


# ====================================================================================================================
# one case, all routes
# ====================================================================================================================
def _route_env(hip, kernels, CF, route):
    """(sink wanted, scg factory) of a route, with its globals set: the caller restores them"""
    if route == "R0":
        kernels.set_precision("fp32")
    else:
        kernels.set_precision(BENCH["mode"], wgrad=BENCH["wgrad"], dgrad=BENCH["dgrad"])
    inside = route in ("R3", "R4")
    kernels.POISON_UNWRITTEN_CARRIERS = inside
    hip.wgrad_async = route == "R4"
    return route in ("R2", "R3", "R4"), (CF.single_consumer_graph if inside else contextlib.nullcontext)


def run_case(hip, monkeypatch, name, n, size, log=print):
    """every route of one (graph, shape); returns ({route: census}, [failure messages], [(run, worst err / bound, its tensor)],
    {run: {tensor: (error, bound)}}).  Prints the measured yardsticks and every run's worst ratio through `log`."""
    from cwf import functional as CF, kernels
    from cwf.optim import GradSink
    ref = B.reference(name, n, size)
    old_units = hip.lib.cwf_debug_ws_min_units(1) if name == "U2" else None        # the small 32- / 64-channel layers reach conv_ws's image launch
    poison0, async0 = kernels.POISON_UNWRITTEN_CARRIERS, hip.wgrad_async
    prec0 = (kernels._PRECISION, kernels._WGRAD_PRECISION, kernels._DGRAD_PRECISION)
    census, fails, runs, table, allrows = {}, [], {}, [], {}
    live = [k for k in ref.e32 if k not in ref.zero and k not in B.GRAPHS[name].no_grad]
    zero = sorted(ref.zero)
    log("%-4s %-10s yardsticks (largest over tensors): e32 %.2e  flips ek %.2e (%.3f expected per pass, %d allowed for)  e16 %.2e%s"
        % (name, "%dx%dx%dx%d" % (n, *size), max(ref.e32[k] for k in live), max(ref.ek[k] for k in live), ref.kink_lam, ref.kink_flips,
           max(ref.e16[k] for k in live), ";  true zeros: e32 %.2e  e16 %.2e" % (max(ref.e32[k] for k in zero), max(ref.e16[k] for k in zero))
           if zero else ""))
    try:
        mods, packer = B.build(name, DEV)
        sink = GradSink([p for p in mods.parameters() if p.requires_grad])
        I = {k: v.to(DEV) for k, v in B.make_inputs(name, n, size).items()}
        q = [t.to(DEV) for t in ref.q]
        double = [1.0] + [2.0] * (len(q) - 1) if len(q) > 1 else None

        def go(route, tag, scales=None):
            use_sink, scg = _route_env(hip, kernels, CF, route)

            def after():
                hip.wgrad_async = False
                hip.join_wgrad_stream()
                hip.wgrad_flush()
                torch.cuda.synchronize()
            with B.record_links() as seen, _spy(hip, monkeypatch) as cen:
                run = B.run_device(name, mods, packer, I, q, hip, sink=sink if use_sink else None, scg=scg, scales=scales, after_backward=after)
            B.assert_links_clean(seen, (name, tag))
            assert not hip._wg_pending, (name, tag)
            rows, bad = B.compare(run, ref, route != "R0", scales, (name, tag))
            worst = max(((e / b if b > 0 else (0.0 if e == 0 else float("inf"))), k) for k, (e, b) in rows.items())
            log("%-4s %-10s %-9s worst err/bound %.3f at %s" % (name, "%dx%dx%dx%d" % (n, *size), tag, worst[0], worst[1]))
            for k, e, b in bad:
                fails.append("%s: %s err %.3e > bound %.3e (e32 %.3e, kink %.3e, e16 %.3e)" % (tag, k, e, b, ref.e32[k], ref.ek[k], ref.e16[k]))
            table.append((tag, worst[0], worst[1]))
            allrows[tag] = rows
            runs[tag] = run
            if scales is None and route not in census:
                census[route] = dict(cen)
            return run

        # R3 -> R1 -> R3 in one process, then the rest; R1 twice for the run-to-run noise
        for route, tag in (("R3", "R3"), ("R1", "R1"), ("R3", "R3again"), ("R0", "R0"), ("R1", "R1again"), ("R2", "R2"), ("R4", "R4")):
            go(route, tag)
        if double:
            for route in ("R1", "R3"):
                go(route, route + "x2", double)

        def equal(a, b, what, noise_of=None):
            """relative L2 of every tensor of run a from run b < max(5e-5, 10 x noise) (tests/test_model_gpu.py); true zeros are
            cancellation noise whose summation order differs between routes: they are held to the float64 bound above only"""
            for k in ["out%d" % i for i in range(len(b.out))] + [k for k in ref.names if k not in ref.zero and k not in B.GRAPHS[name].no_grad]:
                ta, tb = (a.out[int(k[3:])], b.out[int(k[3:])]) if k.startswith("out") else (a.grad[k], b.grad[k])
                d = B._rel(ta, tb)
                if noise_of is None:
                    yield k, d
                elif not d < max(5e-5, 10 * noise_of[k]):
                    fails.append("%s: %s differs by %.3e (noise %.3e)" % (what, k, d, noise_of[k]))
        noise = dict(equal(runs["R1again"], runs["R1"], "noise"))
        for tag in ("R2", "R3", "R4"):
            list(equal(runs[tag], runs["R1"], "%s vs R1" % tag, noise))
        list(equal(runs["R3again"], runs["R3"], "R3 after R1 vs R3", noise))
        if double:
            list(equal(runs["R3x2"], runs["R1x2"], "R3 vs R1, consumer doubled", noise))
        log("%-4s %-10s noise (R1 twice) worst %.3e" % (name, "%dx%dx%dx%d" % (n, *size), max(noise.values())))
    finally:
        kernels.set_precision(prec0[0], wgrad=prec0[1], dgrad=prec0[2])
        kernels.POISON_UNWRITTEN_CARRIERS = poison0
        hip.wgrad_async = async0
        hip.join_wgrad_stream()
        if old_units is not None:
            hip.lib.cwf_debug_ws_min_units(old_units)
    return census, fails, table, allrows


@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_block_graph_routes(hip, monkeypatch, case):
    name, n, size = case
    census, fails, _, _ = run_case(hip, monkeypatch, name, n, size, log=lambda s: print("\n" + s, end=""))
    for route in ROUTES:
        _check_route_facts(name, n, size, route, census[route])
    want = CENSUS[case]
    for route in ROUTES:
        assert census[route] == want[route], (case, route, "census", sorted(set(census[route].items()) ^ set(want[route].items())))
    assert not fails, (case, fails)
