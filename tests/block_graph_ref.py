"""Block graphs for the conv autograd glue (cwf/functional.py) and their float64 references (a helper module for the tests, not a test file).

Every graph is stated twice:
  device(ctx)   assembles the project's own modules (InitConv, EnBlock, EnDown, EnBlock2 / DeBlock, DeUp_Cat, HipConv) and calls
                CF.conv / CF.norm_act_add directly for the stand-alone cases; activations [N, D, H, W, C];
  ref(ops, P, I) the same graph in plain torch (NCDHW) over an `ops` object that owns the convolutions, so that ONE statement serves
                three references:
                  Ops          F.conv3d / F.conv_transpose3d in the dtype of its operands: float64 = the truth, float32 = the yardstick e32;
                  RoundedOps   float64 with the operands rounded where the bench-precision kernels round them (the yardstick e16).
Both return the list of the graph's loss consumers [out, alias, ...]; the loss is sum_k sum(consumer_k * q_k) with seeded q_k.  A q of a
consumer that lies upstream of consumer 0 (an alias with a second use) is scaled so that both of its gradients are of one size, as
tests/test_gradient_sink_gpu.py does.

What RoundedOps rounds (tests/bf16_operand_ref.py lists the kernels' rules; precision "bf16x3", wgrad "bf16", dgrad "bf16"):
  forward           split-bf16 products hi(a) hi(b) + hi(a) lo(b) + lo(a) hi(b) of the activated input a and the weight b;
  data gradient     hi(dy) * hi(w)                                  (every layer);
  weight gradient   hi(a) * hi(dy), or exact products where bf16_operand_ref.wgrad_operand_mode says "fp32" (pw_wgrad_kernel);
  bias gradient     sum hi(dy) where the weight gradient takes bf16 operands (its bias slot is ones . hi(dy)), the exact sum of dy for
                    the pw_wgrad_kernel layers and for every ConvTranspose (a channel sum of the fp32 tensor).
InstanceNorm, the activations, the residual additions and the softmax stay exact: the kernels compute them in fp32, which e32 measures.
"""
from __future__ import annotations

import contextlib
import functools
import math

import torch
import torch.nn as nn
import torch.nn.functional as F

import bf16_operand_ref as R
from oracle import reference_model as rm

IN_EPS = rm.IN_EPS
KINK_M = 1024.0
# the flip count allowed for is exceeded in 5 % of all runs of the 25 GPU cases together: 0.2 % per case (an expected count below 0.002 -- every
# 16-channel graph at 2 x 8 x 8 x 16 -- allows no flip at all)
KINK_Q = 1.0 - 0.05 / 25


# ====================================================================================================================
# reference side
# ====================================================================================================================
def _inorm(x):
    return F.instance_norm(x, eps=IN_EPS)


def _plain_conv(kind, x, w, b):
    if kind == "c3":
        return F.conv3d(x, w, b, padding=1)
    if kind == "c3s2":
        return F.conv3d(x, w, b, stride=2, padding=1)
    if kind == "c1":
        return F.conv3d(x, w, b)
    if kind == "ct":
        return F.conv_transpose3d(x, w, b, stride=2)
    raise ValueError(kind)


_OP_OF = {"c3": R.CONV3_S1, "c3s2": R.CONV3_S2, "c1": R.CONV1, "ct": R.CONVT2}


class Ops:
    """the convolutions of a reference graph; records every conv output (in call order, under the layer's name) so that the caller can
    ask autograd for dL/d(output) of each layer"""

    def __init__(self):
        self.outs = []          # (layer name, output tensor)
        self.pre = []           # normalised pre-activations IN(x), one per activation site, in call order

    def _conv(self, kind, x, w, b):
        return _plain_conv(kind, x, w, b)

    def act(self, x, slope):
        """act(IN(x)): ReLU (slope 0) or LeakyReLU"""
        n = _inorm(x)
        self.pre.append(n.detach())
        return self._act(n, slope, len(self.pre) - 1)

    def _act(self, n, slope, site):
        return F.relu(n) if slope == 0.0 else F.leaky_relu(n, slope)

    def conv(self, P, name, x, kind="c3"):
        y = self._conv(kind, x, P[name + ".weight"], P[name + ".bias"])
        self.outs.append((name, y))
        return y


class _RoundedConv(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, b, kind):
        ctx.kind = kind
        ctx.save_for_backward(x, w)
        xh, wh = R.hi(x), R.hi(w)
        xl, wl = R.hi(x - xh), R.hi(w - wh)
        return _plain_conv(kind, xh, wh + wl, b) + _plain_conv(kind, xl, wh, None)

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        kind = ctx.kind
        gh = R.hi(dy)
        cin, cout = (w.shape[0], w.shape[1]) if kind == "ct" else (w.shape[1], w.shape[0])
        mode = R.wgrad_operand_mode(_OP_OF[kind], cin, cout, tuple(x.shape[2:]), "bf16")
        with torch.enable_grad():
            xin = x.detach().requires_grad_(True)
            (dx,) = torch.autograd.grad(_plain_conv(kind, xin, R.hi(w), None), xin, gh)
            wz = w.detach().requires_grad_(True)
            xa, g = (R.hi(x), gh) if mode == "bf16" else (x.detach(), dy)
            (dw,) = torch.autograd.grad(_plain_conv(kind, xa, wz, None), wz, g)
        # the bias slot of the bf16 weight-gradient kernels is ones . dy with the bf16 operand (sum hi(dy)); pw_wgrad_kernel adds the fp32
        # values, and a ConvTranspose layer's bias gradient is a channel sum of the fp32 dy in every mode (functional.py: no bias slot)
        return dx, dw, (gh if (mode == "bf16" and kind != "ct") else dy).sum((0, 2, 3, 4)), None


class RoundedOps(Ops):
    def _conv(self, kind, x, w, b):
        assert x.dtype == torch.float64
        return _RoundedConv.apply(x, w, b, kind)


class _KinkAct(torch.autograd.Function):
    @staticmethod
    def forward(ctx, n, slope, shifted):
        ctx.slope = slope
        ctx.save_for_backward(shifted)
        return torch.where(n > 0, n, n * slope)

    @staticmethod
    def backward(ctx, d):
        (shifted,) = ctx.saved_tensors
        return d * torch.where(shifted > 0, torch.ones_like(d), torch.full_like(d, ctx.slope)), None, None


class MaskedOps(Ops):
    """the activations' DERIVATIVE taken on the branch the given pre-activations choose (those of the float64 run): the float32 run with
    the truth's activation pattern, i.e. its summation error without its own draw of branch flips.  The forward values are its own."""

    def __init__(self, pre):
        super().__init__()
        self.mask_from = pre

    def _act(self, n, slope, site):
        return _KinkAct.apply(n, slope, self.mask_from[site].to(n.dtype))


class KinkOps(Ops):
    """float64, with the activations' DERIVATIVE taken at IN(x) + tau * xi, xi = +-1 seeded per element, tau >= 0 per element (one tensor
    per activation site): an element within its tau of the kink takes the other branch with probability 1/2 -- what another realisation
    with pre-activation errors of that size does.  The forward values are exact."""

    def __init__(self, taus):
        super().__init__()
        self.taus = taus
        self.flips = 0          # elements whose derivative was taken on the other branch

    def _act(self, n, slope, site):
        gen = torch.Generator().manual_seed(4000 + site)
        xi = torch.randint(0, 2, n.shape, generator=gen).double() * 2 - 1
        shifted = n.detach() + self.taus[site] * xi
        self.flips += int(((shifted > 0) != (n.detach() > 0)).sum())
        return _KinkAct.apply(n, slope, shifted)


def en_block(ops, P, pre, x):
    """IN -> ReLU -> conv -> IN -> ReLU -> conv -> + x  (oracle.reference_model.en_block)"""
    h = ops.conv(P, pre + ".conv1", ops.act(x, 0.0))
    h = ops.conv(P, pre + ".conv2", ops.act(h, 0.0))
    return h + x


def post_block(ops, P, pre, x):
    """conv -> IN -> LeakyReLU -> conv -> IN -> LeakyReLU -> + x  (oracle.reference_model.post_block)"""
    h = ops.act(ops.conv(P, pre + ".conv1", x), 0.01)
    h = ops.act(ops.conv(P, pre + ".conv2", h), 0.01)
    return h + x


def de_up_cat(ops, P, pre, x, prev):
    """1x1x1 conv -> ConvTranspose k2 s2 -> concat(prev, y) -> 1x1x1 conv  (oracle.reference_model.de_up_cat)"""
    t = ops.conv(P, pre + ".conv1", x, "c1")
    u = ops.conv(P, pre + ".conv2", t, "ct")
    return ops.conv(P, pre + ".conv3", torch.cat((prev, u), 1), "c1")


def _lk(ops, x):
    return ops.act(x, 0.01)


# ====================================================================================================================
# device side helpers
# ====================================================================================================================
class Ctx:
    """what a graph's device statement gets: the modules `m` (a ModuleDict of the project's modules), the inputs `I` (dict of device
    tensors, NDHWC), the kernel backend `K` and `scg`, a context-manager factory: functional.single_consumer_graph where the route
    declares it, a null context otherwise"""

    def __init__(self, m, I, K, scg):
        self.m, self.I, self.K, self.scg = m, I, K, scg


def _stats_of(K, t):
    """(scale, shift) of a tensor no conv epilogue produced statistics for (an input, a block tail)"""
    t = t.detach()
    return K.in_finalize(K.in_stats(t), t.shape[1] * t.shape[2] * t.shape[3])


def _mods(**kw):
    return nn.ModuleDict(kw)


def _hc(cin, cout, **kw):
    from models.clswiseformer.layers import HipConv
    return HipConv(cin, cout, **kw)


# ====================================================================================================================
# the catalogue
# ====================================================================================================================
class Graph:
    """name; cin = channels of the input x; x_grad = x is a leaf that wants its gradient; frozen = parameter names without gradient;
    no_grad = parameters the graph never reaches (their gradient is None / zero); keep = channels of a seeded [n, keep] scale input"""
    cin, x_grad, frozen, no_grad, keep, down = 16, True, (), (), 0, 1

    def modules(self):
        raise NotImplementedError

    def device(self, c: Ctx):
        raise NotImplementedError

    def ref(self, ops, P, I):
        raise NotImplementedError


def _keep_mask(n, c, zero):
    """[n, c] channel scales with two different non-zero values (and, with `zero`, a zero channel: another one in each sample)"""
    k = torch.full((n, c), 1.25)
    for i in range(n):
        k[i, (5 + 3 * i) % c] = 2.0
        k[i, (9 + i) % c] = 0.5
        if zero:
            k[i, (3 + 4 * i) % c] = 0.0
    return k


class U1(Graph):
    """one-level U, 16 / 32 channels: stem with a keep mask -> EnBlock -> EnBlock(skip buffer) -> EnDown(carry) -> EnBlock -> DeUp_Cat onto
    the prefilled skip -> DeBlock(emit16) -> DeBlock -> 1x1x1 16 -> 4 -> channel softmax"""
    cin, x_grad, keep, keep_zero = 4, False, 16, True

    def modules(self):
        from models.clswiseformer.Unet_skipconnection import EnBlock, EnDown, InitConv
        from models.clswiseformer.cls_wise_former import DeBlock, DeUp_Cat
        return _mods(stem=InitConv(4, 16, dropout=0.0), eb1=EnBlock(16), eb2=EnBlock(16), down=EnDown(16, 32), eb3=EnBlock(32),
                     up=DeUp_Cat(32, 16), db1=DeBlock(16), db2=DeBlock(16), end=_hc(16, 4, k=1))

    def device(self, c):
        from cwf import functional as CF
        m = c.m
        with c.scg():
            y, s = m["stem"](c.I["x"], c.I["keep"])
            y, s = m["eb1"](y, s)
            x1, _ = m["eb2"](y, s, want_stats=False, skip_cb=16)
            y, s, x1 = m["down"](x1, carry=True)
            y, _ = m["eb3"](y, s, want_stats=False)
            y = m["up"](y, x1)
            y = m["db2"](m["db1"](y, emit16=True))
            logits, _ = m["end"](y)
            return [CF.channel_softmax(logits)]

    def ref(self, ops, P, I):
        y = ops.conv(P, "stem.conv", I["x"]) * I["keep"][:, :, None, None, None]
        x1 = en_block(ops, P, "eb2", en_block(ops, P, "eb1", y))
        y = en_block(ops, P, "eb3", ops.conv(P, "down.conv", x1, "c3s2"))
        y = de_up_cat(ops, P, "up", y, x1)
        y = post_block(ops, P, "db2", post_block(ops, P, "db1", y))
        return [torch.softmax(ops.conv(P, "end", y, "c1"), 1)]


class U2(Graph):
    """deep level, 32 / 64 channels: EnBlock -> EnDown(carry) -> EnBlock -> EnBlock -> DeUp_Cat with a plain `prev` (cat_buffer, _CatIntoFn)
    -> DeBlock(emit16) -> DeBlock"""
    cin = 32

    def modules(self):
        from models.clswiseformer.Unet_skipconnection import EnBlock, EnDown
        from models.clswiseformer.cls_wise_former import DeBlock, DeUp_Cat
        return _mods(eb1=EnBlock(32), down=EnDown(32, 64), eb2=EnBlock(64), eb3=EnBlock(64), up=DeUp_Cat(64, 32), db1=DeBlock(32), db2=DeBlock(32))

    def device(self, c):
        m = c.m
        with c.scg():
            x = c.I["x"]
            y, _ = m["eb1"](x, _stats_of(c.K, x), want_stats=False)
            y, s, skip = m["down"](y, carry=True)
            y, s = m["eb2"](y, s)
            y, _ = m["eb3"](y, s, want_stats=False)
            y = m["up"](y, skip)
            return [m["db2"](m["db1"](y, emit16=True))]

    def ref(self, ops, P, I):
        skip = en_block(ops, P, "eb1", I["x"])
        y = ops.conv(P, "down.conv", skip, "c3s2")
        y = en_block(ops, P, "eb3", en_block(ops, P, "eb2", y))
        y = de_up_cat(ops, P, "up", y, skip)
        return [post_block(ops, P, "db2", post_block(ops, P, "db1", y))]


class S1(Graph):
    """a block tail act(IN(g)) + x with TWO conv consumers: link.shared, the tail keeps its own reduction"""

    def modules(self):
        return _mods(c0=_hc(16, 16), cB=_hc(16, 16), cC=_hc(16, 16))

    def device(self, c):
        from cwf import functional as CF
        m, x = c.m, c.I["x"]
        with c.scg():
            g, st = m["c0"](x, want_stats=True)
            y = CF.norm_act_add(g, st, 0.01, residual=x)
            return [m["cB"](y)[0], m["cC"](y)[0]]

    def ref(self, ops, P, I):
        y = _lk(ops, ops.conv(P, "c0", I["x"])) + I["x"]
        return [ops.conv(P, "cB", y), ops.conv(P, "cC", y)]


class S2(Graph):
    """a block tail whose single consumer normalises (in_norm given): the tail is shared as well"""

    def modules(self):
        return _mods(c0=_hc(16, 16), cB=_hc(16, 16))

    def device(self, c):
        from cwf import functional as CF
        m = c.m
        with c.scg():
            g, st = m["c0"](c.I["x"], want_stats=True)
            y = CF.norm_act_add(g, st, 0.01)
            return [m["cB"](y, in_norm=_stats_of(c.K, y), slope=0.0)[0]]

    def ref(self, ops, P, I):
        return [ops.conv(P, "cB", ops.act(_lk(ops, ops.conv(P, "c0", I["x"])), 0.0))]


class S3(Graph):
    """a carried alias with a link consumer (a residual) plus an autograd consumer: the K.add in _ConvFn.backward"""

    def modules(self):
        return _mods(c0=_hc(16, 16), c1=_hc(16, 16), c2=_hc(16, 16))

    def device(self, c):
        m = c.m
        with c.scg():
            x0, _ = m["c0"](c.I["x"])
            h, hs, xc = m["c1"](x0, want_stats=True, carry=True)
            z, _ = m["c2"](h, in_norm=hs, slope=0.01, residual=xc)
            return [z, xc]

    def ref(self, ops, P, I):
        x0 = ops.conv(P, "c0", I["x"])
        return [ops.conv(P, "c2", _lk(ops, ops.conv(P, "c1", x0))) + x0, x0]


class S4(Graph):
    """a conv whose y is unused while its carried alias is used: dy is None"""
    no_grad = ("c1.weight", "c1.bias")

    def modules(self):
        return _mods(c0=_hc(16, 16), c1=_hc(16, 16), c2=_hc(16, 16))

    def device(self, c):
        m = c.m
        with c.scg():
            x0, _ = m["c0"](c.I["x"])
            _h, _, xc = m["c1"](x0, carry=True)
            return [m["c2"](xc)[0]]

    def ref(self, ops, P, I):
        return [ops.conv(P, "c2", ops.conv(P, "c0", I["x"]))]


class S5(Graph):
    """a residual that is a plain tensor (no res_link): dres returns through autograd"""

    def modules(self):
        return _mods(c0=_hc(16, 16), c1=_hc(16, 16), c2=_hc(16, 16))

    def device(self, c):
        m = c.m
        with c.scg():
            x0, _ = m["c0"](c.I["x"])
            h, hs = m["c1"](x0, want_stats=True)
            return [m["c2"](h, in_norm=hs, slope=0.01, residual=x0)[0]]

    def ref(self, ops, P, I):
        x0 = ops.conv(P, "c0", I["x"])
        return [ops.conv(P, "c2", _lk(ops, ops.conv(P, "c1", x0))) + x0]


class S6(Graph):
    """one weight applied twice (spec.uses == 2): no sink, no side stream for it"""

    def modules(self):
        return _mods(cA=_hc(16, 16))

    def device(self, c):
        m = c.m
        with c.scg():
            y, st = m["cA"](c.I["x"], want_stats=True)
            return [m["cA"](y, in_norm=st, slope=0.01)[0]]

    def ref(self, ops, P, I):
        return [ops.conv(P, "cA", _lk(ops, ops.conv(P, "cA", I["x"])))]


class S7(Graph):
    """a frozen weight (bias trained), a fully frozen layer, and an input that needs no gradient"""
    x_grad, frozen = False, ("cF.weight", "cG.weight", "cG.bias")

    def modules(self):
        return _mods(c0=_hc(16, 16), cF=_hc(16, 16), cG=_hc(16, 16), cB=_hc(16, 16))

    def device(self, c):
        m = c.m
        with c.scg():
            y, s = m["c0"](c.I["x"], want_stats=True)
            y, s = m["cF"](y, in_norm=s, slope=0.01, want_stats=True)
            y, s = m["cG"](y, in_norm=s, slope=0.01, want_stats=True)
            return [m["cB"](y, in_norm=s, slope=0.01)[0]]

    def ref(self, ops, P, I):
        y = ops.conv(P, "c0", I["x"])
        for name in ("cF", "cG", "cB"):
            y = ops.conv(P, name, _lk(ops, y))
        return [y]


class S8(Graph):
    """out_scale on a conv whose input does need a gradient: channel_scale, never the dy_scale fold"""
    keep, keep_zero = 16, False

    def modules(self):
        return _mods(c0=_hc(16, 16), cS=_hc(16, 16), cB=_hc(16, 16))

    def device(self, c):
        m = c.m
        with c.scg():
            y, s = m["c0"](c.I["x"], want_stats=True)
            y, s = m["cS"](y, in_norm=s, slope=0.01, out_scale=c.I["keep"], want_stats=True)
            return [m["cB"](y, in_norm=s, slope=0.01)[0]]

    def ref(self, ops, P, I):
        y = ops.conv(P, "cS", _lk(ops, ops.conv(P, "c0", I["x"]))) * I["keep"][:, :, None, None, None]
        return [ops.conv(P, "cB", _lk(ops, y))]


class S9(Graph):
    """a conv output with a second consumer, behind a chain that IS single-consumer: cP -> cQ are declared (single_consumer_graph, where
    the route declares at all), cA -> cB and the second consumer of cA's output are built outside the declaration"""

    def modules(self):
        return _mods(cP=_hc(16, 16), cQ=_hc(16, 16), cA=_hc(16, 16), cB=_hc(16, 16))

    def device(self, c):
        m = c.m
        with c.scg():
            h, s = m["cP"](c.I["x"], want_stats=True)
            h, s = m["cQ"](h, in_norm=s, slope=0.01, want_stats=True)
        y, sy = m["cA"](h, in_norm=s, slope=0.01, want_stats=True)
        return [m["cB"](y, in_norm=sy, slope=0.01)[0], y]

    def ref(self, ops, P, I):
        h = ops.conv(P, "cQ", _lk(ops, ops.conv(P, "cP", I["x"])))
        y = ops.conv(P, "cA", _lk(ops, h))
        return [ops.conv(P, "cB", _lk(ops, y)), y]


class S10(Graph):
    """a block tail with ONE conv consumer and a second consumer that is not a conv (the loss reads the tail's output): the conv's data
    gradient is not the tail's whole dL/dy, so the tail must not take its InstanceNorm-backward sums from that epilogue"""

    def modules(self):
        return _mods(c0=_hc(16, 16), cB=_hc(16, 16))

    def device(self, c):
        from cwf import functional as CF
        m, x = c.m, c.I["x"]
        g, st = m["c0"](x, want_stats=True)
        y = CF.norm_act_add(g, st, 0.01, residual=x)
        return [m["cB"](y)[0], y]

    def ref(self, ops, P, I):
        y = _lk(ops, ops.conv(P, "c0", I["x"])) + I["x"]
        return [ops.conv(P, "cB", y), y]


GRAPHS = {g.__name__: g() for g in (U1, U2, S1, S2, S3, S4, S5, S6, S7, S8, S9, S10)}
CPU_SHAPE = (2, (8, 6, 16))
S_SHAPES = [(1, (34, 38, 50)), (2, (8, 8, 16))]
GPU_SHAPES = {"U1": [(2, (32, 32, 32)), (1, (34, 38, 50)), (2, (16, 16, 32))], "U2": [(2, (8, 8, 32)), (1, (4, 12, 16))]}
for _g in GRAPHS:
    GPU_SHAPES.setdefault(_g, S_SHAPES)


# ====================================================================================================================
# seeded parameters and inputs
# ====================================================================================================================
def _rand(shape, gen, scale=1.0):
    return (torch.rand(*shape, generator=gen) * 2 - 1) * scale


@functools.lru_cache(maxsize=None)
def make_params(name):
    """{parameter name: float32 CPU tensor}, seeded: weights uniform in +-sqrt(3 / fan_in) (unit gain; fan_in of a ConvTranspose k2 s2: its
    input channels, one tap per output voxel), biases in +-0.1"""
    from cwf import packing as pk
    from models.clswiseformer.layers import HipConv
    gen = torch.Generator().manual_seed(1000 + sum(map(ord, name)))
    out = {}
    for mn, mod in GRAPHS[name].modules().named_modules():
        if isinstance(mod, HipConv):
            w = mod.weight
            fan = w.shape[0] if mod.spec.op == pk.CONVT2 else w[0].numel()
            out[mn + ".weight"] = _rand(w.shape, gen, math.sqrt(3.0 / fan))
            out[mn + ".bias"] = _rand(mod.bias.shape, gen, 0.1)
    return out


def build(name, device):
    """the project's modules of graph `name` with the seeded parameters on `device`, and their WeightPacker"""
    from cwf import functional as CF
    from models.clswiseformer.layers import collect_convs
    g = GRAPHS[name]
    mods = g.modules()
    with torch.no_grad():
        for pn, p in mods.named_parameters():
            p.copy_(make_params(name)[pn])
    mods = mods.to(device)
    for pn, p in mods.named_parameters():
        p.requires_grad_(pn not in g.frozen)
    packer = CF.WeightPacker()
    collect_convs(mods, packer)
    return mods, packer


def make_inputs(name, n, size):
    """{"x": [n, D, H, W, cin], "keep": [n, c]} float32 CPU tensors (NDHWC), seeded"""
    g = GRAPHS[name]
    gen = torch.Generator().manual_seed(2000 + sum(map(ord, name)) + n * 7 + size[0] * 11 + size[1] * 13 + size[2] * 17)
    I = {"x": _rand((n, *size, g.cin), gen)}
    if g.keep:
        I["keep"] = _keep_mask(n, g.keep, g.keep_zero)
    return I


def _ncdhw(t):
    return t.permute(0, 4, 1, 2, 3).contiguous() if t.dim() == 5 else t


def _ndhwc(t):
    return t.permute(0, 2, 3, 4, 1).contiguous() if t.dim() == 5 else t


# ====================================================================================================================
# running a reference
# ====================================================================================================================
def _run_ref(name, n, size, dtype, ops, qs, split):
    """forward + backward of the reference statement.  qs: consumer weights (NCDHW float64) or None (forward only).  split: one backward
    pass per consumer (the truth: gradients are linear in the q_k) instead of one for the sum.  Returns a dict:
       outs [NCDHW], grads[k] = {parameter name / "x": gradient}, dys[k] = [(layer name, dL/d(conv output) or None), ...], one k per pass"""
    g = GRAPHS[name]
    P = {k: v.to(dtype).clone().requires_grad_(k not in g.frozen) for k, v in make_params(name).items()}
    I = {k: _ncdhw(v).to(dtype) for k, v in make_inputs(name, n, size).items()}
    if g.x_grad:
        I["x"].requires_grad_(True)
    outs = g.ref(ops, P, I)
    res = dict(outs=[o.detach() for o in outs], grads=[], dys=[], pre=ops.pre)
    if qs is None:
        return res
    leaves = [(k, v) for k, v in P.items() if v.requires_grad] + ([("x", I["x"])] if g.x_grad else [])
    inner = [(k, v) for k, v in ops.outs if v.requires_grad]
    terms = [(o * q.to(dtype)).sum() for o, q in zip(outs, qs)]
    passes = terms if split else [sum(terms)]
    for i, t in enumerate(passes):
        gr = torch.autograd.grad(t, [v for _, v in leaves] + [v for _, v in inner], retain_graph=i + 1 < len(passes), allow_unused=True)
        res["grads"].append({k: (torch.zeros_like(v) if a is None else a.detach()) for (k, v), a in zip(leaves, gr[:len(leaves)])})
        res["dys"].append([(k, None if a is None else a.detach()) for (k, _), a in zip(inner, gr[len(leaves):])])
    return res


def _seeded_q(name, n, size, outs):
    gen = torch.Generator().manual_seed(3000 + sum(map(ord, name)) + n + sum(size))
    return [_rand(tuple(o.shape), gen).double() for o in outs]


class Reference:
    """everything the tests need of one (graph, n, size), computed once and never modified:
       q[k]            consumer weights, NDHWC float32 (q[k >= 1] scaled to the size of consumer 0's gradient where consumer k lies upstream)
       out[k]          float64 consumer values, NDHWC
       part[k][name]   float64 gradient of sum(consumer_k * q_k) alone; grad(scales) = sum_k scales[k] * part[k]  (exact: linear in q)
       dy_abs[name]    sum |dL/d(conv output)| of layer `name` (bias `name`.bias), for the sum of all consumers
       e32 / e16 / ek  per tensor ("out0", ..., parameter names, "x"): relative L2 distance from the truth of the float32 run (on the truth's
                       activation pattern) / the operand-rounded run / the expected activation-branch flips (see __init__); for a true-zero gradient
                       (below) the largest |element| over dy_abs of its layer instead
       zero            names of true-zero gradients: biases in front of an InstanceNorm, |ref| <= 1e-9 * dy_abs"""

    def __init__(self, name, n, size, rounded=True):
        self.name, self.n, self.size = name, n, size
        fwd = _run_ref(name, n, size, torch.float64, Ops(), None, False)
        q = _seeded_q(name, n, size, fwd["outs"])
        if len(q) > 1:
            # consumers upstream of consumer 0: match the size of the gradient consumer 0 sends them
            g = GRAPHS[name]
            P = {k: v.double().clone().requires_grad_(k not in g.frozen) for k, v in make_params(name).items()}
            I = {k: _ncdhw(v).double() for k, v in make_inputs(name, n, size).items()}
            if g.x_grad:
                I["x"].requires_grad_(True)
            outs = g.ref(Ops(), P, I)
            gs = torch.autograd.grad((outs[0] * q[0]).sum(), outs[1:], allow_unused=True)
            q = [q[0]] + [qk if gk is None else qk * float(gk.norm() / qk.norm()) for qk, gk in zip(q[1:], gs)]
        q = [t.float().double() for t in q]                  # (the device gets float32 weights: the truth uses the same values)
        t64 = _run_ref(name, n, size, torch.float64, Ops(), q, True)
        # The derivative of a (Leaky)ReLU net jumps where a pre-activation changes sign, and an fp32 realisation takes the other branch for
        # every element whose error exceeds its distance from zero: a Poisson number of elements, ONE of which is 10^-3 of its layer's
        # gradient at 10^6 elements.  A plain float32 run is one draw of that number (often none, and then says nothing about the next
        # realisation), so the two effects are measured apart:
        #   e32  the float32 run with the truth's activation pattern (MaskedOps): summation error alone; the issue's factor 16 applies;
        #   ek   the expected error of the flips, added ONCE.  tau = the float32 run's own pre-activation errors, element by element.  The
        #        probe (KinkOps) widens every tau by KINK_M, which multiplies the expected number of flips by KINK_M (a stable count):
        #        lam = flips / KINK_M is the expected number per realisation, and the probe's distance from the truth over sqrt(flips)
        #        -- flips add up incoherently -- the root-mean-square error e1 of one flip.  K ~ Poisson(lam) flips cost about e1 sqrt(K);
        #        ek = 2 e1 sqrt(k_q), k_q the KINK_Q quantile of K: 0 where a flip is that unlikely, else at least one WHOLE flip (the
        #        expected contribution e1 lam is no bound: at lam = 0.13, S3 at 34 x 38 x 50, the plain float32 run and the fp32 kernels
        #        both flip an element, 1.35e-3 of c0.weight, where e1 lam would allow 1e-4).  The 2: one flip costs |dL/da| at ITS
        #        element, which varies about the rms (that flip of S3 costs 1.8 e1); for a roughly normal |dL/da|, 95 % stay below 2 e1.
        t32 = _run_ref(name, n, size, torch.float32, MaskedOps(t64["pre"]), q, False)
        t16 = _run_ref(name, n, size, torch.float64, RoundedOps(), q, False) if rounded else None
        self.tau = [(a.double() - b).abs() for a, b in zip(t32["pre"], t64["pre"])]
        kops = KinkOps([t * KINK_M for t in self.tau])
        tk = _run_ref(name, n, size, torch.float64, kops, q, False)
        self.kink_lam = kops.flips / KINK_M
        self.kink_flips = _poisson_quantile(self.kink_lam, KINK_Q)
        kink_scale = 2.0 * math.sqrt(self.kink_flips / kops.flips) if kops.flips else 0.0
        self.q = [_ndhwc(t).float() for t in q]
        self.out = [_ndhwc(o) for o in t64["outs"]]
        self.part = [{k: (_ndhwc(v) if k == "x" else v) for k, v in p.items()} for p in t64["grads"]]
        self.names = list(self.part[0])
        self._dys = t64["dys"]
        self.dy_abs = self.dy_abs_of(None)
        full = self.grad()
        self.zero = set()
        for k in self.names:
            if k.endswith(".bias") and k not in GRAPHS[name].no_grad:
                lay = self.dy_abs.get(k[:-len(".bias")], 0.0)
                if float(full[k].abs().max()) <= 1e-9 * lay:
                    self.zero.add(k)
        self.e32, self.e16, self.ek = {}, {}, {}
        for e, t in ((self.e32, t32), (self.e16, t16), (self.ek, tk)):
            if t is None:
                continue
            for i, o in enumerate(t["outs"]):
                e["out%d" % i] = _rel(_ndhwc(o), self.out[i])
            for k in self.names:
                got = (_ndhwc(t["grads"][0][k]) if k == "x" else t["grads"][0][k]).double()
                if k in self.zero:
                    e[k] = float(got.abs().max()) / self.dy_abs[k[:-len(".bias")]]
                else:
                    e[k] = _rel(got, full[k])
                if t is tk:
                    e[k] *= kink_scale

    def grad(self, scales=None):
        scales = scales or [1.0] * len(self.part)
        return {k: sum(s * p[k] for s, p in zip(scales, self.part)) for k in self.names}

    def dy_abs_of(self, scales):
        """{layer name: sum |dL/d(conv output)|} of the loss with the consumers weighted by `scales` (a layer applied twice: both outputs)"""
        scales = scales or [1.0] * len(self._dys)
        out = {}
        for i, (k, _) in enumerate(self._dys[0]):
            t = [s * d[i][1] for s, d in zip(scales, self._dys) if d[i][1] is not None]
            out[k] = out.get(k, 0.0) + (float(sum(t).abs().sum()) if t else 0.0)
        return out

    def bound(self, key, bench):
        """16 e32 + ek on the fp32 routes, 3 e16 + 16 e32 + ek on the bench-precision routes"""
        return (3.0 * self.e16[key] if bench else 0.0) + 16.0 * self.e32[key] + self.ek[key]


def _poisson_quantile(lam, p):
    """the smallest k with P(Poisson(lam) <= k) >= p"""
    k, term = 0, math.exp(-lam)
    cum = term
    while cum < p:
        k += 1
        term *= lam / k
        cum += term
    return k


def _rel(got, ref):
    ref = ref.double()
    rn = float(ref.norm())
    d = float((got.double() - ref).norm())
    return d / rn if rn > 0 else (0.0 if d == 0 else float("inf"))


@functools.lru_cache(maxsize=None)
def reference(name, n, size, rounded=True):
    return Reference(name, n, tuple(size), rounded)


# ====================================================================================================================
# running the device statement
# ====================================================================================================================
class Run:
    """consumer values and gradients of one forward + backward of the device statement (CPU float64 copies, NDHWC)"""

    def __init__(self, outs, grads):
        self.out, self.grad = outs, grads


def run_device(name, mods, packer, I, q, K, sink=None, scg=None, scales=None, after_backward=None):
    """packer.refresh(), forward, loss = sum_k scales[k] * sum(consumer_k * q_k), backward (under `sink` if given), flush.  I / q: device
    tensors.  Gradients come from the sink where it was written, from .grad otherwise (None: zeros)."""
    g = GRAPHS[name]
    params = dict(mods.named_parameters())
    for p in params.values():
        p.grad = None
    I = dict(I)
    if g.x_grad:
        I["x"] = I["x"].detach().clone().requires_grad_(True)
    packer.refresh()
    outs = g.device(Ctx(mods, I, K, scg or contextlib.nullcontext))
    scales = scales or [1.0] * len(outs)
    loss = sum((o * (qk * s if s != 1.0 else qk)).sum() for o, qk, s in zip(outs, q, scales))
    if sink is not None:
        sink.begin()
        with sink:
            loss.backward()
            K.wgrad_flush()
    else:
        loss.backward()
    if after_backward is not None:
        after_backward()
    grads = {}
    for k, p in params.items():
        if not p.requires_grad:
            continue
        if sink is not None and p.data_ptr() in sink.written:
            assert p.grad is None, k                      # one route per parameter: the sink or autograd, never both
            gr = sink.view(p)
        else:
            gr = p.grad
        grads[k] = torch.zeros(p.shape, dtype=torch.float64) if gr is None else gr.detach().cpu().double()
    if g.x_grad:
        grads["x"] = I["x"].grad.detach().cpu().double()
    return Run([o.detach().cpu().double() for o in outs], grads)


def compare(run, ref, bench, scales=None, what=""):
    """every consumer value, parameter gradient and the input gradient against the truth; returns {key: (error, bound)} and the list of
    keys over their bound.  True-zero gradients: largest |element| against bound * sum |dy_ref| of the layer."""
    truth = ref.grad(scales)
    dy_abs = ref.dy_abs if scales is None else ref.dy_abs_of(scales)
    rows, bad = {}, []
    for i, o in enumerate(run.out):
        rows["out%d" % i] = (_rel(o, ref.out[i]), ref.bound("out%d" % i, bench))
    for k in ref.names:
        got = run.grad[k]
        assert bool(torch.isfinite(got).all()), (what, k, "non-finite gradient")
        if k in GRAPHS[ref.name].no_grad:
            rows[k] = (float(got.abs().max()), 0.0)
        elif k in ref.zero:
            rows[k] = (float(got.abs().max()) / dy_abs[k[:-len(".bias")]], ref.bound(k, bench))
        else:
            rows[k] = (_rel(got, truth[k]), ref.bound(k, bench))
    for k, (e, b) in rows.items():
        if not e <= b:
            bad.append((k, e, b))
    return rows, bad


@contextlib.contextmanager
def record_links():
    """every NaaLink / CarryLink that functional.py creates inside the block, for the no-state-left-behind checks"""
    from cwf import functional as CF
    seen = {"naa": [], "carry": []}
    naa0, carry0 = CF.NaaLink, CF.CarryLink

    class Naa(naa0):
        __slots__ = ()

        def __init__(self, *a):
            super().__init__(*a)
            seen["naa"].append(self)

    class Carry(carry0):
        __slots__ = ()

        def __init__(self):
            super().__init__()
            seen["carry"].append(self)

    CF.NaaLink, CF.CarryLink = Naa, Carry
    try:
        yield seen
    finally:
        CF.NaaLink, CF.CarryLink = naa0, carry0


def assert_links_clean(seen, what=""):
    assert all(l.sums is None for l in seen["naa"]), (what, "a NaaLink kept its sums")
    assert all(not l.grads for l in seen["carry"]), (what, "a CarryLink kept gradients")
