"""CPU: the block-graph catalogue (tests/block_graph_ref.py) through the kernel emulation, against its float64 references -- and the
references against oracle/reference_model.py and against central differences, so that the restatement is not trusted blindly.

This pins the catalogue and the default branches of cwf/functional.py (no bf16 images, no fused norm-backward sums, no gradient sink);
tests/test_block_graph_gpu.py runs the same graphs on the HIP kernels under every route.  Bound per tensor: 16 x e32 + ek, e32 = the
distance of the same reference graph run in torch float32 (on the truth's activation pattern) from float64 -- the emulation and ATen sum
in different orders -- and ek the error of the activation-branch flips to allow for (block_graph_ref.Reference)."""
import pytest
import torch

import block_graph_ref as B
from oracle import reference_model as rm

N, SIZE = B.CPU_SHAPE


def _tiny(seed, *shape):
    return torch.rand(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64) * 2 - 1


def _tiny_params(pre, convs):
    """{name: float64 leaf}: convs = [(layer, weight shape)]"""
    P = {}
    for i, (name, shape) in enumerate(convs):
        P[pre + name + ".weight"] = (_tiny(10 + i, *shape) * 0.5).requires_grad_(True)
        P[pre + name + ".bias"] = (_tiny(20 + i, shape[1] if name == "conv2T" else shape[0]) * 0.1).requires_grad_(True)
    return P


def test_the_block_statements_are_the_oracle_models():
    """en_block / post_block / de_up_cat of the catalogue == oracle.reference_model's, bit for bit in float64"""
    c = 4
    P = _tiny_params("b.", [("conv1", (c, c, 3, 3, 3)), ("conv2", (c, c, 3, 3, 3))])
    x = _tiny(1, 2, c, 4, 5, 6)
    assert torch.equal(B.en_block(B.Ops(), P, "b", x), rm.en_block(P, "b", x))
    assert torch.equal(B.post_block(B.Ops(), P, "b", x), rm.post_block(P, "b", x))
    Pu = {"u.conv1.weight": _tiny(2, c, 2 * c, 1, 1, 1), "u.conv1.bias": _tiny(3, c), "u.conv2.weight": _tiny(4, c, c, 2, 2, 2),
          "u.conv2.bias": _tiny(5, c), "u.conv3.weight": _tiny(6, c, 2 * c, 1, 1, 1), "u.conv3.bias": _tiny(7, c)}
    xu, prev = _tiny(8, 2, 2 * c, 2, 3, 2), _tiny(9, 2, c, 4, 6, 4)
    assert torch.equal(B.de_up_cat(B.Ops(), Pu, "u", xu, prev), rm.de_up_cat(Pu, "u", xu, prev))


@pytest.mark.parametrize("block", ["en_block", "post_block", "de_up_cat", "stem_down", "tail"])
def test_reference_gradients_are_central_differences(block):
    """torch.autograd.gradcheck (central differences, float64) on one tiny instance of every block type of the catalogue: the analytic
    gradients the tests call the truth are the derivatives of the stated forward"""
    c = 2
    if block in ("en_block", "post_block"):
        P = _tiny_params("b.", [("conv1", (c, c, 3, 3, 3)), ("conv2", (c, c, 3, 3, 3))])
        x = _tiny(31, 1, c, 3, 4, 4).requires_grad_(True)
        keys = sorted(P)
        fn = getattr(B, block)

        def f(x, *ps):
            return fn(B.Ops(), dict(zip(keys, ps)), "b", x)
        args = (x, *[P[k] for k in keys])
    elif block == "de_up_cat":
        P = {"u.conv1.weight": _tiny(2, c, 2 * c, 1, 1, 1), "u.conv1.bias": _tiny(3, c), "u.conv2.weight": _tiny(4, c, c, 2, 2, 2),
             "u.conv2.bias": _tiny(5, c), "u.conv3.weight": _tiny(6, c, 2 * c, 1, 1, 1), "u.conv3.bias": _tiny(7, c)}
        keys = sorted(P)
        x, prev = _tiny(32, 1, 2 * c, 2, 2, 3).requires_grad_(True), _tiny(33, 1, c, 4, 4, 6).requires_grad_(True)

        def f(x, prev, *ps):
            return B.de_up_cat(B.Ops(), dict(zip(keys, ps)), "u", x, prev)
        args = (x, prev, *[P[k].requires_grad_(True) for k in keys])
    elif block == "stem_down":
        # conv * keep (a zero channel, two scales) -> stride-2 conv -> softmax: the stem, EnDown and the head of U1
        P = _tiny_params("", [("stem", (4, 2, 3, 3, 3)), ("down", (3, 4, 3, 3, 3))])
        keys = sorted(P)
        x = _tiny(34, 2, 2, 4, 5, 4).requires_grad_(True)
        keep = torch.tensor([[1.25, 0.0, 2.0, 1.25], [0.0, 1.25, 1.25, 0.5]], dtype=torch.float64)

        def f(x, *ps):
            p = dict(zip(keys, ps))
            ops = B.Ops()
            y = ops.conv(p, "stem", x) * keep[:, :, None, None, None]
            return torch.softmax(ops.conv(p, "down", y, "c3s2"), 1)
        args = (x, *[P[k] for k in keys])
    else:
        # the stand-alone tail act(IN(g)) + x feeding a conv (S1, S10)
        P = _tiny_params("", [("c0", (c, c, 3, 3, 3)), ("cB", (c, c, 3, 3, 3))])
        keys = sorted(P)
        x = _tiny(35, 1, c, 3, 4, 4).requires_grad_(True)

        def f(x, *ps):
            p = dict(zip(keys, ps))
            ops = B.Ops()
            y = B._lk(ops, ops.conv(p, "c0", x)) + x
            return ops.conv(p, "cB", y) + y
        args = (x, *[P[k] for k in keys])
    assert torch.autograd.gradcheck(f, args, eps=1e-6, atol=1e-6, rtol=1e-5)


def test_the_rounded_reference_rounds_what_it_says():
    """RoundedOps on operands that ARE bf16 values computes the exact conv, forward and backward (nothing is rounded but the operands);
    on general operands its forward differs from the exact one by about 2^-16 (the dropped lo * lo products) and its gradients by
    about 2^-9 (single-bf16 products); a layer whose weight gradient runs on fp32 operands (a ConvTranspose with 4 | W) keeps exact ones"""
    for kind, wshape, xshape in (("c3", (4, 4, 3, 3, 3), (1, 4, 4, 4, 6)), ("ct", (4, 4, 2, 2, 2), (1, 4, 3, 2, 3)), ("ct", (4, 4, 2, 2, 2), (1, 4, 3, 2, 4)),
                                 ("c3s2", (4, 4, 3, 3, 3), (1, 4, 5, 4, 6))):
        for exact in (True, False):
            w, b, x = _tiny(41, *wshape), _tiny(42, 4), _tiny(43, *xshape)
            if exact:
                w, x = w.float().bfloat16().double(), x.float().bfloat16().double()
            res = []
            for ops in (B.Ops(), B.RoundedOps()):
                P = {"c.weight": w.clone().requires_grad_(True), "c.bias": b.clone().requires_grad_(True)}
                xi = x.clone().requires_grad_(True)
                y = ops.conv(P, "c", xi, kind)
                q = _tiny(44, *y.shape)
                if exact:
                    q = q.float().bfloat16().double()
                res.append((y.detach(),) + torch.autograd.grad((y * q).sum(), (xi, P["c.weight"], P["c.bias"])))
            rel = [float((a - r).norm() / r.norm()) for r, a in zip(*res)]
            if exact:
                assert max(rel) < 1e-14, (kind, rel)
            else:
                assert 1e-8 < rel[0] < 2.0 ** -15, (kind, rel)
                assert 2.0 ** -12 < rel[1] < 2.0 ** -7, (kind, rel)
                # weight and bias gradients: single-bf16 operands in the tiled kernels (the bias slot is ones . hi(dy)); fp32 operands
                # where wgrad_operand_mode sends the layer to pw_wgrad_kernel (this ConvTranspose: 4 | D*H*W and 4 | W fails -> bf16)
                mode = B.R.wgrad_operand_mode(B._OP_OF[kind], 4, 4, tuple(xshape[2:]), "bf16")
                assert (2.0 ** -12 < rel[2] < 2.0 ** -7) if mode == "bf16" else rel[2] < 1e-14, (kind, rel)
                assert (2.0 ** -14 < rel[3] < 2.0 ** -7) if (mode == "bf16" and kind != "ct") else rel[3] < 1e-14, (kind, rel)


@pytest.mark.parametrize("name", list(B.GRAPHS))
def test_graph_on_the_emulated_backend_matches_float64(emul_backend, name):
    """forward output, every parameter gradient and the input gradient of every graph, through cwf/functional.py on the kernel emulation,
    within 16 x e32 + ek of the float64 reference; with a second consumer, also after its weight is doubled (a dropped contribution);
    no link keeps state; a second pass on the same modules reproduces the first"""
    from cwf import functional as CF
    K = CF.backend()
    ref = B.reference(name, N, SIZE, False)
    mods, packer = B.build(name, "cpu")
    I, q = B.make_inputs(name, N, SIZE), ref.q
    cases = [None] + ([[1.0] + [2.0] * (len(q) - 1)] if len(q) > 1 else [])
    first = None
    for scales in cases + [None]:
        with B.record_links() as seen:
            run = B.run_device(name, mods, packer, I, q, K, scales=scales)
        B.assert_links_clean(seen, name)
        rows, bad = B.compare(run, ref, False, scales, name)
        print("\n%s %s" % (name, "scales %s" % scales if scales else ""))
        for k, (e, b) in rows.items():
            print("   %-22s err %.3e  bound %.3e  e32 %.3e  kink %.3e%s" % (k, e, b, ref.e32[k], ref.ek[k], "  (true zero)" if k in ref.zero else ""))
        assert not bad, (name, scales, bad)
        if scales is None:
            if first is None:
                first = run
            else:               # the emulation is deterministic: a second pass on the same modules is the first
                assert all(torch.equal(run.grad[k], first.grad[k]) for k in run.grad), name
    if name in ("U1", "U2"):
        # the conv biases in front of an InstanceNorm are the true zeros, found from the reference alone
        want = {k for k in ref.names if k.endswith((".conv1.bias",)) and not k.startswith("up.")}
        assert want <= ref.zero, (want - ref.zero)
