"""ORACLE TOOLING (build container only; never runs on the GPU box).

Imports the real reference from /root/reference, pushes the generator-defined weights
and inputs through it, checks ``oracle/reference_model.py`` (the CPU restatement)
against it, and writes the golden fixtures ``tests/golden/*.npz`` that pin the oracle
and the HIP path everywhere else.

Bridges: a synthesized ``fix_index.txt`` (F1) in a scratch cwd, an empty
``medpy`` stub module (only Hausdorff metrics touch it), ``InitConv.dropout = 0`` and
``model.eval()`` (F4), ``image_size``/``edge_image_size`` patched for non-128 inputs (F3).

    python oracle/make_golden.py            # writes tests/golden/*.npz, prints deviations
"""
import importlib.util
import os
import sys
import tempfile
import types

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "decouple-and-couple_learning_in_multi-modal_brain_tumor_segmentation_amd")
REF = "/root/reference"
GOLD = os.path.join(REPO, "tests", "golden")


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    m = importlib.util.module_from_spec(spec)
    sys.modules[name] = m
    spec.loader.exec_module(m)
    return m


syn = _load("cwf_synthetic", os.path.join(PKG, "utils", "synthetic.py"))
rm = _load("oracle_reference_model", os.path.join(REPO, "oracle", "reference_model.py"))
gs = _load("grad_sketch", os.path.join(REPO, "tests", "grad_sketch.py"))


def import_reference(n_index=8192):
    scratch = tempfile.mkdtemp(prefix="cwf_ref_")
    d = os.path.join(scratch, "2-MICCAI_BraTS_2018", "MICCAI_BraTS_2018_Data_Training")
    os.makedirs(d)
    with open(os.path.join(d, "fix_index.txt"), "w") as f:
        f.write(repr({str(i): [i] * 512 for i in range(n_index)}))
    os.chdir(scratch)
    for n in ("medpy", "medpy.metric"):
        sys.modules[n] = types.ModuleType(n)
    sys.modules["medpy"].metric = sys.modules["medpy.metric"]
    sys.path.insert(0, REF)
    from models.clswiseformer.cls_wise_former import get_cls_wise_former
    from models import criterions
    from utils import tools
    return get_cls_wise_former, criterions, tools


def ref_model(get_model, state, size):
    m = get_model(dataset="brats", _conv_repr=True, _pe_type="fixed", gpu=0)
    m.Unet_list.InitConv.dropout = 0.0
    m.image_size = tuple(s // 8 for s in size)
    m.edge_image_size = tuple(s // 4 for s in size)
    sd = m.state_dict()
    full = dict(state)
    for k in sd:
        if k.endswith(".pe"):
            full[k] = sd[k]
    assert list(sd.keys()) == [n for n, _, _ in rm.param_shapes()], "state_dict key order differs from Appendix B"
    for n, shp, _ in rm.param_shapes():
        assert tuple(sd[n].shape) == tuple(shp), (n, sd[n].shape, shp)
    m.load_state_dict(full)
    m.eval()
    return m, full


def sample_idx(n, k=4096):
    """Deterministic strided sample positions for big tensors."""
    return (np.arange(k, dtype=np.int64) * 2654435761 % n).astype(np.int64)


def maxrel(a, b):
    a, b = a.detach().double(), b.detach().double()
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))


def whole_model(get_model, criterions, tools, size, tag, with_grad=True):
    torch.manual_seed(0)
    state = syn.det_state_dict(rm.param_shapes())
    m, full = ref_model(get_model, state, size)
    x, target, edge = syn.synthetic_batch([0], size)
    assert torch.equal(m.fusion_label_pos.pe, rm.fixed_pe_table()), "pe table restatement differs"

    # ---- reference, fp32 (the pinned numerics)
    def run_ref(model, xin):
        for q in model.parameters():
            q.requires_grad_(True)
            q.grad = None
        o = model(xin, None)
        pr = [criterions.softmax_dice(o[0], target), tools.get_separate_loss(o[1], target),
              tools.get_edge_separate_loss(o[2], edge), tools.get_separate_loss(o[3], target),
              tools.get_edge_separate_loss(o[4], edge)]
        tot = sum(pr)
        if with_grad:
            tot.backward()
        return o, pr, tot, ({n: q.grad.detach().clone() for n, q in model.named_parameters()} if with_grad else {})

    outs, parts, loss, ref_grads = run_ref(m, x)

    # ---- restatement, fp32
    p = {k: v.clone().requires_grad_(not k.endswith(".pe")) for k, v in full.items()}
    o_outs, aux = rm.forward(p, x, return_aux=True)
    o_loss, o_parts = rm.total_loss(o_outs, target, edge)

    dev = {"prob": maxrel(o_outs[0], outs[0])}
    for j, nm in ((1, "sup"), (2, "edge"), (3, "mid_sup"), (4, "mid_edge")):
        for r in rm.REGIONS:
            dev["%s_%s" % (nm, r)] = maxrel(o_outs[j][r], outs[j][r])
    dev["loss"] = abs(float(o_loss) - float(loss)) / abs(float(loss))

    # ---- gradients: fp32 backprop through ~40 InstanceNorm layers is noisy (the fp32
    # reference itself deviates from its own float64 run by up to a few 1e-2 relative), so
    # the truth is the reference run in float64; the restatement must match THAT to 1e-10
    # and the per-tensor fp32 noise floor is recorded for the HIP tests' tolerances.
    if with_grad:
        m64 = m.double()
        _, _, loss64, g64 = run_ref(m64, x.double())
        p64 = {k: v.double().clone().requires_grad_(not k.endswith(".pe")) for k, v in full.items()}
        o64 = rm.forward(p64, x.double())
        l64, _ = rm.total_loss(o64, target, edge)
        l64.backward()
        live = [n for n in g64 if float(g64[n].norm()) > 1e-9]
        dev["grad64_restatement"] = max(float((p64[n].grad - g64[n]).norm() / g64[n].norm()) for n in live)
        dev["loss64"] = abs(float(l64) - float(loss64))
        noise = {n: float((ref_grads[n].double() - g64[n]).norm() / (g64[n].norm() + 1e-30)) for n in g64}
        print("[%s] fp32 reference grad noise vs its float64 run: median %.2e max(live) %.2e" % (
            tag, float(np.median([noise[n] for n in live])), max(noise[n] for n in live)))
    print("[%s] restatement vs reference:" % tag, {k: "%.2e" % v for k, v in dev.items()})
    assert all(v < 1e-5 for v in dev.values()), dev

    # ---- fixtures (from the REFERENCE's outputs)
    fx = {"size": np.array(size), "loss_parts": np.array([float(v) for v in parts], dtype=np.float64),
          "loss": np.float64(float(loss))}
    prob = outs[0].detach()
    n = prob.numel()
    si = sample_idx(n)
    fx["prob_sample_idx"] = si
    fx["prob_sample"] = prob.reshape(-1)[si].numpy()
    fx["logits_sample"] = aux["logits"].detach().reshape(-1)[si].numpy()      # restatement's logits (reference exposes none)
    fx["prob_sum_per_class"] = prob.double().sum((0, 2, 3, 4)).numpy()
    fx["argmax_hist"] = np.bincount(prob.argmax(1).reshape(-1).numpy(), minlength=4)
    fx["argmax_sample"] = prob.argmax(1).reshape(-1)[sample_idx(n // 4)].numpy().astype(np.int8)
    for j, nm in ((1, "sup"), (2, "edge"), (3, "mid_sup"), (4, "mid_edge")):
        for r in rm.REGIONS:
            t = outs[j][r].detach()
            s2 = sample_idx(t.numel(), 1024)
            fx["%s_%s_sample" % (nm, r)] = t.reshape(-1)[s2].numpy()
            fx["%s_%s_sum" % (nm, r)] = t.double().sum((0, 2, 3, 4)).numpy()
    for k, v in aux.items():
        if v.dtype == torch.int64:
            fx["topk_" + k] = v.numpy().astype(np.int32)
    bt = aux["bottleneck"].detach()
    s3 = sample_idx(bt.numel(), 8192)
    fx["bottleneck_sample"] = bt.reshape(-1)[s3].numpy()
    fx["bottleneck_l2"] = np.float64(float(bt.double().norm()))
    if with_grad:
        names = list(g64.keys())
        fx["grad_names"] = np.array(names)
        fx["grad_l2_f64"] = np.array([float(g64[n].norm()) for n in names])          # truth
        fx["grad_l2_ref32"] = np.array([float(ref_grads[n].double().norm()) for n in names])
        fx["grad_noise_ref32"] = np.array([noise[n] for n in names])                 # fp32 noise floor per tensor
        fx["loss_f64"] = np.float64(float(loss64))
        for n in ("e_token_01", "s_token_04", "decoder.endconv.weight", "decoder.endconv.bias",
                  "Unet_list.InitConv.conv.weight", "transformer_02.cross_attention_list.0.fn.norm2.weight",
                  "fusion_transformer_1_2_4.cross_ffn_list.0.fn.fn.net.3.bias", "conv_64_to_32.bias",
                  "mid_edge_supervise_label.edge_down_label_2.weight", "supervise_label.down_label_4.weight"):
            fx["grad::" + n] = g64[n].float().numpy()
    np.savez_compressed(os.path.join(GOLD, "model_%s.npz" % tag), **fx)
    return dev


def gradient_sketches(get_model, criterions, tools, size, tag, samples=(0,)):
    """tests/golden/grads_<tag>.npz: a count-sketch (tests/grad_sketch.py, 256 float64 numbers per tensor, tensors of at most 256
    elements whole) of EVERY parameter gradient of the imported reference run in float64, on the weights and inputs whole_model()
    uses; the reference's own fp32 distance from it in the same metric (the noise floor the tests scale their bound by); the five loss
    parts and the total in fp32 and float64; and the top-k index sets of the float64 forward, for teacher forcing (a near-tie flip
    changes gradients wholesale and is not what the sketch measures).  ``samples`` = the synthetic subjects of the batch: [0, 1] pins
    batch 2, where softmax_dice and the separate losses sum over the batch before they divide.  The reference's forward raises at
    B = 2 (its class tokens are concatenated as [1, 1, E]), and the only consistent meaning of a batch is independent samples:
    so the reference model runs once per sample, and the reference's loss functions -- which do take a batch -- run on the
    concatenated outputs.  The restatement runs the batch in one forward and has to agree.

    128^3 is left out on purpose: the float64 reference backward at that size does not fit the build container's 62 GB with margin, and
    the wiring these fixtures pin (which gradient lands in which tensor, slice and order) is the same at 64^3; what differs at 128^3 is
    tile geometry, which the kernel suites own."""
    torch.manual_seed(0)
    state = syn.det_state_dict(rm.param_shapes())
    m, full = ref_model(get_model, state, size)
    x, target, edge = syn.synthetic_batch(list(samples), size)

    def run_ref(model, xin):
        for q in model.parameters():
            q.requires_grad_(True)
            q.grad = None
        per = [model(xin[b:b + 1], None) for b in range(xin.shape[0])]
        o = [torch.cat([q[0] for q in per])] + [{r: torch.cat([q[j][r] for q in per]) for r in rm.REGIONS} for j in (1, 2, 3, 4)]
        pr = [criterions.softmax_dice(o[0], target), tools.get_separate_loss(o[1], target),
              tools.get_edge_separate_loss(o[2], edge), tools.get_separate_loss(o[3], target),
              tools.get_edge_separate_loss(o[4], edge)]
        tot = sum(pr)
        tot.backward()
        return [float(v.detach()) for v in pr], float(tot.detach()), {n: q.grad.detach().clone() for n, q in model.named_parameters()}

    parts32, loss32, g32 = run_ref(m, x)
    parts64, loss64, g64 = run_ref(m.double(), x.double())
    names = list(g64.keys())
    fx = gs.pack_reference(names, g64, g32)
    fx.update(size=np.array(size), samples=np.array(samples), n_not_live=np.int64(int((fx["l2_f64"] <= gs.LIVE_L2).sum())),
              loss_parts=np.array(parts32), loss=np.float64(loss32), loss_parts_f64=np.array(parts64), loss_f64=np.float64(loss64))

    # ---- the same computation as the existing fixture (B = 1 tags)
    if len(samples) == 1:
        old = np.load(os.path.join(GOLD, "model_%s.npz" % tag))
        assert list(old["grad_names"]) == names
        live = old["grad_l2_f64"] > gs.LIVE_L2
        rel = np.abs(fx["l2_f64"][live] - old["grad_l2_f64"][live]) / old["grad_l2_f64"][live]
        assert rel.max() < 1e-9 and (fx["l2_f64"][~live] <= gs.LIVE_L2).all(), rel.max()
        print("[grads_%s] l2_f64 vs model_%s.npz grad_l2_f64: max rel %.1e" % (tag, tag, rel.max()))

    # ---- the restatement in float64 on the same inputs: every live tensor within 1e-8 in the sketch metric; its top-k sets are the fixture's
    p64 = {k: v.double().clone().requires_grad_(not k.endswith(".pe")) for k, v in full.items()}
    o64, aux = rm.forward(p64, x.double(), return_aux=True)
    l64, _ = rm.total_loss(o64, target, edge, ce_float32=True)      # (the reference's CE term is fp32 arithmetic even in this run)
    l64.backward()
    refs = gs.reference_sketches(fx)
    dr = {n: gs.distance(gs.sketch_np(p64[n].grad.numpy(), i), r) for n, (i, r) in refs.items() if fx["l2_f64"][i] > gs.LIVE_L2}
    worst = max(dr, key=dr.get)
    print("[grads_%s] restatement float64 vs reference float64, sketch distance: worst %.1e (%s); loss %.1e" % (
        tag, dr[worst], worst, abs(float(l64.detach()) - loss64)))
    assert dr[worst] < 1e-8 and abs(float(l64.detach()) - loss64) < 1e-8 * abs(loss64), (worst, dr[worst])
    for k, v in aux.items():
        if v.dtype == torch.int64:
            fx["topk_" + k] = v.numpy().astype(np.int32)
    with torch.no_grad():                              # (the fp32 forward's selections, for the record: a near tie would show here)
        _, aux32 = rm.forward(full, x, return_aux=True)
    flips = {k: int((np.sort(fx["topk_" + k], -1) != np.sort(v.numpy(), -1)).sum()) for k, v in aux32.items() if v.dtype == torch.int64}
    lv = fx["l2_f64"] > gs.LIVE_L2
    print("[grads_%s] %d tensors, %d not live; reference fp32 noise in the sketch metric: median %.1e max %.1e; fp32 vs float64 top-k "
          "entries differing: %d" % (tag, len(names), int(fx["n_not_live"]), float(np.median(fx["noise_sketch"][lv])),
                                     float(fx["noise_sketch"][lv].max()), sum(flips.values())))
    np.savez_compressed(os.path.join(GOLD, "grads_%s.npz" % tag), **fx)


def loss_fixtures(criterions, tools):
    """tools.dice_loss / softmax_weighted_loss / get_separate_loss / get_edge_separate_loss
    on 2 x 16^3 random probabilities (values and gradients w.r.t. the probabilities)."""
    g = torch.Generator().manual_seed(7)
    fx = {}
    B, S = 2, 16
    target = torch.randint(0, 4, (B, S, S, S), generator=g)
    target[0, :4] = 0                              # unbalanced class frequencies
    edge = torch.tensor([0, 1, 2, 4, 5, 6, 7, 8])[torch.randint(0, 8, (B, S, S, S), generator=g)]
    p4 = torch.rand(B, 4, S, S, S, generator=g).pow(3)      # many values below the 0.005 clamp
    p4 = (p4 / p4.sum(1, keepdim=True)).requires_grad_(True)
    l = criterions.softmax_dice(p4, target)
    l.backward()
    fx.update(target=target.numpy(), edge=edge.numpy(), p4=p4.detach().numpy(), softmax_dice=np.float64(float(l)),
              softmax_dice_grad=p4.grad.numpy())
    outs, grads = {}, {}
    for r in ("01", "02", "04"):
        q = torch.rand(B, 2, S, S, S, generator=g).pow(2)
        outs[r] = (q / q.sum(1, keepdim=True)).requires_grad_(True)
    ls = tools.get_separate_loss(outs, target)
    ls.backward()
    for r in outs:
        fx["p2_" + r] = outs[r].detach().numpy()
        fx["sep_grad_" + r] = outs[r].grad.numpy().copy()
        outs[r].grad = None
    le = tools.get_edge_separate_loss(outs, edge)
    le.backward()
    for r in outs:
        fx["edge_grad_" + r] = outs[r].grad.numpy().copy()
    fx["separate_loss"] = np.float64(float(ls))
    fx["edge_separate_loss"] = np.float64(float(le))
    # restatement check
    p4b = torch.from_numpy(fx["p4"]).requires_grad_(True)
    lb = rm.softmax_dice(p4b, target)
    lb.backward()
    ob = {r: torch.from_numpy(fx["p2_" + r]).requires_grad_(True) for r in outs}
    lsb = rm.get_separate_loss(ob, target)
    leb = rm.get_edge_separate_loss(ob, edge)
    print("[loss] restatement vs reference: %.2e %.2e %.2e grad %.2e" % (
        abs(float(lb) - float(l)), abs(float(lsb) - float(ls)), abs(float(leb) - float(le)),
        float((p4b.grad - p4.grad).abs().max())))
    assert abs(float(lb) - float(l)) < 1e-6 and abs(float(lsb) - float(ls)) < 1e-6 and abs(float(leb) - float(le)) < 1e-6
    np.savez_compressed(os.path.join(GOLD, "losses.npz"), **fx)


def adam_fixture():
    """torch.optim.Adam(lr 2e-4, wd 1e-5, amsgrad) x 3 steps (train_no_amp.py:136,239)."""
    g = torch.Generator().manual_seed(3)
    p = torch.randn(1000, generator=g)
    w = p.clone().requires_grad_(True)
    opt = torch.optim.Adam([w], lr=2e-4, weight_decay=1e-5, amsgrad=True)
    grads = [torch.randn(1000, generator=g) * (10.0 ** (i - 1)) for i in range(3)]
    traj = []
    for gr in grads:
        w.grad = gr.clone()
        opt.step()
        traj.append(w.detach().clone().numpy())
    st = opt.state[w]
    np.savez_compressed(os.path.join(GOLD, "adam.npz"), p0=p.numpy(), grads=np.stack([x.numpy() for x in grads]),
                        traj=np.stack(traj), exp_avg=st["exp_avg"].numpy(), exp_avg_sq=st["exp_avg_sq"].numpy(),
                        max_exp_avg_sq=st["max_exp_avg_sq"].numpy())


def main():
    """python oracle/make_golden.py [--only TAG ...]   TAG in {losses, adam, 64, 128, noncubic, config4, grads_64, grads_noncubic, grads_64_b2}"""
    os.makedirs(GOLD, exist_ok=True)
    torch.set_num_threads(8)
    only = set(sys.argv[sys.argv.index("--only") + 1:]) if "--only" in sys.argv else None
    want = lambda t: only is None or t in only
    get_model, criterions, tools = import_reference()
    if want("losses"):
        loss_fixtures(criterions, tools)
    if want("adam"):
        adam_fixture()
    if want("64"):
        whole_model(get_model, criterions, tools, (64, 64, 64), "64")
    if want("128"):
        whole_model(get_model, criterions, tools, (128, 128, 128), "128")
    # non-cubic patches (BASELINE configs[4] trains on 160x192x160): the reference with image_size / edge_image_size patched and a
    # fix_index.txt of >= 4800 keys (SURVEY 8d "Config 5") -- pins the repo's size generalisation (F3) against the reference itself
    if want("noncubic"):
        whole_model(get_model, criterions, tools, (64, 96, 80), "noncubic")
    if want("config4"):
        whole_model(get_model, criterions, tools, (160, 192, 160), "config4", with_grad=False)
    # every parameter gradient, by count-sketch (after the model_* fixtures: the B = 1 tags assert against them)
    if want("grads_64"):
        gradient_sketches(get_model, criterions, tools, (64, 64, 64), "64")
    if want("grads_noncubic"):
        gradient_sketches(get_model, criterions, tools, (64, 96, 80), "noncubic")
    if want("grads_64_b2"):
        gradient_sketches(get_model, criterions, tools, (64, 64, 64), "64_b2", samples=(0, 1))
    print("golden fixtures written to", GOLD)


if __name__ == "__main__":
    main()
