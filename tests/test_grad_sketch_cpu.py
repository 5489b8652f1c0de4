"""CPU: the count-sketch of tests/grad_sketch.py -- one hash in numpy and torch, the new fixtures tied to the old ones, the estimator's
accuracy on real gradients, and the edits a per-tensor norm cannot see."""
import os

import numpy as np
import pytest
import torch

import grad_sketch as gs
from conftest import GOLDEN

FULL = ("e_token_01", "s_token_04", "decoder.endconv.weight", "decoder.endconv.bias", "Unet_list.InitConv.conv.weight",
        "transformer_02.cross_attention_list.0.fn.norm2.weight", "fusion_transformer_1_2_4.cross_ffn_list.0.fn.fn.net.3.bias",
        "conv_64_to_32.bias", "mid_edge_supervise_label.edge_down_label_2.weight", "supervise_label.down_label_4.weight")


@pytest.fixture(scope="module")
def fx64():
    return np.load(os.path.join(GOLDEN, "grads_64.npz"))


@pytest.fixture(scope="module")
def full64():
    g = np.load(os.path.join(GOLDEN, "model_64.npz"))
    return {n: g["grad::" + n].astype(np.float64) for n in FULL}


@pytest.mark.parametrize("n,start", [(1, 0), (255, 0), (256, 0), (257, 0), (27 * 256 * 128, 0), (512, 2 ** 31 - 256), (512, 2 ** 32 - 256),
                                     (64, 2 ** 40)])
def test_numpy_and_torch_give_the_same_pattern(n, start):
    for seed in (0, 7, 217):
        b, s = gs.pattern_np(n, seed, start)
        bt, st = gs.pattern_torch(n, seed, "cpu", start)
        assert b.dtype == np.int64 and bt.dtype == torch.int64 and s.dtype == np.float64 and st.dtype == torch.float64
        assert np.array_equal(b, bt.numpy()) and np.array_equal(s, st.numpy())
        assert b.min() >= 0 and b.max() < gs.S and set(np.unique(s)) <= {-1.0, 1.0}
    # the pattern is a function of the absolute index (a window equals the slice of a longer run) and of the seed
    if start == 0 and n > 256:
        b2, s2 = gs.pattern_np(100, 217, 150)
        assert np.array_equal(b2, b[150:250]) and np.array_equal(s2, s[150:250])
        b3, s3 = gs.pattern_np(n, 8, start)
        assert 0.98 < np.mean(b3 != gs.pattern_np(n, 7, start)[0]) and 0.4 < np.mean(s3 != gs.pattern_np(n, 7, start)[1]) < 0.6


def test_pattern_is_balanced_and_pinned():
    """buckets uniform and signs fair to counting noise on the largest tensor's size; a handful of values pinned, so that a change of
    the hash (which would orphan the fixtures) shows here first"""
    n = 27 * 256 * 128
    b, s = gs.pattern_np(n, 5)
    cnt = np.bincount(b, minlength=gs.S)
    assert abs(cnt - n / gs.S).max() < 5 * np.sqrt(n / gs.S) and abs(s.sum()) < 5 * np.sqrt(n)
    for k in range(gs.S):                                   # sign and bucket independent: each bucket's signs fair too
        assert abs(s[b == k].sum()) < 5 * np.sqrt(cnt[k])
    assert gs.pattern_np(8, 5)[0].tolist() == [234, 128, 179, 7, 225, 68, 112, 17]
    assert gs.pattern_np(8, 5)[1].tolist() == [-1.0, -1.0, 1.0, -1.0, 1.0, 1.0, -1.0, 1.0]


def test_sketch_numpy_equals_torch_and_small_tensors_stay_whole():
    rng = np.random.default_rng(0)
    for shape in [(1,), (4,), (256,), (257,), (2, 8, 3, 3, 3), (1536, 512)]:
        a = rng.standard_normal(shape)
        sn, st = gs.sketch_np(a, 3), gs.sketch_torch(torch.from_numpy(a).float(), 3).numpy()
        assert sn.shape == st.shape == (min(a.size, gs.S),)
        assert np.abs(sn - st).max() <= 1e-6 * np.abs(sn).max()                     # (the torch input was rounded to fp32)
        assert np.abs(sn - gs.sketch_torch(torch.from_numpy(a), 3).numpy()).max() <= 1e-12 * np.abs(sn).max()
        if a.size <= gs.S:
            assert np.array_equal(sn, a.reshape(-1))
        # non-contiguous views are sketched in their contiguous layout
        at = torch.from_numpy(a)
        if at.ndim >= 2:
            view = at.transpose(0, 1).contiguous().transpose(0, 1)
            assert not view.is_contiguous() or 1 in view.shape[:2]
            assert torch.equal(gs.sketch_torch(view, 3), gs.sketch_torch(at, 3))


def test_fixtures_are_consistent_and_tied_to_the_full_gradients(fx64, full64):
    """every grads_*.npz: shapes, the ragged whole tensors against their rows, l2 of a whole tensor from its values; grads_64 and
    grads_noncubic carry the norms of model_64 / model_noncubic; and the sketch of each of the ten full gradients of model_64.npz (stored
    in fp32: 6e-8 per element) reproduces its row of grads_64.npz"""
    import oracle.reference_model as rm
    shapes = {n: tuple(s) for n, s, _ in rm.param_shapes()}
    total = 0
    for tag, old in (("64", "model_64.npz"), ("noncubic", "model_noncubic.npz"), ("64_b2", None)):
        path = os.path.join(GOLDEN, "grads_%s.npz" % tag)
        total += os.path.getsize(path)
        fx = np.load(path)
        names = [str(n) for n in fx["grad_names"]]
        assert len(names) == 218 and fx["sketch_f64"].shape == (218, gs.S) and fx["sketch_f64"].dtype == np.float64
        assert [int(v) for v in fx["numel"]] == [int(np.prod(shapes[n])) for n in names]
        refs = gs.reference_sketches(fx)
        for n, (i, r) in refs.items():
            numel = int(fx["numel"][i])
            assert r.shape == (min(numel, gs.S),) and np.array_equal(fx["sketch_f64"][i, :r.size], r)
            if numel <= gs.S:
                assert not fx["sketch_f64"][i, numel:].any()
                assert abs(np.linalg.norm(r) - fx["l2_f64"][i]) <= 1e-12 * fx["l2_f64"][i] + 1e-300
        assert int(fx["n_not_live"]) == int((fx["l2_f64"] <= gs.LIVE_L2).sum()) == 32
        assert fx["loss_parts"].shape == fx["loss_parts_f64"].shape == (5,)
        assert np.allclose(fx["loss_parts"], fx["loss_parts_f64"], rtol=1e-5) and abs(fx["loss_parts_f64"].sum() - fx["loss_f64"]) < 1e-9
        assert sum(k.startswith("topk_") for k in fx.files) == 13
        assert all(fx[k].shape[0] == len(fx["samples"]) for k in fx.files if k.startswith("topk_"))
        if old:
            g = np.load(os.path.join(GOLDEN, old))
            assert list(g["grad_names"]) == list(fx["grad_names"])
            live = g["grad_l2_f64"] > gs.LIVE_L2
            assert np.abs(fx["l2_f64"][live] / g["grad_l2_f64"][live] - 1).max() < 1e-9
            assert np.allclose(fx["loss_parts"], g["loss_parts"], rtol=1e-7)
            assert all(np.array_equal(np.sort(fx[k], -1), np.sort(g[k], -1)) for k in g.files if k.startswith("topk_"))      # the same sets
    assert total < 1.5e6
    refs = gs.reference_sketches(fx64)
    for n, a in full64.items():
        i, r = refs[n]
        assert gs.distance(gs.sketch_np(a, i), r) < 1e-6, n


def _true_and_estimate(ref, got, seed):
    return float(np.linalg.norm(got - ref) / np.linalg.norm(ref)), gs.distance(gs.sketch_np(got, seed), gs.sketch_np(ref, seed))


def test_estimator_within_its_factor_on_real_gradients(fx64, full64):
    """d_hat against the true relative L2 distance on the ten full gradients, each with its own seed: dense Gaussian noise, one changed
    element, a change confined to one output channel (tensors with more than one), at relative sizes 1e-3, 2e-2, 1e-1, 200 draws each.
    Whole tensors (n <= S) must be exact; of the others' draws at most 1 in 1000 may leave the factor 1.25, either way.  One fixed
    generator, every draw counted, none repeated."""
    rng = np.random.default_rng(20240)
    names = [str(n) for n in fx64["grad_names"]]
    draws = outside = 0
    worst = 1.0
    for n, ref in full64.items():
        seed = names.index(n)
        flat = ref.reshape(-1)
        kinds = ["dense", "element"] + (["channel"] if ref.ndim >= 2 and ref.shape[0] > 1 else [])
        for kind in kinds:
            for size in (1e-3, 2e-2, 1e-1):
                for _ in range(200):
                    e = np.zeros_like(ref)
                    if kind == "dense":
                        e = rng.standard_normal(ref.shape)
                    elif kind == "element":
                        e.reshape(-1)[rng.integers(flat.size)] = 1.0
                    else:
                        e[rng.integers(ref.shape[0])] = rng.standard_normal(ref.shape[1:])
                    e *= size * np.linalg.norm(ref) / np.linalg.norm(e)
                    d, dh = _true_and_estimate(ref, ref + e, seed)
                    assert abs(d - size) < 1e-9 * size
                    if flat.size <= gs.S:
                        assert abs(dh - d) <= 1e-9 * d, (n, kind)
                        continue
                    draws += 1
                    worst = max(worst, dh / d, d / dh)
                    outside += not (d / gs.ESTIMATOR_FACTOR <= dh <= d * gs.ESTIMATOR_FACTOR)
    print("estimator: %d draws on sketched tensors, %d outside the factor %.2f, worst ratio %.3f" % (draws, outside, gs.ESTIMATOR_FACTOR, worst))
    assert draws >= 200 * 9 * 3 and outside * 1000 <= draws, (outside, draws)


def _gradient_like(shape, seed):
    """Gaussian with a per-output-channel and a per-input-channel scale over a decade: rows and columns of a real gradient differ in size"""
    rng = np.random.default_rng(seed)
    a = rng.standard_normal(shape)
    a *= np.exp(rng.uniform(-1.15, 1.15, (shape[0],) + (1,) * (len(shape) - 1)))
    return a * np.exp(rng.uniform(-1.15, 1.15, (1, shape[1]) + (1,) * (len(shape) - 2)))


# the largest bound any live tensor of the three fixtures gets (either floor)
def _largest_bound():
    worst = 0.0
    for tag in ("64", "noncubic", "64_b2"):
        fx = np.load(os.path.join(GOLDEN, "grads_%s.npz" % tag))
        worst = max(worst, max(gs.bound(v, 2e-2) for v, l in zip(fx["noise_sketch"], fx["l2_f64"]) if l > gs.LIVE_L2))
    return worst


def test_edits_a_norm_cannot_see_are_far_in_the_sketch():
    """On tensors of the model's shapes: each edit keeps the tensor's norm to under 1 % -- the per-tensor norm check passes it -- and
    must be far outside any bound in the sketch metric: d_hat > 0.3 for the four rearrangements.  A removed orthogonal component of 14 %
    has the true distance 0.14 / sqrt(1 + 0.14^2) = 0.1386 and so cannot reach 0.3 under any metric; it is held to the estimator's factor
    around 0.1386, which is above the largest bound a tensor of the fixtures has.  A uniform scale by 1.005 stays under the bound."""
    norm_moves = lambda a, b: abs(np.linalg.norm(b) / np.linalg.norm(a) - 1.0)
    conv = _gradient_like((32, 32, 3, 3, 3), 1)
    qkv = _gradient_like((1536, 512), 2)
    pa, pb = _gradient_like((512, 512), 3), _gradient_like((512, 512), 4)
    pb *= np.linalg.norm(pa) / np.linalg.norm(pb) * 1.004
    rolled = conv.copy()
    rolled[:, -16:] = np.roll(conv[:, -16:], 4, axis=1)
    edits = {"mirrored taps, axis %d" % ax: (conv, np.flip(conv, 2 + ax), 82) for ax in range(3)}
    edits["q and k row blocks exchanged"] = (qkv, np.concatenate([qkv[512:1024], qkv[:512], qkv[1024:]]), 12)
    edits["two tensors exchanged (a for b)"] = (pa, pb, 10)
    edits["two tensors exchanged (b for a)"] = (pb, pa, 23)
    edits["last 16 input channels rolled by 4"] = (conv, rolled, 82)
    for what, (ref, got, seed) in edits.items():
        assert norm_moves(ref, got) < 1e-2, what
        d, dh = _true_and_estimate(ref, got, seed)
        assert dh > 0.3, (what, d, dh)
    largest = _largest_bound()
    assert largest < 0.1386 / gs.ESTIMATOR_FACTOR, largest
    for ref, seed in ((conv, 82), (qkv, 12), (_gradient_like((4, 16, 1, 1, 1), 5), 164)):
        got = gs.remove_orthogonal_component(ref, 0.14, np.random.default_rng(seed))
        assert norm_moves(ref, got) < 1e-2
        d, dh = _true_and_estimate(ref, got, seed)
        assert abs(d - 0.14 / np.sqrt(1 + 0.14 ** 2)) < 1e-9 and d / gs.ESTIMATOR_FACTOR <= dh <= d * gs.ESTIMATOR_FACTOR and dh > largest, (d, dh)
        d, dh = _true_and_estimate(ref, 1.005 * ref, seed)
        assert abs(dh - 0.005) < 1e-9 and dh < gs.bound(0.0, 1e-2)
