"""Batch preparation on the CPU: the separable edge-code formulation of tests/batch_prep_ref.py against utils.synthetic.edge_codes,
utils.data.prepare_batch (CPU statement) against that restatement, draw_params, DeviceBraTS(device="cpu") against the existing
datasets, and the new train_no_amp flags."""
import numpy as np
import pytest
import torch

import batch_prep_ref as R


def _edge(t):
    from utils import synthetic as syn
    return syn.edge_codes(torch.from_numpy(np.asarray(t, dtype=np.int64))).numpy()


@pytest.mark.parametrize("shape", [(9, 11, 7), (1, 13, 10), (12, 1, 1), (1, 1, 1), (2, 17, 3)])
def test_separable_edge_codes_dense(shape):
    rng = np.random.default_rng(sum(shape))
    for p in ((0.25, 0.25, 0.25, 0.25), (0.7, 0.1, 0.1, 0.1), (0.05, 0.05, 0.05, 0.85)):
        t = rng.choice(4, size=shape, p=p)
        np.testing.assert_array_equal(R.edge_codes_separable(t), _edge(t))


def test_separable_edge_codes_synthetic_and_flipped():
    from utils import synthetic as syn
    _, t = syn.synthetic_volume(3, (40, 36, 30), 1000)
    t = t.numpy()
    np.testing.assert_array_equal(R.edge_codes_separable(t), _edge(t))
    lab = R.random_labels((30, 25, 20), np.random.default_rng(5))
    for flip in [(a, b, c) for a in (0, 1) for b in (0, 1) for c in (0, 1)]:
        t = R.crop_source(lab.astype(np.int64), (3, 0, 4), flip, (17, 25, 19))
        t[t == 4] = 3
        np.testing.assert_array_equal(R.edge_codes_separable(t), _edge(t))


def _params(rng, shapes, crop, flip=True, intensity=True):
    from utils import data
    out = []
    for S in shapes:
        o = [int(rng.integers(0, max(s - c, 0) + 1)) for s, c in zip(S, crop)]
        fl = tuple(bool(v) for v in rng.integers(0, 2, 3)) if flip else (False,) * 3
        if intensity:
            out.append(data.AugParams(o, fl, rng.uniform(0.5, 1.5, 4), rng.uniform(-1, 1, 4)))
        else:
            out.append(data.AugParams(o, fl))
    return out


@pytest.mark.parametrize("crop", [(17, 23, 9), (1, 40, 33), (24, 24, 24)])
def test_prepare_batch_cpu_matches_restatement(crop):
    from utils import data
    rng = np.random.default_rng(crop[0] * 100 + crop[2])
    shapes = [(30, 20, 40), (12, 44, 33), (17, 23, 9)]
    imgs = [R.random_image(s, rng) for s in shapes]
    labs = [R.random_labels(shapes[0], rng), R.nested_labels(shapes[1], rng), R.random_labels(shapes[2], rng)]
    for flip, inten in ((False, False), (True, False), (True, True)):
        params = _params(rng, shapes, crop, flip, inten)
        x, t, e = data.prepare_batch([torch.from_numpy(i) for i in imgs], [torch.from_numpy(l) for l in labs], params, crop)
        rx, rt, re_ = R.prepare(imgs, labs, params, crop)
        assert x.dtype == torch.float32 and t.dtype == torch.int64 and e.dtype == torch.int64
        np.testing.assert_array_equal(x.numpy().view(np.int32), rx.view(np.int32))
        np.testing.assert_array_equal(t.numpy(), rt)
        np.testing.assert_array_equal(e.numpy(), re_)


def test_draw_params():
    from utils import data
    full, crop = (240, 240, 155), (128, 128, 128)
    a = data.draw_params(7, 2, 5, full, crop, flip=True, intensity=0.1)
    assert a == data.draw_params(7, 2, 5, full, crop, flip=True, intensity=0.1)
    assert a != data.draw_params(7, 3, 5, full, crop, flip=True, intensity=0.1)
    assert a.scale is not None and all(0.9 <= s <= 1.1 for s in a.scale) and all(-0.1 <= s <= 0.1 for s in a.shift)
    assert all(np.float32(v) == v for v in a.scale + a.shift)
    for seed, epoch, index in ((1000, 0, 0), (1000, 4, 17), (3, 1, 2)):
        off = data.draw_params(seed, epoch, index, full, crop)
        rng = np.random.default_rng([seed, epoch, index])
        assert off.origin == data.random_crop_origin(full, crop, rng)
        assert off.flip == (False, False, False) and off.scale is None and off.shift is None
        # the flip / intensity draws come after the origin: the origin does not depend on them
        assert data.draw_params(seed, epoch, index, full, crop, True, 0.2).origin == off.origin


def _write_npz(tmp_path, n, rng, layouts=("chw", "hwc")):
    shapes = [(26, 22, 19), (24, 30, 21), (20, 20, 20)][:n]
    for k, S in enumerate(shapes):
        img = R.random_image(S, rng)
        if layouts[k % len(layouts)] == "hwc":
            img = np.ascontiguousarray(np.moveaxis(img, 0, -1))
        lab = R.nested_labels(S, rng) if k % 2 else R.random_labels(S, rng)
        np.savez(tmp_path / ("s%02d.npz" % k), image=img, label=lab)
    return shapes


def test_device_brats_cpu_equals_npz_brats(tmp_path):
    from utils import data
    _write_npz(tmp_path, 3, np.random.default_rng(1))
    crop = (16, 24, 20)
    ref = data.NpzBraTS(str(tmp_path), crop=crop, seed=11)
    for cache in (True, False):
        dev = data.DeviceBraTS(str(tmp_path), "cpu", crop, seed=11, cache=cache)
        for epoch in (0, 1):
            ref.set_epoch(epoch); dev.set_epoch(epoch)
            x, t, e, m = dev.batch([2, 0, 1])
            items = [ref[i] for i in (2, 0, 1)]
            for got, k in ((x, 0), (t, 1), (e, 2), (m, 3)):
                want = torch.stack([it[k] for it in items])
                assert torch.equal(got, want)
            assert torch.equal(x.view(torch.int32), torch.stack([it[0] for it in items]).view(torch.int32))


def test_device_brats_cpu_equals_synthetic_brats():
    from utils import data
    from utils import synthetic as syn
    full, crop = (30, 28, 26), (24, 24, 24)
    ref = data.SyntheticBraTS(3, crop, seed=1000, full_size=full)
    subjects = [syn.synthetic_volume(i, full, 1000) for i in range(3)]
    dev = data.DeviceBraTS([(x, t.to(torch.uint8)) for x, t in subjects], "cpu", crop, seed=1000)
    for epoch in (0, 3):
        ref.set_epoch(epoch); dev.set_epoch(epoch)
        x, t, e, m = dev.batch([0, 1, 2])
        items = [ref[i] for i in range(3)]
        for got, k in ((x, 0), (t, 1), (e, 2), (m, 3)):
            assert torch.equal(got, torch.stack([it[k] for it in items]))


def test_device_brats_cpu_augmented_matches_restatement():
    from utils import data
    rng = np.random.default_rng(9)
    shapes = [(26, 22, 19), (18, 30, 21)]
    subjects = [(torch.from_numpy(R.random_image(S, rng)), torch.from_numpy(R.random_labels(S, rng))) for S in shapes]
    crop = (20, 24, 20)
    dev = data.DeviceBraTS(subjects, "cpu", crop, seed=4, flip=True, intensity=0.2)
    dev.set_epoch(2)
    x, t, e, _ = dev.batch([1, 0])
    params = [data.draw_params(4, 2, i, shapes[i], crop, True, 0.2) for i in (1, 0)]
    rx, rt, re_ = R.prepare([subjects[i][0].numpy() for i in (1, 0)], [subjects[i][1].numpy() for i in (1, 0)], params, crop)
    np.testing.assert_array_equal(x.numpy().view(np.int32), rx.view(np.int32))
    np.testing.assert_array_equal(t.numpy(), rt)
    np.testing.assert_array_equal(e.numpy(), re_)
    staged = data.DeviceBraTS(subjects, "cpu", crop, seed=4, flip=True, intensity=0.2, cache=False)
    staged.set_epoch(2)
    for a, b in zip(staged.batch([1, 0]), (x, t, e)):
        assert torch.equal(a, b)
    got = list(staged.batches([[1, 0]]))
    assert torch.equal(got[0][0].view(torch.int32), x.view(torch.int32))


def test_normalize_cpu_and_label_validation(tmp_path):
    from utils import data
    rng = np.random.default_rng(3)
    img = rng.standard_normal((4, 12, 10, 8)).astype(np.float32)
    ref, m = R.normalize_ref(img)
    t = torch.from_numpy(img.copy())
    data.normalize_nonzero(t)
    np.testing.assert_array_equal(t.numpy()[:, ~m], img[:, ~m])
    assert np.abs(t.numpy().astype(np.float64) - ref).max() <= np.spacing(np.abs(ref).max())
    bad = np.zeros((8, 8, 8), np.uint8); bad[1, 2, 3] = 5
    np.savez(tmp_path / "bad.npz", image=np.zeros((4, 8, 8, 8), np.float32), label=bad)
    with pytest.raises(ValueError, match="label values"):
        data.DeviceBraTS(str(tmp_path), "cpu", (8, 8, 8))


def test_train_flags_default_off():
    import train_no_amp as T
    a = T.build_parser().parse_args([])
    assert a.device_data == "off" and a.aug_flip is False and a.aug_intensity == 0.0 and a.normalize is False
    b = T.build_parser().parse_args(["--device_data", "staged", "--aug_flip", "1", "--aug_intensity", "0.1", "--normalize", "true"])
    assert b.device_data == "staged" and b.aug_flip is True and b.aug_intensity == 0.1 and b.normalize is True
    with pytest.raises(SystemExit):
        T.build_parser().parse_args(["--device_data", "sometimes"])
    with pytest.raises(SystemExit, match="only --mode train"):
        T.main(["--device_data", "cache", "--mode", "valid", "--synthetic", "1"])


@pytest.fixture()
def fresh_train_log():
    """train_no_amp attaches its log handlers once per process: drop the ones this test adds, so a later run logs to its own files"""
    import logging
    log = logging.getLogger("cwf.train")
    before = list(log.handlers)
    yield
    for h in list(log.handlers):
        if h not in before:
            log.removeHandler(h)
            h.close()


@pytest.mark.parametrize("device_data", ["cache", "staged"])
def test_train_harness_device_data_cpu(emul_backend, fresh_train_log, tmp_path, device_data):
    """--no_cuda with --device_data: the CPU statement of prepare_batch feeds the loop (2 iterations, checkpoint written)"""
    import train_no_amp as T
    rc = T.main(["--synthetic", "2", "--device_data", device_data, "--input_H", "72", "--input_W", "70", "--output_D", "66",
                 "--crop_H", "64", "--crop_W", "64", "--crop_D", "64", "--end_epoch", "1", "--max_iters", "2", "--aug_flip", "1",
                 "--aug_intensity", "0.1", "--project_root", str(tmp_path), "--experiment", "t", "--date", "d", "--no_cuda", "true"])
    assert rc == 0
    ck = torch.load(tmp_path / "checkpoint" / "td" / "model_epoch_last.pth", weights_only=True)
    assert all(bool(torch.isfinite(v).all()) for v in ck["state_dict"].values() if v.is_floating_point())
