"""Device batch preparation (csrc/prep.hip: cwf_prepare_batch, cwf_normalize_nonzero) against the numpy restatement of
tests/batch_prep_ref.py and the CPU statement of utils.data.prepare_batch: bit-exact outputs over flips, intensity, padded and oversized
crops, odd crops and multi-launch batches; guard bands and strided outputs; refusals; normalisation; DeviceBraTS against the existing
datasets in both device modes; and the train_no_amp --device_data path."""
import os

import numpy as np
import pytest
import torch

import batch_prep_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
FLIPS = [(a, b, c) for a in (False, True) for b in (False, True) for c in (False, True)]


def _upload(imgs, labs):
    return ([torch.from_numpy(i).to(DEV).contiguous() for i in imgs], [torch.from_numpy(l).to(DEV).contiguous() for l in labs])


def _check(got, imgs, labs, params, crop):
    x, t, e = got
    rx, rt, re_ = R.prepare(imgs, labs, params, crop)
    xr = torch.from_numpy(rx)
    assert torch.equal(x.cpu().view(torch.int32), xr.view(torch.int32))
    assert torch.equal(x.cpu(), xr) or bool(torch.isnan(xr).any())
    assert torch.equal(t.cpu(), torch.from_numpy(rt))
    assert torch.equal(e.cpu(), torch.from_numpy(re_))


def _p(origin, flip=(False,) * 3, scale=None, shift=None):
    from utils import data
    return data.AugParams(origin, flip, scale, shift)


def test_all_flips_intensity_and_placements(hip):
    """every flip mask, intensity on / off; crops inside, padded past the end, and larger than the volume on one axis"""
    rng = np.random.default_rng(0)
    crop = (16, 20, 24)
    shapes = [(30, 33, 40), (20, 25, 30), (10, 40, 48), (16, 20, 13)]
    imgs = [R.random_image(s, rng) for s in shapes]
    labs = [R.random_labels(shapes[0], rng), R.nested_labels(shapes[1], rng), R.random_labels(shapes[2], rng), R.nested_labels(shapes[3], rng)]
    dimgs, dlabs = _upload(imgs, labs)
    origins = [(7, 13, 16), (4, 5, 6), (0, 20, 24), (0, 0, 0)]       # inside; padded past the end; axis 0 oversized; two axes exact
    for flip in FLIPS:
        for inten in (False, True):
            params = [_p(o, flip, rng.uniform(0.5, 1.5, 4) if inten else None, rng.uniform(-2, 2, 4) if inten else None)
                      for o in origins]
            _check(hip.prepare_batch(dimgs, dlabs, params, crop), imgs, labs, params, crop)


@pytest.mark.parametrize("crop", [(17, 23, 9), (1, 40, 33), (5, 3, 130)])
def test_odd_crops(hip, crop):
    rng = np.random.default_rng(crop[1])
    shapes = [(20, 41, 31), (3, 30, 140)]
    imgs = [R.random_image(s, rng) for s in shapes]
    labs = [R.random_labels(s, rng) for s in shapes]
    dimgs, dlabs = _upload(imgs, labs)
    for flip in FLIPS:
        params = [_p([int(rng.integers(0, max(s - c, 0) + 1)) for s, c in zip(S, crop)], flip, rng.uniform(0.5, 1.5, 4),
                     rng.uniform(-1, 1, 4)) for S in shapes]
        _check(hip.prepare_batch(dimgs, dlabs, params, crop), imgs, labs, params, crop)


@pytest.mark.parametrize("B", [1, 3, 8, 11])
def test_batch_sizes_per_sample_extents(hip, B):
    """B above 8 takes more than one launch; every sample has its own source extents, labels dense or nested"""
    rng = np.random.default_rng(B)
    crop = (20, 16, 28)
    shapes = [tuple(int(v) for v in rng.integers(12, 36, 3)) for _ in range(B)]
    imgs = [R.random_image(s, rng) for s in shapes]
    labs = [R.random_labels(s, rng) if b % 2 else R.nested_labels(s, rng) for b, s in enumerate(shapes)]
    dimgs, dlabs = _upload(imgs, labs)
    params = [_p([int(rng.integers(0, max(s - c, 0) + 1)) for s, c in zip(S, crop)], tuple(bool(v) for v in rng.integers(0, 2, 3)),
                 *((rng.uniform(0.5, 1.5, 4), rng.uniform(-1, 1, 4)) if b % 3 else (None, None))) for b, S in enumerate(shapes)]
    _check(hip.prepare_batch(dimgs, dlabs, params, crop), imgs, labs, params, crop)


def test_full_size_brats_crop(hip):
    """240 x 240 x 155 -> 128^3 at B = 2, against the torch CPU statement"""
    from utils import data
    rng = np.random.default_rng(2)
    S, crop = (240, 240, 155), (128, 128, 128)
    imgs = [torch.from_numpy(rng.standard_normal((4,) + S, dtype=np.float32)) for _ in range(2)]
    labs = [torch.from_numpy(R.nested_labels(S, rng)), torch.from_numpy(R.random_labels(S, rng))]
    params = [data.draw_params(1000, 0, i, S, crop, flip=True, intensity=0.1) for i in range(2)]
    want = data.prepare_batch(imgs, labs, params, crop)
    got = data.prepare_batch([i.to(DEV) for i in imgs], [l.to(DEV) for l in labs], params, crop)
    for g, w in zip(got, want):
        assert g.is_cuda and torch.equal(g.cpu(), w)
    assert torch.equal(got[0].cpu().view(torch.int32), want[0].view(torch.int32))


def test_guard_bands_and_sample_stride(hip):
    """outputs written into views of larger buffers (sample stride > one sample, unaligned and aligned starts): the guard bands around
    and between the samples keep their sentinel"""
    rng = np.random.default_rng(4)
    for crop, lead in (((9, 10, 11), 3), ((8, 12, 16), 4)):
        B, V = 3, crop[0] * crop[1] * crop[2]
        shapes = [(14, 11, 20), (9, 10, 11), (6, 15, 30)]
        imgs = [R.random_image(s, rng) for s in shapes]
        labs = [R.random_labels(s, rng) for s in shapes]
        dimgs, dlabs = _upload(imgs, labs)
        params = [_p([int(rng.integers(0, max(s - c, 0) + 1)) for s, c in zip(S, crop)], (True, False, True), rng.uniform(0.5, 1.5, 4),
                     rng.uniform(-1, 1, 4)) for S in shapes]
        xs, ts = 4 * V + 2 * lead + 8, V + 2 * lead + 6
        xb = torch.full((B * xs + 64,), -7.5, dtype=torch.float32, device=DEV)
        tb = torch.full((B * ts + 64,), -11, dtype=torch.int64, device=DEV)
        eb = torch.full((B * ts + 64,), -13, dtype=torch.int64, device=DEV)
        x = xb.as_strided((B, 4) + crop, (xs, V, crop[1] * crop[2], crop[2], 1), lead)
        t = tb.as_strided((B,) + crop, (ts, crop[1] * crop[2], crop[2], 1), lead)
        e = eb.as_strided((B,) + crop, (ts, crop[1] * crop[2], crop[2], 1), lead)
        xr, tr, er = (b.clone() for b in (xb, tb, eb))
        got = hip.prepare_batch(dimgs, dlabs, params, crop, out=(x, t, e))
        assert got[0].data_ptr() == x.data_ptr()
        _check((x, t, e), imgs, labs, params, crop)
        for buf, ref, n, stride in ((xb, xr, 4 * V, xs), (tb, tr, V, ts), (eb, er, V, ts)):
            mask = torch.ones(buf.numel(), dtype=torch.bool, device=DEV)
            for b in range(B):
                mask[lead + b * stride: lead + b * stride + n] = False
            assert torch.equal(buf[mask], ref[mask])


def test_refusals(hip):
    from cwf import _lib
    rng = np.random.default_rng(5)
    S, crop = (20, 20, 20), (16, 16, 16)
    img = torch.from_numpy(R.random_image(S, rng)).to(DEV)
    lab = torch.from_numpy(R.random_labels(S, rng)).to(DEV)
    ok = _p((2, 3, 4))
    hip.prepare_batch([img], [lab], [ok], crop)
    with pytest.raises(ValueError):
        hip.prepare_batch([], [], [], crop)                                      # B <= 0
    for bad_crop in ((0, 16, 16), (16, -1, 16)):
        with pytest.raises(_lib.CwfError):
            hip.prepare_batch([img], [lab], [ok], bad_crop)                     # crop extent <= 0
    for o in ((5, 0, 0), (0, 0, 5), (-1, 0, 0)):
        with pytest.raises(_lib.CwfError):
            hip.prepare_batch([img], [lab], [_p(o)], crop)                     # origin outside [0, max(S - C, 0)]
    with pytest.raises(_lib.CwfError):
        hip.prepare_batch([img], [lab], [_p((1, 0, 0))], (30, 16, 16))          # crop larger than the volume: only origin 0
    # the C entry directly: every refusal is CWF_E_BADARG (-1) or CWF_E_TOOLARGE (-2), returned before anything is launched
    V = 16 ** 3
    xb = torch.empty(4 * V + 4, dtype=torch.float32, device=DEV)
    t = torch.empty(V + 2, dtype=torch.int64, device=DEV)
    e = torch.empty(V + 2, dtype=torch.int64, device=DEV)
    stream = torch.cuda.current_stream().cuda_stream

    def call(B=1, C=(16, 16, 16), x=None, xs=4 * V, tp=None, ts=V, ep=None, es=V, **sample):
        smp = (_lib.PrepSample * 1)()
        smp[0].image, smp[0].label = img.data_ptr(), lab.data_ptr()
        smp[0].S0 = smp[0].S1 = smp[0].S2 = 20
        for k, v in sample.items():
            setattr(smp[0], k, v)
        return hip.lib.cwf_prepare_batch(smp, B, C[0], C[1], C[2], xb.data_ptr() if x is None else x, xs,
                                         t.data_ptr() if tp is None else tp, ts, e.data_ptr() if ep is None else ep, es, stream)

    assert call() == 0
    torch.cuda.synchronize()
    for kw in (dict(B=0), dict(B=-3), dict(C=(16, 0, 16)), dict(C=(-2, 16, 16)),
               dict(x=0), dict(tp=0), dict(ep=0), dict(image=0), dict(label=0),
               dict(x=xb.data_ptr() + 2), dict(tp=t.data_ptr() + 4), dict(ep=e.data_ptr() + 1), dict(image=img.data_ptr() + 2),
               dict(o0=5), dict(o2=-1), dict(flip=8), dict(xs=4 * V - 1), dict(ts=V - 1), dict(S1=0)):
        assert call(**kw) == -1, kw
    assert call(C=(2048, 2048, 512), xs=1 << 40, ts=1 << 38, es=1 << 38) == -2
    # the same refusals surface through the wrapper as errors, never as "not eligible"
    with pytest.raises(_lib.CwfError, match="status -1"):
        hip.prepare_batch([img], [lab], [_p((0, 0, 9))], crop)
    with pytest.raises(_lib.CwfError, match="status -2"):
        hip.prepare_batch([img], [lab], [_p((0, 0, 0))], (2048, 2048, 512))
    with pytest.raises(ValueError):
        hip.prepare_batch([img], [lab.to(torch.int64)], [ok], crop)             # dtype
    with pytest.raises(ValueError):
        hip.prepare_batch([img.cpu()], [lab], [ok], crop)                       # device
    with pytest.raises(ValueError):
        hip.prepare_batch([img.transpose(1, 2)], [lab], [ok], crop)             # contiguity
    torch.cuda.synchronize()


def test_normalize_nonzero(hip):
    rng = np.random.default_rng(6)
    S = (40, 36, 30)
    img = (rng.standard_normal((4,) + S) * np.array([3.0, 0.5, 7.0, 1.0]).reshape(4, 1, 1, 1) + 1.0).astype(np.float32)
    img[:, :5] = 0.0                                                   # background outside the mask
    img[:, :, :3] = -1.0
    img[2] = np.where(img.sum(0) > 0, 4.25, img[2])                     # channel 2: constant over the mask (std 0: untouched)
    ref, m = R.normalize_ref(img)
    t = torch.from_numpy(img).to(DEV)
    assert hip.normalize_nonzero(t) is t
    got = t.cpu().numpy()
    np.testing.assert_array_equal(got[:, ~m].view(np.int32), img[:, ~m].view(np.int32))
    np.testing.assert_array_equal(got[2].view(np.int32), img[2].view(np.int32))
    ulp = np.spacing(np.abs(ref).astype(np.float32))
    assert np.all(np.abs(got.astype(np.float64) - ref.astype(np.float64)) <= ulp)


def _write_npz(tmp_path, rng):
    shapes = [(40, 36, 30), (34, 40, 28), (30, 30, 36)]
    for k, S in enumerate(shapes):
        img = R.random_image(S, rng)
        if k == 1:
            img = np.ascontiguousarray(np.moveaxis(img, 0, -1))
        lab = R.nested_labels(S, rng) if k % 2 else R.random_labels(S, rng)
        np.savez(tmp_path / ("s%02d.npz" % k), image=img, label=lab)
    return shapes


def test_device_brats_equivalence(hip, tmp_path):
    from utils import data
    rng = np.random.default_rng(7)
    shapes = _write_npz(tmp_path, rng)
    crop = (32, 32, 32)
    ref = data.NpzBraTS(str(tmp_path), crop=crop, seed=21)
    dev = data.DeviceBraTS(str(tmp_path), DEV, crop, seed=21)
    staged = data.DeviceBraTS(str(tmp_path), DEV, crop, seed=21, cache=False)
    for epoch in (0, 1):
        ref.set_epoch(epoch); dev.set_epoch(epoch); staged.set_epoch(epoch)
        got = dev.batch([1, 2, 0])
        items = [ref[i] for i in (1, 2, 0)]
        for k in range(4):
            want = torch.stack([it[k] for it in items])
            assert got[k].is_cuda and torch.equal(got[k].cpu(), want)
        assert torch.equal(got[0].cpu().view(torch.int32), torch.stack([it[0] for it in items]).view(torch.int32))
        for a, b in zip(staged.batch([1, 2, 0]), got):
            assert torch.equal(a, b)
        for a, b in zip(next(iter(staged.batches([[1, 2, 0]], num_workers=2))), got):
            assert torch.equal(a, b)
    # augmentation on: equal to the CPU statement with the same draw_params, cached and staged
    aug = data.DeviceBraTS(str(tmp_path), DEV, crop, seed=21, flip=True, intensity=0.3)
    aug_s = data.DeviceBraTS(str(tmp_path), DEV, crop, seed=21, flip=True, intensity=0.3, cache=False)
    cpu = data.DeviceBraTS(str(tmp_path), "cpu", crop, seed=21, flip=True, intensity=0.3)
    for epoch in (0, 5):
        for d in (aug, aug_s, cpu):
            d.set_epoch(epoch)
        want = cpu.batch([0, 1, 2])
        for d in (aug, aug_s):
            got = d.batch([0, 1, 2])
            for g, w in zip(got, want):
                assert torch.equal(g.cpu(), w)
            assert torch.equal(got[0].cpu().view(torch.int32), want[0].view(torch.int32))
    # normalised cache: every subject z-scored on the device at load (within one ulp of the float64 reference)
    norm = data.DeviceBraTS(str(tmp_path), DEV, crop, seed=21, normalize=True)
    for i in range(3):
        with np.load(str(tmp_path / ("s%02d.npz" % i))) as z:
            img = z["image"]
        if img.shape[0] != 4:
            img = np.ascontiguousarray(np.moveaxis(img, -1, 0))
        r, _ = R.normalize_ref(img)
        got = norm.images[i].cpu().numpy().astype(np.float64)
        assert np.all(np.abs(got - r) <= np.spacing(np.abs(r).astype(np.float32)))


def test_device_brats_synthetic_equals_synthetic_brats(hip):
    from utils import data
    from utils import synthetic as syn
    full, crop = (72, 70, 66), (64, 64, 64)
    ref = data.SyntheticBraTS(2, crop, seed=1000, full_size=full)
    dev = data.DeviceBraTS([(x, t.to(torch.uint8)) for x, t in (syn.synthetic_volume(i, full, 1000) for i in range(2))], DEV, crop, seed=1000)
    for epoch in (0, 1):
        ref.set_epoch(epoch); dev.set_epoch(epoch)
        got = dev.batch([0, 1])
        for k in range(4):
            assert torch.equal(got[k].cpu(), torch.stack([ref[i][k] for i in range(2)]))


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


@pytest.mark.parametrize("device_data,step_mode", [("cache", "eager"), ("staged", "plan")])
def test_train_harness_device_data(fresh_train_log, tmp_path, caplog, device_data, step_mode):
    """train_no_amp on generated 72 x 70 x 66 subjects, 64^3 crops (the model's smallest input), flips and intensity on; plan mode
    writes the later batches straight into the captured step's inputs"""
    import logging
    import re
    import train_no_amp as T
    root = str(tmp_path)
    iters = 2 if step_mode == "eager" else 5                 # plan: two eager warm-up steps, the capture, then replays
    argv = ["--synthetic", "3", "--device_data", device_data, "--input_H", "72", "--input_W", "70", "--output_D", "66",
            "--crop_H", "64", "--crop_W", "64", "--crop_D", "64", "--batch_size", "1", "--end_epoch", "3", "--max_iters", str(iters),
            "--num_workers", "1", "--project_root", root, "--experiment", "e", "--date", "d", "--aug_flip", "1",
            "--aug_intensity", "0.1", "--log_every", "1", "--step_mode", step_mode, "--save_freq", "1000"]
    with caplog.at_level(logging.INFO, logger="cwf.train"):
        assert T.main(argv) == 0
    ck = os.path.join(root, "checkpoint", "ed", "model_epoch_last.pth")
    assert os.path.isfile(ck)
    state = torch.load(ck, map_location="cpu", weights_only=True)
    assert all(bool(torch.isfinite(v).all()) for v in state["state_dict"].values() if v.is_floating_point())
    losses = [float(m.group(1)) for r in caplog.records for m in [re.search(r"_Iter:\d+\s+loss: (\S+)", r.getMessage())] if m]
    assert len(losses) >= iters - 1 and all(np.isfinite(losses)), losses
