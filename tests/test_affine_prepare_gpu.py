"""Rotated / zoomed crops on the device (csrc/prep.hip: cwf_prepare_batch_affine) against the CPU statement of utils.data.prepare_batch:
x as int32 bit patterns, target and edge exactly.  The parameter grid -- the three matrices of tests/affine_prep_ref.py, every flip
mask, intensity on and off, origins negative, inside and overhanging -- is run in full on the small crops (33 x 47 x 70, 1 x 1 x 5 and
8 x 12 x 18: none of their rows is a multiple of four voxels), and at 128^3 as one batch of eight in which every value of every
grid axis occurs (the CPU statement takes seconds per 128^3 sample); then batch sizes with mixed per-sample matrices, strided and misaligned outputs with guard bands, refusals,
host synchronisation and graph capture, DeviceBraTS staged against cached, and one train_no_amp run."""
import os

import numpy as np
import pytest
import torch

import affine_prep_ref as A

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
FLIPS = [(a, b, c) for a in (False, True) for b in (False, True) for c in (False, True)]
IDENT = (1, 0, 0, 0, 1, 0, 0, 0, 1)


def _sources(shapes, seed):
    rng = np.random.default_rng(seed)
    imgs = [torch.from_numpy(A.random_image(s, rng)) for s in shapes]
    labs = [torch.from_numpy(A.blob_labels(s, rng)) for s in shapes]
    return imgs, labs, [i.to(DEV) for i in imgs], [l.to(DEV) for l in labs]


def _origins(S, crop):
    """negative, inside, overhanging the far end"""
    return [tuple(-(2 + d) for d in range(3)), tuple(max(s - c, 0) // 2 for s, c in zip(S, crop)),
            tuple(max(s - c, 0) + 3 + d for d, (s, c) in enumerate(zip(S, crop)))]


def _inten(rng, on):
    return (rng.uniform(0.5, 1.5, 4), rng.uniform(-2, 2, 4)) if on else (None, None)


def _check(got, imgs, labs, params, crop):
    from utils import data
    want = data.prepare_batch(imgs, labs, params, crop)
    x, t, e = (g.cpu() for g in got)
    assert x.dtype == torch.float32 and t.dtype == torch.int64 and e.dtype == torch.int64
    assert not bool(torch.isnan(want[0]).any())
    assert torch.equal(x.view(torch.int32), want[0].view(torch.int32))
    assert torch.equal(t, want[1])
    assert torch.equal(e, want[2])
    return want


@pytest.mark.parametrize("crop", [(33, 47, 70), (1, 1, 5), (8, 12, 18)])
def test_bit_equal_parameter_grid(hip, crop):
    from utils import data
    rng = np.random.default_rng(crop[2])
    shapes = [(40, 50, 75), (30, 60, 64), (36, 44, 90)]
    imgs, labs, dimgs, dlabs = _sources(shapes, crop[1])
    nonzero = 0
    for m in A.MATRICES:
        for inten in (False, True):
            sel, params = [], []
            for k, flip in enumerate(FLIPS):
                for j in range(3):
                    s = (k + j) % 3
                    sel.append(s)
                    params.append(data.AugParams(_origins(shapes[s], crop)[j], flip, *_inten(rng, inten), matrix=m))
            want = _check(hip.prepare_batch([dimgs[s] for s in sel], [dlabs[s] for s in sel], params, crop),
                          [imgs[s] for s in sel], [labs[s] for s in sel], params, crop)
            nonzero += int((want[1] > 0).sum()) + int((want[2] > 0).sum())
    assert crop[0] == 1 or nonzero > 0                        # the labels and their edges are exercised, not all background


def test_bit_equal_128_cube(hip):
    """B = 8 at 128^3 from 240 x 240 x 155 and a smaller subject: all eight flip masks, the three matrices and a sample without one,
    intensity on and off, origins negative, inside and overhanging"""
    from utils import data
    rng = np.random.default_rng(128)
    crop = (128, 128, 128)
    shapes = [(240, 240, 155), (140, 150, 131)]
    imgs, labs, dimgs, dlabs = _sources(shapes, 7)
    sel, params = [], []
    for k, flip in enumerate(FLIPS):
        s = k % 2
        m = A.MATRICES[k % 3] if k != 7 else None
        o = _origins(shapes[s], crop)[(k // 2) % 3] if m is not None else (56, 0, 27)
        sel.append(s)
        params.append(data.AugParams(o, flip, *_inten(rng, k % 2 == 0 or k == 7), matrix=m))
    assert {p.matrix for p in params} == {tuple(float(v) for v in m) for m in A.MATRICES} | {None}
    want = _check(hip.prepare_batch([dimgs[s] for s in sel], [dlabs[s] for s in sel], params, crop),
                  [imgs[s] for s in sel], [labs[s] for s in sel], params, crop)
    assert all(len(torch.unique(want[1][b])) >= 3 and int((want[2][b] > 0).sum()) > 0 for b in range(8))   # no empty sample


@pytest.mark.parametrize("B", [1, 3, 8, 9])
def test_batch_sizes_mixed_matrices(hip, B):
    """B above 8 takes two launches; samples without a matrix ride along with the identity and equal the plain crop"""
    from utils import data
    rng = np.random.default_rng(B)
    crop = (20, 16, 28)
    shapes = [tuple(int(v) for v in rng.integers(18, 40, 3)) for _ in range(B)]
    imgs, labs, dimgs, dlabs = _sources(shapes, 30 + B)
    params = []
    for b, S in enumerate(shapes):
        m = None if b % 4 == 1 else A.MATRICES[b % 3]
        o = [int(rng.integers(0, max(s - c, 0) + 1)) for s, c in zip(S, crop)]
        params.append(data.AugParams(o, tuple(bool(v) for v in rng.integers(0, 2, 3)), *_inten(rng, b % 3 != 0), matrix=m))
    if B == 1:
        params[0] = params[0].at_origin((-3, 2, 30))
    got = hip.prepare_batch(dimgs, dlabs, params, crop)
    _check(got, imgs, labs, params, crop)
    for b, p in enumerate(params):
        if p.matrix is None:                                   # the same sample through cwf_prepare_batch
            plain = hip.prepare_batch([dimgs[b]], [dlabs[b]], [p], crop)
            assert all(torch.equal(g[b], q[0]) for g, q in zip(got, plain))


def test_identity_equals_the_plain_kernel(hip):
    from utils import data
    crop = (24, 20, 32)
    imgs, labs, dimgs, dlabs = _sources([(30, 33, 40)], 3)
    for flip in FLIPS:
        for o in ((0, 0, 0), (6, 13, 8)):
            sc, sh = _inten(np.random.default_rng(1), flip[1])
            plain = hip.prepare_batch(dimgs, dlabs, [data.AugParams(o, flip, sc, sh)], crop)
            ident = hip.prepare_batch(dimgs, dlabs, [data.AugParams(o, flip, sc, sh, IDENT)], crop)
            assert all(torch.equal(a, b) for a, b in zip(plain, ident))


def test_guard_bands_stride_and_misaligned_outputs(hip):
    """outputs written into views of larger buffers: sample stride larger than a sample, a start 12 B past 16-B alignment (per-voxel
    stores) and an aligned one (16-B stores); the bands around and between the samples keep their sentinel"""
    from utils import data
    rng = np.random.default_rng(4)
    for crop, lead in (((9, 10, 12), 3), ((8, 12, 16), 4), ((9, 10, 11), 4)):
        B, V = 3, crop[0] * crop[1] * crop[2]
        shapes = [(14, 11, 20), (9, 10, 11), (16, 15, 30)]
        imgs, labs, dimgs, dlabs = _sources(shapes, 5)
        params = [data.AugParams(o, (True, False, True), *_inten(rng, True), matrix=A.MATRICES[b])
                  for b, o in enumerate([(-2, 0, 3), (0, 0, 0), (4, 9, 17)])]
        xs, ts = 4 * V + 2 * lead + 8, V + 2 * lead + 6
        xb = torch.full((B * xs + 64,), -7.5, dtype=torch.float32, device=DEV)
        tb = torch.full((B * ts + 64,), -11, dtype=torch.int64, device=DEV)
        eb = torch.full((B * ts + 64,), -13, dtype=torch.int64, device=DEV)
        x = xb.as_strided((B, 4) + crop, (xs, V, crop[1] * crop[2], crop[2], 1), lead)
        t = tb.as_strided((B,) + crop, (ts, crop[1] * crop[2], crop[2], 1), lead)
        e = eb.as_strided((B,) + crop, (ts, crop[1] * crop[2], crop[2], 1), lead)
        assert (x.data_ptr() % 16 != 0) == (lead == 3)
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
    from utils import data
    S, crop = (20, 20, 20), (16, 16, 16)
    imgs, labs, dimgs, dlabs = _sources([S], 6)
    img, lab = dimgs[0], dlabs[0]
    m = A.MATRICES[0]
    hip.prepare_batch([img], [lab], [data.AugParams((-40, 9, 2000), matrix=m)], crop)        # any origin
    for bad_crop in ((0, 16, 16), (16, -1, 16)):
        with pytest.raises(_lib.CwfError, match="cwf_prepare_batch_affine failed with status -1"):
            hip.prepare_batch([img], [lab], [data.AugParams((0, 0, 0), matrix=m)], bad_crop)
    with pytest.raises(_lib.CwfError, match="cwf_prepare_batch_affine failed with status -2"):
        hip.prepare_batch([img], [lab], [data.AugParams((0, 0, 0), matrix=m)], (2048, 2048, 512))
    for bad in (float("nan"), float("inf"), -float("inf")):
        mm = list(m)
        mm[4] = bad
        with pytest.raises(_lib.CwfError, match="status -1"):
            hip.prepare_batch([img], [lab], [data.AugParams((0, 0, 0), matrix=mm)], crop)
    # the C entry directly: CWF_E_BADARG (-1) or CWF_E_TOOLARGE (-2), returned before anything is launched
    V = 16 ** 3
    xb = torch.empty(4 * V + 4, dtype=torch.float32, device=DEV)
    t = torch.empty(V + 2, dtype=torch.int64, device=DEV)
    e = torch.empty(V + 2, dtype=torch.int64, device=DEV)
    stream = torch.cuda.current_stream().cuda_stream

    def call(B=1, C=(16, 16, 16), x=None, xs=4 * V, tp=None, ts=V, ep=None, es=V, m4=None, **sample):
        smp = (_lib.PrepAffineSample * 1)()
        smp[0].image, smp[0].label = img.data_ptr(), lab.data_ptr()
        smp[0].S0 = smp[0].S1 = smp[0].S2 = 20
        smp[0].m[:] = [float(v) for v in m]
        if m4 is not None:
            smp[0].m[4] = m4
        for k, v in sample.items():
            setattr(smp[0], k, v)
        return hip.lib.cwf_prepare_batch_affine(smp, B, C[0], C[1], C[2], xb.data_ptr() if x is None else x, xs,
                                                t.data_ptr() if tp is None else tp, ts, e.data_ptr() if ep is None else ep, es, stream)

    assert call() == 0
    for kw in (dict(o0=5), dict(o2=-1), dict(o1=-2 ** 31), dict(o0=2 ** 31 - 1)):           # origins the plain call refuses
        assert call(**kw) == 0, kw
    torch.cuda.synchronize()
    for kw in (dict(B=0), dict(B=-3), dict(C=(16, 0, 16)), dict(C=(-2, 16, 16)),
               dict(x=0), dict(tp=0), dict(ep=0), dict(image=0), dict(label=0),
               dict(x=xb.data_ptr() + 2), dict(tp=t.data_ptr() + 4), dict(ep=e.data_ptr() + 1), dict(image=img.data_ptr() + 2),
               dict(flip=8), dict(flip=-1), dict(xs=4 * V - 1), dict(ts=V - 1), dict(es=V - 1), dict(S1=0),
               dict(m4=float("nan")), dict(m4=float("inf"))):
        assert call(**kw) == -1, kw
    assert call(C=(2048, 2048, 512), xs=1 << 40, ts=1 << 38, es=1 << 38) == -2
    assert hip.lib.cwf_prepare_batch_affine(None, 1, 16, 16, 16, xb.data_ptr(), 4 * V, t.data_ptr(), V, e.data_ptr(), V, stream) == -1
    torch.cuda.synchronize()


def test_huge_finite_matrix_reads_nothing(hip):
    """finite entries whose coordinates overflow (|q| >= 2^30, inf - inf): image 0 then the intensity map, label 0, as on the CPU"""
    from utils import data
    imgs, labs, dimgs, dlabs = _sources([(12, 12, 12)], 8)
    p = data.AugParams((0, 0, 0), scale=(2, 2, 2, 2), shift=(1, 2, 3, 4), matrix=(3e38, 3e38, 0, 0, 1, 0, 0, 0, 1e30))
    _check(hip.prepare_batch(dimgs, dlabs, [p], (4, 6, 8)), imgs, labs, [p], (4, 6, 8))


def _capture_case():
    from utils import data
    crop = (32, 24, 40)
    shapes = [(40, 36, 50), (30, 44, 48)]
    imgs, labs, dimgs, dlabs = _sources(shapes, 9)
    rng = np.random.default_rng(9)
    params = [data.AugParams((3, 4, 5), (True, False, False), *_inten(rng, True), matrix=A.MATRICES[0]),
              data.AugParams((-2, 10, 6), (False, True, True), matrix=A.MATRICES[2])]
    out = (torch.empty((2, 4) + crop, device=DEV), torch.empty((2,) + crop, dtype=torch.int64, device=DEV),
           torch.empty((2,) + crop, dtype=torch.int64, device=DEV))
    return imgs, labs, dimgs, dlabs, params, crop, out


def test_does_not_synchronise_with_the_host(hip):
    imgs, labs, dimgs, dlabs, params, crop, out = _capture_case()
    hip.prepare_batch(dimgs, dlabs, params, crop, out=out)      # code object loaded
    torch.cuda.synchronize()
    for o in out:
        o.zero_()
    old = torch.cuda.get_sync_debug_mode()
    try:
        torch.cuda.set_sync_debug_mode("error")
        try:
            torch.ones(1, device=DEV).item()                    # a synchronising call: the mode must object
            implemented = False
        except RuntimeError:
            implemented = True
        if implemented:
            hip.prepare_batch(dimgs, dlabs, params, crop, out=out)
    finally:
        torch.cuda.set_sync_debug_mode(old)
    if not implemented:
        pytest.skip("this torch build does not raise on synchronising calls under set_sync_debug_mode('error') on ROCm")
    _check(out, imgs, labs, params, crop)


def test_replays_under_graph_capture(hip):
    imgs, labs, dimgs, dlabs, params, crop, out = _capture_case()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        hip.prepare_batch(dimgs, dlabs, params, crop, out=out)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        hip.prepare_batch(dimgs, dlabs, params, crop, out=out)
    for _ in range(2):
        for o in out:
            o.fill_(-1)
        g.replay()
        torch.cuda.synchronize()
        _check(out, imgs, labs, params, crop)
    # the sources are read at replay time: new contents in the same buffers give the new batch
    dimgs[0].mul_(0.5)
    g.replay()
    torch.cuda.synchronize()
    _check(out, [dimgs[0].cpu(), imgs[1]], labs, params, crop)


def test_device_brats_staged_equals_cache(hip, tmp_path):
    from utils import data
    rng = np.random.default_rng(7)
    shapes = [(40, 36, 30), (34, 40, 28), (30, 30, 36)]
    for k, S in enumerate(shapes):
        np.savez(tmp_path / ("s%02d.npz" % k), image=A.random_image(S, rng), label=A.blob_labels(S, rng))
    crop = (32, 32, 32)
    kw = dict(seed=21, flip=True, intensity=0.3, rotate=15.0, scale=0.2)
    cache = data.DeviceBraTS(str(tmp_path), DEV, crop, **kw)
    staged = data.DeviceBraTS(str(tmp_path), DEV, crop, cache=False, **kw)
    cpu = data.DeviceBraTS(str(tmp_path), "cpu", crop, **kw)
    for epoch in (0, 5):
        for d in (cache, staged, cpu):
            d.set_epoch(epoch)
        want = cpu.batch([0, 1, 2])
        got = cache.batch([0, 1, 2])
        for g, w in zip(got, want):
            assert g.is_cuda and torch.equal(g.cpu(), w)
        assert torch.equal(got[0].cpu().view(torch.int32), want[0].view(torch.int32))
        for other in (staged.batch([0, 1, 2]), next(iter(staged.batches([[0, 1, 2]], num_workers=2)))):
            for a, b in zip(other, got):
                assert torch.equal(a, b)
            assert torch.equal(other[0].view(torch.int32), got[0].view(torch.int32))


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


def test_train_harness_rotate_scale(fresh_train_log, tmp_path, caplog):
    import logging
    import re
    import train_no_amp as T
    root = str(tmp_path)
    argv = ["--synthetic", "3", "--device_data", "cache", "--input_H", "72", "--input_W", "70", "--output_D", "66",
            "--crop_H", "64", "--crop_W", "64", "--crop_D", "64", "--batch_size", "1", "--end_epoch", "3", "--max_iters", "3",
            "--num_workers", "1", "--project_root", root, "--experiment", "a", "--date", "d", "--aug_flip", "1",
            "--aug_intensity", "0.1", "--aug_rotate", "15", "--aug_scale", "0.2", "--log_every", "1", "--save_freq", "1000"]
    with caplog.at_level(logging.INFO, logger="cwf.train"):
        assert T.main(argv) == 0
    ck = os.path.join(root, "checkpoint", "ad", "model_epoch_last.pth")
    assert os.path.isfile(ck)
    state = torch.load(ck, map_location="cpu", weights_only=True)
    assert all(bool(torch.isfinite(v).all()) for v in state["state_dict"].values() if v.is_floating_point())
    losses = [float(m.group(1)) for r in caplog.records for m in [re.search(r"_Iter:\d+\s+loss: (\S+)", r.getMessage())] if m]
    assert len(losses) >= 2 and all(np.isfinite(losses)), losses
