"""Elastically deformed crops on the device (csrc/prep.hip: cwf_prepare_batch_elastic) against the CPU statement of
utils.data.prepare_batch: x as int32 bit patterns, target and edge exactly.  Sources are about 24 x 28 x 40; the crops are one tile
(8 x 8 x 32), whole tiles, ragged tiles and rows that are no multiple of four voxels (per-voxel stores).  Then batches of nine with
mixed samples, strided and misaligned outputs with guard bands, non-finite control values, the C entry's refusals, and DeviceBraTS
cached against staged against the CPU."""
import numpy as np
import pytest
import torch

import elastic_prep_ref as E

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
FLIPS = [(a, b, c) for a in (False, True) for b in (False, True) for c in (False, True)]
IDENT = (1, 0, 0, 0, 1, 0, 0, 0, 1)
MATRIX = (0.93, -0.21, 0.08, 0.17, 1.04, -0.12, -0.05, 0.16, 0.88)
SHAPES = [(24, 28, 40), (26, 24, 37), (21, 30, 44)]


def _sources(shapes, seed):
    rng = np.random.default_rng(seed)
    imgs = [torch.from_numpy(E.random_image(s, rng)) for s in shapes]
    labs = [torch.from_numpy(E.blob_labels(s, rng)) for s in shapes]
    return imgs, labs, [i.to(DEV) for i in imgs], [l.to(DEV) for l in labs]


@pytest.fixture(scope="module")
def sources():
    return _sources(SHAPES, 2)


def _origins(S, crop):
    """negative, inside, beyond the volume"""
    return [tuple(-(2 + d) for d in range(3)), tuple(max(s - c, 0) // 2 for s, c in zip(S, crop)), tuple(s + 3 + d for d, s in enumerate(S))]


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


@pytest.mark.parametrize("crop", [(8, 8, 32), (16, 16, 32), (20, 12, 40), (9, 10, 35)])
def test_bit_equal_parameter_grid(hip, sources, crop):
    from utils import data
    imgs, labs, dimgs, dlabs = sources
    rng = np.random.default_rng(crop[2] + crop[0])
    nonzero = outside = 0
    for grid in ((4, 4, 4), (7, 7, 7), (4, 5, 8)):
        for m in (None, MATRIX):
            for inten in (False, True):
                for amp in (2.0, 30.0):
                    sel, params = [], []
                    for k, flip in enumerate(FLIPS):
                        s = (k + grid[2]) % 3
                        o = _origins(SHAPES[s], crop)[(k + int(amp) + grid[1]) % 3] if amp == 2.0 else _origins(SHAPES[s], crop)[k % 2]
                        sel.append(s)
                        params.append(data.AugParams(o, flip, *_inten(rng, inten), matrix=m, disp=E.random_grid(grid, amp, rng)))
                    want = _check(hip.prepare_batch([dimgs[s] for s in sel], [dlabs[s] for s in sel], params, crop),
                                  [imgs[s] for s in sel], [labs[s] for s in sel], params, crop)
                    nonzero += int((want[1] > 0).sum()) + int((want[2] > 0).sum())
                    if amp == 30.0 and not inten:
                        outside += int((want[0][1::2, 3] == 0).sum())       # origins inside; channel 3 is about 100 inside the volume
    assert nonzero > 0 and outside > 0


def test_batch_of_nine_mixed_samples(hip):
    """two launches, the second with one sample; samples with a grid, with only a matrix and with neither.  Those without a grid are
    bit-equal to what cwf_prepare_batch_affine gives them alone."""
    from utils import data
    rng = np.random.default_rng(9)
    crop = (12, 10, 36)
    shapes = [SHAPES[b % 3] for b in range(9)]
    imgs, labs, dimgs, dlabs = _sources(shapes, 19)
    params = []
    for b, S in enumerate(shapes):
        kind = (b + 1) % 3                                     # 0: grid (b = 2, 5, 8: the lone sample of the second launch), 1: matrix, 2: neither
        o = [int(rng.integers(-3, max(s - c, 0) + 4)) for s, c in zip(S, crop)]
        g = tuple(int(v) for v in rng.integers(4, 9, 3))
        params.append(data.AugParams(o, tuple(bool(v) for v in rng.integers(0, 2, 3)), *_inten(rng, b % 2 == 0),
                                     matrix=MATRIX if kind == 1 or b == 5 else None, disp=E.random_grid(g, 5.0, rng) if kind == 0 else None))
    assert params[8].disp is not None and sum(p.disp is None for p in params) == 6
    got = hip.prepare_batch(dimgs, dlabs, params, crop)
    _check(got, imgs, labs, params, crop)
    for b, p in enumerate(params):
        if p.disp is None:
            alone = data.AugParams(p.origin, p.flip, p.scale, p.shift, p.matrix if p.matrix is not None else IDENT)
            ref = hip.prepare_batch([dimgs[b]], [dlabs[b]], [alone], crop)               # cwf_prepare_batch_affine
            assert torch.equal(got[0][b].view(torch.int32), ref[0][0].view(torch.int32))
            assert torch.equal(got[1][b], ref[1][0]) and torch.equal(got[2][b], ref[2][0])


def test_guard_bands_stride_and_misaligned_outputs(hip):
    """outputs written into views of larger buffers: a sample stride larger than a sample, x starting 4 B past 16-B alignment (per-voxel
    stores) and aligned (16-B stores); the bytes around and between the samples keep their sentinel"""
    from utils import data
    rng = np.random.default_rng(4)
    imgs, labs, dimgs, dlabs = _sources(SHAPES, 5)
    for crop, lead in (((9, 10, 12), 1), ((8, 12, 16), 1), ((8, 12, 16), 4)):
        B, V = 3, crop[0] * crop[1] * crop[2]
        params = [data.AugParams(o, (True, False, True), *_inten(rng, True), matrix=MATRIX if b else None,
                                 disp=E.random_grid((5, 4, 6), 3.0, rng))
                  for b, o in enumerate([(-2, 0, 3), (0, 0, 0), (4, 9, 17)])]
        xs, ts = 4 * V + 2 * lead + 8, V + 2 * lead + 6
        xb = torch.full((B * xs + 64,), -7.5, dtype=torch.float32, device=DEV)
        tb = torch.full((B * ts + 64,), -11, dtype=torch.int64, device=DEV)
        eb = torch.full((B * ts + 64,), -13, dtype=torch.int64, device=DEV)
        x = xb.as_strided((B, 4) + crop, (xs, V, crop[1] * crop[2], crop[2], 1), lead)
        t = tb.as_strided((B,) + crop, (ts, crop[1] * crop[2], crop[2], 1), lead)
        e = eb.as_strided((B,) + crop, (ts, crop[1] * crop[2], crop[2], 1), lead)
        assert x.data_ptr() % 4 == 0 and (x.data_ptr() % 16 != 0) == (lead == 1)
        xr, tr, er = (b.clone() for b in (xb, tb, eb))
        got = hip.prepare_batch(dimgs, dlabs, params, crop, out=(x, t, e))
        assert got[0].data_ptr() == x.data_ptr()
        _check((x, t, e), imgs, labs, params, crop)
        for buf, ref, n, stride in ((xb, xr, 4 * V, xs), (tb, tr, V, ts), (eb, er, V, ts)):
            mask = torch.ones(buf.numel(), dtype=torch.bool, device=DEV)
            for b in range(B):
                mask[lead + b * stride: lead + b * stride + n] = False
            assert torch.equal(buf[mask], ref[mask])


def test_non_finite_control_values(hip, sources):
    """NaN and +-inf in some control points: as the CPU statement, and the voxels they reach are 0 / 0"""
    from utils import data
    imgs, labs, dimgs, dlabs = sources
    crop = (16, 12, 36)
    rng = np.random.default_rng(6)
    disp = E.random_grid((5, 6, 7), 3.0, rng)
    disp[0, 0, 0, 0], disp[1, 2, 3, 4], disp[2, 4, 5, 6], disp[1, 4, 0, 6] = np.nan, np.inf, -np.inf, 3e38
    params = [data.AugParams((2, 3, 1), flip, *_inten(rng, False), matrix=m, disp=disp)
              for flip, m in (((False, False, False), None), ((True, False, True), MATRIX))]
    got = hip.prepare_batch(dimgs[:2], dlabs[:2], params, crop)
    want = _check(got, imgs[:2], labs[:2], params, crop)
    D = data._elastic_disp(params[0], crop)
    bad = ~(np.isfinite(D[0]) & np.isfinite(D[1]) & np.isfinite(D[2]))
    assert 0 < int(bad.sum()) < bad.size
    x, t = got[0][0].cpu().numpy(), got[1][0].cpu().numpy()
    assert not x[:, bad].any() and not t[bad].any() and x[:, ~bad].any() and int((want[1] > 0).sum()) > 0


def test_refusals_launch_nothing(hip, sources):
    """the C entry directly: CWF_E_BADARG (-1), returned before anything is launched (the outputs keep their sentinel)"""
    from cwf import _lib
    imgs, labs, dimgs, dlabs = sources
    img, lab = dimgs[0], dlabs[0]
    V = 8 * 8 * 32
    xb = torch.full((4 * V,), -7.5, dtype=torch.float32, device=DEV)
    t = torch.full((V,), -11, dtype=torch.int64, device=DEV)
    e = torch.full((V,), -13, dtype=torch.int64, device=DEV)
    grid = torch.zeros(3 * 9 * 9 * 9 + 1, dtype=torch.float32, device=DEV)
    stream = torch.cuda.current_stream().cuda_stream

    def call(B=1, samples=True, G=(4, 4, 4), disp=None, **sample):
        smp = (_lib.PrepElasticSample * 1)()
        smp[0].image, smp[0].label = img.data_ptr(), lab.data_ptr()
        smp[0].S0, smp[0].S1, smp[0].S2 = SHAPES[0]
        smp[0].m[:] = [float(v) for v in MATRIX]
        smp[0].disp = grid.data_ptr() if disp is None else disp
        smp[0].G0, smp[0].G1, smp[0].G2 = G
        for k, v in sample.items():
            setattr(smp[0], k, v)
        return hip.lib.cwf_prepare_batch_elastic(smp if samples else None, B, 8, 8, 32, xb.data_ptr(), 4 * V, t.data_ptr(), V,
                                                 e.data_ptr(), V, stream)

    for kw in (dict(G=(3, 4, 4)), dict(G=(4, 9, 4)), dict(G=(4, 4, 3)), dict(G=(9, 9, 9)), dict(G=(4, 4, 0)), dict(G=(-1, 4, 4)),
               dict(disp=grid.data_ptr() + 2), dict(disp=grid.data_ptr() + 1), dict(samples=False), dict(B=0), dict(B=-2),
               dict(image=0), dict(label=0), dict(flip=8), dict(S1=0)):
        assert call(**kw) == -1, kw
    torch.cuda.synchronize()
    assert bool((xb == -7.5).all()) and bool((t == -11).all()) and bool((e == -13).all())
    # G is not looked at without a grid; with one, 4 and 8 are the ends of the range
    assert call(disp=0, G=(0, 0, 99)) == 0 and call(G=(4, 8, 4)) == 0 and call(disp=grid.data_ptr() + 4, G=(8, 8, 8)) == 0
    torch.cuda.synchronize()
    assert not bool((xb == -7.5).any()) and not bool((t == -11).any()) and not bool((e == -13).any())


def test_does_not_synchronise_with_the_host(hip, sources):
    from utils import data
    imgs, labs, dimgs, dlabs = sources
    crop = (16, 16, 32)
    rng = np.random.default_rng(12)
    params = [data.AugParams((3, 4, 5), (True, False, False), *_inten(rng, True), matrix=MATRIX, disp=E.random_grid((7, 7, 7), 4.0, rng)),
              data.AugParams((-2, 10, 6), (False, True, True), disp=E.random_grid((4, 6, 8), 4.0, rng)), data.AugParams((1, 2, 3))]
    out = hip.prepare_batch(dimgs, dlabs, params, crop)          # code object loaded
    torch.cuda.synchronize()
    for o in out:
        o.zero_()
    old = torch.cuda.get_sync_debug_mode()
    try:
        torch.cuda.set_sync_debug_mode("error")
        hip.prepare_batch(dimgs, dlabs, params, crop, out=out)
    finally:
        torch.cuda.set_sync_debug_mode(old)
    _check(out, imgs, labs, params, crop)


def test_device_brats_cached_staged_cpu(hip, tmp_path):
    from utils import data
    rng = np.random.default_rng(7)
    shapes = [(40, 36, 30), (34, 40, 28), (30, 30, 36)]
    for k, S in enumerate(shapes):
        np.savez(tmp_path / ("s%02d.npz" % k), image=E.random_image(S, rng), label=E.blob_labels(S, rng))
    crop = (24, 24, 32)
    kw = dict(seed=21, flip=True, intensity=0.3, rotate=15.0, scale=0.2, elastic=5.0, elastic_grid=6)
    cache = data.DeviceBraTS(str(tmp_path), DEV, crop, **kw)
    staged = data.DeviceBraTS(str(tmp_path), DEV, crop, cache=False, **kw)
    cpu = data.DeviceBraTS(str(tmp_path), "cpu", crop, **kw)
    for epoch in (0, 5):
        for d in (cache, staged, cpu):
            d.set_epoch(epoch)
        assert cache.params(1).disp.shape == (3, 6, 6, 6)
        want = cpu.batch([0, 1, 2])
        got = cache.batch([0, 1, 2])
        for g, w in zip(got, want):
            assert g.is_cuda and torch.equal(g.cpu(), w)
        assert torch.equal(got[0].cpu().view(torch.int32), want[0].view(torch.int32))
        for other in (staged.batch([0, 1, 2]), next(iter(staged.batches([[0, 1, 2]], num_workers=0)))):
            for a, b in zip(other, got):
                assert torch.equal(a, b)
            assert torch.equal(other[0].view(torch.int32), got[0].view(torch.int32))
