"""The intensity stage on the device (csrc/intensity.hip: cwf_augment_intensity behind HipBackend.prepare_batch) against the CPU
statement of utils.data.prepare_batch.  Blurred and noised channels: x as int32 bit patterns, target and edge exactly, on crops of one
tile, ragged tiles, axes shorter than the blur's radius and two whole tiles plus a remainder along every axis, over plain, rotated and
elastically deformed samples.  Gamma-mapped channels: within K ulps of the power (below) of the statement evaluated with a float64
pow.  Then a batch of nine, strided and misaligned outputs with guard bands, the all-off batch, the C entry's refusals, host
synchronisation, and DeviceBraTS cached against staged against the CPU.

K.  |got - ref| <= K * ulp32(y) * r + ulp32(ref), with y = pow(u, gamma) in float64 on the statement's float32 u, r, mn and
ref = y * r + mn.  The largest distance of the device's powf from the float64 pow over u in [0, 1] and gamma in [0.5, 2] was measured
once with tools/intensity_prep_micro.py (the intensity stage): POWF_ULPS.  K is twice that plus one."""
import numpy as np
import pytest
import torch

import elastic_prep_ref as E
import intensity_prep_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F = np.float32
POWF_ULPS = 1.3675
K = 2.0 * POWF_ULPS + 1.0
MATRIX = (0.93, -0.21, 0.08, 0.17, 1.04, -0.12, -0.05, 0.16, 0.88)
SHAPES = [(24, 28, 40), (26, 24, 37), (21, 30, 44), (30, 32, 80)]
FLIPS = [(a, b, c) for a in (False, True) for b in (False, True) for c in (False, True)]
# per-channel mixes: each channel meets blur only, noise only, both and neither
BLURS = [(0.5, 0.0, 1.5, 0.0), (0.0, 1.1, 0.0, 0.8), (1.0, 0.9, 0.0, 0.0), (0.0, 0.0, 0.7, 1.3)]
NOISES = [(0.0, 0.3, 0.2, 0.0), (0.0, 0.05, 1.0, 0.0), (0.4, 0.0, 0.0, 2.0), (0.6, 0.0, 0.1, 0.0)]


def _tile_crop():
    """two whole tiles plus a ragged remainder along every axis: every halo seam is crossed"""
    from cwf import _lib
    t = _lib.INTENSITY_TILE
    return (2 * t[0] + 3, 2 * t[1] + 4, 2 * t[2] + 5)


def _sources(shapes, seed):
    rng = np.random.default_rng(seed)
    imgs = [torch.from_numpy(E.random_image(s, rng)) for s in shapes]
    labs = [torch.from_numpy(E.blob_labels(s, rng)) for s in shapes]
    return imgs, labs, [i.to(DEV) for i in imgs], [l.to(DEV) for l in labs]


@pytest.fixture(scope="module")
def sources():
    return _sources(SHAPES, 2)


def _inten(rng, on):
    return (rng.uniform(0.5, 1.5, 4), rng.uniform(-2, 2, 4)) if on else (None, None)


def _spatial(kind, k, S, crop, rng):
    """(origin, matrix, disp) of a plain (0), rotated (1) or elastically deformed (2) sample"""
    if kind == 0:
        return tuple(int(rng.integers(0, max(s - c, 0) + 1)) for s, c in zip(S, crop)), None, None
    o = tuple(int(rng.integers(-3, max(s - c, 0) + 4)) for s, c in zip(S, crop))
    return o, MATRIX if kind == 1 or k % 2 else None, E.random_grid((4, 5, 7), 3.0, rng) if kind == 2 else None


def _check(got, imgs, labs, params, crop):
    """every channel without gamma bit-equal to the CPU statement, target and edge exactly; gamma-mapped channels within K"""
    from utils import data
    want = data.prepare_batch(imgs, labs, params, crop)
    x, t, e = (g.cpu() for g in got)
    assert x.dtype == torch.float32 and t.dtype == torch.int64 and e.dtype == torch.int64
    assert torch.equal(t, want[1]) and torch.equal(e, want[2])
    worst = 0.0
    for b, p in enumerate(params):
        mapped = [c for c in range(4) if p.gamma is not None and p.gamma[c] > 0.0]
        pre = None
        if mapped:
            q = data.AugParams(p.origin, p.flip, p.scale, p.shift, p.matrix, p.disp, blur=p.blur, noise=p.noise, noise_key=p.noise_key)
            pre = data.prepare_batch([imgs[b]], [labs[b]], [q], crop)[0][0].numpy()
        for c in range(4):
            g = x[b, c].numpy()
            if c not in mapped or R.gamma_parts(pre[c])[1] is None:
                assert np.array_equal(g.view(np.int32), want[0][b, c].numpy().view(np.int32)), (b, c)
                continue
            y, ref, r = R.gamma64(pre[c], p.gamma[c])
            err = np.abs(g.astype(np.float64) - ref)
            worst = max(worst, float(np.max((err - R.ulp32(ref)) / (R.ulp32(y) * r))))
            assert np.all(err <= K * R.ulp32(y) * r + R.ulp32(ref)), (b, c, worst)
    return want, worst


def _crops():
    return [(8, 8, 32), (9, 10, 35), (20, 12, 40), (1, 1, 7), (2, 3, 5), _tile_crop()]


@pytest.mark.parametrize("ci", range(6))
def test_bit_equal_blur_and_noise(hip, sources, ci):
    from utils import data
    crop = _crops()[ci]
    imgs, labs, dimgs, dlabs = sources
    rng = np.random.default_rng(40 + ci)
    changed = 0
    for kind in (0, 1, 2):
        sel, params = [], []
        for k in range(4):
            s = 3 if ci == 5 else (k + kind) % 3
            o, m, disp = _spatial(kind, k, SHAPES[s], crop, rng)
            sel.append(s)
            params.append(data.AugParams(o, FLIPS[(3 * k + kind + ci) % 8], *_inten(rng, (k + kind) % 2 == 0), matrix=m, disp=disp,
                                         blur=BLURS[(k + kind) % 4], noise=NOISES[k], noise_key=int(rng.integers(0, 2 ** 63))))
        got = hip.prepare_batch([dimgs[s] for s in sel], [dlabs[s] for s in sel], params, crop)
        want, _ = _check(got, [imgs[s] for s in sel], [labs[s] for s in sel], params, crop)
        off = [data.AugParams(p.origin, p.flip, p.scale, p.shift, p.matrix, p.disp) for p in params]
        base = hip.prepare_batch([dimgs[s] for s in sel], [dlabs[s] for s in sel], off, crop)
        for b, p in enumerate(params):
            for c in range(4):
                same = torch.equal(got[0][b, c].view(torch.int32), base[0][b, c].view(torch.int32))
                if p.blur[c] == 0.0 and p.noise[c] == 0.0:
                    assert same, (b, c)
                changed += not same
    assert changed >= 12


@pytest.mark.parametrize("ci", [1, 5])
def test_gamma_mapped_channels_bounded(hip, sources, ci):
    """gamma alone, after a blur, after noise and after both, exponents over [0.5, 2]; a constant channel stays as it is; the
    channels of the same batch with gamma off stay bit-equal"""
    from utils import data
    crop = _crops()[ci]
    imgs, labs, dimgs, dlabs = sources
    rng = np.random.default_rng(60 + ci)
    sel, params = [], []
    gammas = [(0.5, 0.0, 2.0, 1.0), (0.0, 1.3, 0.0, 0.75), (1.9, 0.6, 1.1, 0.0), (0.9, 0.0, 0.0, 1.6)]
    for k in range(4):
        s = 3 if ci == 5 else k % 3
        o, m, disp = _spatial(k % 3, k, SHAPES[s], crop, rng)
        scale, shift = _inten(rng, k % 2 == 1)
        if k == 3:
            scale, shift = (1.0, 1.0, 1.0, 0.0), (0.0, 0.0, 0.0, 2.5)        # channel 3 is constant: its gamma does nothing
        sel.append(s)
        params.append(data.AugParams(o, FLIPS[(k + ci) % 8], scale, shift, matrix=m, disp=disp, blur=BLURS[k], noise=NOISES[(k + 1) % 4],
                                     noise_key=int(rng.integers(0, 2 ** 63)), gamma=gammas[k]))
    got = hip.prepare_batch([dimgs[s] for s in sel], [dlabs[s] for s in sel], params, crop)
    _, worst = _check(got, [imgs[s] for s in sel], [labs[s] for s in sel], params, crop)
    print("gamma: largest (|got - ref| - ulp32(ref)) / (ulp32(y) * r) = %.3f, K = %.1f" % (worst, K))
    const = got[0][3, 3].cpu()
    assert bool((const == const.reshape(-1)[0]).all()) and abs(float(const.reshape(-1)[0]) - 2.5) < 1e-5 and worst > 0.0 and K <= 16.0
    again = hip.prepare_batch([dimgs[s] for s in sel], [dlabs[s] for s in sel], params, crop)
    assert torch.equal(again[0].view(torch.int32), got[0].view(torch.int32))                 # the device repeats itself bit for bit


def test_batch_of_nine_mixed_samples(hip):
    """two launches of the stage, the second with one sample; samples with blur, with noise, with gamma, with several and with
    nothing.  Those with nothing on equal the same call without the stage, bit for bit."""
    from utils import data
    rng = np.random.default_rng(9)
    crop = (12, 13, 36)
    shapes = [SHAPES[b % 3] for b in range(9)]
    imgs, labs, dimgs, dlabs = _sources(shapes, 19)
    params, plain = [], []
    for b, S in enumerate(shapes):
        o, m, disp = _spatial(b % 3, b, S, crop, rng)
        kw = [dict(), dict(blur=BLURS[b % 4]), dict(noise=NOISES[b % 4], noise_key=b + 1), dict(gamma=(0.0, 0.7, 1.4, 0.0)),
              dict(blur=BLURS[b % 4], noise=NOISES[(b + 1) % 4], noise_key=2 ** 63 - 1, gamma=(1.2, 0.0, 0.0, 0.8))][b % 5]
        if b == 7:
            kw = dict(blur=(0, 0, 0, 0), noise=(0, 0, 0, 0), gamma=(0, 0, 0, 0))
        sc, sh = _inten(rng, b % 2 == 0)
        params.append(data.AugParams(o, FLIPS[b % 8], sc, sh, matrix=m, disp=disp, **kw))
        plain.append(data.AugParams(o, FLIPS[b % 8], sc, sh, matrix=m, disp=disp))
    assert [p.intensity_stage() for p in params] == [False, True, True, True, True, False, True, False, True]
    got = hip.prepare_batch(dimgs, dlabs, params, crop)
    _check(got, imgs, labs, params, crop)
    ref = hip.prepare_batch(dimgs, dlabs, plain, crop)
    for b in (0, 5, 7):
        assert torch.equal(got[0][b].view(torch.int32), ref[0][b].view(torch.int32))
    assert torch.equal(got[1], ref[1]) and torch.equal(got[2], ref[2])


@pytest.mark.parametrize("blur", [True, False])
def test_guard_bands_stride_and_misaligned_outputs(hip, blur):
    """x written into views of larger buffers, with a sample stride larger than a sample, 4 B past 16-B alignment and aligned; with a
    blur (the prepare kernel writes a workspace, the stage writes the view) and without (the stage runs in place on the view).  The
    bytes around and between the samples keep their sentinel."""
    from utils import data
    rng = np.random.default_rng(4)
    imgs, labs, dimgs, dlabs = _sources(SHAPES[:3], 5)
    for crop, lead in (((9, 11, 13), 1), ((8, 12, 16), 1), ((8, 12, 16), 4)):
        B, V = 3, crop[0] * crop[1] * crop[2]
        params = []
        for b, o in enumerate([(2, 0, 3), (0, 0, 0), (4, 9, 17)]):          # (sample 0 is a plain crop: its origin lies in range)
            params.append(data.AugParams(o, (True, False, True), *_inten(rng, True), matrix=MATRIX if b else None,
                                         blur=BLURS[b] if blur and b != 1 else None, noise=NOISES[b + 1], noise_key=b,
                                         gamma=(0.0, 0.0, 1.5, 0.0) if b == 2 else None))
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


def test_all_off_batch_takes_the_parent_path(hip, sources, monkeypatch):
    from utils import data
    imgs, labs, dimgs, dlabs = sources
    crop = (9, 10, 35)
    rng = np.random.default_rng(14)
    base = [data.AugParams((1, 2, 3), (True, False, False), *_inten(rng, True)), data.AugParams((0, 0, 0)),
            data.AugParams((2, 0, 1), (False, True, True), matrix=MATRIX)]
    off = [data.AugParams(p.origin, p.flip, p.scale, p.shift, p.matrix, blur=(0, 0, 0, 0), noise=(0, 0, 0, 0) if k else None,
                          noise_key=77, gamma=(0, 0, 0, 0) if k != 1 else None) for k, p in enumerate(base)]
    want = hip.prepare_batch(dimgs[:3], dlabs[:3], base, crop)
    calls = []
    real = type(hip)._call

    def counting(self, name, *args):
        calls.append(name)
        return real(self, name, *args)

    monkeypatch.setattr(type(hip), "_call", counting)
    got = hip.prepare_batch(dimgs[:3], dlabs[:3], off, crop)
    assert calls == ["cwf_prepare_batch_affine"]
    on = hip.prepare_batch(dimgs[:3], dlabs[:3], off[:2] + [data.AugParams((2, 0, 1), noise=(0, 0, 0, 0.1))], crop)
    assert calls == ["cwf_prepare_batch_affine", "cwf_prepare_batch", "cwf_augment_intensity"]
    assert torch.equal(got[0].view(torch.int32), want[0].view(torch.int32)) and torch.equal(got[1], want[1]) and torch.equal(got[2], want[2])
    assert not torch.equal(on[0][2, 3], got[0][2, 3])


def test_refusals_launch_nothing(hip):
    """the C entry directly: CWF_E_BADARG (-1) before anything is launched (the output keeps its sentinel); the ends of the ranges
    are accepted"""
    from cwf import _lib
    from utils import data
    crop = (4, 5, 9)
    V = crop[0] * crop[1] * crop[2]
    src = torch.randn(2 * 4 * V + 4, device=DEV)
    dst = torch.full((2 * 4 * V + 4,), -7.5, dtype=torch.float32, device=DEV)
    nws = _lib.intensity_ws_floats(2, crop)
    assert nws == 16
    ws = torch.zeros(nws + 1, device=DEV)
    stream = torch.cuda.current_stream().cuda_stream
    inf, nan = float("inf"), float("nan")

    def call(B=2, samples=True, s=None, d=None, sbs=4 * V, dbs=4 * V, w=None, nw=nws, taps=None, amp=None, which=(1,), **field):
        smp = (_lib.IntensitySample * 2)()
        for k in range(2):
            for c in range(4):
                smp[k].taps[c][:] = [float(v) for v in data.blur_taps(1.0)]
            smp[k].blur, smp[k].noise, smp[k].gam, smp[k].key = 5, 3, 9, 2 ** 63 - 1
            smp[k].amp[:] = [0.5, 0.0, 0.25, 1.0]
            smp[k].gamma[:] = [1.5, -1.0, nan, 0.5]              # channels 1 and 2 are off: not looked at
        if taps is not None:
            smp[1].taps[taps[0]][taps[1]] = taps[2]
        if amp is not None:
            smp[1].amp[amp[0]] = amp[1]
        for b in which:
            for k, v in field.items():
                if k == "gamma":
                    smp[b].gamma[v[0]] = v[1]
                else:
                    setattr(smp[b], k, v)
        return hip.lib.cwf_augment_intensity(smp if samples else None, B, crop[0], crop[1], crop[2],
                                             src.data_ptr() if s is None else s, sbs, dst.data_ptr() if d is None else d, dbs,
                                             ws.data_ptr() if w is None else w, nw, stream)

    bad = [dict(taps=(0, 3, nan)), dict(taps=(3, 6, inf)), dict(taps=(1, 0, -inf)), dict(amp=(0, nan)), dict(amp=(1, inf)),
           dict(amp=(2, -0.5)), dict(amp=(1, -1e-30)), dict(gamma=(0, 0.0)), dict(gamma=(3, -1.0)), dict(gamma=(0, inf)),
           dict(gamma=(3, nan)), dict(samples=False), dict(B=0), dict(B=-1), dict(s=0), dict(d=0), dict(s=src.data_ptr() + 2),
           dict(d=dst.data_ptr() + 1), dict(w=0), dict(w=ws.data_ptr() + 2), dict(nw=nws - 1), dict(blur=16), dict(noise=-1),
           dict(gam=31), dict(gam=15), dict(gam=13), dict(sbs=4 * V - 1), dict(dbs=4 * V - 1), dict(d=src.data_ptr()), dict(d=src.data_ptr() + 4 * V)]
    for kw in bad:
        assert call(**kw) == -1, kw
    torch.cuda.synchronize()
    assert bool((dst == -7.5).all())
    ok = [dict(), dict(amp=(0, 0.0)), dict(blur=15, noise=15, gam=0), dict(gamma=(0, 1e-30)), dict(gamma=(3, 3e38)), dict(B=1),
          dict(s=src.data_ptr() + 4, d=dst.data_ptr() + 4), dict(which=(0, 1), blur=0, noise=0, gam=0, w=0, nw=0)]
    for kw in ok:
        assert call(**kw) == 0, kw
    torch.cuda.synchronize()
    assert not bool((dst[1:8 * V] == -7.5).any())
    # in place is accepted only without a blur
    x = torch.randn(2 * 4 * V, device=DEV)
    keep = x.clone()
    assert call(s=x.data_ptr(), d=x.data_ptr()) == -1
    torch.cuda.synchronize()
    assert torch.equal(x, keep)
    assert call(s=x.data_ptr(), d=x.data_ptr(), blur=0) == -1           # (sample 0 still has its blur bits)
    torch.cuda.synchronize()
    assert torch.equal(x, keep)
    assert call(s=x.data_ptr(), d=x.data_ptr(), blur=0, which=(0, 1)) == 0
    torch.cuda.synchronize()
    assert not torch.equal(x[:V], keep[:V]) and torch.equal(x[V:2 * V], keep[V:2 * V])      # channel 0 has noise, channel 1 nothing


def test_does_not_synchronise_with_the_host(hip, sources):
    from utils import data
    imgs, labs, dimgs, dlabs = sources
    crop = (16, 16, 32)
    rng = np.random.default_rng(12)
    params = [data.AugParams((3, 4, 5), (True, False, False), *_inten(rng, True), matrix=MATRIX, disp=E.random_grid((7, 7, 7), 4.0, rng),
                             blur=BLURS[0], noise=NOISES[0], noise_key=5, gamma=(1.3, 0, 0, 0.8)),
              data.AugParams((-2, 10, 6), (False, True, True), matrix=MATRIX, noise=NOISES[1], noise_key=6), data.AugParams((1, 2, 3))]
    inplace = [data.AugParams(p.origin, p.flip, p.scale, p.shift, p.matrix, p.disp, noise=p.noise, noise_key=p.noise_key, gamma=p.gamma)
               for p in params]
    for ps in (params, inplace):
        out = hip.prepare_batch(dimgs[:3], dlabs[:3], ps, crop)          # code object loaded
        torch.cuda.synchronize()
        for o in out:
            o.zero_()
        old = torch.cuda.get_sync_debug_mode()
        try:
            torch.cuda.set_sync_debug_mode("error")
            hip.prepare_batch(dimgs[:3], dlabs[:3], ps, crop, out=out)
        finally:
            torch.cuda.set_sync_debug_mode(old)
        _check(out, imgs[:3], labs[:3], ps, crop)


def test_device_brats_cached_staged_cpu(hip, tmp_path):
    from utils import data
    rng = np.random.default_rng(7)
    shapes = [(40, 36, 30), (34, 40, 28), (30, 30, 36)]
    for k, S in enumerate(shapes):
        np.savez(tmp_path / ("s%02d.npz" % k), image=E.random_image(S, rng), label=E.blob_labels(S, rng))
    crop = (24, 24, 32)
    for gamma in (0.4, 0.0):
        kw = dict(seed=21, flip=True, intensity=0.3, rotate=15.0, scale=0.2, elastic=5.0, elastic_grid=6, blur=1.5, noise=0.3, gamma=gamma)
        cache = data.DeviceBraTS(str(tmp_path), DEV, crop, **kw)
        staged = data.DeviceBraTS(str(tmp_path), DEV, crop, cache=False, **kw)
        cpu = data.DeviceBraTS(str(tmp_path), "cpu", crop, **kw)
        on = set()
        for epoch in (0, 5):
            for d in (cache, staged, cpu):
                d.set_epoch(epoch)
            got = cache.batch([0, 1, 2])
            for i in range(3):
                p = cache.params(i)
                on.update(k for k in ("blur", "noise", "gamma") if getattr(p, k) is not None and any(v > 0 for v in getattr(p, k)))
            for other in (staged.batch([0, 1, 2]), next(iter(staged.batches([[0, 1, 2]], num_workers=0)))):
                for a, b in zip(other, got):
                    assert torch.equal(a, b)
                assert torch.equal(other[0].view(torch.int32), got[0].view(torch.int32))
            if gamma == 0.0:
                want = cpu.batch([0, 1, 2])
                for g, w in zip(got, want):
                    assert g.is_cuda and torch.equal(g.cpu(), w)
                assert torch.equal(got[0].cpu().view(torch.int32), want[0].view(torch.int32))
        assert on == ({"blur", "noise", "gamma"} if gamma else {"blur", "noise"})
