"""The acquisition stage on the device (csrc/acquire.hip: cwf_augment_acquisition behind HipBackend.prepare_batch) against the CPU
statement of utils.data.prepare_batch.  Bias-field and low-resolution channels: x as int32 bit patterns, target and edge exactly.
Contrast-mapped channels: bit-equal where the float64 sum of the channel is exact in every order, within E (below) otherwise.  Then
everything at once with the resampling in front and the intensity stage behind, the workload's own shape, strided outputs with guard
bands, the all-off batch, the C entry's refusals, and DeviceBraTS cached against staged.

E, the contrast bound, derived and not measured (u = 2^-24; eps = 2^-53).  The device and the statement see the same channel x (the
bias step before is bit-equal) and differ only in the order of the float64 sum S of its V values.
  the means.  Every order of a float64 sum of V terms is within V * eps * sum|x| of the exact sum, so the two sums are at most twice
    that apart, and the two quotients S / V at most d = 2 * eps * sum|x| + 2 * eps * |S / V| apart (one rounding each).  Two float64
    numbers d apart round to float32 numbers at most d + ulp32 apart: D = |mean_dev - mean| <= d + ulp32(mean) (two ulps at a binade
    edge: ulp32 is taken at |mean| + d).
  the map.  y = fl(fl(fl(x - m) * f) + m) = ((x - m)(1 + d1) f (1 + d2) + m)(1 + d3), |d_i| <= u, against h(m) = (x - m) f + m:
    |y - h(m)| <= (2u + u^2)(1 + u) f |x - m| + u |h(m)|.  The exact values differ by |h(m_dev) - h(m)| = |1 - f| D.  With a = |x - m| + D
    (which bounds both |x - m| and |x - m_dev|) and |h| <= (|y| + 2.01 u f a) / (1 - u) on either side:
        E = |1 - f| D (1 + 2.1u) + 4.1 u f a + 2.1 u |y|        per voxel, y the statement's value before the clamp.
  the clamp.  mn and mx are taken from the same bits on both sides and min / max are 1-Lipschitz, so E holds after the clamp too.
Where a low-resolution step follows, each of the three lerps fl(a + fl(t fl(b - a))) is within 5 u M of the exact convex
combination (M the largest magnitude in the channel), which carries an input error through unchanged: E_low = max E + 2 * 3 * 5 u M.
Where the intensity stage follows (blur, noise: sums of products with non-negative weights and an added constant, every one of them
monotone non-decreasing in its inputs, as rounding is), the device output lies between the stage applied to the statement's
acquisition output lowered and raised by the bound."""
import numpy as np
import pytest
import torch

import acquisition_prep_ref as A
import elastic_prep_ref as E
import intensity_prep_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F = np.float32
U = 2.0 ** -24
EPS = 2.0 ** -53
POWF_ULPS = 1.3675                  # tests/test_intensity_prepare_gpu.py: the existing gamma bound, not widened
K = 2.0 * POWF_ULPS + 1.0
MATRIX = (0.93, -0.21, 0.08, 0.17, 1.04, -0.12, -0.05, 0.16, 0.88)
SHAPES = [(24, 28, 44), (40, 36, 42), (36, 30, 48)]
CROPS = [(12, 11, 37), (1, 9, 40), (33, 10, 10), (32, 32, 32)]
GRID = (4, 6, 8)
Z_FULL = 0.99                       # the crop's own lattice for every extent up to 50


def _sources(shapes, seed):
    rng = np.random.default_rng(seed)
    imgs = [torch.from_numpy(E.random_image(s, rng)) for s in shapes]
    labs = [torch.from_numpy(E.blob_labels(s, rng)) for s in shapes]
    return imgs, labs, [i.to(DEV) for i in imgs], [l.to(DEV) for l in labs]


@pytest.fixture(scope="module")
def sources():
    return _sources(SHAPES, 3)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _down(a):
    return np.nextafter(a.astype(F), F(-np.inf))


def _up(a):
    return np.nextafter(a.astype(F), F(np.inf))


def contrast_bound(x, f):
    """(E per voxel float64, mn, mx) for the contrast step with factor f on the channel x (float32, finite)"""
    x64 = x.astype(np.float64)
    V = x.size
    mean, mn, mx = A.contrast_parts(x)
    d = 2.0 * EPS * float(np.abs(x64).sum()) + 2.0 * EPS * abs(float(x64.sum()) / V)
    D = d + float(A.ulp32(abs(float(mean)) + d))
    f = float(F(f))
    y = (((x - mean) * F(f)) + mean).astype(np.float64)            # the statement's value before the clamp
    a = np.abs(x64 - float(mean)) + D
    return abs(1.0 - f) * D * (1 + 2.1 * U) + 4.1 * U * f * a + 2.1 * U * np.abs(y), mn, mx


def _check(got, imgs, labs, params, crop):
    """target and edge exactly; channels with neither contrast nor gamma bit-equal to the CPU statement; gamma-mapped channels (their
    contrast is off) within the existing K; contrast-mapped channels between the intensity stage of the statement's acquisition
    output lowered and raised by the bound.  Returns the largest |device - statement| / E over the contrast-mapped voxels that neither
    a low-resolution step nor the intensity stage follows."""
    from utils import data
    want = data.prepare_batch(imgs, labs, params, crop)
    x, t, e = (g.cpu() for g in got)
    assert x.dtype == torch.float32 and torch.equal(t, want[1]) and torch.equal(e, want[2])
    worst = 0.0
    for b, p in enumerate(params):
        con = [c for c in range(4) if p.contrast is not None and p.contrast[c] > 0.0]
        gam = [c for c in range(4) if p.gamma is not None and p.gamma[c] > 0.0]
        assert not set(con) & set(gam)
        for c in range(4):
            if c not in con and c not in gam:
                assert np.array_equal(x[b, c].numpy().view(np.int32), want[0][b, c].numpy().view(np.int32)), (b, c)
        if not con and not gam:
            continue
        x0 = data.prepare_batch([imgs[b]], [labs[b]], [data.AugParams(p.origin, p.flip, p.scale, p.shift, p.matrix, p.disp)], crop)[0][0].numpy()
        acq = data._acquisition_stage_cpu(x0.copy(), p) if p.acquisition_stage() else x0
        if gam:
            pre = data._intensity_stage_cpu(acq.copy(), data.AugParams((0, 0, 0), blur=p.blur, noise=p.noise, noise_key=p.noise_key))
            for c in gam:
                g = x[b, c].numpy()
                if R.gamma_parts(pre[c])[1] is None:
                    assert np.array_equal(g.view(np.int32), want[0][b, c].numpy().view(np.int32)), (b, c)
                    continue
                y, ref, r = R.gamma64(pre[c], p.gamma[c])
                assert np.all(np.abs(g.astype(np.float64) - ref) <= K * R.ulp32(y) * r + R.ulp32(ref)), (b, c)
        if not con:
            continue
        lo, hi = acq.copy(), acq.copy()
        for c in con:
            xb = x0[c] * data.bias_field(p.bias[c], crop) if p.bias_mask[c] else x0[c]
            Ev, mn, mx = contrast_bound(xb, p.contrast[c])
            Emax = float(Ev.max())
            low = p.lowres is not None and p.lowres[c] > 0.0
            if low:
                Emax += 2 * 3 * 5 * U * float(np.abs(xb).max())
            Ef = np.nextafter(F(Emax), F(np.inf))
            lo[c], hi[c] = _down(acq[c] - Ef), _up(acq[c] + Ef)
            if not low and not p.intensity_stage():               # the per-voxel bound, and the clamp limits bit for bit
                g = x[b, c].numpy()
                err = np.abs(g.astype(np.float64) - acq[c].astype(np.float64))
                assert np.all(err <= Ev), (b, c, float((err / Ev).max()))
                worst = max(worst, float((err / Ev).max()))
                assert float(g.min()) >= float(mn) and float(g.max()) <= float(mx)
                if p.contrast[c] > 1.0:
                    assert g.min().view(np.int32) == mn.view(np.int32) and g.max().view(np.int32) == mx.view(np.int32)
        if p.intensity_stage():
            off = data.AugParams((0, 0, 0), blur=p.blur, noise=p.noise, noise_key=p.noise_key)   # (a contrast channel has no gamma)
            lo, hi = data._intensity_stage_cpu(lo, off), data._intensity_stage_cpu(hi, off)
        for c in con:
            g = x[b, c].numpy()
            assert np.all(lo[c] <= g) and np.all(g <= hi[c]), (b, c)
    return want, worst


def _spatial(kind, S, crop, rng):
    """(origin, matrix, disp) of a plain (0), rotated (1) or elastically deformed (2) sample"""
    if kind == 0:
        return tuple(int(rng.integers(0, max(s - c, 0) + 1)) for s, c in zip(S, crop)), None, None
    o = tuple(int(rng.integers(-3, max(s - c, 0) + 4)) for s, c in zip(S, crop))
    return o, MATRIX, E.random_grid((4, 5, 7), 3.0, rng) if kind == 2 else None


BIAS_MASKS = [(True, False, True, False), (False, True, True, False), (True, True, False, True)]
ZOOMS = [(0.5, 0.0, 0.73, 0.0), (0.0, Z_FULL, 0.6, 0.0), (0.9, 0.5, 0.0, 0.55)]


@pytest.mark.parametrize("crop", CROPS)
def test_bias_and_lowres_bit_equal(hip, sources, crop):
    """three samples with different masks: every channel meets bias only, lowres only, both and neither; z = 0.5, the crop's own
    lattice and lattices in between; a plain, a rotated and an elastically deformed crop in front"""
    from utils import data
    imgs, labs, dimgs, dlabs = sources
    rng = np.random.default_rng(sum(crop))
    params = []
    for k in range(3):
        o, m, disp = _spatial(k, SHAPES[k], crop, rng)
        params.append(data.AugParams(o, (k == 1, k == 0, k == 2), matrix=m, disp=disp, bias=A.random_bias(GRID, rng),
                                     bias_mask=BIAS_MASKS[k], lowres=ZOOMS[k]))
    got = hip.prepare_batch(dimgs, dlabs, params, crop)
    want, _ = _check(got, imgs, labs, params, crop)
    base = hip.prepare_batch(dimgs, dlabs, [data.AugParams(p.origin, p.flip, matrix=p.matrix, disp=p.disp) for p in params], crop)
    for b, p in enumerate(params):
        for c in range(4):
            same = torch.equal(_bits(got[0][b, c]), _bits(base[0][b, c]))
            assert same or p.bias_mask[c] or p.lowres[c] > 0.0
            if not p.bias_mask[c] and p.lowres[c] == 0.0:
                assert same
    # the stage alone, one transform at a time
    for kw in (dict(bias=params[0].bias, bias_mask=(True,) * 4), dict(lowres=(0.5, 0.5, 0.8, Z_FULL))):
        one = [data.AugParams(params[0].origin, **kw)]
        _check(hip.prepare_batch(dimgs[:1], dlabs[:1], one, crop), imgs[:1], labs[:1], one, crop)


def test_batch_of_nine_two_launches(hip):
    from utils import data
    rng = np.random.default_rng(9)
    crop = (12, 11, 37)
    shapes = [SHAPES[b % 3] for b in range(9)]
    imgs, labs, dimgs, dlabs = _sources(shapes, 19)
    params = []
    for b, S in enumerate(shapes):
        o, m, disp = _spatial(b % 3, S, crop, rng)
        kw = dict(bias=A.random_bias((4 + b % 5, 4 + (b + 2) % 5, 4 + (b + 4) % 5), rng), bias_mask=BIAS_MASKS[b % 3], lowres=ZOOMS[(b + 1) % 3])
        if b == 4:
            kw = dict(bias=kw["bias"], bias_mask=(False,) * 4, contrast=(0, 0, 0, 0), lowres=(0, 0, 0, 0))         # every mask zero
        if b == 6:
            kw = dict()
        if b == 8:
            kw = dict(lowres=(0.0, 0.0, 0.0, 0.5))                                                    # the second launch: gather only
        params.append(data.AugParams(o, (b % 2 == 0, b % 3 == 0, b % 5 == 0), matrix=m, disp=disp, **kw))
    got = hip.prepare_batch(dimgs, dlabs, params, crop)
    _check(got, imgs, labs, params, crop)
    plain = hip.prepare_batch(dimgs, dlabs, [data.AugParams(p.origin, p.flip, matrix=p.matrix, disp=p.disp) for p in params], crop)
    for b in (4, 6):
        assert torch.equal(_bits(got[0][b]), _bits(plain[0][b]))


def _summable_sources(shapes, rng):
    """images of integers in [-512, 512] divided by 64: every partial sum of up to 2^31 of them is exact in float64"""
    imgs = [torch.from_numpy((rng.integers(-512, 513, (4,) + s) / 64.0).astype(F)) for s in shapes]
    labs = [torch.from_numpy(E.blob_labels(s, rng)) for s in shapes]
    return imgs, labs


@pytest.mark.parametrize("crop", [(12, 11, 37), (33, 10, 10), (32, 32, 32)])
def test_contrast_bit_equal_on_exactly_summable_input(hip, crop):
    from utils import data
    rng = np.random.default_rng(31 + sum(crop))
    shapes = [tuple(c + 4 for c in crop)] * 2
    imgs, labs = _summable_sources(shapes, rng)
    imgs[0][2] = -3.25                                            # a constant channel: mn == mx
    imgs[1][3, 2, 3, 4] = float("nan")                            # a NaN voxel inside the crop: the channel is left alone
    dimgs, dlabs = [i.to(DEV) for i in imgs], [l.to(DEV) for l in labs]
    params = [data.AugParams((1, 2, 3), (True, False, False), contrast=(0.75, 1.25, 1.25, 0.0)),
              data.AugParams((0, 1, 2), (False, True, True), contrast=(1.25, 0.0, 0.75, 0.75), lowres=(0.0, 0.0, 0.6, 0.0))]
    got = hip.prepare_batch(dimgs, dlabs, params, crop)
    want = data.prepare_batch(imgs, labs, params, crop)
    assert torch.equal(_bits(got[0].cpu()), _bits(want[0])) and torch.equal(got[1].cpu(), want[1]) and torch.equal(got[2].cpu(), want[2])
    plain = data.prepare_batch(imgs, labs, [data.AugParams(p.origin, p.flip) for p in params], crop)[0]
    assert torch.equal(_bits(want[0][0, 2]), _bits(plain[0, 2])) and torch.equal(_bits(want[0][1, 3]), _bits(plain[1, 3]))
    assert bool(torch.isnan(plain[1, 3]).any())
    for b, c in ((0, 1), (1, 0)):                                 # f = 1.25: the clamp is active
        assert float(want[0][b, c].max()) == float(plain[b, c].max()) and int((want[0][b, c] == plain[b, c].max()).sum()) > 1
        assert not torch.equal(want[0][b, c], plain[b, c])


@pytest.mark.parametrize("crop", [(12, 11, 37), (32, 32, 32)])
def test_contrast_on_generic_input_is_bounded_and_repeats(hip, sources, crop):
    from utils import data
    imgs, labs, dimgs, dlabs = sources
    rng = np.random.default_rng(50 + sum(crop))
    params = []
    for k in range(3):
        o, m, disp = _spatial(k, SHAPES[k], crop, rng)
        sc, sh = rng.uniform(0.5, 1.5, 4), rng.uniform(-2, 2, 4)
        params.append(data.AugParams(o, (k == 0, k == 1, k == 2), sc, sh, matrix=m, disp=disp, bias=A.random_bias(GRID, rng),
                                     bias_mask=[(True, True, False, True), (True, False, True, True), (False, True, True, True)][k],
                                     contrast=[(1.25, 0.75, 1.4, 0.0), (0.6, 1.3, 0.0, 1.1), (1.5, 1.0, 0.9, 1.2)][k]))
    got = hip.prepare_batch(dimgs, dlabs, params, crop)
    _, worst = _check(got, imgs, labs, params, crop)
    print("contrast: largest |device - statement| / E = %.3g" % worst)
    assert worst <= 1.0
    again = hip.prepare_batch(dimgs, dlabs, params, crop)
    assert torch.equal(_bits(again[0]), _bits(got[0]))                                          # the same bits on every run


def _everything(crop, rng, shapes, affine=True, blur=True):
    """two samples with all three new transforms and blur, noise and gamma; gamma only where the contrast is off"""
    from utils import data
    params = []
    for k in range(2):
        o, m, disp = _spatial(2 if affine else 0, shapes[k], crop, rng)
        sc, sh = rng.uniform(0.5, 1.5, 4), rng.uniform(-2, 2, 4)
        params.append(data.AugParams(o, (k == 0, True, k == 1), sc, sh, matrix=m, disp=disp, bias=A.random_bias(GRID, rng),
                                     bias_mask=[(True, True, False, True), (False, True, True, True)][k],
                                     contrast=[(1.25, 0.0, 0.8, 0.0), (0.0, 1.3, 0.0, 0.7)][k],
                                     lowres=[(0.5, 0.7, 0.0, 0.0), (0.6, 0.0, 0.5, Z_FULL)][k],
                                     blur=[(1.0, 0.0, 0.0, 0.7), (0.0, 1.2, 0.0, 0.0)][k] if blur else None,
                                     noise=[(0.0, 0.1, 0.2, 0.0), (0.1, 0.2, 0.0, 0.0)][k], noise_key=1234 + k,
                                     gamma=[(0.0, 1.3, 0.0, 0.8), (0.7, 0.0, 1.5, 0.0)][k]))
    return params


def test_everything_at_once(hip, sources):
    imgs, labs, dimgs, dlabs = sources
    crop = (32, 32, 32)
    params = _everything(crop, np.random.default_rng(77), SHAPES[1:])
    got = hip.prepare_batch(dimgs[1:], dlabs[1:], params, crop)
    _check(got, imgs[1:], labs[1:], params, crop)


def _workload_case():
    crop = (128, 128, 128)
    shapes = [(132, 130, 136), (130, 136, 129)]
    rng = np.random.default_rng(128)
    imgs = [torch.from_numpy((rng.standard_normal((4,) + s, dtype=F) * F(2.0) + F(0.5))) for s in shapes]
    labs = [torch.from_numpy((rng.random(s) < 0.1).astype(np.uint8)) for s in shapes]
    return imgs, labs, _everything(crop, rng, shapes, affine=False, blur=False), crop


def test_the_workloads_own_shape(hip):
    """128^3, B = 2, the three transforms on with noise and gamma behind them, from plain crops (the resampled crop and the blur at
    this size belong to their own tests: their CPU statements take most of a minute here)"""
    imgs, labs, params, crop = _workload_case()
    got = hip.prepare_batch([i.to(DEV) for i in imgs], [l.to(DEV) for l in labs], params, crop)
    _check(got, imgs, labs, params, crop)


@pytest.mark.parametrize("lowres", [True, False])
def test_guard_bands_and_sample_stride(hip, sources, lowres):
    """x written through out= into views of larger buffers whose sample stride exceeds a sample, 4 B past 16-B alignment: with a
    lowres bit (the prepare kernel writes a workspace, the gather writes the view) and without (the stage runs in place on the view)"""
    from utils import data
    imgs, labs, dimgs, dlabs = sources
    rng = np.random.default_rng(4)
    crop, lead = (9, 11, 13), 1
    B, V = 3, crop[0] * crop[1] * crop[2]
    params = [data.AugParams(o, (True, False, True), matrix=MATRIX if b else None, bias=A.random_bias(GRID, rng),
                             bias_mask=BIAS_MASKS[b], contrast=(0.0, 0.0, 0.0, 1.2), lowres=ZOOMS[b] if lowres and b != 1 else None,
                             noise=(0.1, 0.0, 0.0, 0.0), noise_key=b)
              for b, o in enumerate([(2, 0, 3), (0, 0, 0), (4, 9, 17)])]
    xs, ts = 4 * V + 2 * lead + 8, V + 2 * lead + 6
    xb = torch.full((B * xs + 64,), -7.5, dtype=torch.float32, device=DEV)
    tb = torch.full((B * ts + 64,), -11, dtype=torch.int64, device=DEV)
    eb = torch.full((B * ts + 64,), -13, dtype=torch.int64, device=DEV)
    x = xb.as_strided((B, 4) + crop, (xs, V, crop[1] * crop[2], crop[2], 1), lead)
    t = tb.as_strided((B,) + crop, (ts, crop[1] * crop[2], crop[2], 1), lead)
    e = eb.as_strided((B,) + crop, (ts, crop[1] * crop[2], crop[2], 1), lead)
    assert x.data_ptr() % 16 != 0
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
    base = [data.AugParams((1, 2, 3), (True, False, False), rng.uniform(0.5, 1.5, 4), rng.uniform(-2, 2, 4), blur=(1.0, 0, 0, 0)),
            data.AugParams((0, 0, 0), noise=(0, 0.1, 0, 0), noise_key=3), data.AugParams((2, 0, 1), (False, True, True), matrix=MATRIX)]
    bias = A.random_bias(GRID, rng)
    off = [data.AugParams(p.origin, p.flip, p.scale, p.shift, p.matrix, blur=p.blur, noise=p.noise, noise_key=p.noise_key,
                          bias=bias if k != 1 else None, bias_mask=(False,) * 4 if k != 1 else None, contrast=(0, 0, 0, 0) if k else None,
                          lowres=(0, 0, 0, 0) if k != 2 else None) for k, p in enumerate(base)]
    calls = []
    real = type(hip)._call

    def counting(self, name, *args):
        calls.append(name)
        return real(self, name, *args)

    monkeypatch.setattr(type(hip), "_call", counting)
    want = hip.prepare_batch(dimgs, dlabs, base, crop)
    before, calls[:] = list(calls), []
    got = hip.prepare_batch(dimgs, dlabs, off, crop)
    assert calls == before == ["cwf_prepare_batch_affine", "cwf_augment_intensity"]
    assert torch.equal(_bits(got[0]), _bits(want[0])) and torch.equal(got[1], want[1]) and torch.equal(got[2], want[2])
    calls[:] = []
    on = hip.prepare_batch(dimgs, dlabs, off[:2] + [data.AugParams((2, 0, 1), (False, True, True), matrix=MATRIX, lowres=(0, 0, 0, 0.5))], crop)
    assert calls == ["cwf_prepare_batch_affine", "cwf_augment_acquisition", "cwf_augment_intensity"]
    assert not torch.equal(on[0][2, 3], got[0][2, 3]) and torch.equal(_bits(on[0][:2]), _bits(got[0][:2]))


def test_refusals_launch_nothing(hip):
    """the C entry directly: CWF_E_BADARG (-1) or CWF_E_TOOLARGE (-2) before anything is launched (the output keeps its sentinel); the
    ends of the ranges are accepted"""
    from cwf import _lib
    crop = (4, 5, 9)
    V = crop[0] * crop[1] * crop[2]
    src = torch.randn(2 * 4 * V + 4, device=DEV)
    keep = src.clone()
    dst = torch.full((2 * 4 * V + 4,), -7.5, dtype=torch.float32, device=DEV)
    grids = torch.ones(4 * 8 * 8 * 8 + 1, device=DEV)
    nws = _lib.acquire_ws_doubles(2, crop)
    assert nws == 24
    ws = torch.zeros(nws + 1, dtype=torch.float64, device=DEV)
    stream = torch.cuda.current_stream().cuda_stream
    inf, nan = float("inf"), float("nan")

    def call(B=2, samples=True, s=None, d=None, sbs=4 * V, dbs=4 * V, w=None, nw=nws, c=crop, which=(1,), **field):
        smp = (_lib.AcquireSample * 2)()
        for k in range(2):
            smp[k].bias_mask, smp[k].contrast_mask, smp[k].lowres_mask = 5, 9, 6
            smp[k].G0, smp[k].G1, smp[k].G2 = 4, 6, 8
            for ch in range(4):
                smp[k].bias[ch] = grids.data_ptr() + 4 * 192 * ch if ch in (0, 2) else 0      # channels 1 and 3 are off: not looked at
                smp[k].lattice[ch][:] = [2, 5, 9] if ch in (1, 2) else [0, 99, -1]            # channels 0 and 3 are off
            smp[k].factor[:] = [1.5, -1.0, nan, 0.5]                                        # channels 1 and 2 are off
        for b in which:
            for k, v in field.items():
                if k in ("factor", "bias"):
                    getattr(smp[b], k)[v[0]] = v[1]
                elif k == "lattice":
                    smp[b].lattice[v[0]][v[1]] = v[2]
                else:
                    setattr(smp[b], k, v)
        return hip.lib.cwf_augment_acquisition(smp if samples else None, B, c[0], c[1], c[2], src.data_ptr() if s is None else s, sbs,
                                               dst.data_ptr() if d is None else d, dbs, ws.data_ptr() if w is None else w, nw, stream)

    bad = [dict(samples=False), dict(B=0), dict(B=-1), dict(c=(0, 5, 9)), dict(c=(4, -1, 9)), dict(c=(4, 5, 0)), dict(s=0), dict(d=0),
           dict(s=src.data_ptr() + 2), dict(d=dst.data_ptr() + 1), dict(w=0), dict(w=ws.data_ptr() + 4), dict(nw=nws - 1),
           dict(sbs=4 * V - 1), dict(dbs=4 * V - 1), dict(bias_mask=16), dict(contrast_mask=-1), dict(lowres_mask=31), dict(G0=3), dict(G1=9),
           dict(G2=0), dict(bias=(0, 0)), dict(bias=(2, grids.data_ptr() + 2)), dict(bias_mask=7), dict(factor=(0, 0.0)), dict(factor=(3, -1.0)),
           dict(factor=(0, inf)), dict(factor=(3, nan)), dict(contrast_mask=11), dict(lattice=(1, 0, 0)), dict(lattice=(2, 0, 5)),
           dict(lattice=(1, 1, 6)), dict(lattice=(2, 2, 10)), dict(lattice=(1, 2, -3)), dict(lowres_mask=7), dict(d=src.data_ptr()),
           dict(d=src.data_ptr() + 4 * V)]
    for kw in bad:
        assert call(**kw) == -1, kw
    assert call(c=(2048, 1024, 1024), sbs=2 ** 33, dbs=2 ** 33) == -2 and call(c=(1290, 1290, 1291), sbs=2 ** 33 + 2 ** 30, dbs=2 ** 34) == -2
    torch.cuda.synchronize()
    assert bool((dst == -7.5).all()) and torch.equal(src, keep)
    ok = [dict(), dict(factor=(0, 1e-30)), dict(factor=(3, 3e38)), dict(lattice=(1, 0, 1)), dict(lattice=(2, 0, 4)), dict(B=1),
          dict(s=src.data_ptr() + 4, d=dst.data_ptr() + 4), dict(G0=8, G1=8, G2=8), dict(which=(0, 1), contrast_mask=0, w=0, nw=0)]
    for kw in ok:
        assert call(**kw) == 0, kw
        torch.cuda.synchronize()
        src.copy_(keep)
    assert not bool((dst[1:8 * V] == -7.5).any())
    # in place is accepted only without a lowres bit
    x = torch.randn(2 * 4 * V, device=DEV)
    held = x.clone()
    assert call(s=x.data_ptr(), d=x.data_ptr()) == -1
    assert call(s=x.data_ptr(), d=x.data_ptr(), lowres_mask=0) == -1                                  # (sample 0 still has its bits)
    torch.cuda.synchronize()
    assert torch.equal(x, held)
    assert call(s=x.data_ptr(), d=x.data_ptr(), lowres_mask=0, which=(0, 1)) == 0
    torch.cuda.synchronize()
    assert not torch.equal(x[:V], held[:V]) and torch.equal(x[V:2 * V], held[V:2 * V])               # channel 0: bias and contrast; 1: nothing


def test_device_brats_cached_equals_staged(hip):
    from utils import data
    rng = np.random.default_rng(7)
    S = (40, 36, 28)
    subjects = [(torch.from_numpy(E.random_image(S, rng)), torch.from_numpy(E.blob_labels(S, rng))) for _ in range(3)]
    crop = (24, 24, 24)
    kw = dict(seed=21, flip=True, intensity=0.3, rotate=15.0, scale=0.2, elastic=4.0, elastic_grid=6, blur=1.5, noise=0.3, bias=0.5, bias_grid=5,
              contrast=0.3, lowres=0.5)
    cache = data.DeviceBraTS(subjects, DEV, crop, **kw)
    staged = data.DeviceBraTS(subjects, DEV, crop, cache=False, **kw)
    on = set()
    for epoch in (0, 3):
        cache.set_epoch(epoch)
        staged.set_epoch(epoch)
        got = cache.batch([0, 1, 2])
        for i in range(3):
            p = cache.params(i)
            on.update(k for k in ("bias_mask", "contrast", "lowres") if any(getattr(p, k)))
        for other in (staged.batch([0, 1, 2]), next(iter(staged.batches([[0, 1, 2]], num_workers=0)))):
            assert torch.equal(_bits(other[0]), _bits(got[0])) and torch.equal(other[1], got[1]) and torch.equal(other[2], got[2])
        assert got[0].is_cuda
        _check(got[:3], [s[0] for s in subjects], [s[1] for s in subjects], [cache.params(i) for i in range(3)], crop)
    assert on == {"bias_mask", "contrast", "lowres"}
