"""The intensity stage of the batch preparer on the CPU (utils.data._intensity_stage_cpu through prepare_batch): blur against the scalar
restatement of tests/intensity_prep_ref.py bit for bit and against the float64 filter within a derived bound; the noise integers, its
moments and what it depends on; the properties of the gamma map; draw_params, AugParams, DeviceBraTS("cpu") and the train_no_amp flags.

The blur bound, derived and not tuned.  One pass forms y = sum_j w_j a_j, seven products and six sums, each rounded once (u = 2^-24);
with the sums taken in sequence the first product passes through seven roundings, so |y32 - y_exact| <= g7 * sum_j |w_j a_j| <=
g7 * S * M with g7 = 7u / (1 - 7u), S = sum_j w_j (the float32 taps are >= 0) and M = max |a| of the pass's input.  An error e in the
input reaches the output as at most S * e.  Three passes on inputs bounded by M, S*M + e1, S^2*M + e2 give
|y32 - y64| <= g7 * M * (S^3 + S^2 + S) * (1 + g7)^2, which is what BOUND evaluates; float64's own roundings are 2^-29 of that."""
import numpy as np
import pytest
import torch

import elastic_prep_ref as E
import intensity_prep_ref as R

F = np.float32
U = 2.0 ** -24


def blur_bound(w, m):
    s, g7 = float(np.sum(w.astype(np.float64))), 7 * U / (1 - 7 * U)
    return g7 * m * (s ** 3 + s ** 2 + s) * (1 + g7) ** 2


def _stage(x, **kw):
    """the stage alone: x [4, *crop] float32 through prepare_batch as a source volume at origin 0"""
    from utils import data
    x = torch.from_numpy(np.ascontiguousarray(x, dtype=F))
    lab = torch.zeros(tuple(x.shape[1:]), dtype=torch.uint8)
    return data.prepare_batch([x], [lab], [data.AugParams((0, 0, 0), **kw)], tuple(x.shape[1:]))[0][0].numpy()


def _bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.int32)


def test_taps():
    from utils import data
    for sigma in (0.5, 0.73, 1.0, 1.5, 4.0):
        w = data.blur_taps(sigma)
        assert w.dtype == F and np.array_equal(w, R.taps(sigma)) and np.array_equal(w, w[::-1]) and abs(float(w.sum()) - 1) < 1e-6
    assert np.array_equal(data.blur_taps(1e-30), F([0, 0, 0, 1, 0, 0, 0]))


@pytest.mark.parametrize("shape", [(13, 11, 9), (1, 1, 7), (2, 3, 5), (7, 1, 2)])
def test_blur_equals_the_scalar_restatement_and_bounds_float64(shape):
    rng = np.random.default_rng(sum(shape))
    x = rng.standard_normal((4,) + shape).astype(F) * F([1, 3.5, 0.25, 10]).reshape(4, 1, 1, 1)
    sig = (0.5, 1.0, 0.0, 1.5)
    got = _stage(x, blur=sig)
    worst = 0.0
    for c in range(4):
        if sig[c] == 0.0:
            assert np.array_equal(_bits(got[c]), _bits(x[c]))
            continue
        assert np.array_equal(_bits(got[c]), _bits(R.blur(x[c], sig[c])))
        w = R.taps(sig[c])
        err = float(np.max(np.abs(got[c].astype(np.float64) - R.blur64(x[c], w))))
        bound = blur_bound(w, float(np.max(np.abs(x[c]))))
        print("blur", shape, "channel", c, "max |f32 - f64| %.3g, bound %.3g" % (err, bound))
        assert err <= bound
        worst = max(worst, err / bound)
    assert worst <= 1.0


def test_blur_border_is_replicate_and_zero_padding_is_data():
    """a crop that leaves its volume: the padded zeros are blurred into the data, and the crop's own border replicates"""
    from utils import data
    img = torch.full((4, 6, 6, 6), 2.0)
    lab = torch.zeros((6, 6, 6), dtype=torch.uint8)
    x = data.prepare_batch([img], [lab], [data.AugParams((0, 0, 0), blur=(1.0, 0, 0, 0))], (6, 6, 10))[0][0].numpy()
    assert np.all(x[0, :, :, :2] == x[0, 0, 0, 0]) and abs(float(x[0, 0, 0, 0]) - 2.0) < 1e-5     # far from the padding: constant 2
    assert 0.0 < float(x[0, 0, 0, 6]) < float(x[0, 0, 0, 5]) < 2.0                                # the padding's edge is smeared
    assert np.array_equal(x[1], np.concatenate([np.full((6, 6, 6), 2.0, F), np.zeros((6, 6, 4), F)], axis=2))


def test_noise_integers():
    """splitmix64 seeded with 0 gives 0xE220A8397B1DCDAF first (the published test vector): 0xE220 + 0xA839 + 0x7B1D + 0xCDAF =
    57888 + 43065 + 31517 + 52655 = 185125, less 131070 is 54055.  The others were computed once with Python integers; the last key
    makes key + 0x9E3779B97F4A7C15 wrap to 2."""
    from utils import data
    cases = [(0, 0, 54055), (5, 0, 1268), (5, 1, 61742), (12345678901234567, 4242, -42064), (2 ** 63 - 1, 2 ** 33, 48184),
             (7046029254386353133, 0, -40160)]
    for key, ctr, want in cases:
        assert R.noise_int(key, ctr) == want
        assert int(data.noise_ints(key, ctr, 1)[0]) == want
    assert data.noise_ints(5, 0, 3).tolist() == [1268, 61742, R.noise_int(5, 2)]
    assert float(data.noise_amp(1.0)) == float(R.noise_amp(1.0)) == float(F(1.0 / np.sqrt((65536.0 ** 2 - 1) / 3)))


def test_noise_moments():
    """2^20 voxels: the mean within five standard errors of 0, the standard deviation within five of sigma (the kurtosis of a sum of
    four uniforms is 3 - 1.2 / 4 = 2.7, so se(std) = sigma * sqrt((2.7 - 1) / (4 N)))"""
    shape, sigma = (64, 128, 128), 0.37
    n = shape[0] * shape[1] * shape[2]
    x = _stage(np.zeros((4,) + shape, F), noise=(sigma, 0, 0, 0), noise_key=99)
    sg = float(F(sigma))
    mean, std = float(x[0].astype(np.float64).mean()), float(x[0].astype(np.float64).std())
    print("noise mean %.3g (se %.3g), std %.6g of %.6g (se %.3g), range %.3f .. %.3f sigma"
          % (mean, sg / np.sqrt(n), std, sg, sg * np.sqrt(1.7 / (4 * n)), x[0].min() / sg, x[0].max() / sg))
    assert abs(mean) <= 5 * sg / np.sqrt(n)
    assert abs(std - sg) <= 5 * sg * np.sqrt(1.7 / (4 * n))
    assert float(np.abs(x[0]).max()) <= 3.4642 * sg and not x[1:].any()


def test_noise_depends_on_key_channel_and_voxel_only():
    rng = np.random.default_rng(3)
    a = rng.standard_normal((4, 4, 6, 8)).astype(F)
    sig, key = (0.1, 0.2, 0.0, 0.4), 2 ** 62 + 17
    got = _stage(a, noise=sig, noise_key=key)
    assert np.array_equal(_bits(got), _bits(R.blur_noise(a, None, sig, key)))
    assert np.array_equal(_bits(got[2]), _bits(a[2]))
    # the same V in another shape, other data, other channels on: voxel v of channel c gets the same addend
    z1 = _stage(np.zeros((4, 4, 6, 8), F), noise=sig, noise_key=key)
    z2 = _stage(np.zeros((4, 8, 6, 4), F), noise=(0.1, 0.0, 0.3, 0.4), noise_key=key, gamma=(0, 1.5, 0, 0))
    assert np.array_equal(z1[0].reshape(-1), z2[0].reshape(-1)) and np.array_equal(z1[3].reshape(-1), z2[3].reshape(-1))
    assert not np.array_equal(z1, _stage(np.zeros((4, 4, 6, 8), F), noise=sig, noise_key=key + 1))
    amp = R.noise_amp(sig[1])
    assert float(z1[1].reshape(-1)[7]) == float(F(F(R.noise_int(key, 1 * 192 + 7)) * amp))


def test_gamma_properties():
    rng = np.random.default_rng(8)
    a = rng.standard_normal((4, 5, 6, 7)).astype(F) * F(3.0) + F(1.0)
    a[2] = F(4.25)                                          # a constant channel
    g = (0.6, 1.7, 1.3, 0.0)
    got = _stage(a, gamma=g)
    for c in (0, 1):
        order = np.argsort(a[c], axis=None, kind="stable")
        assert np.all(np.diff(got[c].reshape(-1)[order]) >= 0)                  # monotone
        lo, hi = int(np.argmin(a[c])), int(np.argmax(a[c]))
        assert got[c].reshape(-1)[lo] == a[c].reshape(-1)[lo]                   # the minimum maps to itself exactly
        mx = a[c].reshape(-1)[hi]
        assert abs(float(got[c].reshape(-1)[hi]) - float(mx)) <= float(np.spacing(np.abs(mx)))   # the maximum within one rounding
        assert not np.array_equal(got[c], a[c])
        y, ref, r = R.gamma64(a[c], g[c])
        # a float32 power: one ulp of y for the host powf (glibc documents 1 ulp), as much again for the rounded product with r
        # (half an ulp of y*r is at most an ulp of y times r), and the rounded sum's half ulp of the result (its own ulp leaves slack)
        assert np.max(np.abs(got[c] - ref) - (2 * R.ulp32(y) * r + R.ulp32(ref))) <= 0
    assert np.array_equal(_bits(got[2]), _bits(a[2])) and np.array_equal(_bits(got[3]), _bits(a[3]))
    zero = _stage(np.zeros((4, 3, 4, 5), F), gamma=(0.5, 2.0, 1.0, 1.5))
    assert np.array_equal(_bits(zero), np.zeros((4, 3, 4, 5), np.int32))
    # NaN is ignored by the minimum and maximum (and stays NaN); a range that is not finite leaves the channel alone
    b = a.copy()
    b[0, 0, 0, 0] = np.nan
    b[1, 0, 0, 0] = np.inf
    gb = _stage(b, gamma=g)
    assert np.isnan(gb[0, 0, 0, 0]) and np.array_equal(_bits(gb[0].reshape(-1)[1:]), _bits(_stage_rest(a, b, g)))
    assert np.array_equal(_bits(gb[1]), _bits(b[1]))


def _stage_rest(a, b, g):
    """channel 0 of b without its NaN voxel, mapped with the range of the remaining voxels"""
    rest = b[0].reshape(-1)[1:]
    mn, r, u = R.gamma_parts(rest)
    return (np.power(u, F(g[0])).astype(F) * r + mn).astype(F)


def test_steps_off_keep_bits():
    """-0.0, inf, NaN payloads and denormals pass a stage in which their channel's steps are off, beside channels that are on"""
    a = np.zeros((4, 3, 3, 8), F)
    a[1].reshape(-1)[:6] = np.array([0x80000000, 0x7F800000, 0x7FC01234, 0x00000001, 0xFF800000, 0x3F800000], np.uint32).view(F)
    a[3] = a[1]
    got = _stage(a, blur=(1.0, 0, 0.7, 0), noise=(0.5, 0, 0, 0), noise_key=4, gamma=(0, 0, 1.2, 0))
    assert np.array_equal(_bits(got[1]), _bits(a[1])) and np.array_equal(_bits(got[3]), _bits(a[3]))
    assert got[0].any() and np.array_equal(_bits(got[2]), _bits(a[2]))


def test_full_stage_order_blur_noise_gamma():
    rng = np.random.default_rng(12)
    a = rng.standard_normal((4, 6, 5, 9)).astype(F)
    blur, noise, gamma, key = (1.2, 0.0, 0.8, 0.6), (0.3, 0.2, 0.0, 0.1), (0.0, 0.0, 0.0, 1.4), 77
    got = _stage(a, blur=blur, noise=noise, noise_key=key, gamma=gamma)
    pre = R.blur_noise(a, blur, noise, key)
    assert np.array_equal(_bits(got[:3]), _bits(pre[:3]))
    mn, r, u = R.gamma_parts(pre[3])
    assert np.array_equal(_bits(got[3]), _bits((np.power(u, F(1.4)).astype(F) * r + mn).astype(F)))


def test_draw_params_stream():
    from utils import data
    full, crop = (40, 44, 36), (16, 16, 16)
    old = dict(flip=True, intensity=0.2, rotate=10.0, scale=0.1, elastic=3.0, elastic_grid=5)
    seen = {k: set() for k in ("blur", "noise", "gamma")}
    keys = set()
    for n in range(200):
        epoch, index = n // 10, n % 10 + (n % 3) * 100
        for base in ({}, old):
            p0 = data.draw_params(7, epoch, index, full, crop, **base)
            p = data.draw_params(7, epoch, index, full, crop, blur=1.5, noise=0.25, gamma=0.4, **base)
            assert p == data.draw_params(7, epoch, index, full, crop, blur=1.5, noise=0.25, gamma=0.4, **base)      # a pure function
            for k in ("origin", "flip", "scale", "shift", "matrix"):
                assert getattr(p, k) == getattr(p0, k)
            assert (p.disp is None and p0.disp is None) or p.disp.tobytes() == p0.disp.tobytes()
            assert p0.blur is None and p0.noise is None and p0.gamma is None and p0.noise_key == 0 and not p0.intensity_stage()
            assert all(v == 0.0 or F(0.5) <= F(v) <= F(1.5) for v in p.blur)
            assert all(0.0 <= v <= float(F(0.25)) for v in p.noise) and 0 <= p.noise_key < 2 ** 63
            assert all(v == 0.0 or F(0.6) <= F(v) <= F(1.4) for v in p.gamma)
            for k in seen:
                seen[k].update(c for c in range(4) if getattr(p, k)[c] > 0.0)
                seen[k].update(-1 - c for c in range(4) if getattr(p, k)[c] == 0.0)
            keys.add(p.noise_key)
            if not base:
                # the stream as the documentation states it: every draw of a transform is made whether or not a channel ends up on
                rng = np.random.default_rng([7, epoch, index])
                assert data.random_crop_origin(full, crop, rng) == p.origin
                for name, lo, hi in (("blur", 0.5, 1.5), ("noise", 0.0, 0.25), ("gamma", 0.6, 1.4)):
                    u, val = rng.random(4), rng.uniform(lo, hi, 4)
                    assert getattr(p, name) == tuple(float(v) for v in np.where(u < 0.5, val, 0.0).astype(F))
                    if name == "noise":
                        assert p.noise_key == int(rng.integers(0, 2 ** 63))
    assert all(len(v) == 8 for v in seen.values()) and len(keys) == 400          # every channel on and off somewhere
    assert data.draw_params(7, 0, 0, full, crop, blur=0.5).blur in [tuple(F(0.5) * b for b in bits) for bits in
                                                                    np.ndindex(2, 2, 2, 2)]
    for kw in (dict(blur=0.4), dict(blur=1.6), dict(blur=-1.0), dict(noise=-0.1), dict(noise=float("inf")), dict(gamma=1.0),
               dict(gamma=-0.1)):
        with pytest.raises(ValueError, match="draw_params"):
            data.draw_params(7, 0, 0, full, crop, **kw)


def test_aug_params():
    from utils import data
    disp = np.zeros((3, 4, 4, 4), F)
    a = data.AugParams((1, 2, 3), (True, False, True), (1, 1, 1, 1), (0, 0, 0, 0), None, disp, blur=(0.5, 0, 1, 0),
                       noise=np.array([0.1, 0, 0, 0]), noise_key=2 ** 63 - 1, gamma=[0, 0.7, 0, 1.5])
    b = data.AugParams((1, 2, 3), (True, False, True), (1, 1, 1, 1), (0, 0, 0, 0), disp=disp.copy(), blur=(0.5, 0, 1, 0),
                       noise=(F(0.1), 0, 0, 0), noise_key=2 ** 63 - 1, gamma=(0, F(0.7), 0, 1.5))
    assert a == b and a.at_origin((1, 2, 3)) == a and a.at_origin((0, 0, 0)) != a and a.at_origin((0, 0, 0)).gamma == a.gamma
    assert a.blur == (0.5, 0.0, 1.0, 0.0) and a.noise == (float(F(0.1)), 0.0, 0.0, 0.0) and a.intensity_stage()
    for kw in (dict(blur=(0.5, 0, 1.25, 0)), dict(noise=(0.2, 0, 0, 0)), dict(noise_key=5), dict(gamma=(0, 0.7, 0, 0)), dict(blur=None)):
        args = dict(blur=a.blur, noise=a.noise, noise_key=a.noise_key, gamma=a.gamma)
        args.update(kw)
        assert data.AugParams((1, 2, 3), (True, False, True), (1, 1, 1, 1), (0, 0, 0, 0), disp=disp, **args) != a
    r = repr(a)
    assert "blur=(0.5, 0.0, 1.0, 0.0)" in r and "noise_key=9223372036854775807" in r and "gamma=(0.0, " in r and "disp=float32" in r
    plain = data.AugParams((1, 2, 3))
    assert repr(plain) == "AugParams(origin=(1, 2, 3), flip=(False, False, False), scale=None, shift=None)"
    assert plain.blur is None and plain.noise is None and plain.gamma is None and plain.noise_key == 0 and not plain.intensity_stage()
    assert not data.AugParams((0, 0, 0), blur=(0, 0, 0, 0), noise=(0, 0, 0, 0), gamma=(0, 0, 0, 0)).intensity_stage()
    assert plain == data.AugParams((1, 2, 3), (False, False, False), None, None, None, None)                 # positional, as before
    for kw in (dict(blur=(1, 1, 1)), dict(blur=(1, -0.5, 1, 1)), dict(noise=(0, 0, 0, float("nan"))), dict(gamma=(0, 0, float("inf"), 0)),
               dict(noise=(0.1, 0, 0, 0), noise_key=-1), dict(noise_key=2 ** 63), dict(gamma=(1, 1, 1, 1, 1))):
        with pytest.raises(ValueError, match="AugParams"):
            data.AugParams((0, 0, 0), **kw)
    with pytest.raises(TypeError):
        data.AugParams((0, 0, 0), (False, False, False), None, None, None, None, (1, 1, 1, 1))               # keyword-only


def test_device_brats_cpu():
    from utils import data
    rng = np.random.default_rng(5)
    subjects = [(torch.from_numpy(E.random_image(S, rng)), torch.from_numpy(E.blob_labels(S, rng))) for S in ((20, 22, 18), (18, 20, 24))]
    crop = (12, 12, 16)
    kw = dict(seed=3, flip=True, intensity=0.2, rotate=10.0)
    base = data.DeviceBraTS(subjects, "cpu", crop, **kw)
    off = data.DeviceBraTS(subjects, "cpu", crop, blur=0.0, noise=0.0, gamma=0.0, **kw)
    on = data.DeviceBraTS(subjects, "cpu", crop, blur=1.5, noise=0.2, gamma=0.3, **kw)
    staged = data.DeviceBraTS(subjects, "cpu", crop, cache=False, blur=1.5, noise=0.2, gamma=0.3, **kw)
    changed = 0
    for epoch in (0, 1, 2):
        for d in (base, off, on, staged):
            d.set_epoch(epoch)
        want, got, full = base.batch([0, 1]), off.batch([0, 1]), on.batch([0, 1])
        assert torch.equal(got[0].view(torch.int32), want[0].view(torch.int32)) and torch.equal(got[1], want[1])
        assert torch.equal(got[2], want[2]) and off.params(1) == base.params(1)
        assert torch.equal(full[1], want[1]) and torch.equal(full[2], want[2])               # target and edge are not touched
        st = staged.batch([0, 1])
        assert torch.equal(st[0].view(torch.int32), full[0].view(torch.int32)) and torch.equal(st[1], full[1])
        for b in (0, 1):
            p = on.params(b)
            for c in range(4):
                same = torch.equal(full[0][b, c].view(torch.int32), want[0][b, c].view(torch.int32))
                assert same == (p.blur[c] == 0.0 and p.noise[c] == 0.0 and p.gamma[c] == 0.0)
                changed += not same
    assert changed > 0


def test_train_flags():
    import train_no_amp as T
    a = T.build_parser().parse_args([])
    assert a.aug_blur == 0.0 and a.aug_noise == 0.0 and a.aug_gamma == 0.0
    b = T.build_parser().parse_args(["--device_data", "staged", "--aug_blur", "1.5", "--aug_noise", "0.1", "--aug_gamma", "0.3"])
    assert (b.aug_blur, b.aug_noise, b.aug_gamma) == (1.5, 0.1, 0.3)
    T.check_intensity_aug(b)
    for flag in ("--aug_blur", "--aug_noise", "--aug_gamma"):
        with pytest.raises(SystemExit, match="device_data cache"):
            T.main(["--synthetic", "1", flag, "0.5"])
    for flag, bad, rule in (("--aug_blur", "0.4", r"--aug_blur takes 0 \(off\) or a largest sigma in \[0.5, 1.5\]"),
                            ("--aug_blur", "1.6", "--aug_blur takes"), ("--aug_blur", "-1", "--aug_blur takes"),
                            ("--aug_noise", "-0.1", "--aug_noise takes a finite largest sigma >= 0"), ("--aug_noise", "inf", "--aug_noise"),
                            ("--aug_noise", "nan", "--aug_noise"), ("--aug_gamma", "1.0", r"--aug_gamma takes a half-width in \[0, 1\)"),
                            ("--aug_gamma", "-0.2", "--aug_gamma"), ("--aug_gamma", "nan", "--aug_gamma")):
        with pytest.raises(SystemExit, match=rule):
            T.main(["--synthetic", "1", "--device_data", "cache", flag, bad])
    for flag, ok in (("--aug_blur", "0.5"), ("--aug_blur", "1.5"), ("--aug_gamma", "0.99"), ("--aug_noise", "0")):
        T.check_intensity_aug(T.build_parser().parse_args(["--device_data", "cache", flag, ok]))
    # the flags reach the dataset
    c = T.build_parser().parse_args(["--synthetic", "1", "--device_data", "cache", "--aug_blur", "1.25", "--aug_noise", "0.1", "--aug_gamma",
                                     "0.3", "--input_H", "20", "--input_W", "18", "--output_D", "16", "--crop_H", "8", "--crop_W", "8",
                                     "--crop_D", "8"])
    ds = T.make_device_dataset(c, "cpu")
    assert (ds.blur, ds.noise, ds.gamma) == (1.25, 0.1, 0.3) and ds.params(0).intensity_stage()
