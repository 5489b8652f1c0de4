"""The acquisition stage of the batch preparer on the CPU (utils.data._acquisition_stage_cpu: bias field, contrast, low-resolution
simulation) against the restatement of tests/acquisition_prep_ref.py bit for bit; the range of the bias field; draw_params, AugParams,
prepare_batch's order of the stages, DeviceBraTS("cpu") and the train_no_amp flags.

The range of the bias field, derived and not tuned (u = 2^-24, the unit roundoff).  All control multipliers and weights are >= 0, so
every rounding acts as a relative error on a sum of non-negative terms.  One 4-term sum ((w0*a + w1*b) + w2*c) + w3*d passes its first
product through four roundings (the product and three sums): its value lies within (1 +- u)^4 of the exact sum of w_j * v_j, which
lies between W * min v and W * max v, W the exact sum of the four float32 weights.  Three nested sums give
    min(grid) * W0*W1*W2 * (1 - u)^12 <= m(p) <= max(grid) * W0*W1*W2 * (1 + u)^12.
W differs from 1 by the weights' own rounding: the four cubic polynomials sum to 1 for every t; their evaluations keep every
intermediate value at or below 6 in magnitude, take at most 6 roundings each before the product with h = float32(1/6) (itself within
u of 1/6), and s = 1 - t adds one more to w0, so the absolute errors are at most 7u/6 (w0), 4u/6 (w3), 6u (w1) and 7u (w2):
|W - 1| < 16u, which the test checks on the weights it uses.  (1 + 16u)^3 * (1 + u)^12 < 1 + 64u, so
    min(grid) * (1 - 64u) <= m(p) <= max(grid) * (1 + 64u)."""
import numpy as np
import pytest
import torch

import acquisition_prep_ref as A
import elastic_prep_ref as E

F = np.float32
U = 2.0 ** -24
CROPS = [(12, 11, 37), (1, 9, 40), (33, 10, 10)]
GRIDS = [(4, 4, 4), (8, 8, 8), (4, 6, 8)]
Z_FULL = 0.99          # floor(C * 0.99 + 0.5) == C for every C <= 50: the lattice is the crop's own


def _bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.int32)


def _image(crop, seed):
    return E.random_image(crop, np.random.default_rng(seed))


def _run(x, **kw):
    """utils.data's statement on a copy of x [4, *crop]"""
    from utils import data
    p = data.AugParams((0, 0, 0), **kw)
    assert p.acquisition_stage()
    return data._acquisition_stage_cpu(np.array(x, dtype=F, order="C"), p)


@pytest.mark.parametrize("crop", CROPS)
@pytest.mark.parametrize("G", GRIDS)
def test_bias_field_equals_the_restatement_and_stays_in_range(crop, G):
    from utils import data
    rng = np.random.default_rng(sum(crop) + sum(G))
    x = _image(crop, 1)
    bias = A.random_bias(G, rng)
    mask = (True, False, True, True)
    got = _run(x, bias=bias, bias_mask=mask)
    want = A.stage(x, bias=bias, bias_mask=mask)
    assert np.array_equal(_bits(got), _bits(want))
    assert np.array_equal(_bits(got[1]), _bits(x[1])) and not np.array_equal(_bits(got[0]), _bits(x[0]))
    W = A.weight_sums(crop, G)
    assert all(float(np.max(np.abs(w - 1.0))) < 16 * U for w in W)
    for c in (0, 2, 3):
        m = data.bias_field(bias[c], crop).astype(np.float64)
        assert np.array_equal(_bits(m), _bits(A.bias_field(bias[c], crop)))
        lo, hi = float(bias[c].min()), float(bias[c].max())
        assert np.all(m >= lo * (1 - 64 * U)) and np.all(m <= hi * (1 + 64 * U)) and np.all(m > 0)
    const = data.bias_field(np.full(G, 1.25, F), crop)
    assert np.all(np.abs(const.astype(np.float64) - 1.25) <= 1.25 * 64 * U)


@pytest.mark.parametrize("crop", CROPS)
def test_contrast_equals_the_restatement(crop):
    x = _image(crop, 2)
    x[2] = F(-3.25)                                  # constant: mn == mx
    x[3].reshape(-1)[5] = np.nan                     # a NaN voxel: the mean is not finite, the channel stays
    f = (0.75, 1.25, 1.1, 0.8)
    got = _run(x, contrast=f)
    assert np.array_equal(_bits(got), _bits(A.stage(x, factor=f)))
    assert np.array_equal(_bits(got[2]), _bits(x[2])) and np.array_equal(_bits(got[3]), _bits(x[3]))
    assert float(x[0].min()) < float(got[0].min()) and float(got[0].max()) < float(x[0].max())       # f < 1 narrows the range
    assert float(got[1].min()) == float(x[1].min()) and float(got[1].max()) == float(x[1].max())   # f > 1 runs into the clamp
    assert int(np.sum(got[1] == x[1].max())) > 1
    off = _run(x, contrast=(0.0, 1.25, 0.0, 0.0))
    assert np.array_equal(_bits(off[0]), _bits(x[0])) and np.array_equal(_bits(off[1]), _bits(got[1]))


@pytest.mark.parametrize("crop", CROPS)
def test_lowres_equals_the_restatement(crop):
    """z = 0.5, a lattice in between, the crop's own lattice (n_d == C_d), and n_d == 1 on a unit axis"""
    from utils import data
    x = _image(crop, 3)
    z = (0.5, 0.73, Z_FULL, 0.0)
    assert data.lowres_lattice(crop, Z_FULL) == crop == A.lattice(crop, Z_FULL)
    assert data.lowres_lattice(crop, 0.5) == A.lattice(crop, 0.5) == tuple(max(1, int(np.floor(c * 0.5 + 0.5))) for c in crop)
    if crop[0] == 1:
        assert data.lowres_lattice(crop, 0.5)[0] == 1
    got = _run(x, lowres=z)
    assert np.array_equal(_bits(got), _bits(A.stage(x, zoom=z)))
    assert np.array_equal(_bits(got[3]), _bits(x[3])) and not np.array_equal(_bits(got[0]), _bits(x[0]))


@pytest.mark.parametrize("crop", CROPS)
def test_lowres_on_the_crops_own_lattice(crop):
    """n_d == C_d: every voxel reads itself with t = 0 and keeps its bits, except on the last index of an axis longer than one voxel.
    There the definition's k = min(floor(u), n_d - 2) makes the taps (C_d - 2, C_d - 1) with t = 1, and lerp returns a + (b - a),
    which is b only up to the rounding of b - a and of the sum: at most ulp(b - a) / 2 + ulp(result) / 2 away.  On values of one
    binade (here [1, 2)) b - a is exact and the whole channel keeps its bits."""
    x = _image(crop, 4)
    got = _run(x, lowres=(Z_FULL,) * 4)
    inner = tuple(slice(0, max(c - 1, 1)) for c in crop)
    for c in range(4):
        assert np.array_equal(_bits(got[c][inner]), _bits(x[c][inner]))
    err = np.abs(got.astype(np.float64) - x.astype(np.float64))
    spread = 2.0 * float(np.max(np.abs(x)))          # |b - a| <= this, and so is every intermediate result
    assert float(err.max()) <= 3 * 1.0 * float(A.ulp32(spread))       # one a + (b - a) per axis, two roundings of <= ulp/2 each
    y = (1.0 + np.random.default_rng(5).random((4,) + crop)).astype(F)
    y[y >= 2.0] = F(1.5)
    assert np.array_equal(_bits(_run(y, lowres=(Z_FULL,) * 4)), _bits(y))


@pytest.mark.parametrize("crop", CROPS)
@pytest.mark.parametrize("G", GRIDS)
def test_all_three_equal_the_restatement(crop, G):
    rng = np.random.default_rng(7 * sum(crop) + sum(G))
    x = _image(crop, 6)
    bias = A.random_bias(G, rng)
    mask = (True, True, False, False)
    f = (1.2, 0.0, 0.8, 0.0)
    z = (0.5, Z_FULL, 0.6, 0.0)
    got = _run(x, bias=bias, bias_mask=mask, contrast=f, lowres=z)
    assert np.array_equal(_bits(got), _bits(A.stage(x, bias=bias, bias_mask=mask, factor=f, zoom=z)))
    assert np.array_equal(_bits(got[3]), _bits(x[3]))
    # the order of the steps matters and is bias -> contrast -> lowres
    step = _run(_run(_run(x, bias=bias, bias_mask=mask), contrast=f), lowres=z)
    assert np.array_equal(_bits(got), _bits(step))
    other = _run(_run(x, lowres=z), bias=bias, bias_mask=mask, contrast=f)
    assert not np.array_equal(_bits(got[0]), _bits(other[0]))


COMBOS = [dict(), dict(flip=True, intensity=0.2), dict(flip=True, intensity=0.2, rotate=15.0, scale=0.1, elastic=3.0, elastic_grid=5,
                                                      blur=1.5, noise=0.2, gamma=0.3),
          dict(rotate=10.0, gamma=0.5), dict(elastic=2.0, blur=1.0)]
NEW = dict(bias=0.5, bias_grid=6, contrast=0.3, lowres=0.5)
OLD_FIELDS = ("origin", "flip", "scale", "shift", "matrix", "blur", "noise", "noise_key", "gamma")


def test_draw_params_keeps_every_earlier_field_and_is_pure():
    from utils import data
    full, crop = (40, 36, 28), (24, 24, 24)
    seen = {k: set() for k in ("bias_mask", "contrast", "lowres")}
    for kw in COMBOS:
        for index in range(12):
            base = data.draw_params(11, 2, index, full, crop, **kw)
            off = data.draw_params(11, 2, index, full, crop, bias=0.0, bias_grid=4, contrast=0.0, lowres=0.0, **kw)
            assert off == base and base.bias is None and base.bias_mask == (False,) * 4 and base.contrast is None
            assert base.lowres is None and not base.acquisition_stage() and "bias" not in repr(base) and "lowres" not in repr(base)
            on = data.draw_params(11, 2, index, full, crop, **kw, **NEW)
            assert on == data.draw_params(11, 2, index, full, crop, **kw, **NEW)                 # a pure function of its arguments
            assert on != base
            for k in OLD_FIELDS:
                assert getattr(on, k) == getattr(base, k), k
            assert (on.disp is None) == (base.disp is None) and (on.disp is None or on.disp.tobytes() == base.disp.tobytes())
            # each new transform alone draws what it draws with the others on only when nothing precedes it: bias comes first
            alone = data.draw_params(11, 2, index, full, crop, bias=0.5, bias_grid=6, **kw)
            assert alone.bias.tobytes() == on.bias.tobytes() and alone.bias_mask == on.bias_mask and alone.contrast is None
            assert on.bias.shape == (4, 6, 6, 6) and on.bias.dtype == F and not on.bias.flags.writeable
            assert float(on.bias.min()) >= float(F(np.exp(-0.5))) and float(on.bias.max()) <= float(F(np.exp(0.5)))
            assert all(v == 0.0 or float(F(0.7)) <= v <= float(F(1.3)) for v in on.contrast)
            assert all(v == 0.0 or 0.5 <= v < 1.0 for v in on.lowres)
            for k in seen:
                seen[k].update((c, bool(getattr(on, k)[c])) for c in range(4))
    assert all(len(v) == 8 for v in seen.values())                                                   # every channel on and off somewhere
    # the stream as the documentation states it, after everything drawn before
    rng = np.random.default_rng([11, 2, 3])
    assert data.random_crop_origin(full, crop, rng) == data.draw_params(11, 2, 3, full, crop, **NEW).origin
    u, a = rng.random(4), rng.uniform(-0.5, 0.5, (4, 6, 6, 6))
    p = data.draw_params(11, 2, 3, full, crop, **NEW)
    assert p.bias_mask == tuple(bool(v) for v in u < 0.5) and np.array_equal(p.bias, np.exp(a).astype(F))
    u, f = rng.random(4), rng.uniform(0.7, 1.3, 4)
    assert p.contrast == tuple(float(v) for v in np.where(u < 0.5, f, 0.0).astype(F))
    u, z = rng.random(4), rng.uniform(0.5, 1.0, 4)
    assert p.lowres == tuple(float(v) for v in np.where(u < 0.5, z, 0.0).astype(F))


def test_range_errors():
    from utils import data
    full, crop = (40, 36, 28), (24, 24, 24)
    for kw in (dict(bias=-0.1), dict(bias=1.5), dict(bias=float("nan")), dict(bias=0.5, bias_grid=3), dict(bias=0.5, bias_grid=9),
               dict(contrast=1.0), dict(contrast=-0.2), dict(contrast=float("inf")), dict(lowres=0.4), dict(lowres=1.0),
               dict(lowres=-0.5), dict(lowres=float("nan"))):
        with pytest.raises(ValueError, match="draw_params"):
            data.draw_params(7, 0, 0, full, crop, **kw)
    for kw in (dict(bias=1.0), dict(contrast=0.99), dict(lowres=0.5), dict(lowres=0.999), dict(bias=0.3, bias_grid=8)):
        assert data.draw_params(7, 0, 0, full, crop, **kw).origin == data.draw_params(7, 0, 0, full, crop).origin
    ones = np.ones((4, 4, 5, 6), F)
    m = (True, False, False, True)

    def bad_value(v):
        g = ones.copy()
        g[2, 1, 2, 3] = v
        return g

    for kw in (dict(bias=np.ones((3, 4, 4, 4), F), bias_mask=m), dict(bias=np.ones((4, 4, 4), F), bias_mask=m),
               dict(bias=np.ones((4, 3, 4, 4), F), bias_mask=m), dict(bias=np.ones((4, 4, 9, 4), F), bias_mask=m),
               dict(bias=bad_value(0.0), bias_mask=m), dict(bias=bad_value(-1.0), bias_mask=m), dict(bias=bad_value(np.nan), bias_mask=m),
               dict(bias=bad_value(np.inf), bias_mask=m), dict(bias=ones), dict(bias_mask=m), dict(bias=ones, bias_mask=(True, False)),
               dict(contrast=(1, 1, 1)), dict(contrast=(1, -0.5, 1, 1)), dict(contrast=(0, 0, np.nan, 0)), dict(contrast=(0, np.inf, 0, 0)),
               dict(lowres=(0.4, 0, 0, 0)), dict(lowres=(0, 1.0, 0, 0)), dict(lowres=(0, 0, np.nan, 0)), dict(lowres=(0.5,) * 5)):
        with pytest.raises(ValueError, match="AugParams"):
            data.AugParams((0, 0, 0), **kw)


def test_aug_params():
    from utils import data
    bias = A.random_bias((4, 6, 8), np.random.default_rng(1))
    kw = dict(bias=bias, bias_mask=(True, False, True, False), contrast=(0, 1.2, 0, 0.8), lowres=[0.5, 0, 0, 0.75])
    a = data.AugParams((1, 2, 3), **kw)
    b = data.AugParams((1, 2, 3), bias=bias.copy(), bias_mask=[1, 0, 1, 0], contrast=np.array([0, 1.2, 0, 0.8]), lowres=(0.5, 0, 0, F(0.75)))
    assert a == b and a.at_origin((1, 2, 3)) == a and a.at_origin((0, 0, 0)) != a and a.acquisition_stage() and not a.intensity_stage()
    assert a.at_origin((0, 0, 0)).bias.tobytes() == bias.tobytes() and not a.bias.flags.writeable
    nudged = bias.copy()
    nudged[3, 3, 5, 7] = np.nextafter(nudged[3, 3, 5, 7], F(2.0))
    for change in (dict(bias=nudged), dict(bias_mask=(True, False, True, True)), dict(contrast=(0, 1.2, 0, 0)), dict(lowres=(0.5, 0, 0, 0)),
                   dict(bias=None, bias_mask=None), dict(contrast=None), dict(bias=bias[:, :, :, :4])):
        args = dict(kw)
        args.update(change)
        assert data.AugParams((1, 2, 3), **args) != a
    r = repr(a)
    assert "bias=float32[4, 4, 6, 8]" in r and "bias_mask=(True, False, True, False)" in r and "contrast=(0.0, " in r and "lowres=(0.5, " in r
    plain = data.AugParams((1, 2, 3))
    assert repr(plain) == "AugParams(origin=(1, 2, 3), flip=(False, False, False), scale=None, shift=None)"
    assert not plain.acquisition_stage() and plain.bias is None and plain.bias_mask == (False,) * 4
    assert not data.AugParams((0, 0, 0), bias=bias, bias_mask=(False,) * 4, contrast=(0, 0, 0, 0), lowres=(0, 0, 0, 0)).acquisition_stage()
    with pytest.raises(TypeError):
        data.AugParams((0, 0, 0), (False, False, False), None, None, None, None, None, None, None, None, bias)     # keyword-only


def test_prepare_batch_runs_the_stage_before_the_intensity_stage():
    from utils import data
    rng = np.random.default_rng(8)
    S, crop = (20, 22, 18), (12, 11, 16)
    img, lab = torch.from_numpy(E.random_image(S, rng)), torch.from_numpy(E.blob_labels(S, rng))
    acq = dict(bias=A.random_bias((4, 5, 6), rng), bias_mask=(True, True, False, False), contrast=(1.2, 0, 0.8, 0), lowres=(0.5, 0, 0, 0.8))
    inten = dict(blur=(1.0, 0, 0, 0.6), noise=(0, 0.2, 0, 0), noise_key=77, gamma=(0, 0, 1.4, 0))
    head = ((3, 4, 1), (True, False, True), (1.1, 0.9, 1.0, 1.2), (0.1, -0.2, 0.0, 0.3))
    plain = data.prepare_batch([img], [lab], [data.AugParams(*head)], crop)
    got = data.prepare_batch([img], [lab], [data.AugParams(*head, **acq, **inten)], crop)
    x = A.stage(plain[0][0].numpy(), bias=acq["bias"], bias_mask=acq["bias_mask"], factor=acq["contrast"], zoom=acq["lowres"])
    want = data._intensity_stage_cpu(x.copy(), data.AugParams((0, 0, 0), **inten))
    assert np.array_equal(_bits(got[0][0].numpy()), _bits(want))
    assert torch.equal(got[1], plain[1]) and torch.equal(got[2], plain[2])
    swapped = A.stage(data._intensity_stage_cpu(plain[0][0].numpy().copy(), data.AugParams((0, 0, 0), **inten)), bias=acq["bias"],
                      bias_mask=acq["bias_mask"], factor=acq["contrast"], zoom=acq["lowres"])
    assert not np.array_equal(_bits(want[0]), _bits(swapped[0]))
    only = data.prepare_batch([img], [lab], [data.AugParams(*head, **acq)], crop)
    assert np.array_equal(_bits(only[0][0].numpy()), _bits(x))
    out = tuple(torch.zeros_like(t) for t in got)
    again = data.prepare_batch([img], [lab], [data.AugParams(*head, **acq, **inten)], crop, out=out)
    assert again[0] is out[0] and torch.equal(out[0].view(torch.int32), got[0].view(torch.int32))


def test_device_brats_cpu_cached_equals_staged():
    from utils import data
    rng = np.random.default_rng(5)
    subjects = [(torch.from_numpy(E.random_image(S, rng)), torch.from_numpy(E.blob_labels(S, rng))) for S in ((20, 22, 18), (18, 20, 24))]
    crop = (12, 12, 16)
    kw = dict(seed=3, flip=True, intensity=0.2, rotate=10.0, blur=1.0)
    new = dict(bias=0.5, bias_grid=5, contrast=0.3, lowres=0.5)
    base = data.DeviceBraTS(subjects, "cpu", crop, **kw)
    on = data.DeviceBraTS(subjects, "cpu", crop, **kw, **new)
    staged = data.DeviceBraTS(subjects, "cpu", crop, cache=False, **kw, **new)
    assert (on.bias, on.bias_grid, on.contrast, on.lowres) == (0.5, 5, 0.3, 0.5)
    changed, steps = 0, set()
    for epoch in range(4):
        for d in (base, on, staged):
            d.set_epoch(epoch)
        want, full, st = base.batch([0, 1]), on.batch([0, 1]), staged.batch([0, 1])
        assert torch.equal(st[0].view(torch.int32), full[0].view(torch.int32)) and torch.equal(st[1], full[1]) and torch.equal(st[2], full[2])
        assert torch.equal(full[1], want[1]) and torch.equal(full[2], want[2])                   # target and edge are not touched
        for b in (0, 1):
            p = on.params(b)
            assert p == staged.params(b)
            for c in range(4):
                touched = p.bias_mask[c] or p.contrast[c] > 0.0 or p.lowres[c] > 0.0
                same = torch.equal(full[0][b, c].view(torch.int32), want[0][b, c].view(torch.int32))
                assert touched or same
                changed += not same
            steps.update(k for k in ("bias_mask", "contrast", "lowres") if any(getattr(p, k)))
    assert changed > 0 and steps == {"bias_mask", "contrast", "lowres"}
    with pytest.raises(ValueError, match="bias_grid"):
        data.DeviceBraTS(subjects, "cpu", crop, bias=0.5, bias_grid=9)


def test_train_flags():
    import train_no_amp as T
    a = T.build_parser().parse_args([])
    assert (a.aug_bias, a.aug_bias_grid, a.aug_contrast, a.aug_lowres) == (0.0, 4, 0.0, 0.0)
    T.check_acquisition_aug(a)
    for flag in ("--aug_bias", "--aug_contrast", "--aug_lowres"):
        with pytest.raises(SystemExit, match="device_data"):
            T.main(["--synthetic", "1", flag, "0.5"])
    for flag, bad in (("--aug_bias", "1.5"), ("--aug_bias", "-1"), ("--aug_bias", "nan"), ("--aug_contrast", "1.0"), ("--aug_contrast", "-0.1"),
                      ("--aug_lowres", "0.4"), ("--aug_lowres", "1.0"), ("--aug_lowres", "nan")):
        with pytest.raises(SystemExit, match=flag + " takes"):
            T.main(["--synthetic", "1", "--device_data", "cache", flag, bad])
    with pytest.raises(SystemExit, match="--aug_bias_grid takes 4..8"):
        T.main(["--synthetic", "1", "--device_data", "staged", "--aug_bias", "0.5", "--aug_bias_grid", "9"])
    c = T.build_parser().parse_args(["--synthetic", "1", "--device_data", "cache", "--aug_bias", "0.4", "--aug_bias_grid", "6", "--aug_contrast",
                                     "0.25", "--aug_lowres", "0.5", "--input_H", "20", "--input_W", "18", "--output_D", "16", "--crop_H", "8",
                                     "--crop_W", "8", "--crop_D", "8"])
    T.check_acquisition_aug(c)
    ds = T.make_device_dataset(c, "cpu")
    assert (ds.bias, ds.bias_grid, ds.contrast, ds.lowres) == (0.4, 6, 0.25, 0.5)
    assert ds.params(0).bias.shape == (4, 6, 6, 6)
