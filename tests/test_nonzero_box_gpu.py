"""The nonzero box on the device: cwf_nonzero_box against the float-free statement of tests/nonzero_box_ref.py (bit-equal, on every
volume shape, input family, alignment and batch stride), cwf_window_gather_box / cwf_window_finalize_box against the plain entry
points on the contiguous crop, sliding_window_inference(crop_nonzero=True) against its crop-and-paste statement with a pointwise
stand-in and with the real model, validate_softmax(window={"crop_nonzero": True}), DeviceBraTS(crop_nonzero=True) in its three
modes, and the argument checks of the three new entry points."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import nonzero_box_ref as ref
import predict_overlap as po
from oracle import reference_model as rm
from utils import data
from utils import synthetic as syn

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BADARG, TOOLARGE, ALIGN = -1, -2, -3
SHAPES = [(37, 29, 23), (5, 3, 300), (300, 3, 5), (9, 7, 1)]


def _zeros(shape):
    x = np.zeros((4,) + shape, dtype=np.float32)
    x[:, ::2] = -0.0                                            # background of both signs
    return x


def _bits(shape, where, channel, bits):
    x = _zeros(shape)
    x.view(np.uint32)[(channel,) + tuple(where)] = bits
    return x


def _dense(shape, lo, hi, seed):
    x = _zeros(shape)
    sl = tuple(slice(a, b) for a, b in zip(lo, hi))
    x[(slice(None),) + sl] = np.random.default_rng(seed).standard_normal((4,) + tuple(b - a for a, b in zip(lo, hi))).astype(np.float32)
    return x


def _families(shape):
    """name -> x float32 [4, *shape]"""
    fam = {"minus zero": -np.zeros((4,) + shape, dtype=np.float32)}
    corners = [tuple((s - 1) * ((k >> d) & 1) for d, s in enumerate(shape)) for k in range(8)]
    for k, c in enumerate(corners):
        fam["corner %d" % k] = _bits(shape, c, k % 4, 0x3F800000)
    mid = tuple(s // 2 for s in shape)
    fam["interior"] = _bits(shape, mid, 0, 0xBF800000)
    fam["channel 3 only"] = _bits(shape, mid, 3, 0x3F800000)
    fam["denormal"] = _bits(shape, mid, 1, 0x00000001)
    fam["negative denormal"] = _bits(shape, mid, 2, 0x80000001)
    fam["nan"] = _bits(shape, mid, 2, 0x7FC00000)
    fam["inf"] = _bits(shape, mid, 1, 0xFF800000)
    inner_lo, inner_hi = tuple(min(1, s - 1) for s in shape), tuple(max(s - 1, min(1, s - 1) + 1) for s in shape)
    fam["dense inner"] = _dense(shape, inner_lo, inner_hi, 1)
    for d in range(3):                                          # a dense box touching each face in turn
        lo, hi = list(inner_lo), list(inner_hi)
        lo[d] = 0
        fam["dense low face %d" % d] = _dense(shape, lo, hi, 2 + d)
        lo, hi = list(inner_lo), list(inner_hi)
        hi[d] = shape[d]
        fam["dense high face %d" % d] = _dense(shape, lo, hi, 5 + d)
    return fam


def _strided(x, offset=0, pad=0):
    """x [B, 4, S] (numpy) on the device at `offset` floats past an allocation's base, samples 4 V + pad floats apart"""
    B, V4 = x.shape[0], int(np.prod(x.shape[1:]))
    stride = V4 + pad
    buf = torch.full((offset + B * stride + 8,), float("nan"), device=DEV)       # NaN is nonzero: a read outside a sample shows
    view = torch.as_strided(buf, tuple(x.shape), (stride,) + tuple(torch.from_numpy(x[0]).stride()), offset)
    view.copy_(torch.from_numpy(x))
    return view


def _check(hip, x, view):
    want_box, want_count = ref.boxes_counts(x)
    box, count = hip.nonzero_box(view)
    assert box.dtype == torch.int32 and count.dtype == torch.int64 and box.is_cuda
    got_box, got_count = box.cpu().numpy(), count.cpu().numpy()
    assert np.array_equal(got_box, want_box), (got_box, want_box)
    assert np.array_equal(got_count, want_count), (got_count, want_count)


# ------------------------------------------------------------------ the kernel against the statement
@pytest.mark.parametrize("shape", SHAPES)
def test_box_and_count_are_bit_equal_to_the_statement(hip, shape):
    for name, x in _families(shape).items():
        view = _strided(x[None])
        assert view.data_ptr() % 16 == 0
        _check(hip, x[None], view)
    fam = _families(shape)
    assert ref.box_count(fam["minus zero"])[1] == 0 and ref.box_count(fam["denormal"])[1] == 1


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("offset", [1, 2, 3])
def test_pointers_of_any_alignment(hip, shape, offset):
    fam = _families(shape)
    for name in ("corner 0", "corner 7", "dense inner", "dense low face 2", "dense high face 2", "minus zero"):
        view = _strided(fam[name][None], offset=offset)
        assert view.data_ptr() % 16 == 4 * offset
        _check(hip, fam[name][None], view)


@pytest.mark.parametrize("shape", SHAPES)
def test_batches_and_batch_strides(hip, shape):
    fam = _families(shape)
    x = np.stack([fam["dense low face 0"], fam["minus zero"], fam["corner 5"]])            # three boxes, one sample empty
    for offset, pad in ((0, 0), (0, 7), (1, 5), (3, 4096)):
        view = _strided(x, offset, pad)
        assert view.stride(0) == 4 * int(np.prod(shape)) + pad
        _check(hip, x, view)
    _check(hip, x, torch.from_numpy(x).to(DEV))


def test_one_full_size_subject(hip):
    shape = (240, 240, 155)
    xm, _ = syn.synthetic_masked_volume(0, shape)
    d = xm.to(DEV)[None]
    box, count = hip.nonzero_box(d)
    torch.cuda.synchronize()
    x = xm.numpy()[None]
    want_box, want_count = ref.boxes_counts(x)
    assert tuple(want_box[0]) == (50, 35, 8, 190, 205, 148)
    assert np.array_equal(box.cpu().numpy(), want_box) and np.array_equal(count.cpu().numpy(), want_count)
    assert data.nonzero_box(d[0]) == data.nonzero_box(xm) == ((50, 35, 8), (190, 205, 148))
    assert po.nonzero_box(d, 3) == ref.union_box(want_box, shape, 3) == ((47, 32, 5), (193, 208, 151))
    d.zero_()
    d[0, 3, 239, 239, 154] = 1.0                               # the last voxel of the last channel alone
    d[0, 1, 0, 0, 0] = -1.0
    box, count = hip.nonzero_box(d)
    assert box.cpu().tolist() == [[0, 0, 0, 240, 240, 155]] and count.cpu().tolist() == [2]


def _raw_call(hip, view, fill):
    """cwf_nonzero_box on buffers pre-filled with `fill` bytes (guard bytes behind box and count): rc and their bytes afterwards"""
    B, (S0, S1, S2) = view.shape[0], view.shape[2:]
    nbytes = hip.lib.cwf_nonzero_box_workspace(B, S0, S1, S2)
    assert nbytes > 0 and nbytes % 256 == 0
    ws = torch.full((nbytes,), fill, dtype=torch.uint8, device=DEV)
    box = torch.full((24 * B + 64,), fill, dtype=torch.uint8, device=DEV)
    count = torch.full((8 * B + 64,), fill, dtype=torch.uint8, device=DEV)
    rc = hip.lib.cwf_nonzero_box(view.data_ptr(), view.stride(0), B, S0, S1, S2, box.data_ptr(), count.data_ptr(), ws.data_ptr(),
                                 torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc, box.cpu().numpy(), count.cpu().numpy()


@pytest.mark.parametrize("shape", [(37, 29, 23), (5, 3, 300)])
def test_buffers_are_fully_written_and_calls_repeat(hip, shape):
    fam = _families(shape)
    for names in (("dense inner", "minus zero", "corner 3"), ("minus zero", "minus zero", "minus zero")):
        x = np.stack([fam[n] for n in names])
        view = _strided(x, 1, 9)
        want_box, want_count = ref.boxes_counts(x)
        first, again = _raw_call(hip, view, 0xFF), _raw_call(hip, view, 0x00)
        for rc, box, count in (first, again):
            assert rc == 0
            assert np.array_equal(box[:72].view(np.int32).reshape(3, 6), want_box)
            assert np.array_equal(count[:24].view(np.int64), want_count)
        assert bool((first[1][72:] == 0xFF).all()) and bool((first[2][24:] == 0xFF).all())          # and nothing behind them


def test_out_rows_and_graph_capture(hip):
    """out= fills one subject's rows of a bigger pair; the call records into a graph (no synchronisation, nothing read back) and a
    replay follows x's current content"""
    shape = (9, 7, 11)
    fam = _families(shape)
    boxes = torch.full((3, 6), -7, dtype=torch.int32, device=DEV)
    counts = torch.full((3,), -1, dtype=torch.int64, device=DEV)
    d = torch.from_numpy(fam["dense inner"])[None].to(DEV)
    hip.nonzero_box(d, out=(boxes[1:2], counts[1:2]))
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        hip.nonzero_box(d, out=(boxes[1:2], counts[1:2]))
    for name in ("corner 6", "minus zero", "dense inner"):
        d.copy_(torch.from_numpy(fam[name])[None])
        boxes.fill_(-7)
        counts.fill_(-1)
        g.replay()
        torch.cuda.synchronize()
        want = ref.box_count(fam[name])
        assert np.array_equal(boxes[1].cpu().numpy(), want[0]) and int(counts[1]) == want[1], name
        assert bool((boxes[[0, 2]] == -7).all()) and bool((counts[[0, 2]] == -1).all())


# ------------------------------------------------------------------ windows on a sub-box
GATHER_BOXES = {"interior": ((9, 20, 6), (120, 171, 90)), "short axis": ((40, 3, 10), (131, 43, 97)), "whole": ((0, 0, 0), (131, 181, 97))}


@pytest.mark.parametrize("name", sorted(GATHER_BOXES))
@pytest.mark.parametrize("nb", [1, 3])
def test_gather_box_equals_gather_of_the_crop(hip, name, nb):
    full, roi = (131, 181, 97), (48, 64, 40)
    lo, hi = GATHER_BOXES[name]
    ext = tuple(b - a for a, b in zip(lo, hi))
    x = torch.randn((nb, 4) + full, generator=torch.Generator().manual_seed(11)).to(DEV)       # dense: a read outside the box shows
    crop = x[:, :, lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]].contiguous()
    starts = po.window_grid(ext, roi, 0.5)
    nw = len(po.windows(starts))
    grid, box = hip.window_grid(nb, ext, roi, starts), hip.window_box(full, lo)
    for w0 in range(0, nw, 8):
        cnt = min(8, nw - w0)
        got, want = hip.window_gather_box(x, grid, box, w0, cnt), hip.window_gather(crop, grid, w0, cnt)
        assert tuple(got.shape) == (cnt * nb, 4) + roi and got.permute(0, 2, 3, 4, 1).is_contiguous()
        assert torch.equal(got, want), (name, w0)
    if nb == 1:                                                 # and the statement itself, for the first and the last window
        want = ref.gather_box(x.cpu().numpy(), (lo, hi), starts, roi)
        for w in (0, nw - 1):
            assert np.array_equal(hip.window_gather_box(x, grid, box, w, 1).cpu().numpy(), want[w])
        if name == "short axis":
            assert bool((want[0][:, :, :, 40:, :] == 0).all())                             # beyond the box: zero, though x is not


@pytest.mark.parametrize("overlap", [0.0, 0.5])
@pytest.mark.parametrize("box", [((3, 0, 5), (30, 29, 20)), ((0, 0, 0), (37, 29, 23)), ((36, 28, 0), (37, 29, 9))],
                         ids=["inner", "whole", "corner"])
def test_finalize_box_writes_every_voxel_once(hip, overlap, box):
    full, roi, nb = (37, 29, 23), (16, 12, 10), 2
    lo, hi = box
    ext = tuple(b - a for a, b in zip(lo, hi))
    starts = po.window_grid(ext, roi, overlap)
    nw = len(po.windows(starts))
    probs = torch.rand((nw, nb, 4) + roi, generator=torch.Generator().manual_seed(int(overlap * 10) + lo[0])).to(DEV)
    tabs = torch.from_numpy(np.concatenate(po.importance_tables(roi, "gaussian"))).to(DEV)
    grid, wbox = hip.window_grid(nb, ext, roi, starts), hip.window_box(full, lo)
    outs = []
    for chunk in (1, 3, nw):
        acc = torch.empty((nb,) + ext + (4,), device=DEV)
        for w0 in range(0, nw, chunk):
            cnt = min(chunk, nw - w0)
            hip.window_blend(probs[w0:w0 + cnt].reshape((cnt * nb, 4) + roi), tabs, acc, grid, w0, cnt, w0 > 0)
        y = torch.full((nb, 4) + full, float("nan"), device=DEV)
        assert hip.window_finalize_box(acc, tabs, grid, wbox, out=y) is y
        outs.append(y)
    inner = hip.window_finalize(acc, tabs, grid)
    y = outs[-1]
    assert not bool(torch.isnan(y).any())
    assert torch.equal(y[:, :, lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]], inner)
    assert np.array_equal(y.cpu().numpy(), ref.paste(inner.cpu().numpy(), full, lo))       # outside: exactly (1, 0, 0, 0)
    assert torch.equal(hip.window_finalize_box(acc, tabs, grid, wbox), y)
    for o in outs[:-1]:
        assert torch.equal(o, y)                                # chunk sizes 1, 3, all: bitwise identical


# ------------------------------------------------------------------ sliding_window_inference(crop_nonzero=True)
class _Softmax:
    """the pointwise stand-in of test_sliding_window_gpu.py, counting the windows it is given"""

    def __init__(self):
        self.windows = 0

    def __call__(self, xb, mm):
        assert xb.permute(0, 2, 3, 4, 1).is_contiguous()
        self.windows += xb.shape[0]
        return (torch.softmax(xb.double(), dim=1).float(),)


def _statement(x, box, model, **kw):
    """crop x to the box, today's sliding_window_inference on the contiguous crop, paste into background"""
    infer = lambda crop: po.sliding_window_inference(torch.from_numpy(crop).to(DEV), None, model, **kw).cpu().numpy()      # noqa: E731
    return ref.crop_and_paste(x.cpu().numpy(), box, infer)


def test_pointwise_model_on_the_box(hip):
    full, box = (137, 181, 96), ((5, 20, 3), (130, 170, 90))
    x = syn.synthetic_masked_volume(1, full, box)[0][None].to(DEV)
    off = _Softmax()
    whole = po.sliding_window_inference(x, None, off)
    assert off.windows == ref.window_count(full, (128,) * 3, 0.5, po.window_grid) == 4
    for margin, want_box in ((0, box), (5, ((0, 15, 0), (135, 175, 95))), (40, ((0, 0, 0), full))):
        assert po.nonzero_box(x, margin) == ref.union_box(ref.boxes_counts(x.cpu().numpy())[0], full, margin) == want_box
        m = _Softmax()
        got = po.sliding_window_inference(x, None, m, crop_nonzero=True, nonzero_margin=margin)
        ext = tuple(b - a for a, b in zip(*want_box))
        assert m.windows == ref.window_count(ext, (128,) * 3, 0.5, po.window_grid) == {0: 2, 5: 4, 40: 4}[margin]
        assert got.shape == x.shape
        assert np.array_equal(got.cpu().numpy(), _statement(x, want_box, _Softmax()))
        if margin == 40:                                        # the box is the volume: the off path itself
            assert torch.equal(got, whole)
    got = po.sliding_window_inference(x, None, _Softmax(), crop_nonzero=True, sw_batch_size=1, blend="constant")
    assert np.array_equal(got.cpu().numpy(), _statement(x, box, _Softmax(), blend="constant"))
    z = torch.zeros_like(x)
    z[:, :, ::2] = -0.0
    m = _Softmax()
    assert torch.equal(po.sliding_window_inference(z, None, m, crop_nonzero=True), po.sliding_window_inference(z, None, _Softmax()))
    assert m.windows == 4                                       # no box: the whole volume


def test_two_samples_take_the_union(hip):
    full = (137, 140, 96)
    a = syn.synthetic_masked_volume(1, full, ((5, 20, 3), (60, 100, 50)))[0]
    b = syn.synthetic_masked_volume(2, full, ((40, 10, 30), (120, 90, 90)))[0]
    x = torch.stack([a, b, torch.zeros_like(a)]).to(DEV)
    box = ((5, 10, 3), (120, 100, 90))
    assert po.nonzero_box(x) == box
    m = _Softmax()
    got = po.sliding_window_inference(x, None, m, crop_nonzero=True)
    assert m.windows == 3                                       # one window, three samples
    assert np.array_equal(got.cpu().numpy(), _statement(x, box, _Softmax()))


@functools.lru_cache(maxsize=None)
def _model():
    from models.clswiseformer.cls_wise_former import get_cls_wise_former
    m = get_cls_wise_former(dataset="brats", _conv_repr=True, _pe_type="fixed")
    m.load_state_dict(syn.det_state_dict(rm.param_shapes()), strict=False)
    m.Unet_list.InitConv.dropout = 0.0
    return m.to(DEV).eval()


REAL_FULL, REAL_BOX = (144, 150, 136), ((10, 12, 5), (130, 138, 125))


def test_real_model_on_the_box(hip):
    m = _model()
    x = syn.synthetic_masked_volume(3, REAL_FULL, REAL_BOX)[0][None].to(DEV)
    assert po.nonzero_box(x) == REAL_BOX
    got = po.sliding_window_inference(x, None, m, crop_nonzero=True)
    assert got.shape == x.shape
    assert np.array_equal(got.cpu().numpy(), _statement(x, REAL_BOX, m))


def test_validate_softmax_crop_nonzero(hip):
    m = _model()
    x, t = syn.synthetic_masked_volume(3, REAL_FULL, REAL_BOX)
    x, t = x[None].to(DEV), t[None].to(DEV)
    win = {"roi_size": (128, 128, 128), "overlap": 0.5, "crop_nonzero": True}
    seg, prob, dice = po.validate_softmax(x, t, m, window=win)
    assert prob.shape == (1, 4) + REAL_FULL and seg.shape == (1,) + REAL_FULL and len(dice) == 3
    assert torch.equal(prob, po.sliding_window_inference(x, None, m, **win)) and torch.equal(seg, prob.argmax(1))
    outside = torch.ones(REAL_FULL, dtype=torch.bool, device=DEV)
    lo, hi = REAL_BOX
    outside[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]] = False
    assert int(outside.sum()) > 0 and bool((seg[0][outside] == 0).all())
    assert bool((prob[0, 0][outside] == 1).all()) and bool((prob[0, 1:][:, outside] == 0).all())


# ------------------------------------------------------------------ DeviceBraTS(crop_nonzero=True)
FULL, CROP = (40, 36, 31), (16, 20, 24)
BOXES = [((6, 5, 4), (30, 29, 27)), ((12, 0, 10), (20, 36, 18)), None]          # the last subject is zero everywhere


@functools.lru_cache(maxsize=None)
def _subjects():
    out = []
    for i, box in enumerate(BOXES):
        if box is None:
            x, t = syn.synthetic_volume(i, FULL, 4321)
            x, t = x * 0.0, t * 0
        else:
            x, t = syn.synthetic_masked_volume(i, FULL, box, 4321)
        out.append((x, t.to(torch.uint8)))
    return out


@pytest.mark.parametrize("normalize", [False, True])
def test_device_modes_agree_with_the_host(hip, normalize):
    order = [[2, 0, 1]]
    kw = dict(seed=5, normalize=normalize)
    host = data.DeviceBraTS(_subjects(), "cpu", CROP, crop_nonzero=True, **kw)
    cached = data.DeviceBraTS(_subjects(), DEV, CROP, cache=True, crop_nonzero=True, **kw)
    staged = data.DeviceBraTS(_subjects(), DEV, CROP, cache=False, crop_nonzero=True, **kw)
    off = data.DeviceBraTS(_subjects(), DEV, CROP, cache=True, crop_nonzero=False, **kw)
    plain = data.DeviceBraTS(_subjects(), DEV, CROP, cache=True, **kw)
    want_boxes = {i: (FULL + (0, 0, 0) if b is None else b[0] + b[1]) for i, b in enumerate(BOXES)}
    assert cached.source.boxes == want_boxes == host.source.boxes                         # the raw image's, normalised or not
    moved = 0
    for epoch in (0, 1, 2):
        for ds in (host, cached, staged, off, plain):
            ds.set_epoch(epoch)
        want = next(iter(host.batches(order)))[:3]
        for ds in (cached, staged):
            got = next(iter(ds.batches(order)))[:3]
            for a, b in zip(got, want):
                assert a.is_cuda and a.dtype == b.dtype and torch.equal(a.cpu(), b), (epoch, ds.cache)
        for i, box in enumerate(BOXES):
            o = cached.params(i).origin
            assert o == staged.params(i).origin == host.params(i).origin
            if box is None:
                assert o == plain.params(i).origin
                continue
            moved += o != plain.params(i).origin
            for d in range(3):
                assert ref.overlap(o[d], CROP[d], box[0][d], box[1][d]) == min(CROP[d], box[1][d] - box[0][d])
        for a, b in zip(next(iter(off.batches(order))), next(iter(plain.batches(order)))):
            assert torch.equal(a, b)
    assert moved >= 3 and staged.source.boxes == want_boxes


# ------------------------------------------------------------------ bad arguments
def test_nonzero_box_error_codes_come_before_any_launch(hip):
    from cwf import _lib
    lib = hip.lib
    S = (5, 3, 7)
    assert lib.cwf_nonzero_box_workspace(1, *S) == 256 and lib.cwf_nonzero_box_workspace(3, 240, 240, 155) % 256 == 0
    for b, s in ((0, S), (-1, S), (1, (0, 3, 7)), (1, (5, -1, 7)), (1, (5, 3, 0))):
        assert lib.cwf_nonzero_box_workspace(b, *s) == BADARG, (b, s)
    for b, s in ((1, (2048, 1024, 1024)), (1, (2 ** 31 - 1, 2 ** 31 - 1, 2 ** 31 - 1)), (65536, S)):
        assert lib.cwf_nonzero_box_workspace(b, *s) == TOOLARGE, (b, s)
    assert lib.cwf_nonzero_box_workspace(1, 2 ** 31 - 1, 1, 1) > 0
    x = torch.ones((2, 4) + S, device=DEV)
    ws = torch.full((1024,), 0xFF, dtype=torch.uint8, device=DEV)
    box = torch.full((2, 6), -7, dtype=torch.int32, device=DEV)
    count = torch.full((2,), -1, dtype=torch.int64, device=DEV)
    assert ws.data_ptr() % 256 == 0
    st = torch.cuda.current_stream().cuda_stream
    V4 = 4 * 105

    def call(xp=x.data_ptr(), bs=V4, b=2, s=S, bp=box.data_ptr(), cp=count.data_ptr(), w=ws.data_ptr()):
        return lib.cwf_nonzero_box(xp, bs, b, s[0], s[1], s[2], bp, cp, w, st)

    bad = {"null x": dict(xp=None), "null box": dict(bp=None), "null count": dict(cp=None), "null ws": dict(w=None), "B = 0": dict(b=0),
           "B < 0": dict(b=-2), "S0 = 0": dict(s=(0, 3, 7)), "S1 < 0": dict(s=(5, -3, 7)), "S2 = 0": dict(s=(5, 3, 0)),
           "samples overlap": dict(bs=V4 - 1)}
    for name, kw in bad.items():
        assert call(**kw) == BADARG, name
    assert call(s=(2048, 1024, 1024), bs=2 ** 33) == TOOLARGE and call(b=65536) == TOOLARGE
    for name, kw in {"ws off 256": dict(w=ws.data_ptr() + 64), "x off 4": dict(xp=x.data_ptr() + 2), "box off 4": dict(bp=box.data_ptr() + 1),
                     "count off 8": dict(cp=count.data_ptr() + 4)}.items():
        assert call(**kw) == ALIGN, name
    torch.cuda.synchronize()
    assert bool((box == -7).all()) and bool((count == -1).all()) and bool((ws == 0xFF).all())       # nothing ran
    assert call() == 0
    torch.cuda.synchronize()
    assert box.cpu().tolist() == [[0, 0, 0, 5, 3, 7]] * 2 and count.cpu().tolist() == [105, 105]
    for bad_x in (x.double(), x[:, :3], x[0], x.cpu()):
        with pytest.raises(ValueError):
            hip.nonzero_box(bad_x)
    with pytest.raises(ValueError):
        hip.nonzero_box(x, out=(box[:1], count))
    assert _lib.NONZERO_BOX_TILE == 4096


def test_window_box_error_codes_come_before_any_launch(hip):
    full, ext, roi, lo = (20, 22, 24), (12, 20, 9), (8, 8, 8), (5, 2, 15)
    x = torch.zeros((1, 4) + full, device=DEV)
    starts = po.window_grid(ext, roi, 0.5)
    nw = len(po.windows(starts))
    tabs = torch.from_numpy(np.concatenate(po.importance_tables(roi, "gaussian"))).to(DEV)
    acc = torch.full((1,) + ext + (4,), 0.25, device=DEV)
    win = torch.full((1, 8, 8, 8, 4), -3.0, device=DEV)
    y = torch.full((1, 4) + full, -3.0, device=DEV)
    lib, st = hip.lib, hip._stream()
    good, gbox = hip.window_grid(1, ext, roi, starts), hip.window_box(full, lo)
    ref_ = ctypes.byref

    def gather(xp=x.data_ptr(), wp=win.data_ptr(), g=good, b=gbox, w0=0, cnt=1):
        return lib.cwf_window_gather_box(xp, wp, None if g is None else ref_(g), None if b is None else ref_(b), w0, cnt, st)

    def finalize(ap=acc.data_ptr(), tp=tabs.data_ptr(), yp=y.data_ptr(), g=good, b=gbox):
        return lib.cwf_window_finalize_box(ap, tp, yp, None if g is None else ref_(g), None if b is None else ref_(b), st)

    bad_grids = [hip.window_grid(1, ext, roi, ([0, 12], starts[1], starts[2])), hip.window_grid(1, ext, roi, ([-8], starts[1], starts[2])),
                 hip.window_grid(0, ext, roi, starts), hip.window_grid(1, ext, (8, 0, 8), starts), None]
    bad_boxes = [hip.window_box(full, (9, 2, 15)), hip.window_box(full, (5, 3, 15)), hip.window_box(full, (5, 2, 16)),       # past a far face
                 hip.window_box(full, (-1, 2, 15)), hip.window_box((20, 0, 24), lo), hip.window_box((11, 22, 24), (0, 2, 15)), None]
    for g in bad_grids:
        assert gather(g=g) == BADARG and finalize(g=g) == BADARG
    for b in bad_boxes:
        assert gather(b=b) == BADARG and finalize(b=b) == BADARG
    huge = hip.window_box((2048, 1024, 1024), lo)
    assert gather(b=huge) == TOOLARGE and finalize(b=huge) == TOOLARGE
    for kw in (dict(xp=None), dict(wp=None), dict(wp=win.data_ptr() + 4), dict(xp=x.data_ptr() + 2), dict(cnt=0), dict(w0=nw), dict(w0=-1),
               dict(w0=nw - 1, cnt=2)):
        assert gather(**kw) == BADARG, kw
    for kw in (dict(ap=None), dict(tp=None), dict(yp=None), dict(ap=acc.data_ptr() + 4), dict(tp=tabs.data_ptr() + 2), dict(yp=y.data_ptr() + 1)):
        assert finalize(**kw) == BADARG, kw
    torch.cuda.synchronize()
    assert bool((win == -3).all()) and bool((y == -3).all())   # nothing ran
    assert gather() == 0 and finalize() == 0
    torch.cuda.synchronize()
    assert bool((win == 0).all())
    assert np.array_equal(y.cpu().numpy(), ref.paste(hip.window_finalize(acc, tabs, good).cpu().numpy(), full, lo))
