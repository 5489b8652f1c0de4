"""Sliding-window inference on the device (csrc/window.hip through predict_overlap.sliding_window_inference): the gather against
torch slicing, blend + finalize against the float64 reference of tests/sliding_window_ref.py within its bound and bitwise independent
of the chunk size, a pointwise stand-in model reproduced on any volume (and tailor_and_concat's misplacement caught), the real model
against a host restatement, validate_softmax(window=...) and argument checks."""
import ctypes

import numpy as np
import pytest
import torch

import hausdorff_ref as H
import predict_overlap as po
import sliding_window_ref as R
from oracle import reference_model as rm
from utils import synthetic as syn

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _model():
    from models.clswiseformer.cls_wise_former import get_cls_wise_former
    m = get_cls_wise_former(dataset="brats", _conv_repr=True, _pe_type="fixed")
    m.load_state_dict(syn.det_state_dict(rm.param_shapes()), strict=False)
    m.Unet_list.InitConv.dropout = 0.0
    return m.to(DEV).eval()


def _tables_dev(roi, blend):
    return torch.from_numpy(np.concatenate(po.importance_tables(roi, blend))).to(DEV)


# ------------------------------------------------------------------ gather
@pytest.mark.parametrize("shape", [(131, 181, 97), (131, 40, 97)], ids=["ragged", "short-axis"])
@pytest.mark.parametrize("nb", [1, 3])
def test_gather_bit_exact(hip, shape, nb):
    roi = (48, 64, 40)
    g = torch.Generator().manual_seed(11)
    x = torch.randn((nb, 4) + shape, generator=g)
    starts = po.window_grid(shape, roi, 0.5)
    nw = len(po.windows(starts))
    want = torch.from_numpy(R.gather(x.numpy(), starts, roi))                    # [nw, B, 4, r0, r1, r2]
    grid = hip.window_grid(nb, shape, roi, starts)
    xd = x.to(DEV)
    for w0, cnt in ((0, nw), (2, 3), (nw - 1, 1)):
        xb = hip.window_gather(xd, grid, w0, cnt)
        assert tuple(xb.shape) == (cnt * nb, 4) + roi
        cl = xb.permute(0, 2, 3, 4, 1)
        assert cl.is_contiguous() and cl.contiguous().data_ptr() == xb.data_ptr()      # the model's permute copies nothing
        got = xb.cpu().reshape((cnt, nb, 4) + roi)
        assert torch.equal(got, want[w0:w0 + cnt])


# ------------------------------------------------------------------ blend + finalize
def _blend_dev(hip, probs, starts, roi, shape, blend, chunk):
    """probs: device [nw, B, 4, r0, r1, r2] (plain NCDHW per chunk: window_blend makes it channels-last)"""
    nw, nb = probs.shape[:2]
    grid = hip.window_grid(nb, shape, roi, starts)
    tabs = _tables_dev(roi, blend)
    acc = torch.empty((nb,) + shape + (4,), device=DEV)
    for w0 in range(0, nw, chunk):
        cnt = min(chunk, nw - w0)
        hip.window_blend(probs[w0:w0 + cnt].reshape((cnt * nb, 4) + roi), tabs, acc, grid, w0, cnt, w0 > 0)
    return hip.window_finalize(acc, tabs, grid)


@pytest.mark.parametrize("overlap", [0.0, 0.25, 0.5, 0.75])
@pytest.mark.parametrize("blend", ["gaussian", "constant"])
def test_blend_finalize_within_bound_and_chunk_invariant(hip, overlap, blend):
    shape, roi, nb = (37, 29, 23), (16, 12, 10), 2
    starts = po.window_grid(shape, roi, overlap)
    nw = len(po.windows(starts))
    g = torch.Generator().manual_seed(int(overlap * 100) + len(blend))
    probs = torch.rand((nw, nb, 4) + roi, generator=g)
    ref = R.blend(probs.numpy(), starts, roi, shape, po.importance_tables(roi, blend))
    k = R.max_coverage(shape, roi, starts)
    pd = probs.to(DEV)
    outs = [_blend_dev(hip, pd, starts, roi, shape, blend, c) for c in (1, 3, nw, 3)]
    torch.cuda.synchronize()
    got = outs[0].cpu().numpy()
    assert got.shape == (nb, 4) + shape
    assert R.excess(got, ref, k) <= 1.0, R.excess(got, ref, k)
    for o in outs[1:]:
        assert torch.equal(o, outs[0])                  # sw_batch_size 1, 3, all, and a second run: bitwise identical


# ------------------------------------------------------------------ a pointwise stand-in model
def _softmax(xb, mm):
    return (torch.softmax(xb.double(), dim=1).float(),)


def _softmax_model(xb, mm):
    assert xb.permute(0, 2, 3, 4, 1).is_contiguous()    # the gathered windows arrive in channels-last memory
    return _softmax(xb, mm)


@pytest.mark.parametrize("shape", [(240, 240, 155), (137, 181, 96)])
def test_pointwise_model_reproduced(hip, shape):
    x = torch.randn((1, 4) + shape, generator=torch.Generator().manual_seed(3)).to(DEV)
    want = _softmax(x, None)[0]
    starts = po.window_grid(shape, (128,) * 3, 0.5)
    k = R.max_coverage(shape, (128,) * 3, starts)
    for blend in ("gaussian", "constant"):
        got = po.sliding_window_inference(x, None, _softmax_model, blend=blend)
        assert got.shape == want.shape
        assert float((got - want).abs().max()) <= R.gamma(k), blend
    if shape == (240, 240, 155):                    # the reference stitcher misplaces depth 128..154 by 5 voxels
        y = po.tailor_and_concat(x, None, _softmax)
        assert float((y - want)[..., :128].abs().max()) <= R.gamma(k)
        assert float((y - want)[..., 128:].abs().max()) >= 30 * R.gamma(k)


# ------------------------------------------------------------------ the real model
def _restatement(m, x, roi, overlap, blend):
    """each window through m at B = 1 (torch slicing + zero padding), blended by the float64 reference"""
    shape = tuple(x.shape[2:])
    starts = po.window_grid(shape, roi, overlap)
    pad = [max(0, s + r - n) for s, r, n in zip((max(st) for st in starts), roi, shape)]
    xp = torch.nn.functional.pad(x, (0, pad[2], 0, pad[1], 0, pad[0]))
    probs = []
    with torch.no_grad():
        for s in po.windows(starts):
            w = xp[..., s[0]:s[0] + roi[0], s[1]:s[1] + roi[1], s[2]:s[2] + roi[2]]
            probs.append(m(w, None)[0].cpu().numpy())
    return R.blend(probs, starts, roi, shape, po.importance_tables(roi, blend)), R.max_coverage(shape, roi, starts)


def test_real_model_single_window_equals_forward(hip):
    m = _model()
    x, _, _ = syn.synthetic_batch([0], (128, 128, 128))
    x = x.to(DEV)
    with torch.no_grad():
        want = m(x, None)[0]
        got = po.sliding_window_inference(x, None, m, blend="constant")
        assert torch.equal(got, want)
        got = po.sliding_window_inference(x, None, m)
        assert float((got - want).abs().max()) <= R.gamma(1)


@pytest.mark.parametrize("roi", [(128, 128, 128), (160, 192, 160)])
def test_real_model_matches_host_restatement(hip, roi):
    m = _model()
    x = torch.randn(1, 4, 240, 240, 155, generator=torch.Generator().manual_seed(5)).to(DEV)
    got = po.sliding_window_inference(x, None, m, roi_size=roi, overlap=0.5, sw_batch_size=8 if roi[0] == 128 else 2)
    assert got.shape == (1, 4, 240, 240, 155)
    ref, k = _restatement(m, x, roi, 0.5, "gaussian")
    err = np.abs(got.cpu().numpy() - ref).max()
    assert err <= R.gamma(k) + 3e-5, err          # + the model's batch-independence tolerance (test_model_gpu.py)


# ------------------------------------------------------------------ validate_softmax(window=...)
def test_validate_softmax_window_any_shape(hip):
    from utils import tools
    m = _model()
    shape = (144, 160, 120)
    x = torch.randn((1, 4) + shape, generator=torch.Generator().manual_seed(8)).to(DEV)
    target = torch.from_numpy(H.nested_labels(shape, np.random.default_rng(4))[None]).to(DEV)
    win = {"roi_size": (128, 128, 128), "overlap": 0.5}
    seg, prob, dice, hd95 = po.validate_softmax(x, target, m, window=win, with_hd95=True)
    assert prob.shape == (1, 4) + shape and seg.shape == (1,) + shape
    assert torch.equal(prob, po.sliding_window_inference(x, None, m, **win))
    assert torch.equal(seg, prob.argmax(1))
    want = tools.softmax_output_dice(prob.argmax(1).cpu(), target.cpu())
    assert all(abs(float(a) - float(b)) < 1e-6 for a, b in zip(dice, want))
    assert hd95.dtype == torch.float64 and tuple(hd95.shape) == (1, 3) and bool(torch.isfinite(hd95).all())
    seg2, prob2, dice2 = po.validate_softmax(x, target, m, window=win, use_TTA=True)
    want2 = po.flip_tta(x, None, lambda xb, mm: po.sliding_window_inference(xb, mm, m, **win), batch=1)
    assert torch.equal(prob2, want2) and torch.equal(seg2, prob2.argmax(1))


# ------------------------------------------------------------------ bad arguments
def test_bad_arguments(hip):
    from cwf import _lib
    shape, roi = (20, 20, 20), (8, 8, 8)
    x = torch.zeros((1, 4) + shape, device=DEV)
    starts = po.window_grid(shape, roi, 0.5)
    tabs = _tables_dev(roi, "gaussian")
    acc = torch.zeros((1,) + shape + (4,), device=DEV)
    win = torch.zeros((1, 8, 8, 8, 4), device=DEV)
    lib, stream = hip.lib, hip._stream()
    good = hip.window_grid(1, shape, roi, starts)
    outside = hip.window_grid(1, shape, roi, ([0, 20], starts[1], starts[2]))            # a window entirely past the far face
    before = hip.window_grid(1, shape, roi, ([-8], starts[1], starts[2]))               # ... and one entirely before the volume
    empty = hip.window_grid(0, shape, roi, starts)
    zero_roi = hip.window_grid(1, shape, (8, 0, 8), starts)
    E = -1                                              # CWF_E_BADARG
    p = win.data_ptr()
    assert lib.cwf_window_gather(x.data_ptr(), p, ctypes.byref(good), 0, 1, stream) == 0
    for g in (outside, before, empty, zero_roi):
        assert lib.cwf_window_gather(x.data_ptr(), p, ctypes.byref(g), 0, 1, stream) == E
        assert lib.cwf_window_blend(p, tabs.data_ptr(), acc.data_ptr(), ctypes.byref(g), 0, 1, 0, stream) == E
        assert lib.cwf_window_finalize(acc.data_ptr(), tabs.data_ptr(), x.data_ptr(), ctypes.byref(g), stream) == E
    assert lib.cwf_window_gather(None, p, ctypes.byref(good), 0, 1, stream) == E
    assert lib.cwf_window_gather(x.data_ptr(), p + 4, ctypes.byref(good), 0, 1, stream) == E                 # misaligned
    assert lib.cwf_window_gather(x.data_ptr(), p, None, 0, 1, stream) == E
    assert lib.cwf_window_gather(x.data_ptr(), p, ctypes.byref(good), 0, 0, stream) == E                     # no windows
    nw = len(po.windows(starts))
    assert lib.cwf_window_gather(x.data_ptr(), p, ctypes.byref(good), nw, 1, stream) == E                    # past the last
    assert lib.cwf_window_gather(x.data_ptr(), p, ctypes.byref(good), nw - 1, 2, stream) == E
    assert lib.cwf_window_blend(p + 4, tabs.data_ptr(), acc.data_ptr(), ctypes.byref(good), 0, 1, 0, stream) == E
    assert lib.cwf_window_blend(p, tabs.data_ptr(), acc.data_ptr() + 8, ctypes.byref(good), 0, 1, 0, stream) == E
    assert lib.cwf_window_blend(p, None, acc.data_ptr(), ctypes.byref(good), 0, 1, 0, stream) == E
    assert lib.cwf_window_finalize(acc.data_ptr() + 4, tabs.data_ptr(), x.data_ptr(), ctypes.byref(good), stream) == E
    assert lib.cwf_window_finalize(acc.data_ptr(), tabs.data_ptr(), None, ctypes.byref(good), stream) == E
    with pytest.raises(_lib.CwfError):
        hip.window_gather(x, outside, 0, 1)
    torch.cuda.synchronize()
    m = lambda xb, mm: (torch.softmax(xb, 1),)       # noqa: E731
    xv = torch.zeros((1, 4, 130, 130, 130), device=DEV)
    for kw in ({"roi_size": (120, 128, 128)}, {"roi_size": (48, 64, 64)}, {"overlap": 1.0}, {"blend": "box"}, {"sw_batch_size": 0}):
        with pytest.raises(ValueError):
            po.sliding_window_inference(xv, None, m, **kw)
    with pytest.raises(ValueError):
        po.sliding_window_inference(xv.cpu(), None, m)
    with pytest.raises(ValueError):
        po.sliding_window_inference(xv[:, :3], None, m)
