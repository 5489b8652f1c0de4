"""The prediction and evaluation glue on the device against the statement of tests/predict_ref.py: cwf_argmax_dice /
cwf_argmax_metrics (every row of the nine special values, every address form the wrapper derives, padded batch and channel strides,
exact counts, accumulation, guard elements), cwf_label_metrics (a second grid-stride round included), cwf_region_bits, cwf_stitch_windows
(bit patterns, one and two samples), the refusals of the five entry points and of their wrappers, and the two routes of
predict_overlap._validate.  Everything is exact -- integers, bit patterns, or IEEE double arithmetic on the same integers -- except the
comparison with the host expression of the CPU route, which divides in float32."""
import functools

import numpy as np
import pytest
import torch

import predict_overlap as po
import predict_ref as ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BADARG, TOOLARGE = -1, -2
GUARD, SENT = 16, -7777
INF = float("inf")
SHAPES = {1: (1, 1, 1), 63: (3, 3, 7), 64: (4, 4, 4), 65: (5, 1, 13), 255: (3, 5, 17), 256: (4, 8, 8), 257: (1, 257, 1), 1000: (10, 10, 10)}
ENTRIES = {"cwf_argmax_dice": 3, "cwf_argmax_metrics": 6}


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _bits64(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.int64)


@functools.lru_cache(maxsize=None)
def _case(v, nb):
    """(probabilities [nb, 4, *SHAPES[v]], their argmax by the statement, the target families): computed once, never written to"""
    rng = np.random.default_rng(1000 * v + nb)
    p = ref.tied_probabilities(rng, (nb,) + SHAPES[v])
    seg = ref.argmax4(p)
    return p, seg, ref.target_families(rng, seg)


def _forms(p):
    """name -> device view of the values p [B, 4, D0, D1, D2] (numpy): the address forms HipBackend.argmax_dice meets; what lies
    between the elements of a view is +inf, which would win any argmax it entered"""
    t = torch.from_numpy(np.ascontiguousarray(p))
    B, _, D0, D1, D2 = t.shape
    V = D0 * D1 * D2
    out = {"NCDHW": t.to(DEV), "channels-last": t.permute(0, 2, 3, 4, 1).contiguous().to(DEV).permute(0, 4, 1, 2, 3)}
    wide = torch.full((B, 4, D0, D1, D2 + 3), INF)
    wide[..., :D2] = t
    out["cut along the last axis"] = wide.to(DEV)[..., :D2]
    two = torch.full((B, 4, D0, D1, 2 * D2), INF)
    two[..., ::2] = t
    out["::2"] = two.to(DEV)[..., ::2]
    for off in (1, 3):
        for name, strides in (("NCDHW", tuple(t.stride())), ("channels-last", (4 * V, 1, 4 * D1 * D2, 4 * D2, 4))):
            buf = torch.full((off + t.numel() + 4,), INF, device=DEV)
            view = torch.as_strided(buf, tuple(t.shape), strides, off)
            view.copy_(t)
            assert view.data_ptr() == buf.data_ptr() + 4 * off
            out["%s at an offset of %d floats" % (name, off)] = view
    return out


def _launch(hip, entry, prob_ptr, sb, sc, sv, target, B, V, init=None, counts=True):
    """The raw entry point on guarded buffers of its own: (rc, seg buffer, counts buffer) as numpy int64, guards included"""
    nc = ENTRIES[entry] * 3
    seg = torch.full((GUARD + B * V + GUARD,), SENT, dtype=torch.int64, device=DEV)
    cnt = torch.full((GUARD + nc + GUARD,), SENT, dtype=torch.int64, device=DEV)
    cnt[GUARD:GUARD + nc] = 0 if init is None else torch.from_numpy(np.asarray(init, dtype=np.int64).reshape(-1)).to(DEV)
    rc = getattr(hip.lib, entry)(prob_ptr, sb, sc, sv, None if target is None else target.data_ptr(), seg.data_ptr() + 8 * GUARD,
                                 cnt.data_ptr() + 8 * GUARD if counts else None, B, V, _stream())
    torch.cuda.synchronize()
    return rc, seg.cpu().numpy(), cnt.cpu().numpy()


def _inner(buf, n):
    assert bool((buf[:GUARD] == SENT).all()) and bool((buf[GUARD + n:] == SENT).all()) and buf.size == n + 2 * GUARD, "a guard was written"
    return buf[GUARD:GUARD + n]


# ------------------------------------------------------------------ argmax
def test_argmax_of_every_row_of_the_value_table(hip):
    rows = ref.value_table()
    rng = np.random.default_rng(0)
    one = rows.T.reshape(1, 4, 27, 27, 9)                          # V = 6561: 25 full workgroups and one of 161
    three = np.stack([rows[rng.permutation(6561)].T.reshape(4, 27, 27, 9) for _ in range(3)])
    for p in (one, three):
        want = ref.argmax4(p)
        assert sorted(set(want.reshape(-1).tolist())) == [0, 1, 2, 3]
        for name, view in _forms(p).items():
            seg, dice = hip.argmax_dice(view)
            assert dice is None and seg.dtype == torch.int64 and seg.device == view.device and tuple(seg.shape) == want.shape
            got = seg.cpu().numpy()
            bad = np.argwhere(got != want)
            assert bad.size == 0, (name, len(bad), [(p[i[0], :, i[1], i[2], i[3]].tolist(), int(got[tuple(i)]), int(want[tuple(i)])) for i in bad[:5]])


def _special_probabilities(p):
    """p with classes 1 and 3 never winning (TC and ET empty), and p with class 0 always winning (every region empty)"""
    no13, only0 = p.copy(), p.copy()
    no13[:, 1], no13[:, 3] = -1.0, -1.0
    only0[:, 0] = 3.0
    return no13, only0


@pytest.mark.parametrize("v", sorted(SHAPES))
def test_every_address_form_gives_the_statements_labels_and_quotients(hip, v):
    for nb in (1, 2, 3):
        p, want, fam = _case(v, nb)
        forms = _forms(p)
        c = {k: ref.counts(want, t) for k, t in fam.items()}
        dev = {k: torch.from_numpy(t).to(DEV) for k, t in fam.items()}
        for name, view in forms.items():
            seg, dice = hip.argmax_dice(view)
            assert dice is None and np.array_equal(seg.cpu().numpy(), want), (name, nb)
            seg, dice, iou = hip.argmax_dice(view, dev["foreign"], miou=True)
            assert np.array_equal(seg.cpu().numpy(), want), (name, nb)
            assert dice.dtype == torch.float64 and iou.dtype == torch.float64 and dice.is_cuda and iou.is_cuda
            assert np.array_equal(_bits64(dice.cpu().numpy()), _bits64(ref.dice(c["foreign"][:3]))), (name, nb)
            assert np.array_equal(_bits64(iou.cpu().numpy()), _bits64(ref.iou(c["foreign"][3:]))), (name, nb)
        for k in fam:
            seg, dice = hip.argmax_dice(forms["NCDHW"], dev[k])
            seg2, dice2, iou2 = hip.argmax_dice(forms["channels-last"], dev[k], miou=True)
            assert torch.equal(seg, seg2) and np.array_equal(seg.cpu().numpy(), want)
            for d in (dice, dice2):
                assert np.array_equal(_bits64(d.cpu().numpy()), _bits64(ref.dice(c[k][:3]))), (k, nb)
            assert np.array_equal(_bits64(iou2.cpu().numpy()), _bits64(ref.iou(c[k][3:]))), (k, nb)
        assert ref.dice(c["seg"][:3]).tolist() == [1.0] * 3 and ref.iou(c["seg"][3:]).tolist() == [1.0] * 3
        no13, only0 = _special_probabilities(p)
        seg, dice, iou = hip.argmax_dice(torch.from_numpy(no13).to(DEV), dev["class 2"], miou=True)
        assert set(seg.cpu().numpy().reshape(-1).tolist()) <= {0, 2}
        assert dice[1:].tolist() == [1.0, 1.0] and iou[[0, 2]].tolist() == [1.0, 1.0]          # eps / eps: empty on both sides
        assert np.array_equal(_bits64(dice.cpu().numpy()), _bits64(ref.dice(ref.counts(ref.argmax4(no13), fam["class 2"])[:3])))
        seg, dice, iou = hip.argmax_dice(torch.from_numpy(only0).to(DEV), dev["zero"], miou=True)
        assert not bool(seg.any()) and dice.tolist() == [1.0] * 3 and iou.tolist() == [1.0] * 3


@pytest.mark.parametrize("v", sorted(SHAPES))
def test_raw_entry_points_strides_counts_accumulation_and_guards(hip, v):
    """prob[b sb + c sc + v sv] with padding between the samples (and between the channels) that holds +inf: a read outside a sample
    changes the labels; counts are exact, accumulate, and nothing is written outside seg [B V] and counts [3 or 6][3]"""
    for nb in (1, 2, 3):
        p, want, fam = _case(v, nb)
        flat = torch.from_numpy(p.reshape(nb, 4, v))
        layouts = {"NCDHW, padded samples": (4 * v + 7, v, 1), "channels-last, padded samples": (4 * v + 5, 1, 4),
                   "padded channels and samples": (4 * (v + 3) + 2, v + 3, 1)}
        dev = {k: torch.from_numpy(t).to(DEV) for k, t in fam.items()}
        for li, (name, (sb, sc, sv)) in enumerate(layouts.items()):
            lead = 5
            buf = torch.full((lead + nb * sb + 8,), INF, device=DEV)
            view = torch.as_strided(buf, (nb, 4, v), (sb, sc, sv), lead)
            assert lead + (nb - 1) * sb + 3 * sc + (v - 1) * sv < buf.numel()                  # the last element addressed
            view.copy_(flat)
            ptr = buf.data_ptr() + 4 * lead
            for entry, rows in ENTRIES.items():
                for k in (fam if li == 0 else ("random", "foreign")):
                    stated = ref.counts(want, fam[k])[:rows]
                    rc, seg, cnt = _launch(hip, entry, ptr, sb, sc, sv, dev[k], nb, v)
                    assert rc == 0
                    assert np.array_equal(_inner(seg, nb * v), want.reshape(-1)), (name, entry, k, nb)
                    assert np.array_equal(_inner(cnt, rows * 3).reshape(rows, 3), stated), (name, entry, k, nb)
                    again = _launch(hip, entry, ptr, sb, sc, sv, dev[k], nb, v, init=stated)[2]          # the += contract
                    assert np.array_equal(_inner(again, rows * 3).reshape(rows, 3), 2 * stated), (name, entry, k, nb)
            # no target: no counts buffer is needed, and one that is passed stays as it was
            rc, seg, _ = _launch(hip, "cwf_argmax_dice", ptr, sb, sc, sv, None, nb, v, counts=False)
            assert rc == 0 and np.array_equal(_inner(seg, nb * v), want.reshape(-1))
            rc, seg, cnt = _launch(hip, "cwf_argmax_dice", ptr, sb, sc, sv, None, nb, v, init=np.full(9, SENT))
            assert rc == 0 and np.array_equal(_inner(seg, nb * v), want.reshape(-1)) and bool((cnt == SENT).all())
            assert bool(torch.isinf(buf[:lead]).all()) and bool(torch.isinf(buf[lead + nb * sb:]).all())
        no13, only0 = _special_probabilities(p)
        for q, k in ((no13, "class 2"), (only0, "zero")):
            d = torch.from_numpy(q).to(DEV)
            rc, seg, cnt = _launch(hip, "cwf_argmax_metrics", d.data_ptr(), 4 * v, v, 1, dev[k], nb, v)
            stated = ref.counts(ref.argmax4(q), fam[k])
            assert rc == 0 and np.array_equal(_inner(cnt, 18).reshape(6, 3), stated)
            assert stated[1:3].tolist() == [[0, 0, 0]] * 2 and (k != "zero" or not stated.any())


# ------------------------------------------------------------------ label_metrics
def _label_metrics(hip, seg, target, n, init=None):
    cnt = torch.full((GUARD + 18 + GUARD,), SENT, dtype=torch.int64, device=DEV)
    cnt[GUARD:GUARD + 18] = 0 if init is None else torch.from_numpy(np.asarray(init, dtype=np.int64).reshape(-1)).to(DEV)
    rc = hip.lib.cwf_label_metrics(seg.data_ptr(), target.data_ptr(), cnt.data_ptr() + 8 * GUARD, n, _stream())
    torch.cuda.synchronize()
    assert rc == 0
    return _inner(cnt.cpu().numpy(), 18).reshape(6, 3)


@pytest.mark.parametrize("n", [1, 255, 257, 2048 * 256 + 257])
def test_label_metrics_counts(hip, n):
    """n = 2048 * 256 + 257: a second grid-stride round of 257 voxels, the last workgroup of it partial"""
    rng = np.random.default_rng(n)
    p = ref.tied_probabilities(rng, (1, n, 1, 1))
    want_seg = ref.argmax4(p).reshape(-1)
    fam = ref.target_families(rng, want_seg)
    if n > 2048 * 256:
        fam["tail only"] = np.where(np.arange(n) >= 2048 * 256, 3, 0).astype(np.int64)         # what only the second round reads
    d = torch.from_numpy(p).to(DEV)
    init = np.arange(18, dtype=np.int64) * 1000 + 7
    for k, t in fam.items():
        tgt = torch.from_numpy(t).to(DEV)
        rc, seg, cnt = _launch(hip, "cwf_argmax_metrics", d.data_ptr(), 4 * n, n, 1, tgt, 1, n)
        assert rc == 0 and np.array_equal(_inner(seg, n), want_seg)
        dseg = torch.from_numpy(_inner(seg, n).copy()).to(DEV)                                 # the seg that launch produced
        stated = ref.counts(want_seg, t)
        got = _label_metrics(hip, dseg, tgt, n)
        assert np.array_equal(got, stated), k
        assert np.array_equal(got, _inner(cnt, 18).reshape(6, 3)), k
        assert np.array_equal(_label_metrics(hip, dseg, tgt, n, init), stated + init.reshape(6, 3)), k
        dice, iou = hip.label_metrics(dseg, tgt)
        assert dice.dtype == torch.float64 and iou.dtype == torch.float64 and dice.is_cuda
        assert np.array_equal(_bits64(dice.cpu().numpy()), _bits64(ref.dice(stated[:3]))), k
        assert np.array_equal(_bits64(iou.cpu().numpy()), _bits64(ref.iou(stated[3:]))), k
    if n > 2048 * 256:
        assert ref.counts(want_seg, fam["tail only"])[2, 2] == 257
    both = torch.from_numpy(fam["foreign"]).to(DEV)                # foreign labels on the seg side too
    other = ref.target_families(rng, want_seg)["foreign"]
    assert np.array_equal(_label_metrics(hip, both, torch.from_numpy(other).to(DEV), n), ref.counts(fam["foreign"], other))


def test_label_metrics_wrapper_takes_any_shape_and_strides(hip):
    rng = np.random.default_rng(5)
    seg, tgt = rng.integers(0, 4, (2, 5, 6, 7)), rng.integers(0, 4, (2, 5, 6, 7))
    stated = ref.counts(seg, tgt)
    dseg = torch.from_numpy(seg.transpose(0, 3, 2, 1).copy()).to(DEV).permute(0, 3, 2, 1)      # the same values, other strides
    assert not dseg.is_contiguous()
    dice, iou = hip.label_metrics(dseg, torch.from_numpy(tgt).to(DEV))
    assert np.array_equal(_bits64(dice.cpu().numpy()), _bits64(ref.dice(stated[:3])))
    assert np.array_equal(_bits64(iou.cpu().numpy()), _bits64(ref.iou(stated[3:])))


# ------------------------------------------------------------------ region_bits
LABELS = list(range(-3, 7)) + [2 ** 32 + 1, 2 ** 32 + 3, -2 ** 63, 2 ** 63 - 1]


def _region_bits_raw(hip, labels):
    n = labels.size
    out = torch.full((GUARD + n + GUARD,), 0xEE, dtype=torch.uint8, device=DEV)
    d = torch.from_numpy(labels).to(DEV)
    rc = hip.lib.cwf_region_bits(d.data_ptr(), out.data_ptr() + GUARD, n, _stream())
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert rc == 0 and bool((got[:GUARD] == 0xEE).all()) and bool((got[GUARD + n:] == 0xEE).all())
    return got[GUARD:GUARD + n]


@pytest.mark.parametrize("n", [0, 1, 255, 256, 257])
def test_region_bits(hip, n):
    pool = np.array(LABELS, dtype=np.int64)
    if n == 0:
        for shape in ((0,), (2, 0, 3)):
            bits = hip.region_bits(torch.empty(shape, dtype=torch.int64, device=DEV))
            assert bits.dtype == torch.uint8 and bits.is_cuda and tuple(bits.shape) == shape
        return
    cases = [pool[k:k + 1] for k in range(len(pool))] if n == 1 else [np.resize(np.roll(pool, s), n) for s in (0, 5)]
    for labels in cases:
        want = ref.region_bits(labels)
        assert np.array_equal(_region_bits_raw(hip, labels), want)
        d = torch.from_numpy(labels).to(DEV)
        bits = hip.region_bits(d)
        assert bits.dtype == torch.uint8 and bits.device == d.device and tuple(bits.shape) == (n,)
        assert np.array_equal(bits.cpu().numpy(), want)
    if n == 256:                                                   # a view with strides: the wrapper makes it contiguous
        d = torch.from_numpy(np.resize(pool, 2 * n)).to(DEV)[::2]
        assert np.array_equal(hip.region_bits(d.view(16, 16)).cpu().numpy(), ref.region_bits(np.resize(pool, 2 * n)[::2]).reshape(16, 16))


# ------------------------------------------------------------------ stitch
def _random_windows(nb, seed):
    """int32 [8 nb, 128, 128, 128, 4] of random bit patterns (about one in 256 is a NaN or an infinity when read as fp32)"""
    g = torch.Generator(device=DEV).manual_seed(seed)
    return torch.randint(-2 ** 31, 2 ** 31, (8 * nb, 128, 128, 128, 4), generator=g, device=DEV, dtype=torch.int64).to(torch.int32)


def _stitch_statement(win, nb):
    """the gather ref.stitch_source describes, index tensors built on the device: int32 [nb, 240, 240, 155, 4]"""
    ar = lambda n, shape: torch.arange(n, device=DEV).view(shape)                              # noqa: E731
    b, a, bb, c = ar(nb, (nb, 1, 1, 1)), ar(240, (1, 240, 1, 1)), ar(240, (1, 1, 240, 1)), ar(155, (1, 1, 1, 155))
    wb, la, lb, lc = ref.stitch_source(b, a, bb, c, nb)
    voxel = ((wb * 128 + la) * 128 + lb) * 128 + lc
    assert tuple(voxel.shape) == (nb, 240, 240, 155) and int(voxel.min()) == 0 and int(voxel.max()) == 8 * nb * 128 ** 3 - 1 - (127 - 122)
    return win.reshape(-1, 4)[voxel]


@pytest.mark.parametrize("nb", [1, 2])
def test_stitch_is_the_gather_of_the_statement_bit_for_bit(hip, nb):
    win = _random_windows(nb, nb)
    out8 = win.view(torch.float32).permute(0, 4, 1, 2, 3)          # logical [8 nb, 4, 128, 128, 128] over channels-last memory
    assert bool(torch.isnan(out8).any()) and win.data_ptr() % 16 == 0
    y = hip.stitch_windows(out8, nb)
    assert tuple(y.shape) == (nb, 4, 240, 240, 155) and y.dtype == torch.float32 and y.is_contiguous() and y.device == win.device
    want = _stitch_statement(win, nb)
    assert torch.equal(y.view(torch.int32).permute(0, 2, 3, 4, 1), want)
    if nb == 1:                                                    # NCDHW memory: the wrapper's .contiguous() branch
        plain = out8.contiguous()
        assert not plain.permute(0, 2, 3, 4, 1).is_contiguous()
        assert torch.equal(hip.stitch_windows(plain, 1).view(torch.int32), y.view(torch.int32))


def test_tailor_and_concat_batched_equals_the_slice_assignments(hip, monkeypatch):
    nb = 2
    x = torch.randn((nb, 4, 240, 240, 155), generator=torch.Generator().manual_seed(9)).to(DEV)
    names, real, shapes = [], hip._call, []
    monkeypatch.setattr(hip, "_call", lambda name, *a: (names.append(name), real(name, *a))[1])

    def model(xb, mm):                                             # a per-sample function, its result in channels-last memory
        shapes.append(tuple(xb.shape))
        out = (xb.flip(1) * 0.5 + 1.0).permute(0, 2, 3, 4, 1).contiguous().permute(0, 4, 1, 2, 3)
        assert not out.is_contiguous()
        return (out,)

    got = po.tailor_and_concat(x, None, model, batched=True)
    assert names == ["cwf_stitch_windows"] and shapes == [(8 * nb, 4, 128, 128, 128)]
    want = po.tailor_and_concat(x, None, model, batched=False)
    assert names == ["cwf_stitch_windows"] and shapes[1:] == [(nb, 4, 128, 128, 128)] * 8
    assert tuple(got.shape) == tuple(want.shape) == (nb, 4, 240, 240, 155)
    assert torch.equal(got.view(torch.int32), want.contiguous().view(torch.int32))


# ------------------------------------------------------------------ refusals
def test_entry_points_refuse_before_any_launch(hip):
    lib, st = hip.lib, _stream()
    v, nb = 65, 2
    prob = torch.rand((nb, 4, v), device=DEV)
    tgt = torch.randint(0, 4, (nb, v), device=DEV)
    seg = torch.full((nb * v,), SENT, dtype=torch.int64, device=DEV)
    cnt = torch.full((18,), SENT, dtype=torch.int64, device=DEV)
    bits = torch.full((nb * v,), 0xEE, dtype=torch.uint8, device=DEV)

    def argmax(entry, pp=prob.data_ptr(), tp=tgt.data_ptr(), sp=seg.data_ptr(), cp=cnt.data_ptr(), b=nb, vv=v):
        return getattr(lib, entry)(pp, 4 * v, v, 1, tp, sp, cp, b, vv, st)

    shared = {"null prob": dict(pp=None), "null seg": dict(sp=None), "B = 0": dict(b=0), "B < 0": dict(b=-1), "V = 0": dict(vv=0),
              "V < 0": dict(vv=-5), "a target without counts": dict(cp=None)}
    for entry in ENTRIES:
        for name, kw in shared.items():
            assert argmax(entry, **kw) == BADARG, (entry, name)
    assert argmax("cwf_argmax_metrics", tp=None) == BADARG and argmax("cwf_argmax_metrics", tp=None, cp=None) == BADARG

    def metrics(sp=seg.data_ptr(), tp=tgt.data_ptr(), cp=cnt.data_ptr(), n=nb * v):
        return lib.cwf_label_metrics(sp, tp, cp, n, st)

    for name, kw in {"null seg": dict(sp=None), "null target": dict(tp=None), "null counts": dict(cp=None), "n = 0": dict(n=0),
                     "n < 0": dict(n=-1)}.items():
        assert metrics(**kw) == BADARG, name
    assert metrics(n=2 ** 62) == TOOLARGE                          # more rounds than the per-thread int counters hold

    def region(lp=tgt.data_ptr(), bp=bits.data_ptr(), n=nb * v):
        return lib.cwf_region_bits(lp, bp, n, st)

    for name, kw in {"null labels": dict(lp=None), "null bits": dict(bp=None), "n = 0": dict(n=0), "n < 0": dict(n=-3)}.items():
        assert region(**kw) == BADARG, name

    win = torch.zeros((8 * 128 ** 3 * 4 + 4,), device=DEV)
    y = torch.full((1, 4, 240, 240, 155), -3.0, device=DEV)
    assert win.data_ptr() % 16 == 0
    for name, (wp, yp, b) in {"null windows": (None, y.data_ptr(), 1), "null y": (win.data_ptr(), None, 1), "B = 0": (win.data_ptr(), y.data_ptr(), 0),
                              "B < 0": (win.data_ptr(), y.data_ptr(), -1), "windows off 16 bytes": (win.data_ptr() + 4, y.data_ptr(), 1),
                              "windows off 16 bytes by 8": (win.data_ptr() + 8, y.data_ptr(), 1)}.items():
        assert lib.cwf_stitch_windows(wp, yp, b, st) == BADARG, name
    torch.cuda.synchronize()
    assert bool((seg == SENT).all()) and bool((cnt == SENT).all()) and bool((bits == 0xEE).all()) and bool((y == -3.0).all())     # nothing ran
    assert argmax("cwf_argmax_dice") == 0 and lib.cwf_stitch_windows(win.data_ptr(), y.data_ptr(), 1, st) == 0
    torch.cuda.synchronize()
    assert bool((seg != SENT).all()) and bool((y == 0).all())


def test_wrappers_refuse_with_value_error_before_any_launch(hip, monkeypatch):
    calls = []
    monkeypatch.setattr(hip, "_call", lambda name, *a: calls.append(name))          # records, launches nothing
    sp = (3, 4, 5)
    prob = torch.rand((2, 4) + sp, device=DEV)
    tgt = torch.randint(0, 4, (2,) + sp, device=DEV)
    big = lambda dtype, shape, dev=DEV: torch.zeros((1,), dtype=dtype, device=dev).expand(shape)          # noqa: E731
    bad = {
        "argmax_dice": [
            ("float64 prob", (prob.double(),)), ("bf16 prob", (prob.bfloat16(),)), ("three channels", (prob[:, :3],)),
            ("five channels", (torch.rand((2, 5) + sp, device=DEV),)), ("no spatial axis", (prob[:, :, 0, 0, 0],)), ("one axis", (prob[0, 0, 0, 0],)),
            ("prob on the host", (prob.cpu(),)), ("no tensor", (prob.cpu().numpy(),)), ("empty prob", (prob[:, :, :0],)),
            ("int32 target", (prob, tgt.int())), ("float target", (prob, tgt.float())), ("target of another shape", (prob, tgt[:, :2])),
            ("target with a channel axis", (prob, tgt[:, None])), ("target on the host", (prob, tgt.cpu())), ("miou without a target", (prob, None, True))],
        "label_metrics": [
            ("int32 seg", (tgt.int(), tgt)), ("int32 target", (tgt, tgt.int())), ("float seg", (tgt.float(), tgt)), ("shapes differ", (tgt, tgt[:1])),
            ("seg on the host", (tgt.cpu(), tgt)), ("target on the host", (tgt, tgt.cpu())), ("empty", (tgt[:0], tgt[:0])), ("no tensor", (tgt, None))],
        "region_bits": [("int32 labels", (tgt.int(),)), ("uint8 labels", (tgt.to(torch.uint8),)), ("labels on the host", (tgt.cpu(),)),
                        ("no tensor", (tgt.cpu().numpy(),))],
        "stitch_windows": [
            ("float64 windows", (big(torch.float64, (8, 4, 128, 128, 128)), 1)), ("bf16 windows", (big(torch.bfloat16, (8, 4, 128, 128, 128)), 1)),
            ("three channels", (big(torch.float32, (8, 3, 128, 128, 128)), 1)), ("64^3 windows", (big(torch.float32, (8, 4, 64, 64, 64)), 1)),
            ("channels last in the shape", (big(torch.float32, (8, 128, 128, 128, 4)), 1)), ("nb does not match", (big(torch.float32, (8, 4, 128, 128, 128)), 2)),
            ("nb = 0", (torch.empty((0, 4, 128, 128, 128), device=DEV), 0)), ("windows on the host", (big(torch.float32, (8, 4, 128, 128, 128), "cpu"), 1)),
            ("no tensor", (None, 1))],
    }
    for method, cases in bad.items():
        for name, args in cases:
            with pytest.raises(ValueError, match=method):
                getattr(hip, method)(*args)
            assert calls == [], (method, name)
    # and what is accepted launches exactly once
    hip.argmax_dice(prob, tgt, miou=True)
    hip.argmax_dice(prob.permute(0, 2, 3, 4, 1).contiguous().permute(0, 4, 1, 2, 3))
    hip.argmax_dice(prob[:, :, 0], tgt[:, 0])                      # [B, 4, 4, 5]: any rank from 3 on
    hip.argmax_dice(prob[:, :, 0, 0], tgt[:, 0, 0])
    hip.label_metrics(tgt, tgt)
    hip.region_bits(tgt)
    hip.region_bits(tgt[:0])                                       # empty: nothing to launch
    assert calls == ["cwf_argmax_metrics", "cwf_argmax_dice", "cwf_argmax_dice", "cwf_argmax_dice", "cwf_label_metrics", "cwf_region_bits"]


def test_argmax_dice_on_other_ranks(hip):
    """[B, 4, N] and [B, 4, H, W]: NCDHW-like, channels-last-like and strided, all by the statement"""
    rng = np.random.default_rng(11)
    for shape in ((3, 257), (2, 9, 31)):
        p = ref.tied_probabilities(rng, (shape[0], int(np.prod(shape[1:])), 1, 1)).reshape((shape[0], 4) + shape[1:])
        want = ref.argmax4(p)
        t = torch.from_numpy(p).to(DEV)
        last = t.movedim(1, -1).contiguous().movedim(-1, 1)
        assert not last.is_contiguous() and last.movedim(1, -1).is_contiguous()
        wide = torch.full(tuple(t.shape[:-1]) + (t.shape[-1] + 2,), INF, device=DEV)
        wide[..., :-2] = t
        for view in (t, last, wide[..., :-2]):
            seg, dice = hip.argmax_dice(view)
            assert tuple(seg.shape) == want.shape and np.array_equal(seg.cpu().numpy(), want)


# ------------------------------------------------------------------ the two routes of _validate
def test_validate_on_the_device_and_on_the_host_agree(hip):
    rng = np.random.default_rng(21)
    rows = ref.value_table()[rng.choice(6561, size=2 * 5 * 6 * 7, replace=False)]
    assert int(np.isnan(rows).any(axis=1).sum()) > 50 and int((rows == rows.max(axis=1, keepdims=True)).sum(axis=1).max()) >= 2
    p = np.ascontiguousarray(rows.reshape(2, 5, 6, 7, 4).transpose(0, 4, 1, 2, 3))
    want = ref.argmax4(p)
    fam = ref.target_families(rng, want)
    fam["no class 3"] = rng.integers(0, 3, size=want.shape, dtype=np.int64)                   # an empty region on the target's side
    prob = torch.from_numpy(p).to(DEV)
    for k, t in fam.items():
        tgt = torch.from_numpy(t)
        seg, prob_out, dice, iou = po._validate(prob, tgt.to(DEV), True)
        hseg, _, hdice, hiou = po._validate(prob.cpu(), tgt, True)
        assert prob_out is prob and seg.is_cuda and not hseg.is_cuda
        assert torch.equal(seg.cpu(), hseg) and np.array_equal(hseg.numpy(), want), k
        c = ref.counts(want, t)
        assert [float(d) for d in dice] == ref.dice(c[:3]).tolist() and [float(i) for i in iou] == ref.iou(c[3:]).tolist(), k
        for a, b in zip(list(dice) + list(iou), list(hdice) + list(hiou)):
            assert abs(float(a) - float(b)) < 1e-6, k                                          # the host expression divides in float32
        seg2, _, dice2 = po._validate(prob, tgt.to(DEV), False)
        assert torch.equal(seg2, seg) and [float(d) for d in dice2] == [float(d) for d in dice]
        again = po._revalidate(seg, prob, tgt.to(DEV), True, 155)
        assert again[0] is seg and [float(d) for d in again[2]] == [float(d) for d in dice] and [float(i) for i in again[3]] == [float(i) for i in iou]
        hagain = po._revalidate(hseg, prob.cpu(), tgt, True, 155)
        assert [float(d) for d in hagain[2]] == [float(d) for d in hdice] and [float(i) for i in hagain[3]] == [float(i) for i in hiou]
        from_host = po._validate(prob, tgt, True)                                              # a target still on the host
        assert torch.equal(from_host[0], seg) and [float(d) for d in from_host[2]] == [float(d) for d in dice]
    seg, _, dice = po._validate(prob, None, False)
    assert dice is None and np.array_equal(seg.cpu().numpy(), want)
