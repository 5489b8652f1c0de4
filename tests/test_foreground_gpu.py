"""The class location tables on the GPU (csrc/locations.hip and its way up through cwf.kernels and utils.data): counts and table
bit-equal to tests/foreground_ref.py on every label family, tile edge, pointer alignment and table length; the buffers fully written;
the error codes, returned before any launch; and DeviceBraTS with oversampling in both device modes against the host."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import foreground_ref as ref
from cwf import _lib
from utils import data
from utils import synthetic as syn

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
T = _lib.LOCATIONS_TILE
# fewer voxels than one lane's 16-byte runs times the lanes, with a tail; two synthetic volumes; exactly one tile, one voxel less, one
# more (a second tile of one voxel), and three tiles plus five voxels
SHAPES = ((5, 3, 7), (24, 20, 17), (40, 36, 31), (1, 1, T), (1, 1, T - 1), (1, 1, T + 1), (1, 1, 3 * T + 5))
COMBOS = ((ref.FOREGROUND_CLASSES, 4096), (ref.OVERLAPPING, 64), ((0b1000,), 1), (ref.EIGHT, 64))
BADARG, ALIGN = -1, -3


@functools.lru_cache(maxsize=None)
def _families(shape):
    fam = dict(ref.label_families(shape, T))
    if len([s for s in shape if s > 1]) == 3 and min(shape) >= 17:
        lab = syn.synthetic_volume(0, shape)[1].numpy().astype(np.uint8)
        assert all(int((lab == c).sum()) > 0 for c in (1, 2, 3))                # all three classes are present
        fam["synthetic"] = lab
    for a in fam.values():
        a.setflags(write=False)
    return fam


@functools.lru_cache(maxsize=None)
def _want(shape, name, masks, K):
    """the restatement's (counts, table) of one case, computed once and left unchanged"""
    counts, table = ref.class_locations(_families(shape)[name], masks, K)
    counts.setflags(write=False)
    table.setflags(write=False)
    return counts, table


def _equal(got, want):
    counts, table = got
    return (counts.dtype == torch.int64 and table.dtype == torch.int32 and tuple(table.shape) == want[1].shape
            and np.array_equal(counts.cpu().numpy(), want[0]) and np.array_equal(table.cpu().numpy(), want[1]))


@pytest.mark.parametrize("shape", SHAPES)
def test_tables_are_bit_equal_to_the_restatement(hip, shape):
    V = int(np.prod(shape))
    families = _families(shape)
    assert ("single_tile_end" in families) == (V >= T) and ("single_tile_start" in families) == (V > T)
    for name, lab in families.items():
        dlab = torch.from_numpy(lab.copy()).to(DEV)
        for masks, K in COMBOS:
            assert _equal(hip.class_locations(dlab, masks, K), _want(shape, name, masks, K)), (name, masks, K)
    lab = families["foreign"]
    assert all((lab == v).any() for v in (4, 5, 255)) or V < 200
    # the same label with n <= K and with n > K
    for name, masks in (("one_class", ref.FOREGROUND_CLASSES), ("mixed", ref.EIGHT)):
        dlab = torch.from_numpy(families[name].copy()).to(DEV)
        below = above = 0
        for K in (1, 64, 4096, 65536):
            want = _want(shape, name, masks, K)
            assert _equal(hip.class_locations(dlab, masks, K), want), (name, K)
            below += int(((want[0] > 0) & (want[0] <= K)).sum())
            above += int((want[0] > K).sum())
        assert below > 0 and above > 0
    # through utils.data, with the defaults
    got = data.class_locations(torch.from_numpy(families["mixed"].copy()).to(DEV))
    assert got[0].is_cuda and _equal(got, _want(shape, "mixed", ref.FOREGROUND_CLASSES, 4096))


def test_one_full_size_subject(hip):
    shape = (240, 240, 155)
    lab = ref.ellipsoid_label(shape, 3)
    assert all((lab == v).any() for v in (1, 2, 4)) and not (lab == 3).any()    # the enhancing core is stored as label 4
    dlab = torch.from_numpy(lab).to(DEV)
    seen = set()
    for masks, K in ((ref.FOREGROUND_CLASSES, 4096), (ref.OVERLAPPING, 65536), (ref.EIGHT, 1)):
        want = ref.class_locations(lab, masks, K)
        assert _equal(hip.class_locations(dlab, masks, K), want), (masks, K)
        seen.update("below" if 0 < n <= K else "above" for n in want[0].tolist() if n)
    assert seen == {"below", "above"}


@pytest.mark.parametrize("offset", [3, 17])
def test_label_pointers_of_any_alignment(hip, offset):
    for shape in ((5, 3, 7), (1, 1, T + 1), (1, 1, 3 * T + 5)):
        V = int(np.prod(shape))
        for name, lab in _families(shape).items():
            buf = torch.full((V + 64,), 1, dtype=torch.uint8, device=DEV)       # class 1 on both sides: reading them would show
            view = buf[offset:offset + V]
            view.copy_(torch.from_numpy(lab.reshape(-1).copy()))
            assert view.data_ptr() % 16 == offset % 16
            for masks, K in ((ref.FOREGROUND_CLASSES, 4096), (ref.OVERLAPPING, 64)):
                assert _equal(hip.class_locations(view, masks, K), _want(shape, name, masks, K)), (shape, name, K)


def _raw_call(hip, dlab, masks, K, fill=0xFF):
    """cwf_class_locations on buffers pre-filled with `fill` bytes (guard words behind counts and table): their bytes afterwards"""
    R, V = len(masks), int(dlab.numel())
    cm = (ctypes.c_uint32 * R)(*masks)
    nbytes = hip.lib.cwf_class_locations_workspace(V, R)
    assert nbytes > 0 and nbytes % 256 == 0
    ws = torch.full((nbytes,), fill, dtype=torch.uint8, device=DEV)
    counts = torch.full((8 * R + 64,), fill, dtype=torch.uint8, device=DEV)
    table = torch.full((4 * R * K + 64,), fill, dtype=torch.uint8, device=DEV)
    rc = hip.lib.cwf_class_locations(dlab.data_ptr(), V, ctypes.addressof(cm), R, K, counts.data_ptr(), table.data_ptr(), ws.data_ptr(),
                                     torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc, counts.cpu().numpy(), table.cpu().numpy()


@pytest.mark.parametrize("shape", [(5, 3, 7), (1, 1, 3 * T + 5)])
def test_buffers_are_fully_written_and_calls_repeat(hip, shape):
    for name in ("background", "mixed", "one_class"):
        dlab = torch.from_numpy(_families(shape)[name].copy()).to(DEV)
        for masks, K in ((ref.FOREGROUND_CLASSES, 4096), (ref.EIGHT, 64)):
            want = _want(shape, name, masks, K)
            first = _raw_call(hip, dlab, masks, K)
            again = _raw_call(hip, dlab, masks, K, fill=0x00)
            R = len(masks)
            for rc, counts, table in (first, again):
                assert rc == 0
                assert np.array_equal(counts[:8 * R].view(np.int64), want[0])
                assert np.array_equal(table[:4 * R * K].view(np.int32).reshape(R, K), want[1])
            assert bool((first[1][8 * R:] == 0xFF).all()) and bool((first[2][4 * R * K:] == 0xFF).all())      # and nothing behind them
            assert first[1][:8 * R].tobytes() == again[1][:8 * R].tobytes() and first[2][:4 * R * K].tobytes() == again[2][:4 * R * K].tobytes()


def test_error_codes_come_before_any_launch(hip):
    lib = hip.lib
    V, R, K = 105, 3, 16
    assert lib.cwf_class_locations_workspace(V, R) == 256
    for v, r in ((0, 3), (-5, 3), (2 ** 31, 3), (V, 0), (V, 9), (V, -1)):
        assert lib.cwf_class_locations_workspace(v, r) == BADARG, (v, r)
    assert lib.cwf_class_locations_workspace(2 ** 31 - 1, 8) > 0
    dlab = torch.from_numpy(_families((5, 3, 7))["mixed"].copy()).to(DEV)
    ws = torch.full((512,), 0xFF, dtype=torch.uint8, device=DEV)
    counts = torch.full((8,), -1, dtype=torch.int64, device=DEV)
    table = torch.full((8, K), -7, dtype=torch.int32, device=DEV)
    assert ws.data_ptr() % 256 == 0
    good = (ctypes.c_uint32 * 8)(2, 4, 8, 1, 2, 4, 8, 1)
    high = (ctypes.c_uint32 * 8)(2, 4, 0b10000, 1, 2, 4, 8, 1)
    st = torch.cuda.current_stream().cuda_stream

    def call(label=dlab.data_ptr(), v=V, masks=good, r=R, k=K, c=counts.data_ptr(), t=table.data_ptr(), w=ws.data_ptr()):
        return lib.cwf_class_locations(label, v, ctypes.addressof(masks) if masks is not None else None, r, k, c, t, w, st)

    cases = {"null label": dict(label=None), "null posmasks": dict(masks=None), "null counts": dict(c=None), "null table": dict(t=None),
             "null ws": dict(w=None), "V = 0": dict(v=0), "V < 0": dict(v=-1), "V = 2^31": dict(v=2 ** 31), "R = 0": dict(r=0),
             "R = 9": dict(r=9), "K = 0": dict(k=0), "K = 65537": dict(k=65537), "bits above class 3": dict(masks=high)}
    for name, kw in cases.items():
        assert call(**kw) == BADARG, name
    assert call(masks=high, r=2) == 0                                           # the high mask lies past R: not looked at
    torch.cuda.synchronize()
    table.fill_(-7)
    counts.fill_(-1)
    assert call(w=ws.data_ptr() + 64) == ALIGN
    torch.cuda.synchronize()
    assert bool((counts == -1).all()) and bool((table == -7).all()) and bool((ws[256:] == 0xFF).all())   # nothing ran
    assert call() == 0
    torch.cuda.synchronize()
    assert np.array_equal(counts[:R].cpu().numpy(), _want((5, 3, 7), "mixed", ref.FOREGROUND_CLASSES, K)[0])
    with pytest.raises(ValueError):
        hip.class_locations(dlab.to(torch.int64), ref.FOREGROUND_CLASSES, K)
    with pytest.raises(ValueError):
        hip.class_locations(dlab.cpu(), ref.FOREGROUND_CLASSES, K)
    with pytest.raises(_lib.CwfError):
        hip.class_locations(dlab, (0b10000,), K)
    with pytest.raises(_lib.CwfError):
        hip.class_locations(dlab, ref.FOREGROUND_CLASSES, 65537)


def test_out_rows_and_graph_capture(hip):
    """out= fills one subject's rows of a bigger pair; the call records into a graph (no synchronisation, nothing read back) and a
    replay follows the label's current content"""
    shape, K = (1, 1, T + 1), 64
    fam = _families(shape)
    counts = torch.full((3, 3), -1, dtype=torch.int64, device=DEV)
    table = torch.full((3, 3, K), -7, dtype=torch.int32, device=DEV)
    dlab = torch.from_numpy(fam["mixed"].copy()).to(DEV)
    hip.class_locations(dlab, ref.FOREGROUND_CLASSES, K, out=(counts[1], table[1]))
    assert _equal((counts[1], table[1]), _want(shape, "mixed", ref.FOREGROUND_CLASSES, K))
    assert bool((counts[[0, 2]] == -1).all()) and bool((table[[0, 2]] == -7).all())
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        hip.class_locations(dlab, ref.FOREGROUND_CLASSES, K, out=(counts[1], table[1]))
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        hip.class_locations(dlab, ref.FOREGROUND_CLASSES, K, out=(counts[1], table[1]))
    for name in ("runs16", "mixed"):
        dlab.copy_(torch.from_numpy(fam[name].copy()))
        counts.fill_(-1)
        table.fill_(-7)
        g.replay()
        torch.cuda.synchronize()
        assert _equal((counts[1], table[1]), _want(shape, name, ref.FOREGROUND_CLASSES, K)), name


@functools.lru_cache(maxsize=None)
def _subjects():
    out = []
    for i in range(3):
        x, t = syn.synthetic_volume(i, (40, 36, 31), 4321)
        out.append((x, t.to(torch.uint8)))
    return out


@pytest.mark.parametrize("oversample", [0.33, 1.0])
def test_device_modes_agree_with_the_host(hip, oversample):
    crop, order = (16, 20, 24), [[2, 0, 1]]
    host = data.DeviceBraTS(_subjects(), "cpu", crop, seed=5, oversample=oversample)
    cached = data.DeviceBraTS(_subjects(), DEV, crop, seed=5, cache=True, oversample=oversample)
    staged = data.DeviceBraTS(_subjects(), DEV, crop, seed=5, cache=False, oversample=oversample)
    plain = data.DeviceBraTS(_subjects(), "cpu", crop, seed=5)
    for i, (x, t) in enumerate(_subjects()):
        want = ref.class_locations(t.numpy(), ref.FOREGROUND_CLASSES, 4096)
        for ds in (host, cached, staged):
            assert np.array_equal(ds.foreground[i][0], want[0]) and np.array_equal(ds.foreground[i][1], want[1])
    moved = 0
    for epoch in (0, 1, 2):
        for ds in (host, cached, staged, plain):
            ds.set_epoch(epoch)
        moved += sum(host.params(i).origin != plain.params(i).origin for i in range(3))
        want = next(iter(host.batches(order)))[:3]
        for ds in (cached, staged):
            got = next(iter(ds.batches(order)))[:3]
            for a, b in zip(got, want):
                assert a.is_cuda and a.dtype == b.dtype and torch.equal(a.cpu(), b), (epoch, ds.cache)
    assert moved >= (8 if oversample == 1.0 else 1)
