"""cwf_debug_wgrad_bf16_plan (host code of libcwf_hip.so, no GPU needed): the plan cwf_wgrad makes for a bf16-form descriptor, made by
the same function the launch runs.  Every case of tests/wgrad_bf16_cases.py must reach the kernel instance the table names, write
no more slabs than the workspace was sized for, use the slab size Python allocates by, and split its tiles into non-empty ranges
that cover every tile exactly once; the table must reach every instance and every ring-kernel edge; refused descriptors carry the
codes cwf_wgrad's conditions give.  The GPU side of the same table: tests/test_wgrad_bf16_exact_gpu.py."""
import ctypes
import re

import pytest

import bf16_operand_ref as R
import wgrad_bf16_cases as T
from cwf import _lib, packing as pk


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def _plan(lib, name, mode, **over):
    rc, p = T.query(lib, T.dummy_descriptor(_lib, T.BY_NAME[name], mode, **over))
    assert rc == 0, (name, mode, rc)
    return p


def _status(lib, name, mode, edit=None, **over):
    a = T.dummy_descriptor(_lib, T.BY_NAME[name], mode, **over)
    if edit:
        edit(a)
    return T.query(lib, a)[0]


def test_header_binding_and_names_agree(lib):
    hdr = re.sub(r"/\*.*?\*/", " ", open(T.HDR).read(), flags=re.S)
    m = re.search(r"\bint\s+cwf_debug_wgrad_bf16_plan\s*\(([^)]*)\)\s*;", hdr)
    assert m and [p.strip() for p in m.group(1).split(",")] == ["const struct cwf_wgrad_args* args", "int64_t* out"]
    assert re.search(r"\bconst\s+char\s*\*\s*cwf_debug_wgrad_bf16_name\s*\(\s*int\s+instance\s*\)\s*;", hdr)
    assert _lib.SIGNATURES["cwf_debug_wgrad_bf16_plan"] == [ctypes.c_void_p] * 2
    assert sorted(T.NAME_OF) == list(range(T.COUNT)) and T.COUNT == 22
    names = [T.instance_name(lib, i) for i in range(T.COUNT)]
    assert all(names) and len(set(names)) == T.COUNT, names
    assert T.instance_name(lib, T.COUNT) is None and T.instance_name(lib, -1) is None
    out = (ctypes.c_int64 * T.PLAN_FIELDS)()
    assert lib.cwf_debug_wgrad_bf16_plan(None, out) == T.E_BADARG
    assert lib.cwf_debug_wgrad_bf16_plan(ctypes.addressof(T.dummy_descriptor(_lib, T.CASES[0], "bf16")), None) == T.E_BADARG


@pytest.mark.parametrize("name,mode", T.RUNS, ids=["%s-%s" % r for r in T.RUNS])
def test_case_plan(lib, name, mode):
    c = T.BY_NAME[name]
    p = _plan(lib, name, mode)
    assert T.NAME_OF[p.inst] == c.inst[mode], (T.NAME_OF[p.inst], c.inst[mode])
    do, ho, wo = T.out_dims(c.op, *c.size)
    nsplit = lib.cwf_wgrad_nsplit(c.op, c.n, do, ho, wo, c.cin, c.cout)
    assert 1 <= p.used <= nsplit, (p.used, nsplit)
    np_inv, has_bias, slab = pk.wgrad_inverse_map(c.op, c.cin, c.cout)
    assert p.slab == lib.cwf_wgrad_slab_floats(c.op, c.cin, c.cout) == np_inv.size == slab
    # every workgroup has work, and together they take every item exactly once
    items = T.workgroup_items(p)
    assert all(items), [len(i) for i in items]
    assert sorted(v for i in items for v in i) == list(range(p.items))
    assert (min(map(len, items)), max(map(len, items))) == (p.lo, p.hi)
    per_plane = {T.WALK_RANGES: p.gx, T.WALK_STRIDED: p.gx, T.WALK_PW: p.wps}[p.walk]
    assert len(items) == per_plane
    tiles_sp = -(-do // (2 if c.op == T.S2 else 4)) * -(-ho // (2 if c.op == T.S2 else 4)) * -(-wo // 16)
    if p.walk == T.WALK_PW:
        assert p.gx == p.wps * c.n and p.used == p.gx and p.items * 4 == c.size[0] * c.size[1] * c.size[2] and p.waves * 64 == p.threads
    elif c.op == T.CT:
        assert p.items == c.n * -(-c.size[0] // 4) * -(-c.size[1] // 4) * -(-c.size[2] // 16) and p.gz == 8
    else:
        assert p.items == c.n * tiles_sp
    if p.walk != T.WALK_PW and T.NAME_OF[p.inst].startswith("TILED_2"):
        assert p.used == 4 * p.gx                         # the 1-tap kernel: a slab per wave
    elif p.walk != T.WALK_PW:
        assert p.used == p.gx
    G = T.groups_of(c.form)
    if G:
        assert p.gz == G
    # the Python mirror the CPU reference tests use says what the library says
    assert ("fp32" if p.exact else mode) == R.wgrad_operand_mode(c.op, c.cin, c.cout, c.size, mode)
    assert bool(p.exact) == (p.walk == T.WALK_PW)


def test_table_reaches_every_instance(lib):
    seen = {_plan(lib, name, mode).inst for name, mode in T.RUNS}
    assert seen == set(range(T.COUNT)), sorted(T.NAME_OF[i] for i in set(range(T.COUNT)) - seen)
    # each instance in every precision mode it exists in: the pointwise stream kernel in both, a split instance in bf16x3 only
    by_mode = {(T.NAME_OF[_plan(lib, name, mode).inst], mode) for name, mode in T.RUNS}
    for inst in T.NAME_OF.values():
        if inst.startswith("PW_"):
            assert (inst, "bf16") in by_mode and (inst, "bf16x3") in by_mode, inst
        else:
            assert (inst, "bf16x3" if inst.endswith("_X3") else "bf16") in by_mode, inst
    forms = {T.BY_NAME[name].form for name, _ in T.RUNS}
    assert forms == {"contig", "slice", "dy4", "images", "dys", "g2", "g3", "g2dy4"}


@pytest.mark.parametrize("inst", list(T.RING))
def test_ring_kernel_ranges(lib, inst):
    """ranges of exactly 1, 2, 3, 4 and >= 5 tiles; a last range shorter than the rest; a range that crosses from one sample to the next"""
    by_len, short_cross = T.RING[inst]
    for k, name in by_len.items():
        c = T.BY_NAME[name]
        p = _plan(lib, name, "bf16")
        assert T.NAME_OF[p.inst] == inst
        assert (p.lo, p.hi) == (k, k) and p.walk == T.WALK_RANGES, (name, p)
    c = T.BY_NAME[short_cross]
    p = _plan(lib, short_cross, "bf16")
    assert T.NAME_OF[p.inst] == inst and 0 < p.lo < p.hi, p
    items = T.workgroup_items(p)
    assert len(items[-1]) == p.lo and all(len(i) == p.hi for i in items[:-1])
    per_sample = p.items // c.n
    assert c.n >= 2 and per_sample % p.step != 0
    assert any(i[0] // per_sample != i[-1] // per_sample for i in items), "no range crosses a sample boundary"


def test_full_resolution_kernel_grids(lib):
    """wgrad16_kernel: 256 workgroups for Cin <= 4, else 160, cut in steps of 8 while above the tile count; wgrad16d_kernel: 160"""
    grid = lambda name, mode="bf16": (_plan(lib, name, mode).gx, _plan(lib, name, mode).items)
    assert grid("w16_cin4_dys") == (256, 432) and grid("w16_cin4_dys", "bf16x3") == (256, 432)
    assert grid("w16_cin4_cut") == (128, 128)
    assert grid("w16_cin8_ragged") == (160, 216)
    assert grid("w16_cin12_cut", "bf16x3") == (128, 128)
    assert grid("w16_cin16") == (160, 432)
    assert grid("w16d") == (160, 432) and grid("w16d_cut") == (128, 128) and grid("w16d_ragged") == (160, 216)
    assert {T.BY_NAME[n].cin for n in T.BY_NAME if n.startswith("w16_")} == {4, 8, 12, 16}
    for name in ("w16_cin8_ragged", "w16d_ragged"):
        d, h, w = T.BY_NAME[name].size
        assert d % 4 and h % 4 and w % 16 and d * h * w >= 32768


def test_pointwise_stream_kernel_walks(lib):
    """all six instances; a sample of one 4-voxel group (all waves but one idle); ragged runs; more than one workgroup per sample; n = 3"""
    seen = {}
    for name, mode in T.RUNS:
        p = _plan(lib, name, mode)
        if p.walk == T.WALK_PW:
            seen.setdefault(T.NAME_OF[p.inst], []).append((T.BY_NAME[name], p))
    assert sorted(seen) == ["PW_1_1_1", "PW_1_1_8", "PW_2_1_1", "PW_2_2_8", "PW_4_2_1", "PW_8_4_1"]
    for inst, runs in seen.items():
        assert any(c.n == 3 for c, _ in runs), inst
        assert any(p.items % (p.step * p.waves) for _, p in runs), (inst, "no ragged run of groups")
    assert any(p.items == 1 for _, p in seen["PW_1_1_1"]) and any(p.items == 1 for _, p in seen["PW_1_1_8"])
    for inst in ("PW_2_1_1", "PW_4_2_1", "PW_8_4_1", "PW_2_2_8"):
        assert any(p.wps > 1 for _, p in seen[inst]), inst
    assert {p.waves for _, p in seen["PW_8_4_1"]} == {8} and {p.waves for _, p in seen["PW_1_1_1"]} == {16}


def test_alignment_and_argument_errors(lib):
    base = "t71_s1_x3"
    assert _status(lib, base, "bf16x3") == 0
    assert _status(lib, base, "bf16x3", x=T.DUMMY["x"] + 4) == T.E_ALIGN
    assert _status(lib, base, "bf16x3", part=T.DUMMY_PART[0] + 4) == T.E_ALIGN
    assert _status(lib, base, "bf16x3", edit=lambda a: setattr(a, "x_ldc", a.x_ldc + 2)) == T.E_ALIGN
    assert _status(lib, base, "bf16x3", edit=lambda a: setattr(a, "Cin", 46)) == T.E_ALIGN
    for field in ("x", "dy", "partial"):
        assert _status(lib, base, "bf16x3", edit=lambda a: setattr(a, field, None)) == T.E_BADARG
    assert _status(lib, base, "bf16x3", shift=0) == T.E_BADARG                       # a scale without a shift
    assert _status(lib, base, "bf16x3", edit=lambda a: setattr(a, "op", 4)) == T.E_BADARG
    assert _status(lib, base, "bf16x3", edit=lambda a: setattr(a, "Do", a.Do + 1)) == T.E_BADARG
    assert _status(lib, base, "bf16x3", edit=lambda a: setattr(a, "precision", 3)) == T.E_BADARG
    assert _status(lib, base, "bf16x3", edit=lambda a: setattr(a, "precision", 0)) == T.E_BADARG      # (fp32: cwf_debug_wgrad_fp32_plan's)
    assert _status(lib, base, "bf16x3", edit=lambda a: setattr(a, "N", 0)) == T.E_BADARG


def test_dy_scale_outside_its_layer_class(lib):
    """dy_scale is implemented by wgrad16_kernel alone: Cin <= 16 -> 16 channels, >= 32768 voxels, aligned dy, no groups, no images"""
    s = T.DUMMY["dy_scale"]
    for mode in ("bf16", "bf16x3"):
        assert _status(lib, "w16_cin4_dys", mode) == 0
        assert _status(lib, "w16_cin16", mode, dy_scale=s) == 0
        assert _status(lib, "w16_cin16", mode, dy_scale=s, dy=T.DUMMY["dy"] + 4) == T.E_BADARG       # the generic kernel would drop it
        assert _status(lib, "w16_cin16", mode, dy_scale=s, edit=lambda a: setattr(a, "dy_ldc", 18)) == T.E_BADARG
    assert _status(lib, "s1_1_r1", "bf16", dy_scale=s) == T.E_BADARG                  # 128 input channels
    assert _status(lib, "t71_s1_x3", "bf16x3", dy_scale=s) == T.E_BADARG              # below 32768 voxels
    assert _status(lib, "t72_s1_x3", "bf16x3", dy_scale=s) == T.E_BADARG              # 48 output channels
    assert _status(lib, "pw111_ragged", "bf16", dy_scale=s) == T.E_BADARG
    assert _status(lib, "g2_cout8", "bf16", dy_scale=s) == T.E_BADARG
    assert _status(lib, "w16d", "bf16", dy_scale=s) == T.E_BADARG


def test_image_and_group_refusals(lib):
    assert _status(lib, "w16d", "bf16") == 0 and _status(lib, "s1d_32_32", "bf16") == 0
    for name in ("w16d", "s1d_32_32"):
        assert _status(lib, name, "bf16x3") == T.E_BADARG                            # the image kernels are single-bf16 only
        assert _status(lib, name, "bf16", xa16=0) == T.E_BADARG and _status(lib, name, "bf16", dy16=0) == T.E_BADARG
        assert _status(lib, name, "bf16", zero16=0) == T.E_BADARG
        assert _status(lib, name, "bf16", edit=lambda a: setattr(a, "groups", 2)) == T.E_BADARG
        assert _status(lib, name, "bf16", edit=lambda a: setattr(a, "op", T.S2)) == T.E_BADARG
        assert _status(lib, name, "bf16", xa16=T.DUMMY["xa16"] + 8) == T.E_ALIGN
        assert _status(lib, name, "bf16", part=T.DUMMY_PART[0] + 8) == T.E_ALIGN
    assert _status(lib, "s1d_32_32", "bf16", edit=lambda a: setattr(a, "Cout", 48)) == T.E_BADARG     # Cout no multiple of 32
    assert _status(lib, "s1d_32_32", "bf16", edit=lambda a: setattr(a, "Cin", 24)) == T.E_BADARG      # Cin no multiple of 16
    for mode in ("bf16", "bf16x3"):
        assert _status(lib, "g2_cout8", mode) == 0
        assert _status(lib, "g2_cout8", mode, edit=lambda a: setattr(a, "groups", 1)) == T.E_BADARG
        assert _status(lib, "g2_cout8", mode, edit=lambda a: setattr(a, "groups", 4)) == T.E_BADARG
        assert _status(lib, "g2_cout8", mode, scale=T.DUMMY["scale"], shift=T.DUMMY["shift"]) == T.E_BADARG      # no prologue
        assert _status(lib, "g2_cout8", mode, edit=lambda a: setattr(a, "op", T.S2)) == T.E_BADARG
        assert _status(lib, "g2_cout8", mode, x=T.DUMMY["x"] + 4) == T.E_ALIGN
        assert _status(lib, "g2_cout8", mode, part=[T.DUMMY_PART[0], 0]) == T.E_ALIGN
    assert _status(lib, "g2_cout8", "bf16", edit=lambda a: setattr(a, "precision", 0)) == T.E_BADARG


@pytest.mark.parametrize("name,mode,generic", [
    ("s1_1_r3", "bf16", "TILED_7_1"), ("s1_2_r3", "bf16", "TILED_7_2"), ("w16_cin16", "bf16", "TILED_7_1"), ("w16_cin16", "bf16x3", "TILED_7_1_X3"),
    ("g2_cout8", "bf16", "TILED_7_1"), ("g3_cout32", "bf16", "TILED_7_2"), ("t71_s1_x3", "bf16x3", "TILED_7_1_X3")])
def test_dy_moved_by_four_bytes_takes_the_generic_kernel(lib, name, mode, generic):
    """the fast kernels read dy in 16-byte pieces; the same descriptor with dy 4 bytes on is no error: the generic kernel takes it,
    with the generic split plan (one slab per range of the 512-workgroup plan)"""
    c = T.BY_NAME[name]
    p0 = _plan(lib, name, mode)
    p1 = _plan(lib, name, mode, dy=T.DUMMY["dy"] + 4)
    assert T.NAME_OF[p0.inst] == c.inst[mode] and T.NAME_OF[p1.inst] == generic
    do, ho, wo = T.out_dims(c.op, *c.size)
    assert p1.used == p1.gx == lib.cwf_wgrad_nsplit(c.op, c.n, do, ho, wo, c.cin, c.cout)
    assert p1.slab == p0.slab and p1.items == p0.items and p1.threads == 256
    # a pointwise layer reads dy by dwords: the stream kernel keeps it
    q = _plan(lib, "pw211_two_wgs", mode, dy=T.DUMMY["dy"] + 4)
    assert T.NAME_OF[q.inst] == "PW_2_1_1"


def test_slab_workspace_too_small_for_a_slab_per_sample_falls_through(lib):
    """launch_pw_wgrad's refusal: with more samples than the workspace has slabs (4 x the generic splits) the stream kernel cannot give
    every sample a workgroup, and the layer falls through to the generic 1-tap kernel -- not an error"""
    c = T.BY_NAME["pw111_tiny"]                           # one tile per sample; the generic plan wants at most 512 ranges
    a = T.dummy_descriptor(_lib, c, "bf16")
    a.N = 2049                                           # ranges of 5 tiles: 410 ranges x 4 waves = 1640 slabs < 2049 samples
    rc, p = T.query(lib, a)
    assert rc == 0 and T.NAME_OF[p.inst] == "TILED_2_1" and (p.gx, p.step, p.used) == (410, 5, 1640), p
    assert p.used == lib.cwf_wgrad_nsplit(c.op, a.N, 1, 2, 2, c.cin, c.cout)
    a.N = 2048                                           # ranges of 4: 512 x 4 = 2048 slabs, one per sample
    rc, p = T.query(lib, a)
    assert rc == 0 and T.NAME_OF[p.inst] == "PW_1_1_1" and p.gx == 2048 and p.wps == 1, p
