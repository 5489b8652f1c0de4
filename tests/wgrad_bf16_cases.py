"""The case table of the bf16-form weight-gradient kernels (csrc/wgrad_bf16.hip), shared by tests/test_wgrad_bf16_plan_cpu.py (the
library's host code alone) and tests/test_wgrad_bf16_exact_gpu.py (a helper module, not a test file).

A case is a launch -- (op, cin -> cout, forward input extent, batch, the form of x and dy) -- with the precision modes it runs in and
the kernel instance each mode must reach (enum cwf_wgrad_bf16_instance, include/cwf_hip.h).  cwf_debug_wgrad_bf16_plan answers
which instance a descriptor reaches with the host code cwf_wgrad itself runs; the table pins that answer, so a changed condition in
the dispatcher shows as a failing case instead of a fast kernel that silently stopped being tested.

Forms of x / dy (`memory` below lays them out; the CPU file fills in aligned dummy addresses, the GPU file real tensors):
  contig   x [n, D, H, W, cin] contiguous; dy in rows of ca = cout rounded up to 4 floats
  slice    x channels [8, 8 + cin) of a buffer cin + 12 wide, dy channels [4, 4 + cout) of one ca + 8 wide: 16-byte aligned starts
  dy4      dy channels [1, 1 + cout) of a buffer ca + 4 wide: a start that is 4-byte but not 16-byte aligned
  images   x and dy as bf16 images (xa16 / dy16), single-bf16 only
  dys      contig with dy_scale [n, cout]
  g2 / g3  2 / 3 same-shape layers in one launch: x_g[q] / dy_g[q] channel groups of shared buffers, a slab buffer each
  g2dy4    g2 whose dy groups start 4 bytes into their rows (the grouped launch's route to the generic kernel)
Shapes: the smallest that reach the instance and the edge.  The 16 -> 16 persistent kernels need >= 32768 output voxels by rule;
everything else gets its tile counts from channel counts and from thin extents (a 4 x 4 x 16 tile that holds few voxels is still a
tile), because the float64 reference costs voxels x taps x cin x cout."""
import collections
import ctypes
import os
import re

S1, S2, C1, CT = 0, 1, 2, 3                                # CWF_CONV3_S1, CWF_CONV3_S2, CWF_CONV1, CWF_CONVT2
HDR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "cwf_hip.h")
E_BADARG, E_TOOLARGE, E_ALIGN = -1, -2, -3
WALK_RANGES, WALK_STRIDED, WALK_PW = 0, 1, 2


def _header_enum():
    """{short name: id} of enum cwf_wgrad_bf16_instance, read from the header (COUNT included)"""
    hdr = re.sub(r"/\*.*?\*/", " ", open(HDR).read(), flags=re.S)
    body = re.search(r"enum\s+cwf_wgrad_bf16_instance\s*\{([^}]*)\}", hdr).group(1)
    ids, nxt = {}, 0
    for item in body.split(","):
        item = item.strip()
        if not item:
            continue
        m = re.fullmatch(r"CWF_WGB_(\w+?)(?:\s*=\s*(\d+))?", item)
        assert m, item
        nxt = int(m.group(2)) if m.group(2) else nxt
        ids[m.group(1)] = nxt
        nxt += 1
    return ids


IDS = _header_enum()
COUNT = IDS["COUNT"]
NAME_OF = {v: k for k, v in IDS.items() if k != "COUNT"}
PLAN_FIELDS = int(re.search(r"#define\s+CWF_WGB_PLAN_FIELDS\s+(\d+)", open(HDR).read()).group(1))

Case = collections.namedtuple("Case", "name op cin cout size n form inst")      # inst: {precision mode: instance short name}
Plan = collections.namedtuple("Plan", "inst gx gy gz threads walk step wps waves items slab used exact lo hi")
assert len(Plan._fields) == PLAN_FIELDS


def _c(name, op, cin, cout, size, n, form, **inst):
    return Case(name, op, cin, cout, size, n, form, inst)


B, X = "bf16", "bf16x3"
CASES = [
    # ---- wgrad16_kernel<X3>: Cin 4 / 8 / 12 / 16; grid 256 (Cin <= 4) and 160; cut to the tile count; ragged tiles in all three axes
    _c("w16_cin4_dys", S1, 4, 16, (32, 33, 34), 2, "dys", bf16="WGRAD16", bf16x3="WGRAD16_X3"),        # 432 tiles on 256: 1 and 2 each
    _c("w16_cin4_cut", S1, 4, 16, (32, 32, 32), 1, "contig", bf16="WGRAD16"),                          # 128 tiles: grid 256 -> 128
    _c("w16_cin8_ragged", S1, 8, 16, (31, 33, 35), 1, "slice", bf16="WGRAD16"),                        # 216 tiles on 160, ragged d, h, w
    _c("w16_cin12_cut", S1, 12, 16, (32, 32, 32), 1, "contig", bf16x3="WGRAD16_X3"),                   # grid 160 -> 128
    _c("w16_cin16", S1, 16, 16, (32, 33, 34), 2, "contig", bf16="WGRAD16", bf16x3="WGRAD16_X3"),       # 432 tiles on 160: 2 and 3 each
    # ---- wgrad16d_kernel (bf16 images): the same edges
    _c("w16d", S1, 16, 16, (32, 33, 34), 2, "images", bf16="WGRAD16D"),
    _c("w16d_cut", S1, 16, 16, (32, 32, 32), 1, "images", bf16="WGRAD16D"),
    _c("w16d_ragged", S1, 16, 16, (31, 33, 35), 1, "images", bf16="WGRAD16D"),
    # ---- pw_wgrad_kernel, 1x1x1: exact fp32 products in both modes.  tiny = one 4-voxel group per sample (15 of 16 waves idle)
    _c("pw111_tiny", C1, 16, 16, (1, 2, 2), 3, "contig", bf16="PW_1_1_1", bf16x3="PW_1_1_1"),
    _c("pw111_ragged", C1, 8, 12, (3, 4, 7), 3, "slice", bf16="PW_1_1_1", bf16x3="PW_1_1_1"),            # 21 groups on 16 waves: 2, .., 2, 1, 0..
    _c("pw211_two_wgs", C1, 32, 16, (8, 9, 10), 3, "contig", bf16="PW_2_1_1", bf16x3="PW_2_1_1"),       # 180 groups: two workgroups per sample
    _c("pw211_dy4", C1, 20, 4, (5, 4, 9), 3, "dy4", bf16="PW_2_1_1"),                                  # (dword loads: dy need not be 16-byte aligned)
    _c("pw421", C1, 64, 32, (4, 5, 7), 3, "contig", bf16="PW_4_2_1", bf16x3="PW_4_2_1"),
    _c("pw421_ragged_ch", C1, 52, 20, (8, 9, 10), 2, "slice", bf16="PW_4_2_1"),
    _c("pw841", C1, 128, 64, (3, 4, 11), 3, "contig", bf16="PW_8_4_1", bf16x3="PW_8_4_1"),
    _c("pw841_two_wgs", C1, 116, 52, (8, 9, 10), 2, "contig", bf16x3="PW_8_4_1"),                      # 8-wave workgroups: three per sample
    # ---- pw_wgrad_kernel, ConvTranspose (W % 4 == 0)
    _c("pw118", CT, 16, 16, (3, 5, 4), 3, "contig", bf16="PW_1_1_8", bf16x3="PW_1_1_8"),
    _c("pw118_tiny", CT, 8, 4, (1, 1, 4), 3, "slice", bf16="PW_1_1_8"),
    _c("pw228", CT, 32, 32, (2, 3, 8), 3, "contig", bf16="PW_2_2_8", bf16x3="PW_2_2_8"),
    _c("pw228_two_wgs", CT, 20, 24, (5, 6, 12), 2, "contig", bf16="PW_2_2_8"),                         # 90 groups on 8 waves: two workgroups
    # ---- the generic 1-tap kernel: pointwise layers that fail the stream kernel's conditions
    _c("t21_conv1_odd", C1, 16, 16, (3, 5, 7), 2, "contig", bf16="TILED_2_1", bf16x3="TILED_2_1_X3"),   # 105 voxels: not a multiple of 4
    _c("t21_convT_w6", CT, 16, 12, (4, 3, 6), 2, "contig", bf16="TILED_2_1", bf16x3="TILED_2_1_X3"),    # ConvTranspose with W % 4 != 0
    _c("t22_conv1_32_32", C1, 32, 32, (4, 5, 17), 2, "slice", bf16="TILED_2_2", bf16x3="TILED_2_2_X3"),  # (2 chunks, 2 tiles): not in the table
    _c("t22_convT_w5", CT, 32, 32, (3, 4, 5), 2, "contig", bf16="TILED_2_2", bf16x3="TILED_2_2_X3"),
    _c("t24_conv1_16_64", C1, 16, 64, (4, 4, 18), 2, "contig", bf16="TILED_2_4", bf16x3="TILED_2_4_X3"),
    _c("t24_convT_20_48", CT, 20, 48, (3, 5, 7), 2, "contig", bf16="TILED_2_4", bf16x3="TILED_2_4_X3"),
    # ---- the generic 27-tap kernel: split mode; stride 2 (odd input extents); single-bf16 stride 1 behind a misaligned dy or Cout % 4 != 0
    _c("t71_s1_x3", S1, 48, 16, (9, 10, 20), 2, "slice", bf16x3="TILED_7_1_X3"),
    _c("t71_s1_dy4", S1, 20, 12, (6, 8, 19), 2, "dy4", bf16="TILED_7_1", bf16x3="TILED_7_1_X3"),
    _c("t71_s1_cout2", S1, 8, 2, (6, 7, 15), 2, "contig", bf16="TILED_7_1"),                            # a 2-channel gradient in 4-float rows
    _c("t71_s2_odd", S2, 16, 16, (9, 7, 33), 2, "contig", bf16="TILED_7_1", bf16x3="TILED_7_1_X3"),
    _c("t72_s1_x3", S1, 32, 48, (6, 8, 20), 2, "contig", bf16x3="TILED_7_2_X3"),
    _c("t72_s1_dy4", S1, 32, 32, (5, 6, 17), 2, "dy4", bf16="TILED_7_2"),
    _c("t72_s2_odd", S2, 16, 32, (11, 13, 35), 2, "slice", bf16="TILED_7_2", bf16x3="TILED_7_2_X3"),
    _c("t72_s1_ranges2", S1, 256, 32, (1, 9, 170), 1, "contig", bf16x3="TILED_7_2_X3"),               # 33 tiles, 16 blocks: ranges of 2, last 1
    # ---- walks as long as the model's layers have them (five or more tiles per workgroup; thin extents keep the voxel count down)
    _c("w16_cin4_long", S1, 4, 16, (1, 2, 16400), 2, "dys", bf16="WGRAD16"),                            # 2050 tiles on 256
    _c("w16_cin16_long", S1, 16, 16, (2, 3, 5470), 2, "contig", bf16="WGRAD16", bf16x3="WGRAD16_X3"),   # 684 tiles on 160: 4 and 5 each
    _c("w16d_long", S1, 16, 16, (2, 3, 5470), 2, "images", bf16="WGRAD16D"),
    _c("pw111_long", C1, 16, 4, (8, 9, 10), 2, "contig", bf16="PW_1_1_1", bf16x3="PW_1_1_1"),           # 6 groups per wave, two workgroups
    _c("pw118_long", CT, 16, 16, (5, 6, 12), 2, "contig", bf16="PW_1_1_8"),
    _c("t24_conv1_ranges2", C1, 16, 64, (1, 1, 8200), 1, "contig", bf16="TILED_2_4", bf16x3="TILED_2_4_X3"),   # 513 tiles: ranges of 2
    _c("t24_conv1_ranges4", C1, 256, 128, (1, 2, 960), 1, "contig", bf16="TILED_2_4", bf16x3="TILED_2_4_X3"),  # 60 tiles, 32 blocks: ranges of 4
    _c("t72_s2_ranges4", S2, 64, 128, (1, 3, 1599), 2, "contig", bf16="TILED_7_2"),                    # 100 tiles, 16 blocks: ranges of 4
    _c("t72_s2_ranges5", S2, 64, 128, (1, 3, 2079), 2, "contig", bf16="TILED_7_2"),                    # 130 tiles: ranges of 5
    # ---- grouped launches
    _c("g2_cout8", S1, 32, 8, (8, 12, 16), 2, "g2", bf16="S1_1", bf16x3="TILED_7_1_X3"),
    _c("g3_cout32", S1, 16, 32, (5, 6, 17), 2, "g3", bf16="S1_2", bf16x3="TILED_7_2_X3"),
    _c("g2_dy4", S1, 16, 8, (5, 6, 17), 2, "g2dy4", bf16="TILED_7_1"),
    # ---- wgrad_s1_kernel<1> (Cout <= 16): 128 input channels = 8 (chunk, group) blocks -> 20 ranges: 1, 2, 3, 4, 5 tiles each;
    #      50 tiles in ranges of 3 leave a last range of 2, and 25 tiles per sample put range 8 = tiles [24, 27) across the samples
    _c("s1_1_r1", S1, 128, 16, (2, 5, 33), 2, "contig", bf16="S1_1"),                                  # 12 tiles
    _c("s1_1_r2", S1, 128, 16, (2, 9, 65), 2, "slice", bf16="S1_1"),                                   # 30 tiles
    _c("s1_1_r3", S1, 128, 8, (5, 5, 65), 3, "contig", bf16="S1_1"),                                   # 60 tiles
    _c("s1_1_r4", S1, 128, 16, (1, 17, 113), 2, "contig", bf16="S1_1"),                                # 80 tiles
    _c("s1_1_r5", S1, 128, 12, (1, 17, 150), 2, "contig", bf16="S1_1"),                                # 100 tiles
    _c("s1_1_short_cross", S1, 128, 16, (17, 17, 3), 2, "contig", bf16="S1_1"),                        # 50 tiles
    # ---- wgrad_s1_kernel<2> (Cout > 16) and wgrad_s1d_kernel (the same layers as bf16 images): 128 -> 64 = 16 blocks -> 10 ranges;
    #      28 tiles in ranges of 3 leave a last range of 1, and 14 tiles per sample put range 4 = tiles [12, 15) across the samples
    _c("s1_2_r1", S1, 128, 64, (2, 5, 33), 1, "contig", bf16="S1_2"),                                  # 6 tiles
    _c("s1_2_r2", S1, 128, 64, (2, 5, 33), 2, "contig", bf16="S1_2"),                                  # 12 tiles
    _c("s1_2_r3", S1, 128, 64, (5, 9, 17), 2, "slice", bf16="S1_2"),                                   # 24 tiles
    _c("s1_2_r4", S1, 128, 64, (5, 17, 17), 2, "contig", bf16="S1_2"),                                 # 40 tiles
    _c("s1_2_r5", S1, 128, 64, (2, 17, 33), 3, "contig", bf16="S1_2"),                                 # 45 tiles
    _c("s1_2_short_cross", S1, 128, 64, (2, 5, 100), 2, "contig", bf16="S1_2"),                        # 28 tiles
    _c("s1_2_cin20_cout48", S1, 20, 48, (6, 8, 20), 2, "contig", bf16="S1_2"),                         # a ragged chunk and a ragged group
    _c("s1d_r1", S1, 128, 64, (2, 5, 33), 1, "images", bf16="S1D"),
    _c("s1d_r2", S1, 128, 64, (2, 5, 33), 2, "images", bf16="S1D"),
    _c("s1d_r3", S1, 128, 64, (5, 9, 17), 2, "images", bf16="S1D"),
    _c("s1d_r4", S1, 128, 64, (5, 17, 17), 2, "images", bf16="S1D"),
    _c("s1d_r5", S1, 128, 64, (2, 17, 33), 3, "images", bf16="S1D"),
    _c("s1d_short_cross", S1, 128, 64, (2, 5, 100), 2, "images", bf16="S1D"),
    _c("s1d_32_32", S1, 32, 32, (8, 12, 20), 2, "images", bf16="S1D"),
]
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
RUNS = [(c.name, mode) for c in CASES for mode in (B, X) if mode in c.inst]      # (case, precision mode) pairs that exist

# the ring kernels' edges: {instance: {tiles per range: case}}, a case whose last range is shorter, a case whose ranges cross samples
RING = {
    "S1_1": ({1: "s1_1_r1", 2: "s1_1_r2", 3: "s1_1_r3", 4: "s1_1_r4", 5: "s1_1_r5"}, "s1_1_short_cross"),
    "S1_2": ({1: "s1_2_r1", 2: "s1_2_r2", 3: "s1_2_r3", 4: "s1_2_r4", 5: "s1_2_r5"}, "s1_2_short_cross"),
    "S1D": ({1: "s1d_r1", 2: "s1d_r2", 3: "s1d_r3", 4: "s1d_r4", 5: "s1d_r5"}, "s1d_short_cross"),
}


def out_dims(op, d, h, w):
    if op == S2:
        return ((d - 1) // 2 + 1, (h - 1) // 2 + 1, (w - 1) // 2 + 1)
    if op == CT:
        return (2 * d, 2 * h, 2 * w)
    return (d, h, w)


def groups_of(form):
    return {"g2": 2, "g3": 3, "g2dy4": 2}.get(form, 0)


Memory = collections.namedtuple("Memory", "x_width x_off x_ldc dy_width dy_off dy_ldc x_goff dy_goff")


def memory(case):
    """the buffers behind a case's x and dy views, in floats: buffer width (channels per voxel row), first channel of the view (of
    group 0), row pitch, and for grouped launches the channel distance between groups"""
    cin, cout, G = case.cin, case.cout, groups_of(case.form)
    ca = (cout + 3) // 4 * 4
    if case.form == "slice":
        return Memory(cin + 12, 8, cin + 12, ca + 8, 4, ca + 8, 0, 0)
    if case.form == "dy4":
        return Memory(cin, 0, cin, ca + 4, 1, ca + 4, 0, 0)
    if G:
        off = 1 if case.form == "g2dy4" else 0
        return Memory(G * cin, 0, G * cin, G * ca + 4 * off, off, G * ca + 4 * off, cin, ca)
    return Memory(cin, 0, cin, ca, 0, ca, 0, 0)


def descriptor(_lib, case, mode, x, dy, part, scale=0, shift=0, slope=1.0, dy_scale=0, xa16=0, dy16=0, zero16=0):
    """struct cwf_wgrad_args of a case from the ADDRESSES of its buffers (x, dy: the buffers `memory` describes; part: the slab buffer,
    or one per group).  images: xa16 / dy16 / zero16 as well.  The CPU file passes aligned dummies: the plan query dereferences nothing."""
    m = memory(case)
    do, ho, wo = out_dims(case.op, *case.size)
    a = _lib.WgradArgs(op=case.op, precision=_lib.PRECISION[mode], x_ldc=m.x_ldc, in_scale=scale, in_shift=shift, in_slope=slope,
                       dy_ldc=m.dy_ldc, dy_scale=dy_scale, xa16=xa16, dy16=dy16, zero16=zero16, N=case.n, Di=case.size[0], Hi=case.size[1],
                       Wi=case.size[2], Cin=case.cin, Do=do, Ho=ho, Wo=wo, Cout=case.cout)
    G = groups_of(case.form)
    if G:
        a.groups = G
        for q in range(G):
            a.x_g[q], a.dy_g[q], a.partial_g[q] = x + 4 * (m.x_off + q * m.x_goff), dy + 4 * (m.dy_off + q * m.dy_goff), part[q]
    else:
        a.x, a.dy, a.partial = x + 4 * m.x_off, dy + 4 * m.dy_off, part
    return a


DUMMY = dict(x=0x10000000, dy=0x20000000, scale=0x30000000, shift=0x30001000, dy_scale=0x30002000, xa16=0x40000000, dy16=0x50000000,
             zero16=0x60000000)
DUMMY_PART = [0x70000000, 0x78000000, 0x7c000000]


def dummy_descriptor(_lib, case, mode, **over):
    """the descriptor of a case on host-side dummy addresses of the alignment the GPU file's tensors have (256-byte aligned buffers)"""
    kw = dict(x=DUMMY["x"], dy=DUMMY["dy"], part=DUMMY_PART if groups_of(case.form) else DUMMY_PART[0])
    if case.form == "images":
        kw.update(xa16=DUMMY["xa16"], dy16=DUMMY["dy16"], zero16=DUMMY["zero16"])
    elif not groups_of(case.form):
        kw.update(scale=DUMMY["scale"], shift=DUMMY["shift"], slope=0.01)
    if case.form == "dys":
        kw.update(dy_scale=DUMMY["dy_scale"])
    kw.update(over)
    return descriptor(_lib, case, mode, **kw)


def query(lib, args):
    """(status, Plan or None) of cwf_debug_wgrad_bf16_plan"""
    out = (ctypes.c_int64 * PLAN_FIELDS)(*([-7] * PLAN_FIELDS))
    rc = lib.cwf_debug_wgrad_bf16_plan(ctypes.addressof(args), out)
    return rc, (Plan(*[int(v) for v in out]) if rc == 0 else None)


def operand_form(_lib, lib, op, cin, cout, size, n, mode, form="contig"):
    """the operand form ("fp32": exact products, else `mode`) of the kernel cwf_wgrad runs for such a layer in a bf16 mode, as the
    library says it (contiguous, aligned operands unless `form` says otherwise) -- what bf16_operand_ref.wgrad_operand_mode mirrors"""
    rc, p = query(lib, dummy_descriptor(_lib, Case("-", op, cin, cout, tuple(size), n, form, {}), mode))
    assert rc == 0, rc
    return "fp32" if p.exact else mode


def instance_name(lib, inst):
    s = lib.cwf_debug_wgrad_bf16_name(inst)
    return None if s is None else s.decode()


def workgroup_items(p):
    """the work items (tiles; WALK_PW: 4-voxel groups of one sample) of every workgroup of one (grid y, grid z) plane, as the header
    states the walks -- for WALK_PW the workgroups of one sample"""
    if p.walk == WALK_RANGES:
        return [list(range(s * p.step, min(p.items, (s + 1) * p.step))) for s in range(p.gx)]
    if p.walk == WALK_STRIDED:
        G = p.gx
        assert G == p.step and G % 8 == 0
        return [list(range((b & 7) * (G // 8) + (b >> 3), p.items, G)) for b in range(G)]
    assert p.walk == WALK_PW
    return [[g for v in range(p.waves) for g in range((w * p.waves + v) * p.step, min(p.items, (w * p.waves + v + 1) * p.step))]
            for w in range(p.wps)]


def tiles_class(p):
    """1, 2, 3, 4 or 5 (= five or more): the most tiles one workgroup walks (WALK_PW: the 4-voxel groups one wave walks)"""
    return min(p.step if p.walk == WALK_PW else p.hi, 5)
