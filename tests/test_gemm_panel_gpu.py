"""GPU: the K-panel GEMM kernels (gemm_mfma_p_kernel) against the 16-byte-load kernel they replace, bit for bit.

Every case runs the same argument struct twice from the same buffer contents and the same generator state: with
cwf_debug_gemm_panel(0) (the old kernel) and with (2) (every launch that has a panel instantiation; the launch counter must advance by
one).  Every buffer must come back bitwise equal between the two runs -- C, C2, the rowsum targets, each table entry -- and, outside the
elements the GEMM writes, equal to what it held before.  The guard bands of every buffer and the padding between operand rows hold
NaN, so any use of an element outside an operand shows in the result.  The panel result is also held to the float64 bound of
tests/test_token_path_exact_gpu.py (gamma_gemm(K) * A, imported).  Builders, buffers and the reference are that file's and
tests/token_ref.py's.

The shapes are the smallest at which the panel code can go wrong: one full tile plus a sliver for the 32- and the 64-row form (the
64 x 64 form needs >= 256 workgroups: N = 1028 and ZB * ZH = 8, or M = 198 with ZB = 4), a single clamped row, and K of one panel,
exactly D panels, D + 1 panels (the first refill) and the production extents 512 / 516 (a tail panel with 4 live k) / 1024 / 258.
PK = 64 and D = 4 at the 32 x 32 tile (csrc/gemm.hip: GP_PK, GP_D32)."""
import ctypes

import pytest
import torch

import test_token_path_exact_gpu as T
import token_ref as R

pytestmark = pytest.mark.gpu
T_, F_ = True, False
PK, D32 = 64, 4
NAN = float("nan")
TILE64 = {"edge-TF64-m70-n1028", "edge-FT64-m68-n1028", "old-TT64-k512", "prod-qkv-region", "prod-wgrad-qkv"}

# name, M, N, K, ZB, ZH, AK, BN, features, overrides of struct fields, takes the panel route
CASES = []


def _case(name, M, N, K, ZB, ZH, AK, BN, feat, over=None, panel=True):
    CASES.append((name, M, N, K, ZB, ZH, AK, BN, set(feat), over or {}, panel))


# ---- tile edges
_case("edge-TF32-m33-n36", 33, 36, 512, 1, 1, T_, F_, {"bias"})
_case("edge-TF32-m70-n68", 70, 68, 512, 1, 1, T_, F_, {})
_case("edge-TF32-m1", 1, 68, 512, 1, 1, T_, F_, {"bias"})
_case("edge-TF64-m70-n1028", 70, 1028, 512, 4, 2, T_, F_, {"bias"})
_case("edge-TT32-m33-n36", 33, 36, 1024, 1, 1, T_, T_, {})
_case("edge-TT32-m1", 1, 36, 512, 1, 1, T_, T_, {})
_case("edge-FT32-m36-n68", 36, 68, 516, 1, 1, F_, T_, {"rowsum"})
_case("edge-FT64-m68-n1028", 68, 1028, 516, 4, 2, F_, T_, {"a_drop"})
# ---- panel schedule per layout: one panel, D panels, D + 1 panels, the production extents; extents without an instantiation
for lay, AK, BN, M in (("TF", T_, F_, 33), ("TT", T_, T_, 33), ("FT", F_, T_, 36)):
    for K in (PK, D32 * PK, (D32 + 1) * PK):
        _case("sched-%s-k%d" % (lay, K), M, 36, K, 1, 1, AK, BN, {"rowsum"})
_case("sched-TF-k512", 33, 36, 512, 1, 1, T_, F_, {"rowsum"})
_case("sched-TT-k512", 33, 36, 512, 1, 1, T_, T_, {"rowsum"})
_case("sched-TT-k1024", 33, 36, 1024, 1, 1, T_, T_, {"rowsum"})
_case("sched-FT-k516", 36, 36, 516, 1, 1, F_, T_, {"rowsum"})
_case("sched-FT-k258", 36, 36, 258, 1, 1, F_, T_, {"rowsum"})
_case("old-TF-k2048", 33, 36, 2048, 1, 1, T_, F_, {"rowsum"}, panel=False)
_case("old-TT-k60", 33, 36, 60, 1, 1, T_, T_, {"rowsum"}, panel=False)
_case("old-TF-k1024", 33, 36, 1024, 1, 1, T_, F_, {}, panel=False)
_case("old-FF-k516", 36, 36, 516, 1, 1, F_, F_, {}, panel=False)
_case("old-TT64-k512", 198, 1028, 512, 4, 1, T_, T_, {}, panel=False)
# ---- operand forms
_case("view0-TT", 33, 36, 512, 3, 1, T_, T_, {"B_tab", "a_drop", "view0"})
_case("view512-TT", 33, 36, 1024, 3, 1, T_, T_, {"B_tab", "view512"})
_case("A2-split64", 33, 132, 512, 1, 1, T_, F_, {"A2"}, {"split_n": 64})
_case("B2-split64", 68, 36, 516, 1, 1, F_, T_, {"B2", "rowsum"}, {"split_m": 64})
# ---- batch strides and tables
_case("tabs-TF-zb3", 33, 36, 512, 3, 1, T_, F_, {"B_tab", "bias_tab", "C_tab", "rowsum_tab"})
_case("tabs-FT-zb3", 36, 36, 516, 3, 1, F_, T_, {"B_tab", "bias_tab", "C_tab", "rowsum_tab"})
_case("strided-zb2-zh2", 33, 36, 512, 2, 2, T_, F_, {"bias", "residual"})
# ---- fused features alone
_case("f-a_drop", 33, 36, 512, 1, 1, T_, F_, {"a_drop", "rowsum"})
_case("f-a_drop-p2", 33, 36, 512, 1, 1, T_, T_, {"a_drop", "rowsum"}, {"a_drop_p2": 0.2})
_case("f-a_drop-FT", 36, 36, 516, 1, 1, F_, T_, {"a_drop", "rowsum"}, {"a_drop_p2": 0.2})
_case("f-c_drop", 33, 36, 512, 1, 1, T_, F_, {"c_drop"})
_case("f-act-C2", 33, 36, 512, 1, 1, T_, F_, {"act", "C2"})
_case("f-residual", 33, 36, 512, 1, 1, T_, F_, {"residual"})
_case("f-accumulate-rowsum_acc", 36, 36, 516, 1, 1, F_, T_, {"accumulate", "rowsum", "rowsum_acc"})
_case("f-alpha", 33, 36, 512, 1, 1, T_, F_, {"alpha"})
_case("f-bias", 33, 36, 1024, 1, 1, T_, T_, {"bias"})
# ---- the production feature combinations of GEMM_CASES, on small extents (both tiles for the two 64 x 64 launches)
_case("prod-qkv-region", 198, 1028, 512, 4, 1, T_, F_, {"A2", "B_tab"})
_case("prod-outproj-ffn", 33, 36, 512, 3, 1, T_, F_, {"bias_tab", "c_drop", "residual", "act", "C2"})
_case("prod-ffn-drop2", 33, 36, 512, 1, 1, T_, F_, {"bias", "c_drop2", "residual", "C2", "alpha"})
_case("prod-fusion-258", 33, 36, 512, 1, 1, T_, F_, {"bias", "act", "C2"})
_case("prod-wgrad-qkv", 196, 1028, 516, 4, 1, F_, T_, {"C_tab", "rowsum_tab", "B2", "accumulate", "rowsum_acc", "a_drop"}, {"split_m": 128})
_case("prod-wgrad-qkv-32", 68, 36, 516, 3, 1, F_, T_, {"C_tab", "rowsum_tab", "B2", "accumulate", "rowsum_acc", "a_drop"}, {"split_m": 64})
_case("prod-wgrad-512", 36, 36, 516, 3, 1, F_, T_, {"C_tab", "rowsum_tab", "a_drop"})
_case("prod-wgrad-single", 68, 36, 516, 1, 1, F_, T_, {"rowsum", "accumulate", "rowsum_acc", "B2", "a_drop"}, {"split_m": 64})
_case("prod-FT-k258", 36, 36, 258, 1, 1, F_, T_, {"rowsum", "a_drop", "C2", "act"})


def _bits(t):
    return t.view(torch.int32)


def _same(x, y):
    """bitwise equality (NaN guard bands compare equal to themselves)"""
    return torch.equal(_bits(x), _bits(y))


def _live(g):
    """{id(buffer): bool mask of the elements the GEMM may read (inputs) or write (outputs)}"""
    M, N, K, ZB, ZH = g["M"], g["N"], g["K"], g["ZB"], g["ZH"]
    live = {}

    def mark(pair, zoff, sizes, strides):
        buf, off = pair
        m = live.setdefault(id(buf), torch.zeros(buf.numel(), dtype=torch.bool, device=buf.device))
        m[R._view(buf, off + zoff, sizes, strides).reshape(-1)] = True

    for z in range(ZB * ZH):
        zb, zh = z // ZH, z % ZH
        for key in ("A", "A2"):
            if g.get(key) is not None:
                mark(g[key], zb * g["sa_zb"] + zh * g["sa_zh"], (M, K), (g["sa_m"], g["sa_k"]))
        bz = zb * g["sb_zb"] + zh * g["sb_zh"]
        if g.get("B_tab"):
            mark(g["B_tab"][z], 0, (K, N), (g["sb_k"], g["sb_n"]))
        else:
            mark(g["B"], bz, (K, N), (g["sb_k"], g["sb_n"]))
        if g.get("B2") is not None:
            mark(g["B2"], bz, (K, N), (g["sb_k"], g["sb_n"]))
        cz = zb * g["sc_zb"] + zh * g["sc_zh"]
        if g.get("C_tab"):
            mark(g["C_tab"][z], 0, (M, N), (g["sc_m"], 1))
        else:
            mark(g["C"], cz, (M, N), (g["sc_m"], 1))
        if g.get("C2") is not None:
            mark(g["C2"], cz, (M, N), (g["sc_m"], 1))
        if g.get("bias_tab"):
            mark(g["bias_tab"][z], 0, (N,), (1,))
        elif g.get("bias") is not None:
            mark(g["bias"], 0, (N,), (1,))
        if g.get("residual") is not None:
            mark(g["residual"], zb * g["sr_zb"] + zh * g["sr_zh"], (M, N), (g["sr_m"], 1))
        if g.get("rowsum_tab"):
            mark(g["rowsum_tab"][z], 0, (M,), (1,))
        elif g.get("rowsum") is not None:
            mark(g["rowsum"], 0, (M,), (1,))
    return live


def _prepare(hip, case):
    """(args struct, reference dict, buffers, live masks): T._build's case with the overrides applied and NaN everywhere else"""
    name, M, N, K, ZB, ZH, AK, BN, feat, over, panel = case
    a, g, bufs = T._build(hip, (name, M, N, K, ZB, ZH, AK, BN, feat, None), "random", seed=7 * CASES.index(case))
    for k, v in over.items():
        setattr(a, k, v)
        g[k] = v
    live = _live(g)
    for b in bufs.values():
        b[~live[id(b)]] = NAN
    return a, g, bufs, live


def _launch(hip, a, route):
    """one cwf_gemm_ex launch with the route forced; returns how many launches took the panel kernel"""
    count = hip.lib.cwf_debug_gemm_panel_launches
    old = hip.lib.cwf_debug_gemm_panel(route)
    try:
        n0 = count()
        hip._call("cwf_gemm_ex", ctypes.addressof(a), hip._stream())
        torch.cuda.synchronize()
        return count() - n0
    finally:
        hip.lib.cwf_debug_gemm_panel(old)


def test_switch_returns_the_previous_value(hip):
    old = hip.lib.cwf_debug_gemm_panel(2)
    try:
        assert hip.lib.cwf_debug_gemm_panel(0) == 2
        assert hip.lib.cwf_debug_gemm_panel(1) == 0
    finally:
        hip.lib.cwf_debug_gemm_panel(old)


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_panel_equals_vector_kernel(hip, case):
    name, M, N, K, ZB, ZH, AK, BN, feat, over, panel = case
    a, g, bufs, live = _prepare(hip, case)
    rc, variant = T._variant(hip, a)
    assert rc == 0
    if panel:
        assert variant[0] == 1 and variant[2:] == (int(AK), int(BN)), (name, variant)
    assert variant[1] == (64 if name in TILE64 else 32), (name, variant)
    before = {k: v.clone() for k, v in bufs.items()}
    E = T._emul(hip)
    ref = R.gemm_ex(g, E)
    assert _launch(hip, a, 0) == 0, (name, "route 0 took the panel kernel")
    old = {k: v.clone() for k, v in bufs.items()}
    for k, v in bufs.items():
        v.copy_(before[k])
    assert _launch(hip, a, 2) == (1 if panel else 0), (name, "panel route taken / not taken")
    outputs = {next(k for k, b in bufs.items() if id(b) == key) for key in list(ref["C"]) + list(ref["rowsum"])}
    if ref["C2"] is not None:
        outputs.add("C2")
    for k, v in bufs.items():
        assert _same(v, old[k]), (name, k, "differs from the 16-byte-load kernel's result")
        if k in outputs:
            m = ~live[id(v)]
            assert _same(v[m], before[k][m]), (name, k, "guard band / untouched elements changed")
        else:
            assert _same(v, before[k]), (name, k, "an input buffer changed")
    gam = R.gamma_gemm(K)
    for key, (v, A, wr) in list(ref["C"].items()) + list(ref["rowsum"].items()):
        bname = next(k for k, b in bufs.items() if id(b) == key)
        assert torch.equal(wr, live[key]), (name, bname, "the test's written mask and the reference's disagree")
        assert R.worst(bufs[bname][wr], v[wr], gam * A[wr], "%s %s" % (name, bname)) <= 1.0
    if ref["C2"] is not None:
        v, A, wr = ref["C2"]
        assert R.worst(bufs["C2"][wr], v[wr], gam * A[wr], "%s C2" % name) <= 1.0


def test_panel_determinism(hip):
    """fixed summation order, plain stores: a second panel launch is bitwise equal to the first"""
    case = next(c for c in CASES if c[0] == "prod-FT-k258")
    outs = []
    for _ in range(2):
        a, g, bufs, _ = _prepare(hip, case)
        assert _launch(hip, a, 2) == 1
        outs.append({k: v.clone() for k, v in bufs.items()})
    assert all(_same(outs[0][k], outs[1][k]) for k in outs[0])
