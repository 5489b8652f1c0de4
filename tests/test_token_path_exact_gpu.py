"""GPU: the couplers' token path -- cwf_gemm_ex on all ten kernel instantiations, one-launch attention, paired LayerNorm, GELU
backward with dropout and the round-2 token kernels -- against the float64 reference of tests/token_ref.py, elementwise:
|got - ref| <= gamma * A, or bit for bit where the kernel rounds once per step in a fixed order.  Every output lands in a wider
buffer whose other elements must come back untouched.  Dropout masks are matched exactly (the counter generator, synced with
the device state).  Run with -s to see the worst err/bound of every path next to its gamma.

Which test covers what: the GEMM variant table (cwf_debug_gemm_variant, every case asserts the kernel it reaches) --
test_gemm_variant_reach and test_gemm_case[*]; production shapes -- test_gemm_case[qkv-region / outproj-ffn / wgrad-* /
dgrad-*-view / fusion-258]; K tails 258 / 516 and K < 64 -- test_gemm_case[FT-k258 / wgrad-* / s32-*]; refusals --
test_gemm_refusals, test_attention_refusal, test_layernorm_refusals, test_topk_refusal; fixed-order claims --
test_determinism."""
import ctypes
import math

import pytest
import torch

import token_ref as R
from oracle.kernel_emul import EmulBackend

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BADARG, TOOLARGE = -1, -2
_WORST = {}


def _record(path, r, gamma):
    """keep the worst err/bound per path; printed at the end of the module (with -s)"""
    w, g = _WORST.get(path, (0.0, gamma))
    _WORST[path] = (max(w, r), max(g, gamma))


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    print("\n  worst err/bound per path (err/bound = |got - ref| / (gamma A); <= 1 passes), largest gamma the path used")
    for path in sorted(_WORST):
        w, g = _WORST[path]
        print("    %-34s err/bound %.3f   gamma = %5.1f u = 2^%.1f" % (path, w, g / R.U, math.log2(g)))


def _worst(path, got, ref, bound, gamma):
    r = R.worst(got, ref, bound, path)
    _record(path, r, gamma)
    return r


def _u(*shape, seed, s=1.0):
    g = torch.Generator().manual_seed(seed)
    return ((torch.rand(*shape, generator=g) * 2 - 1) * s).float().to(DEV)


def _emul(hip):
    E = EmulBackend()
    seed, step = hip.rng(DEV).cpu().tolist()
    E.set_rng(seed, step)
    return E


def _sync():
    torch.cuda.synchronize()


# ====================================================================================================== GEMM
T_, F_ = True, False
# name, M, N, K, ZB, ZH, AK, BN, features, expected variant (vector, TM, AK, BN)
GEMM_CASES = [
    ("qkv-region", 516, 1536, 512, 3, 1, T_, F_, {"A2", "B_tab"}, (1, 64, 1, 0)),
    ("outproj-ffn", 516, 512, 512, 3, 1, T_, F_, {"bias_tab", "c_drop", "residual", "act", "C2"}, (1, 32, 1, 0)),
    ("ffn-drop2", 516, 512, 512, 1, 1, T_, F_, {"bias", "c_drop2", "residual", "C2", "alpha"}, (1, 32, 1, 0)),
    ("fusion-258", 258, 512, 512, 1, 1, T_, F_, {"bias", "act", "C2"}, (1, 32, 1, 0)),
    ("TF-tabs-zb4", 33, 129, 512, 4, 1, T_, F_, {"B_tab", "bias_tab", "C_tab"}, (1, 32, 1, 0)),
    ("TF-zb2-zh2", 129, 256, 512, 2, 2, T_, F_, {"bias", "A2", "residual"}, (1, 32, 1, 0)),
    ("wgrad-qkv", 1536, 512, 516, 3, 1, F_, T_, {"C_tab", "rowsum_tab", "B2", "accumulate", "rowsum_acc", "a_drop"}, (1, 64, 0, 1)),
    ("wgrad-512", 512, 512, 516, 3, 1, F_, T_, {"C_tab", "rowsum_tab", "a_drop"}, (1, 32, 0, 1)),
    ("wgrad-single", 512, 512, 516, 1, 1, F_, T_, {"rowsum", "accumulate", "rowsum_acc", "B2", "a_drop"}, (1, 32, 0, 1)),
    ("FT-k258", 516, 516, 258, 1, 1, F_, T_, {"rowsum", "a_drop", "C2", "act"}, (1, 32, 0, 1)),
    ("dgrad-dq-view", 516, 512, 512, 3, 1, T_, T_, {"B_tab", "a_drop", "view0"}, (1, 32, 1, 1)),
    ("dgrad-dkv-view", 516, 512, 1024, 3, 1, T_, T_, {"B_tab", "view512"}, (1, 32, 1, 1)),
    ("TT-64", 1548, 512, 512, 2, 1, T_, T_, {"residual", "accumulate", "alpha", "bias"}, (1, 64, 1, 1)),
    ("FF-32", 516, 33, 516, 1, 1, F_, F_, {"bias", "act", "C2", "c_drop", "rowsum"}, (1, 32, 0, 0)),
    ("FF-64", 1548, 1548, 64, 1, 1, F_, F_, {"rowsum", "residual", "a_drop"}, (1, 64, 0, 0)),
    ("s32-k4", 1, 33, 4, 1, 1, T_, F_, {"bias"}, (0, 32, 0, 0)),
    ("s32-k60", 33, 129, 60, 1, 1, T_, T_, {"rowsum", "a_drop", "c_drop", "act", "C2"}, (0, 32, 0, 0)),
    ("s32-k65", 129, 258, 65, 1, 1, T_, F_, {"bias", "residual", "accumulate"}, (0, 32, 0, 0)),
    ("s32-k258-FT", 33, 129, 258, 3, 1, F_, T_, {"C_tab", "rowsum_tab", "a_drop"}, (0, 32, 0, 0)),
    ("s64-k65", 1548, 516, 65, 1, 2, T_, F_, {"bias", "c_drop", "C2"}, (0, 64, 0, 0)),
    ("s64-misaligned", 1548, 516, 512, 2, 1, F_, F_, {"misalign", "residual", "a_drop", "A2"}, (0, 64, 0, 0)),
]
PROBES = ("random", "positive", "impulse", "mixed")
EXACT_OK = {"bias", "bias_tab", "B_tab", "C_tab", "A2", "B2", "rowsum", "rowsum_tab", "rowsum_acc", "C2", "view0", "view512", "misalign"}


def _fill(n, seed, probe):
    v = _u(n, seed=seed)
    return v.abs() if probe == "positive" else v


def _place(buf, off, sizes, strides, logical):
    idx = R._view(buf, off, sizes, strides)
    buf[idx] = logical.reshape(sizes)


def _operand(probe, Zt, rows, cols, seed, one_hot):
    """logical [Zt, rows, cols] values of a probe; one_hot: this operand carries the impulse (one 1.0 per row)"""
    v = _u(Zt, rows, cols, seed=seed)
    if probe == "positive":
        v = v.abs()
    elif probe == "impulse" and one_hot:
        v = torch.zeros_like(v)
        r = torch.arange(rows, device=DEV)
        for z in range(Zt):
            v[z, r, (7 * r + 3 + z) % cols] = 1.0
    elif probe == "mixed" and one_hot:
        v[:, torch.arange(rows, device=DEV) % 3 == 1, :] *= 2.0 ** -16
    return v


def _build(hip, case, probe, seed=0):
    """(args struct, reference-args dict, {name: buffer}) of a case with every buffer inside guard bands"""
    name, M, N, K, ZB, ZH, AK, BN, feat, _ = case
    Zt = ZB * ZH
    tabs = {"B_tab", "bias_tab", "C_tab", "rowsum_tab"} & feat
    bufs, g = {}, dict(M=M, N=N, K=K, ZB=ZB, ZH=ZH, alpha=0.5 if "alpha" in feat else 1.0, act=int("act" in feat),
                       accumulate=int("accumulate" in feat))
    # A (and A2): [Zt][M][K] at zoff + m sa_m + k sa_k
    if "view0" in feat or "view512" in feat:               # dy[:, :512] / dy[:, 512:] of a [Zt * M, 1536] matrix
        sa_m, sa_k, aoff = 1536, 1, (0 if "view0" in feat else 512)
        sa_zb = M * 1536
    else:
        sa_m, sa_k = (K + (4 if K % 4 == 0 else 3), 1) if AK else (1, M + (4 if M % 4 == 0 else 3))
        aoff = 1 if "misalign" in feat else 4
        span = (M - 1) * sa_m + (K - 1) * sa_k + 1
        sa_zb = (span + 7) // 4 * 4
    g.update(sa_m=sa_m, sa_k=sa_k, sa_zb=sa_zb * ZH, sa_zh=sa_zb)
    a_n = aoff + Zt * sa_zb + 8
    for key in (("A", "A2") if "A2" in feat else ("A",)):
        buf = _u(a_n, seed=seed + (1 if key == "A" else 2))
        lg = _operand(probe, Zt, M, K, seed + (3 if key == "A" else 4), True)
        for z in range(Zt):
            _place(buf, aoff + (z // ZH) * g["sa_zb"] + (z % ZH) * g["sa_zh"], (M, K), (sa_m, sa_k), lg[z])
        bufs[key] = buf
        g[key] = (buf, aoff)
    if "A2" in feat:
        g["split_n"] = 512 if N > 512 else (128 if N > 128 else 64)
    # B (and B2 / B_tab): [Zt][K][N]
    sb_k, sb_n = (N + 4, 1) if BN else (1, K + 4)
    span = (K - 1) * sb_k + (N - 1) * sb_n + 1
    sb_zb = (span + 7) // 4 * 4
    g.update(sb_k=sb_k, sb_n=sb_n, sb_zb=sb_zb * ZH, sb_zh=sb_zb)
    boff = 1 if "misalign" in feat else 4
    b_n = boff + Zt * sb_zb + 8
    lgB = _operand(probe, Zt, K, N, seed + 5, False)
    if "B_tab" in feat:
        g["B_tab"] = []
        for z in range(Zt):
            buf = _u(b_n, seed=seed + 40 + z)
            _place(buf, boff, (K, N), (sb_k, sb_n), lgB[z])
            bufs["B_tab%d" % z] = buf
            g["B_tab"].append((buf, boff))
    else:
        buf = _u(b_n, seed=seed + 6)
        for z in range(Zt):
            _place(buf, boff + (z // ZH) * g["sb_zb"] + (z % ZH) * g["sb_zh"], (K, N), (sb_k, sb_n), lgB[z])
        bufs["B"] = buf
        g["B"] = (buf, boff)
    if "B2" in feat:
        buf = _u(b_n, seed=seed + 7)
        lg2 = _operand(probe, Zt, K, N, seed + 8, False)
        for z in range(Zt):
            _place(buf, boff + (z // ZH) * g["sb_zb"] + (z % ZH) * g["sb_zh"], (K, N), (sb_k, sb_n), lg2[z])
        bufs["B2"] = buf
        g["B2"] = (buf, boff)
        g["split_m"] = 512 if M > 512 else 256
    # C (or C_tab), C2: [Zt][M][N] at coff + zoff + m sc_m + n, guard bands all round
    sc_m = N + 3
    c_z = M * sc_m + 5
    g.update(sc_m=sc_m, sc_zb=c_z * ZH, sc_zh=c_z)
    coff = 7
    c_n = coff + Zt * c_z + 9
    if "C_tab" in feat:
        g["C_tab"] = []
        for z in range(Zt):
            bufs["C_tab%d" % z] = _fill(c_n, seed + 50 + z, probe)
            g["C_tab"].append((bufs["C_tab%d" % z], coff))
    else:
        bufs["C"] = _fill(c_n, seed + 9, probe)
        g["C"] = (bufs["C"], coff)
    if "C2" in feat:
        bufs["C2"] = _u(c_n, seed=seed + 10)
        g["C2"] = (bufs["C2"], coff)
    if "bias" in feat:
        bufs["bias"] = _fill(N + 8, seed + 11, probe)
        g["bias"] = (bufs["bias"], 4)
    if "bias_tab" in feat:
        g["bias_tab"] = []
        for z in range(Zt):
            bufs["bias_tab%d" % z] = _fill(N + 8, seed + 60 + z, probe)
            g["bias_tab"].append((bufs["bias_tab%d" % z], 4))
    if "residual" in feat:
        sr_m = N + 2
        bufs["res"] = _fill(4 + Zt * M * sr_m + 4, seed + 12, probe)
        g.update(residual=(bufs["res"], 4), sr_m=sr_m, sr_zb=M * sr_m * ZH, sr_zh=M * sr_m)
    if "rowsum" in feat:
        bufs["rowsum"] = _fill(M + 16, seed + 13, probe)
        g["rowsum"] = (bufs["rowsum"], 8)
    if "rowsum_tab" in feat:
        g["rowsum_tab"] = []
        for z in range(Zt):
            bufs["rowsum_tab%d" % z] = _fill(M + 16, seed + 70 + z, probe)
            g["rowsum_tab"].append((bufs["rowsum_tab%d" % z], 8))
    g["rowsum_acc"] = int("rowsum_acc" in feat)
    if "a_drop" in feat:
        g.update(a_drop_off=1000, a_drop_n=a_n, a_drop_p=0.1, a_drop_p2=0.0)
    if "c_drop" in feat or "c_drop2" in feat:
        g.update(c_drop_off=5000 + 3 * a_n, c_drop_n=c_n, c_drop_p=0.1, c_drop_p2=0.2 if "c_drop2" in feat else 0.0)
    assert not tabs or ZH == 1
    return _struct(hip, g), g, bufs


def _ptr(pair):
    buf, off = pair
    return buf.data_ptr() + 4 * off


def _struct(hip, g):
    from cwf import _lib
    a = _lib.GemmArgs()
    for k, v in g.items():
        if k in ("A", "A2", "B", "B2", "C", "C2", "bias", "residual", "rowsum"):
            setattr(a, k, _ptr(v))
        elif k in ("B_tab", "bias_tab", "C_tab", "rowsum_tab"):
            setattr(a, k, (ctypes.c_void_p * 4)(*([_ptr(p) for p in v] + [0] * (4 - len(v)))))
        else:
            setattr(a, k, v)
    if g.get("a_drop_p", 0) > 0 or g.get("c_drop_p", 0) > 0:
        a.rng = hip.rng(DEV).data_ptr()
    return a


def _variant(hip, a):
    out = (ctypes.c_int * 4)()
    rc = hip.lib.cwf_debug_gemm_variant(ctypes.byref(a), out)
    return rc, tuple(out)


def test_gemm_variant_reach(hip):
    """the case table reaches all ten kernels: vector 64x64 / 32x32 x four <AK, BN> forms, scalar 64x64 / 32x32"""
    seen = {}
    for case in GEMM_CASES:
        a, _, _ = _build(hip, case, "random")
        rc, v = _variant(hip, a)
        assert rc == 0 and v == case[-1], (case[0], rc, v)
        seen.setdefault(v, []).append(case[0])
    want = {(1, tm, ak, bn) for tm in (32, 64) for ak in (0, 1) for bn in (0, 1)} | {(0, 64, 0, 0), (0, 32, 0, 0)}
    for v in sorted(seen):
        print("  variant vec=%d TM=%d AK=%d BN=%d: %s" % (v + (", ".join(seen[v]),)))
    assert set(seen) == want


@pytest.mark.parametrize("probe", PROBES)
@pytest.mark.parametrize("case", GEMM_CASES, ids=[c[0] for c in GEMM_CASES])
def test_gemm_case(hip, case, probe):
    name, M, N, K, ZB, ZH, AK, BN, feat, expect = case
    a, g, bufs = _build(hip, case, probe, seed=100 * GEMM_CASES.index(case))
    assert _variant(hip, a) == (0, expect)
    before = {k: v.clone() for k, v in bufs.items()}
    E = _emul(hip)
    ref = R.gemm_ex(g, E)
    hip._call("cwf_gemm_ex", ctypes.addressof(a), hip._stream())
    _sync()
    form = "%s%d %s%s" % ("vec" if expect[0] else "scalar", expect[1], "T" if expect[2] else "F", "T" if expect[3] else "F")
    gam = R.gamma_gemm(K)
    exact = probe == "impulse" and feat <= EXACT_OK
    outputs = set()
    for key, (v, A, wr) in ref["C"].items():
        bname = next(k for k, b in bufs.items() if id(b) == key)
        outputs.add(bname)
        got = bufs[bname]
        assert torch.equal(got[~wr], before[bname][~wr]), (name, probe, bname, "guard band / untouched elements changed")
        if exact:
            assert torch.equal(got[wr], v[wr].float()), (name, bname, "impulse probe must be exact")
        _worst("gemm %s" % form, got[wr], v[wr], gam * A[wr], gam)
    for key, (v, A, wr) in ref["rowsum"].items():
        bname = next(k for k, b in bufs.items() if id(b) == key)
        outputs.add(bname)
        got = bufs[bname]
        assert torch.equal(got[~wr], before[bname][~wr]), (name, bname, "rowsum guard band changed")
        if exact:
            assert torch.equal(got[wr], v[wr].float()), (name, bname, "impulse rowsum must be exact")
        _worst("gemm rowsum", got[wr], v[wr], gam * A[wr], gam)
    if ref["C2"] is not None:
        v, A, wr = ref["C2"]
        outputs.add("C2")
        assert torch.equal(bufs["C2"][~wr], before["C2"][~wr]), (name, "C2 guard band changed")
        _worst("gemm pre-activation (C2)", bufs["C2"][wr], v[wr], gam * A[wr], gam)
        for zi in ref["z"]:                                  # the epilogue alone, on the kernel's own pre-activation
            bname = next(k for k, b in bufs.items() if id(b) == zi["C"])
            pre = bufs["C2"][zi["c2_idx"]]
            e_ref, e_A = R.gemm_epilogue(pre, g["act"], zi["keep"], zi["scale"], zi["residual"], zi["old"])
            _worst("gemm epilogue from own C2", bufs[bname][zi["c_idx"]], e_ref, R.GAMMA_EPI * e_A, R.GAMMA_EPI)
    for k in bufs:                                           # inputs are never written
        if k not in outputs:
            assert torch.equal(bufs[k], before[k]), (name, k, "an input buffer changed")


def test_gemm_refusals(hip):
    """each refusal returns its code from cwf_gemm_ex (and the variant query) without launching: C stays as it was"""
    from cwf import _lib
    case = ("refusal", 129, 128, 64, 1, 1, T_, F_, {"A2"}, None)

    def attempt(mutate, code, what):
        a, g, bufs = _build(hip, case, "random")
        mutate(a, bufs)
        before = bufs["C"].clone()
        rc = hip.lib.cwf_gemm_ex(ctypes.addressof(a), hip._stream())
        _sync()
        assert rc == code, (what, rc)
        assert _variant(hip, a)[0] == code, what
        assert torch.equal(bufs["C"], before), (what, "launched anyway")

    def split(a, b):
        a.split_n = 96
    attempt(split, BADARG, "split_n not a multiple of 64")

    def split_m(a, b):
        a.B2 = a.B
        a.split_m = 32
    attempt(split_m, BADARG, "split_m not a multiple of 64")

    def tab_zh(a, b):
        a.B_tab = (ctypes.c_void_p * 4)(a.B, a.B, 0, 0)
        a.ZB, a.ZH = 1, 2
    attempt(tab_zh, BADARG, "B_tab with ZH != 1")

    def tab_zb(a, b):
        a.C_tab = (ctypes.c_void_p * 4)(a.C, a.C, a.C, a.C)
        a.ZB = 5
    attempt(tab_zb, BADARG, "C_tab with ZB > 4")

    def rowsum(a, b):
        a.rowsum = a.C
        a.ZB = 2
    attempt(rowsum, BADARG, "rowsum with ZB * ZH != 1")

    def adrop(a, b):
        a.a_drop_p, a.a_drop_n, a.rng = 0.1, 1 << 20, 0
    attempt(adrop, BADARG, "a_drop without rng")

    def cdrop(a, b):
        a.c_drop_p, a.c_drop_n, a.rng = 0.1, 1 << 20, 0
    attempt(cdrop, BADARG, "c_drop without rng")
    assert _lib.GemmArgs is not None


# ====================================================================================================== attention
ATTN_T = (1, 2, 15, 16, 17, 31, 32, 33, 64, 65, 128, 129, 143, 144)


def _attn_case(hip, Z, T, heads, probe, p, seed):
    E = _emul(hip)
    e = heads * 64
    ld, ldo = 3 * e + 8, e + 4
    qkv = _u(Z * T, ld, seed=seed)
    if probe == "peaked":
        qkv[:, :e] *= 8.0
    elif probe == "mixed":
        rows = torch.arange(Z * T, device=DEV) % 3 == 1
        qkv[rows, 2 * e:3 * e] *= 2.0 ** -16
    d_o = _u(Z * T, ldo, seed=seed + 1)
    if probe == "mixed":
        d_o[torch.arange(Z * T, device=DEV) % 4 == 2, :e] *= 2.0 ** -16
    off = 777 + seed
    scale = float(64 ** -0.5)
    o = _u(Z * T, ldo, seed=seed + 2)
    o0 = o.clone()
    rng = hip.rng(DEV).data_ptr()
    hip._call("cwf_attn_fwd", qkv.data_ptr(), ld, o.data_ptr(), ldo, Z, T, e, heads, scale, rng, off, float(p), hip._stream())
    dqkv = _u(Z * T, ld, seed=seed + 3)
    dq0 = dqkv.clone()
    hip._call("cwf_attn_bwd", qkv.data_ptr(), ld, d_o.data_ptr(), ldo, dqkv.data_ptr(), Z, T, e, heads, scale, rng, off, float(p),
              hip._stream())
    _sync()
    mask = R.attn_mask(E, Z, T, heads, off, p)
    ref, A = R.attn_fwd(qkv, Z, T, heads, mask)
    tag = "T=%d h=%d %s p=%g" % (T, heads, probe, p)
    assert torch.equal(o[:, e:], o0[:, e:]), (tag, "o padding columns written")
    _worst("attn fwd", o[:, :e], ref, R.GAMMA_ATTN * A, R.GAMMA_ATTN)
    (dq, dk, dv), (Aq, Ak, Av) = R.attn_bwd(qkv, d_o, Z, T, heads, mask)
    assert torch.equal(dqkv[:, 3 * e:], dq0[:, 3 * e:]), (tag, "dqkv padding columns written")
    g = R.GAMMA_ATTN_BWD
    _worst("attn bwd dQ", dqkv[:, :e], dq, g * Aq, g)
    _worst("attn bwd dK", dqkv[:, e:2 * e], dk, g * Ak, g)
    _worst("attn bwd dV", dqkv[:, 2 * e:3 * e], dv, g * Av, g)


@pytest.mark.parametrize("heads", [1, 8])
@pytest.mark.parametrize("T", ATTN_T)
def test_attention(hip, T, heads):
    for probe in ("flat", "peaked", "mixed"):
        for p in (0.0, 0.1):
            _attn_case(hip, 2, T, heads, probe, p, seed=T * 10 + heads)


def test_attention_production_z12(hip):
    for p in (0.0, 0.1):
        _attn_case(hip, 12, 129, 8, "flat", p, seed=5)


def test_attention_refusal(hip):
    qkv = torch.zeros(145, 192, device=DEV)
    o = torch.zeros(145, 64, device=DEV)
    rc = hip.lib.cwf_attn_fwd(qkv.data_ptr(), 192, o.data_ptr(), 64, 1, 145, 64, 1, ctypes.c_float(0.125), None,
                              ctypes.c_uint64(0), ctypes.c_float(0.0), ctypes.c_void_p(hip._stream()))
    assert rc == TOOLARGE
    rc = hip.lib.cwf_attn_bwd(qkv.data_ptr(), 192, o.data_ptr(), 64, qkv.data_ptr(), 1, 145, 64, 1, ctypes.c_float(0.125), None,
                              ctypes.c_uint64(0), ctypes.c_float(0.0), ctypes.c_void_p(hip._stream()))
    assert rc == TOOLARGE


# ====================================================================================================== LayerNorm
def _ln_inputs(rows, E, seed):
    x = _u(rows, E, seed=seed) * 2 + 0.3
    r = torch.arange(rows, device=DEV)
    x[r % 7 == 3] += 100.0                                    # |mean| >> std
    x[r % 11 == 5] = 0.3                                      # constant rows
    x[r % 13 == 6] *= 2.0 ** -12
    return x


def _ln_params(G, E, seed):
    return [[(_u(E, seed=seed + 10 * i + g) * 0.1 + (1.0 if i % 2 == 0 else 0.0)) for g in range(G)] for i in range(4)]


@pytest.mark.parametrize("E,G", [(64, 1), (128, 2), (256, 3), (512, 4), (512, 1), (64, 4)])
@pytest.mark.parametrize("form", ["dual", "self", "single"])
def test_layernorm(hip, E, G, form):
    perm_T = 129 if form == "self" else 0
    rpg = 258 if form == "self" else 129 + (E == 512)       # rows per group: not a multiple of 4 (or of 64) off the self form
    rows = G * rpg
    x = _ln_inputs(rows, E, seed=E + G)
    x2 = x if form == "self" else (None if form == "single" else _ln_inputs(rows, E, seed=E + G + 1) * 0.5)
    g1, b1, g2, b2 = _ln_params(G, E, seed=E * 3 + G)
    grp = torch.arange(rows, device=DEV) // rpg
    rowp = lambda ps: torch.stack(ps)[grp]
    ya, yb, st = hip.ln_pair_fwd(x, x2, perm_T, g1, b1, g2 if x2 is not None else None, b2 if x2 is not None else None)
    _sync()
    gam = R.gamma_ln(E)
    perm = R.ln_perm(rows, perm_T).to(DEV)
    y, A, mu, rs, Amu, Ars = R.ln_fwd(x, rowp(g1), rowp(b1))
    _worst("ln fwd y", ya, y, gam * A, gam)
    _worst("ln fwd mean", st[0, :, 0], mu, gam * Amu, gam)
    _worst("ln fwd rstd", st[0, :, 1], rs, gam * Ars, gam)
    if x2 is not None:
        y, A, mu, rs, Amu, Ars = R.ln_fwd(x2[perm], rowp(g2), rowp(b2))
        _worst("ln fwd y", yb, y, gam * A, gam)
        _worst("ln fwd mean", st[1, :, 0], mu, gam * Amu, gam)
        _worst("ln fwd rstd", st[1, :, 1], rs, gam * Ars, gam)
    # backward from the kernel's own stats
    dy, da, db = _u(rows, E, seed=1), _u(rows, E, seed=2), _u(rows, E, seed=3)
    db_ = db if x2 is not None else None
    for acc in (False, True):
        old = [[_u(E, seed=90 + 4 * i + g) for g in range(G)] for i in range(4)]
        pg = [[t.clone() for t in o] for o in old]
        dx, dx2 = hip.ln_pair_bwd(dy, da, db_, x, x2, perm_T, g1, g2 if x2 is not None else None, st, pg[0], pg[1],
                                  pg[2] if x2 is not None else None, pg[3] if x2 is not None else None, acc, form == "dual")
        _sync()
        ref, A = R.ln_bwd_term(da, x, rowp(g1), st[0, :, 0], st[0, :, 1])
        ref, A = ref + dy.double(), A + dy.double().abs()
        if form == "self":
            t, tA = R.ln_bwd_term(db[perm], x, rowp(g2), st[1, perm, 0], st[1, perm, 1])
            ref, A = ref + t, A + tA
        _worst("ln bwd dx", dx, ref, gam * A, gam)
        if form == "dual":
            t, tA = R.ln_bwd_term(db, x2, rowp(g2), st[1, :, 0], st[1, :, 1])
            _worst("ln bwd dx", dx2, t, gam * tA, gam)
        gp = R.gamma_params(rpg)
        probs = [(da, x, st[0, :, 0], st[0, :, 1], 0)]
        if x2 is not None:
            probs.append((db, x2[perm], st[1, :, 0], st[1, :, 1], 2))
        for d, xs, mu, rs, i in probs:
            dg, Ag, dbt, Ab = R.ln_params(d, xs, mu, rs, G)
            for gi in range(G):
                o_g, o_b = (old[i][gi].double(), old[i + 1][gi].double()) if acc else (0.0, 0.0)
                _worst("ln params dgamma", pg[i][gi], dg[gi] + o_g, gp * (Ag[gi] + abs(o_g) if acc else Ag[gi]), gp)
                _worst("ln params dbeta", pg[i + 1][gi], dbt[gi] + o_b, gp * (Ab[gi] + abs(o_b) if acc else Ab[gi]), gp)
        if x2 is None:
            for i in (2, 3):
                for gi in range(G):
                    assert torch.equal(pg[i][gi], old[i][gi])


def test_layernorm_refusals(hip):
    from cwf import _lib, kernels
    x = torch.zeros(258, 96, device=DEV)
    ya, st = torch.zeros_like(x), torch.zeros(2, 258, 2, device=DEV)
    gm = [torch.ones(96, device=DEV)] * 2
    P, _ = kernels._ln_params(g1=gm, b1=gm)
    call = lambda rows, E, G, perm, x2: hip.lib.cwf_ln_pair_fwd_g(x.data_ptr(), x2, perm, ctypes.addressof(P), G, ya.data_ptr(),
                                                                    ya.data_ptr() if x2 else None, st.data_ptr(), rows, E,
                                                                    ctypes.c_float(1e-5), ctypes.c_void_p(hip._stream()))
    assert call(258, 96, 1, 0, None) == BADARG                        # E = 96
    assert call(257, 64, 2, 0, None) == BADARG                        # rows % G
    P2, _ = kernels._ln_params(g1=gm, b1=gm, g2=gm, b2=gm)
    P = P2
    assert call(258, 64, 2, 129, x.data_ptr()) == BADARG              # perm_T does not divide the 129 rows per group
    _sync()
    assert _lib is not None


# ====================================================================================================== GELU backward
@pytest.mark.parametrize("p", [0.0, 0.1])
def test_gelu_bwd_drop(hip, p):
    n = 516 * 2048 + 3
    z, dh = _u(n, seed=7, s=6.0), _u(n, seed=8)
    E = _emul(hip)
    dz = hip.gelu_bwd_drop(z, dh, (4242, p) if p else None)
    _sync()
    keep = E.keep(4242, n, p).double().to(DEV) if p else None
    ref, A = R.gelu_bwd_drop(z, dh, keep, R.keep_scale(p))
    _worst("gelu_bwd_drop", dz, ref, R.GAMMA_GELU * A, R.GAMMA_GELU)


# ====================================================================================================== token kernels
TOPK_T = (1, 128, 1023, 1024, 1025, 2048, 4800, 16384)


def _special_scores(s, seed):
    """ties, +-0.0, +-inf and NaN planted into fp32 scores"""
    s = s.clone()
    B, T = s.shape
    g = torch.Generator().manual_seed(seed)
    pick = lambda: torch.randint(0, T, (max(1, T // 64),), generator=g).to(DEV)
    s[:, pick()] = 0.0
    s[:, pick()] = -0.0
    s[:, pick()] = s[0, 0].item()                                    # ties with a live score
    if T > 8:
        s[:, pick()] = float("inf")
        s[:, pick()] = -float("inf")
        s[:, pick()] = float("nan")
    return s


@pytest.mark.parametrize("T", TOPK_T)
def test_scores_and_topk(hip, T):
    B, E = 2, 512
    feats = _u(B, T, E, seed=T)
    q1, q2 = _u(B, 1, E, seed=T + 1), _u(1, 1, E, seed=T + 2)
    s1, s2 = hip.token_scores2(feats, q1, q2)
    _sync()
    gs = R.gamma_score(E)
    for got, q in ((s1, q1), (s2, q2)):
        ref, A = R.scores(feats, q.reshape(q.shape[0], E))
        _worst("token_scores2", got, ref, gs * A, gs)
    for k in sorted({1, max(1, T // 3), T}):
        for special in (False, True):
            a, b = (_special_scores(s1, T + k), _special_scores(s2, T - k)) if special else (s1, s2)
            i0, v0, i1, v1 = hip.topk_inv(a.contiguous(), b.contiguous(), k)
            _sync()
            for got_i, got_v, sc in ((i0, v0, a), (i1, v1, b)):
                ri, rv = R.topk_inv(sc, k)
                assert torch.equal(got_i, ri), ("topk index", T, k, special)
                assert torch.equal(got_v, rv), ("topk inverse map", T, k, special)
            idx, inv = hip.index_inv(i0, T)
            _sync()
            assert torch.equal(inv, R.index_inv(i0, T)), ("index_inv", T, k)


def test_scores_grouped(hip):
    G, gB, T, E = 3, 2, 1025, 512
    feats = _u(G * gB, T, E, seed=3)
    q1 = [_u(1, 1, E, seed=10 + g) for g in range(G)]
    q2 = [_u(1, 1, E, seed=20 + g) for g in range(G)]
    s1, s2 = hip.token_scores2(feats, q1, q2)
    _sync()
    gs = R.gamma_score(E)
    for got, qs in ((s1, q1), (s2, q2)):
        q = torch.cat([qs[b // gB].reshape(1, E) for b in range(G * gB)])
        ref, A = R.scores(feats, q)
        _worst("token_scores2_g", got, ref, gs * A, gs)


def test_topk_refusal(hip):
    s = torch.zeros(1, 16385, device=DEV)
    i = torch.zeros(1, 16385, dtype=torch.int32, device=DEV)
    rc = hip.lib.cwf_topk_inv(s.data_ptr(), i.data_ptr(), i.data_ptr(), None, None, None, 1, 16385, 8, ctypes.c_void_p(hip._stream()))
    assert rc == TOOLARGE


def _selection(B, T, k, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.stack([torch.randperm(T, generator=g)[:k] for _ in range(B)]).to(torch.int32).to(DEV)


@pytest.mark.parametrize("T,k", [(1, 1), (129, 128), (1025, 128), (4800, 128)])
@pytest.mark.parametrize("p", [0.0, 0.1])
def test_gather_scatter_token_grad(hip, T, k, p):
    B, E = 2, 512
    Em = _emul(hip)
    feats = _u(B, T, E, seed=T)
    ip, iq = _selection(B, T, k, T + 1), _selection(B, T, k, T + 2)
    _, inv_p = hip.index_inv(ip, T)
    _, inv_q = hip.index_inv(iq, T)
    head = _u(B, 1, E, seed=5)
    head_g = [_u(1, 1, E, seed=6 + g) for g in range(2)]
    offs = (100, 100 + 2 * B * k * E)
    o0, o1 = torch.empty(B, k + 1, E, device=DEV), torch.empty(B, k + 1, E, device=DEV)
    hip.gather_multi([(feats, ip, head, o0, offs[0]), (feats, iq, head_g, o1, offs[1])], k, E, p=p, pe_odd=0.25)
    _sync()
    n = B * k * E
    for got, idx, hd, off in ((o0, ip, head, offs[0]), (o1, iq, torch.cat([head_g[b // 1] for b in range(B)]), offs[1])):
        keep = Em.keep(off, n, p).to(DEV).reshape(B, k, E) if p else None
        ref = R.gather_job(feats, idx, hd, k, 0.25, keep)
        assert torch.equal(got, ref), ("gather_multi", T, k, p)
    # scatter_inv: scat / gated
    rows = _u(B, k, E + 4, seed=9)[:, :, :E]
    gate = _u(B, 1, E, seed=10)
    gated, scat = hip.scatter_inv(feats, inv_p, rows, gate, want_gated=True, want_scat=True)
    _sync()
    sel = inv_p.long()
    ref_scat = torch.where((sel >= 0).unsqueeze(-1), rows.gather(1, sel.clamp_min(0).unsqueeze(-1).expand(B, T, E)), feats)
    assert torch.equal(scat, ref_scat) and torch.equal(gated, ref_scat * gate)
    # scatter_bwd: drows (one rounding or a contracted fma) and dgate (bounded, fixed order)
    dgated, dscat, extra = _u(B, T, E, seed=11), _u(B, T, E, seed=12), _u(B, 1, E, seed=13)
    drows_buf = _u(B, k, E + 4, seed=14)
    dgate_buf = _u(B, 1, E + 4, seed=15)
    d0, g0 = drows_buf.clone(), dgate_buf.clone()
    hip.scatter_bwd(dgated, dscat, feats, inv_p, ip, rows, gate, extra, drows_buf[:, :, :E], dgate_buf[:, :, :E])
    _sync()
    assert torch.equal(drows_buf[:, :, E:], d0[:, :, E:]) and torch.equal(dgate_buf[:, :, E:], g0[:, :, E:])
    t = ip.long().clamp(0, T - 1).unsqueeze(-1).expand(B, k, E)
    two, one = R.fp32_mul_add(dgated.gather(1, t), gate.expand(B, k, E), dscat.gather(1, t))
    got = drows_buf[:, :, :E]
    assert bool(((got == two) | (got == one)).all()), ("scatter_bwd drows", T, k)
    dref = (dgated.double() * ref_scat.double()).sum(1, keepdim=True) + extra.double()
    dA = (dgated.double().abs() * ref_scat.double().abs()).sum(1, keepdim=True) + extra.double().abs()
    gd = R.gamma_dgate(T)
    _worst("scatter_bwd dgate", dgate_buf[:, :, :E], dref, gd * dA, gd)
    # token_grad
    dsp, dsq = _u(B, k + 1, E, seed=16), _u(B, k + 1, E, seed=17)
    dfe = hip.token_grad(dgated, dscat, gate, inv_p, inv_q, dsp, dsq, k, p=p, off_p=offs[0], off_q=offs[1])
    _sync()
    kp = Em.keep(offs[0], n, p).to(DEV).reshape(B, k, E) if p else torch.ones(B, k, E, device=DEV)
    kq = Em.keep(offs[1], n, p).to(DEV).reshape(B, k, E) if p else torch.ones(B, k, E, device=DEV)
    jp, jq = inv_p.long(), inv_q.long()
    gat = lambda src, j: src.gather(1, j.clamp_min(0).unsqueeze(-1).expand(B, T, E))
    base_two, base_one = R.fp32_mul_add(dgated, gate.expand(B, T, E), dscat)
    sel_p = gat(dsp[:, 1:], jp) * gat(kp, jp)                 # one fp32 rounding (a product)
    q_two = gat(dsq[:, 1:], jq)
    q_k = gat(kq, jq)
    ok = torch.zeros(B, T, E, dtype=torch.bool, device=DEV)
    for base in (base_two, base_one):
        v = torch.where((jp >= 0).unsqueeze(-1), sel_p, base)
        for cand in (v + q_two * q_k, (v.double() + q_two.double() * q_k.double()).float()):
            full = torch.where((jq >= 0).unsqueeze(-1), cand, v)
            ok |= dfe == full
    assert bool(ok.all()), ("token_grad", T, k, p)


def test_head_grad(hip):
    B, E = 6, 512
    a1, c1, a2, c2 = (_u(B, 1, E + 4, seed=s)[:, 0, :E] for s in range(4))
    o1, o2 = hip.head_grad(a1, c1, a2, c2)
    _sync()
    assert torch.equal(o1.reshape(E), R.head_grad(a1, c1)[0]) and torch.equal(o2.reshape(E), R.head_grad(a2, c2)[0])
    G = 3
    outs1 = [torch.empty(1, 1, E, device=DEV) for _ in range(G)]
    outs2 = [torch.empty(1, 1, E, device=DEV) for _ in range(G)]
    hip.head_grad(a1, c1, a2, c2, outs1, outs2)
    _sync()
    for gi, (r1, r2) in enumerate(zip(R.head_grad(a1, c1, G), R.head_grad(a2, c2, G))):
        assert torch.equal(outs1[gi].reshape(E), r1) and torch.equal(outs2[gi].reshape(E), r2)


# ====================================================================================================== determinism
def test_determinism(hip):
    """fixed summation order, plain stores: a second launch is bitwise equal to the first"""
    # GEMM with rowsum (and the weight-gradient form's a_drop)
    case = next(c for c in GEMM_CASES if c[0] == "FT-k258")
    outs = []
    for _ in range(2):
        a, g, bufs = _build(hip, case, "random", seed=3)
        hip._call("cwf_gemm_ex", ctypes.addressof(a), hip._stream())
        _sync()
        outs.append((bufs["C"].clone(), bufs["rowsum"].clone()))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    # ln_pair_bwd (dx and the four parameter sums)
    rows, E = 516, 512
    x = _ln_inputs(rows, E, 1)
    g1, b1, g2, b2 = _ln_params(1, E, 2)
    _, _, st = hip.ln_pair_fwd(x, x, 129, g1, b1, g2, b2)
    dy, da, db = _u(rows, E, seed=1), _u(rows, E, seed=2), _u(rows, E, seed=3)
    res = []
    for _ in range(2):
        pg = [[torch.empty(E, device=DEV)] for _ in range(4)]
        dx, _ = hip.ln_pair_bwd(dy, da, db, x, x, 129, g1, g2, st, pg[0], pg[1], pg[2], pg[3], False, False)
        _sync()
        res.append([dx] + [p[0] for p in pg])
    assert all(torch.equal(u, v) for u, v in zip(*res))
    # scatter_bwd dgate and gelu_bwd_drop
    B, T, k = 2, 4800, 128
    feats = _u(B, T, E, seed=4)
    ip = _selection(B, T, k, 5)
    _, inv = hip.index_inv(ip, T)
    rows_, gate = _u(B, k, E, seed=6), _u(B, 1, E, seed=7)
    dgated, dscat = _u(B, T, E, seed=8), _u(B, T, E, seed=9)
    res = []
    for _ in range(2):
        drows, dgate = torch.empty(B, k, E, device=DEV), torch.empty(B, 1, E, device=DEV)
        hip.scatter_bwd(dgated, dscat, feats, inv, ip, rows_, gate, None, drows, dgate)
        z = hip.gelu_bwd_drop(dgated.reshape(-1), dscat.reshape(-1), (99, 0.1))
        _sync()
        res.append((drows, dgate, z))
    assert all(torch.equal(u, v) for u, v in zip(*res))
