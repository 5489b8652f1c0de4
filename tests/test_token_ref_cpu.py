"""CPU: the float64 token-path reference of tests/token_ref.py against torch (F.linear, F.layer_norm, F.gelu and a softmax
attention restatement, with autograd), a correct fp32 emulation passing its bounds, and planted defects -- inserted into the
reference's own output, never into a kernel -- failing them by >= 30x.  The mixed-scale probe (rows scaled by 2^-16) pins which
defects the suite's earlier normwise check (close(..., 2e-5) of tests/test_coupler_gpu.py) could not see."""
import math

import pytest
import torch
import torch.nn.functional as F

import token_ref as R
from oracle.kernel_emul import EmulBackend

FACTOR = 30.0


def _u(*shape, seed, s=1.0):
    g = torch.Generator().manual_seed(seed)
    return ((torch.rand(*shape, generator=g) * 2 - 1) * s).float()


def _emul():
    E = EmulBackend()
    E.set_rng(1234567, 3)
    return E


def _mixed(x, seed):
    """every other row (and a random third of the rest) scaled by 2^-16"""
    g = torch.Generator().manual_seed(seed)
    sel = (torch.arange(x.shape[0]) % 2 == 1) | (torch.rand(x.shape[0], generator=g) < 0.33)
    y = x.clone()
    y[sel] *= 2.0 ** -16
    return y, sel


def _linear_args(x, w, out, bias=None, **kw):
    M, K = x.shape
    N = w.shape[0]
    g = dict(A=(x.reshape(-1), 0), sa_m=K, sa_k=1, B=(w.reshape(-1), 0), sb_k=1, sb_n=K, C=(out.reshape(-1), 0), sc_m=N,
             M=M, N=N, K=K, ZB=1, ZH=1, alpha=1.0)
    if bias is not None:
        g["bias"] = (bias, 0)
    g.update(kw)
    return g


def _C(res, buf):
    """(ref, A, written) of the single output buffer of a reference call, shaped like buf"""
    v, A, wr = next(iter(res["C"].values()))
    return v.reshape(buf.shape), A.reshape(buf.shape), wr.reshape(buf.shape)


def _emulate_fp32_gemm(A, B, K):
    """fp32 accumulation in 4-wide K steps (each step's four products summed in float64 and rounded once)"""
    acc = torch.zeros(A.shape[0], B.shape[1], dtype=torch.float32)
    for k0 in range(0, K, 4):
        step = (A[:, k0:k0 + 4].double() @ B[k0:k0 + 4].double()).float()
        acc = acc + step
    return acc


# ------------------------------------------------------------------ the references equal torch in float64
def test_gemm_ref_is_linear_and_its_gradients():
    M, K, N = 33, 65, 40
    x, w, b = _u(M, K, seed=1).double(), _u(N, K, seed=2).double(), _u(N, seed=3).double()
    dy = _u(M, N, seed=4).double()
    xr, wr, br = x.clone().requires_grad_(True), w.clone().requires_grad_(True), b.clone().requires_grad_(True)
    y = F.linear(xr, wr, br)
    y.backward(dy)
    out = torch.zeros(M, N, dtype=torch.float64)
    v, _, wrt = _C(R.gemm_ex(_linear_args(x, w, out, bias=b.reshape(-1))), out)
    assert bool(wrt.all()) and torch.allclose(v, y.detach(), rtol=1e-13, atol=1e-13)
    # data gradient: dx = dy w (A = dy row-major, B = w with k = rows of w)
    dx = torch.zeros(M, K, dtype=torch.float64)
    g = dict(A=(dy.reshape(-1), 0), sa_m=N, sa_k=1, B=(w.reshape(-1), 0), sb_k=K, sb_n=1, C=(dx.reshape(-1), 0), sc_m=K,
             M=M, N=K, K=N, ZB=1, ZH=1)
    v, _, _ = _C(R.gemm_ex(g), dx)
    assert torch.allclose(v, xr.grad, rtol=1e-13, atol=1e-13)
    # weight gradient with the bias gradient as rowsum: dw = dy^T x (A = dy^T: sa_m = 1, sa_k = N)
    dw, db = torch.zeros(N, K, dtype=torch.float64), torch.zeros(N, dtype=torch.float64)
    g = dict(A=(dy.reshape(-1), 0), sa_m=1, sa_k=N, B=(x.reshape(-1), 0), sb_k=K, sb_n=1, C=(dw.reshape(-1), 0), sc_m=K,
             M=N, N=K, K=M, ZB=1, ZH=1, rowsum=(db, 0))
    res = R.gemm_ex(g)
    v, _, _ = _C(res, dw)
    assert torch.allclose(v, wr.grad, rtol=1e-13, atol=1e-13)
    rv = next(iter(res["rowsum"].values()))[0]
    assert torch.allclose(rv, br.grad, rtol=1e-13, atol=1e-13)


def test_gemm_ref_operand_switch_tabs_and_epilogue():
    """split_n / split_m, B_tab / bias_tab / C_tab, GELU, residual, accumulate and two-stage dropout, restated with torch"""
    E = _emul()
    M, K, N, Z = 40, 12, 128, 2
    x, x2 = _u(Z * M, K, seed=1).double(), _u(Z * M, K, seed=2).double()
    ws = [_u(N, K, seed=10 + z).double() for z in range(Z)]
    bs = [_u(N, seed=20 + z).double() for z in range(Z)]
    res = _u(Z * M, N, seed=5).double()
    out = _u(Z * M, N, seed=6).double()
    pre = torch.zeros(Z * M, N, dtype=torch.float64)
    g = dict(A=(x.reshape(-1), 0), sa_m=K, sa_k=1, sa_zb=M * K, A2=(x2.reshape(-1), 0), split_n=64,
             B_tab=[(w.reshape(-1), 0) for w in ws], sb_k=1, sb_n=K, bias_tab=[(b, 0) for b in bs],
             C=(out.reshape(-1), 0), sc_m=N, sc_zb=M * N, C2=(pre.reshape(-1), 0), residual=(res.reshape(-1), 0), sr_m=N, sr_zb=M * N,
             M=M, N=N, K=K, ZB=Z, ZH=1, alpha=0.5, act=1, accumulate=1,
             c_drop_off=77, c_drop_n=Z * M * N, c_drop_p=0.1, c_drop_p2=0.2)
    r = R.gemm_ex(g, E)
    v = next(iter(r["C"].values()))[0].reshape(Z * M, N)
    keep = E.keep(77, Z * M * N, 0.1, 0.2).double().reshape(Z * M, N)
    for z in range(Z):
        rows = slice(z * M, (z + 1) * M)
        xin = torch.cat([x[rows] @ ws[z][:64].t(), x2[rows] @ ws[z][64:].t()], 1)
        p = 0.5 * xin + bs[z]
        ref = F.gelu(p) * keep[rows] + res[rows] + out[rows]
        assert torch.allclose(v[rows], ref, rtol=1e-12, atol=1e-12)
        assert torch.allclose(r["C2"][0].reshape(Z * M, N)[rows], p, rtol=1e-12, atol=1e-12)
    # split_m: rows >= split_m of the output read B2; a_drop keyed on the element offset inside A (column-major A here)
    M, N, K = 130, 20, 24
    A = _u(K, M, seed=7).double()                       # A^T stored: sa_m = 1, sa_k = M
    B1, B2 = _u(K, N, seed=8).double(), _u(K, N, seed=9).double()
    C = torch.zeros(M, N, dtype=torch.float64)
    g = dict(A=(A.reshape(-1), 0), sa_m=1, sa_k=M, B=(B1.reshape(-1), 0), B2=(B2.reshape(-1), 0), split_m=64, sb_k=N, sb_n=1,
             C=(C.reshape(-1), 0), sc_m=N, M=M, N=N, K=K, ZB=1, ZH=1, a_drop_off=5, a_drop_n=M * K, a_drop_p=0.25, a_drop_p2=0.0)
    v = next(iter(R.gemm_ex(g, E)["C"].values()))[0].reshape(M, N)
    Ad = (A * E.keep(5, M * K, 0.25).double().reshape(K, M)).t()
    ref = torch.cat([Ad[:64] @ B1, Ad[64:] @ B2], 0)
    assert torch.allclose(v, ref, rtol=1e-12, atol=1e-12)


def test_layernorm_and_gelu_refs_are_torch():
    rows, E = 24, 128
    x = (_u(rows, E, seed=1) * 3 + 0.7).double()
    gm, bt = (_u(E, seed=2) * 0.1 + 1).double(), (_u(E, seed=3) * 0.1).double()
    d = _u(rows, E, seed=4).double()
    xr, gr, br = x.clone().requires_grad_(True), gm.clone().requires_grad_(True), bt.clone().requires_grad_(True)
    y = F.layer_norm(xr, (E,), gr, br, eps=1e-5)
    y.backward(d)
    yr, _, mu, rs, _, _ = R.ln_fwd(x, gm, bt)
    assert torch.allclose(yr, y.detach(), rtol=1e-12, atol=1e-12)
    dx, _ = R.ln_bwd_term(d, x, gm, mu, rs)
    assert torch.allclose(dx, xr.grad, rtol=1e-10, atol=1e-12)
    dg, _, db, _ = R.ln_params(d, x, mu, rs, 2)
    assert torch.allclose(dg.sum(0), gr.grad, rtol=1e-10, atol=1e-12) and torch.allclose(db.sum(0), br.grad, rtol=1e-12, atol=1e-12)
    z = (_u(1000, seed=5) * 6).double().requires_grad_(True)
    dh = _u(1000, seed=6).double()
    F.gelu(z).backward(dh)
    assert torch.allclose(R.gelu_bwd_drop(z.detach(), dh)[0], z.grad, rtol=1e-12, atol=1e-14)
    assert torch.allclose(R.gelu(z.detach()), F.gelu(z.detach()), rtol=1e-14, atol=1e-15)


@pytest.mark.parametrize("p", [0.0, 0.1])
def test_attention_ref_is_autograd_of_a_restatement(p):
    E = _emul()
    Z, T, heads = 2, 17, 2
    e = heads * 64
    qkv = (_u(Z * T, 3 * e, seed=1) * 2).double()
    d_o = _u(Z * T, e, seed=2).double()
    mask = R.attn_mask(E, Z, T, heads, 99, p)
    leaf = qkv.clone().requires_grad_(True)
    q, k, v = (leaf[:, i * e:(i + 1) * e].reshape(Z, T, heads, 64).transpose(1, 2) for i in range(3))
    P = torch.softmax(q @ k.transpose(-1, -2) / 8.0, -1)
    if mask is not None:
        P = P * mask
    o = (P @ v).transpose(1, 2).reshape(Z * T, e)
    o.backward(d_o)
    o_ref, _ = R.attn_fwd(qkv, Z, T, heads, mask)
    assert torch.allclose(o_ref, o.detach(), rtol=1e-12, atol=1e-13)
    (dq, dk, dv), _ = R.attn_bwd(qkv, d_o, Z, T, heads, mask)
    assert torch.allclose(torch.cat([dq, dk, dv], 1), leaf.grad, rtol=1e-10, atol=1e-12)


def test_topk_reference_order():
    s = torch.tensor([[0.5, float("nan"), float("inf"), -0.0, 0.0, 0.5, -float("inf"), float("nan")]], dtype=torch.float32)
    idx, inv = R.topk_inv(s, 8)
    assert idx.tolist() == [[1, 7, 2, 0, 5, 3, 4, 6]]          # NaN above +inf, ties by index, -0.0 ties +0.0
    idx, inv = R.topk_inv(s, 3)
    assert inv.tolist() == [[-1, 0, 2, -1, -1, -1, -1, 1]]


# ------------------------------------------------------------------ a correct fp32 emulation passes
@pytest.mark.parametrize("K", [4, 60, 65, 258, 516])
@pytest.mark.parametrize("probe", ["random", "positive", "mixed"])
def test_fp32_gemm_emulation_passes(K, probe):
    M, N = 33, 48
    x, w = _u(M, K, seed=K), _u(N, K, seed=K + 1)
    if probe == "positive":
        x, w = x.abs(), w.abs()
    if probe == "mixed":
        x, _ = _mixed(x, K)
    out = torch.zeros(M, N, dtype=torch.float64)
    ref, A, _ = _C(R.gemm_ex(_linear_args(x, w, out)), out)
    got = _emulate_fp32_gemm(x, w.t().contiguous(), K)
    assert R.worst(got, ref, R.gamma_gemm(K) * A, "fp32 emulation K=%d %s" % (K, probe)) <= 1.0


def test_fp32_attention_and_layernorm_emulation_pass():
    Z, T, heads = 2, 33, 1
    qkv = _u(Z * T, 192, seed=3) * 2
    q, k, v = (qkv[:, i * 64:(i + 1) * 64].reshape(Z, T, 64) for i in range(3))
    o32 = (torch.softmax((q @ k.transpose(-1, -2)) * 0.125, -1) @ v).reshape(Z * T, 64)
    ref, A = R.attn_fwd(qkv, Z, T, heads)
    assert R.worst(o32, ref, R.GAMMA_ATTN * A, "fp32 attention") <= 1.0
    x = _u(40, 256, seed=4) * 3 + 50.0                     # |mean| >> std
    gm, bt = _u(256, seed=5) + 1, _u(256, seed=6)
    y32 = F.layer_norm(x, (256,), gm, bt)
    ref, A = R.ln_fwd(x, gm, bt)[:2]
    assert R.worst(y32, ref, R.gamma_ln(256) * A, "fp32 LayerNorm") <= 1.0


# ------------------------------------------------------------------ planted defects
def _gemm_case(probe, K=516, M=129, N=64):
    """x [M, K] (mixed: rows 16..31 and every other row from 40 scaled by 2^-16), w [N, K]; the rows a defect is planted in"""
    x, w = _u(M, K, seed=11), _u(N, K, seed=12)
    rows = torch.arange(M)
    if probe == "mixed":
        sel = torch.zeros(M, dtype=torch.bool)
        sel[16:32] = True
        sel[40::2] = True
        x[sel] *= 2.0 ** -16
        rows = torch.nonzero(sel).squeeze(1)
    out = torch.zeros(M, N, dtype=torch.float64)
    ref, A, _ = _C(R.gemm_ex(_linear_args(x, w, out)), out)
    return x.double(), w.double(), ref, R.gamma_gemm(K) * A, rows


def _rowsum_case(probe, defect):
    """the bias gradient of a Linear as the weight-gradient GEMM's rowsum: dy [129, 516] dropped (p = 0.1), rowsum = column sums
    of dy over the 129 rows; the GEMM's 516 output rows end in a ragged tile (512..515).  Defect: that tile loses the mask."""
    E = _emul()
    T, N, K, p = 129, 516, 64, 0.1
    dy, x = _u(T, N, seed=15), _u(T, K, seed=16)
    if probe == "mixed":
        dy[:, 500:] *= 2.0 ** -16
    rs, out = torch.zeros(N, dtype=torch.float64), torch.zeros(N, K, dtype=torch.float64)
    g = dict(A=(dy.reshape(-1), 0), sa_m=1, sa_k=N, B=(x.reshape(-1), 0), sb_k=K, sb_n=1, C=(out.reshape(-1), 0), sc_m=K,
             M=N, N=K, K=T, ZB=1, ZH=1, rowsum=(rs, 0), a_drop_off=3, a_drop_n=T * N, a_drop_p=p, a_drop_p2=0.0)
    ref, A, _ = next(iter(R.gemm_ex(g, E)["rowsum"].values()))
    bad = ref.clone()
    bad[512:] = dy.double()[:, 512:].sum(0)
    return bad, ref, R.gamma_gemm(T) * A


# which defects today's close(..., 2e-5) passes (True) on each probe: pinned
OLD_PASSES = {
    ("dropped_k_step", "random"): False, ("dropped_k_step", "mixed"): True,
    ("dropped_last_partial_k_step", "random"): False, ("dropped_last_partial_k_step", "mixed"): True,
    ("transposed_tile", "random"): False, ("transposed_tile", "mixed"): True,
    ("rowsum_ragged_tile", "random"): False, ("rowsum_ragged_tile", "mixed"): True,
}


@pytest.mark.parametrize("probe", ["random", "mixed"])
@pytest.mark.parametrize("defect", ["dropped_k_step", "dropped_last_partial_k_step", "transposed_tile", "rowsum_ragged_tile"])
def test_planted_gemm_defects(defect, probe):
    if defect == "rowsum_ragged_tile":
        bad, ref, bound = _rowsum_case(probe, defect)
    else:
        x, w, ref, bound, rows = _gemm_case(probe, K=258 if defect == "dropped_last_partial_k_step" else 516)
        bad = ref.clone()
        if defect == "dropped_k_step":
            bad[rows] -= x[rows, 256:260] @ w[:, 256:260].t()
        elif defect == "dropped_last_partial_k_step":                 # K = 258: the last step holds two live columns
            bad[rows] -= x[rows, 256:258] @ w[:, 256:258].t()
        else:
            bad[16:32, 16:32] = ref[16:32, 16:32].t()
    r = R.ratio(bad, ref, bound)
    print("  planted %-30s %-7s err/bound = %.3g  old close passes: %s" % (defect, probe, r, R.old_close_passes(bad, ref)))
    assert r >= FACTOR, (defect, probe, r)
    assert R.old_close_passes(bad, ref) == OLD_PASSES[(defect, probe)], (defect, probe)


@pytest.mark.parametrize("probe", ["random", "mixed"])
def test_planted_softmax_denominator(probe):
    Z, T, heads = 2, 129, 1
    qkv = _u(Z * T, 192, seed=21)
    if probe == "mixed":                                  # small-magnitude value rows: their outputs are tiny
        qkv[:, 128:], _ = _mixed(qkv[:, 128:], 22)
    ref, A = R.attn_fwd(qkv, Z, T, heads)
    bad, _ = R.attn_fwd(qkv, Z, T, heads, drop_last_key=True)
    assert R.ratio(bad, ref, R.GAMMA_ATTN * A) >= FACTOR
    assert not R.old_close_passes(bad, ref)             # missing 1/129 of the mass moves every output by ~1 %


@pytest.mark.parametrize("probe", ["random", "mixed"])
def test_planted_shifted_dropout_mask(probe):
    E = _emul()
    Z, T, heads, p = 2, 33, 1, 0.1
    qkv = _u(Z * T, 192, seed=31)
    if probe == "mixed":
        qkv, _ = _mixed(qkv, 32)
    mask = R.attn_mask(E, Z, T, heads, 500, p)
    shifted = E.keep(501, Z * heads * T * T, p).double().reshape(Z, heads, T, T)
    ref, A = R.attn_fwd(qkv, Z, T, heads, mask)
    bad, _ = R.attn_fwd(qkv, Z, T, heads, shifted)
    assert R.ratio(bad, ref, R.GAMMA_ATTN * A) >= FACTOR
    assert not R.old_close_passes(bad, ref, rtol=2e-5)
    # the same shift in the GEMM epilogue mask (c_drop)
    x, w = _u(33, 64, seed=33), _u(48, 64, seed=34)
    if probe == "mixed":
        x, _ = _mixed(x, 35)
    out = torch.zeros(33, 48, dtype=torch.float64)
    g = _linear_args(x, w, out, c_drop_off=40, c_drop_n=33 * 48, c_drop_p=p, c_drop_p2=0.0)
    ref, A, _ = _C(R.gemm_ex(g, E), out)
    g["c_drop_off"] = 41
    bad, _, _ = _C(R.gemm_ex(g, E), out)
    assert R.ratio(bad, ref, R.gamma_gemm(64) * A) >= FACTOR


@pytest.mark.parametrize("probe", ["random", "mixed"])
def test_planted_neighbour_rstd(probe):
    rows, E = 64, 512
    x = _u(rows, E, seed=41) * (1.0 + torch.arange(rows).float().unsqueeze(1) % 3)
    if probe == "mixed":
        x, _ = _mixed(x, 42)
    gm, bt = _u(E, seed=43) * 0.1 + 1, _u(E, seed=44) * 0.1
    ref, A = R.ln_fwd(x, gm, bt)[:2]
    bad = R.ln_fwd(x, gm, bt, rstd_shift=1)[0]
    assert R.ratio(bad, ref, R.gamma_ln(E) * A) >= FACTOR
    # LayerNorm output is scale-free: the mixed probe does not hide a wrong rstd from the normwise check either
    assert not R.old_close_passes(bad, ref)


def test_mixed_scale_probe_shows_the_gap():
    """one dropped K step on 2^-16-scaled rows: invisible to the normwise check, >= 30x over the elementwise bound"""
    x, w, ref, bound, rows = _gemm_case("mixed")
    bad = ref.clone()
    bad[rows] -= x[rows, 0:4] @ w[:, 0:4].t()
    assert R.old_close_passes(bad, ref) and R.ratio(bad, ref, bound) >= FACTOR
