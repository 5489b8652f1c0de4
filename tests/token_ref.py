"""Float64 reference for the couplers' token path (a helper module for the tests, not a test file): the extended GEMM
(cwf_gemm_ex), one-launch attention, paired LayerNorm, GELU backward with dropout, and the round-2 token kernels.  Everything
is written from the formulas in float64 and runs on whatever device its inputs live on.  Dropout masks are the counter
generator's (oracle.kernel_emul.EmulBackend.keep), scaled by the kernel's fp32 1.f / (1.f - p).

Error model: |got - ref| <= gamma * A elementwise, u = 2^-24 (fp32 unit roundoff).  A is the float64 magnitude of the same
computation with every operand replaced by its absolute value (plus the terms named below); gamma counts the fp32 roundings a
term can meet on its way to the output.  A sum of n terms accumulated in fp32, in any order, is within (n - 1) u sum |term|
(first order); a tree over 64 lanes adds 6.

Which kernel rounds what (read from csrc/gemm.hip, csrc/attn.hip, csrc/tokens.hip)
  gemm_mfma_kernel / gemm_mfma_v_kernel: v_mfma_f32_16x16x4_f32 accumulates four exact-or-rounded products per K step of 4 into
      an fp32 accumulator, ceil(K / 4) steps: at most ceil(K/4) + 4 roundings per product term.  Epilogue per element:
      v = acc * alpha + bias (2 roundings), C2 = v, GELU 0.5 v (1 + erff(v / sqrt 2)) (erff within 2 ulp; |gelu'| <= 1.13, the
      product chain 3 roundings of |v|), * keep (1 rounding), + residual (1), + C_old (1).  The rowsum is one more MFMA column
      against ones: the row sum of the (dropped) A operand, ceil(K/4) + 4 roundings, + the old value when rowsum_acc.
      gamma_gemm(K) = (ceil(K/4) + 4 + 12) u with A = s (|alpha| sum_k |a||b| + |bias|) (1.13 if GELU) + |residual| + |C_old|
      (s = the keep scale); 516-deep contractions give 149 u.  Epilogue alone, from the kernel's own C2: GAMMA_EPI = 8 u with
      A = s |pre| (1.13 if GELU) + |residual| + |C_old|.  rowsum: gamma_gemm(K) with A = sum_k |a| + |old|.
  attn_fwd_kernel: S = scale q.k (16 MFMA steps: 20 u of scale sum |q||k|; scale = 2^-3 exact); x = S - max S enters expf twice:
      42 u M_x, M_x = scale max_y sum_d |q_xd||k_yd|, plus u |x| <= 2 u M_x; expf 1 ulp (2 u); the 64-lane sum of <= 3 terms per
      lane 8 u; 1.f / sum and the product 2 u: rel(p) <= 2 (44 M + 2) u + 10 u <= (88 M + 14) u.  O = P V over 36 MFMA steps (40 u)
      and the keep product (u): |dO| <= (88 M + 55) u sum_y p m |v| -> GAMMA_ATTN = 144 u with A_o = sum_y p_xy m_xy |v_yd| (1 + M_x).
  attn_bwd_kernel: P recomputed as above (rho = (88 M + 14) u); dP = dO.V (20 u of W_xy = m_xy sum_d |dO_xd||v_yd|), g = dP m (u),
      dot = sum g p (rho + 9 u relative to sum p W, + 20 u for dP), dS = p (g - dot) scale: rho p |g - dot| + p (|dg| + |ddot|)
      + 3 u.  With W >= |g|:  |ddS| <= (2 rho + 56 u) p (W + sum p W) scale <= 176 u (1 + M) p (W + sum p W) scale = GAMMA_DS A_dS.
      dQ = dS K (36 steps, 40 u), dK = dS^T Q (ceil(T/4) <= 36 steps, 40 u), dV = Pm^T dO (rho + 42 u):
      GAMMA_ATTN_BWD = 216 u with A_dq = sum_y A_dS |k|, A_dk = sum_x A_dS |q|, A_dv = sum_x p m |dO| (1 + M_x).
  ln_pair_fwd_kernel (one wave per row, PER = E / 64 values per lane): mean = wave_sum / E ((PER + 6) u of mean|x|, E a power
      of two), var = wave_sum((v - mu)^2) / E, rstd = rsqrtf(var + eps) (1 ulp).  The mean error d_mu <= (PER + 6) u mean|x|
      shifts every v - mu; it reaches y through rstd, so rows with |mean| >> std lose (PER + 6) u mean|x| rstd absolutely:
      A_y = |gamma| (1 + |xhat|) (1 + mean|x| rstd) + |beta|, GAMMA_LN(PER) = (2 PER + 24) u; stats: |d mu| <= GAMMA_LN mean|x|,
      |d rstd| <= GAMMA_LN rstd (1 + mean|x| rstd).
  ln_pair_bwd_kernel (from the given fp32 stats, which are inputs here): h = (v - mu) rs, g = d gamma, s1 = mean g,
      s2 = mean g h, o = dy + rs (g - s1 - h s2) per LayerNorm term: A_dx = |dy| + sum_terms rs (|g| + mean|g| + |h| mean|g h|),
      GAMMA_LN(PER).
  ln_pair_params_kernel: 16 row lanes each sum rows / 16 terms of d (x - mu) rs, then 16 partials in order, + the old value:
      gamma_params(rows) = (ceil(rows / 16) + 20) u with A = sum |d| |xhat| (+ |old|), and sum |d| (+ |old|) for dbeta.
  gelu_bwd_drop_kernel: dh (cdf + v pdf) keep: cdf = 0.5 (1 + erff) carries an absolute error of a few u however small cdf is
      (the 1 + erff cancellation), expf 1 ulp: GAMMA_GELU = 8 u with A = s |dh| (1 + |v pdf(v)|).
  token_scores2(_g)_kernel: a lane adds E / 256 float4 dot products (4 products each), then the wave tree:
      gamma_score(E) = (E / 64 + 8) u with A = sum |f||q|.
  topk_inv / index_inv: integer outputs, exact: the reference is a float64 stable descending sort of the kernel's own fp32
      scores with NaN largest (above +inf); +0.0 and -0.0 tie.
  gather_multi, scatter_inv, token_grad, scatter_bwd's rows, head_grad(_g): one fp32 rounding per step in a fixed order: emulated
      bit for bit.  Where a product feeds an addition (d * gate + dscat, dseq * keep + ...) the compiler may contract the pair
      into one fma; either rounding is accepted, elementwise, and nothing else.
  scatter_bwd's dgate: 16 row lanes of ceil(T / 16) products, 16 partials in order, + dgate_extra:
      gamma_dgate(T) = (ceil(T / 16) + 20) u with A = sum_t |d||scat| + |extra|.
Each gamma grows with the length of the fp32 sum it covers.  At the shapes the suite runs none exceeds 2^-16 = 256 u except
two, where the kernel's own sum is that long: the dkv data gradient contracts over K = 1024 (gamma_gemm = 272 u) and scatter_bwd's
dgate sums T = 4800 tokens (gamma_dgate = 320 u).
"""
from __future__ import annotations

import math

import numpy as np
import torch

U = 2.0 ** -24
GELU_D_MAX = 1.13                       # max |gelu'(v)| = 1.1289...
GAMMA_EPI = 8 * U
GAMMA_ATTN = 144 * U
GAMMA_DS = 176 * U
GAMMA_ATTN_BWD = 216 * U
GAMMA_GELU = 8 * U


def gamma_gemm(K):
    return (-(-K // 4) + 16) * U


def gamma_ln(E):
    return (2 * (E // 64) + 24) * U


def gamma_params(rows):
    return (-(-rows // 16) + 20) * U


def gamma_score(E):
    return (E / 64 + 8) * U


def gamma_dgate(T):
    return (-(-T // 16) + 20) * U


# ------------------------------------------------------------------ dropout (the counter generator, bit-exact with cwf_keep)
def keep_at(emul, off, n, p, p2, idx):
    """fp32 keep factor keep(off, i, n, p, p2) at the integer element indices idx (any shape, 0 <= idx < n), as float64"""
    idx = torch.as_tensor(idx)
    if p <= 0.0:
        return torch.ones(idx.shape, dtype=torch.float64, device=idx.device)
    assert int(idx.min()) >= 0 and int(idx.max()) < n, "mask index outside the declared extent"
    return emul.keep(off, n, p, p2).double().to(idx.device)[idx.long()]


def keep_scale(p, p2=0.0):
    s = 1.0 if p <= 0.0 else float(np.float32(1.0) / (np.float32(1.0) - np.float32(p)))
    return s * (1.0 if p2 <= 0.0 else float(np.float32(1.0) / (np.float32(1.0) - np.float32(p2))))


# ------------------------------------------------------------------ GEMM
def _view(buf, off, sizes, strides):
    """flat element indices of a strided view: element (i, j, ...) at off + sum idx * stride (strides may be 0 or overlap)"""
    idx = torch.full(sizes, int(off), dtype=torch.int64, device=buf.device)
    for d, (n, s) in enumerate(zip(sizes, strides)):
        shape = [1] * len(sizes)
        shape[d] = n
        idx = idx + torch.arange(n, device=buf.device).reshape(shape) * int(s)
    return idx


def gemm_ex(g, emul=None):
    """The full struct cwf_gemm_args semantics in float64.  g: dict with the struct's fields, pointers given as (flat fp32 tensor,
    element offset) pairs (None = NULL) and the tab entries as lists of such pairs.  Returns a dict:
      'C'      : {buffer id: (flat float64 new contents, flat float64 A, flat bool written)} for every output buffer
      'C2'     : (flat float64, flat A, flat bool written) of the pre-activation buffer, if any
      'rowsum' : {buffer id: (flat float64, flat A, flat written)}
      'pre'    : [z] float64 [M, N] pre-activation (acc * alpha + bias) per z
      'z'      : [z] the epilogue's inputs per z (output indices, keep factors and scale, residual, old C) for gemm_epilogue
    The output buffers' other elements keep their old contents (the caller checks them bit for bit)."""
    M, N, K, ZB, ZH = g["M"], g["N"], g["K"], g["ZB"], g.get("ZH", 1)
    alpha = float(g.get("alpha", 1.0))
    act, accumulate = g.get("act", 0), g.get("accumulate", 0)
    a_p, a_p2 = g.get("a_drop_p", 0.0), g.get("a_drop_p2", 0.0)
    c_p, c_p2 = g.get("c_drop_p", 0.0), g.get("c_drop_p2", 0.0)
    tab = lambda name: g.get(name) or []
    m_idx = torch.arange(M)
    out_C, out_R, pres, zinfo = {}, {}, [], []
    C2 = None
    if g.get("C2") is not None:
        buf, _ = g["C2"]
        C2 = [buf.double().clone(), torch.zeros(buf.numel(), dtype=torch.float64, device=buf.device),
              torch.zeros(buf.numel(), dtype=torch.bool, device=buf.device)]
    for z in range(ZB * ZH):
        zb, zh = z // ZH, z % ZH
        # A: columns n >= split_n read A2 (the switch is per output column tile; split_n is a multiple of 64)
        a_zoff = zb * g.get("sa_zb", 0) + zh * g.get("sa_zh", 0)
        abuf, aoff = g["A"]
        dev = abuf.device
        a_idx = _view(abuf, a_zoff, (M, K), (g["sa_m"], g["sa_k"])).to(dev)
        Aop = abuf.double()[a_idx + aoff]
        A2op = None
        if g.get("A2") is not None:
            a2buf, a2off = g["A2"]
            A2op = a2buf.double()[a_idx + a2off]
        if a_p > 0.0:
            kp = keep_at(emul, g["a_drop_off"], g["a_drop_n"], a_p, a_p2, a_idx)
            Aop = Aop * kp
            if A2op is not None:
                A2op = A2op * kp
        # B: B_tab[z] (no z offset) or B + z offsets; rows m >= split_m read B2 + z offsets
        if tab("B_tab"):
            bbuf, boff = g["B_tab"][z]
            b_zoff = 0
        else:
            bbuf, boff = g["B"]
            b_zoff = zb * g.get("sb_zb", 0) + zh * g.get("sb_zh", 0)
        b_idx = _view(bbuf, b_zoff, (K, N), (g["sb_k"], g["sb_n"])).to(dev)
        Bop = bbuf.double()[b_idx + boff]
        acc = torch.empty(M, N, dtype=torch.float64, device=dev)
        accA = torch.empty_like(acc)
        split_n = g.get("split_n", 0) if A2op is not None else N
        split_m = g.get("split_m", 0) if g.get("B2") is not None else M
        split_n, split_m = min(split_n, N), min(split_m, M)
        for (m0, m1) in ((0, split_m), (split_m, M)):
            if m1 <= m0:
                continue
            if m0 == 0:
                Bm = Bop
            else:
                b2buf, b2off = g["B2"]
                Bm = b2buf.double()[_view(b2buf, zb * g.get("sb_zb", 0) + zh * g.get("sb_zh", 0), (K, N), (g["sb_k"], g["sb_n"])).to(dev) + b2off]
            for (n0, n1, Am) in ((0, split_n, Aop), (split_n, N, A2op)):
                if n1 <= n0:
                    continue
                acc[m0:m1, n0:n1] = Am[m0:m1] @ Bm[:, n0:n1]
                accA[m0:m1, n0:n1] = Am[m0:m1].abs() @ Bm[:, n0:n1].abs()
        bias = None
        if tab("bias_tab"):
            bb, bo = g["bias_tab"][z]
            bias = bb.double()[bo:bo + N]
        elif g.get("bias") is not None:
            bb, bo = g["bias"]
            bias = bb.double()[bo:bo + N]
        pre = acc * alpha + (bias if bias is not None else 0.0)
        preA = accA * abs(alpha) + (bias.abs() if bias is not None else 0.0)
        pres.append(pre)
        c_zoff = zb * g.get("sc_zb", 0) + zh * g.get("sc_zh", 0)
        c_rel = _view(acc, c_zoff, (M, N), (g["sc_m"], 1))     # C + z offsets: the element offset the mask and C2 are keyed on
        if tab("C_tab"):                                        # C_tab[z] carries no z offset
            cbuf, coff = g["C_tab"][z]
            c_idx = c_rel - c_zoff + coff
        else:
            cbuf, coff = g["C"]
            c_idx = c_rel + coff
        if C2 is not None:
            C2[0][c_rel + g["C2"][1]] = pre
            C2[1][c_rel + g["C2"][1]] = preA
            C2[2][c_rel + g["C2"][1]] = True
        v = gelu(pre) if act == 1 else pre
        s, keep, resid = 1.0, None, None
        if c_p > 0.0:
            keep = keep_at(emul, g["c_drop_off"], g["c_drop_n"], c_p, c_p2, c_rel)
            v = v * keep
            s = keep_scale(c_p, c_p2)
        Amag = s * preA * (GELU_D_MAX if act == 1 else 1.0)
        if g.get("residual") is not None:
            rbuf, roff = g["residual"]
            r_idx = _view(rbuf, zb * g.get("sr_zb", 0) + zh * g.get("sr_zh", 0), (M, N), (g["sr_m"], 1)).to(dev) + roff
            resid = rbuf.double()[r_idx]
            v = v + resid
            Amag = Amag + resid.abs()
        key = id(cbuf)
        if key not in out_C:
            out_C[key] = [cbuf.double().clone(), torch.zeros(cbuf.numel(), dtype=torch.float64, device=dev),
                          torch.zeros(cbuf.numel(), dtype=torch.bool, device=dev)]
        old = out_C[key][0][c_idx]
        if accumulate:
            v = v + old
            Amag = Amag + old.abs()
        zinfo.append(dict(C=key, c_idx=c_idx, c2_idx=(c_rel + g["C2"][1]) if C2 is not None else None, keep=keep, scale=s,
                          residual=resid, old=old if accumulate else None))
        out_C[key][0][c_idx] = v
        out_C[key][1][c_idx] = Amag
        out_C[key][2][c_idx] = True
        # rowsum: the row sums of the (dropped) operand of column tile 0
        rs_buf = None
        if tab("rowsum_tab"):
            rs_buf = g["rowsum_tab"][z]
        elif g.get("rowsum") is not None:
            rs_buf = g["rowsum"]
        if rs_buf is not None:
            rbuf, roff = rs_buf
            A0 = A2op if (A2op is not None and g.get("split_n", 0) <= 0) else Aop
            rkey = id(rbuf)
            if rkey not in out_R:
                out_R[rkey] = [rbuf.double().clone(), torch.zeros(rbuf.numel(), dtype=torch.float64, device=dev),
                               torch.zeros(rbuf.numel(), dtype=torch.bool, device=dev)]
            oldr = out_R[rkey][0][roff:roff + M].clone()
            rsum, rA = A0.sum(1), A0.abs().sum(1)
            if g.get("rowsum_acc", 0):
                rsum, rA = rsum + oldr, rA + oldr.abs()
            out_R[rkey][0][roff:roff + M] = rsum
            out_R[rkey][1][roff:roff + M] = rA
            out_R[rkey][2][roff:roff + M] = True
    return {"C": out_C, "C2": C2, "rowsum": out_R, "pre": pres, "z": zinfo}


def gemm_epilogue(pre, act, keep=None, scale=1.0, residual=None, old=None):
    """(ref, A) of the epilogue alone from a given pre-activation (the kernel's own C2): drop(act(pre)) + residual (+ old)"""
    pre = pre.double()
    v = gelu(pre) if act == 1 else pre
    A = scale * pre.abs() * (GELU_D_MAX if act == 1 else 1.0)
    if keep is not None:
        v = v * keep
    if residual is not None:
        v, A = v + residual.double(), A + residual.double().abs()
    if old is not None:
        v, A = v + old.double(), A + old.double().abs()
    return v, A


def gelu(v):
    return 0.5 * v * (1.0 + torch.erf(v / math.sqrt(2.0)))


def gelu_grad(v):
    return 0.5 * (1.0 + torch.erf(v / math.sqrt(2.0))) + v * torch.exp(-0.5 * v * v) / math.sqrt(2.0 * math.pi)


def gelu_bwd_drop(z, dh, keep=None, scale=1.0):
    """(ref, A): dh * gelu'(z) * keep"""
    z, dh = z.double(), dh.double()
    pdf = torch.exp(-0.5 * z * z) / math.sqrt(2.0 * math.pi)
    r = dh * gelu_grad(z)
    if keep is not None:
        r = r * keep
    return r, scale * dh.abs() * (1.0 + (z * pdf).abs())


# ------------------------------------------------------------------ attention
ATTN_D = 64


def attn_mask(emul, Z, T, heads, off, p):
    """[Z, heads, T, T] float64 keep factors of the attention dropout: counter off + ((z heads + h) T + t) T + key"""
    if p <= 0.0:
        return None
    n = Z * heads * T * T
    return emul.keep(off, n, p).double().reshape(Z, heads, T, T)


def _split(qkv, Z, T, heads):
    E = heads * ATTN_D
    x = qkv.double()[:, :3 * E].reshape(Z, T, 3, heads, ATTN_D).permute(2, 0, 3, 1, 4)   # [3, Z, H, T, D]
    return x[0], x[1], x[2]


def _merge(t):
    Z, H, T, D = t.shape
    return t.permute(0, 2, 1, 3).reshape(Z * T, H * D)


def attn_probs(q, k, scale, drop_last_key=False):
    s = scale * q @ k.transpose(-1, -2)
    e = torch.exp(s - s.amax(-1, keepdim=True))
    den = e.sum(-1, keepdim=True) if not drop_last_key else e[..., :-1].sum(-1, keepdim=True)
    M = scale * (q.abs() @ k.abs().transpose(-1, -2)).amax(-1, keepdim=True)
    return e / den, M


def attn_fwd(qkv, Z, T, heads, mask=None, scale=ATTN_D ** -0.5, drop_last_key=False):
    """(o [Z T, E], A_o) from qkv [Z T, >= 3E]: o = (softmax(scale q k^T) * mask) v"""
    q, k, v = _split(qkv, Z, T, heads)
    p, M = attn_probs(q, k, scale, drop_last_key)
    pm = p if mask is None else p * mask.to(p.device)
    o = pm @ v
    A = (pm @ v.abs()) * (1.0 + M)
    return _merge(o), _merge(A)


def attn_bwd(qkv, d_o, Z, T, heads, mask=None, scale=ATTN_D ** -0.5):
    """((dq, dk, dv) each [Z T, E], (A_dq, A_dk, A_dv)) for o = (softmax(scale q k^T) * mask) v"""
    q, k, v = _split(qkv, Z, T, heads)
    E = heads * ATTN_D
    dO = d_o.double()[:, :E].reshape(Z, T, heads, ATTN_D).permute(0, 2, 1, 3)
    p, M = attn_probs(q, k, scale)
    m = torch.ones_like(p) if mask is None else mask.to(p.device)
    dP = dO @ v.transpose(-1, -2)
    g = dP * m
    dot = (g * p).sum(-1, keepdim=True)
    dS = p * (g - dot) * scale
    W = m * (dO.abs() @ v.abs().transpose(-1, -2))
    AdS = scale * p * (W + (p * W).sum(-1, keepdim=True)) * (1.0 + M)
    dq, dk, dv = dS @ k, dS.transpose(-1, -2) @ q, (p * m).transpose(-1, -2) @ dO
    Adq = (GAMMA_DS / GAMMA_ATTN_BWD) * (AdS @ k.abs()) + (dS.abs() @ k.abs())
    Adk = (GAMMA_DS / GAMMA_ATTN_BWD) * (AdS.transpose(-1, -2) @ q.abs()) + (dS.abs().transpose(-1, -2) @ q.abs())
    Adv = ((p * m) * (1.0 + M)).transpose(-1, -2) @ dO.abs()
    return tuple(_merge(t) for t in (dq, dk, dv)), tuple(_merge(t) for t in (Adq, Adk, Adv))


# ------------------------------------------------------------------ LayerNorm
def ln_perm(rows, perm_T):
    r = torch.arange(rows)
    if perm_T <= 0:
        return r
    return ((r // perm_T) ^ 1) * perm_T + r % perm_T


def ln_fwd(x, gamma, beta, eps=1e-5, rstd_shift=0):
    """(y, A_y, mean, rstd, A_mean, A_rstd) of one LayerNorm over the rows of x; gamma / beta [rows, E] (per-row parameter sets)
    or [E].  rstd_shift != 0: row r uses row r + shift's rstd (a planted defect only)."""
    x = x.double()
    mu = x.mean(1, keepdim=True)
    var = ((x - mu) ** 2).mean(1, keepdim=True)
    rs = 1.0 / torch.sqrt(var + eps)
    rs_used = torch.roll(rs, -rstd_shift, 0) if rstd_shift else rs
    xh = (x - mu) * rs_used
    g, b = gamma.double(), beta.double()
    y = xh * g + b
    ax = x.abs().mean(1, keepdim=True)
    A = g.abs() * (1.0 + xh.abs()) * (1.0 + ax * rs) + b.abs()
    return y, A, mu.squeeze(1), rs.squeeze(1), ax.squeeze(1), (rs * (1.0 + ax * rs)).squeeze(1)


def ln_bwd_term(d, x, gamma, mu, rs):
    """(dx, A) of one LayerNorm backward from the given (fp32) stats: rs (g - mean g - h mean(g h)), g = d gamma"""
    d, x, gm = d.double(), x.double(), gamma.double()
    mu, rs = mu.double().unsqueeze(1), rs.double().unsqueeze(1)
    h = (x - mu) * rs
    g = d * gm
    s1, s2 = g.mean(1, keepdim=True), (g * h).mean(1, keepdim=True)
    o = rs * (g - s1 - h * s2)
    A = rs * (g.abs() + g.abs().mean(1, keepdim=True) + h.abs() * (g * h).abs().mean(1, keepdim=True))
    return o, A


def ln_params(d, x, mu, rs, groups):
    """per-group (dgamma, A_dgamma, dbeta, A_dbeta) [G, E]: column sums over each group's rows of d xhat and d"""
    d, x = d.double(), x.double()
    h = (x - mu.double().unsqueeze(1)) * rs.double().unsqueeze(1)
    G = groups
    dg, db = (d * h).reshape(G, -1, d.shape[1]).sum(1), d.reshape(G, -1, d.shape[1]).sum(1)
    Ag, Ab = (d * h).abs().reshape(G, -1, d.shape[1]).sum(1), d.abs().reshape(G, -1, d.shape[1]).sum(1)
    return dg, Ag, db, Ab


# ------------------------------------------------------------------ token kernels
def scores(feats, q):
    """(score, A) [B, T]: feats [B, T, E] . q [B|1, E]"""
    f, q = feats.double(), q.double().reshape(-1, 1, feats.shape[2])
    return (f * q).sum(-1), (f.abs() * q.abs()).sum(-1)


def topk_inv(score, k):
    """(index [B, k], inv [B, T]) int32: a stable float64 descending sort of the given fp32 scores, NaN above +inf"""
    s = score.double()
    nan = torch.isnan(s)
    key = torch.where(nan, torch.zeros_like(s), s)
    # stable descending sort on (is_nan, value): sort by value first, then stably by the NaN flag
    o1 = torch.sort(key, dim=1, descending=True, stable=True).indices
    o2 = torch.sort(nan.gather(1, o1).to(torch.int8), dim=1, descending=True, stable=True).indices
    order = o1.gather(1, o2)
    B, T = s.shape
    inv = torch.full((B, T), -1, dtype=torch.int32, device=s.device)
    inv.scatter_(1, order[:, :k], torch.arange(k, dtype=torch.int32, device=s.device).expand(B, k).contiguous())
    return order[:, :k].to(torch.int32), inv


def index_inv(index, T):
    B, k = index.shape
    inv = torch.full((B, T), -1, dtype=torch.int32, device=index.device)
    ok = (index >= 0) & (index < T)
    for b in range(B):
        j = torch.arange(k, device=index.device)[ok[b]]
        inv[b, index[b, ok[b]].long()] = j.to(torch.int32)
    return inv


def gather_job(feats, index, head, k, pe_odd, keep):
    """[B, k + 1, E] fp32, bit for bit: row 0 = head, row 1 + j = (feats[b][clamp(index[j])] + pe on odd e) * keep"""
    B, T, E = feats.shape
    t = index.long().clamp(0, T - 1)
    rows = feats.gather(1, t.unsqueeze(-1).expand(B, k, E)).clone()
    rows[..., 1::2] = rows[..., 1::2] + np.float32(pe_odd)
    if keep is not None:
        rows = rows * keep.float()
    return torch.cat([head.float().expand(B, 1, E), rows], 1)


def fp32_mul_add(d, g, s):
    """the two fp32 results a * b + c can have: two roundings, or one (a contracted fma)"""
    two = (d.float() * g.float()) + s.float()
    one = (d.double() * g.double() + s.double()).float()
    return two, one


def head_grad(a, c, groups=1):
    """out[g][e] = sum_b in group (a[b][e] + c[b][e]), fp32 in the kernel's order, bit for bit"""
    B = a.shape[0]
    gb = B // groups
    outs = []
    for gi in range(groups):
        s = torch.zeros_like(a[0]).float()
        for b in range(gi * gb, (gi + 1) * gb):
            s = s + (a[b].float() + c[b].float())
        outs.append(s)
    return outs


# ------------------------------------------------------------------ the check
def worst(got, ref, bound, what, limit=1.0):
    """max |got - ref| / bound (where the bound is 0, got must equal ref); asserts <= limit and returns it"""
    got = got.detach().cpu().double()
    ref, bound = ref.detach().cpu().double(), bound.detach().cpu().double()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert bool(torch.isfinite(got).all()), (what, "non-finite output")
    err = (got - ref).abs()
    zero = bound == 0
    assert not bool((zero & (err > 0)).any()), (what, "differs where the reference is exact")
    r = torch.where(zero, torch.zeros_like(err), err / bound.clamp_min(1e-300))
    w = float(r.max()) if r.numel() else 0.0
    if w > limit:
        idx = tuple(int(i) for i in np.unravel_index(int(r.argmax()), r.shape))
        raise AssertionError("%s: worst err/bound = %.3g at %s: got %r ref %r bound %r" % (
            what, w, idx, float(got[idx]), float(ref[idx]), float(bound[idx])))
    return w


def ratio(got, ref, bound):
    """worst err/bound without asserting (the planted-defect tests)"""
    got, ref, bound = got.detach().cpu().double(), ref.detach().cpu().double(), bound.detach().cpu().double()
    return float(((got - ref).abs() / bound.clamp_min(1e-300)).max())


def old_close_passes(got, ref, rtol=2e-5):
    """the suite's earlier normwise check (tests/test_coupler_gpu.py: close): |got - ref| <= 2 rtol max|ref|"""
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    return float((got - ref).abs().max()) <= 2 * rtol * float(ref.abs().max() + 1e-30)
