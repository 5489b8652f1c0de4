"""Float64 autograd reference for the coupler Functions of cwf/coupler.py (a helper module for the tests, not a test file).

Every Function (RegionCouplerFn, FusionCouplerFn, IntraCouplerBlockFn, FusionBlockFn, the coupler section of ClsWiseFormer.encode and
the small adjoints) is restated here as a plain differentiable torch forward; every gradient of the reference comes from torch
autograd, none from a hand-written adjoint.

  dropout off   the committed restatements of oracle/reference_model.py are composed: select_tokens with a forced index,
                intra_region_coupler, cross_region_coupler, scatter_rows, convert_dim, split_dim;
  dropout on    the same graph written out with an explicit keep factor at every site (test_coupler_ref_cpu.py holds the written-out
                graph with all factors 1 against the composition above).  A factor is EmulBackend.keep(off, n, p, p2) in the layouts
                tests/token_ref.py documents: selection rows [G B, k, E] after the positional row is added, attention
                [Z, heads, T, T], GEMM epilogues row-major over rows x N with p2 on the second counter stream.

Site offsets are not read out of coupler.py: the run under test records the (offset, n) pair of every K.rng_site call and the
reference consumes them in its own stated order (Sites): per coupler call the selection sites in gather_multi's job order (edge,
sem, sem_supp, edge_supp), then per cross-attention block the attention site and -- whenever p_attn > 0 or p_pre > 0 -- the output
site, then the two FFN sites.  Each recorded n must be the extent the reference expects, the list must be used up, and no two sites'
counter ranges [off, off + 2n) may overlap.

Selections are teacher-forced on the reference with the index sets the run under test returned, in their order; separately every
returned set must equal, as a set, the float64 top-k of the reference's own scores, and the inputs must leave a gap between the
k-th and (k+1)-th score of more than 2 gamma_score(E) A (token_ref) in EVERY row (A: the largest sum |f||q| of the row), so that no
fp32 realisation of the score may legitimately pick another set.

Three runs per case: float64 (truth), float32 of the same statement with the same indices and masks (the yardstick e32) and the
run under test.  Bound, per tensor (rule R0 of test_block_graph_gpu.py): relative L2 <= 16 e32 and max |err| <= 16 x the float32
run's max |err|; a reference tensor that is exactly zero must come back exactly zero, and so must every element that is exactly
zero in both reference runs (rows nothing flows into, dropped elements).
"""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F

import token_ref as TR
from oracle import reference_model as rm

E_DIM, HEADS = 512, 8
FACTOR = 16.0
WN = ("ln1.w", "ln1.b", "ln2.w", "ln2.b", "out.w", "out.b", "qkv.w", "ffn.ln.w", "ffn.ln.b", "w1", "b1", "w2", "b2")
SEL = ("edge", "sem_supp", "sem", "edge_supp")
_KEYS = ("cross_attention_list.0.fn.norm.weight", "cross_attention_list.0.fn.norm.bias", "cross_attention_list.0.fn.norm2.weight",
         "cross_attention_list.0.fn.norm2.bias", "cross_attention_list.0.fn.fn.out_proj.weight", "cross_attention_list.0.fn.fn.out_proj.bias",
         "cross_attention_list.0.fn.fn.qkv.weight", "cross_ffn_list.0.fn.norm.weight", "cross_ffn_list.0.fn.norm.bias",
         "cross_ffn_list.0.fn.fn.net.0.weight", "cross_ffn_list.0.fn.fn.net.0.bias", "cross_ffn_list.0.fn.fn.net.3.weight",
         "cross_ffn_list.0.fn.fn.net.3.bias")


class Rates:
    def __init__(self, sel=0.0, attn=0.0, pre=0.0, ffn=0.0):
        self.sel, self.attn, self.pre, self.ffn = sel, attn, pre, ffn

    @property
    def off(self):
        return not (self.sel or self.attn or self.pre or self.ffn)


#          route: (rates, sink, frozen weight, forced group)
ROUTES = {
    "C0": (Rates(), False, False, False),
    "C1": (Rates(0.1, 0.1, 0.1, 0.1), False, False, False),
    "C1a": (Rates(0.0, 0.0, 0.1, 0.1), False, False, False),
    "C1b": (Rates(0.1, 0.1, 0.0, 0.0), False, False, False),
    "C2": (Rates(0.1, 0.1, 0.1, 0.1), True, False, False),
    "C3": (Rates(0.1, 0.1, 0.1, 0.1), True, True, False),
    "C4": (Rates(), False, False, True),
}


# ====================================================================================================================
# dropout sites
# ====================================================================================================================
def check_disjoint(rec):
    """no two recorded sites' counter ranges [off, off + 2n) overlap"""
    end = -1
    for off, n in sorted(rec):
        assert off >= end, ("dropout sites share counters", rec)
        end = off + 2 * n


class Sites:
    """The recorded (offset, n) pairs of one run, consumed in the reference's order; `emul` evaluates the counter generator at the
    run's {seed, step}.  ones=True: every factor is 1 (the written-out graph against the composition of reference_model)."""

    def __init__(self, rec=(), emul=None, ones=False):
        self.rec, self.emul, self.ones, self.i = list(rec), emul, ones, 0

    def take(self, shape, p, p2, like):
        if self.ones:
            return torch.ones(shape, dtype=like.dtype)
        n = int(math.prod(shape))
        assert self.i < len(self.rec), "the run under test drew fewer dropout sites than the reference consumes"
        off, got = self.rec[self.i]
        self.i += 1
        assert got == n, ("site %d has extent %d, the reference expects %d" % (self.i - 1, got, n))
        return self.emul.keep(off, n, p, p2).to(like.dtype).reshape(shape)

    def done(self):
        assert self.ones or self.i == len(self.rec), ("dropout sites left over", self.i, len(self.rec))


# ====================================================================================================================
# the written-out graph (explicit keep factors); x: [G, Z, t, E], Ws: G weight sets of 13 tensors
# ====================================================================================================================
def _ln(x, w, b):
    return F.layer_norm(x, (x.shape[-1],), w, b, rm.LN_EPS)


def ca_explicit(Ws, x, x2, rates, sites):
    """Residual(PreNormDrop(DualSelfAttention)) (reference_model.cross_attention) with attn_drop on the probabilities and the
    attention's output dropout followed by PreNormDrop's on the out_proj result"""
    G, Z, t, e = x.shape
    hd = e // HEADS
    m_att = sites.take((G, Z, HEADS, t, t), rates.attn, 0.0, x) if rates.attn > 0 else None
    m_out = None
    if rates.attn > 0 or rates.pre > 0:
        p, p2 = (rates.attn, rates.pre) if rates.attn > 0 else (rates.pre, 0.0)
        m_out = sites.take((G, Z, t, e), p, p2, x)
    ys = []
    for g, W in enumerate(Ws):
        a, b = _ln(x[g], W[0], W[1]), _ln(x2[g], W[2], W[3])
        q = F.linear(a, W[6][:e]).reshape(Z, t, HEADS, hd).permute(0, 2, 1, 3)
        k = F.linear(b, W[6][e:2 * e]).reshape(Z, t, HEADS, hd).permute(0, 2, 1, 3)
        v = F.linear(b, W[6][2 * e:]).reshape(Z, t, HEADS, hd).permute(0, 2, 1, 3)
        att = (torch.einsum("bhxd,bhyd->bhxy", q, k) * (hd ** -0.5)).softmax(dim=-1)
        if m_att is not None:
            att = att * m_att[g]
        o = torch.einsum("bhxy,bhyd->bhxd", att, v).permute(0, 2, 1, 3).reshape(Z, t, e)
        o = F.linear(o, W[4], W[5])
        if m_out is not None:
            o = o * m_out[g]
        ys.append(o + x[g])
    return torch.stack(ys, 0)


def ffn_explicit(Ws, x, rates, sites):
    G, Z, t, e = x.shape
    hid = Ws[0][9].shape[0]
    m1 = sites.take((G, Z, t, hid), rates.ffn, 0.0, x) if rates.ffn > 0 else None
    m2 = sites.take((G, Z, t, e), rates.ffn, 0.0, x) if rates.ffn > 0 else None
    ys = []
    for g, W in enumerate(Ws):
        h = F.gelu(F.linear(_ln(x[g], W[7], W[8]), W[9], W[10]))
        if m1 is not None:
            h = h * m1[g]
        h = F.linear(h, W[11], W[12])
        if m2 is not None:
            h = h * m2[g]
        ys.append(h + x[g])
    return torch.stack(ys, 0)


def _state(W):
    return {"T." + k: w for k, w in zip(_KEYS, W)}


def _rows(feats, index, keep):
    """(feats[index] + pe[0]) * keep: the selection rows; the class token in front of them is never dropped"""
    r = torch.gather(feats, 1, index[:, :, None].expand(-1, -1, feats.shape[2])) + rm.pe_row0(feats.shape[2]).to(feats)
    return r if keep is None else r * keep


def check_selection(feats, q, index, k, what, forced=None):
    """float64 only: the returned set equals the top-k of the reference's own scores, and the gap below the k-th score exceeds
    2 gamma_score(E) A in every row (k == T: the set is everything and there is nothing to flip)"""
    assert feats.dtype == torch.float64
    with torch.no_grad():
        if forced is not None:
            assert torch.equal(index, forced), (what, "a teacher-forced selection came back changed")
            return
        b, t, e = feats.shape
        score = torch.einsum("be,bne->bn", q.expand(b, -1, -1)[:, 0], feats)
        A = torch.einsum("be,bne->bn", q.expand(b, -1, -1)[:, 0].abs(), feats.abs()).amax(1)
        srt, order = torch.sort(score, dim=1, descending=True, stable=True)
        assert index.shape == (b, k) and all(len(set(r)) == k for r in index.tolist()), (what, "not k distinct rows")
        if k < t:
            gap = srt[:, k - 1] - srt[:, k]
            assert bool((gap > 2 * TR.gamma_score(e) * A).all()), (what, "a row's k-th / (k+1)-th score gap is within fp32 noise: change the seed",
                                                                   gap.tolist(), (2 * TR.gamma_score(e) * A).tolist())
        assert torch.equal(torch.sort(index, 1).values, torch.sort(order[:, :k], 1).values), (what, "not the float64 top-k set")


# ====================================================================================================================
# references of the Functions (dtype follows the inputs)
# ====================================================================================================================
def intra_ref(Ws, edge, sem_supp, sem, edge_supp, rates, sites):
    """[G, b, t, E] x 4 -> [G, b, 2, t, E] (result_edge ; result_sem); sites None = dropout off, reference_model's composition"""
    G, b, t, e = edge.shape
    if sites is None:
        assert rates.off
        return torch.stack([rm.intra_region_coupler(_state(W), "T", edge[g], sem_supp[g], sem[g], edge_supp[g]).reshape(b, 2, t, e)
                            for g, W in enumerate(Ws)], 0)
    X1 = torch.stack((edge, sem), 2).reshape(G, 2 * b, t, e)
    X2 = torch.stack((sem_supp, edge_supp), 2).reshape(G, 2 * b, t, e)
    y1 = ca_explicit(Ws, X1, X2, rates, sites)                                   # a = CA(edge, sem'), b = CA(sem, edge')
    y2 = ca_explicit(Ws, y1, y1.reshape(G, b, 2, t, e).flip(2).reshape(G, 2 * b, t, e), rates, sites)   # CA(a, b), CA(b, a)
    return ffn_explicit(Ws, y2, rates, sites).reshape(G, b, 2, t, e)


def fusion_block_ref(W, x, rates, sites):
    if sites is None:
        assert rates.off
        return rm.cross_region_coupler(_state(W), "T", x)
    y1 = ca_explicit([W], x[None], x[None], rates, sites)
    return ffn_explicit([W], y1, rates, sites)[0]


def region_ref(E, S, etoks, stoks, Ws, idx, k, rates, sites, forced=None):
    """E [G,b,Te,E], S [G,b,Ts,E], idx = (edge, sem_supp, sem, edge_supp) index sets [G b, k] int64
    -> gated_e, gated_s, scat_s, sem_tok"""
    G, b, te, e = E.shape
    I = [i.reshape(G, b, k) for i in idx]
    forced = forced or {}
    if E.dtype == torch.float64:
        for g in range(G):
            for j, (feats, q) in enumerate(((E[g], etoks[g]), (S[g], etoks[g]), (S[g], stoks[g]), (E[g], stoks[g]))):
                check_selection(feats.detach(), q.detach(), I[j][g], k, "group %d %s" % (g, SEL[j]), forced.get((g, j)))
    if sites is None:
        assert rates.off
        seqs = []
        for g in range(G):
            edge_seq, _ = rm.select_tokens(etoks[g], E[g], forced_index=I[0][g])
            sem_supp, _ = rm.select_tokens(etoks[g], S[g], forced_index=I[1][g])          # scored by e_tok, led by s_tok
            sem_supp = torch.cat((stoks[g].expand(b, -1, -1), sem_supp[:, 1:]), 1)
            sem_seq, _ = rm.select_tokens(stoks[g], S[g], forced_index=I[2][g])
            edge_supp, _ = rm.select_tokens(stoks[g], E[g], forced_index=I[3][g])         # scored by s_tok, led by e_tok
            edge_supp = torch.cat((etoks[g].expand(b, -1, -1), edge_supp[:, 1:]), 1)
            seqs.append((edge_seq, sem_supp, sem_seq, edge_supp))
    else:
        m = [sites.take((G, b, k, e), rates.sel, 0.0, E) if rates.sel > 0 else None for _ in range(4)]   # edge, sem, sem_supp, edge_supp
        pick = lambda mk, g: None if mk is None else mk[g]
        seqs = []
        for g in range(G):
            et, st = etoks[g].expand(b, -1, -1), stoks[g].expand(b, -1, -1)
            seqs.append((torch.cat((et, _rows(E[g], I[0][g], pick(m[0], g))), 1), torch.cat((st, _rows(S[g], I[1][g], pick(m[2], g))), 1),
                         torch.cat((st, _rows(S[g], I[2][g], pick(m[1], g))), 1), torch.cat((et, _rows(E[g], I[3][g], pick(m[3], g))), 1)))
    R = intra_ref(Ws, *[torch.stack([s[j] for s in seqs], 0) for j in range(4)], rates, sites)
    ge, gs, sc, tok = [], [], [], []
    for g in range(G):
        res_e, res_s = R[g, :, 0], R[g, :, 1]
        E2 = rm.scatter_rows(E[g], I[0][g], res_e[:, 1:])
        S2 = rm.scatter_rows(S[g], I[2][g], res_s[:, 1:])
        ge.append(res_e[:, 0:1] * E2); gs.append(res_s[:, 0:1] * S2); sc.append(S2); tok.append(res_s[:, 0:1])
    return torch.stack(ge, 0), torch.stack(gs, 0), torch.stack(sc, 0), torch.stack(tok, 0)


def fusion_ref(feats, tok, W, idx, k, rates, sites, forced=None):
    """feats [b,Ts,E], per-sample class token [b,1,E] -> fused (reference_model.forward's Mutual Cross-region Coupler)"""
    b, ts, e = feats.shape
    if feats.dtype == torch.float64:
        check_selection(feats.detach(), tok.detach(), idx, k, "fusion", forced)
    keep = sites.take((b, k, e), rates.sel, 0.0, feats) if (sites is not None and rates.sel > 0) else None
    seq = torch.cat((tok, _rows(feats, idx, keep)), 1)
    res = fusion_block_ref(W, seq, rates, sites)
    return res[:, 0:1] * rm.scatter_rows(feats, idx, res[:, 1:])


# ====================================================================================================================
# inputs
# ====================================================================================================================
def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed * 7919 + int(math.prod(shape)) % 9973)
    return (torch.rand(*shape, generator=g) * 2 - 1) * scale


def weights(seed):
    e = E_DIM
    shapes = [(e,), (e,), (e,), (e,), (e, e), (e,), (3 * e, e), (e,), (e,), (e, e), (e,), (e, e), (e,)]
    out = []
    for i, s in enumerate(shapes):
        w = rnd(*s, seed=seed + i) * (1.0 / math.sqrt(e) if len(s) == 2 else 0.1)
        if len(s) == 1 and i in (0, 2, 7):
            w = w + 1.0
        out.append(w)
    return out


def _wdict(prefix, seed):
    return {"%s.%s" % (prefix, n): w for n, w in zip(WN, weights(seed))}


def _wlist(L, prefix):
    return [L["%s.%s" % (prefix, n)] for n in WN]


class Case:
    """One graph: `leaves` name -> fp32 CPU tensor, `params` the names a GradSink holds, `fut(L, rates, forced)` the Functions
    under test on the leaves L -> (outputs, selections), `ref(L, sel, rates, sites)` the reference -> outputs, `used` the outputs
    the loss contracts (the others reach the Function as None), `frozen` the weight route C3 freezes, `forced(dev)` the
    teacher-forced sets of route C4."""

    def __init__(self, name, leaves, params, fut, ref, used, frozen=None, forced=None):
        self.name, self.leaves, self.params, self.fut, self.ref, self.used, self.frozen, self.forced = \
            name, leaves, params, fut, ref, used, frozen, forced

    def cotangent(self, name, shape):
        return rnd(*shape, seed=1000 + sum(map(ord, name)))


def _cfg(k, rates, forced=None, names=None, groups=1):
    from cwf import coupler as CP
    return CP.CouplerConfig(HEADS, k, True, rates.sel, rates.attn, rates.pre, rates.ffn, forced=forced, names=names, groups=groups)


def region_case(G, b, te, ts, kcfg, seed=0, used=("gated_e", "gated_s", "scat_s", "sem_tok")):
    from cwf import coupler as CP
    e = E_DIM
    k = min(kcfg, ts, te)
    leaves = {"E": rnd(G, b, te, e, seed=seed + 1), "S": rnd(G, b, ts, e, seed=seed + 2)}
    for g in range(G):
        leaves["e_tok%d" % g] = rnd(1, 1, e, seed=seed + 3 + g) * 0.05
        leaves["s_tok%d" % g] = rnd(1, 1, e, seed=seed + 13 + g) * 0.05
        leaves.update(_wdict("set%d" % g, seed + 100 + 50 * g))
    params = [n for n in leaves if n not in ("E", "S")]
    names = [tuple("r%d_%s" % (g, n) for n in SEL) for g in range(G)]

    def forced_sets():            # group 1 only: k distinct rows in an order no score would give
        out = {}
        for j, t in enumerate((te, ts, ts, te)):
            gen = torch.Generator().manual_seed(seed + 77 + j)
            out[(1, j)] = torch.stack([torch.randperm(t, generator=gen)[:k] for _ in range(b)], 0)
        return out

    def fut(L, rates, forced):
        fo = {names[g][j]: v.to(L["E"].device) for (g, j), v in (forced or {}).items()}
        flat = [L["e_tok%d" % g] for g in range(G)] + [L["s_tok%d" % g] for g in range(G)]
        for g in range(G):
            flat += _wlist(L, "set%d" % g)
        out = CP.RegionCouplerFn.apply(_cfg(kcfg, rates, fo, names, G), L["E"], L["S"], *flat)
        return dict(zip(("gated_e", "gated_s", "scat_s", "sem_tok"), out[:4])), [o.long().cpu() for o in out[4:]]

    def ref(L, sel, rates, sites, forced=None):
        out = region_ref(L["E"], L["S"], [L["e_tok%d" % g] for g in range(G)], [L["s_tok%d" % g] for g in range(G)],
                         [_wlist(L, "set%d" % g) for g in range(G)], sel, k, rates, sites, forced)
        return dict(zip(("gated_e", "gated_s", "scat_s", "sem_tok"), out))

    return Case("region", leaves, params, fut, ref, used, frozen="set1.w1", forced=forced_sets)


def fusion_case(b, ts, kcfg, seed=0):
    from cwf import coupler as CP
    e = E_DIM
    k = min(kcfg, ts)
    leaves = {"feats": rnd(b, ts, e, seed=seed + 21), "tok": rnd(b, 1, e, seed=seed + 22) * 0.05}
    leaves.update(_wdict("set0", seed + 300))
    params = [n for n in leaves if n.startswith("set0")]

    def forced_sets():
        gen = torch.Generator().manual_seed(seed + 78)
        return {(0, 0): torch.stack([torch.randperm(ts, generator=gen)[:k] for _ in range(b)], 0)}

    def fut(L, rates, forced):
        fo = {"fusion": v.to(L["feats"].device) for v in (forced or {}).values()}
        fused, idx = CP.FusionCouplerFn.apply(_cfg(kcfg, rates, fo, [("fusion",)]), L["feats"], L["tok"], *_wlist(L, "set0"))
        return {"fused": fused}, [idx.long().cpu()]

    def ref(L, sel, rates, sites, forced=None):
        return {"fused": fusion_ref(L["feats"], L["tok"], _wlist(L, "set0"), sel[0], k, rates, sites, (forced or {}).get((0, 0)))}

    return Case("fusion", leaves, params, fut, ref, ("fused",), frozen="set0.qkv.w", forced=forced_sets)


def intra_block_case(b, t, seed=0, twice=False):
    """IntraCouplerBlockFn on four sequences; twice: its two result halves go through the SAME weight set again (route C5)"""
    from cwf import coupler as CP
    e = E_DIM
    leaves = {n: rnd(b, t, e, seed=seed + 31 + i) for i, n in enumerate(SEL)}
    leaves.update(_wdict("set0", seed + 400))
    params = [n for n in leaves if n.startswith("set0")]

    def fut(L, rates, forced):
        W = _wlist(L, "set0")
        r = CP.IntraCouplerBlockFn.apply(_cfg(0, rates), *[L[n] for n in SEL], *W)
        if twice:
            r = CP.IntraCouplerBlockFn.apply(_cfg(0, rates), r[:, :t], L["sem_supp"], r[:, t:], L["edge_supp"], *W)
        return {"r": r}, []

    def ref(L, sel, rates, sites, forced=None):
        W = _wlist(L, "set0")
        r = intra_ref([W], *[L[n][None] for n in SEL], rates, sites)[0]
        if twice:
            r = intra_ref([W], r[None, :, 0], L["sem_supp"][None], r[None, :, 1], L["edge_supp"][None], rates, sites)[0]
        return {"r": r.reshape(b, 2 * t, e)}

    return Case("intra_block", leaves, params, fut, ref, ("r",), frozen="set0.out.w")


def fusion_block_case(b, t, seed=0, twice=False):
    from cwf import coupler as CP
    e = E_DIM
    leaves = {"x": rnd(b, t, e, seed=seed + 41)}
    leaves.update(_wdict("set0", seed + 500))
    params = [n for n in leaves if n.startswith("set0")]

    def fut(L, rates, forced):
        W = _wlist(L, "set0")
        r = CP.FusionBlockFn.apply(_cfg(0, rates), L["x"], *W)
        if twice:
            r = CP.FusionBlockFn.apply(_cfg(0, rates), r, *W)
        return {"r": r}, []

    def ref(L, sel, rates, sites, forced=None):
        W = _wlist(L, "set0")
        r = fusion_block_ref(W, L["x"], rates, sites)
        if twice:
            r = fusion_block_ref(W, r, rates, sites)
        return {"r": r}

    return Case("fusion_block", leaves, params, fut, ref, ("r",), frozen="set0.w2")


def shared_set_case(b, t, ts, kcfg, seed=0):
    """route C5: FusionBlockFn and FusionCouplerFn sharing ONE weight set -- the block's class row is the coupler's class token"""
    from cwf import coupler as CP
    e = E_DIM
    k = min(kcfg, ts)
    leaves = {"x": rnd(b, t, e, seed=seed + 51), "feats": rnd(b, ts, e, seed=seed + 52)}
    leaves.update(_wdict("set0", seed + 600))
    params = [n for n in leaves if n.startswith("set0")]

    def fut(L, rates, forced):
        W = _wlist(L, "set0")
        y = CP.FusionBlockFn.apply(_cfg(0, rates), L["x"], *W)
        fused, idx = CP.FusionCouplerFn.apply(_cfg(kcfg, rates, None, [("fusion",)]), L["feats"], y[:, 0:1] * 0.05, *W)
        return {"y": y, "fused": fused}, [idx.long().cpu()]

    def ref(L, sel, rates, sites, forced=None):
        W = _wlist(L, "set0")
        y = fusion_block_ref(W, L["x"], Rates(0.0, rates.attn, rates.pre, rates.ffn), sites)
        return {"y": y, "fused": fusion_ref(L["feats"], y[:, 0:1] * 0.05, W, sel[0], k, rates, sites)}

    return Case("shared_set", leaves, params, fut, ref, ("y", "fused"))


def encode_case(seed=0, kcfg=32):
    """The coupler section of ClsWiseFormer.encode as one graph: window_to_tokens_g -> RegionCouplerFn -> tokens_to_window_g x 2 and
    sum_groups3 x 2 -> FusionCouplerFn -> tokens_to_window; the reference goes through reference_model.convert_dim / split_dim."""
    from cwf import coupler as CP, functional as CF
    e, G, b = E_DIM, 3, 2
    esz, ssz, ec, sc = (16, 16, 16), (8, 8, 8), 32, 128
    leaves = {"ef": rnd(b, *esz, G * ec, seed=seed + 61), "sf": rnd(b, *ssz, G * sc, seed=seed + 62)}
    for g in range(G):
        leaves["e_tok%d" % g] = rnd(1, 1, e, seed=seed + 3 + g) * 0.05
        leaves["s_tok%d" % g] = rnd(1, 1, e, seed=seed + 13 + g) * 0.05
        leaves.update(_wdict("set%d" % g, seed + 100 + 50 * g))
    leaves.update(_wdict("fusion", seed + 700))
    params = [n for n in leaves if n not in ("ef", "sf")]
    names = [tuple("r%d_%s" % (g, n) for n in SEL) for g in range(G)]
    k = kcfg

    def forced_sets():            # region group 1 only (256 edge tokens, 128 semantic ones)
        out = {}
        for j, t in enumerate((256, 128, 128, 256)):
            gen = torch.Generator().manual_seed(seed + 79 + j)
            out[(1, j)] = torch.stack([torch.randperm(t, generator=gen)[:k] for _ in range(b)], 0)
        return out

    def fut(L, rates, forced):
        fo = {names[g][j]: v.to(L["ef"].device) for (g, j), v in (forced or {}).items()}
        Em = CP.window_to_tokens_g(L["ef"], G, rm.EDGE_PATCH)
        Sm = CP.window_to_tokens_g(L["sf"], G, rm.SEM_PATCH)
        flat = [L["e_tok%d" % g] for g in range(G)] + [L["s_tok%d" % g] for g in range(G)]
        for g in range(G):
            flat += _wlist(L, "set%d" % g)
        out = CP.RegionCouplerFn.apply(_cfg(kcfg, rates, fo, names, G), Em, Sm, *flat)
        gated_e, gated_s, scat_s, sem_tok = out[:4]
        sup_edge = CP.tokens_to_window_g(gated_e, esz, ec, rm.EDGE_PATCH)
        sup_sem = CP.tokens_to_window_g(gated_s, ssz, sc, rm.SEM_PATCH)
        f_tok, f_feat = CP.sum_groups3(sem_tok), CP.sum_groups3(scat_s)
        fused, f_idx = CP.FusionCouplerFn.apply(_cfg(kcfg, rates, None, [("fusion",)]), f_feat, f_tok, *_wlist(L, "fusion"))
        xb = CF.tokens_to_window(fused, ssz, sc, rm.SEM_PATCH)
        return {"sup_edge": sup_edge, "sup_sem": sup_sem, "xb": xb}, [o.long().cpu() for o in out[4:]] + [f_idx.long().cpu()]

    def ref(L, sel, rates, sites, forced=None):
        cf = lambda x: x.permute(0, 4, 1, 2, 3)                       # NDHWC -> NCDHW (the reference's layout)
        cl = lambda x: x.permute(0, 2, 3, 4, 1)
        Em = torch.stack([rm.convert_dim(cf(L["ef"][..., g * ec:(g + 1) * ec]), rm.EDGE_PATCH) for g in range(G)], 0)
        Sm = torch.stack([rm.convert_dim(cf(L["sf"][..., g * sc:(g + 1) * sc]), rm.SEM_PATCH) for g in range(G)], 0)
        gated_e, gated_s, scat_s, sem_tok = region_ref(Em, Sm, [L["e_tok%d" % g] for g in range(G)], [L["s_tok%d" % g] for g in range(G)],
                                                       [_wlist(L, "set%d" % g) for g in range(G)], sel[:4], k, rates, sites, forced)
        sup_edge = torch.cat([cl(rm.split_dim(gated_e[g], ec, esz, rm.EDGE_PATCH)) for g in range(G)], -1)
        sup_sem = torch.cat([cl(rm.split_dim(gated_s[g], sc, ssz, rm.SEM_PATCH)) for g in range(G)], -1)
        f_tok = sem_tok[0] + sem_tok[1] + sem_tok[2]
        f_feat = scat_s[0] + scat_s[1] + scat_s[2]
        fused = fusion_ref(f_feat, f_tok, _wlist(L, "fusion"), sel[4], k, rates, sites)
        return {"sup_edge": sup_edge, "sup_sem": sup_sem, "xb": cl(rm.split_dim(fused, sc, ssz, rm.SEM_PATCH))}

    return Case("encode", leaves, params, fut, ref, ("sup_edge", "sup_sem", "xb"), frozen="set2.qkv.w", forced=forced_sets)


# ====================================================================================================================
# the three runs and the comparison
# ====================================================================================================================
class Env:
    """Where the run under test happens: K the backend the Functions call (HipBackend, or EmulBackend on the CPU), `begin()` starts
    a step on it and returns the EmulBackend that evaluates the counter generator at that step's {seed, step}."""

    def __init__(self, K, dev, begin):
        self.K, self.dev, self.begin = K, dev, begin


def _loss(case, outs, dev, dtype):
    return sum((outs[n] * case.cotangent(n, outs[n].shape).to(device=dev, dtype=dtype)).sum() for n in case.used)


def run_under_test(case, env, monkeypatch, rates, sink=False, freeze=False, force=False, expect_sunk=True):
    """-> (results name -> CPU tensor: 'out:<name>' and 'd:<leaf>', selections, recorded sites, emul, forced sets)"""
    from cwf.optim import GradSink
    frozen = {case.frozen} if freeze else set()
    forced = case.forced() if force else None
    L = {n: t.clone().to(env.dev).requires_grad_(n not in frozen) for n, t in case.leaves.items()}
    rec = []
    emul = env.begin()
    with monkeypatch.context() as m:
        real = env.K.rng_site

        def spy(n):
            off = real(n)
            rec.append((int(off), int(n)))
            return off
        m.setattr(env.K, "rng_site", spy, raising=False)
        outs, sel = case.fut(L, rates, forced)
        loss = _loss(case, outs, env.dev, torch.float32)
        res = {"out:" + n: outs[n].detach().cpu().clone() for n in case.used}
        if sink:
            held = [n for n in case.params if n not in frozen]
            s = GradSink([L[n] for n in held])
            s.begin()
            s.flat.fill_(float("nan"))                     # nothing may be accumulated onto stale contents
            with s:
                loss.backward()
            s.finish()
            assert bool(torch.isfinite(s.flat).all()), "a gradient slice kept (or added onto) its stale contents"
            by_autograd = [n for n in held if L[n].grad is not None]
            unwritten = [n for n in held if L[n].data_ptr() not in s.written]
            if freeze:
                # one frozen weight: _grad_buffers falls back to autograd for the whole weight call, finish() copies the gradients in
                # (the weight sets "set*" of that call; class tokens and another Function's set stay on the sink's path)
                wn = [n for n in held if n.startswith("set")]
                assert set(wn) <= set(by_autograd) and set(wn) <= set(unwritten), ("no fall-back to autograd", by_autograd, unwritten)
                assert set(by_autograd) <= set(wn) and set(unwritten) <= set(wn), ("left the sink without cause", by_autograd, unwritten)
            elif expect_sunk:
                assert not by_autograd, ("parameters with a .grad under the sink", by_autograd)
                assert not unwritten, ("sink.written misses", unwritten)
            for n in held:
                res["d:" + n] = s.view(L[n]).detach().cpu().clone()
        else:
            loss.backward()
        for n in L:
            if "d:" + n not in res and n not in frozen:
                res["d:" + n] = torch.zeros_like(case.leaves[n]) if L[n].grad is None else L[n].grad.detach().cpu().clone()
    check_disjoint(rec)
    return res, sel, rec, emul, forced


def run_reference(case, dtype, sel, rates, sites, forced=None, skip=()):
    L = {n: t.clone().to(dtype).requires_grad_(True) for n, t in case.leaves.items()}
    outs = case.ref(L, sel, rates, sites, forced)
    if sites is not None:
        sites.done()
    _loss(case, outs, "cpu", dtype).backward()
    res = {"out:" + n: outs[n].detach().clone() for n in case.used}
    for n in L:
        if n not in skip:
            res["d:" + n] = torch.zeros_like(L[n]) if L[n].grad is None else L[n].grad.clone()
    return res


def group_of(name):
    if name.startswith("out:"):
        return "outputs"
    if "tok" in name and "." not in name:
        return "token grads"
    return "weight grads" if "." in name else "data grads"


def compare(got, r64, r32, tag, log=None):
    """per tensor: rel L2 <= 16 e32, max |err| <= 16 x the float32 run's; exact zeros stay exact.
    -> {group: (largest e32, worst rel-L2 ratio, worst max-abs ratio, the tensor with the worst ratio)}"""
    assert set(got) == set(r64) == set(r32), (sorted(got), sorted(r64))
    table, fails = {}, []
    for n in sorted(r64):
        t, y, g = r64[n], r32[n].double(), got[n].double()
        assert g.shape == t.shape, (tag, n, g.shape, t.shape)
        if not bool(torch.isfinite(g).all()):
            fails.append("%s: non-finite" % n)
            continue
        zero = (t == 0) & (y == 0)
        if bool((g[zero] != 0).any()):
            fails.append("%s: %d elements that are exactly zero in both references are not" % (n, int((g[zero] != 0).sum())))
            continue
        norm = float(t.norm())
        if norm == 0.0:
            continue
        e32, err = float((y - t).norm()) / norm, float((g - t).norm()) / norm
        m32, merr = float((y - t).abs().max()), float((g - t).abs().max())
        div = lambda a, b: a / b if b > 0 else (0.0 if a == 0 else math.inf)
        r2, rmax = div(err, e32), div(merr, m32)
        if err > FACTOR * e32 or merr > FACTOR * m32:
            fails.append("%s: rel L2 %.3e vs e32 %.3e (x%.2f), max abs %.3e vs %.3e (x%.2f)" % (n, err, e32, r2, merr, m32, rmax))
        gname = group_of(n)
        a, b, c, who = table.get(gname, (0.0, 0.0, 0.0, ""))
        table[gname] = (max(a, e32), max(b, r2), max(c, rmax), n.split(":")[1] if max(r2, rmax) > max(b, c) else who)
    if log is not None:
        log("%-34s " % tag + "  ".join("%s: e32 %.2e L2 x%.2f max x%.2f (%s)" % (k, *table[k])
                                       for k in ("outputs", "data grads", "token grads", "weight grads") if k in table))
    assert not fails, (tag, fails)
    return table


def run_case(case, env, monkeypatch, route, log=None, tag="", rates=None, sink=None):
    """the three runs of one case under one route, compared"""
    r, s, freeze, force = ROUTES[route] if route in ROUTES else (rates, sink, False, False)
    if rates is not None:
        r = rates
    if sink is not None:
        s = sink
    force = force and case.forced is not None
    got, sel, rec, emul, forced = run_under_test(case, env, monkeypatch, r, sink=s, freeze=freeze, force=force)
    assert r.off == (not rec), ("dropout sites drawn", rec)
    skip = {case.frozen} if freeze else ()
    refs = [run_reference(case, dt, sel, r, None if r.off else Sites(rec, emul), forced, skip) for dt in (torch.float64, torch.float32)]
    return compare(got, refs[0], refs[1], "%s %s %s" % (case.name, tag, route), log)


# ====================================================================================================================
# the cases (E = 512, heads = 8: the smallest shapes at which these paths differ), shared by the CPU and the GPU file
# ====================================================================================================================
REGION_SHAPES = {            # (G = 3)  B, Te, Ts, cfg.k
    "1-t17": (2, 80, 48, 16),            # 204 GEMM rows, a partly filled key tile
    "2-t129": (1, 256, 128, 128),        # k = Ts: every S row replaced, inv of S has no -1; the production t
    "3-clip": (2, 40, 24, 128),          # k clipped by min(cfg.k, ts, te) to 24
    "4-odd": (3, 144, 72, 33),           # an odd batch
}
FUSION_SHAPES = {"t17": (2, 48, 16), "t129": (1, 128, 128)}          # B, Ts, k
INTRA_T = (17, 129)
FUSION_BLOCK_T = (17, 144)
SUBSETS = ("gated_s", "sem_tok", "gated_e", "scat_s")
FN_ROUTES = ("C0", "C1", "C1a", "C1b", "C2", "C3", "C4")
BLOCK_ROUTES = ("C0", "C1", "C1a", "C1b", "C2", "C3")            # no selection to teacher-force
ENCODE_ROUTES = FN_ROUTES
C5_RATES = Rates(0.1, 0.1, 0.1, 0.1)


def c5_case(kind):
    if kind == "fusion_block_twice":
        return fusion_block_case(2, 17, seed=5, twice=True)
    if kind == "intra_block_twice":
        return intra_block_case(2, 17, seed=5, twice=True)
    return shared_set_case(2, 17, 48, 16, seed=5)


C5_KINDS = ("fusion_block_twice", "intra_block_twice", "block_and_coupler")


def small_adjoints(dev):
    """add3 and split_channels3 (one slice unused: its gradient reaches the adjoint as None) against float64 autograd; both are exact
    copies / one fp32 addition chain, so the float32 statement of the reference is the bound itself"""
    from cwf import coupler as CP
    a, b, c = (rnd(2, 4, 4, 4, 24, seed=80 + i) for i in range(3))
    d = rnd(2, 4, 4, 4, 24, seed=83)
    L = [t.clone().to(dev).requires_grad_(True) for t in (a, b, c)]
    y = CP.add3(*L)
    (y * d.to(dev)).sum().backward()
    assert torch.equal(y.detach().cpu(), (a + b) + c)
    R = [t.double().requires_grad_(True) for t in (a, b, c)]
    ((R[0] + R[1] + R[2]) * d.double()).sum().backward()
    for got, ref in zip(L, R):
        assert torch.equal(got.grad.cpu().double(), ref.grad)
    x = rnd(2, 4, 4, 4, 3 * 8, seed=84)
    d0, d2 = rnd(2, 4, 4, 4, 8, seed=85), rnd(2, 4, 4, 4, 8, seed=86)
    xl = x.clone().to(dev).requires_grad_(True)
    p0, p1, p2 = CP.split_channels3(xl)
    assert torch.equal(p1.detach().cpu(), x[..., 8:16])
    ((p0 * d0.to(dev)).sum() + (p2 * d2.to(dev)).sum()).backward()           # the middle slice is unused
    xr = x.double().requires_grad_(True)
    ((xr[..., :8] * d0.double()).sum() + (xr[..., 16:] * d2.double()).sum()).backward()
    assert torch.equal(xl.grad.cpu().double(), xr.grad) and float(xl.grad[..., 8:16].abs().max()) == 0.0
