"""CPU: tests/norm_ref.py tested where it can be -- against float64 autograd of the reference op chain, against a plain fp32 emulation
of each kernel of csrc/norm.hip (same operation order: fp32 partial sums of L terms, f64 fold, fp32 apply), which must stay inside
every bound on every input family, and against seeded defects of that emulation, each of which must leave a bound.  The vacuity
caps (norm_ref.AMBIGUOUS_CAP, TWO_CANDIDATE_CAP) are evaluated here by the reference alone on the inputs the GPU file uses."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import bf16_operand_ref as R
import norm_ref as NR
from test_norm_exact_gpu import CASES, FAMILIES, FAMILY_NAMES, _id, make_inputs, with_reference_stats

EMUL_CASES = [(3, (10, 14, 15), 16), (1, (10, 14, 15), 96), (2, (6, 8, 9), 384), (1, (8, 8, 9), 1024)]
F1 = torch.float32


# ------------------------------------------------------------------ the emulation
def emul_reduce(t1, t2, N, V, C, drop_last_lane=False, drop_block=None):
    """in_reduce_kernel: thread (cq, vs) of workgroup b adds voxels b vpb + vs + j nvs, j = 0 .. L-1, in fp32; f64 beyond"""
    L, vpb, nvs = NR.launch_L(N, V, C)
    nb = -(-V // vpb)
    b, j, vs = torch.meshgrid(torch.arange(nb), torch.arange(L), torch.arange(nvs), indexing="ij")
    inb = j * nvs + vs
    v = b * vpb + inb
    idx = torch.where((inb < vpb) & (v < V), v, torch.full_like(v, V))
    out = torch.zeros(N, C, 2, dtype=torch.float64)
    for k, t in enumerate((t1, t2)):
        tp = torch.cat([t.reshape(N, V, C), torch.zeros(N, 1, C, dtype=F1)], 1)[:, idx]       # [N, nb, L, nvs, C]
        acc = torch.zeros(N, nb, nvs, C, dtype=F1)
        for jj in range(L):
            acc = acc + tp[:, :, jj]
        if drop_last_lane:
            acc[:, :, nvs - 1] = 0
        if drop_block is not None:
            acc[:, drop_block] = 0
        out[:, :, k] = acc.double().sum((1, 2))
    return out


def emul_h(x, sc, sh, fused):
    x = x.reshape(x.shape[0], -1, x.shape[-1])
    if fused:
        return (x.double() * sc.double()[:, None] + sh.double()[:, None]).float()
    return x * sc[:, None] + sh[:, None]


def emul_fwd_stats(x, N, V, C, **kw):
    x = x.reshape(N, V, C)
    return emul_reduce(x, x * x, N, V, C, **kw)


def emul_finalize(S, V, eps=1e-5, clamp=True, eps_outside=False):
    invV = 1.0 / float(V)
    mean = S[..., 0] * invV
    var = S[..., 1] * invV - mean * mean
    if clamp:
        var = var.clamp_min(0.0)
    e = float(np.float32(eps))
    rstd = 1.0 / (torch.sqrt(var) + e) if eps_outside else 1.0 / torch.sqrt(var + e)
    return rstd.float(), (-mean * rstd).float()


def emul_norm_act_add(x, sc, sh, slope, res, fused=False, sample0=False, swap_quads=False, res_ldc_c_of=None):
    N, C = x.shape[0], x.shape[-1]
    if sample0:
        sc, sh = sc[:1].expand_as(sc), sh[:1].expand_as(sh)
    if swap_quads:
        perm = (torch.arange(C) // 4 ^ 1) * 4 + torch.arange(C) % 4
        perm = torch.where(perm < C, perm, torch.arange(C))
        sc, sh = sc[:, perm], sh[:, perm]
    h = emul_h(x, sc, sh, fused)
    s = torch.tensor(slope, dtype=F1)
    y = torch.where(h > 0, h, h * s)
    if res is not None:
        if res_ldc_c_of is not None:                     # the residual is a slice of res_ldc_c_of, read as if it were dense
            V = h.shape[1]
            res = res_ldc_c_of.reshape(N, -1)[:, :V * C].reshape(N, V, C)
        y = y + res.reshape(y.shape)
    return y


def emul_bwd_stats(dy, x, sc, sh, slope, N, V, C, fused=False, s2_from_x=False, act_from_x=False):
    h = emul_h(x, sc, sh, fused)
    s = torch.tensor(slope, dtype=F1)
    xf = x.reshape(N, V, C)
    g = dy.reshape(N, V, C) * torch.where((xf if act_from_x else h) > 0, torch.ones((), dtype=F1), s)
    return emul_reduce(g, g * (xf if s2_from_x else h), N, V, C)


def emul_apply(dy, x, sc, sh, slope, S, add, N, V, C, drop_hm2=False, div_nv=False, act_from_x=False):
    h = emul_h(x, sc, sh, True)
    s = torch.tensor(slope, dtype=F1)
    xf = x.reshape(N, V, C)
    g = dy.reshape(N, V, C) * torch.where((xf if act_from_x else h) > 0, torch.ones((), dtype=F1), s)
    invV = (torch.ones((), dtype=F1) / torch.tensor(float(V * (N if div_nv else 1)), dtype=F1)).double()
    m1, m2 = (S[:, None, :, 0] * invV).float(), (S[:, None, :, 1] * invV).float()
    o = g - m1
    if not drop_hm2:
        o = o - h * m2
    o = sc[:, None] * o
    if add is not None:
        o = o + add.reshape(N, V, C)
    xa = torch.maximum(h, h * s)
    return o, xa


def rne16(t):
    return t.to(torch.bfloat16).double()


# ------------------------------------------------------------------ one pass of every check over an emulation
def run_checks(r, defect=None, per_family=None):
    """every check of the GPU file on the emulation of one case; returns {check: worst err / bound}.  defect: the name of a seeded
    defect (see DEFECTS)."""
    N, V, C = r.N, r.V, r.C
    d = defect
    L = NR.launch_L(N, V, C)[0]
    rel = NR.sum_rel(L)
    out = {}

    def note(name, rt, nc_shape=False):
        out[name] = max(out.get(name, 0.0), float(rt.max()))
        if per_family is not None:
            for f in range(len(FAMILIES)):
                m = r.fam == f
                m = m[:, :, None].expand_as(rt) if nc_shape else m[:, None, :].expand_as(rt)
                if bool(m.any()):
                    k = (name, f)
                    per_family[k] = max(per_family.get(k, 0.0), float(rt[m].max()))

    # sums
    st = emul_fwd_stats(r.x, N, V, C, drop_last_lane=d == "last voxel sub-lane dropped", drop_block=0 if d == "one workgroup dropped" else None)
    note("in_stats", NR.ratios(st, r.S, NR.sums_bound(r.T, rel)), True)
    # finalize on those sums
    sc_e, sh_e = emul_finalize(st, V, eps_outside=d == "eps outside the square root")
    sc_ref, sh_ref = NR.finalize_ref(r.S, V)
    b_sc, b_sh = NR.finalize_bound(r.S, r.T, rel, V)
    note("in_finalize(own sums) scale", NR.ratios(sc_e, sc_ref, b_sc)[:, :, None], True)
    note("in_finalize(own sums) shift", NR.ratios(sh_e, sh_ref, b_sh)[:, :, None], True)
    # finalize alone: reference sums, and crafted ones (clamped / zero variance)
    S2 = r.S.clone()
    S2[:, 0::5, 1] = (S2[:, 0::5, 0] / V) ** 2 * V * (1 - 2.0 ** -40)
    sc_a, sh_a = emul_finalize(S2, V, clamp=d != "variance clamp removed", eps_outside=d == "eps outside the square root")
    sc_r, sh_r = NR.finalize_ref(S2, V)
    b1, b2 = NR.finalize_bound(S2, S2.abs(), 0.0, V)
    note("in_finalize(ref sums) scale", NR.ratios(sc_a, sc_r, b1)[:, :, None], True)
    note("in_finalize(ref sums) shift", NR.ratios(sh_a, sh_r, b2)[:, :, None], True)
    # forward tail
    wide = torch.full((N, V, C + 32), 1e4, dtype=F1)
    wide[..., 16:16 + C] = r.residual.reshape(N, V, C)
    for slope in (0.0, 0.01, 1.0):
        for fused in (False, True):
            y, ya, B, amb = NR.norm_act_add_ref(r.x, r.scale, r.shift, slope, r.residual)
            got = emul_norm_act_add(r.x, r.scale, r.shift, slope, r.residual, fused=fused, sample0=d == "sample 0's scale and shift",
                                    swap_quads=d == "channel quads swapped",
                                    res_ldc_c_of=wide if d == "residual read with ldc = C" else None)
            note("norm_act_add", NR.ratios(got, y, B, alt=ya))
            got16 = R.hi_trunc(got) if d == "truncating bf16" else rne16(got)
            lo16, hi16 = NR.bf16_hull(y, ya, B)
            out["y16 candidates"] = max(out.get("y16 candidates", 0.0), NR.bf16_ratio(got16, lo16, hi16)[0])
    # backward
    for slope in (0.0, 0.01):
        S, T, D = NR.bwd_sums_ref(r.dy, r.x, r.scale, r.shift, slope)
        for fused in (False, True):
            sb = emul_bwd_stats(r.dy, r.x, r.scale, r.shift, slope, N, V, C, fused=fused, s2_from_x=d == "S2 from g*x",
                                act_from_x=d == "act' from x")
            note("in_bwd_stats", NR.ratios(sb, S, NR.sums_bound(T, rel, D)), True)
        kw = dict(drop_hm2=d == "h*m2 term dropped", div_nv=d == "division by N*V", act_from_x=d == "act' from x")
        two = NR.in_bwd_ref(r.dy, r.x, r.scale, r.shift, slope, dx_add=r.dx_add, rel=rel)
        o, _ = emul_apply(r.dy, r.x, r.scale, r.shift, slope, sb, r.dx_add, N, V, C, **kw)
        note("in_bwd (two-pass)", NR.ratios(o, two.dx, two.B, alt=two.dx_alt))
        one = NR.in_bwd_ref(r.dy, r.x, r.scale, r.shift, slope, S=S, dx_add=r.dx_add)
        o, xa = emul_apply(r.dy, r.x, r.scale, r.shift, slope, S, r.dx_add, N, V, C, **kw)
        note("in_bwd_apply(ref sums)", NR.ratios(o, one.dx, one.B, alt=one.dx_alt))
        cv = R.hi_trunc if d == "truncating bf16" else rne16
        out["dx16 candidates"] = max(out.get("dx16 candidates", 0.0), NR.bf16_ratio(cv(o), *NR.bf16_hull(one.dx, one.dx_alt, one.B))[0])
        a_lo, a_hi = NR.act_h_ref(r.x, r.scale, r.shift, slope)
        out["xa16 candidates"] = max(out.get("xa16 candidates", 0.0), NR.bf16_ratio(cv(xa), R.hi(a_lo), R.hi(a_hi))[0])
    # bias gradient
    dyf = NR.flat(r.dy)
    db, Tb = dyf.sum((0, 1)), dyf.abs().sum((0, 1))
    got_db = emul_fwd_stats(r.dy, N, V, C)[:, :, 0].sum(0).float()
    out["bias gradient"] = float(NR.ratios(got_db, db, (rel * Tb + R.U32 * db.abs()) * NR.SECOND_ORDER).max())
    return out


DEFECTS = ["last voxel sub-lane dropped", "one workgroup dropped", "sample 0's scale and shift", "channel quads swapped", "S2 from g*x",
           "h*m2 term dropped", "division by N*V", "act' from x", "truncating bf16", "variance clamp removed",
           "eps outside the square root", "residual read with ldc = C"]

_cache = {}


def _case(case):
    if case not in _cache:
        _cache[case] = with_reference_stats(make_inputs(*case))
    return _cache[case]


@pytest.mark.parametrize("case", EMUL_CASES, ids=_id)
def test_emulation_stays_inside_every_bound(case):
    r = _case(case)
    fam = {}
    out = run_checks(r, per_family=fam)
    for (name, f), v in sorted(fam.items()):
        print("EMUL %-34s %-22s %-12s %.4g" % (name, _id(case), FAMILY_NAMES[f], v))
    for name, v in out.items():
        print("EMUL %-34s %-22s %-12s %.4g" % (name, _id(case), "all", v))
    assert all(v <= 1.0 for v in out.values()), {k: v for k, v in out.items() if not v <= 1.0}
    # the bounds are not far too wide either: the long sums come within two orders of theirs
    assert out["in_stats"] > 1e-3 and out["in_bwd_apply(ref sums)"] > 0.05, out


@pytest.mark.parametrize("defect", DEFECTS)
def test_seeded_defect_leaves_a_bound(defect):
    r = _case(EMUL_CASES[0])                              # N = 3, nine workgroups per sample, every family
    clean, bad = run_checks(r), run_checks(r, defect=defect)
    caught = sorted(k for k, v in bad.items() if v > 1.0 and clean[k] <= 1.0)
    print("DEFECT %-30s caught by: %s" % (defect, ", ".join("%s (%.3g)" % (k, bad[k]) for k in caught)))
    assert caught, (defect, bad)


@pytest.mark.parametrize("slope", [0.0, 0.01])
@pytest.mark.parametrize("use_add", [False, True])
@pytest.mark.parametrize("case", EMUL_CASES[:2], ids=_id)
def test_reference_against_float64_autograd(case, slope, use_add):
    """both sides are float64: they agree to float64 rounding times kappa -- 1e-9 of the magnitude terms of the bounds"""
    r = _case(case)
    N, V, C = r.N, r.V, r.C
    eps, s = NR.f32(1e-5), NR.f32(slope)
    x = r.x.double().permute(0, 4, 1, 2, 3).clone().requires_grad_(True)
    res = r.residual.double().permute(0, 4, 1, 2, 3)
    y = F.leaky_relu(F.instance_norm(x, eps=eps), s) + res
    y.backward(r.dy.double().permute(0, 4, 1, 2, 3))
    dx = x.grad.permute(0, 2, 3, 4, 1).reshape(N, V, C) + (NR.flat(r.dx_add) if use_add else 0.0)
    y = y.detach().permute(0, 2, 3, 4, 1).reshape(N, V, C)
    sc, sh = NR.finalize_ref(r.S, V, eps)                  # unrounded float64 operands
    y_ref, _, _, _ = NR.norm_act_add_ref(r.x, sc, sh, slope, r.residual)
    xs = NR.flat(r.x) * sc[:, None]
    mag_y = xs.abs() + sh[:, None].abs() + NR.flat(r.residual).abs()
    b = NR.in_bwd_ref(r.dy, r.x, sc, sh, slope, dx_add=r.dx_add if use_add else None)
    V_ = float(V)
    mag_dx = sc[:, None].abs() * (b.g.abs() + (b.S[:, None, :, 0] / V_).abs() + (b.h * b.S[:, None, :, 1] / V_).abs()) + \
        (NR.flat(r.dx_add).abs() if use_add else 0.0)
    # (instance_norm centres before it scales: in the constant channel it gives h = 0 exactly, as x*scale + shift does in float64)
    for f in range(len(FAMILIES)):
        m = (r.fam == f)[:, None, :].expand(N, V, C)
        ry = float(((y - y_ref).abs()[m] / mag_y[m].clamp_min(1e-300)).max())
        rd = float(((dx - b.dx).abs()[m] / mag_dx[m].clamp_min(1e-300)).max())
        print("AUTOGRAD %-12s y %.3g dx %.3g" % (FAMILY_NAMES[f], ry, rd))
        assert ry <= 1e-9 and rd <= 1e-9, (FAMILY_NAMES[f], ry, rd)


def test_sum_rel_and_launch_rule():
    u = R.U32
    assert NR.launch_L(1, 128 ** 3, 16) == (16, 1024, 64)
    assert NR.launch_L(3, 2431, 96)[1:] == (256, 10) and NR.launch_L(3, 2431, 96)[0] == 26
    assert NR.launch_L(1, 2431, 1024) == (256, 256, 1)
    assert NR.launch_L(2, 1, 16) == (1, 1, 64)
    assert NR.sum_rel(16) == 17 * u                         # short chains: deterministic
    assert NR.sum_rel(256) == R.gamma_fp32(257) < 257 * u   # long ones: the probabilistic model


def test_scale_moves_less_than_a_bf16_ulp_on_the_offset_family():
    """the threshold past which the fp32 partial chain would have to be shortened: kappa * sum_rel(L) moving `scale` of the
    `-10 +- 1` family by more than 2^-9 of itself.  Both the bound and the emulation stay far below, at every L up to C = 1024."""
    for case in EMUL_CASES:
        r = _case(case)
        N, V, C = case[0], r.V, case[2]
        rel = NR.sum_rel(NR.launch_L(N, V, C)[0])
        m = r.fam == 2
        sc_ref, _ = NR.finalize_ref(r.S, V)
        b_sc, _ = NR.finalize_bound(r.S, r.T, rel, V)
        sc_e, _ = emul_finalize(emul_fwd_stats(r.x, N, V, C), V)
        bound_rel = float((b_sc / sc_ref)[m].max())
        moved = float(((sc_e.double() - sc_ref).abs() / sc_ref)[m].max())
        print("SCALE %-22s L %4d  bound %.3g  emulation %.3g  (2^-9 = %.3g)" % (_id(case), NR.launch_L(N, V, C)[0], bound_rel, moved, 2.0 ** -9))
        assert moved <= bound_rel < 2.0 ** -9


@pytest.mark.parametrize("case", [c for c in CASES if c[0] * c[1][0] * c[1][1] * c[1][2] * c[2] <= 5_000_000], ids=_id)
def test_vacuity_caps_by_the_reference_alone(case):
    """section `conditions that keep the test from hiding a failure`: the share of sign-ambiguous elements and of elements with two
    bf16 candidates, on the inputs the GPU file uses, without any kernel"""
    r = _case(case) if case in _cache else with_reference_stats(make_inputs(*case))
    for slope in (0.0, 0.01):
        y, ya, B, amb = NR.norm_act_add_ref(r.x, r.scale, r.shift, slope, r.residual)
        v = NR.assert_not_vacuous(amb, *NR.bf16_hull(y, ya, B), r.kappa_nominal, r.degen, "y16")
        one = NR.in_bwd_ref(r.dy, r.x, r.scale, r.shift, slope, S=NR.bwd_sums_ref(r.dy, r.x, r.scale, r.shift, slope)[0], dx_add=r.dx_add)
        w = NR.assert_not_vacuous(one.amb, *NR.bf16_hull(one.dx, one.dx_alt, one.B), r.kappa_nominal, r.degen, "dx16")
        a_lo, a_hi = NR.act_h_ref(r.x, r.scale, r.shift, slope)
        z = NR.assert_not_vacuous(amb, R.hi(a_lo), R.hi(a_hi), r.kappa_nominal, r.degen, "xa16")
        print("CAPS %-22s slope %-4g ambiguous %.2g  two candidates (kappa <= 1.25 / above): y16 %.2g / %.2g  dx16 %.2g / %.2g  xa16 %.2g / %.2g"
              % (_id(case), slope, v[0], v[1], v[2], w[1], w[2], z[1], z[2]))
