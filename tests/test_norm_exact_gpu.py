"""GPU: the InstanceNorm kernel family (csrc/norm.hip) and the bias-gradient channel sum that rides on it (csrc/optim.hip) against the
float64 reference of tests/norm_ref.py, per element or per (sample, channel) -- never against a tensor-wide maximum.  The bounds and
their derivations are in norm_ref.py; tests/test_norm_ref_cpu.py tests that reference, and that it fails on seeded defects.

Inputs (make_inputs): every (sample, channel) takes its mean and spread from FAMILIES by (c + 3 n) % 7, so neighbouring channels,
channel quads (c + 4) and samples all differ -- a wrong n, c or quad index lands in another family.  dy, residual and dx_add carry
per-channel magnitudes 1e-3 .. 1e2.  scale / shift handed to the elementwise kernels are the fp32 roundings of finalize_ref on the
reference sums, so every case (and its vacuity caps) is reproducible without a GPU; what the kernels make of sums has its own checks.

Every check prints `RATIO <check> <case> <worst err / bound>`; above 1 it fails.  A case collects all its failures before it raises."""
import pytest
import torch

import bf16_operand_ref as R
import norm_ref as NR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
E_BADARG, E_TOOLARGE, E_ALIGN = -1, -2, -3

FAMILIES = [(0.0, 1.0), (0.3, 0.6), (-10.0, 1.0), (50.0, 0.5), (3.0, 30.0), (0.0, 0.0), (7.25, 0.0)]      # (mean, standard deviation)
FAMILY_NAMES = ["0+-1", "0.3+-0.6", "-10+-1", "50+-0.5", "3+-30", "zero", "const 7.25"]


def family_of(n, c):
    return (c + 3 * n) % len(FAMILIES)


def _per_channel(N, C, rot):
    """[N, 1, C] magnitudes 10^(-3 .. 2) that differ between neighbouring channels and samples"""
    n, c = torch.arange(N)[:, None], torch.arange(C)[None, :]
    return (10.0 ** (-3.0 + 5.0 * ((c * 5 + n * 3 + rot) % 8).float() / 7.0))[:, None, :]


class Inputs:
    pass


def make_inputs(N, dims, C, seed=0):
    """x, dy, residual, dx_add [N, D, H, W, C] fp32 (CPU) and the per-(n, c) tables: fam, kappa_nominal"""
    g = torch.Generator().manual_seed(1000 * seed + 7 * C + N)
    D, H, W = dims
    V = D * H * W
    fam = torch.tensor([[family_of(n, c) for c in range(C)] for n in range(N)])
    mean = torch.tensor([m for m, _ in FAMILIES])[fam][:, None, :]
    std = torch.tensor([s for _, s in FAMILIES])[fam][:, None, :]
    r = Inputs()
    r.N, r.dims, r.V, r.C, r.fam = N, dims, V, C, fam
    r.x = (mean + std * torch.randn(N, V, C, generator=g)).view(N, D, H, W, C)
    r.dy = (torch.randn(N, V, C, generator=g) * _per_channel(N, C, 0)).view(N, D, H, W, C)
    r.residual = (torch.randn(N, V, C, generator=g) * _per_channel(N, C, 3)).view(N, D, H, W, C)
    r.dx_add = (torch.randn(N, V, C, generator=g) * _per_channel(N, C, 5)).view(N, D, H, W, C)
    m2, s2 = mean[:, 0].double() ** 2, std[:, 0].double() ** 2
    r.kappa_nominal = torch.where(s2 > 0, (m2 + s2) / s2.clamp_min(1e-300), torch.full_like(s2, float("inf")))
    return r


def with_reference_stats(r, eps=1e-5):
    """adds S, T (forward sums), scale, shift (fp32 [N, C] of finalize_ref), degen"""
    r.S, r.T = NR.fwd_sums_ref(r.x)
    sc, sh = NR.finalize_ref(r.S, r.V, eps)
    r.scale, r.shift = sc.float(), sh.float()
    r.degen = NR.degenerate(r.x)
    return r


GEOMETRY = [(n, (11, 13, 17), c) for c in (4, 16, 32, 96, 128, 256, 384, 1024) for n in (1, 3)]
EDGES = [(2, d, c) for c in (16, 96) for d in ((1, 1, 1), (3, 5, 17), (4, 8, 8), (1, 257, 1), (5, 10, 20))]      # V = 1, 255, 256, 257, 1000
PRODUCT = [(2, (64, 64, 64), 32), (2, (32, 32, 32), 64), (2, (16, 16, 16), 128), (2, (8, 8, 8), 256)]            # (1, 128^3, 16): below
CASES = GEOMETRY + EDGES + PRODUCT


def _id(case):
    n, d, c = case
    return "n%d-%dx%dx%d-c%d" % (n, d[0], d[1], d[2], c)


class Report:
    def __init__(self, case):
        self.case, self.fails = case, []

    def __call__(self, check, ratio_at):
        r, at = ratio_at if isinstance(ratio_at, tuple) else (ratio_at, None)
        print("RATIO %-34s %-24s %.4g" % (check, self.case, r))
        if not r <= 1.0:
            self.fails.append((check, r, at))
        return r

    def done(self):
        assert not self.fails, (self.case, self.fails)


def _dev(t):
    return t.to(DEV)


def _bwd_stats(hip, dy, x, scale, shift, slope):
    from cwf.kernels import cl
    dy, dy_ldc = cl(dy)
    x, x_ldc = cl(x)
    n, d, h, w, c = x.shape
    sums = torch.zeros((n, c, 2), dtype=torch.float64, device=x.device)
    hip._call("cwf_in_bwd_stats", dy.data_ptr(), dy_ldc, x.data_ptr(), x_ldc, scale.data_ptr(), shift.data_ptr(), float(slope),
              sums.data_ptr(), n, d * h * w, c, hip._stream())
    return sums


def _stats_checks(hip, r, rep, slopes=(0.0, 0.01)):
    """in_stats, in_finalize on the GPU's sums, in_bwd_stats; returns the GPU's forward sums"""
    L = NR.launch_L(r.N, r.V, r.C)[0]
    rel = NR.sum_rel(L)
    xd, dyd, scd, shd = _dev(r.x), _dev(r.dy), _dev(r.scale), _dev(r.shift)
    st = hip.in_stats(xd)
    rep("in_stats", NR.ratio(st, r.S, NR.sums_bound(r.T, rel)))
    sc, sh = hip.in_finalize(st, r.V)
    sc_ref, sh_ref = NR.finalize_ref(r.S, r.V)
    b_sc, b_sh = NR.finalize_bound(r.S, r.T, rel, r.V)
    rep("in_finalize(gpu sums) scale", NR.ratio(sc, sc_ref, b_sc))
    rep("in_finalize(gpu sums) shift", NR.ratio(sh, sh_ref, b_sh))
    for slope in slopes:
        S, T, D = NR.bwd_sums_ref(r.dy, r.x, r.scale, r.shift, slope)
        rep("in_bwd_stats slope %g" % slope, NR.ratio(_bwd_stats(hip, dyd, xd, scd, shd, slope), S, NR.sums_bound(T, rel, D)))
    return st


def _apply_ex(hip, dy, x, scale, shift, slope, sums, dx_add, f32_, dx16_, xa16_):
    return hip.in_bwd_apply16(dy, x, scale, shift, slope, sums, dx_add=dx_add, want_dx16=dx16_, want_xa16=xa16_, need_f32=f32_)


def _elementwise_checks(hip, r, rep, fwd_slopes=(0.0, 0.01, 1.0), bwd=((0.0, True), (0.01, False), (0.01, True))):
    xd, dyd, scd, shd = _dev(r.x), _dev(r.dy), _dev(r.scale), _dev(r.shift)
    resd, addd = _dev(r.residual), _dev(r.dx_add)
    kap, degen = r.kappa_nominal, r.degen
    # ---- norm_act_add, y16
    for slope in fwd_slopes:
        for res in (None, r.residual):
            tag = "slope %g%s" % (slope, "" if res is None else " +res")
            y, y_alt, B, amb = NR.norm_act_add_ref(r.x, r.scale, r.shift, slope, res)
            got, got16 = hip.norm_act_add(xd, scd, shd, slope, None if res is None else resd, want16=True)
            rep("norm_act_add " + tag, NR.ratio(got, y, B, alt=y_alt))
            assert torch.equal(got16, got.to(torch.bfloat16)), "y16 is not bf16_rne of the kernel's own y"
            lo16, hi16 = NR.bf16_hull(y, y_alt, B)
            rep("y16 candidates " + tag, NR.bf16_ratio(got16, lo16, hi16))
            NR.assert_not_vacuous(amb, lo16, hi16, kap, degen, (rep.case, "y16", tag))
            if res is None:                                   # the all-zero channel: act(0) exactly
                z = (r.fam == 5)[:, None, :].expand(r.N, r.V, r.C)
                assert bool((NR.flat(got)[z] == 0).all()), "all-zero channel: y != 0"
            else:
                z = (r.fam == 5)[:, None, :].expand(r.N, r.V, r.C)
                assert torch.equal(NR.flat(got)[z], NR.flat(res)[z]), "all-zero channel: y != residual"
    # ---- the backward
    L = NR.launch_L(r.N, r.V, r.C)[0]
    rel = NR.sum_rel(L)
    for slope, use_add in bwd:
        tag = "slope %g%s" % (slope, " +add" if use_add else "")
        add, add_d = (r.dx_add, addd) if use_add else (None, None)
        two = NR.in_bwd_ref(r.dy, r.x, r.scale, r.shift, slope, dx_add=add, rel=rel)
        rep("in_bwd (two-pass) " + tag, NR.ratio(hip.in_bwd(dyd, xd, scd, shd, slope, dx_add=add_d), two.dx, two.B, alt=two.dx_alt))
        S = two.S                                            # the apply kernel alone: fed the reference sums
        one = NR.in_bwd_ref(r.dy, r.x, r.scale, r.shift, slope, S=S, dx_add=add)
        Sd = _dev(S.contiguous())
        rep("in_bwd_apply(ref sums) " + tag, NR.ratio(hip.in_bwd_apply(dyd, xd, scd, shd, slope, Sd, dx_add=add_d), one.dx, one.B, alt=one.dx_alt))
        lo16, hi16 = NR.bf16_hull(one.dx, one.dx_alt, one.B)
        a_lo, a_hi = NR.act_h_ref(r.x, r.scale, r.shift, slope)
        xlo16, xhi16 = R.hi(a_lo), R.hi(a_hi)
        NR.assert_not_vacuous(one.amb, lo16, hi16, kap, degen, (rep.case, "dx16", tag))
        NR.assert_not_vacuous(one.amb, xlo16, xhi16, kap, degen, (rep.case, "xa16", tag))
        tb = hip.to_bf16(xd, scd, shd, slope)
        rep("to_bf16 candidates " + tag, NR.bf16_ratio(tb, xlo16, xhi16))
        for f32_, dx16_, xa16_ in ((True, True, True), (True, True, False), (True, False, True), (True, False, False),
                                   (False, True, True), (False, True, False)):
            v = "<%d%d%d> " % (f32_, dx16_, xa16_) + tag
            dx, dx16, xa16 = _apply_ex(hip, dyd, xd, scd, shd, slope, Sd, add_d, f32_, dx16_, xa16_)
            if f32_:
                rep("apply_ex dx " + v, NR.ratio(dx, one.dx, one.B, alt=one.dx_alt))
            if dx16_:
                rep("apply_ex dx16 " + v, NR.bf16_ratio(dx16, lo16, hi16))
                if f32_:
                    assert torch.equal(dx16, dx.to(torch.bfloat16)), "dx16 is not bf16_rne of the kernel's own dx"
            if xa16_:
                rep("apply_ex xa16 " + v, NR.bf16_ratio(xa16, xlo16, xhi16))
                assert torch.equal(xa16, tb), "xa16 differs from cwf_to_bf16"


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_norm_family_against_float64(hip, case):
    """every kernel of the family on one input case: sums, finalize on those sums, the forward tail, the two-pass backward, the apply
    kernel alone and its six <F32, DX16, XA16> variants, cwf_to_bf16"""
    N, dims, C = case
    r = with_reference_stats(make_inputs(N, dims, C))
    rep = Report(_id(case))
    _stats_checks(hip, r, rep)
    _elementwise_checks(hip, r, rep)
    rep.done()


# ------------------------------------------------------------------ the full-resolution product shape: two cases
def test_sums_at_full_resolution(hip):
    """(1, 128^3, 16): 2048 workgroups of 1024 voxels, L = 16, f64 atomics between them"""
    r = with_reference_stats(make_inputs(1, (128, 128, 128), 16))
    assert NR.launch_L(1, r.V, 16) == (16, 1024, 64)
    rep = Report("n1-128x128x128-c16")
    _stats_checks(hip, r, rep, slopes=(0.01,))
    rep.done()


def test_elementwise_at_full_resolution(hip):
    """(1, 128^3, 16): the forward tail with residual and the bf16-only hand-off (dx == NULL) the trainer takes, in voxel chunks"""
    r = with_reference_stats(make_inputs(1, (128, 128, 128), 16))
    rep = Report("n1-128x128x128-c16")
    xd, dyd, scd, shd, resd, addd = (_dev(t) for t in (r.x, r.dy, r.scale, r.shift, r.residual, r.dx_add))
    slope = 0.01
    y, y16 = hip.norm_act_add(xd, scd, shd, slope, resd, want16=True)
    S = torch.zeros(1, 16, 2, dtype=torch.float64)
    step = 1 << 18
    fl = lambda t: t.reshape(1, -1, 16)
    for v0 in range(0, r.V, step):
        S += NR.bwd_sums_ref(fl(r.dy)[:, v0:v0 + step], fl(r.x)[:, v0:v0 + step], r.scale, r.shift, slope)[0]
    _, dx16, xa16 = _apply_ex(hip, dyd, xd, scd, shd, slope, _dev(S), addd, False, True, True)
    assert torch.equal(xa16, hip.to_bf16(xd, scd, shd, slope))
    worst = {"norm_act_add": 0.0, "y16 candidates": 0.0, "apply_ex dx16 <011>": 0.0, "apply_ex xa16 <011>": 0.0}
    amb_n, two_n = 0, 0
    for v0 in range(0, r.V, step):
        sl = slice(v0, v0 + step)
        xs, dys, rs, as_ = (fl(t)[:, sl] for t in (r.x, r.dy, r.residual, r.dx_add))
        yr, ya, B, amb = NR.norm_act_add_ref(xs, r.scale, r.shift, slope, rs)
        worst["norm_act_add"] = max(worst["norm_act_add"], NR.ratio(fl(y)[:, sl], yr, B, alt=ya)[0])
        lo16, hi16 = NR.bf16_hull(yr, ya, B)
        worst["y16 candidates"] = max(worst["y16 candidates"], NR.bf16_ratio(fl(y16)[:, sl], lo16, hi16)[0])
        one = NR.in_bwd_ref(dys, xs, r.scale, r.shift, slope, S=S, dx_add=as_, V=r.V)
        dlo, dhi = NR.bf16_hull(one.dx, one.dx_alt, one.B)
        worst["apply_ex dx16 <011>"] = max(worst["apply_ex dx16 <011>"], NR.bf16_ratio(fl(dx16)[:, sl], dlo, dhi)[0])
        a_lo, a_hi = NR.act_h_ref(xs, r.scale, r.shift, slope)
        worst["apply_ex xa16 <011>"] = max(worst["apply_ex xa16 <011>"], NR.bf16_ratio(fl(xa16)[:, sl], R.hi(a_lo), R.hi(a_hi))[0])
        live = (~r.degen)[:, None, :].expand_as(amb)
        amb_n += int((amb & live).sum())
        two_n += int(((dlo != dhi) & live).sum())
    for k, v in worst.items():
        rep(k, v)
    live_total = int((~r.degen).sum()) * r.V
    assert amb_n / live_total <= NR.AMBIGUOUS_CAP and two_n / live_total <= NR.TWO_CANDIDATE_CAP[False]
    assert torch.equal(y16, y.to(torch.bfloat16))
    rep.done()


def test_xa16_is_the_weight_gradient_operand(hip):
    """(64^3, 16 -> 16): xa16 of the apply kernel, cwf_to_bf16 and the operand bf16_operand_ref.prologue + hi hands the weight-gradient
    reference are one definition, bit for bit"""
    r = with_reference_stats(make_inputs(1, (64, 64, 64), 16))
    xd, dyd, scd, shd = (_dev(t) for t in (r.x, r.dy, r.scale, r.shift))
    for slope in (0.0, 0.01):
        S = hip.in_stats(dyd)
        _, _, xa16 = _apply_ex(hip, dyd, xd, scd, shd, slope, S, None, True, False, True)
        tb = hip.to_bf16(xd, scd, shd, slope)
        assert torch.equal(xa16, tb)
        ref = NR.prologue_operand(r.x, r.scale, r.shift, slope)
        assert torch.equal(NR.flat(tb), ref), int((NR.flat(tb) != ref).sum())


# ------------------------------------------------------------------ finalize alone
@pytest.mark.parametrize("nc", [1, 255, 257, 3072])
def test_finalize_alone(hip, nc):
    """cwf_in_finalize fed the reference's own doubles: only the two casts remain, 2u |value|.  Sums of all input families at
    V = 128^3, sums whose S2/V - mean^2 is exactly zero, and sums where it is slightly negative (the clamp)."""
    rep = Report("nc%d" % nc)
    V = 128 ** 3
    g = torch.Generator().manual_seed(nc)
    fam = torch.arange(nc) % 5
    mean = torch.tensor([m for m, _ in FAMILIES[:5]], dtype=torch.float64)[fam] * (1 + 0.01 * torch.rand(nc, generator=g, dtype=torch.float64))
    std = torch.tensor([s for _, s in FAMILIES[:5]], dtype=torch.float64)[fam]
    S = torch.stack([mean * V, (mean * mean + std * std) * V], -1)
    S[0::7] = torch.tensor([3.0 * V, 9.0 * V * (1 - 2.0 ** -40)], dtype=torch.float64)      # var slightly negative: clamped
    S[3::7] = torch.tensor([7.25 * V, 52.5625 * V], dtype=torch.float64)   # var exactly zero
    if nc > 5:
        S[5] = 0.0
    S = S.view(1, nc, 2)
    raw_var = S[0, :, 1] / V - (S[0, :, 0] / V) ** 2
    assert bool((raw_var[0::7] < 0).all()) and bool((raw_var[3::7] == 0).all())
    sc, sh = hip.in_finalize(_dev(S), V)
    sc_ref, sh_ref = NR.finalize_ref(S, V)
    b_sc, b_sh = NR.finalize_bound(S, S.abs(), 0.0, V)
    rep("in_finalize(ref sums) scale", NR.ratio(sc, sc_ref, b_sc))
    rep("in_finalize(ref sums) shift", NR.ratio(sh, sh_ref, b_sh))
    rep.done()


# ------------------------------------------------------------------ bias gradient
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("c", [4, 16, 96, 132])
def test_bias_gradient_channel_sum(hip, c, n):
    """stats_channel_sum(in_stats(dy)) against the f64 sum over samples and voxels: sum_rel(L) T + u |db| (the fp32 cast); C = 132
    leaves the 64-thread launch a ragged last block"""
    r = make_inputs(n, (11, 13, 17), c)
    rep = Report("n%d-c%d" % (n, c))
    out = torch.full((c + 8,), float("nan"), device=DEV)
    hip.stats_channel_sum(hip.in_stats(_dev(r.dy)), out[:c])
    d = NR.flat(r.dy)
    db, T = d.sum((0, 1)), d.abs().sum((0, 1))
    rel = NR.sum_rel(NR.launch_L(n, r.V, c)[0])
    rep("bias gradient", NR.ratio(out[:c], db, (rel * T + R.U32 * db.abs()) * NR.SECOND_ORDER))
    assert bool(torch.isnan(out[c:]).all()), "the channel sum wrote past C"
    rep.done()


# ------------------------------------------------------------------ channel slices of wider buffers
def test_channel_slices_of_concat_buffers(hip):
    """x, dy, residual, dx_add each the slice [..., 16:48] of a 64-wide buffer whose other channels hold NaN (kernels.cl: ldc = 64)"""
    N, dims, C = 2, (7, 9, 12), 32
    r = with_reference_stats(make_inputs(N, dims, C))
    rep = Report("slices-n2-7x9x12-c32")

    def wide(t):
        b = torch.full((N,) + dims + (64,), float("nan"), device=DEV)
        b[..., 16:48] = t.to(DEV)
        return b[..., 16:48]
    from cwf.kernels import cl
    xd, dyd, resd, addd = wide(r.x), wide(r.dy), wide(r.residual), wide(r.dx_add)
    assert cl(xd)[1] == 64 and cl(xd)[0].data_ptr() == xd.data_ptr()
    scd, shd = _dev(r.scale), _dev(r.shift)
    rel = NR.sum_rel(NR.launch_L(N, r.V, C)[0])
    rep("in_stats", NR.ratio(hip.in_stats(xd), r.S, NR.sums_bound(r.T, rel)))
    slope = 0.01
    S, T, D = NR.bwd_sums_ref(r.dy, r.x, r.scale, r.shift, slope)
    rep("in_bwd_stats", NR.ratio(_bwd_stats(hip, dyd, xd, scd, shd, slope), S, NR.sums_bound(T, rel, D)))
    y, ya, B, _ = NR.norm_act_add_ref(r.x, r.scale, r.shift, slope, r.residual)
    got, got16 = hip.norm_act_add(xd, scd, shd, slope, resd, want16=True)
    rep("norm_act_add", NR.ratio(got, y, B, alt=ya))
    rep("y16 candidates", NR.bf16_ratio(got16, *NR.bf16_hull(y, ya, B)))
    two = NR.in_bwd_ref(r.dy, r.x, r.scale, r.shift, slope, dx_add=r.dx_add, rel=rel)
    rep("in_bwd (two-pass)", NR.ratio(hip.in_bwd(dyd, xd, scd, shd, slope, dx_add=addd), two.dx, two.B, alt=two.dx_alt))
    one = NR.in_bwd_ref(r.dy, r.x, r.scale, r.shift, slope, S=two.S, dx_add=r.dx_add)
    _, dx16, xa16 = _apply_ex(hip, dyd, xd, scd, shd, slope, _dev(two.S.contiguous()), addd, False, True, True)
    rep("apply_ex dx16 <011>", NR.bf16_ratio(dx16, *NR.bf16_hull(one.dx, one.dx_alt, one.B)))
    a_lo, a_hi = NR.act_h_ref(r.x, r.scale, r.shift, slope)
    rep("apply_ex xa16 <011>", NR.bf16_ratio(xa16, R.hi(a_lo), R.hi(a_hi)))
    rep("to_bf16", NR.bf16_ratio(hip.to_bf16(xd, scd, shd, slope), R.hi(a_lo), R.hi(a_hi)))
    rep.done()


# ------------------------------------------------------------------ strided outputs through the C ABI
def test_strided_outputs_leave_their_neighbours_alone(hip):
    """y (y_ldc) and dx (dx_ldc) written into the slice [..., 16:48] of a 64-wide buffer pre-filled with a sentinel: the slice is
    within its bound, every other float of the buffer keeps its bits"""
    N, dims, C = 2, (5, 6, 9), 32
    r = with_reference_stats(make_inputs(N, dims, C))
    rep = Report("strided-n2-5x6x9-c32")
    xd, dyd, resd, addd, scd, shd = (_dev(t) for t in (r.x, r.dy, r.residual, r.dx_add, r.scale, r.shift))
    slope = 0.01
    sentinel = -12345.678

    def buf():
        return torch.full((N,) + dims + (64,), sentinel, device=DEV)

    def neighbours_untouched(b):
        return bool((b[..., :16] == sentinel).all()) and bool((b[..., 48:] == sentinel).all())
    yb = buf()
    hip._call("cwf_norm_act_add_ex", xd.data_ptr(), C, scd.data_ptr(), shd.data_ptr(), slope, resd.data_ptr(), C,
              yb[..., 16:48].data_ptr(), 64, 0, N, r.V, C, hip._stream())
    y, ya, B, _ = NR.norm_act_add_ref(r.x, r.scale, r.shift, slope, r.residual)
    rep("norm_act_add y_ldc 64", NR.ratio(yb[..., 16:48], y, B, alt=ya))
    assert neighbours_untouched(yb), "norm_act_add wrote outside its channel slice"
    S = NR.bwd_sums_ref(r.dy, r.x, r.scale, r.shift, slope)[0].contiguous()
    Sd = _dev(S)
    one = NR.in_bwd_ref(r.dy, r.x, r.scale, r.shift, slope, S=S, dx_add=r.dx_add)
    for name, extra in (("cwf_in_bwd_apply", ()), ("cwf_in_bwd_apply_ex", (0, 0))):
        db = buf()
        hip._call(name, dyd.data_ptr(), C, xd.data_ptr(), C, scd.data_ptr(), shd.data_ptr(), slope, Sd.data_ptr(), addd.data_ptr(), C,
                  db[..., 16:48].data_ptr(), 64, *extra, N, r.V, C, hip._stream())
        rep(name + " dx_ldc 64", NR.ratio(db[..., 16:48], one.dx, one.B, alt=one.dx_alt))
        assert neighbours_untouched(db), name + " wrote outside its channel slice"
    rep.done()


# ------------------------------------------------------------------ refusals (return codes only; nothing is launched)
def test_refusals(hip):
    lib, st = hip.lib, hip._stream()
    N, V = 1, 8
    buf = torch.zeros(N * V * 1032 + 8, device=DEV)
    sums = torch.zeros(N * 1032 * 2, dtype=torch.float64, device=DEV)
    sc = torch.ones(N * 1032, device=DEV)
    b16 = torch.zeros(N * V * 1032, dtype=torch.bfloat16, device=DEV)
    p, ps, pc, p16 = buf.data_ptr(), sums.data_ptr(), sc.data_ptr(), b16.data_ptr()

    def stats(ptr, ldc, c):
        return lib.cwf_in_stats(ptr, ldc, ps, N, V, c, st)

    def bwd_stats(ptr, ldc, c, scale=pc):
        return lib.cwf_in_bwd_stats(ptr, ldc, ptr, ldc, scale, pc, 0.01, ps, N, V, c, st)

    def naa(ptr, ldc, c, scale=pc):
        return lib.cwf_norm_act_add_ex(ptr, ldc, scale, pc, 0.01, 0, 0, p, ldc, 0, N, V, c, st)

    def apply_ex(ptr, ldc, c, scale=pc, dx=p, dx16=0):
        return lib.cwf_in_bwd_apply_ex(ptr, ldc, ptr, ldc, scale, pc, 0.01, ps, 0, 0, dx, ldc, dx16, 0, N, V, c, st)

    def to16(ptr, ldc, c):
        return lib.cwf_to_bf16(ptr, ldc, pc, pc, 0.01, p16, N, V, c, st)
    for f in (stats, bwd_stats, naa, apply_ex, to16):
        assert f(p, 1028, 1028) == E_TOOLARGE, f.__name__
        assert f(p, 8, 6) == E_ALIGN, f.__name__               # C % 4
        assert f(p, 18, 16) == E_ALIGN, f.__name__             # ldc % 4
        assert f(p + 4, 16, 16) == E_ALIGN, f.__name__         # a pointer off by 4 bytes
        assert f(p, 12, 16) == E_ALIGN, f.__name__             # ldc < C
        assert f(0, 16, 16) == E_BADARG, f.__name__
    for f in (bwd_stats, naa, apply_ex):
        assert f(p, 16, 16, scale=0) == E_BADARG, f.__name__   # NULL scale
    assert apply_ex(p, 16, 16, dx=0, dx16=0) == E_BADARG       # neither output
    assert lib.cwf_in_bwd_apply(p, 16, p, 16, pc, pc, 0.01, ps, 0, 0, 0, 16, N, V, 16, st) == E_BADARG
    assert apply_ex(p, 16, 16, dx=0, dx16=p16 + 2) == E_ALIGN  # bf16 image off its 8 bytes
    assert lib.cwf_in_finalize(0, pc, pc, 16, V, 1e-5, st) == E_BADARG
    assert lib.cwf_stats_channel_sum(ps, 0, 1, 16, st) == E_BADARG
    torch.cuda.synchronize()
    assert float(buf.abs().sum()) == 0.0 and float(sums.abs().sum()) == 0.0, "a refused call wrote"


# ------------------------------------------------------------------ the two forms of h see the same sign
@pytest.mark.parametrize("case", [(3, (11, 13, 17), 16), (2, (5, 10, 20), 96), (2, (32, 32, 32), 64)], ids=_id)
def test_the_two_forms_of_h_agree_on_the_sign(hip, case):
    """norm_act_add_kernel writes h as a plain multiply-add, in_bwd_apply_kernel as fmaf; act'(h) is a step at 0.  Outside the
    sign-ambiguous mask both must see the sign of h_ref on every element (slope 0: y > 0 and xa16 > 0 are that sign)."""
    N, dims, C = case
    r = with_reference_stats(make_inputs(N, dims, C))
    xd, dyd, scd, shd = (_dev(t) for t in (r.x, r.dy, r.scale, r.shift))
    h, e, amb = NR.h_ref(r.x, r.scale, r.shift)
    plain = NR.flat(hip.norm_act_add(xd, scd, shd, 0.0)) > 0
    S = hip.in_stats(dyd)
    fused = NR.flat(_apply_ex(hip, dyd, xd, scd, shd, 0.0, S, None, True, False, True)[2].float()) > 0
    want = h > 0
    # (an h below the smallest bf16 subnormal would round xa16 to 0: none of these inputs comes near, e is ~1e-7 at the least)
    assert bool(((plain == want) | amb).all()), int(((plain != want) & ~amb).sum())
    assert bool(((fused == want) | amb).all()), int(((fused != want) & ~amb).sum())
    live = (~r.degen)[:, None, :].expand_as(amb)
    assert float((amb & live).sum()) / max(1, int(live.sum())) <= NR.AMBIGUOUS_CAP
