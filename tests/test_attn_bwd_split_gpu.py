"""GPU: the attention backward pass in two launches (cwf_attn_bwd_ws, csrc/attn.hip: attn_bwd_rows_kernel per query tile, then
attn_bwd_keys_kernel per key tile) against the one-launch attn_bwd_kernel, bit for bit: every element is the same chain of operations
in both, nothing is summed across workgroups.  dqkv sits in guard bands, the workspace is NaN before the call (launch B may read
nothing launch A did not write) and has a canary band behind its stated size.  The route is proved by the launch counter.  On top:
the float64 bound of tests/token_ref.py on the new route, the refusals of a bad workspace, and determinism."""
import ctypes

import pytest
import torch

import token_ref as R
from oracle.kernel_emul import EmulBackend

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BADARG = -1
CANARY = 4321.5
GUARD = 3                     # rows of guard band before and behind dqkv


def _u(*shape, seed, s=1.0):
    g = torch.Generator().manual_seed(seed)
    return ((torch.rand(*shape, generator=g) * 2 - 1) * s).float().to(DEV)


def _bits(t):
    return t.contiguous().view(torch.int32)


class Case:
    def __init__(self, hip, Z, T, heads, p, seed):
        self.hip, self.Z, self.T, self.heads, self.p = hip, Z, T, heads, p
        self.e = e = heads * 64
        self.ld, self.ldo = 3 * e + 8, e + 4                     # ld > 3E, ldo > E
        self.qkv = _u(Z * T, self.ld, seed=seed)
        self.d_o = _u(Z * T, self.ldo, seed=seed + 1)
        self.off = 901 + seed                                    # non-zero drop_off
        self.fill = _u(Z * T + 2 * GUARD, self.ld, seed=seed + 2)
        self.need = int(hip.lib.cwf_attn_bwd_ws_bytes(Z, T, heads))
        assert self.need == 2 * Z * heads * ((T + 31) // 32 * 32) * 144 * 4

    def run(self, route, waves=None, ws=None, ws_bytes=None):
        """one call of cwf_attn_bwd_ws under cwf_debug_attn_split(route); returns (status, dqkv buffer with its guard rows, split launches, ws)"""
        hip = self.hip
        buf = self.fill.clone()
        dqkv = buf[GUARD:GUARD + self.Z * self.T]
        if ws is None:
            ws = torch.full((self.need // 4 + 256,), float("nan"), device=DEV)
            ws[self.need // 4:] = CANARY
        old = hip.lib.cwf_debug_attn_split(route)
        oldw = hip.lib.cwf_debug_attn_split_waves(waves if waves else 0)
        try:
            n0 = hip.lib.cwf_debug_attn_split_launches()
            rc = hip.lib.cwf_attn_bwd_ws(self.qkv.data_ptr(), self.ld, self.d_o.data_ptr(), self.ldo, dqkv.data_ptr(), self.Z, self.T, self.e,
                                         self.heads, ctypes.c_float(64 ** -0.5), hip.rng(DEV).data_ptr(), ctypes.c_uint64(self.off),
                                         ctypes.c_float(self.p), ws if isinstance(ws, int) else ws.data_ptr(),
                                         self.need if ws_bytes is None else ws_bytes, ctypes.c_void_p(hip._stream()))
            torch.cuda.synchronize()
            took = hip.lib.cwf_debug_attn_split_launches() - n0
        finally:
            hip.lib.cwf_debug_attn_split(old)
            hip.lib.cwf_debug_attn_split_waves(oldw)
        return rc, buf, took, ws

    def untouched(self, buf):
        """guard rows and the padding columns behind 3E are as before the call"""
        f = self.fill
        return (torch.equal(_bits(buf[:GUARD]), _bits(f[:GUARD])) and torch.equal(_bits(buf[-GUARD:]), _bits(f[-GUARD:]))
                and torch.equal(_bits(buf[:, 3 * self.e:]), _bits(f[:, 3 * self.e:])))


def _equal_routes(hip, Z, T, heads, p, seed, waves=None):
    c = Case(hip, Z, T, heads, p, seed)
    tag = "Z=%d T=%d heads=%d p=%g waves=%s" % (Z, T, heads, p, waves)
    rc0, old, took0, _ = c.run(0)
    rc1, new, took1, ws = c.run(1, waves)
    assert rc0 == 0 and rc1 == 0, tag
    assert took0 == 0 and took1 == 1, (tag, "route", took0, took1)
    mism = int((_bits(old) != _bits(new)).sum())
    assert mism == 0, (tag, "elements whose bit patterns differ", mism)
    assert c.untouched(new) and c.untouched(old), (tag, "guard band written")
    assert not bool(torch.isnan(new[GUARD:-GUARD, :3 * c.e]).any()), (tag, "NaN from the poisoned workspace")
    assert bool((ws[c.need // 4:] == CANARY).all()), (tag, "written behind the workspace's stated size")
    return c, new


@pytest.mark.parametrize("heads", [1, 2, 8])
@pytest.mark.parametrize("T", [1, 31, 32, 33, 129, 144])
def test_bit_equal_to_one_launch_kernel(hip, T, heads):
    for Z in (1, 3):
        for p in (0.0, 0.1):
            _equal_routes(hip, Z, T, heads, p, seed=T * 7 + heads + Z)


@pytest.mark.parametrize("waves", [4, 8, 16])
def test_bit_equal_at_every_wave_count(hip, waves):
    for T in (33, 129):
        _equal_routes(hip, 3, T, 2, 0.1, seed=50 + T, waves=waves)


@pytest.mark.parametrize("T", [33, 129])
def test_float64_bound_on_the_split_route(hip, T):
    Z, heads = 2, 8
    for p in (0.0, 0.1):
        E = EmulBackend()
        seed, step = hip.rng(DEV).cpu().tolist()
        E.set_rng(seed, step)
        c, buf = _equal_routes(hip, Z, T, heads, p, seed=300 + T)
        got = buf[GUARD:-GUARD]
        mask = R.attn_mask(E, Z, T, heads, c.off, p)
        (dq, dk, dv), (Aq, Ak, Av) = R.attn_bwd(c.qkv, c.d_o, Z, T, heads, mask)
        e = c.e
        for name, g_, ref, A in (("dQ", got[:, :e], dq, Aq), ("dK", got[:, e:2 * e], dk, Ak), ("dV", got[:, 2 * e:3 * e], dv, Av)):
            r = R.ratio(g_, ref, R.GAMMA_ATTN * A)
            print("  split attn bwd %s T=%d p=%g: err / (GAMMA_ATTN A) = %.3f  (err / (GAMMA_ATTN_BWD A) = %.3f)"
                  % (name, T, p, r, r * R.GAMMA_ATTN / R.GAMMA_ATTN_BWD))
            assert R.worst(g_, ref, R.GAMMA_ATTN * A, "split attn bwd " + name) <= 1.0


def test_refusals_leave_dqkv_untouched(hip):
    c = Case(hip, 2, 33, 2, 0.1, seed=11)
    good = torch.full((c.need // 4 + 8,), float("nan"), device=DEV)
    for what, ws, nbytes in (("too small", good, c.need - 4), ("null", 0, c.need), ("misaligned", good.data_ptr() + 4, c.need)):
        for route in (1, 0):
            rc, buf, took, _ = c.run(route, ws=ws, ws_bytes=nbytes)
            assert rc == BADARG, (what, route, rc)
            assert took == 0, (what, route)
            assert torch.equal(_bits(buf), _bits(c.fill)), (what, route, "dqkv written by a refused call")
    assert bool(torch.isnan(good).all()), "workspace written by a refused call"


def test_switch_returns_previous_value(hip):
    assert hip.lib.cwf_debug_attn_split(0) == 1                 # the product route is the default
    assert hip.lib.cwf_debug_attn_split(1) == 0
    w = hip.lib.cwf_debug_attn_split_waves(0)                   # 0: unchanged
    assert w in (4, 8, 16) and hip.lib.cwf_debug_attn_split_waves(w) == w


def test_determinism(hip):
    c = Case(hip, 3, 129, 8, 0.1, seed=77)
    _, a, ta, _ = c.run(1)
    _, b, tb, _ = c.run(1)
    assert ta == 1 and tb == 1
    assert torch.equal(_bits(a), _bits(b))


def test_backend_attn_bwd_takes_the_split_route(hip):
    """HipBackend.attn_bwd hands its persistent workspace to cwf_attn_bwd_ws"""
    Z, T, heads = 2, 33, 2
    qkv, d_o = _u(Z * T, 3 * heads * 64, seed=5), _u(Z * T, heads * 64, seed=6)
    n0 = hip.lib.cwf_debug_attn_split_launches()
    new = hip.attn_bwd(qkv, d_o, Z, T, heads, (123, 0.1))
    assert hip.lib.cwf_debug_attn_split_launches() - n0 == 1
    old = hip.lib.cwf_debug_attn_split(0)
    try:
        ref = hip.attn_bwd(qkv, d_o, Z, T, heads, (123, 0.1))
    finally:
        hip.lib.cwf_debug_attn_split(old)
    assert hip.lib.cwf_debug_attn_split_launches() - n0 == 1
    assert torch.equal(_bits(new), _bits(ref))
