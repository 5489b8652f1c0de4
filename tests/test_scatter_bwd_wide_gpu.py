"""GPU: scatter_bwd's narrow-block kernel (scatter_bwd_wide_kernel, csrc/tokens.hip: 8 / 16 / 32 columns per workgroup, the loads of
16 rows per thread ahead of the adds) against scatter_bwd_kernel (64 columns per workgroup), bit for bit: dgate is summed in the same
chains -- 16 row lanes in ascending row order, the 16 partials in order, then dgate_extra -- and drows keeps its arithmetic.  Outputs sit
inside wider buffers whose other elements must come back untouched; inv has hits and misses."""
import itertools

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROUTES = (1, 8, 16, 32)       # the product route and every column width, each against route 0


def _u(*shape, seed, s=1.0):
    g = torch.Generator().manual_seed(seed)
    return ((torch.rand(*shape, generator=g) * 2 - 1) * s).float().to(DEV)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _selection(B, T, k, seed):
    """index [B, k] (distinct tokens while k <= T) and its inverse map inv [B, T]: position in the selection, or -1"""
    g = torch.Generator().manual_seed(seed)
    index = torch.stack([torch.randperm(max(T, k), generator=g)[:k] % T for _ in range(B)]).to(torch.int32)
    inv = torch.full((B, T), -1, dtype=torch.int32)
    for b in range(B):
        for j in range(k):
            inv[b, int(index[b, j])] = j
    return index.to(DEV), inv.to(DEV)


def _case(hip, B, T, k, E, use_g, use_s, use_x, seed):
    feats = _u(B, T, E, seed=seed)
    index, inv = _selection(B, T, k, seed + 1)
    Rm = _u(B, 1 + k, E, seed=seed + 2)                        # gate row, then the k selected rows (the couplers' layout)
    rows, gate = Rm[:, 1:], Rm[:, 0:1]
    dgated = _u(B, T, E, seed=seed + 3) if use_g else None
    dscat = _u(B, T, E, seed=seed + 4) if use_s else None
    extra = _u(B, 1, E, seed=seed + 5) if use_x else None
    fill = _u(B, 3 + k, E + 8, seed=seed + 6)                  # dgate at row 1, drows at rows 2 .. 2 + k, columns [4, 4 + E)
    out = {}
    for route in (0,) + ROUTES:
        buf = fill.clone()
        drows, dgate = buf[:, 2:2 + k, 4:4 + E], buf[:, 1:2, 4:4 + E]
        old = hip.lib.cwf_debug_scatter_bwd(route)
        try:
            hip.scatter_bwd(dgated, dscat, feats, inv, index, rows, gate, extra, drows, dgate)
            torch.cuda.synchronize()
        finally:
            hip.lib.cwf_debug_scatter_bwd(old)
        out[route] = buf
    tag = "B=%d T=%d k=%d E=%d dgated=%d dscat=%d extra=%d" % (B, T, k, E, use_g, use_s, use_x)
    ref = out[0]
    guard = torch.ones_like(fill, dtype=torch.bool)
    guard[:, 1:2 + k, 4:4 + E] = False
    assert torch.equal(_bits(ref)[guard], _bits(fill)[guard]), (tag, "route 0 wrote a guard band")
    for route in ROUTES:
        got = out[route]
        assert torch.equal(_bits(got)[guard], _bits(fill)[guard]), (tag, route, "guard band written")
        mism = int((_bits(got[:, 2:2 + k, 4:4 + E]) != _bits(ref[:, 2:2 + k, 4:4 + E])).sum())
        assert mism == 0, (tag, route, "drows elements whose bit patterns differ", mism)
        mism = int((_bits(got[:, 1, 4:4 + E]) != _bits(ref[:, 1, 4:4 + E])).sum())
        assert mism == 0, (tag, route, "dgate elements whose bit patterns differ", mism)
    if use_g:                                                  # the comparison is of computed values, not of two untouched buffers
        assert not torch.equal(_bits(ref[:, 1, 4:4 + E]), _bits(fill[:, 1, 4:4 + E])), tag


@pytest.mark.parametrize("E", [64, 128, 512])
@pytest.mark.parametrize("T", [1, 15, 16, 17, 63, 64, 65, 300])
def test_bit_equal_to_the_64_column_kernel(hip, T, E):
    seed = T * 13 + E
    for k, B in itertools.product((1, 8), (1, 3)):
        for use_g, use_s, use_x in itertools.product((True, False), repeat=3):
            _case(hip, B, T, k, E, use_g, use_s, use_x, seed)
            seed += 7


def test_switch_returns_previous_value(hip):
    assert hip.lib.cwf_debug_scatter_bwd(0) == 1               # the product route is the default
    assert hip.lib.cwf_debug_scatter_bwd(16) == 0
    assert hip.lib.cwf_debug_scatter_bwd(5) == 16              # not a route: unchanged
    assert hip.lib.cwf_debug_scatter_bwd(1) == 16
