"""cwf_conv_x16_ok (host code of libcwf_hip.so, no GPU needed): the one predicate that says whether a single-bf16 3x3x3 stride-1 launch may be
handed its input as a bf16 image alone.  cwf_conv evaluates the same function, so a "yes" here is a launch that reads the image and a "no" is
CWF_E_BADARG -- never a launch that reads an fp32 gradient nobody wrote (the GPU side of that: tests/test_conv_ws_image_gpu.py)."""
import ctypes
import os
import re

import pytest

from cwf import _lib

S1 = 0          # CWF_CONV3_S1
HDR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "cwf_hip.h")


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def test_benchmark_layers(lib):
    """the data gradients of the benchmark step (batch 2 at 128^3): arguments are those of the LAUNCH (N, D, H, W, Cin, Cout)"""
    ok = lib.cwf_conv_x16_ok
    assert ok(S1, 2, 64, 64, 64, 32, 32) == 1
    assert ok(S1, 2, 32, 32, 32, 64, 64) == 1
    assert ok(S1, 2, 128, 128, 128, 16, 16) == 1
    assert ok(S1, 2, 16, 16, 16, 128, 128) == 0          # 32 tiles x 4 output groups: below the 256-unit occupancy threshold


def test_rejections(lib):
    ok = lib.cwf_conv_x16_ok
    assert ok(S1, 2, 64, 64, 64, 32, 32) == 1
    for op in (1, 2, 3, 4, 5):                          # stride 2, 1x1x1, ConvTranspose and the two data-gradient-only ops
        assert ok(op, 2, 64, 64, 64, 32, 32) == 0
    assert ok(S1, 2, 62, 64, 64, 32, 32) == 0            # D no multiple of 4
    assert ok(S1, 2, 64, 66, 64, 32, 32) == 0            # H no multiple of 4
    assert ok(S1, 2, 64, 64, 72, 32, 32) == 0            # W no multiple of 16
    assert ok(S1, 2, 64, 64, 64, 16, 32) == 0            # Cin < 32 (other than 16 -> 16)
    assert ok(S1, 2, 64, 64, 64, 8, 32) == 0
    assert ok(S1, 2, 64, 64, 64, 40, 32) == 0            # Cin no multiple of 16
    assert ok(S1, 2, 64, 64, 64, 32, 16) == 0            # Cout no multiple of 32
    assert ok(S1, 2, 64, 64, 64, 32, 48) == 0
    assert ok(S1, 0, 64, 64, 64, 32, 32) == 0
    assert ok(S1, 2, 16, 16, 16, 16, 16) == 0            # 16 -> 16 below 32768 voxels
    assert ok(S1, 2, 32, 32, 32, 16, 16) == 1


def test_image_must_stay_below_4_gib(lib):
    """the kernel forms 32-bit byte offsets into the image: N * D * H * W * Cin * 2 bytes < 2^32"""
    ok = lib.cwf_conv_x16_ok
    assert ok(S1, 1, 256, 256, 512, 32, 32) == 1         # 2^31 bytes
    assert ok(S1, 1, 256, 256, 1008, 32, 32) == 1        # just below 2^32
    assert ok(S1, 1, 256, 256, 1024, 32, 32) == 0        # 2^32 bytes
    assert ok(S1, 2, 256, 256, 512, 64, 64) == 0         # 2^33 bytes
    assert ok(S1, 2, 1024, 1024, 512, 16, 16) == 0       # 16 -> 16: 2^30 voxels


def test_debug_knob_moves_the_threshold(lib):
    ok = lib.cwf_conv_x16_ok
    small = (S1, 2, 8, 8, 32, 32, 64)                    # 16 tiles x 2 groups
    assert ok(*small) == 0
    old = lib.cwf_debug_ws_min_units(1)
    try:
        assert old == 256
        assert ok(*small) == 1
        assert ok(S1, 2, 16, 16, 16, 128, 128) == 1
        assert ok(S1, 2, 8, 8, 32, 16, 32) == 0          # the channel conditions do not move
        lib.cwf_debug_ws_min_units(33)
        assert ok(*small) == 0
        lib.cwf_debug_ws_min_units(32)
        assert ok(*small) == 1
    finally:
        lib.cwf_debug_ws_min_units(old)
    assert ok(*small) == 0
    assert ok(S1, 2, 64, 64, 64, 32, 32) == 1


def test_header_and_binding_agree():
    hdr = re.sub(r"/\*.*?\*/", " ", open(HDR).read(), flags=re.S)
    m = re.search(r"\bint\s+cwf_conv_x16_ok\s*\(([^)]*)\)\s*;", hdr)
    assert m, "cwf_conv_x16_ok is not declared in include/cwf_hip.h"
    params = [p.strip() for p in m.group(1).split(",")]
    assert [p.rsplit(None, 1)[0] for p in params] == ["int"] * 7, params
    assert [p.rsplit(None, 1)[1] for p in params] == ["op", "N", "D", "H", "W", "Cin", "Cout"], params
    assert _lib.SIGNATURES["cwf_conv_x16_ok"] == [ctypes.c_int] * 7
    assert "cwf_conv_x16_ok" not in _lib.RESTYPE_INT64
