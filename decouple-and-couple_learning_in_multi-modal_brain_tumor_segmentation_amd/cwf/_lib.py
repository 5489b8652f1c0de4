"""ctypes binding of libcwf_hip.so (include/cwf_hip.h).  The product path has NO fallback: if the
library is missing this raises, and every wrapper raises on a non-zero status."""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libcwf_hip.so")

P = C.c_void_p
I = C.c_int
L = C.c_int64
F = C.c_float
U = C.c_uint32
U64 = C.c_uint64
D = C.c_double

# name -> argtypes, exactly as declared in include/cwf_hip.h
SIGNATURES = {
    "cwf_version": [],
    "cwf_conv": [P, P],
    "cwf_conv_x16_ok": [I, I, I, I, I, I, I],
    "cwf_debug_wsd": [I],
    "cwf_debug_wsd_launches": [],
    "cwf_wgrad": [P, P, P],
    "cwf_debug_wgrad_bf16_plan": [P, P],
    "cwf_debug_wgrad_bf16_name": [I],              # returns const char* (restype set in load())
    "cwf_debug_wgrad_s2": [I],
    "cwf_debug_wgrad_s2_launches": [],
    "cwf_gather_split_bf16": [P, I, L, P],
    "cwf_wgrad_nsplit": [I, I, I, I, I, I, I],
    "cwf_wgrad_partial_floats": [I, I, I, I, I, I, I],
    "cwf_wgrad_slab_floats": [I, I, I],
    "cwf_wgrad_reduce": [P, I, L, P, P, P, P],
    "cwf_gather_batched": [P, I, L, P],
    "cwf_in_finalize": [P, P, P, I, L, F, P],
    "cwf_in_stats": [P, I, P, I, L, I, P],
    "cwf_norm_act_add": [P, I, P, P, F, P, I, P, I, I, L, I, P],
    "cwf_in_bwd_stats": [P, I, P, I, P, P, F, P, I, L, I, P],
    "cwf_in_bwd_apply": [P, I, P, I, P, P, F, P, P, I, P, I, I, L, I, P],
    "cwf_in_bwd_apply_ex": [P, I, P, I, P, P, F, P, P, I, P, I, P, P, I, L, I, P],
    "cwf_norm_act_add_ex": [P, I, P, P, F, P, I, P, I, P, I, L, I, P],
    "cwf_to_bf16": [P, I, P, P, F, P, I, L, I, P],
    "cwf_gemm": [P, L, L, L, L, P, L, L, L, L, P, L, L, L, P, P, L, L, L, I, I, I, I, I, F, I, I, P],
    "cwf_layernorm_fwd": [P, P, P, P, P, P, I, I, F, P],
    "cwf_layernorm_bwd": [P, P, P, P, P, P, P, P, I, I, I, P],
    "cwf_softmax_rows": [P, L, I, I, P],
    "cwf_softmax_rows_bwd": [P, P, L, I, I, P],
    "cwf_gelu_bwd": [P, P, P, L, P],
    "cwf_colsum": [P, L, I, I, P, I, P],
    "cwf_window_to_tokens": [P, I, P, I, I, I, I, I, I, I, I, P],
    "cwf_tokens_to_window": [P, P, I, I, I, I, I, I, I, I, I, I, P],
    "cwf_token_scores": [P, P, L, P, I, I, I, P],
    "cwf_topk": [P, P, I, I, I, P],
    "cwf_gather_tokens": [P, P, P, L, P, F, P, I, I, I, I, P],
    "cwf_gather_tokens_bwd": [P, P, P, P, P, L, I, I, I, I, P],
    "cwf_scatter_rows": [P, P, P, L, L, P, L, P, I, I, I, I, P],
    "cwf_scatter_rows_bwd": [P, P, P, P, L, P, I, P, L, L, P, L, I, I, I, I, P],
    "cwf_upsample_softmax": [P, I, P, I, I, I, I, I, I, P],
    "cwf_upsample_softmax_bwd": [P, P, P, I, I, I, I, I, I, I, P, P],
    "cwf_channel_softmax": [P, I, P, L, I, P],
    "cwf_channel_softmax_bwd": [P, P, P, I, L, I, P],
    "cwf_dice_ce_sums": [P, P, U, P, I, L, I, P],
    "cwf_dice_ce_finalize": [P, P, P, I, L, I, P],
    "cwf_dice_ce_bwd": [P, P, U, P, P, P, I, L, I, P],
    "cwf_adam_amsgrad": [P, I, L, C.c_double, C.c_double, C.c_double, C.c_double, C.c_double, I, I, P, P],
    "cwf_adam_amsgrad_scaled": [P, I, L, C.c_double, C.c_double, C.c_double, C.c_double, C.c_double, I, I, P, F, P],
    "cwf_grad_add": [P, P, P, L, P],
    "cwf_grad_norm_clip": [P, L, F, F, P, P, P],
    "cwf_adam_amsgrad_ex": [P, I, L, C.c_double, C.c_double, C.c_double, C.c_double, C.c_double, I, I, P, F, P, P, F, P],
    "cwf_optim_step": [I, P, I, L, C.c_double, C.c_double, P, C.c_double, C.c_double, C.c_double, I, I, P, C.c_double, C.c_double, I, I,
                       F, P, P, F, P],
    "cwf_wgrad_reduce_batched": [P, I, P],
    "cwf_dropout_mask": [P, L, F, F, C.c_uint64, C.c_uint64, P],
    "cwf_mul": [P, P, P, L, P],
    "cwf_add": [P, P, P, L, P],
    "cwf_channel_scale": [P, I, P, P, I, I, L, I, P],
    "cwf_copy_strided": [P, I, P, I, L, I, P],
    "cwf_add3": [P, P, P, P, L, P],
    "cwf_bcast3": [P, P, L, P],
    "cwf_stats_channel_sum": [P, P, I, I, P],
    "cwf_gemm_ex": [P, P],
    "cwf_debug_gemm_panel": [I],
    "cwf_debug_gemm_panel_launches": [],
    "cwf_attn_fwd": [P, L, P, L, I, I, I, I, F, P, U64, F, P],
    "cwf_attn_bwd": [P, L, P, L, P, I, I, I, I, F, P, U64, F, P],
    "cwf_attn_bwd_ws": [P, L, P, L, P, I, I, I, I, F, P, U64, F, P, L, P],
    "cwf_attn_bwd_ws_bytes": [I, I, I],
    "cwf_debug_attn_split": [I],
    "cwf_debug_attn_split_waves": [I],
    "cwf_debug_attn_split_launches": [],
    "cwf_ln_pair_fwd": [P, P, I, P, P, P, P, P, P, P, I, I, F, P],
    "cwf_ln_pair_bwd": [P, P, P, P, P, I, P, P, P, P, P, P, P, P, P, I, I, I, P],
    "cwf_gelu_bwd_drop": [P, P, P, L, P, U64, F, P],
    "cwf_token_scores2": [P, P, L, P, L, P, P, I, I, I, P],
    "cwf_topk_inv": [P, P, P, P, P, P, I, I, I, P],
    "cwf_index_inv": [P, P, I, I, I, P],
    "cwf_gather_multi": [P, I, I, I, I, F, P, F, P],
    "cwf_scatter_inv": [P, P, P, L, L, P, L, P, P, I, I, I, P],
    "cwf_scatter_bwd": [P, P, P, P, P, P, L, L, P, L, P, L, P, L, L, P, L, I, I, I, I, P],
    "cwf_debug_scatter_bwd": [I],
    "cwf_token_grad": [P, P, P, L, P, P, P, L, P, L, P, U64, U64, F, P, I, I, I, I, P],
    "cwf_head_grad": [P, P, P, P, L, P, P, I, I, P],
    "cwf_dice_ce_finalize_multi": [P, P, P, P, I, I, L, I, P],
    "cwf_head_loss_sums": [P, I, I, P, P, P, I, I, I, I, I, P],
    "cwf_head_loss_bwd": [P, I, I, P, P, P, P, P, I, P, I, I, I, I, I, P],
    "cwf_head_loss_bwd_ex": [P, I, I, P, P, P, P, P, I, I, P, I, I, I, I, I, P],
    "cwf_ln_pair_fwd_g": [P, P, I, P, I, P, P, P, I, I, F, P],
    "cwf_ln_pair_bwd_g": [P, P, P, P, P, I, P, I, P, P, P, I, I, I, P],
    "cwf_token_scores2_g": [P, P, P, I, I, P, P, I, I, I, P],
    "cwf_head_grad_g": [P, P, P, P, L, P, P, I, I, I, P],
    "cwf_window_to_tokens_g": [P, I, P, I, I, I, I, I, I, I, I, I, P],
    "cwf_tokens_to_window_g": [P, P, I, I, I, I, I, I, I, I, I, I, P],
    "cwf_cat3_channels": [P, P, P, P, L, I, P],
    "cwf_stitch_windows": [P, P, I, P],
    "cwf_argmax_dice": [P, L, L, L, P, P, P, I, L, P],
    "cwf_argmax_metrics": [P, L, L, L, P, P, P, I, L, P],
    "cwf_region_bits": [P, P, L, P],
    "cwf_hausdorff_workspace": [I, I, I, I, I],
    "cwf_hausdorff": [P, P, I, I, I, I, I, D, D, D, I, I, P, P, P, P, L, P],
    "cwf_surface_metrics_workspace": [I, I, I, I, I],
    "cwf_surface_metrics": [P, P, I, I, I, I, I, D, D, D, I, I, P, I, P, P, P, P, P, P, P, P, L, P],
    "cwf_signed_distance_workspace": [I, I, I, I, I],
    "cwf_signed_distance": [P, P, P, I, I, I, I, I, P, P],
    "cwf_boundary_sums": [P, P, P, P, I, I, L, I, P],
    "cwf_boundary_finalize": [P, P, P, P, I, I, L, P],
    "cwf_boundary_bwd": [P, P, P, P, P, I, I, L, I, P],
    "cwf_topk_ce_workspace": [I, L],
    "cwf_topk_ce": [P, P, U, L, P, P, P, I, L, I, P, P],
    "cwf_topk_ce_bwd": [P, P, U, P, P, P, I, L, I, P],
    "cwf_focal_workspace": [I, L, I],
    "cwf_focal_loss": [P, P, P, I, P, P, P, P, I, L, I, P, P],
    "cwf_focal_loss_bwd": [P, P, P, I, P, P, P, P, I, L, I, P],
    "cwf_lovasz_workspace": [I, L, I],
    "cwf_lovasz": [P, P, P, I, I, P, P, P, P, I, L, P, P],
    "cwf_lovasz_bwd": [P, P, I, P, P, P, I, L, P],
    "cwf_components_workspace": [I, I, I, I, I],
    "cwf_components": [P, I, I, I, I, I, I, P, P, P, P, P, L, P],
    "cwf_postprocess_labels": [P, P, P, P, P, I, I, I, I, I, I, I, I, I, I, I, I, P, P, P],
    "cwf_label_metrics": [P, P, P, L, P],
    "cwf_dilate_bits": [P, P, I, I, I, I, I, I, P, L, P],
    "cwf_lesionwise_workspace": [I, I, I, I, I],
    "cwf_lesionwise": [P, P, I, I, I, I, I, I, L, D, P, P, P, P, P, P, L, P],
    "cwf_lesionwise_ex_workspace": [I, I, I, I, I],
    "cwf_lesionwise_ex": [P, P, I, I, I, I, I, I, L, D, P, I, P, P, P, P, P, P, P, P, L, P],
    "cwf_prepare_batch": [P, I, I, I, I, P, L, P, L, P, L, P],
    "cwf_prepare_batch_affine": [P, I, I, I, I, P, L, P, L, P, L, P],
    "cwf_prepare_batch_elastic": [P, I, I, I, I, P, L, P, L, P, L, P],
    "cwf_augment_intensity": [P, I, I, I, I, P, L, P, L, P, L, P],
    "cwf_augment_acquisition": [P, I, I, I, I, P, L, P, L, P, L, P],
    "cwf_window_gather": [P, P, P, I, I, P],
    "cwf_window_blend": [P, P, P, P, I, I, I, P],
    "cwf_window_finalize": [P, P, P, P, P],
    "cwf_window_gather_box": [P, P, P, P, I, I, P],
    "cwf_window_finalize_box": [P, P, P, P, P, P],
    "cwf_normalize_nonzero": [P, L, P, P],
    "cwf_class_locations_workspace": [L, I],
    "cwf_class_locations": [P, L, P, I, I, P, P, P, P],
    "cwf_nonzero_box_workspace": [I, I, I, I],
    "cwf_nonzero_box": [P, L, I, I, I, I, P, P, P, P],
    "cwf_rng_advance": [P, P],
    "cwf_dropout_mask_rng": [P, L, F, F, P, U64, P],
    "cwf_plan_create": [P, P],
    "cwf_plan_info": [P, P],
    "cwf_plan_run": [P, P, P, I, P, P],
    "cwf_plan_destroy": [P],
    "cwf_plan_marker": [I, P],
    "cwf_plan_schedule": [I, P, P, I, P, P, P, P, P, P, P],
    "cwf_plan_counts": [P, P],
    "cwf_plan_describe": [P, P, P, P, P, P, P, P, P, P],
    "cwf_plan_kernel_name": [P, I, P, I],
}

PLAN_KERNEL, PLAN_MEMSET, PLAN_EMPTY, PLAN_MARKER = 0, 1, 3, 4     # CWF_PLAN_*
PLAN_CLASS_MAIN, PLAN_CLASS_SIDE, PLAN_CLASS_CONVERSION = 0, 1, 2  # CWF_PLAN_CLASS_*


def plan_describe(lib, plan):
    """What cwf_plan_counts / cwf_plan_describe / cwf_plan_kernel_name say about a built plan, as Python lists indexed by plan
    position: kind, stream, marker_id, record, creation, waits (a list per position), name ('' for a node that is no kernel), and
    edges (position pairs).  Nothing is launched."""
    cnt = (I * 3)()
    check(lib.cwf_plan_counts(plan, cnt), "cwf_plan_counts")
    n, nw, ne = cnt[0], cnt[1], cnt[2]
    kind, stream, marker, record, creation = ((I * n)() for _ in range(5))
    off, wait = (I * (n + 1))(), (I * max(nw, 1))()
    ef, et = (I * max(ne, 1))(), (I * max(ne, 1))()
    check(lib.cwf_plan_describe(plan, kind, stream, marker, record, creation, off, wait, ef, et), "cwf_plan_describe")
    names = []
    for i in range(n):
        ln = lib.cwf_plan_kernel_name(plan, i, None, 0)
        if ln < 0:
            raise CwfError("cwf_plan_kernel_name failed with status %d" % ln)
        buf = C.create_string_buffer(ln + 1)
        lib.cwf_plan_kernel_name(plan, i, buf, ln + 1)
        names.append(buf.value.decode())
    return {"kind": list(kind), "stream": list(stream), "marker_id": list(marker), "record": [int(r) for r in record],
            "creation": list(creation), "waits": [list(wait[off[i]:off[i + 1]]) for i in range(n)], "name": names,
            "edges": [(ef[j], et[j]) for j in range(ne)]}


class GemmArgs(C.Structure):
    """struct cwf_gemm_args (include/cwf_hip.h)"""
    _fields_ = [("A", P), ("sa_m", L), ("sa_k", L), ("sa_zb", L), ("sa_zh", L),
                ("B", P), ("sb_k", L), ("sb_n", L), ("sb_zb", L), ("sb_zh", L),
                ("C", P), ("sc_m", L), ("sc_zb", L), ("sc_zh", L),
                ("bias", P), ("residual", P), ("sr_m", L), ("sr_zb", L), ("sr_zh", L),
                ("M", I), ("N", I), ("K", I), ("ZB", I), ("ZH", I), ("alpha", F), ("act", I), ("accumulate", I),
                ("A2", P), ("split_n", I), ("B2", P), ("split_m", I), ("C2", P), ("rowsum", P), ("rowsum_acc", I), ("rng", P),
                ("a_drop_off", C.c_uint64), ("a_drop_n", C.c_uint64), ("a_drop_p", F), ("a_drop_p2", F),
                ("c_drop_off", C.c_uint64), ("c_drop_n", C.c_uint64), ("c_drop_p", F), ("c_drop_p2", F),
                ("B_tab", P * 4), ("bias_tab", P * 4), ("C_tab", P * 4), ("rowsum_tab", P * 4)]


class ConvArgs(C.Structure):
    """struct cwf_conv_args (include/cwf_hip.h)"""
    _fields_ = [("op", I), ("precision", I),
                ("x", P), ("x_ldc", I), ("wpk", P), ("bias", P), ("y", P), ("y_ldc", I),
                ("in_scale", P), ("in_shift", P), ("in_slope", F),
                ("residual", P), ("r_ldc", I), ("out_scale", P), ("stats", P),
                ("nb_x", P), ("nb_ldc", I), ("nb_scale", P), ("nb_shift", P), ("nb_slope", F),
                ("x16", P), ("zero16", P), ("y16", P),
                ("w_raw", P),
                ("groups", I), ("x_goff", I), ("y_goff", I), ("wpk_g", P * 3), ("bias_g", P * 3),
                ("N", I), ("Di", I), ("Hi", I), ("Wi", I), ("Cin", I), ("Do", I), ("Ho", I), ("Wo", I), ("Cout", I)]


class WgradArgs(C.Structure):
    """struct cwf_wgrad_args (include/cwf_hip.h)"""
    _fields_ = [("op", I), ("precision", I),
                ("x", P), ("x_ldc", I), ("in_scale", P), ("in_shift", P), ("in_slope", F),
                ("dy", P), ("dy_ldc", I),
                ("dy_scale", P), ("xa16", P), ("dy16", P), ("zero16", P),
                ("partial", P),
                ("groups", I), ("x_g", P * 3), ("dy_g", P * 3), ("partial_g", P * 3),
                ("N", I), ("Di", I), ("Hi", I), ("Wi", I), ("Cin", I), ("Do", I), ("Ho", I), ("Wo", I), ("Cout", I)]


# struct cwf_conv_args / cwf_wgrad_args .precision
PRECISION = {"fp32": 0, "bf16x3": 1, "bf16": 2}


class LnGroupParams(C.Structure):
    """struct cwf_ln_group_params (include/cwf_hip.h)"""
    _fields_ = [(n, P * 4) for n in ("g1", "b1", "g2", "b2", "dg1", "db1", "dg2", "db2")]


class GatherJob(C.Structure):
    """struct cwf_gather_job (include/cwf_hip.h)"""
    _fields_ = [("feats", P), ("index", P), ("head", P), ("out", P), ("head_bstride", L), ("out_bstride", L), ("T", I),
                ("drop_off", C.c_uint64), ("head_g", P * 4), ("group_B", I)]


class PrepSample(C.Structure):
    """struct cwf_prep_sample (include/cwf_hip.h)"""
    _fields_ = [("image", P), ("label", P), ("S0", I), ("S1", I), ("S2", I), ("o0", I), ("o1", I), ("o2", I), ("flip", I),
                ("intensity", I), ("scale", F * 4), ("shift", F * 4)]


class PrepAffineSample(C.Structure):
    """struct cwf_prep_affine_sample (include/cwf_hip.h)"""
    _fields_ = PrepSample._fields_ + [("m", F * 9)]


class PrepElasticSample(C.Structure):
    """struct cwf_prep_elastic_sample (include/cwf_hip.h)"""
    _fields_ = PrepAffineSample._fields_ + [("disp", P), ("G0", I), ("G1", I), ("G2", I)]


class IntensitySample(C.Structure):
    """struct cwf_intensity_sample (include/cwf_hip.h)"""
    _fields_ = [("taps", (F * 7) * 4), ("amp", F * 4), ("key", U64), ("gamma", F * 4), ("blur", I), ("noise", I), ("gam", I)]


class FocalParams(C.Structure):
    """struct cwf_focal_params (include/cwf_hip.h)"""
    _fields_ = [("fn", D), ("fp", D), ("exponent", D), ("smooth", D), ("gamma", D), ("ce_ratio", D), ("class_weight", D * 4)]


INTENSITY_TILE = (10, 10, 32)   # CWF_INTENSITY_T0, _T1, _T2: the blur's output tile (3-voxel halo on every side)


def intensity_ws_floats(nb, crop):
    """floats of device scratch cwf_augment_intensity needs for nb samples of `crop` voxels when some gamma bit is set"""
    tiles = 1
    for c, t in zip(crop, INTENSITY_TILE):
        tiles *= (int(c) + t - 1) // t
    return 8 * int(nb) * tiles


class AcquireSample(C.Structure):
    """struct cwf_acquire_sample (include/cwf_hip.h)"""
    _fields_ = [("bias", P * 4), ("G0", I), ("G1", I), ("G2", I), ("bias_mask", I), ("contrast_mask", I), ("lowres_mask", I),
                ("factor", F * 4), ("lattice", (I * 3) * 4)]


ACQUIRE_TILE = (32, 8, 32)   # CWF_ACQUIRE_T0, _T1, _T2: the voxels of one (sum, min, max) partial


def acquire_ws_doubles(nb, crop):
    """doubles of device scratch cwf_augment_acquisition needs for nb samples of `crop` voxels when some contrast bit is set"""
    tiles = 1
    for c, t in zip(crop, ACQUIRE_TILE):
        tiles *= (int(c) + t - 1) // t
    return 12 * int(nb) * tiles


WINDOW_MAX_STARTS = 128   # CWF_WINDOW_MAX_STARTS


class WindowGrid(C.Structure):
    """struct cwf_window_grid (include/cwf_hip.h)"""
    _fields_ = [("B", I), ("S", I * 3), ("r", I * 3), ("n", I * 3), ("start", (I * WINDOW_MAX_STARTS) * 3)]


class WindowBox(C.Structure):
    """struct cwf_window_box (include/cwf_hip.h)"""
    _fields_ = [("full", I * 3), ("lo", I * 3)]


NORM_WS_DOUBLES = 2568     # CWF_NORM_WS_DOUBLES
GRADNORM_WS_DOUBLES = 1024     # CWF_GRADNORM_WS_DOUBLES
RULE_ADAMW, RULE_SGD = 1, 2    # CWF_RULE_ADAMW, CWF_RULE_SGD
RESTYPE_INT64 = {"cwf_debug_wsd_launches", "cwf_debug_wgrad_s2_launches", "cwf_debug_gemm_panel_launches", "cwf_debug_attn_split_launches", "cwf_attn_bwd_ws_bytes", "cwf_wgrad_partial_floats", "cwf_wgrad_slab_floats", "cwf_hausdorff_workspace", "cwf_components_workspace",
                 "cwf_lesionwise_workspace", "cwf_surface_metrics_workspace", "cwf_lesionwise_ex_workspace", "cwf_signed_distance_workspace",
                 "cwf_topk_ce_workspace", "cwf_focal_workspace", "cwf_lovasz_workspace", "cwf_class_locations_workspace", "cwf_nonzero_box_workspace"}
LOCATIONS_TILE = 16384     # CWF_LOCATIONS_TILE: the voxels of one workgroup of cwf_class_locations (a 16-byte aligned label starts tile 0)
NONZERO_BOX_TILE = 4096    # CWF_NONZERO_BOX_TILE: the voxels of one workgroup of cwf_nonzero_box (a 16-byte aligned sample starts tile 0)

_lib = None


class CwfError(RuntimeError):
    pass


def load():
    """dlopen the in-tree library and attach prototypes.  Raises if it is not built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise CwfError("libcwf_hip.so is not built (%s); run `python __graft_entry__.py` or `make -C csrc`. "
                       "There is no CPU fallback." % LIB_PATH)
    lib = C.CDLL(LIB_PATH)
    for name, args in SIGNATURES.items():
        fn = getattr(lib, name)
        fn.argtypes = args
        fn.restype = L if name in RESTYPE_INT64 else I
    lib.cwf_arch.restype = C.c_char_p
    lib.cwf_arch.argtypes = []
    lib.cwf_plan_last_error.restype = C.c_char_p
    lib.cwf_plan_last_error.argtypes = []
    lib.cwf_debug_wgrad_bf16_name.restype = C.c_char_p
    _lib = lib
    return lib


def check(rc, name):
    if rc != 0:
        raise CwfError("%s failed with status %d" % (name, rc))
