"""ctypes binding of libi2vsgg_hip.so -- the ONLY compute backend of this package.

There is no CPU or eager-PyTorch fallback: if the shared library is missing or an entry
point is absent, import fails loudly.  Signatures mirror include/i2vsgg_hip.h.
"""
import ctypes as C
import os

# torch first: its wheel bundles the HIP runtime (libamdhip64) the process must share; loading our
# library before torch would bind it to a second copy of the runtime and launches would fail.
import torch  # noqa: F401

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libi2vsgg_hip.so")

LAYOUT_NHWC, LAYOUT_NCHW = 0, 1
EPI_RELU, EPI_RESIDUAL, EPI_SCALE, EPI_BIAS, EPI_ZEROED = 1, 2, 4, 8, 16

_p, _i, _f, _z, _l = C.c_void_p, C.c_int32, C.c_float, C.c_size_t, C.c_int64

# name -> (restype, argtypes); kept in the same order as the header
SIGNATURES = {
    "i2v_version": (_i, []),
    "i2v_last_error": (C.c_char_p, []),
    "i2v_build_flags": (_i, []),
    "i2v_stream_create": (_i, [_i, _i, C.POINTER(C.c_void_p)]),
    "i2v_stream_destroy": (_i, [_p]),
    "i2v_roi_align_fwd": (_i, [_p, _i, _i, _i, _i, _i, _p, _i, _i, _i, _f, _i, _p, _i, _p]),
    "i2v_roi_align_bwd": (_i, [_p, _i, _p, _i, _i, _i, _f, _i, _p, _i, _i, _i, _i, _i, _p]),
    "i2v_roi_align_bwd_gather_workspace_bytes": (_z, [_i, _i, _i, _i, _i]),
    "i2v_roi_align_bwd_gather": (_i, [_p, _p, _i, _i, _i, _f, _i, _p, _i, _i, _i, _i, _p, _z, _p]),
    "i2v_roi_align_sampled_fwd": (_i, [_p, _i, _i, _i, _i, _i, _p, _i, _i, _i, _f, _i, _p, _i, _p]),
    "i2v_roi_align_sampled_bwd": (_i, [_p, _i, _p, _i, _i, _i, _f, _i, _p, _i, _i, _i, _i, _i, _p]),
    "i2v_roi_pool_fwd": (_i, [_p, _i, _i, _i, _i, _i, _p, _i, _i, _i, _f, _p, _p, _i, _p]),
    "i2v_roi_pool_fwd_geom": (_i, [_p, _i, _i, _p, _l, _p, _i, _i, _i, _f, _p, _p, _i, _p]),
    "i2v_roi_pool_bwd": (_i, [_p, _p, _i, _p, _i, _i, _i, _p, _i, _i, _i, _i, _i, _p]),
    "i2v_nms_workspace_bytes": (_z, [_i, _i]),
    "i2v_nms_sorted": (_i, [_p, _i, _i, _f, _i, _p, _p, _p, _z, _p]),
    "i2v_rpn_proposal_workspace_bytes": (_z, [_i, _i, _i, _i, _i]),
    "i2v_rpn_proposal": (_i, [_p, _i, _p, _p, _p, _i, _i, _i, _i, _i, _i, _i, _f, _p, _p, _p, _p, _z, _p]),
    "i2v_rpn_decode": (_i, [_p, _i, _p, _p, _p, _i, _i, _i, _i, _i, _p, _p, _p]),
    "i2v_sort_desc_workspace_bytes": (_z, [_i, _i]),
    "i2v_sort_desc": (_i, [_p, _i, _i, _p, _p, _z, _p]),
    "i2v_bbox_overlaps": (_i, [_p, _i, _i, _i, _p, _i, _i, _i, _p, _p, _p, _p]),
    "i2v_conv_fwd": (_i, [_p, _p, _p, _p, _p, _p, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _p, _z, _p]),
    "i2v_conv_fwd_splits": (_i, [_i, _i, _i, _i, _i, _i, _i, _i, _i, _z]),
    "i2v_conv_split_workspace_bytes": (_z, [_i, _i, _i, _i, _i, _i, _i, _i, _i]),
    "i2v_conv_fwd_plan": (_i, [_i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _z, _p, _i]),
    "i2v_conv_wgrad_plan": (_i, [_i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _z, _p, _i]),
    "i2v_roi_align_fwd_plan": (_i, [_i] * 10 + [_p, _i]),
    "i2v_roi_align_bwd_plan": (_i, [_i] * 10 + [_p, _i]),
    "i2v_nms_plan": (_i, [_i, _i, _p, _i]),
    "i2v_set_tuning": (_i, [_i, _i]),
    "i2v_get_tuning": (_i, [_i]),
    "i2v_gemm_nt_batched": (_i, [_p, _p, _p, _i, _i, _i, _i, _l, _l, _l, _p, _z, _p]),
    "i2v_winograd_filter": (_i, [_p, _p, _i, _i, _p]),
    "i2v_conv3x3_winograd_workspace_bytes": (_z, [_i, _i, _i, _i, _i]),
    "i2v_conv3x3_winograd_fwd": (_i, [_p, _p, _p, _p, _p, _i, _i, _i, _i, _i, _i, _p, _z, _p]),
    "i2v_winograd4_filter": (_i, [_p, _p, _i, _i, _p]),
    "i2v_winograd4_filter_dgrad": (_i, [_p, _p, _i, _i, _p]),
    "i2v_conv3x3_winograd4_workspace_bytes": (_z, [_i, _i, _i, _i, _i]),
    "i2v_conv3x3_winograd4_fwd": (_i, [_p, _p, _p, _p, _p, _i, _i, _i, _i, _i, _i, _p, _z, _p]),
    "i2v_conv_set_tile": (_i, [_i]),
    "i2v_conv_debug_clock": (_i, [_p]),
    "i2v_debug_clock_stamp": (_i, [_p, _p]),
    "i2v_conv_dgrad_workspace_bytes": (_z, [_i, _i, _i, _i]),
    "i2v_conv_dgrad": (_i, [_p, _p, _p, _i, _i, _i, _i, _i, _i, _i, _i, _i, _p, _z, _p, _z, _p]),
    "i2v_conv_wgrad_workspace_bytes": (_z, [_i, _i, _i, _i, _i, _i, _i, _i, _i]),
    "i2v_conv_wgrad": (_i, [_p, _p, _p, _i, _i, _i, _i, _i, _i, _i, _i, _i, _f, _p, _z, _p]),
    "i2v_conv_dgrad_fused": (_i, [_p, _p, _p, _p, _p, _p, _p, _i, _i, _i, _i, _i, _i, _i, _i, _i, _p, _z, _p, _z, _p]),
    "i2v_conv_wgrad_scaled": (_i, [_p, _p, _p, _p, _i, _i, _i, _i, _i, _i, _i, _i, _i, _f, _p, _z, _p]),
    "i2v_ordered_fallbacks": (_i, [_i]),
    "i2v_conv3x3_winograd4_dgrad": (_i, [_p, _p, _p, _p, _p, _i, _i, _i, _i, _i, _p, _z, _p]),
    "i2v_conv3x3_winograd4_wgrad_workspace_bytes": (_z, [_i, _i, _i, _i, _i]),
    "i2v_conv3x3_winograd4_wgrad": (_i, [_p, _p, _p, _p, _i, _i, _i, _i, _i, _f, _p, _z, _p]),
    "i2v_gemm_tn_batched": (_i, [_p, _p, _p, _i, _i, _i, _i, _l, _l, _l, _p]),
    "i2v_gemm_tn_batched_acc": (_i, [_p, _p, _p, _i, _i, _i, _i, _l, _l, _l, _p]),
    "i2v_conv3x3_winograd4_v_bytes": (_z, [_i, _i, _i, _i]),
    "i2v_conv3x3_winograd4_fwd_keep": (_i, [_p, _p, _p, _p, _p, _p, _i, _i, _i, _i, _i, _i, _p, _z, _p]),
    "i2v_conv3x3_winograd4_wgrad_v": (_i, [_p, _p, _p, _p, _i, _i, _i, _i, _i, _f, _p, _z, _p]),
    "i2v_conv_wgrad_sgd": (_i, [_p, _p, _p, _p, _i, _i, _i, _i, _i, _i, _i, _i, _i, _f, _f, _f, _p]),
    "i2v_epilogue_bwd": (_i, [_p, _p, _p, _p, _p, _p, _l, _i, _i, _p, _p, _z, _p]),
    "i2v_maxpool3x3s2_fwd": (_i, [_p, _p, _p, _i, _i, _i, _i, _p]),
    "i2v_sgd_momentum": (_i, [_p, _p, _p, _l, _f, _f, _f, _p]),
    "i2v_sgd_momentum_multi": (_i, [_p, _p, _p, _p, _p, _p, _i, _f, _p]),
    "i2v_adam_step": (_i, [_p, _p]),
    "i2v_adam_multi": (_i, [_p, _p, _p, _p, _p, _p, _p, _i, C.c_double, C.c_double, C.c_double, _p, _p]),
    "i2v_dstyle_pool_fwd": (_i, [_p, _p, _p, _l, _i, _i, _i, _p]),
    "i2v_dstyle_pool_bwd": (_i, [_p, _p, _p, _p, _p, _l, _i, _i, _i, _p]),
    "i2v_dstyle_fused_workspace_bytes": (_z, [_l, _i, _i, _i]),
    "i2v_dstyle_fused_fwd": (_i, [_p, _p, _p, _p, _p, _p, _p, _p, _l, _i, _i, _i, _i, _p, _z, _p]),
    "i2v_relation_topk_workspace_bytes": (_z, [_i, _i]),
    "i2v_relation_topk": (_i, [_p, _p, _p, _p, _i, _i, _i, _p, _p, _p, _p, _z, _p]),
    "i2v_video_associate_workspace_bytes": (_z, [_i, _i, _i]),
    "i2v_video_associate": (_i, [_p, _p, _p, _p, _p, _p, _i, _i, _i, _i, _p, _p, _p, _p, _p, _p, _z, _p]),
    "i2v_video_associate_tracks_workspace_bytes": (_z, [_i, _i, _i]),
    "i2v_video_associate_tracks": (_i, [_p, _p, _p, _p, _p, _p, _i, _i, _i, _i, _p, _p, _p, _p, _p, _p, _p, _z, _p]),
    "i2v_video_viou_match_workspace_bytes": (_z, [_i, _i]),
    "i2v_video_viou_match": (_i, [_p, _p, _p, _p, _p, _p, _i, _i, _i, _l, _i, _i, C.c_double, _p, _p, _p, _p, _z, _p]),
    "i2v_video_relation_nms_workspace_bytes": (_z, [_i, _i]),
    "i2v_video_relation_nms": (_i, [_p, _p, _p, _i, _i, _l, C.c_double, _p, _p, _p, _p, _p, _z, _p]),
    "i2v_seqnms_workspace_bytes": (_z, [_i, _i, _i]),
    "i2v_seqnms": (_i, [_p, _p, _p, _p, _p, _i, _i, _i, C.c_double, C.c_double, _i, _p, _p, _p, _p, _z, _p]),
    "i2v_track_stitch_workspace_bytes": (_z, [_i, _i, _i, _i]),
    "i2v_track_stitch": (_i, [_p] * 6 + [_i, _i, _i, _i, C.c_double, _i] + [_p] * 8 + [_p, _z, _p]),
    "i2v_relation_targets_workspace_bytes": (_z, [_i]),
    "i2v_relation_targets": (_i, [_p] * 11 + [_i] * 5 + [_p] * 10 + [_z, _p]),
    "i2v_recognition_rows_workspace_bytes": (_z, [_i]),
    "i2v_recognition_rows": (_i, [_p, _p, _p, _p, _p, _i, _i, _i, _i, _p, _p, _p, _p, _p, _z, _p]),
    "i2v_recognition_align_workspace_bytes": (_z, [_i, _i]),
    "i2v_recognition_align": (_i, [_p, _p, _p, _p, _i, _i, _i, _i, _i, _i, _p, _p, _p, _p, _p, _p, _p, _z, _p]),
    "i2v_image_relation_match_workspace_bytes": (_z, [_i]),
    "i2v_image_relation_match": (_i, [_p, _p, _p, _p, _p, _p, _i, _i, _i, _i, C.c_double, _p, _p, _p, _p, _z, _p]),
    "i2v_image_relation_count": (_i, [_p, _p, _p, _p, _i, _i, _i, _p, _p, _p, _p, _z, _p]),
    "i2v_relation_feature_pool_workspace_bytes": (_z, [_i]),
    "i2v_relation_feature_pool": (_i, [_p, _p, _p, _p, _p, _i, _i, _i, _i, _i, _p, _p, _p, _z, _p]),
    "i2v_det_eval_match_workspace_bytes": (_z, [_i]),
    "i2v_det_eval_match": (_i, [_p, _p, _p, _p, _p, _p, _p, _i, _i, _i, _i, _i, C.c_double, _p, _p, _p, _p, _z, _p]),
    "i2v_det_eval_curve_workspace_bytes": (_z, [_i]),
    "i2v_det_eval_curve": (_i, [_p, _p, _p, _p, _i, _i, _p, _p, _p, _p, _p, _p, _p, _p, _z, _p]),
    "i2v_proposal_cover_workspace_bytes": (_z, [_i]),
    "i2v_proposal_cover": (_i, [_p] * 7 + [_i] * 7 + [_p, _p, _p, _p, _z, _p]),
    "i2v_image_prep_size": (_i, [_i, _i, _i, _p, _p, _p]),
    "i2v_image_prep": (_i, [_p, _i, _i, _i, _i, _p, _i, _p, _i, _i, _p]),
    "i2v_det_postprocess_workspace_bytes": (_z, [_i, _i]),
    "i2v_det_postprocess": (_i, [_p, _p, _p, _i, _p, _p, _f, _f, _f, _i, _i, _f, _f, _i, _p, _p, _p, _z, _p]),
    "i2v_det_postprocess_info": (_i, [_p, _p, _p, _i, _p, _p, _p, _i, _i, _f, _f, _i, _p, _p, _p, _z, _p]),
    "i2v_soft_nms_workspace_bytes": (_z, [_i, _i]),
    "i2v_soft_nms": (_i, [_p, _p, _i, _i, _i, _f, _f, _f, _p, _p, _p, _p, _z, _p]),
    "i2v_soft_nms_plan": (_i, [_i, _i, _p, _i]),
    "i2v_det_postprocess_soft": (_i, [_p, _p, _p, _i, _p, _p, _f, _f, _f, _i, _i, _f, _f, _i, _i, _f, _f, _p, _p, _p, _z, _p]),
    "i2v_det_postprocess_soft_info": (_i, [_p, _p, _p, _i, _p, _p, _p, _i, _i, _f, _f, _i, _i, _f, _f, _p, _p, _p, _z, _p]),
    "i2v_l2norm_rows_fwd": (_i, [_p, _p, _p, _i, _i, _f, _p]),
    "i2v_l2norm_rows_bwd": (_i, [_p, _p, _p, _p, _i, _i, _f, _p]),
    "i2v_bce_rows_fwd": (_i, [_p, _p, _p, _p, _i, _i, _p]),
    "i2v_bce_rows_bwd": (_i, [_p, _p, _p, _p, _p, _i, _i, _p]),
    "i2v_half_mse_fwd": (_i, [_p, _l, _f, _p, _p]),
    "i2v_half_mse_bwd": (_i, [_p, _l, _f, _p, _p, _p]),
    "i2v_smooth_l1_fwd": (_i, [_p, _p, _p, _p, _l, _i, _i, _f, _p, _p]),
    "i2v_smooth_l1_bwd": (_i, [_p, _p, _p, _p, _l, _i, _i, _f, _p, _p, _p]),
    "i2v_bbox_transform": (_i, [_p, _i, _p, _i, _p, _i, _i, _p, _p, _p]),
    "i2v_signed_sqrt_fwd": (_i, [_p, _p, _l, _p]),
    "i2v_signed_sqrt_bwd": (_i, [_p, _p, _p, _l, _p]),
    "i2v_pair_gather_fwd": (_i, [_p, _p, _p, _p, _i, _i, _i, _p]),
    "i2v_pair_gather_bwd": (_i, [_p, _p, _p, _p, _i, _i, _i, _p]),
    "i2v_dpixel_fwd": (_i, [_p, _p, _p, _p, _p, _p, _p, _p, _i, _i, _p]),
    "i2v_dpixel_bwd_workspace_bytes": (_z, []),
    "i2v_dpixel_bwd": (_i, [_p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _i, _i, _f, _p, _z, _p]),
}


class I2VError(RuntimeError):
    pass


def _load():
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            "i2vsgg_amd: %s not found. Build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950). There is no CPU fallback." % LIB_PATH)
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        try:
            fn = getattr(lib, name)
        except AttributeError:
            raise ImportError("i2vsgg_amd: %s does not export %s (stale build?)" % (LIB_PATH, name))
        fn.restype, fn.argtypes = res, args
    return lib


lib = _load()

# The library reads no environment variable; the documented I2V_* tuning switches are forwarded here, once, at import.
TUNE = {"I2V_CONV_SPEC": 0, "I2V_SPLIT_TARGET": 1, "I2V_SPLIT_TARGET_SKINNY": 2, "I2V_SPLIT_BELOW": 3, "I2V_SPLIT_ATOMICS": 4,
        "I2V_BIG_FC_TILE": 5, "I2V_WGRAD_V2": 6, "I2V_WGRAD_FUSED_TILE": 7, "I2V_WINO_ROWS": 8, "I2V_ROIPOOL_C128": 9, "I2V_CONV_GEMM": 10, "I2V_STAGGER": 11, "I2V_ROIALIGN_COLS": 12, "I2V_WGRAD_PER_CU": 13, "I2V_WGRAD_XCD": 14, "I2V_FC_FOLD": 15, "I2V_GEMM_X3": 16,
        "I2V_GEMM_PERSIST": 17, "I2V_WGRAD_PRIO": 18, "I2V_STREAM_TILE": 19, "I2V_KGROUPS": 20, "I2V_WGRAD_ORDERED_GFLOP": 21, "I2V_GEMM_DMA": 22,
        "I2V_WGRAD_DMA": 23, "I2V_ROIALIGN_BWD": 24, "I2V_NMS_SCAN": 25, "I2V_FC_UPDATE": 26}
# The knobs the environment may set (README.md has the table): the ones a deployment has a reason to move.  The rest of TUNE is
# reachable through lib.i2v_set_tuning (tests, tools): I2V_ROIALIGN_COLS, I2V_WGRAD_V2, I2V_CONV_GEMM, ... select older forms of
# kernels; I2V_CONV_SPEC, I2V_STAGGER, I2V_FC_FOLD, I2V_GEMM_X3, I2V_GEMM_PERSIST, I2V_WGRAD_PRIO are the reserved indices of
# experiment kernels that left the library in round 6 (the library refuses any value but "off").
ENV_TUNE = ("I2V_SPLIT_ATOMICS", "I2V_SPLIT_TARGET", "I2V_SPLIT_TARGET_SKINNY", "I2V_SPLIT_BELOW", "I2V_BIG_FC_TILE",
            "I2V_WGRAD_FUSED_TILE", "I2V_WGRAD_PER_CU", "I2V_KGROUPS", "I2V_WGRAD_ORDERED_GFLOP", "I2V_WINO_ROWS", "I2V_GEMM_DMA", "I2V_WGRAD_DMA", "I2V_ROIALIGN_BWD", "I2V_NMS_SCAN")
# Settled A/B switches of rounds 1-5 that no longer read the environment (their comments in ops.py / train.py / optim.py name the module
# attribute that replaced them).  A run that still sets one would measure the default without knowing (round-5 advice): say so.
RETIRED_ENV = ("I2V_WINOGRAD_TRAIN", "I2V_BLOCK_FUSED", "I2V_WINOGRAD_WGRAD", "I2V_KEEP_V", "I2V_WGRAD_BRANCH", "I2V_ISD_BATCHED",
               "I2V_DEFER_FC", "I2V_EXPERIMENTS")
for _name, _key in TUNE.items():
    if os.environ.get(_name) in (None, ""):
        continue
    if _name not in ENV_TUNE:
        raise ImportError("i2vsgg_amd: %s is set but is not an environment knob (README.md lists them); it would be ignored. "
                          "Use i2vsgg_amd._lib.lib.i2v_set_tuning(TUNE[%r], value) from a tool or test" % (_name, _name))
    if lib.i2v_set_tuning(_key, int(os.environ[_name])) != 0:
        raise ImportError("i2vsgg_amd: %s=%s refused: %s" % (_name, os.environ[_name], lib.i2v_last_error().decode()))
for _name in RETIRED_ENV:
    if os.environ.get(_name) not in (None, ""):
        import warnings
        warnings.warn("i2vsgg_amd: %s is set but no longer read (a settled switch of rounds 1-5): the default runs" % _name)


def check(rc, what):
    if rc != 0:
        raise I2VError("%s failed (%d): %s" % (what, rc, lib.i2v_last_error().decode()))


def ptr(t):
    """Device pointer of a torch tensor (None -> NULL)."""
    return None if t is None else t.data_ptr()


def stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def need_cuda(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise I2VError("i2vsgg_amd ops run on the GPU only (got a %s tensor); there is no CPU fallback" % t.device.type)
