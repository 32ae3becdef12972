"""ctypes binding of the C ABI in include/yololite_hip.h (libyololite_hip.so, built for gfx950 by
csrc/build.py).  There is NO CPU fallback: if the library is missing or fails to load, importing
this module raises -- the product path must fail loudly rather than run somewhere else."""
from __future__ import annotations

import ctypes as C
import os
import sys
import warnings


def _default_hw_queues():
    """The executor overlaps two batch chunks on two internal HIP streams.  ROCm maps streams onto
    GPU_MAX_HW_QUEUES hardware queues (default 4) round-robin at creation; once RCCL (or a host with many
    torch streams) has created its own streams, a chunk stream can share a hardware queue with the caller's
    stream, which serialises the chunks and their fork/join barriers (measured: -25 % images/s as soon as
    init_process_group("nccl") has run).  8 queues avoid the aliasing.  The variable is read when the HIP
    runtime initialises (first device call), so it is set HERE -- on import of the package, whatever the host
    program is (bench.py, the CLIs, a serving process) -- unless the user chose a value; if the runtime is
    already up the default cannot take effect any more and that is said loudly."""
    if "GPU_MAX_HW_QUEUES" in os.environ or os.environ.get("YOLOLITE_NO_ENV_DEFAULTS"):
        return          # the user's value, or an explicit opt-out: the host application owns its environment
    os.environ["GPU_MAX_HW_QUEUES"] = "8"
    t = sys.modules.get("torch")
    try:
        late = t is not None and t.cuda.is_initialized()
    except Exception:   # pragma: no cover
        late = False
    if late:
        warnings.warn("yololite_amd: the HIP runtime was initialised before this package was imported, so "
                      "GPU_MAX_HW_QUEUES=8 cannot be applied; export it in the environment (multi-stream overlap "
                      "of the executor degrades by ~25 % next to RCCL streams otherwise)", RuntimeWarning)


_default_hw_queues()

_HERE = os.path.dirname(os.path.abspath(__file__))
# YOLOLITE_HIP_LIB selects another build of the same ABI (kernel A/B runs); default: the in-tree library
LIB_PATH = os.environ.get("YOLOLITE_HIP_LIB") or os.path.join(_HERE, "libyololite_hip.so")

YL_ABI_VERSION = 7
YL_MAX_LEVELS = 8
YL_OK = 0
ACT = {"none": 0, "relu": 1, "relu6": 2, "silu": 3, "gelu": 4, "relu_lab": 5}
OP_STEM, OP_CONV, OP_DW, OP_STEMBLOCK, OP_SE = 0, 1, 2, 3, 4
OP_POOL, OP_COPY, OP_LN, OP_GRN, OP_NHWC4 = 5, 6, 7, 8, 9
POST_MAIN, POST_FALLBACK, POST_EVAL = 0, 1, 2
CENTER = {"v8": 0, "simple": 1}
WH = {"softplus": 0, "v8": 1, "exp": 2}
NMS_TORCHVISION, NMS_GREEDY = 0, 1

# "dev_select" bits (developer A/B, bitwise kernel-equivalence tests; see yl_get_option in the header)
DEV_DW_TILE_OFF, DEV_PWS_OFF, DEV_S2C_OFF, DEV_DWC_ALL, DEV_DWT_OFF = 1, 2, 4, 8, 16
DEV_DWT_NOSPLIT = 1 << 10
DEV_WINO_V1 = 1 << 11            # Winograd: yl_conv_wino_kernel (every position in one wave) instead of yl_conv_wino2_kernel
DEV_DWL_OFF = 1 << 14             # depthwise 3x3 -> wide 1x1: yl_conv_dwk_kernel instead of yl_conv_dwl_kernel (window in LDS)
DEV_DWL_ALL = 1 << 15             # ... yl_conv_dwl_kernel on every grid (partial windows, few items: the bitwise test)
DEV_DPW_OFF = 1 << 16             # fused head launch: yl_conv_dpp_kernel (taps from L1/L2) instead of yl_conv_dpw_kernel (window in LDS)
DEV_K3W_OFF = 1 << 17             # small-channel dense 3x3: Winograd / direct kernels instead of yl_conv_k3w_kernel
DEV_POISON = 1 << 18              # workspace poison (isolation tests): activation storage filled with 0xFF (NaN) before every call
DEV_CHAIN_OFF = 1 << 19           # UIB projection + next block's 1x1 expansion: two launches instead of yl_conv_dwx_kernel
DEV_HEAD_SKIP_OFF = 1 << 20       # fused head launch: no objectness skip (every tile runs the whole head-output GEMM and class scan)
DEV_PWX_OFF = 1 << 21             # 1x1 -> 1x1 pair around a single-reader tensor: two launches instead of yl_conv_pwx_kernel
DEV_WINO_SHAPE_SHIFT = 12        # yl_conv_wino2_kernel item shape (2 bits): 0 auto, 1 (4,4), 2 (2,7), 3 two m-tiles

_fp = C.POINTER(C.c_float)
_ip = C.POINTER(C.c_int32)


class yl_layer(C.Structure):
    _fields_ = [(n, C.c_int32) for n in (
        "op", "in_slot", "out_slot", "res_slot", "up_slot", "head_level", "cin", "cout",
        "k", "stride", "pad_t", "pad_l", "act", "in_shift", "dw_k", "dw_stride", "dw_pad_t", "dw_pad_l", "dw_act")] + [
        ("w", _fp), ("b", _fp), ("dw_w", _fp), ("dw_b", _fp),
        ("c2", C.c_int32), ("act2", C.c_int32), ("c3", C.c_int32), ("act3", C.c_int32),
        ("w2", _fp), ("b2", _fp), ("w3", _fp), ("b3", _fp), ("scale_slot", C.c_int32), ("reserved0", C.c_int32),
        ("lab_scale", C.c_float), ("lab_bias", C.c_float), ("eps", C.c_float), ("out_ch_off", C.c_int32)]


class yl_model_desc(C.Structure):
    _fields_ = [("abi_version", C.c_int32), ("img_size", C.c_int32), ("in_channels", C.c_int32),
                ("num_classes", C.c_int32), ("num_masks", C.c_int32), ("proto_slot", C.c_int32),
                ("num_levels", C.c_int32),
                ("level_size", C.c_int32 * YL_MAX_LEVELS), ("level_anchors", C.c_int32 * YL_MAX_LEVELS),
                ("num_slots", C.c_int32), ("slot_h", _ip), ("slot_w", _ip), ("slot_c", _ip),
                ("num_layers", C.c_int32), ("layers", C.POINTER(yl_layer))]


class yl_post_cfg(C.Structure):
    _fields_ = [("mode", C.c_int32), ("conf_thr", C.c_float), ("iou_thr", C.c_float),
                ("per_class_cap", C.c_int32), ("topk", C.c_int32), ("max_out", C.c_int32),
                ("center_mode", C.c_int32), ("wh_mode", C.c_int32), ("backmap_dev", C.c_void_p),
                ("fallback_nms", C.c_int32)]


YL_LOSS_MAX_TOPK = 64


class yl_loss_cfg(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("num_classes", "img_size", "center_mode", "wh_mode", "topk_limit")] + [
        (n, C.c_float) for n in ("lambda_box", "lambda_obj", "lambda_cls", "assign_cls_weight", "center_radius_cells",
                                 "cls_smoothing", "area_cells_min", "area_cells_max", "area_tol", "size_prior_w",
                                 "ar_prior_w", "iou_cost_w", "center_cost_w")]


YL_TRAIN_ADAMW, YL_TRAIN_ADAM, YL_TRAIN_SGD = 0, 1, 2
YL_TRAIN_SEG_EMA_ONLY, YL_TRAIN_SEG_BYTES = 1, 2
YL_TRAIN_MAX_GROUPS = 8
YL_TRAIN_CHUNK_DEFAULT = 4096
YL_TRAIN_STATE_WORDS = 8


class yl_train_segment(C.Structure):
    _fields_ = [("param", C.c_void_p), ("grad", C.c_void_p), ("state0", C.c_void_p), ("state1", C.c_void_p),
                ("ema", C.c_void_p), ("count", C.c_int64), ("group", C.c_int32), ("flags", C.c_uint32)]


class yl_train_chunk(C.Structure):
    _fields_ = [("seg", C.c_int32), ("len", C.c_int32), ("off", C.c_int64)]


class yl_train_cfg(C.Structure):
    _fields_ = [("kind", C.c_int32), ("amp", C.c_int32), ("growth_interval", C.c_int32), ("chunk_elems", C.c_int32),
                ("init_scale", C.c_float), ("growth_factor", C.c_double), ("backoff_factor", C.c_double)]


class yl_train_hyper(C.Structure):
    _fields_ = [("lr", C.c_double * YL_TRAIN_MAX_GROUPS), ("weight_decay", C.c_double * YL_TRAIN_MAX_GROUPS),
                ("beta1", C.c_double), ("beta2", C.c_double), ("eps", C.c_double), ("momentum", C.c_double),
                ("ema_decay", C.c_double), ("max_norm", C.c_double), ("nesterov", C.c_int32), ("reserved0", C.c_int32)]


YL_HEAD_MAX_DEPTH = 4
YL_HEAD_TRAIN, YL_HEAD_SAVE = 1, 2
YL_HEAD_F16, YL_HEAD_BF16 = 0x100, 0x200                   # yl_head_forward's flags: the 1x1 GEMMs' operand type
YL_HEAD_SITE_OUT = -1                                      # yl_head_gemm's site: the output convolutions (else a trunk block)
YL_HEAD_PASS_FORWARD, YL_HEAD_PASS_DGRAD, YL_HEAD_PASS_WGRAD = 0, 1, 2
YL_DNECK_F16, YL_DNECK_BF16 = 0x100, 0x200                 # yl_dneck_forward's flags: the 3x3 GEMMs' operand type
YL_DNECK_PASS_FORWARD, YL_DNECK_PASS_DGRAD, YL_DNECK_PASS_WGRAD = 0, 1, 2


class yl_head_cfg(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("channels", "num_classes", "num_anchors", "head_depth", "num_masks", "reserved0")]


class yl_head_block(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("dw", "pw", "gamma", "beta", "running_mean", "running_var",
                                          "num_batches_tracked")]


class yl_head_tensors(C.Structure):
    _fields_ = [("block", yl_head_block * YL_HEAD_MAX_DEPTH)] + [
        (n, C.c_void_p) for n in ("box_w", "box_b", "obj_w", "obj_b", "cls_w", "cls_b")]


class yl_head_plan_info(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("rows", "stat_rows", "stat_tiles", "gemm_rows", "gemm_tiles", "wgrad_rows",
                                         "wgrad_splits", "ograd_rows", "ograd_splits", "reserved0")] + [
        ("saved_bytes", C.c_int64), ("workspace_bytes", C.c_int64)]


YL_NECK_MAX_DEPTH, YL_NECK_MAX_LEVELS = 4, 4


class yl_neck_cfg(C.Structure):
    _fields_ = [("channels", C.c_int32), ("depth", C.c_int32), ("num_levels", C.c_int32),
                ("in_channels", C.c_int32 * YL_NECK_MAX_LEVELS), ("reserved0", C.c_int32)]


class yl_neck_level(C.Structure):
    _fields_ = [("lat_w", C.c_void_p), ("lat_b", C.c_void_p), ("block", yl_head_block * YL_NECK_MAX_DEPTH)]


class yl_neck_tensors(C.Structure):
    _fields_ = [("level", yl_neck_level * YL_NECK_MAX_LEVELS)]


class yl_neck_level_plan(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("rows", "stat_tiles", "gemm_tiles", "wgrad_rows", "wgrad_splits", "lgrad_rows",
                                         "lgrad_splits", "reserved0")] + [("saved_bytes", C.c_int64)]


class yl_neck_plan_info(C.Structure):
    _fields_ = [("stat_rows", C.c_int32), ("gemm_rows", C.c_int32), ("level", yl_neck_level_plan * YL_NECK_MAX_LEVELS),
                ("saved_bytes", C.c_int64), ("nosave_bytes", C.c_int64), ("workspace_bytes", C.c_int64),
                ("table_bytes", C.c_int64)]


class yl_dneck_block(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("w", "gamma", "beta", "running_mean", "running_var", "num_batches_tracked")]


class yl_dneck_level(C.Structure):
    _fields_ = [("lat_w", C.c_void_p), ("lat_b", C.c_void_p), ("block", yl_dneck_block * YL_NECK_MAX_DEPTH)]


class yl_dneck_tensors(C.Structure):
    _fields_ = [("level", yl_dneck_level * YL_NECK_MAX_LEVELS)]


class yl_dneck_level_plan(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("rows", "stat_tiles", "gemm_tiles", "conv_tiles", "lgrad_rows", "lgrad_splits",
                                         "w3grad_tiles", "w3grad_splits")] + [("saved_bytes", C.c_int64)]


class yl_dneck_plan_info(C.Structure):
    _fields_ = [("stat_rows", C.c_int32), ("gemm_rows", C.c_int32), ("conv_tile", C.c_int32), ("reserved0", C.c_int32),
                ("level", yl_dneck_level_plan * YL_NECK_MAX_LEVELS),
                ("saved_bytes", C.c_int64), ("nosave_bytes", C.c_int64), ("workspace_bytes", C.c_int64),
                ("table_bytes", C.c_int64)]


YL_STAGE_MAX_BLOCKS = 16
YL_STAGE_UIR, YL_STAGE_CN = 0, 1
YL_STAGE_PASS_FORWARD, YL_STAGE_PASS_DGRAD, YL_STAGE_PASS_WGRAD = 0, 1, 2
YL_STAGE_ACT_RELU, YL_STAGE_ACT_RELU6 = 0, 1


class yl_stage_block_cfg(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("type", "a", "k", "s", "mid", "cout", "reserved0", "reserved1")]


class yl_stage_cfg(C.Structure):
    _fields_ = [("in_channels", C.c_int32), ("num_blocks", C.c_int32), ("eps", C.c_double),
                ("block", yl_stage_block_cfg * YL_STAGE_MAX_BLOCKS)]


class yl_stage_unit(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("w", "gamma", "beta", "running_mean", "running_var", "num_batches_tracked")]


class yl_stage_block(C.Structure):
    _fields_ = [(n, yl_stage_unit) for n in ("dw_start", "pw_exp", "dw_mid", "pw_proj")]


class yl_stage_tensors(C.Structure):
    _fields_ = [("block", yl_stage_block * YL_STAGE_MAX_BLOCKS)]


class yl_stage_block_plan(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("size_in", "size_mid", "size_out", "rows_mid", "rows_out", "stat_tiles_mid",
                                         "stat_tiles_out", "exp_rows", "exp_splits", "proj_rows", "proj_splits",
                                         "units")] + [("saved_bytes", C.c_int64)]


class yl_stage_plan_info(C.Structure):
    _fields_ = [("stat_rows", C.c_int32), ("gemm_rows", C.c_int32), ("block", yl_stage_block_plan * YL_STAGE_MAX_BLOCKS),
                ("saved_bytes", C.c_int64), ("nosave_bytes", C.c_int64), ("workspace_bytes", C.c_int64)]


YL_STEM_MAX_UNITS = 8


class yl_stem_unit_cfg(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("k", "s", "cout", "reserved0")]


class yl_stem_cfg(C.Structure):
    _fields_ = [("in_channels", C.c_int32), ("num_units", C.c_int32), ("input_nchw", C.c_int32), ("reserved0", C.c_int32),
                ("eps", C.c_double), ("unit", yl_stem_unit_cfg * YL_STEM_MAX_UNITS)]


class yl_stem_tensors(C.Structure):
    _fields_ = [("unit", yl_stage_unit * YL_STEM_MAX_UNITS)]


class yl_stem_unit_plan(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("size_in", "size_out", "rows_out", "stat_rows", "stat_tiles", "wgrad_rows",
                                         "wgrad_splits", "conv_block")] + [("saved_bytes", C.c_int64)]


class yl_stem_plan_info(C.Structure):
    _fields_ = [("stat_rows", C.c_int32), ("gemm_rows", C.c_int32), ("conv_tile", C.c_int32), ("stat_tiles_max", C.c_int32),
                ("unit", yl_stem_unit_plan * YL_STEM_MAX_UNITS),
                ("saved_bytes", C.c_int64), ("nosave_bytes", C.c_int64), ("workspace_bytes", C.c_int64)]


# every symbol include/yololite_hip.h declares: (name, restype, argtypes)
_vp = C.c_void_p
_vpp = C.POINTER(C.c_void_p)
SYMBOLS = [
    ("yl_create", C.c_int32, [C.POINTER(yl_model_desc), C.c_int32, C.POINTER(_vp)]),
    ("yl_clone", C.c_int32, [_vp, C.POINTER(_vp)]),
    ("yl_streams_overlap", C.c_int32, [C.c_int32, _vp, _vp, C.POINTER(C.c_int32)]),
    ("yl_destroy", None, [_vp]),
    ("yl_strerror", C.c_char_p, [C.c_int32]),
    ("yl_last_error", C.c_char_p, [_vp]),
    ("yl_abi_version", C.c_int32, []),
    ("yl_forward", C.c_int32, [_vp, _vp, C.c_int32, _vpp, _vp]),
    ("yl_forward_timed", C.c_int32, [_vp, _vp, C.c_int32, _vpp, _vp, _fp]),
    ("yl_last_timing", C.c_int32, [_vp, _fp, _fp]),
    ("yl_activation_bytes", C.c_int64, [_vp]),
    ("yl_read_slot", C.c_int32, [_vp, C.c_int32, C.c_int32, _vp, _vp]),
    ("yl_set_option", C.c_int32, [_vp, C.c_char_p, C.c_int32]),
    ("yl_get_option", C.c_int32, [_vp, C.c_char_p, _ip]),
    ("yl_query_fused_block", C.c_int32, [C.c_int32] * 7),
    ("yl_query_dw_prologue", C.c_int32, [C.c_int32] * 6),
    ("yl_query_wino_form", C.c_int32, [C.c_int32] * 7 + [_ip, _ip]),
    ("yl_query_ir_form", C.c_int32, [C.c_int32] * 15 + [_ip]),
    ("yl_query_dw_form", C.c_int32, [C.c_int32] * 17 + [_ip]),
    ("yl_forward_decoded", C.c_int32, [_vp, _vp, C.c_int32, C.c_int32, C.c_int32, _vp, _vp, _vp, _vp]),
    ("yl_preprocess", C.c_int32, [_vp, _vp, _vp, C.c_int32, _vp, _vp]),
    ("yl_decode", C.c_int32, [_vp, _vpp, C.c_int32, C.c_int32, C.c_int32, _vp, _vp, _vp, _vp]),
    ("yl_postprocess", C.c_int32, [_vp, _vpp, C.c_int32, C.POINTER(yl_post_cfg), _vp, _vp, _vp, _vp]),
    ("yl_predict", C.c_int32, [_vp, _vp, C.c_int32, C.POINTER(yl_post_cfg), _vp, _vp, _vp, _vp]),
    ("yl_allgather_dets", C.c_int32, [_vp, _vp, _vp, C.c_int64, _vp, _vp]),
    ("yl_masks", C.c_int32, [_vp, _vpp, C.c_int32, _vp, _vp, C.c_int32, C.c_float, _vp, _vp]),
    ("yl_masks_image", C.c_int32, [_vp, _vpp, C.c_int32, _vp, _vp, _vp, C.c_int32, C.c_float, _vp, _vp, _vp, C.c_int32,
                                   C.c_int32, C.c_int32, _vp, _vp]),
    ("yl_nms", C.c_int32, [_vp, _vp, _vp, C.c_int32, C.c_float, C.c_int32, C.c_int32, _vp, _vp, _vp]),
    ("yl_eval_match", C.c_int32, [_vp, _vp, _vp, _vp, C.c_int32, C.c_int32, C.c_double, _vp, _vp, _vp, _vp]),
    ("yl_eval_sweep", C.c_int32, [_vp, _vp, _vp, C.c_int32, _vp, C.c_int32, _vp, _vp, _vp]),
    ("yl_eval_confusion", C.c_int32, [_vp, _vp, _vp, _vp, _vp, _vp, C.c_int32, C.c_int32, C.c_int32, C.c_float,
                                      _vp, _vp, _vp]),
    ("yl_eval_coco_match", C.c_int32, [_vp, _vp, _vp, _vp, _vp, _vp, C.c_int32, C.c_int32, C.c_int32, _vp, C.c_int32,
                                       _vp, C.c_int32, _vp, _vp, _vp]),
    ("yl_eval_coco_accumulate", C.c_int32, [_vp, _vp, _vp, _vp, C.c_int32, _vp, C.c_int32, C.c_int32, C.c_int32, _vp,
                                            C.c_int32, _vp, C.c_int32, _vp, _vp, _vp]),
    ("yl_loss_af", C.c_int32, [_vp, _vpp, C.c_int32, _vp, _vp, _vp, C.c_int32, C.POINTER(yl_loss_cfg), _vp, _vp, _vp, _vp]),
    ("yl_loss_af_train", C.c_int32, [_vp, _vpp, C.c_int32, _vp, _vp, _vp, C.c_int32, C.POINTER(yl_loss_cfg), _vp, _vp, _vp,
                                     _vp, _vp]),
    ("yl_loss_af_backward", C.c_int32, [_vp, _vpp, C.c_int32, _vp, _vp, _vp, C.c_int32, C.POINTER(yl_loss_cfg), _vp, _vp,
                                        _vp, _vpp, _vp]),
    ("yl_track_create", C.c_int32, [C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_int32, C.c_int32, C.c_int32,
                                    C.POINTER(_vp)]),
    ("yl_track_destroy", None, [_vp]),
    ("yl_track_reset", C.c_int32, [_vp, C.c_int32, _vp]),
    ("yl_track_update", C.c_int32, [_vp, _vp, _vp, C.c_int32, _vp, _vp, _vp, _vp, _vp, _vp]),
    ("yl_track_grow", C.c_int32, [_vp, C.c_int32]),
    ("yl_track_stats", C.c_int32, [_vp, _ip, _ip]),
    ("yl_train_plan", C.c_int64, [C.POINTER(C.c_int64), C.c_int32, C.c_int32, C.POINTER(yl_train_chunk), C.c_int64]),
    ("yl_train_create", C.c_int32, [C.c_int32, C.POINTER(yl_train_cfg), C.POINTER(yl_train_segment), C.c_int32, _vp,
                                    C.POINTER(_vp)]),
    ("yl_train_destroy", None, [_vp]),
    ("yl_train_set_grads", C.c_int32, [_vp, _vpp, _vp]),
    ("yl_train_step", C.c_int32, [_vp, C.POINTER(yl_train_hyper), _vp]),
    ("yl_train_scale_ptr", _vp, [_vp]),
    ("yl_train_read_state", C.c_int32, [_vp, _fp, _ip, _fp, _ip, _fp]),
    ("yl_train_write_state", C.c_int32, [_vp, C.c_float, C.c_int32, _fp]),
    ("yl_head_plan", C.c_int32, [C.POINTER(yl_head_cfg), C.c_int32, C.c_int32, C.POINTER(yl_head_plan_info)]),
    ("yl_head_create", C.c_int32, [C.c_int32, C.POINTER(yl_head_cfg), C.POINTER(_vp)]),
    ("yl_head_destroy", None, [_vp]),
    ("yl_head_forward", C.c_int32, [_vp, C.POINTER(yl_head_tensors), _vp, C.c_int32, C.c_int32, C.c_uint32, _vp, _vp,
                                    _ip]),
    ("yl_head_backward", C.c_int32, [_vp, C.POINTER(yl_head_tensors), C.POINTER(yl_head_tensors), _vp, _vp, _vp,
                                     C.c_int32, C.c_int32, _vp, _ip]),
    ("yl_head_held", C.c_int32, [_vp, C.POINTER(C.c_int64), C.POINTER(C.c_int64), _ip]),
    ("yl_head_gemm", C.c_int32, [_vp, C.c_int32, C.c_int32, C.c_uint32, C.POINTER(yl_head_tensors), _vp, _vp, _vp,
                                 C.c_int32, C.c_int32, _vp, _ip]),
    ("yl_neck_plan", C.c_int32, [C.POINTER(yl_neck_cfg), C.c_int32, _ip, C.POINTER(yl_neck_plan_info)]),
    ("yl_neck_nearest_map", C.c_int32, [C.c_int32, C.c_int32, _ip, _ip, _ip]),
    ("yl_neck_create", C.c_int32, [C.c_int32, C.POINTER(yl_neck_cfg), C.POINTER(_vp)]),
    ("yl_neck_destroy", None, [_vp]),
    ("yl_neck_forward", C.c_int32, [_vp, C.POINTER(yl_neck_tensors), _vpp, C.c_int32, _ip, C.c_uint32, _vpp, _vp, _ip]),
    ("yl_neck_backward", C.c_int32, [_vp, C.POINTER(yl_neck_tensors), C.POINTER(yl_neck_tensors), _vpp, _vpp, _vpp,
                                     C.c_int32, _ip, _vp, _ip]),
    ("yl_neck_held", C.c_int32, [_vp, C.POINTER(C.c_int64), C.POINTER(C.c_int64), _ip]),
    ("yl_dneck_plan", C.c_int32, [C.POINTER(yl_neck_cfg), C.c_int32, _ip, C.POINTER(yl_dneck_plan_info)]),
    ("yl_dneck_create", C.c_int32, [C.c_int32, C.POINTER(yl_neck_cfg), C.POINTER(_vp)]),
    ("yl_dneck_destroy", None, [_vp]),
    ("yl_dneck_forward", C.c_int32, [_vp, C.POINTER(yl_dneck_tensors), _vpp, C.c_int32, _ip, C.c_uint32, _vpp, _vp, _ip]),
    ("yl_dneck_backward", C.c_int32, [_vp, C.POINTER(yl_dneck_tensors), C.POINTER(yl_dneck_tensors), _vpp, _vpp, _vpp,
                                      C.c_int32, _ip, _vp, _ip]),
    ("yl_dneck_held", C.c_int32, [_vp, C.POINTER(C.c_int64), C.POINTER(C.c_int64), _ip]),
    ("yl_stage_plan", C.c_int32, [C.POINTER(yl_stage_cfg), C.c_int32, C.c_int32, C.POINTER(yl_stage_plan_info)]),
    ("yl_stage_create", C.c_int32, [C.c_int32, C.POINTER(yl_stage_cfg), C.POINTER(_vp)]),
    ("yl_stage_destroy", None, [_vp]),
    ("yl_stage_held", C.c_int32, [_vp, C.POINTER(C.c_int64), C.POINTER(C.c_int64), _ip]),
    ("yl_stage_forward", C.c_int32, [_vp, C.POINTER(yl_stage_tensors), _vp, C.c_int32, C.c_int32, C.c_uint32, _vp, _vp, _ip]),
    ("yl_stage_backward", C.c_int32, [_vp, C.POINTER(yl_stage_tensors), C.POINTER(yl_stage_tensors), _vp, _vp, _vp, _ip]),
    ("yl_stage_depthwise", C.c_int32, [_vp, _vp, _vp, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _vp,
                                       _ip]),
    ("yl_stem_plan", C.c_int32, [C.POINTER(yl_stem_cfg), C.c_int32, C.c_int32, C.POINTER(yl_stem_plan_info)]),
    ("yl_stem_create", C.c_int32, [C.c_int32, C.POINTER(yl_stem_cfg), C.POINTER(_vp)]),
    ("yl_stem_destroy", None, [_vp]),
    ("yl_stem_held", C.c_int32, [_vp, C.POINTER(C.c_int64), C.POINTER(C.c_int64), _ip]),
    ("yl_stem_forward", C.c_int32, [_vp, C.POINTER(yl_stem_tensors), _vp, C.c_int32, C.c_int32, C.c_uint32, _vp, _vp, _ip]),
    ("yl_stem_backward", C.c_int32, [_vp, C.POINTER(yl_stem_tensors), C.POINTER(yl_stem_tensors), _vp, _vp, _vp, _ip]),
    ("yl_stem_conv", C.c_int32, [_vp, _vp, _vp] + [C.c_int32] * 8 + [_vp, _ip]),
    ("yl_amp_stage_set", C.c_int32, [_vp, C.c_uint32]),
    ("yl_amp_stem_set", C.c_int32, [_vp, C.c_uint32]),
    ("yl_amp_stage_get", C.c_int32, [_vp, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    ("yl_amp_stem_get", C.c_int32, [_vp, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    ("yl_amp_stem_conv", C.c_int32, [_vp, _vp, _vp] + [C.c_int32] * 8 + [C.c_uint32, _vp, _ip]),
    ("yl_variant_stage_set", C.c_int32, [_vp, C.c_int32, C.c_int32]),
    ("yl_variant_stage_get", C.c_int32, [_vp, _ip, _ip]),
    ("yl_variant_stage_depthwise", C.c_int32, [_vp, _vp, _vp, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                               C.c_int32, _vp, _ip]),
    ("yl_augment", C.c_int32, [_vp, _vp, _vp, C.c_int32, C.c_int32, _vp, _vp]),
]
# entries whose names carry a digit, bound like the others.  Listed apart: SYMBOLS is held, name for name, to what a
# letters-only pattern finds declared in the header (tests/test_host_cpu.py), and that pattern does not see these
SYMBOLS_DIGITS = [
    ("yl_dneck_conv3x3", C.c_int32, [_vp, C.c_int32, C.c_uint32, _vp, _vp, _vp, C.c_int32, C.c_int32, _vp, _ip]),
]

_lib = None


class YoloLiteHipError(RuntimeError):
    pass


def load():
    """Load libyololite_hip.so once.  torch is imported first so that the HIP runtime the library
    binds to (libamdhip64.so.7) is the one PyTorch-ROCm already mapped into the process -- device
    pointers of torch tensors are then valid for our kernels."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise YoloLiteHipError(
            f"{LIB_PATH} not found: build it with `python yololite-official-repo_amd/csrc/build.py` "
            "(or __graft_entry__.build()). There is no CPU fallback.")
    import torch  # noqa: F401  (maps PyTorch's libamdhip64 first)
    try:
        lib = C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL)
    except OSError as e:  # pragma: no cover
        raise YoloLiteHipError(f"cannot load {LIB_PATH}: {e}") from e
    for name, res, args in SYMBOLS + SYMBOLS_DIGITS:
        fn = getattr(lib, name)          # AttributeError if the ABI lost a symbol
        fn.restype = res
        fn.argtypes = args
    if lib.yl_abi_version() != YL_ABI_VERSION:
        raise YoloLiteHipError("libyololite_hip.so ABI version mismatch")
    _lib = lib
    return lib


def check(status: int, ctx=None, what: str = ""):
    if status == YL_OK:
        return
    lib = load()
    msg = lib.yl_strerror(status).decode()
    detail = lib.yl_last_error(ctx).decode() if ctx else ""
    raise YoloLiteHipError(f"{what or 'yololite_hip'}: {msg} ({status}) {detail}".strip())
