"""ctypes binding of libsegmamba_hip.so (C ABI declared in include/segmamba_hip.h).

The product path loads exactly one thing: the HIP library built in-tree by
`__graft_entry__.build()` / `segmamba_amd.build`.  There is no CPU fallback: if
the library is missing, `get_lib()` raises (imports must succeed
*and* the native path must be the one that runs).

PyTorch is used here only as the owner of device memory and streams: tensors are
passed as raw pointers + element strides, the current HIP stream as a handle.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_NAME = "libsegmamba_hip.so"
LIB_PATH = os.environ.get("SEGM_LIB_OUT") or os.path.join(_HERE, LIB_NAME)     # SEGM_LIB_OUT: a variant built for an A/B run

SEGM_F32, SEGM_F16, SEGM_BF16 = 0, 1, 2
TIME_FORWARD, TIME_REVERSED, TIME_INTERLEAVED = 0, 1, 2
_DTYPES = {torch.float32: SEGM_F32, torch.float16: SEGM_F16, torch.bfloat16: SEGM_BF16}

_STATUS = {
    -1: "a required pointer is NULL", -2: "bad shape / stride", -3: "dstate out of range ([1, 16] for the scan, [1, 256] for the decode step)",
    -4: "unsupported dtype", -5: "conv width must be in [2, 4]", -6: "workspace missing or too small",
    -7: "unknown time order",
}


class SegmSeq(C.Structure):
    _fields_ = [("ptr", C.c_void_p), ("stride_b", C.c_int64), ("stride_t", C.c_int64), ("stride_d", C.c_int64)]


class SegmBC(C.Structure):
    _fields_ = [("ptr", C.c_void_p), ("stride_b", C.c_int64), ("stride_g", C.c_int64),
                ("stride_t", C.c_int64), ("stride_n", C.c_int64)]


class ScanFwdArgs(C.Structure):
    _fields_ = [
        ("batch", C.c_int32), ("dim", C.c_int32), ("dstate", C.c_int32), ("n_groups", C.c_int32),
        ("seqlen", C.c_int64),
        ("dtype", C.c_int32), ("delta_softplus", C.c_int32), ("time_order", C.c_int32), ("nslices", C.c_int32),
        ("chunk", C.c_int32), ("reserved", C.c_int32),
        ("u", SegmSeq), ("delta", SegmSeq), ("z", SegmSeq), ("out", SegmSeq), ("out_z", SegmSeq),
        ("B", SegmBC), ("C", SegmBC),
        ("A", C.c_void_p), ("D", C.c_void_p), ("delta_bias", C.c_void_p),
        ("last_state", C.c_void_p), ("ckpt", C.c_void_p),
        ("workspace", C.c_void_p), ("workspace_bytes", C.c_size_t),
        ("stream", C.c_void_p),
        ("conv_weight", C.c_void_p), ("conv_bias", C.c_void_p), ("conv_width", C.c_int32), ("reserved2", C.c_int32),
        ("dt_x", C.c_void_p), ("dt_stride_b", C.c_int64), ("dt_stride_t", C.c_int64),
        ("dt_weight", C.c_void_p), ("dt_rank", C.c_int32), ("reserved3", C.c_int32),
    ]


class ScanBwdArgs(C.Structure):
    _fields_ = [
        ("f", ScanFwdArgs),
        ("dout", SegmSeq), ("du", SegmSeq), ("ddelta", SegmSeq), ("dz", SegmSeq),
        ("dB", SegmBC), ("dC", SegmBC),
        ("dA", C.c_void_p), ("dD", C.c_void_p), ("ddelta_bias", C.c_void_p),
        ("workspace", C.c_void_p), ("workspace_bytes", C.c_size_t),
        ("dbc_native", C.c_int32), ("reserved_b", C.c_int32),
    ]


class Conv1dArgs(C.Structure):
    _fields_ = [
        ("batch", C.c_int32), ("dim", C.c_int32), ("width", C.c_int32), ("silu", C.c_int32),
        ("seqlen", C.c_int64),
        ("dtype", C.c_int32), ("time_order", C.c_int32), ("nslices", C.c_int32), ("reserved", C.c_int32),
        ("x", SegmSeq), ("out", SegmSeq),
        ("weight", C.c_void_p), ("bias", C.c_void_p),
        ("dout", SegmSeq), ("dx", SegmSeq),
        ("dweight", C.c_void_p), ("dbias", C.c_void_p),
        ("workspace", C.c_void_p), ("workspace_bytes", C.c_size_t),
        ("stream", C.c_void_p),
    ]


class Conv3dWgradArgs(C.Structure):
    _fields_ = [
        ("batch", C.c_int32), ("cin", C.c_int32), ("cout", C.c_int32), ("depth", C.c_int32), ("height", C.c_int32),
        ("width", C.c_int32), ("dtype", C.c_int32), ("dw_dtype", C.c_int32),
        ("x", C.c_void_p), ("x_stride_b", C.c_int64), ("x_stride_c", C.c_int64), ("x_stride_z", C.c_int64),
        ("x_stride_y", C.c_int64),
        ("dy", C.c_void_p), ("dy_stride_b", C.c_int64), ("dy_stride_c", C.c_int64), ("dy_stride_z", C.c_int64),
        ("dy_stride_y", C.c_int64),
        ("dw", C.c_void_p), ("workspace", C.c_void_p), ("workspace_bytes", C.c_size_t), ("stream", C.c_void_p),
    ]


class Conv3dFwdArgs(C.Structure):
    _fields_ = [
        ("batch", C.c_int32), ("cin", C.c_int32), ("cout", C.c_int32), ("depth", C.c_int32), ("height", C.c_int32),
        ("width", C.c_int32), ("dtype", C.c_int32), ("flags", C.c_int32),
        ("x", C.c_void_p), ("x_stride_b", C.c_int64), ("x_stride_c", C.c_int64), ("x_stride_z", C.c_int64),
        ("x_stride_y", C.c_int64),
        ("y", C.c_void_p), ("y_stride_b", C.c_int64), ("y_stride_c", C.c_int64), ("y_stride_z", C.c_int64),
        ("y_stride_y", C.c_int64),
        ("w_packed", C.c_void_p), ("bias", C.c_void_p), ("stream", C.c_void_p),
        ("stats_partials", C.c_void_p), ("stats_nparts", C.c_int32), ("reserved", C.c_int32),
    ]


class Conv3dClArgs(C.Structure):
    _fields_ = [
        ("batch", C.c_int32), ("channels", C.c_int32), ("depth", C.c_int32), ("height", C.c_int32), ("width", C.c_int32),
        ("dtype", C.c_int32), ("flags", C.c_int32), ("reserved", C.c_int32),
        ("x", C.c_void_p), ("x_stride_b", C.c_int64), ("x_stride_z", C.c_int64), ("x_stride_y", C.c_int64), ("x_stride_x", C.c_int64),
        ("y", C.c_void_p), ("y_stride_b", C.c_int64), ("y_stride_z", C.c_int64), ("y_stride_y", C.c_int64), ("y_stride_x", C.c_int64),
        ("w_image", C.c_void_p), ("bias", C.c_void_p), ("stream", C.c_void_p),
    ]


class Conv3dCubeArgs(C.Structure):
    _fields_ = [
        ("batch", C.c_int32), ("cin", C.c_int32), ("cout", C.c_int32), ("depth", C.c_int32), ("height", C.c_int32), ("width", C.c_int32),
        ("dtype", C.c_int32), ("flags", C.c_int32), ("nt", C.c_int32), ("splits", C.c_int32),
        ("x", C.c_void_p), ("x_stride_b", C.c_int64), ("x_stride_c", C.c_int64), ("x_stride_z", C.c_int64), ("x_stride_y", C.c_int64),
        ("y", C.c_void_p), ("y_stride_b", C.c_int64), ("y_stride_c", C.c_int64), ("y_stride_z", C.c_int64), ("y_stride_y", C.c_int64),
        ("w_image", C.c_void_p), ("bias", C.c_void_p), ("workspace", C.c_void_p), ("workspace_elems", C.c_int64), ("stream", C.c_void_p),
        ("stats_partials", C.c_void_p), ("stats_nparts", C.c_int32), ("reserved", C.c_int32),
    ]


class Add3Args(C.Structure):
    _fields_ = [("count", C.c_int64), ("dtype", C.c_int32), ("reserved", C.c_int32),
                ("a", C.c_void_p), ("b", C.c_void_p), ("c", C.c_void_p), ("out", C.c_void_p), ("stream", C.c_void_p)]


class Gather16Args(C.Structure):
    _fields_ = [("count", C.c_int64), ("mode", C.c_int32), ("reserved", C.c_int32),
                ("src", C.c_void_p), ("map", C.c_void_p), ("out", C.c_void_p), ("stream", C.c_void_p)]


class InstNormFwdArgs(C.Structure):
    _fields_ = [
        ("instances", C.c_int32), ("dtype", C.c_int32), ("act", C.c_int32), ("reserved", C.c_int32),
        ("spatial", C.c_int64), ("slope", C.c_float), ("eps", C.c_float),
        ("x", C.c_void_p), ("residual", C.c_void_p), ("y", C.c_void_p), ("mean", C.c_void_p), ("rstd", C.c_void_p),
        ("workspace", C.c_void_p), ("workspace_bytes", C.c_size_t), ("stream", C.c_void_p),
        ("x_instance_stride", C.c_int64), ("residual_instance_stride", C.c_int64), ("y_instance_stride", C.c_int64),
        ("stats_partials", C.c_void_p), ("stats_nparts", C.c_int32), ("reserved2", C.c_int32),
    ]


class InstNormBwdArgs(C.Structure):
    _fields_ = [
        ("instances", C.c_int32), ("dtype", C.c_int32), ("act", C.c_int32), ("reserved", C.c_int32),
        ("spatial", C.c_int64), ("slope", C.c_float), ("reserved2", C.c_float),
        ("x", C.c_void_p), ("dy", C.c_void_p), ("y", C.c_void_p), ("mean", C.c_void_p), ("rstd", C.c_void_p),
        ("dx", C.c_void_p), ("dresidual", C.c_void_p),
        ("workspace", C.c_void_p), ("workspace_bytes", C.c_size_t), ("stream", C.c_void_p),
        ("x_instance_stride", C.c_int64), ("dy_instance_stride", C.c_int64), ("y_instance_stride", C.c_int64),
        ("dx_instance_stride", C.c_int64), ("dresidual_instance_stride", C.c_int64),
    ]


class InstNormStatsArgs(C.Structure):
    _fields_ = [
        ("instances", C.c_int32), ("dtype", C.c_int32), ("spatial", C.c_int64),
        ("x", C.c_void_p), ("x_instance_stride", C.c_int64),
        ("partials", C.c_void_p), ("partials_bytes", C.c_size_t), ("stream", C.c_void_p),
    ]


class InstNormTailFwdArgs(C.Structure):
    _fields_ = [
        ("instances", C.c_int32), ("dtype", C.c_int32), ("act", C.c_int32), ("reserved", C.c_int32),
        ("spatial", C.c_int64), ("slope", C.c_float), ("eps", C.c_float),
        ("x", C.c_void_p), ("skip", C.c_void_p), ("y", C.c_void_p), ("mean", C.c_void_p), ("rstd", C.c_void_p),
        ("skip_mean", C.c_void_p), ("skip_rstd", C.c_void_p), ("skip_partials", C.c_void_p), ("skip_partials_bytes", C.c_size_t),
        ("workspace", C.c_void_p), ("workspace_bytes", C.c_size_t), ("stream", C.c_void_p),
        ("x_instance_stride", C.c_int64), ("skip_instance_stride", C.c_int64), ("y_instance_stride", C.c_int64),
        ("stats_partials", C.c_void_p), ("stats_nparts", C.c_int32), ("reserved2", C.c_int32),
    ]


class InstNormTailBwdArgs(C.Structure):
    _fields_ = [
        ("instances", C.c_int32), ("dtype", C.c_int32), ("act", C.c_int32), ("reserved", C.c_int32),
        ("spatial", C.c_int64), ("slope", C.c_float), ("reserved2", C.c_float),
        ("x", C.c_void_p), ("skip", C.c_void_p), ("dy", C.c_void_p), ("y", C.c_void_p), ("mean", C.c_void_p), ("rstd", C.c_void_p),
        ("skip_mean", C.c_void_p), ("skip_rstd", C.c_void_p), ("dx", C.c_void_p), ("dskip", C.c_void_p),
        ("workspace", C.c_void_p), ("workspace_bytes", C.c_size_t), ("stream", C.c_void_p),
        ("x_instance_stride", C.c_int64), ("skip_instance_stride", C.c_int64), ("dy_instance_stride", C.c_int64),
        ("y_instance_stride", C.c_int64), ("dx_instance_stride", C.c_int64), ("dskip_instance_stride", C.c_int64),
    ]


class LayerNormArgs(C.Structure):
    _fields_ = [
        ("batch", C.c_int32), ("channels", C.c_int32), ("dtype", C.c_int32), ("reserved", C.c_int32),
        ("spatial", C.c_int64), ("eps", C.c_float), ("reserved2", C.c_float),
        ("x", C.c_void_p), ("y", C.c_void_p), ("gamma", C.c_void_p), ("beta", C.c_void_p), ("mean", C.c_void_p),
        ("rstd", C.c_void_p), ("dy", C.c_void_p), ("dx", C.c_void_p), ("dgamma", C.c_void_p), ("dbeta", C.c_void_p),
        ("workspace", C.c_void_p), ("workspace_bytes", C.c_size_t), ("stream", C.c_void_p),
    ]


class SgdArgs(C.Structure):
    _fields_ = [
        ("ntensors", C.c_int32), ("nesterov", C.c_int32),
        ("params", C.c_void_p), ("grads", C.c_void_p), ("momenta", C.c_void_p), ("numel", C.c_void_p),
        ("lr", C.c_float), ("momentum", C.c_float), ("weight_decay", C.c_float), ("max_norm", C.c_float),
        ("workspace", C.c_void_p), ("workspace_bytes", C.c_size_t), ("stream", C.c_void_p),
        ("loss_scale", C.c_void_p), ("found_inf", C.c_void_p),
    ]


class CrossEntropyArgs(C.Structure):
    _fields_ = [
        ("batch", C.c_int32), ("classes", C.c_int32), ("dtype", C.c_int32), ("reserved", C.c_int32),
        ("spatial", C.c_int64), ("ignore_index", C.c_int64),
        ("logits", C.c_void_p), ("labels", C.c_void_p), ("dlogits", C.c_void_p), ("loss_partial", C.c_void_p),
        ("count_partial", C.c_void_p), ("stream", C.c_void_p),
    ]


class Conv1dUpdateArgs(C.Structure):
    _fields_ = [
        ("batch", C.c_int32), ("dim", C.c_int32), ("width", C.c_int32), ("silu", C.c_int32),
        ("dtype", C.c_int32), ("reserved", C.c_int32),
        ("x", C.c_void_p), ("x_stride_b", C.c_int64), ("x_stride_d", C.c_int64),
        ("conv_state", C.c_void_p), ("state_stride_b", C.c_int64), ("state_stride_d", C.c_int64), ("state_stride_w", C.c_int64),
        ("out", C.c_void_p), ("out_stride_b", C.c_int64), ("out_stride_d", C.c_int64),
        ("weight", C.c_void_p), ("bias", C.c_void_p), ("stream", C.c_void_p),
    ]


class StateUpdateArgs(C.Structure):
    _fields_ = [
        ("batch", C.c_int32), ("dim", C.c_int32), ("dstate", C.c_int32), ("dt_softplus", C.c_int32),
        ("dtype", C.c_int32), ("state_dtype", C.c_int32),
        ("state", C.c_void_p), ("state_stride_b", C.c_int64), ("state_stride_d", C.c_int64), ("state_stride_n", C.c_int64),
        ("x", C.c_void_p), ("x_stride_b", C.c_int64), ("x_stride_d", C.c_int64),
        ("dt", C.c_void_p), ("dt_stride_b", C.c_int64), ("dt_stride_d", C.c_int64),
        ("z", C.c_void_p), ("z_stride_b", C.c_int64), ("z_stride_d", C.c_int64),
        ("out", C.c_void_p), ("out_stride_b", C.c_int64), ("out_stride_d", C.c_int64),
        ("B", C.c_void_p), ("B_stride_b", C.c_int64), ("B_stride_n", C.c_int64),
        ("C", C.c_void_p), ("C_stride_b", C.c_int64), ("C_stride_n", C.c_int64),
        ("A", C.c_void_p), ("D", C.c_void_p), ("dt_bias", C.c_void_p), ("stream", C.c_void_p),
    ]


class LinearArgs(C.Structure):
    _fields_ = [
        ("rows", C.c_int64), ("k", C.c_int32), ("n", C.c_int32), ("dtype", C.c_int32), ("accumulate", C.c_int32),
        ("x", C.c_void_p), ("x_stride_row", C.c_int64), ("w", C.c_void_p), ("bias", C.c_void_p),
        ("y", C.c_void_p), ("y_stride_row", C.c_int64), ("stream", C.c_void_p),
    ]


class PointwiseArgs(C.Structure):
    _fields_ = [
        ("batch", C.c_int32), ("cin", C.c_int32), ("cout", C.c_int32), ("dtype", C.c_int32), ("accumulate", C.c_int32),
        ("spatial", C.c_int64),
        ("x", C.c_void_p), ("x_stride_b", C.c_int64), ("x_stride_c", C.c_int64),
        ("w", C.c_void_p), ("w_stride", C.c_int32), ("bias", C.c_void_p),
        ("y", C.c_void_p), ("y_stride_b", C.c_int64), ("y_stride_c", C.c_int64), ("stream", C.c_void_p),
    ]


class StemArgs(C.Structure):
    _fields_ = [
        ("batch", C.c_int32), ("cout", C.c_int32), ("din", C.c_int32), ("hin", C.c_int32), ("win", C.c_int32), ("dtype", C.c_int32),
        ("x4", C.c_void_p), ("w_packed", C.c_void_p), ("bias", C.c_void_p), ("y", C.c_void_p), ("stream", C.c_void_p),
        ("kernel_size", C.c_int32), ("stride", C.c_int32), ("y_channel_stride", C.c_int64),
    ]


class StemWgradArgs(C.Structure):
    _fields_ = [
        ("batch", C.c_int32), ("cout", C.c_int32), ("din", C.c_int32), ("hin", C.c_int32), ("win", C.c_int32), ("dtype", C.c_int32),
        ("x4", C.c_void_p), ("dy", C.c_void_p), ("dw_packed", C.c_void_p),
        ("workspace", C.c_void_p), ("workspace_bytes", C.c_size_t), ("stream", C.c_void_p),
        ("kernel_size", C.c_int32), ("stride", C.c_int32), ("dy_channel_stride", C.c_int64),
    ]


class WgradGemmArgs(C.Structure):
    _fields_ = [
        ("layout", C.c_int32), ("dtype", C.c_int32), ("m", C.c_int32), ("n", C.c_int32), ("k", C.c_int64),
        ("batch", C.c_int32), ("reserved", C.c_int32),
        ("a", C.c_void_p), ("a_stride_row", C.c_int64), ("a_stride_batch", C.c_int64),
        ("b", C.c_void_p), ("b_stride_row", C.c_int64), ("b_stride_batch", C.c_int64),
        ("out", C.c_void_p), ("workspace", C.c_void_p), ("workspace_bytes", C.c_size_t), ("stream", C.c_void_p),
    ]


class D2sArgs(C.Structure):
    _fields_ = [
        ("batch", C.c_int32), ("channels", C.c_int32), ("depth", C.c_int32), ("height", C.c_int32), ("width", C.c_int32),
        ("dtype", C.c_int32), ("direction", C.c_int32), ("reserved", C.c_int32),
        ("blk", C.c_void_p), ("vol", C.c_void_p),
        ("vol_stride_b", C.c_int64), ("vol_stride_c", C.c_int64), ("vol_stride_z", C.c_int64), ("vol_stride_y", C.c_int64),
        ("stream", C.c_void_p),
    ]


class TransposeArgs(C.Structure):
    _fields_ = [
        ("batch", C.c_int32), ("rows", C.c_int32), ("cols", C.c_int32), ("dtype", C.c_int32),
        ("in_", C.c_void_p), ("add", C.c_void_p), ("out", C.c_void_p), ("stream", C.c_void_p),
    ]


EXPORTS = (
    "segm_selective_scan_fwd", "segm_selective_scan_fwd_workspace_bytes", "segm_selective_scan_ckpt_bytes",
    "segm_selective_scan_default_chunk", "segm_selective_scan_bwd", "segm_selective_scan_bwd_workspace_bytes",
    "segm_selective_scan_bwd_deterministic",
    "segm_selective_scan_fwd_multi", "segm_selective_scan_bwd_multi", "segm_causal_conv1d_fwd_multi", "segm_causal_conv1d_bwd_multi",
    "segm_causal_conv1d_fwd", "segm_causal_conv1d_bwd", "segm_causal_conv1d_bwd_workspace_bytes",
    "segm_conv3d_k3_wgrad", "segm_conv3d_k3_wgrad_workspace_bytes", "segm_conv3d_k3_fwd", "segm_conv3d_k3_fwd_stats_parts",
    "segm_conv3d_k3_fwd_cl", "segm_conv3d_k3_cl_pack_index", "segm_add3",
    "segm_conv3d_k3_cube_fwd", "segm_conv3d_k3_cube_plan", "segm_conv3d_k3_cube_pack_index",
    "segm_conv3d_k3_cube_wgrad", "segm_conv3d_k3_cube_wgrad_workspace_bytes", "segm_gather16",
    "segm_conv3d_k3_cube_pack_multi", "segm_conv3d_k3_cube_stats_parts",
    "segm_instnorm_fwd", "segm_instnorm_bwd", "segm_instnorm_workspace_bytes", "segm_transpose_add", "segm_depth_to_space2",
    "segm_instnorm_stats", "segm_instnorm_tail_fwd", "segm_instnorm_tail_bwd", "segm_instnorm_tail_workspace_bytes",
    "segm_layernorm_tokens_fwd", "segm_layernorm_tokens_bwd", "segm_layernorm_tokens_workspace_bytes",
    "segm_sgd_clip_step", "segm_sgd_clip_step_workspace_bytes", "segm_cross_entropy", "segm_cross_entropy_partials",
    "segm_causal_conv1d_update", "segm_selective_state_update", "segm_linear_rows", "segm_pointwise_cf", "segm_stem_conv_fwd",
    "segm_stem_conv_wgrad", "segm_stem_conv_wgrad_workspace_bytes", "segm_stem_conv_wgrad_workspace_bytes2", "segm_wgrad_gemm", "segm_wgrad_gemm_workspace_bytes",
    "segm_skinny_tn", "segm_skinny_tn_workspace_bytes", "segm_channel_sum", "segm_channel_sum_workspace_bytes", "segm_selective_scan_regular_shape",
    "segm_seg_regions", "segm_seg_regions_workspace_bytes", "segm_edt_sq", "segm_border_distances", "segm_border_distances_workspace_bytes",
    "segm_border_stats", "segm_border_stats_workspace_bytes",
    "segm_edt_sq_long", "segm_edt_sq_long_workspace_bytes", "segm_planes_bbox",
    "segm_sdm_masks", "segm_sdm_compose",
    "segm_resample_argmax", "segm_ccl_roots", "segm_ccl_roots_workspace_bytes", "segm_ccl_sizes", "segm_ccl_select",
    "segm_ccl_select_workspace_bytes",
    "segm_ccl_label_roots", "segm_ccl_label_roots_workspace_bytes", "segm_ccl_label_select", "segm_ccl_label_select_workspace_bytes",
    "segm_ccl_roots_conn", "segm_ccl_label_roots_conn",
    "segm_nonzero_mask_bbox", "segm_crop_stats", "segm_crop_stats_workspace_bytes", "segm_crop_normalize",
    "segm_crop_clip_normalize", "segm_fg_workspace_bytes", "segm_fg_count", "segm_fg_order_stats", "segm_fg_gather",
    "segm_cross_entropy_map", "segm_cross_entropy_map_bwd", "segm_topk_select", "segm_topk_select_workspace_bytes",
    "segm_region_loss_workspace_bytes", "segm_region_loss_fwd", "segm_region_loss_bwd",
    "segm_softmax_dice_workspace_bytes", "segm_softmax_dice_fwd", "segm_softmax_dice_bwd",
    "segm_zoom", "segm_zoom_workspace_bytes", "segm_zoom_labels",
    "segm_zoom_slices", "segm_zoom_slices_workspace_bytes", "segm_zoom_labels_slices",
    "segm_spline_coefs", "segm_spline_coefs_workspace_bytes", "segm_affine_spline3", "segm_affine_labels", "segm_zoom_nearest",
    "segm_gauss_blur",
    "segm_intensity_workspace_bytes", "segm_intensity_stats", "segm_intensity_apply",
    "segm_window_gather", "segm_window_count", "segm_window_blend", "segm_window_finish",
    "segm_add_norm_fwd", "segm_add_norm_bwd", "segm_add_norm_workspace_bytes",
    "segm_abi_version", "segm_status_string",
)


class SkinnyTnArgs(C.Structure):
    _fields_ = [("k", C.c_int64), ("m", C.c_int32), ("n", C.c_int32), ("dtype", C.c_int32), ("reserved", C.c_int32),
                ("wide", C.c_void_p), ("wide_stride_row", C.c_int64), ("skinny", C.c_void_p), ("skinny_stride_row", C.c_int64),
                ("out", C.c_void_p), ("workspace", C.c_void_p), ("workspace_bytes", C.c_size_t), ("stream", C.c_void_p)]


class ChannelSumArgs(C.Structure):
    _fields_ = [("x", C.c_void_p), ("stride_batch", C.c_int64), ("stride_channel", C.c_int64), ("spatial", C.c_int64),
                ("batch", C.c_int32), ("channels", C.c_int32), ("dtype", C.c_int32), ("reserved", C.c_int32),
                ("out", C.c_void_p), ("workspace", C.c_void_p), ("workspace_bytes", C.c_size_t), ("stream", C.c_void_p)]


METRICS_MAX_REGIONS, METRICS_MAX_PLANES, METRICS_MAX_VOXELS, EDT_MAX_LINE = 8, 16, 1 << 30, 256       # SEGM_METRICS_* / SEGM_EDT_MAX_LINE


class SegRegionsArgs(C.Structure):
    _fields_ = [("depth", C.c_int32), ("height", C.c_int32), ("width", C.c_int32), ("reserved", C.c_int32),
                ("pred", C.c_void_p), ("gt", C.c_void_p), ("table", C.c_void_p), ("border_pred", C.c_void_p), ("border_gt", C.c_void_p),
                ("counts", C.c_void_p), ("workspace", C.c_void_p), ("workspace_bytes", C.c_size_t), ("stream", C.c_void_p)]


class EdtSqArgs(C.Structure):
    _fields_ = [("depth", C.c_int32), ("height", C.c_int32), ("width", C.c_int32),
                ("n_volumes", C.c_int32), ("n_planes", C.c_int32), ("fp32", C.c_int32),
                ("spacing_z", C.c_float), ("spacing_y", C.c_float), ("spacing_x", C.c_float), ("reserved", C.c_int32),
                ("plane_volume", C.c_int32 * METRICS_MAX_PLANES), ("plane_bit", C.c_int32 * METRICS_MAX_PLANES),
                ("volumes", C.c_void_p), ("out", C.c_void_p), ("stream", C.c_void_p)]


EDT_LONG_MAX_LINE = 2048                                                       # SEGM_EDT_LONG_MAX_LINE


class EdtSqLongArgs(C.Structure):
    _fields_ = [("depth", C.c_int32), ("height", C.c_int32), ("width", C.c_int32),
                ("n_volumes", C.c_int32), ("n_planes", C.c_int32), ("fp32", C.c_int32),
                ("spacing_z", C.c_float), ("spacing_y", C.c_float), ("spacing_x", C.c_float), ("max_workgroups", C.c_int32),
                ("plane_volume", C.c_int32 * METRICS_MAX_PLANES), ("plane_bit", C.c_int32 * METRICS_MAX_PLANES),
                ("volumes", C.c_void_p), ("out", C.c_void_p), ("stream", C.c_void_p),
                ("workspace", C.c_void_p), ("workspace_bytes", C.c_size_t)]


class PlanesBboxArgs(C.Structure):
    _fields_ = [("depth", C.c_int32), ("height", C.c_int32), ("width", C.c_int32),
                ("n_volumes", C.c_int32), ("n_items", C.c_int32), ("reserved", C.c_int32),
                ("item_volume", C.c_int32 * METRICS_MAX_PLANES), ("item_bit", C.c_int32 * METRICS_MAX_PLANES),
                ("item_volume2", C.c_int32 * METRICS_MAX_PLANES), ("item_bit2", C.c_int32 * METRICS_MAX_PLANES),
                ("volumes", C.c_void_p), ("boxes", C.c_void_p), ("stream", C.c_void_p)]


class BorderDistancesArgs(C.Structure):
    _fields_ = [("voxels", C.c_int64), ("n_volumes", C.c_int32), ("n_planes", C.c_int32), ("n_items", C.c_int32), ("fp32", C.c_int32),
                ("border_volume", C.c_int32 * METRICS_MAX_PLANES), ("border_bit", C.c_int32 * METRICS_MAX_PLANES),
                ("edt_plane", C.c_int32 * METRICS_MAX_PLANES),
                ("out_offset", C.c_int64 * METRICS_MAX_PLANES), ("out_count", C.c_int64 * METRICS_MAX_PLANES), ("out_capacity", C.c_int64),
                ("borders", C.c_void_p), ("edt", C.c_void_p), ("out", C.c_void_p),
                ("workspace", C.c_void_p), ("workspace_bytes", C.c_size_t), ("stream", C.c_void_p)]


class BorderStatsArgs(C.Structure):
    _fields_ = [("voxels", C.c_int64), ("n_volumes", C.c_int32), ("n_planes", C.c_int32), ("n_items", C.c_int32), ("n_groups", C.c_int32),
                ("fp32", C.c_int32), ("reserved", C.c_int32),
                ("border_volume", C.c_int32 * METRICS_MAX_PLANES), ("border_bit", C.c_int32 * METRICS_MAX_PLANES),
                ("edt_plane", C.c_int32 * METRICS_MAX_PLANES), ("item_group", C.c_int32 * METRICS_MAX_PLANES),
                ("tolerance", C.c_float * METRICS_MAX_PLANES), ("rank", (C.c_int64 * 2) * METRICS_MAX_PLANES),
                ("borders", C.c_void_p), ("edt", C.c_void_p), ("out", C.c_void_p),
                ("workspace", C.c_void_p), ("workspace_bytes", C.c_size_t), ("stream", C.c_void_p)]


SDM_LABEL_U8, SDM_LABEL_I16, SDM_LABEL_I64 = 0, 1, 2                             # enum segm_sdm_label_dtype
SDM_COMPOSE_WORKSPACE_BYTES = 2 * METRICS_MAX_PLANES * 4                       # SEGM_SDM_COMPOSE_WORKSPACE_BYTES


class SdmMasksArgs(C.Structure):
    _fields_ = [("depth", C.c_int32), ("height", C.c_int32), ("width", C.c_int32),
                ("n", C.c_int32), ("n_regions", C.c_int32), ("label_dtype", C.c_int32),
                ("labels", C.c_void_p), ("table", C.c_void_p), ("inside", C.c_void_p), ("outside", C.c_void_p), ("edge", C.c_void_p),
                ("boundary", C.c_void_p), ("counts", C.c_void_p), ("stream", C.c_void_p)]


class SdmComposeArgs(C.Structure):
    _fields_ = [("voxels", C.c_int64), ("n_items", C.c_int32), ("n_volumes", C.c_int32), ("n_planes", C.c_int32), ("n_out_planes", C.c_int32),
                ("volume", C.c_int32 * METRICS_MAX_PLANES), ("bit", C.c_int32 * METRICS_MAX_PLANES),
                ("pos_plane", C.c_int32 * METRICS_MAX_PLANES), ("neg_plane", C.c_int32 * METRICS_MAX_PLANES),
                ("out_plane", C.c_int32 * METRICS_MAX_PLANES),
                ("edt", C.c_void_p), ("inside", C.c_void_p), ("edge", C.c_void_p), ("boundary", C.c_void_p), ("counts", C.c_void_p),
                ("sdf", C.c_void_p), ("sdm", C.c_void_p), ("edge_out", C.c_void_p),
                ("workspace", C.c_void_p), ("workspace_bytes", C.c_size_t), ("stream", C.c_void_p)]


RESAMPLE_MAX_CLASSES, CCL_MAX_VOXELS = 8, 2 ** 31 - 1                         # SEGM_RESAMPLE_MAX_CLASSES / SEGM_CCL_MAX_VOXELS
CCL_LARGEST, CCL_MIN_SIZE, CCL_FILL = 0, 1, 2                                  # enum segm_ccl_select_mode
RESAMPLE_CLASS_LIMIT = 32                                                      # SEGM_RESAMPLE_CLASS_LIMIT: what the C entry accepts


class ResampleArgmaxArgs(C.Structure):
    _fields_ = [("classes", C.c_int32), ("dtype", C.c_int32),
                ("in_depth", C.c_int32), ("in_height", C.c_int32), ("in_width", C.c_int32),
                ("box_z", C.c_int32), ("box_y", C.c_int32), ("box_x", C.c_int32),
                ("box_depth", C.c_int32), ("box_height", C.c_int32), ("box_width", C.c_int32),
                ("out_depth", C.c_int32), ("out_height", C.c_int32), ("out_width", C.c_int32),
                ("stride_c", C.c_int64), ("stride_z", C.c_int64), ("stride_y", C.c_int64),
                ("logits", C.c_void_p), ("labels", C.c_void_p), ("regions", C.c_void_p), ("table", C.c_void_p), ("stream", C.c_void_p)]


class CclRootsArgs(C.Structure):
    _fields_ = [("depth", C.c_int32), ("height", C.c_int32), ("width", C.c_int32), ("bit", C.c_int32),
                ("invert", C.c_int32), ("reserved", C.c_int32),
                ("volume", C.c_void_p), ("roots", C.c_void_p), ("workspace", C.c_void_p), ("workspace_bytes", C.c_size_t),
                ("stream", C.c_void_p)]


class CclSizesArgs(C.Structure):
    _fields_ = [("depth", C.c_int32), ("height", C.c_int32), ("width", C.c_int32), ("reserved", C.c_int32),
                ("roots", C.c_void_p), ("sizes", C.c_void_p), ("touches", C.c_void_p), ("stream", C.c_void_p)]


class CclSelectArgs(C.Structure):
    _fields_ = [("depth", C.c_int32), ("height", C.c_int32), ("width", C.c_int32),
                ("mode", C.c_int32), ("min_size", C.c_int32), ("reserved", C.c_int32),
                ("roots", C.c_void_p), ("sizes", C.c_void_p), ("touches", C.c_void_p), ("out", C.c_void_p), ("info", C.c_void_p),
                ("workspace", C.c_void_p), ("workspace_bytes", C.c_size_t), ("stream", C.c_void_p)]


class CclLabelRootsArgs(C.Structure):
    _fields_ = [("depth", C.c_int32), ("height", C.c_int32), ("width", C.c_int32), ("reserved", C.c_int32),
                ("labels", C.c_void_p), ("roots", C.c_void_p), ("workspace", C.c_void_p), ("workspace_bytes", C.c_size_t),
                ("stream", C.c_void_p)]


class CclRootsConnArgs(C.Structure):
    _fields_ = [("depth", C.c_int32), ("height", C.c_int32), ("width", C.c_int32), ("bit", C.c_int32),
                ("invert", C.c_int32), ("connectivity", C.c_int32),
                ("volume", C.c_void_p), ("roots", C.c_void_p), ("workspace", C.c_void_p), ("workspace_bytes", C.c_size_t),
                ("stream", C.c_void_p)]


class CclLabelRootsConnArgs(C.Structure):
    _fields_ = [("depth", C.c_int32), ("height", C.c_int32), ("width", C.c_int32), ("connectivity", C.c_int32),
                ("labels", C.c_void_p), ("roots", C.c_void_p), ("workspace", C.c_void_p), ("workspace_bytes", C.c_size_t),
                ("stream", C.c_void_p)]


class CclLabelSelectArgs(C.Structure):
    _fields_ = [("depth", C.c_int32), ("height", C.c_int32), ("width", C.c_int32),
                ("mode", C.c_int32), ("min_size", C.c_int32), ("reserved", C.c_int32),
                ("labels", C.c_void_p), ("roots", C.c_void_p), ("sizes", C.c_void_p), ("apply", C.c_void_p), ("out", C.c_void_p),
                ("info", C.c_void_p), ("workspace", C.c_void_p), ("workspace_bytes", C.c_size_t), ("stream", C.c_void_p)]


PREP_MAX_CHANNELS, PREP_COUNT_BINS = 8, 260                                    # SEGM_PREP_MAX_CHANNELS / SEGM_PREP_COUNT_BINS
PREP_BIN_MINUS, PREP_BIN_ABOVE, PREP_BIN_INVALID = 256, 257, 258               # the bins of segm_crop_normalize's counts past the labels
PREP_SEG_NONE, PREP_SEG_F32, PREP_SEG_U8, PREP_SEG_I16 = 0, 1, 2, 3            # enum segm_prep_seg_dtype


class NonzeroMaskBboxArgs(C.Structure):
    _fields_ = [("channels", C.c_int32), ("depth", C.c_int32), ("height", C.c_int32), ("width", C.c_int32),
                ("stride_c", C.c_int64), ("stride_z", C.c_int64), ("stride_y", C.c_int64),
                ("data", C.c_void_p), ("mask", C.c_void_p), ("bbox", C.c_void_p), ("stream", C.c_void_p)]


class CropArgs(C.Structure):
    _fields_ = [("channels", C.c_int32), ("depth", C.c_int32), ("height", C.c_int32), ("width", C.c_int32),
                ("box_z", C.c_int32), ("box_y", C.c_int32), ("box_x", C.c_int32),
                ("box_depth", C.c_int32), ("box_height", C.c_int32), ("box_width", C.c_int32),
                ("seg_dtype", C.c_int32), ("masked", C.c_int32), ("nonzero_label", C.c_int32), ("reserved", C.c_int32),
                ("stride_c", C.c_int64), ("stride_z", C.c_int64), ("stride_y", C.c_int64),
                ("data", C.c_void_p), ("mask", C.c_void_p), ("seg", C.c_void_p),
                ("stats64", C.c_void_p), ("stats32", C.c_void_p), ("out", C.c_void_p), ("seg_out", C.c_void_p), ("counts", C.c_void_p),
                ("workspace", C.c_void_p), ("workspace_bytes", C.c_size_t), ("stream", C.c_void_p)]


FG_SEGMENT, FG_MAX_RANKS, FG_MAX_INDICES = 4096, 8, 1 << 24                     # SEGM_FG_SEGMENT / _MAX_RANKS / _MAX_INDICES


class FgArgs(C.Structure):
    _fields_ = [("channels", C.c_int32), ("depth", C.c_int32), ("height", C.c_int32), ("width", C.c_int32),
                ("seg_dtype", C.c_int32), ("n_ranks", C.c_int32),
                ("stride_c", C.c_int64), ("stride_z", C.c_int64), ("stride_y", C.c_int64),
                ("data", C.c_void_p), ("seg", C.c_void_p),
                ("n", C.c_int64), ("ranks", C.c_int64 * FG_MAX_RANKS),
                ("idx", C.c_void_p), ("n_idx", C.c_int64), ("idx_stride_c", C.c_int64),
                ("count", C.c_void_p), ("sums", C.c_void_p), ("out", C.c_void_p),
                ("workspace", C.c_void_p), ("workspace_bytes", C.c_size_t), ("stream", C.c_void_p)]


TOPK_RESULT_BYTES = 32                                                         # SEGM_TOPK_RESULT_BYTES


class CrossEntropyMapArgs(C.Structure):
    _fields_ = [("batch", C.c_int32), ("classes", C.c_int32), ("dtype", C.c_int32), ("reserved", C.c_int32),
                ("spatial", C.c_int64), ("ignore_index", C.c_int64),
                ("logits", C.c_void_p), ("labels", C.c_void_p), ("loss_map", C.c_void_p), ("dlogits", C.c_void_p),
                ("coef", C.c_void_p), ("scale", C.c_void_p), ("select", C.c_void_p), ("kk", C.c_int64), ("stream", C.c_void_p)]


class TopkSelectArgs(C.Structure):
    _fields_ = [("values", C.c_void_p), ("n", C.c_int64), ("kk", C.c_int64), ("result", C.c_void_p),
                ("workspace", C.c_void_p), ("workspace_bytes", C.c_size_t), ("stream", C.c_void_p)]


REGION_MAX_REGIONS = 8                                                         # SEGM_REGION_MAX_REGIONS
# enum segm_region_target, by the target's dtype (bool is viewed as uint8 by the caller)
REGION_LABELS = {torch.int64: 0, torch.int16: 1, torch.uint8: 2, torch.float32: 3}
REGION_PLANES = {torch.uint8: 4, torch.float32: 5}


class RegionLossArgs(C.Structure):
    _fields_ = [("batch", C.c_int32), ("regions", C.c_int32), ("dtype", C.c_int32), ("target_kind", C.c_int32),
                ("depth", C.c_int32), ("height", C.c_int32), ("width", C.c_int32), ("ignore_plane", C.c_int32),
                ("has_ignore", C.c_int32), ("reserved", C.c_int32), ("ignore_label", C.c_int64),
                ("stride_b", C.c_int64), ("stride_r", C.c_int64), ("stride_z", C.c_int64), ("stride_y", C.c_int64),
                ("stride_x", C.c_int64),
                ("masks", C.c_uint32 * REGION_MAX_REGIONS),
                ("logits", C.c_void_p), ("target", C.c_void_p), ("sums", C.c_void_p),
                ("g_i", C.c_void_p), ("g_p", C.c_void_p), ("g_e", C.c_void_p), ("dlogits", C.c_void_p),
                ("workspace", C.c_void_p), ("workspace_bytes", C.c_size_t), ("stream", C.c_void_p)]


SOFTMAX_DICE_MAX_CLASSES = 16                                                  # SEGM_SOFTMAX_DICE_MAX_CLASSES


class SoftmaxDiceArgs(C.Structure):
    _fields_ = [("batch", C.c_int32), ("classes", C.c_int32), ("dtype", C.c_int32), ("label_kind", C.c_int32),
                ("depth", C.c_int32), ("height", C.c_int32), ("width", C.c_int32), ("has_ignore", C.c_int32),
                ("ignore_label", C.c_int64),
                ("stride_b", C.c_int64), ("stride_c", C.c_int64), ("stride_z", C.c_int64), ("stride_y", C.c_int64),
                ("stride_x", C.c_int64),
                ("logits", C.c_void_p), ("labels", C.c_void_p), ("mask", C.c_void_p), ("sums", C.c_void_p),
                ("g_i", C.c_void_p), ("g_p", C.c_void_p), ("g_ce", C.c_void_p), ("dlogits", C.c_void_p),
                ("workspace", C.c_void_p), ("workspace_bytes", C.c_size_t), ("stream", C.c_void_p)]


ZOOM_MAX_SIDE = 2048                                                           # SEGM_ZOOM_MAX_SIDE


class ZoomArgs(C.Structure):
    _fields_ = [("channels", C.c_int32), ("depth", C.c_int32), ("height", C.c_int32), ("width", C.c_int32),
                ("out_depth", C.c_int32), ("out_height", C.c_int32), ("out_width", C.c_int32),
                ("order", C.c_int32), ("clip", C.c_int32), ("reserved", C.c_int32),
                ("stride_c", C.c_int64), ("stride_z", C.c_int64), ("stride_y", C.c_int64),
                ("data", C.c_void_p), ("out", C.c_void_p),
                ("workspace", C.c_void_p), ("workspace_bytes", C.c_size_t), ("stream", C.c_void_p)]


class ZoomLabelsArgs(C.Structure):
    _fields_ = [("depth", C.c_int32), ("height", C.c_int32), ("width", C.c_int32),
                ("out_depth", C.c_int32), ("out_height", C.c_int32), ("out_width", C.c_int32),
                ("seg", C.c_void_p), ("out", C.c_void_p), ("counts", C.c_void_p), ("stream", C.c_void_p)]


class ZoomSlicesArgs(C.Structure):
    _fields_ = [("channels", C.c_int32), ("slices", C.c_int32), ("height", C.c_int32), ("width", C.c_int32),
                ("out_slices", C.c_int32), ("out_height", C.c_int32), ("out_width", C.c_int32),
                ("order", C.c_int32), ("clip", C.c_int32), ("reserved", C.c_int32),
                ("stride_c", C.c_int64), ("stride_s", C.c_int64), ("stride_y", C.c_int64),
                ("data", C.c_void_p), ("source", C.c_void_p), ("out", C.c_void_p),
                ("workspace", C.c_void_p), ("workspace_bytes", C.c_size_t), ("stream", C.c_void_p)]


class ZoomLabelsSlicesArgs(C.Structure):
    _fields_ = [("slices", C.c_int32), ("height", C.c_int32), ("width", C.c_int32),
                ("out_slices", C.c_int32), ("out_height", C.c_int32), ("out_width", C.c_int32),
                ("seg", C.c_void_p), ("source", C.c_void_p), ("out", C.c_void_p), ("counts", C.c_void_p), ("stream", C.c_void_p)]


AUG_MAX_SAMPLES, AUG_MAX_VOLUMES, BLUR_MAX_RADIUS = 8, 64, 4                   # SEGM_AUG_MAX_SAMPLES / _VOLUMES, SEGM_BLUR_MAX_RADIUS


class SplineCoefsArgs(C.Structure):
    _fields_ = [("samples", C.c_int32), ("channels", C.c_int32), ("depth", C.c_int32), ("height", C.c_int32), ("width", C.c_int32),
                ("reserved", C.c_int32),
                ("stride_n", C.c_int64), ("stride_c", C.c_int64), ("stride_z", C.c_int64), ("stride_y", C.c_int64),
                ("on", C.c_uint8 * AUG_MAX_SAMPLES),
                ("data", C.c_void_p), ("workspace", C.c_void_p), ("workspace_bytes", C.c_size_t), ("stream", C.c_void_p)]


class AffineSpline3Args(C.Structure):
    _fields_ = [("samples", C.c_int32), ("channels", C.c_int32), ("depth", C.c_int32), ("height", C.c_int32), ("width", C.c_int32),
                ("reserved", C.c_int32),
                ("stride_n", C.c_int64), ("stride_c", C.c_int64), ("stride_z", C.c_int64), ("stride_y", C.c_int64),
                ("matrix", (C.c_double * 12) * AUG_MAX_SAMPLES),
                ("cval", C.c_float), ("reserved2", C.c_int32),
                ("on", C.c_uint8 * AUG_MAX_SAMPLES),
                ("data", C.c_void_p), ("coefs", C.c_void_p), ("out", C.c_void_p), ("stream", C.c_void_p)]


class AffineLabelsArgs(C.Structure):
    _fields_ = [("samples", C.c_int32), ("depth", C.c_int32), ("height", C.c_int32), ("width", C.c_int32), ("wide", C.c_int32),
                ("reserved", C.c_int32),
                ("matrix", (C.c_double * 12) * AUG_MAX_SAMPLES),
                ("on", C.c_uint8 * AUG_MAX_SAMPLES),
                ("seg", C.c_void_p), ("out", C.c_void_p), ("stream", C.c_void_p)]


class ZoomNearestArgs(C.Structure):
    _fields_ = [("channels", C.c_int32), ("depth", C.c_int32), ("height", C.c_int32), ("width", C.c_int32),
                ("out_depth", C.c_int32), ("out_height", C.c_int32), ("out_width", C.c_int32), ("reserved", C.c_int32),
                ("stride_c", C.c_int64), ("stride_z", C.c_int64), ("stride_y", C.c_int64),
                ("data", C.c_void_p), ("out", C.c_void_p), ("stream", C.c_void_p)]


class GaussBlurArgs(C.Structure):
    _fields_ = [("samples", C.c_int32), ("channels", C.c_int32), ("depth", C.c_int32), ("height", C.c_int32), ("width", C.c_int32),
                ("reserved", C.c_int32),
                ("stride_n", C.c_int64), ("stride_c", C.c_int64), ("stride_z", C.c_int64), ("stride_y", C.c_int64),
                ("sigma", C.c_double * AUG_MAX_VOLUMES), ("on", C.c_uint8 * AUG_MAX_VOLUMES),
                ("data", C.c_void_p), ("out", C.c_void_p), ("workspace", C.c_void_p), ("workspace_bytes", C.c_size_t),
                ("stream", C.c_void_p)]


# SEGM_INTENSITY_*: the op of a plane, and the doubles of a statistics row (count, mean, population sd, min, max, zeros)
INTENSITY_OFF, INTENSITY_NOISE, INTENSITY_SCALE, INTENSITY_CONTRAST, INTENSITY_GAMMA = 0, 1, 2, 3, 4
INTENSITY_STATS_DOUBLES = 8


class IntensityArgs(C.Structure):
    _fields_ = [("samples", C.c_int32), ("channels", C.c_int32), ("depth", C.c_int32), ("height", C.c_int32), ("width", C.c_int32),
                ("stage", C.c_int32),
                ("stride_n", C.c_int64), ("stride_c", C.c_int64), ("stride_z", C.c_int64), ("stride_y", C.c_int64),
                ("stride_x", C.c_int64),
                ("out_stride_n", C.c_int64), ("out_stride_c", C.c_int64), ("out_stride_z", C.c_int64), ("out_stride_y", C.c_int64),
                ("op", C.c_uint8 * AUG_MAX_VOLUMES), ("invert", C.c_uint8 * AUG_MAX_VOLUMES), ("mirror", C.c_uint8 * AUG_MAX_VOLUMES),
                ("a", C.c_float * AUG_MAX_VOLUMES), ("b", C.c_float * AUG_MAX_VOLUMES),
                ("noise", C.c_void_p * AUG_MAX_VOLUMES),
                ("data", C.c_void_p), ("out", C.c_void_p), ("stats", C.c_void_p), ("stats2", C.c_void_p),
                ("workspace", C.c_void_p), ("workspace_bytes", C.c_size_t), ("stream", C.c_void_p)]


STITCH_MAX_WINDOWS, STITCH_MAX_STARTS = 64, 64                                  # SEGM_STITCH_MAX_*


class StitchArgs(C.Structure):
    _fields_ = [("batch", C.c_int32), ("channels", C.c_int32), ("size", C.c_int32 * 3), ("roi", C.c_int32 * 3),
                ("n_windows", C.c_int32), ("mirror", C.c_int32), ("dtype", C.c_int32), ("pass_", C.c_int32), ("passes", C.c_int32),
                ("cval", C.c_float), ("n_starts", C.c_int32 * 3), ("reserved", C.c_int32),
                ("window", (C.c_int32 * 4) * STITCH_MAX_WINDOWS), ("starts", (C.c_int32 * STITCH_MAX_STARTS) * 3),
                ("stride_b", C.c_int64), ("stride_c", C.c_int64), ("stride_z", C.c_int64), ("stride_y", C.c_int64),
                ("stride_x", C.c_int64),
                ("volume", C.c_void_p), ("windows_out", C.c_void_p), ("weight", C.c_void_p), ("count", C.c_void_p),
                ("pred", C.c_void_p), ("acc", C.c_void_p), ("total", C.c_void_p), ("stream", C.c_void_p)]


ADD_NORM_MAX_COLS = 8192                                                       # SEGM_ADD_NORM_MAX_COLS


class AddNormArgs(C.Structure):
    _fields_ = [("rows", C.c_int64), ("cols", C.c_int32), ("dtype", C.c_int32), ("res_dtype", C.c_int32), ("rms", C.c_int32),
                ("eps", C.c_float), ("reserved", C.c_int32),
                ("x", C.c_void_p), ("x_stride", C.c_int64), ("residual", C.c_void_p), ("residual_stride", C.c_int64),
                ("y", C.c_void_p), ("y_stride", C.c_int64), ("residual_out", C.c_void_p), ("residual_out_stride", C.c_int64),
                ("weight", C.c_void_p), ("bias", C.c_void_p), ("mean", C.c_void_p), ("rstd", C.c_void_p),
                ("dy", C.c_void_p), ("dy_stride", C.c_int64), ("dresidual", C.c_void_p), ("dresidual_stride", C.c_int64),
                ("dx", C.c_void_p), ("dx_stride", C.c_int64), ("dresidual_in", C.c_void_p), ("dresidual_in_stride", C.c_int64),
                ("dweight", C.c_void_p), ("dbias", C.c_void_p),
                ("workspace", C.c_void_p), ("workspace_bytes", C.c_size_t), ("stream", C.c_void_p)]


def header_abi_version() -> int:
    """SEGM_ABI_VERSION as include/segmamba_hip.h declares it (what a freshly built library must report)"""
    import re
    hdr = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "segmamba_hip.h")
    m = re.search(r"#define\s+SEGM_ABI_VERSION\s+(\d+)", open(hdr).read())
    if not m:
        raise RuntimeError("include/segmamba_hip.h does not define SEGM_ABI_VERSION")
    return int(m.group(1))


class SegmLib:
    """A loaded C-ABI library (the HIP one in production; tests may load the CPU emulation build)."""

    def __init__(self, path: str):
        self.path = path
        self.dll = C.CDLL(path)
        d = self.dll
        self.missing = [n for n in EXPORTS if not hasattr(d, n)]

        def sig(name, argtypes, restype):
            if hasattr(d, name):
                fn = getattr(d, name)
                fn.argtypes, fn.restype = argtypes, restype

        sig("segm_selective_scan_fwd", [C.POINTER(ScanFwdArgs)], C.c_int)
        sig("segm_selective_scan_bwd", [C.POINTER(ScanBwdArgs)], C.c_int)
        sig("segm_selective_scan_bwd_deterministic", [C.POINTER(ScanBwdArgs)], C.c_int)
        sig("segm_selective_scan_fwd_multi", [C.POINTER(ScanFwdArgs), C.c_int32], C.c_int)
        sig("segm_selective_scan_bwd_multi", [C.POINTER(ScanBwdArgs), C.c_int32], C.c_int)
        for n in ("segm_selective_scan_fwd_workspace_bytes", "segm_selective_scan_bwd_workspace_bytes"):
            sig(n, [C.c_int32, C.c_int32, C.c_int32, C.c_int64, C.c_int32], C.c_size_t)
        sig("segm_selective_scan_ckpt_bytes", [C.c_int32, C.c_int32, C.c_int32, C.c_int64], C.c_size_t)
        sig("segm_selective_scan_default_chunk", [C.c_int32, C.c_int32, C.c_int64], C.c_int32)
        sig("segm_causal_conv1d_fwd", [C.POINTER(Conv1dArgs)], C.c_int)
        sig("segm_causal_conv1d_bwd", [C.POINTER(Conv1dArgs)], C.c_int)
        sig("segm_causal_conv1d_fwd_multi", [C.POINTER(Conv1dArgs), C.c_int32], C.c_int)
        sig("segm_causal_conv1d_bwd_multi", [C.POINTER(Conv1dArgs), C.c_int32], C.c_int)
        sig("segm_causal_conv1d_bwd_workspace_bytes", [C.c_int32, C.c_int32, C.c_int32, C.c_int64], C.c_size_t)
        sig("segm_conv3d_k3_wgrad", [C.POINTER(Conv3dWgradArgs)], C.c_int)
        sig("segm_conv3d_k3_wgrad_workspace_bytes", [C.c_int32] * 6, C.c_size_t)
        sig("segm_conv3d_k3_fwd", [C.POINTER(Conv3dFwdArgs)], C.c_int)
        sig("segm_conv3d_k3_fwd_stats_parts", [C.c_int32] * 6, C.c_int32)
        sig("segm_conv3d_k3_fwd_cl", [C.POINTER(Conv3dClArgs)], C.c_int)
        sig("segm_conv3d_k3_cl_pack_index", [C.c_void_p, C.c_int64], C.c_int)
        sig("segm_conv3d_k3_cube_fwd", [C.POINTER(Conv3dCubeArgs)], C.c_int)
        sig("segm_conv3d_k3_cube_plan", [C.c_int32] * 6 + [C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int64)], C.c_int)
        sig("segm_conv3d_k3_cube_pack_index", [C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_int32], C.c_int)
        sig("segm_conv3d_k3_cube_wgrad", [C.POINTER(Conv3dWgradArgs)], C.c_int)
        sig("segm_conv3d_k3_cube_stats_parts", [C.c_int32] * 4, C.c_int32)
        sig("segm_conv3d_k3_cube_pack_multi", [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p], C.c_int)
        sig("segm_conv3d_k3_cube_wgrad_workspace_bytes", [C.c_int32] * 6, C.c_size_t)
        sig("segm_add3", [C.POINTER(Add3Args)], C.c_int)
        sig("segm_gather16", [C.POINTER(Gather16Args)], C.c_int)
        sig("segm_instnorm_fwd", [C.POINTER(InstNormFwdArgs)], C.c_int)
        sig("segm_instnorm_bwd", [C.POINTER(InstNormBwdArgs)], C.c_int)
        sig("segm_instnorm_workspace_bytes", [C.c_int32, C.c_int64], C.c_size_t)
        sig("segm_instnorm_stats", [C.POINTER(InstNormStatsArgs)], C.c_int)
        sig("segm_instnorm_tail_fwd", [C.POINTER(InstNormTailFwdArgs)], C.c_int)
        sig("segm_instnorm_tail_bwd", [C.POINTER(InstNormTailBwdArgs)], C.c_int)
        sig("segm_instnorm_tail_workspace_bytes", [C.c_int32, C.c_int64], C.c_size_t)
        sig("segm_transpose_add", [C.POINTER(TransposeArgs)], C.c_int)
        sig("segm_depth_to_space2", [C.POINTER(D2sArgs)], C.c_int)
        sig("segm_layernorm_tokens_fwd", [C.POINTER(LayerNormArgs)], C.c_int)
        sig("segm_layernorm_tokens_bwd", [C.POINTER(LayerNormArgs)], C.c_int)
        sig("segm_layernorm_tokens_workspace_bytes", [C.c_int32, C.c_int32, C.c_int64], C.c_size_t)
        sig("segm_sgd_clip_step", [C.POINTER(SgdArgs)], C.c_int)
        sig("segm_sgd_clip_step_workspace_bytes", [C.c_int32, C.c_void_p], C.c_size_t)
        sig("segm_cross_entropy", [C.POINTER(CrossEntropyArgs)], C.c_int)
        sig("segm_cross_entropy_partials", [C.c_int32, C.c_int64], C.c_int32)
        sig("segm_causal_conv1d_update", [C.POINTER(Conv1dUpdateArgs)], C.c_int)
        sig("segm_selective_state_update", [C.POINTER(StateUpdateArgs)], C.c_int)
        sig("segm_linear_rows", [C.POINTER(LinearArgs)], C.c_int)
        sig("segm_pointwise_cf", [C.POINTER(PointwiseArgs)], C.c_int)
        sig("segm_stem_conv_fwd", [C.POINTER(StemArgs)], C.c_int)
        sig("segm_stem_conv_wgrad", [C.POINTER(StemWgradArgs)], C.c_int)
        sig("segm_stem_conv_wgrad_workspace_bytes", [C.c_int32] * 4, C.c_size_t)
        sig("segm_stem_conv_wgrad_workspace_bytes2", [C.c_int32] * 6, C.c_size_t)
        sig("segm_wgrad_gemm", [C.POINTER(WgradGemmArgs)], C.c_int)
        sig("segm_wgrad_gemm_workspace_bytes", [C.c_int32, C.c_int32, C.c_int32, C.c_int64, C.c_int32], C.c_size_t)
        sig("segm_skinny_tn", [C.POINTER(SkinnyTnArgs)], C.c_int)
        sig("segm_skinny_tn_workspace_bytes", [C.c_int32, C.c_int32, C.c_int64], C.c_size_t)
        sig("segm_selective_scan_regular_shape", [C.c_int32, C.c_int32, C.c_int32, C.c_int64, C.c_int32, C.c_int32, C.c_int32], C.c_int32)
        sig("segm_channel_sum", [C.POINTER(ChannelSumArgs)], C.c_int)
        sig("segm_channel_sum_workspace_bytes", [C.c_int32, C.c_int32, C.c_int64], C.c_size_t)
        sig("segm_seg_regions", [C.POINTER(SegRegionsArgs)], C.c_int)
        sig("segm_seg_regions_workspace_bytes", [C.c_int64], C.c_size_t)
        sig("segm_edt_sq", [C.POINTER(EdtSqArgs)], C.c_int)
        sig("segm_border_distances", [C.POINTER(BorderDistancesArgs)], C.c_int)
        sig("segm_border_distances_workspace_bytes", [C.c_int64, C.c_int32], C.c_size_t)
        sig("segm_border_stats", [C.POINTER(BorderStatsArgs)], C.c_int)
        sig("segm_border_stats_workspace_bytes", [C.c_int64, C.c_int32], C.c_size_t)
        sig("segm_edt_sq_long", [C.POINTER(EdtSqLongArgs)], C.c_int)
        sig("segm_edt_sq_long_workspace_bytes", [C.c_int32] * 5, C.c_size_t)
        sig("segm_planes_bbox", [C.POINTER(PlanesBboxArgs)], C.c_int)
        sig("segm_sdm_masks", [C.POINTER(SdmMasksArgs)], C.c_int)
        sig("segm_sdm_compose", [C.POINTER(SdmComposeArgs)], C.c_int)
        sig("segm_resample_argmax", [C.POINTER(ResampleArgmaxArgs)], C.c_int)
        sig("segm_ccl_roots", [C.POINTER(CclRootsArgs)], C.c_int)
        sig("segm_ccl_roots_workspace_bytes", [C.c_int64], C.c_size_t)
        sig("segm_ccl_sizes", [C.POINTER(CclSizesArgs)], C.c_int)
        sig("segm_ccl_select", [C.POINTER(CclSelectArgs)], C.c_int)
        sig("segm_ccl_select_workspace_bytes", [C.c_int64], C.c_size_t)
        sig("segm_ccl_label_roots", [C.POINTER(CclLabelRootsArgs)], C.c_int)
        sig("segm_ccl_label_roots_workspace_bytes", [C.c_int64], C.c_size_t)
        sig("segm_ccl_label_select", [C.POINTER(CclLabelSelectArgs)], C.c_int)
        sig("segm_ccl_label_select_workspace_bytes", [C.c_int64], C.c_size_t)
        sig("segm_ccl_roots_conn", [C.POINTER(CclRootsConnArgs)], C.c_int)
        sig("segm_ccl_label_roots_conn", [C.POINTER(CclLabelRootsConnArgs)], C.c_int)
        sig("segm_nonzero_mask_bbox", [C.POINTER(NonzeroMaskBboxArgs)], C.c_int)
        sig("segm_crop_stats", [C.POINTER(CropArgs)], C.c_int)
        sig("segm_crop_stats_workspace_bytes", [C.c_int32] * 4, C.c_size_t)
        sig("segm_crop_normalize", [C.POINTER(CropArgs)], C.c_int)
        sig("segm_crop_clip_normalize", [C.POINTER(CropArgs)], C.c_int)
        sig("segm_fg_workspace_bytes", [C.c_int32, C.c_int64], C.c_size_t)
        sig("segm_fg_count", [C.POINTER(FgArgs)], C.c_int)
        sig("segm_fg_order_stats", [C.POINTER(FgArgs)], C.c_int)
        sig("segm_fg_gather", [C.POINTER(FgArgs)], C.c_int)
        sig("segm_cross_entropy_map", [C.POINTER(CrossEntropyMapArgs)], C.c_int)
        sig("segm_cross_entropy_map_bwd", [C.POINTER(CrossEntropyMapArgs)], C.c_int)
        sig("segm_topk_select", [C.POINTER(TopkSelectArgs)], C.c_int)
        sig("segm_topk_select_workspace_bytes", [C.c_int64], C.c_size_t)
        sig("segm_region_loss_workspace_bytes", [C.c_int32, C.c_int32, C.c_int64], C.c_size_t)
        sig("segm_region_loss_fwd", [C.POINTER(RegionLossArgs)], C.c_int)
        sig("segm_region_loss_bwd", [C.POINTER(RegionLossArgs)], C.c_int)
        sig("segm_softmax_dice_workspace_bytes", [C.c_int32, C.c_int32, C.c_int64], C.c_size_t)
        sig("segm_softmax_dice_fwd", [C.POINTER(SoftmaxDiceArgs)], C.c_int)
        sig("segm_softmax_dice_bwd", [C.POINTER(SoftmaxDiceArgs)], C.c_int)
        sig("segm_zoom", [C.POINTER(ZoomArgs)], C.c_int)
        sig("segm_zoom_workspace_bytes", [C.c_int32] * 5, C.c_size_t)
        sig("segm_zoom_labels", [C.POINTER(ZoomLabelsArgs)], C.c_int)
        sig("segm_zoom_slices", [C.POINTER(ZoomSlicesArgs)], C.c_int)
        sig("segm_zoom_slices_workspace_bytes", [C.c_int32] * 7, C.c_size_t)
        sig("segm_zoom_labels_slices", [C.POINTER(ZoomLabelsSlicesArgs)], C.c_int)
        sig("segm_spline_coefs", [C.POINTER(SplineCoefsArgs)], C.c_int)
        sig("segm_spline_coefs_workspace_bytes", [C.c_int32] * 5, C.c_size_t)
        sig("segm_affine_spline3", [C.POINTER(AffineSpline3Args)], C.c_int)
        sig("segm_affine_labels", [C.POINTER(AffineLabelsArgs)], C.c_int)
        sig("segm_zoom_nearest", [C.POINTER(ZoomNearestArgs)], C.c_int)
        sig("segm_gauss_blur", [C.POINTER(GaussBlurArgs)], C.c_int)
        sig("segm_intensity_workspace_bytes", [C.c_int32, C.c_int64], C.c_size_t)
        sig("segm_intensity_stats", [C.POINTER(IntensityArgs)], C.c_int)
        sig("segm_intensity_apply", [C.POINTER(IntensityArgs)], C.c_int)
        for n in ("segm_window_gather", "segm_window_count", "segm_window_blend", "segm_window_finish"):
            sig(n, [C.POINTER(StitchArgs)], C.c_int)
        sig("segm_add_norm_fwd", [C.POINTER(AddNormArgs)], C.c_int)
        sig("segm_add_norm_bwd", [C.POINTER(AddNormArgs)], C.c_int)
        sig("segm_add_norm_workspace_bytes", [C.c_int64, C.c_int32], C.c_size_t)
        sig("segm_abi_version", [], C.c_int)
        sig("segm_status_string", [C.c_int], C.c_char_p)

    def check(self, rc: int, what: str) -> None:
        if rc == 0:
            return
        if rc < 0:
            msg = _STATUS.get(rc, "unknown status")
            raise RuntimeError(f"{what}: {msg} (status {rc})")
        raise RuntimeError(f"{what}: HIP error {rc}")


_lib: Optional[SegmLib] = None


def get_lib() -> SegmLib:
    """The HIP library.  Raises if it has not been built - the product never falls back to anything else."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(hipcc --offload-arch=gfx950).  segmamba_amd has no CPU / PyTorch fallback for its kernels.")
        _lib = SegmLib(LIB_PATH)
    return _lib


# ---------------------------------------------------------------------------------------------------------
# tensor -> view descriptors
# ---------------------------------------------------------------------------------------------------------
def dtype_code(t: torch.Tensor) -> int:
    try:
        return _DTYPES[t.dtype]
    except KeyError:
        raise RuntimeError(f"unsupported dtype {t.dtype}: expected float32, float16 or bfloat16") from None


def seq_view(t: Optional[torch.Tensor], channel_last: bool) -> SegmSeq:
    """Descriptor of a 3-D tensor: (B, L, D) if channel_last else (B, D, L)."""
    if t is None:
        return SegmSeq(None, 0, 0, 0)
    assert t.dim() == 3
    sb, s1, s2 = t.stride()
    return SegmSeq(t.data_ptr(), sb, s1, s2) if channel_last else SegmSeq(t.data_ptr(), sb, s2, s1)


def bc_view(t: torch.Tensor, channel_last: bool) -> SegmBC:
    """Descriptor of B / C: (B, L, G, N) if channel_last else (B, G, N, L)."""
    assert t.dim() == 4
    s = t.stride()
    if channel_last:
        return SegmBC(t.data_ptr(), s[0], s[2], s[1], s[3])
    return SegmBC(t.data_ptr(), s[0], s[1], s[3], s[2])


def on_device(t: torch.Tensor) -> bool:
    """Whether `t` takes the library's kernels (CUDA tensors do).  Host modules ask this instead of `t.is_cuda` so that the
    CPU tests can send CPU tensors through the emulated kernels; the product never patches it."""
    return t.is_cuda


def stream_handle(t: torch.Tensor) -> Optional[int]:
    if t.is_cuda:
        return torch.cuda.current_stream(t.device).cuda_stream
    return None


def fptr(t: Optional[torch.Tensor]):
    return None if t is None else t.data_ptr()
