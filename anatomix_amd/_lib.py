"""ctypes binding of the C ABI in ``include/anatomix_amd.h`` (libanatomix_amd.so, built in-tree by
``anatomix_amd/csrc/Makefile``).  There is no CPU implementation behind these symbols: if the
shared library is missing the import of the HIP path fails loudly."""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# AMX_LIB_PATH (read here, by the Python loader, never by the library): another build of the same sources, e.g. a parent
# commit's library for an A/B against this tree
LIB_PATH = os.environ.get("AMX_LIB_PATH") or os.path.join(_HERE, "csrc", "libanatomix_amd.so")

NORM = {"none": 0, "batch": 1, "instance": 2, "instance_affine": 3}
ACT = {"none": 0, "relu": 1, "lrelu": 2}
POOL = {"Max": 0, "Avg": 1}
INTERP = {"nearest": 0, "trilinear": 1}
WARP = {"bilinear": 0, "nearest": 1}
SEG_LABEL = {"float32": 0, "int64": 1, "uint8": 2}
SW_MAP = {"constant": 0, "gaussian": 1}
SW_OUT = {"features": 0, "logits": 1, "labels": 2}
# "strict" = bf16x2: split hi + lo operands, fp32-grade results with fp32's exponent range (include/anatomix_amd.h)
# "f16x2mx" (alias "strict_mx") = f16 hi + lo pairs whose correction products run on the block-scaled fp8 MFMA (2 instead of 3 MFMA-
# equivalents per product); implemented for the InstanceNorm configurations, where it is the default (Unet.precision)
PRECISION = {"f16": 0, "fp16": 0, "float16": 0, "bf16": 1, "bfloat16": 1, "f16x2": 2, "bf16x2": 3, "strict": 3, "fp32": 3,
             "f16x2mx": 4, "strict_mx": 4}


class UnetCfg(C.Structure):
    _fields_ = [
        ("input_nc", C.c_int32), ("output_nc", C.c_int32), ("num_downs", C.c_int32), ("ngf", C.c_int32),
        ("norm", C.c_int32), ("norm_eps", C.c_float), ("activation", C.c_int32), ("act_slope", C.c_float),
        ("final_act", C.c_int32), ("pooling", C.c_int32), ("interp", C.c_int32), ("doubleconv", C.c_int32),
        ("use_skip", C.c_int32), ("precision", C.c_int32),
    ]


class VitTap(C.Structure):
    """amx_vit_tap: one request of amx_vit_forward_taps (name, device buffer or None, its capacity; out: the producing launch)."""
    _fields_ = [("name", C.c_char_p), ("d_dst", C.c_void_p), ("bytes", C.c_size_t), ("route", C.c_char * 160)]


class VitCfg(C.Structure):
    _fields_ = [
        ("input_channels", C.c_int32), ("num_classes", C.c_int32), ("embed_dim", C.c_int32), ("depth", C.c_int32),
        ("heads", C.c_int32), ("num_register_tokens", C.c_int32), ("grid_d", C.c_int32), ("grid_h", C.c_int32),
        ("grid_w", C.c_int32), ("hidden", C.c_int32), ("dec1", C.c_int32), ("dec2", C.c_int32), ("qk_norm", C.c_int32),
        ("scale_attn_inner", C.c_int32), ("layer_scale", C.c_int32), ("in_eps", C.c_float), ("out_norm", C.c_int32),
        ("decoder_split", C.c_int32), ("stem_split", C.c_int32),
    ]


_P = C.c_void_p
_I = C.c_int


class PackReq(C.Structure):
    _fields_ = [("d_weight", C.c_void_p), ("d_wpk", C.c_void_p), ("weight_mode", C.c_int32), ("cin_real", C.c_int32),
                ("cin_pad", C.c_int32), ("cout_real", C.c_int32), ("cout", C.c_int32), ("w", C.c_int32)]


WEIGHTS_PREPACKED = 16


class LaunchRecord(C.Structure):
    _fields_ = [("kernel", C.c_char * 64), ("module_idx", C.c_int32), ("cin", C.c_int32), ("cout", C.c_int32),
                ("n", C.c_int32), ("d", C.c_int32), ("h", C.c_int32), ("w", C.c_int32), ("ms", C.c_float),
                ("flops", C.c_double), ("bytes", C.c_double)]


SYMBOLS = {
    "amx_version": (_I, []),
    "amx_debug_fill_lds": (_I, [C.c_uint, _P]),
    "amx_last_error": (C.c_char_p, []),
    "amx_unet_create": (_I, [C.POINTER(_P), C.POINTER(UnetCfg)]),
    "amx_unet_destroy": (None, [_P]),
    "amx_unet_num_modules": (_I, [_P]),
    "amx_unet_num_convs": (_I, [_P]),
    "amx_unet_conv_info": (_I, [_P, _I, C.POINTER(_I), C.POINTER(_I), C.POINTER(_I), C.POINTER(_I)]),
    "amx_unet_load_conv": (_I, [_P, _I, _P, _P, _P, _P, _P, _P, _P]),
    "amx_unet_workspace_bytes": (C.c_size_t, [_P, _I, _I, _I, _I]),
    "amx_unet_forward": (_I, [_P, _P, _P, _I, _I, _I, _I, _P, C.c_size_t, _P]),
    "amx_unet_forward_profiled": (_I, [_P, _P, _P, _I, _I, _I, _I, _P, C.c_size_t, _P, C.POINTER(LaunchRecord), _I,
                                        C.POINTER(_I)]),
    "amx_unet_module_info": (_I, [_P, _I, C.POINTER(_I), C.POINTER(_I)]),
    "amx_unet_numerics_status": (_I, [_P, _I, _P]),
    "amx_unet_forward_taps": (_I, [_P, _P, _P, _I, _I, _I, _I, _P, C.c_size_t, C.POINTER(_I), _I, C.POINTER(_P), _I, _P]),
    "amx_unet_forward_window": (_I, [_P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _I, _P, _P, _P, C.c_size_t, _P]),
    "amx_unet_forward_windows": (_I, [_P, _P, _I, _I, _I, _I, C.POINTER(C.c_int), _I, _I, _I, _P, _P, _P, C.c_size_t, _P]),
    "amx_unet_forward_windows_pipelined": (_I, [_P, _P, _I, _I, _I, _I, C.POINTER(C.c_int), _I, _I, _I, _P, _P, _P, C.c_size_t, _I, _P]),
    "amx_sw_normalize": (_I, [_P, _P, _I, C.c_longlong, _P]),
    "amx_sw_count": (_I, [_P, _I, _I, _I, _I, _I, _I, _I, _I, _I, _P, _P]),
    "amx_sw_plan": (_I, [_I, _I, _I, _I, _I, _I, C.c_double, C.POINTER(C.c_int), _I]),
    "amx_sw_importance_map": (_I, [_P, _I, _I, _I, _I, C.c_double, _P]),
    "amx_sw_count_all": (_I, [_P, _I, _I, _I, _I, _I, _I, C.c_double, _P, _P]),
    "amx_sw_finish": (_I, [_I, _P, _P, _I, C.c_longlong, _P, _P, _I, _P, _P]),
    "amx_sliding_window_workspace_bytes": (C.c_size_t, [_P, _I, _I, _I, _I]),
    "amx_sliding_window": (_I, [_P, _P, _I, _I, _I, _I, _I, _I, C.c_double, _I, C.c_double, _I, _I, _P, _P, _I, _P, _P, _P, _P,
                                C.c_size_t, _P]),
    "amx_conv3d_packed_bytes": (C.c_size_t, [_I, _I]),
    "amx_conv3d_k3_reflect": (_I, [_P, _I, _P, _I, _P, _P, _P, _I, _I, _I, _I, _I, _I, C.c_float, _I, _P, _P, _P, _P]),
    "amx_conv3d_k3_reflect_probe": (_I, [_P, _I, _P, _I, _P, _P, _P, _I, _I, _I, _I, _I, _I, C.c_float, _I, _P, _P, _P, _P, _P, _P, _P, _P]),
    "amx_conv3d_dgrad_interior_supported": (_I, [_I, _I, _I, _I, _I, _I]),
    "amx_conv3d_dgrad_interior": (_I, [_P, _I, _P, _I, _I, _I, _I, _I, _I, _I, _I, _I, _P, _P, _P]),
    "amx_conv3d_dgrad_shell_scratch_bytes": (C.c_size_t, []),
    "amx_conv3d_dgrad_fold_shell": (_I, [_P, _I, _P, _I, _I, _P, _I, _I, _I, _I, _I, _I, _P, _P]),
    "amx_conv3d_pack_batch": (_I, [C.POINTER(PackReq), _I, _I, _P]),
    "amx_conv3d_scratch_bytes": (C.c_size_t, [_I, _I, _I, _I, _I, _I, _I, _I]),
    "amx_conv3d_k3_reflect_ws": (_I, [_P, _I, _P, _I, _P, _P, _P, _I, _I, _I, _I, _I, _I, C.c_float, _I, _P, _P, _P, _P, C.c_size_t, _P]),
    "amx_conv3d_upcat_merged_packed_bytes": (C.c_size_t, [_I, _I, _I]),
    "amx_conv3d_upcat_merged": (_I, [_P, _I, _P, _I, _P, _P, _P, _I, _I, _I, _I, _I, _I, C.c_float, _I, _P, _P, _P, _P]),
    "amx_conv3d_k3_reflect_ex": (_I, [_P, _I, _P, _I, _P, _I, _I, _I, _P, _P, _I, _I, _I, _I, _I, _I, C.c_float, _I, _P, _P, _P, _P]),
    "amx_pool2": (_I, [_P, _P, _I, _I, _I, _I, _I, _I, _I, _P]),
    "amx_instance_norm_scratch_bytes": (C.c_size_t, [_I, _I]),
    "amx_instance_norm": (_I, [_P, _P, _P, C.c_float, _I, C.c_longlong, _I, _I, C.c_float, _P, _I, _P]),
    "amx_upsample2_trilinear": (_I, [_P, _P, _I, _I, _I, _I, _I, _I, _P]),
    "amx_upsample2_trilinear_backward": (_I, [_P, _P, _I, _I, _I, _I, _I, _I, _P]),
    "amx_conv3d_zx_probe_workspace_bytes": (C.c_size_t, []),
    "amx_conv3d_zx_probe_stats_slots": (_I, [_I, _I]),
    "amx_conv3d_zx_probe": (_I, [_P, _P, _P, _P, _P, _I, C.c_float, _I, _I, _I, _I, _I, _P, C.c_size_t, _P, _P, _P, _P, _P, _P]),
    "amx_instance_norm_probe_scratch_bytes": (C.c_size_t, [_I, _I, _I]),
    "amx_instance_norm_probe": (_I, [_P, _P, _P, C.c_float, _I, C.c_longlong, _I, _I, _I, C.c_float, _P, C.c_size_t, _I, _I, _P, _I, _I, _P, _P,
                                     _P]),
    "amx_instance_norm_apply_pool_probe": (_I, [_P, _P, _P, _I, _I, _I, _I, _I, _I, C.c_float, _I, _I, _I, _I, _P, _P]),
    "amx_upsample2_trilinear_pending": (_I, [_P, _P, _I, _I, _I, _I, _I, _I, _I, _P, _I, C.c_float, _P, _P]),
    "amx_upcat_split_backward": (_I, [_P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _P]),
    "amx_upcat_split_backward_framed": (_I, [_P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _P]),
    "amx_export_ncdhw": (_I, [_P, _I, _I, _I, _I, _I, _P, _I, _P]),
    "amx_import_ncdhw": (_I, [_P, _P, _I, _I, _I, _I, _I, C.c_longlong, C.c_longlong, C.c_longlong, C.c_longlong, _I, _I, _P]),
    "amx_train_scratch_bytes": (C.c_size_t, [_I]),
    "amx_bn_train_forward": (_I, [_P, _P, _P, _P, C.c_float, _I, C.c_longlong, _I, _I, C.c_float, _P, _P, _P, _P, _P,
                                  C.c_float, _I, _P]),
    "amx_bn_act_backward": (_I, [_P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, C.c_float, _P, _I, _P]),
    "amx_bn_act_backward_recompute": (_I, [_P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, C.c_float, _P, _I, _P]),
    "amx_pad_fold": (_I, [_P, _P, _I, _I, _I, _I, _I, _I, _I, _P]),
    "amx_adamw_step": (_I, [_P, _I, C.c_double, C.c_double, C.c_double, C.c_double, C.c_double, _I, _P]),
    "amx_adamw_step_dev": (_I, [_P, _I, _P, _I, _P]),
    "amx_adamw_step_clip_dev": (_I, [_P, _I, _P, _I, _P, C.c_double, _P]),
    "amx_grad_norms_scratch_bytes": (C.c_size_t, [_P, _I, _I]),
    "amx_grad_norms": (_I, [_P, _I, _I, _P, _P, C.c_size_t, _P]),
    "amx_pool2_max_backward": (_I, [_P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _P]),
    "amx_conv3d_wgrad_scratch_bytes": (C.c_size_t, [_I, _I, _I, _I, _I, _I]),
    "amx_conv3d_wgrad": (_I, [_P, C.c_longlong, C.c_longlong, C.c_longlong, C.c_longlong, _P, _I, _P, _I, _I, _I, _I, _I, _I,
                              _I, _P, _I, _P, C.c_size_t, _I, _P]),
    "amx_attention_scratch_bytes": (C.c_size_t, [_I, _I, _I, _I]),
    "amx_attention_qknorm_rope": (_I, [_P, _P, _P, _P, _P, _P, _P, C.c_float, _P, _I, _I, _I, _I, _I, _P, _P, C.c_size_t, _P]),
    "amx_attention_prepared": (_I, [_P, C.c_size_t, _I, _I, _I, _I, _P, _P]),
    "amx_attention_train_scratch_bytes": (C.c_size_t, [_I, _I, _I, _I]),
    "amx_attention_qknorm_rope_train": (_I, [_P, _P, _P, _P, _P, _P, _P, C.c_float, _P, _I, _I, _I, _I, _I, _P, _P, _P, C.c_size_t, _P]),
    "amx_attention_backward": (_I, [_P, _P, _P, _P, _P, _P, _P, C.c_float, _P, _I, _I, _I, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P,
                                    _P, C.c_size_t, _P]),
    "amx_linear_train_scratch_bytes": (C.c_size_t, [C.c_longlong, _I, _I]),
    "amx_linear_forward": (_I, [_P, _P, _P, C.c_longlong, _I, _I, _P, _P, C.c_size_t, _P]),
    "amx_linear_backward": (_I, [_P, _P, _P, C.c_longlong, _I, _I, _P, _P, _P, _P, C.c_size_t, _P]),
    "amx_layernorm_train_scratch_bytes": (C.c_size_t, [C.c_longlong, _I]),
    "amx_layernorm_train_forward": (_I, [_P, _P, _P, _P, C.c_float, C.c_longlong, _I, _P, _P, _P, _P]),
    "amx_layernorm_backward": (_I, [_P, _P, _P, _P, _P, _P, C.c_longlong, _I, _P, _P, _P, _P, _P, C.c_size_t, _P]),
    "amx_tokenizer_train_saved_bytes": (C.c_size_t, [_I, _I, _I, _I]),
    "amx_tokenizer_train_scratch_bytes": (C.c_size_t, [_I, _I, _I, _I]),
    "amx_tokenizer_train_forward": (_I, [_P, C.POINTER(_P), _I, _I, _I, _I, C.c_float, _P, _P, C.c_size_t, _P, C.c_size_t, _P]),
    "amx_tokenizer_backward": (_I, [_P, _P, C.POINTER(_P), _P, _I, _I, _I, _I, C.c_float, C.POINTER(_P), _P, C.c_size_t, _P]),
    "amx_tokenizer_train_export": (_I, [_P, _I, _I, _I, _I, _I, _P]),
    "amx_tokenizer_train_route": (_I, [_I, _I, _I, _I, C.c_char_p, C.c_size_t]),
    "amx_vit_decode_rows_scratch_bytes": (C.c_size_t, [_I, _I, _I, _I, _I, _I]),
    "amx_vit_decode_rows_forward": (_I, [_P, _P, C.POINTER(_P), _I, _I, _I, _I, _I, _I, _I, _I, _I, C.c_float, _I, C.c_float, _P, _P,
                                        C.c_size_t, _P]),
    "amx_vit_decode_rows_backward": (_I, [_P, _P, C.POINTER(_P), _I, _I, _I, _I, _I, _I, _I, _I, _I, C.c_float, _I, C.c_float, _P, _P,
                                         C.POINTER(_P), _P, C.c_size_t, _P]),
    "amx_vit_decoder_train_saved_bytes": (C.c_size_t, [_I, _I, _I, _I, _I, _I, _I, _I]),
    "amx_vit_decoder_train_scratch_bytes": (C.c_size_t, [_I, _I, _I, _I, _I, _I, _I, _I]),
    "amx_vit_decoder_train_forward": (_I, [_P, C.POINTER(_P), _I, _I, _I, _I, _I, _I, _I, _I, C.c_float, _I, C.c_float, _P, _P, C.c_size_t, _P,
                                          C.c_size_t, _P]),
    "amx_vit_decoder_backward": (_I, [_P, _P, _P, C.POINTER(_P), _P, C.c_size_t, _I, _I, _I, _I, _I, _I, _I, _I, C.c_float, _I, C.c_float, _P,
                                     C.POINTER(_P), _P, C.c_size_t, _P]),
    "amx_vit_create": (_I, [C.POINTER(_P), C.POINTER(VitCfg)]),
    "amx_vit_destroy": (None, [_P]),
    "amx_vit_num_params": (_I, [_P]),
    "amx_vit_param_name": (C.c_char_p, [_P, _I]),
    "amx_vit_load": (_I, [_P, C.POINTER(_P), _I, _P, _P]),
    "amx_vit_workspace_bytes": (C.c_size_t, [_P, _I]),
    "amx_vit_forward": (_I, [_P, _P, _P, _I, _P, C.c_size_t, _I, _P]),
    "amx_vit_tap_bytes": (C.c_size_t, [_P, _I, C.c_char_p]),
    "amx_vit_forward_taps": (_I, [_P, _P, _P, _I, _P, C.c_size_t, _I, C.POINTER(VitTap), _I, _P]),
    "amx_vit_windows_workspace_bytes": (C.c_size_t, [_P, _I]),
    "amx_vit_forward_windows": (_I, [_P, _P, _I, _I, _I, _I, C.POINTER(C.c_int), _P, _P, _P, C.c_size_t, _P]),
    "amx_vit_sliding_window_workspace_bytes": (C.c_size_t, [_P, _I]),
    "amx_vit_sliding_window": (_I, [_P, _P, _I, _I, _I, C.c_double, _I, C.c_double, _I, _I, _P, _P, _I, _P, _P, _P, _P, C.c_size_t, _P]),
    "amx_linear": (_I, [_P, _P, _P, _I, _I, _I, _I, _P, _P]),
    "amx_supcon_scratch_bytes": (C.c_size_t, [_I, _I]),
    "amx_supcon_loss": (_I, [_P, _P, _I, _I, C.c_float, _I, _I, _I, _P, _P, _P, C.c_size_t, _P]),
    "amx_mlp_head_forward": (_I, [_P, _I, _I, _I, _I, _P, _P, _P, _P, _P, C.c_float, C.c_float, _I, C.c_float, _P, _P, _P, _P, _P]),
    "amx_mlp_head_scratch_bytes": (C.c_size_t, [_I, _I, _I]),
    "amx_mlp_head_backward": (_I, [_P, _P, _I, _I, _I, _I, _P, _P, _I, C.c_float, _P, _P, _P, _P, _P, _P, _P, _P, _P, C.c_size_t, _P]),
    "amx_mlp_heads_forward": (_I, [_I, _P, _I, _P, _I, _I, _P, _P, _P, _P, _P, C.c_float, C.c_float, _I, C.c_float, _P, _P, _P, _P, _P]),
    "amx_mlp_heads_backward": (_I, [_I, _P, _P, _I, _P, _I, _I, _P, _P, _I, C.c_float, _P, _P, _P, _P, _P, _P, _P, _P, _P, C.c_size_t, _P]),
    "amx_supcon_loss_batch": (_I, [_I, _P, _P, _I, _I, C.c_float, _I, _I, _I, _P, _P, _P, C.c_size_t, _P]),
    "amx_gather_labels_batch": (_I, [_P, _I, _I, _I, _I, _P, _I, _P, _I, _P, _P]),
    "amx_conv3d_backward_sampled_scratch_bytes": (C.c_size_t, [_I]),
    "amx_conv3d_backward_sampled": (_I, [_P, _P, _P, _I, _P, _I, _I, _I, _I, _I, _I, _I, _P, _P, _I, _P, C.c_size_t, _I, _P]),
    "amx_gather_rows": (_I, [_P, _I, C.c_longlong, C.c_longlong, C.c_longlong, C.c_longlong, C.c_longlong, _P, _I, _I, _I, _P, _P]),
    "amx_scatter_rows": (_I, [_P, _P, _P, _I, C.c_longlong, C.c_longlong, C.c_longlong, C.c_longlong, _I, _I, _I, _I, _P]),
    "amx_sample_coords": (_I, [_P, _I, _I, _I, _I, _I, _P, _P]),
    "amx_sample_perm": (_I, [_P, _I, _I, _I, _I, _P, _P]),
    "amx_import_input": (_I, [_P, _P, _I, _I, _I, _I, _I, _I, _P]),
    "amx_gather_labels": (_I, [_P, _I, _I, _I, _P, _I, _I, _I, _I, _I, _P, _P]),
    "amx_mindssc_scratch_bytes": (C.c_size_t, [_I, _I, _I]),
    "amx_mindssc": (_I, [_P, _I, _I, _I, _I, _I, _P, _P, C.c_size_t, _P]),
    "amx_avg_pool3d_cat": (_I, [_P, _I, C.c_float, _P, _I, C.c_float, _I, _I, _I, _I, _P, _P]),
    "amx_box_filter3d": (_I, [_P, _P, _I, _I, _I, _I, _I, _P]),
    "amx_correlate_scratch_bytes": (C.c_size_t, [_I, _I, _I, _I]),
    "amx_correlate_ssd": (_I, [_P, _P, _I, _I, _I, _I, _I, _P, _P, _P, C.c_size_t, _P]),
    "amx_coupled_convex_scratch_bytes": (C.c_size_t, [_I, _I, _I]),
    "amx_coupled_convex": (_I, [_P, _P, _I, _I, _I, _I, _P, _P, C.c_size_t, _P]),
    "amx_coupled_convex_step_scratch_bytes": (C.c_size_t, [_I, _I, _I]),
    "amx_coupled_convex_step": (_I, [_P, _P, _I, _I, _I, _I, _I, _P, _P, _P, C.c_size_t, _P]),
    "amx_inverse_consistency_scratch_bytes": (C.c_size_t, [_I, _I, _I]),
    "amx_inverse_consistency": (_I, [_P, _P, _I, _I, _I, _I, _P, _P, _P, C.c_size_t, _P]),
    "amx_resize_trilinear3d": (_I, [_P, _I, _I, _I, _I, _P, _I, _I, _I, C.POINTER(C.c_float), _I, _P]),
    "amx_stage1_registration_scratch_bytes": (C.c_size_t, [_I, _I, _I, _I, _I]),
    "amx_stage1_registration": (_I, [_P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _I, _I, _P, _P, C.c_size_t, _P]),
    "amx_instance_opt_smooth3": (_I, [_P, _P, _I, _I, _I, _P]),
    "amx_instance_opt_scratch_bytes": (C.c_size_t, [_I, _I, _I, _I]),
    "amx_instance_opt_grad": (_I, [_P, _P, _P, _I, _I, _I, _I, C.c_float, _P, _P, _P, _P, C.c_size_t, _P]),
    "amx_instance_opt_adam_step": (_I, [_P, _P, _P, _P, C.c_longlong, C.c_double, _I, _P]),
    "amx_instance_opt": (_I, [_P, _P, _P, _I, _I, _I, _I, C.c_float, C.c_double, _I, _P, _P, C.c_size_t, _P]),
    "amx_run_instance_opt_scratch_bytes": (C.c_size_t, [_I, _I, _I, _I, _I, _I]),
    "amx_run_instance_opt": (_I, [_P, _P, _P, _I, _I, _I, _I, _I, C.c_float, _I, _I, C.c_double, _P, _P, C.c_size_t, _P]),
    "amx_warp3d": (_I, [_P, _I, _P, _I, _I, _I, _I, _P, _P]),
    "amx_seg_loss_scratch_bytes": (C.c_size_t, [_I, C.c_longlong, _I, _I]),
    "amx_seg_loss_forward": (_I, [_P, _I, _P, _P, _P, _I, _I, _I, C.c_longlong, _I, C.c_float, C.c_float, C.c_float, C.c_float, _P, _P,
                                  _P, _P, C.c_size_t, _P]),
    "amx_seg_loss_backward": (_I, [_P, _I, _P, _P, _P, _I, _I, _I, C.c_longlong, _I, C.c_float, C.c_float, C.c_float, C.c_float, _P, _P,
                                   _P, _P, _P, _P, C.c_size_t, _P]),
    "amx_seg_argmax": (_I, [_P, _I, _P, _P, _I, _I, C.c_longlong, _P, _P]),
    "amx_segaug_sample_bytes": (C.c_size_t, []),
    "amx_segaug_scratch_bytes": (C.c_size_t, [_I, C.c_longlong]),
    "amx_segaug_minmax": (_I, [_P, _I, C.c_longlong, _P, _P, C.c_size_t, _P]),
    "amx_segaug_minmax_finalize": (_I, [_P, C.c_size_t, _I, C.c_longlong, _P, _P]),
    "amx_segaug_pointwise": (_I, [_P, _P, _I, C.c_longlong, _P, _I, _P, _P, _P]),
    "amx_segaug_crop": (_I, [_I, _I, _I, _I, _P, _I, _P, _P, _P, _P, _P]),
    "amx_segaug_gaussian": (_I, [_P, _P, _P, _I, _I, _I, _I, _I, _P, _P, _P]),
    "amx_segaug_affine": (_I, [_P, _P, _I, _I, _I, _I, _P, _P, _I, _I, _I, _P, _P, _P, C.c_size_t, _P]),
    "amx_preaug_view_bytes": (C.c_size_t, []),
    "amx_preaug_spatial": (_I, [_P, _P, _I, _I, _I, _I, _P, _P, _P, _P, _P, _P]),
    "amx_preaug_blur": (_I, [_P, _P, _P, _I, _I, _I, _I, _P, _P, _P]),
    "amx_preaug_intensity": (_I, [_P, _P, _P, _I, _I, _I, _I, _P, _P, _P]),
    "amx_synth_view_bytes": (C.c_size_t, []),
    "amx_synth_scratch_bytes": (C.c_size_t, [_I, C.c_longlong]),
    "amx_synth_gmm_minmax": (_I, [_P, _P, _I, C.c_longlong, _P, _P, _P, C.c_size_t, _P]),
    "amx_synth_appearance": (_I, [_P, _P, C.POINTER(_P), C.POINTER(_I), _I, _P, _P, _I, _I, _I, _I, _P, _P, _P, C.c_size_t, _P]),
    "amx_synth_logk_mean": (_I, [_P, _I, C.c_longlong, _P, _P, C.c_size_t, _P]),
    "amx_synth_spike": (_I, [_P, _P, _I, _P, _I, _I, _I, _I, _P, _P, _P]),
    "amx_synth_lowres": (_I, [_P, _P, _I, _I, _I, _I, _P, _P, _P]),
    "amx_synth_clip_minmax": (_I, [_P, _I, C.c_longlong, _P, C.c_size_t, _P]),
    "amx_synth_finish": (_I, [_P, _P, _I, C.c_longlong, _P, _I, _P]),
    "amx_labels_template_bytes": (C.c_size_t, []),
    "amx_labels_ensemble_bytes": (C.c_size_t, []),
    "amx_labels_scratch_bytes": (C.c_size_t, [_I, C.c_longlong]),
    "amx_labels_compose": (_I, [_P, C.c_size_t, _P, _P, _I, _P, _P, _P, _I, _I, _I, _I, _P]),
    "amx_labels_median3": (_I, [_P, _P, _I, _I, _I, _I, _I, _P, _P, _P]),
    "amx_labels_sphere_mask": (_I, [C.POINTER(_P), _P, _I, _I, _P, _P, _P]),
    "amx_labels_apply_mask": (_I, [_P, _P, _P, _I, C.c_longlong, _P, _P, _P, C.c_size_t, _P]),
    "amx_labels_envelope": (_I, [_P, _P, _P, _I, _I, _I, _I, _P, _P, _P]),
    "amx_labels_merge_masks": (_I, [_P, _I, C.c_longlong, C.c_longlong, C.POINTER(_I), _P, _P, _P, _I, _P]),
    "amx_label_overlap": (_I, [_P, _I, _P, _I, C.c_longlong, _I, _P, _P, _P]),
    "amx_jacobian_det_scratch_bytes": (C.c_size_t, [_I, _I, _I]),
    "amx_jacobian_det": (_I, [_P, _I, _I, _I, _I, _P, _P, _P, C.c_size_t, _P]),
}

_lib = None


AMX_ERR_INVALID, AMX_ERR_SHAPE, AMX_ERR_NOT_LOADED, AMX_ERR_WORKSPACE, AMX_ERR_HIP, AMX_ERR_OVERFLOW = -1, -2, -3, -4, -5, -6


class AmxError(RuntimeError):
    """A non-zero status of the C ABI; ``code`` is the status (include/anatomix_amd.h amx_status)."""

    def __init__(self, *args):
        # (code, message) or just a message
        self.code = args[0] if args and isinstance(args[0], int) else None
        super().__init__(*(args[1:] if self.code is not None else args))


class AmxEnvelopeError(AmxError):
    """The configuration lies outside what an engine entry covers (AMX_ERR_INVALID / AMX_ERR_SHAPE at create time)."""


class AmxOverflowError(AmxError, FloatingPointError):
    """AMX_ERR_OVERFLOW: f16 / f16x2 storage met a value outside the f16 range (include/anatomix_amd.h)."""


def load():
    """dlopen the in-tree library and declare prototypes.  Raises if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise AmxError(
            f"{LIB_PATH} not found: build the HIP extension first (python -c 'import __graft_entry__ as g; "
            "g.build()' or make -C anatomix_amd/csrc).  There is no CPU fallback for the HIP path.")
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SYMBOLS.items():
        fn = getattr(lib, name)   # AttributeError if the .so lacks a declared symbol
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def check(status: int):
    if status != 0:
        cls = AmxOverflowError if status == AMX_ERR_OVERFLOW else AmxError
        raise cls(int(status), f"anatomix_amd error {status}: {load().amx_last_error().decode()}")


def check_envelope(status: int):
    """``check`` for the entries whose AMX_ERR_INVALID / AMX_ERR_SHAPE say that the call lies outside what they cover."""
    if status in (AMX_ERR_INVALID, AMX_ERR_SHAPE):
        raise AmxEnvelopeError(int(status), f"anatomix_amd error {status}: {load().amx_last_error().decode()}")
    check(status)


def ptr(t):
    """Device pointer of a torch tensor (or None)."""
    return None if t is None else C.c_void_p(t.data_ptr())


# torch is imported inside the helpers below: importing this module stays torch-free
def stream(dev):
    """The current stream of ``dev`` as the ``void* stream`` argument of the C ABI."""
    import torch
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def scratch(nbytes: int, dev):
    """An uninitialised device buffer for a ``*_scratch_bytes`` answer (one byte when that is 0, so that it has a pointer)."""
    import torch
    return torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev)


def f32c(t):
    """``t`` as a contiguous float32 tensor (itself when it already is one)."""
    import torch
    return t if (t.dtype == torch.float32 and t.is_contiguous()) else t.float().contiguous()
