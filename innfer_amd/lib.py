"""ctypes binding of libinnfer_amd.so (the C ABI declared in include/innfer_amd.h).

The library is the product: there is NO fallback.  If the shared object is
missing the import of this module raises; if a call fails the Python side
raises the exception class the reference would have raised for the same
condition (ValueError / NotImplementedError / RuntimeError).
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
_DEFAULT_LIB = os.path.join(_HERE, "lib", "libinnfer_amd.so")
LIB_PATH = os.environ.get("INNFER_LIB") or _DEFAULT_LIB

F16, F32, U8 = 0, 1, 2
OK, ERR_INVALID, ERR_HIP, ERR_UNSUPPORTED, ERR_NOMEM, ERR_WORKSPACE = 0, -1, -2, -3, -4, -5


class InnferError(RuntimeError):
    pass


def _load():
    if not os.path.isfile(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} not found: build it with `make` (or `python -c 'import __graft_entry__ as g; g.build()'`). "
            "innfer_amd has no CPU or PyTorch fallback for its hot path.")
    # PyTorch-ROCm wheels bundle their own libamdhip64.so.7; it must be the ONE HIP runtime of the
    # process (device pointers, streams and events are shared with torch), so torch is imported
    # first and libinnfer_amd.so's NEEDED libamdhip64.so.7 binds to the copy already loaded.
    import torch  # noqa: F401
    return C.CDLL(LIB_PATH)


_lib = _load()


class ConvArgs(C.Structure):
    _fields_ = [
        ("d_in", C.c_void_p), ("in_group_stride", C.c_int64), ("C", C.c_int),
        ("d_packed", C.c_void_p), ("d_bias", C.c_void_p),
        ("d_out", C.c_void_p), ("out_group_stride", C.c_int64), ("out_ch_off", C.c_int), ("K", C.c_int),
        ("N", C.c_int), ("H", C.c_int), ("W", C.c_int),
        ("act", C.c_int), ("upsample2x", C.c_int),
        ("d_res1", C.c_void_p), ("res1_group_stride", C.c_int64), ("res1_scale", C.c_float),
        ("d_res2", C.c_void_p), ("res2_group_stride", C.c_int64), ("res2_scale", C.c_float),
        ("row_begin", C.c_int), ("row_end", C.c_int),
        ("reflect_pad", C.c_int), ("dilation", C.c_int), ("dilation_groups", C.c_int), ("pixel_shuffle2", C.c_int),
        ("stride2_k4", C.c_int), ("transposed2x", C.c_int), ("column7", C.c_int),
        ("split", C.c_int), ("in_lo", C.c_int64), ("out_lo", C.c_int64), ("res1_lo", C.c_int64), ("res2_lo", C.c_int64),
        ("reserved0", C.c_int), ("res1_from_input", C.c_int), ("plane_rows", C.c_int),
        ("d_stats_part", C.c_void_p), ("stats_part_floats", C.c_int64),
        ("conv1x1", C.c_int), ("prefix_lrelu", C.c_int), ("d_gate_packed", C.c_void_p), ("d_gate_bias", C.c_void_p),
        ("in_relu", C.c_int), ("conv7x7", C.c_int), ("out_planar", C.c_int), ("out_denorm", C.c_int), ("out_round16", C.c_int),
        ("planar_phases", C.c_int), ("outm", C.c_int),
    ]


class F32ConvArgs(C.Structure):
    _fields_ = [
        ("d_in", C.c_void_p), ("in_nstride", C.c_int64), ("in_cstride", C.c_int64), ("C", C.c_int), ("Hin", C.c_int), ("Win", C.c_int),
        ("d_packed", C.c_void_p), ("d_bias", C.c_void_p), ("K", C.c_int),
        ("d_out", C.c_void_p), ("out_nstride", C.c_int64), ("out_cstride", C.c_int64), ("out_pstride", C.c_int64), ("Wout", C.c_int),
        ("Ho", C.c_int), ("Wo", C.c_int),
        ("osy", C.c_int), ("osx", C.c_int), ("ooy", C.c_int), ("oox", C.c_int),
        ("isy", C.c_int), ("isx", C.c_int),
        ("ntap", C.c_int), ("dy", C.c_int * 49), ("dx", C.c_int * 49),
        ("pad_mode", C.c_int), ("up", C.c_int), ("in_act", C.c_int), ("act", C.c_int),
        ("oscale", C.c_float),
        ("d_res", C.c_void_p), ("res_nstride", C.c_int64), ("res_cstride", C.c_int64),
        ("d_mul", C.c_void_p), ("mul_nstride", C.c_int64), ("mul_cstride", C.c_int64),
        ("N", C.c_int),
        ("phase_k", C.c_int),
        ("form", C.c_int),
    ]


class GatherGemmArgs(C.Structure):
    _fields_ = [
        ("d_in", C.c_void_p), ("in_group_stride", C.c_int64), ("cin_pad", C.c_int),
        ("d_packed", C.c_void_p), ("cout_pad", C.c_int),
        ("d_raw", C.c_void_p), ("raw_stride", C.c_int), ("cout_store", C.c_int),
        ("N", C.c_int), ("Hin", C.c_int), ("Win", C.c_int), ("Ho", C.c_int), ("Wo", C.c_int), ("stride", C.c_int),
        ("ntaps", C.c_int), ("dy", C.c_int * 49), ("dx", C.c_int * 49),
        ("Hfull", C.c_int), ("Wfull", C.c_int), ("os", C.c_int), ("ooy", C.c_int), ("oox", C.c_int), ("up", C.c_int), ("reflect", C.c_int),
        ("ngroup", C.c_int), ("g_wbytes", C.c_int64), ("g_outoff", C.c_int64), ("g_tapmul", C.c_int), ("g_phase", C.c_int),
        ("d_scratch", C.c_void_p), ("scratch_bytes", C.c_int64),
        ("keep_partials", C.c_int),
    ]


# name -> (restype, argtypes); every symbol declared in include/innfer_amd.h
SIGNATURES = {
    "innfer_version": (C.c_int, []),
    "innfer_last_error": (C.c_char_p, []),
    "innfer_rrdbnet_create": (C.c_int, [C.POINTER(C.c_void_p)] + [C.c_int] * 7),
    "innfer_srresnet_create": (C.c_int, [C.POINTER(C.c_void_p)] + [C.c_int] * 5),
    "innfer_net_destroy": (None, [C.c_void_p]),
    "innfer_net_num_convs": (C.c_int, [C.c_void_p]),
    "innfer_net_conv_info": (C.c_int, [C.c_void_p, C.c_int, C.c_char_p, C.c_size_t,
                                       C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "innfer_net_set_conv": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "innfer_net_scale": (C.c_int, [C.c_void_p]),
    "innfer_net_workspace_bytes": (C.c_size_t, [C.c_void_p, C.c_int, C.c_int, C.c_int]),
    "innfer_net_forward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int,
                                     C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p]),
    "innfer_net_forward_timed": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int,
                                           C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p,
                                           C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_double), C.POINTER(C.c_double),
                                           C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "innfer_rrdbnet_create_ex": (C.c_int, [C.POINTER(C.c_void_p)] + [C.c_int] * 10),
    "innfer_rrdbnet_create_ex2": (C.c_int, [C.POINTER(C.c_void_p)] + [C.c_int] * 11),
    "innfer_first_conv_unshuffle": (C.c_int, [C.c_void_p] + [C.c_int] * 8 + [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p]),
    "innfer_first_conv": (C.c_int, [C.c_void_p] + [C.c_int] * 7 + [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p] + [C.c_void_p, C.c_int64, C.c_int64] * 2 + [C.c_void_p]),
    "innfer_slab_upsample_nearest": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64] + [C.c_int] * 5 + [C.c_int64, C.c_void_p]),
    "innfer_slab_pixel_shuffle": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64] + [C.c_int] * 5 + [C.c_int64, C.c_void_p]),
    "innfer_slab_input_map": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "innfer_srresnet_create_ex": (C.c_int, [C.POINTER(C.c_void_p)] + [C.c_int] * 6 + [C.c_float, C.c_int]),
    "innfer_net_set_conv_input_map": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int]),
    "innfer_net_set_outm": (C.c_int, [C.c_void_p, C.c_int]),
    "innfer_timer_start": (C.c_int, []),
    "innfer_timer_stop": (C.c_int, [C.c_void_p, C.c_int, C.c_char_p, C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_int)]),
    "innfer_net_set_precision": (C.c_int, [C.c_void_p, C.c_int]),
    "innfer_pack_conv3x3_split": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "innfer_nchw_to_slab_split": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64] + [C.c_int] * 5 + [C.c_void_p]),
    "innfer_slab_split_to_nchw": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_int, C.c_void_p] + [C.c_int] * 4 + [C.c_void_p]),
    "innfer_net_set_band_rows": (C.c_int, [C.c_void_p, C.c_int]),
    "innfer_net_set_fused_tail": (C.c_int, [C.c_void_p, C.c_int]),
    "innfer_net_set_hr_chain": (C.c_int, [C.c_void_p, C.c_int]),
    "innfer_net_set_residual_lds": (C.c_int, [C.c_void_p, C.c_int]),
    "innfer_net_set_consumer_grid": (C.c_int, [C.c_void_p, C.c_int]),
    "innfer_net_set_upconv_phases": (C.c_int, [C.c_void_p, C.c_int]),
    "innfer_net_set_final_act": (C.c_int, [C.c_void_p, C.c_int]),
    "innfer_net_flops": (C.c_double, [C.c_void_p, C.c_int, C.c_int, C.c_int]),
    "innfer_unet_create": (C.c_int, [C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_int, C.c_int]),
    "innfer_unet_create_ex": (C.c_int, [C.POINTER(C.c_void_p)] + [C.c_int] * 6),
    "innfer_unet_destroy": (None, [C.c_void_p]),
    "innfer_unet_num_params": (C.c_int, [C.c_void_p]),
    "innfer_unet_param_info": (C.c_int, [C.c_void_p, C.c_int, C.c_char_p, C.c_size_t, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "innfer_unet_set_param": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p]),
    "innfer_unet_set_eval": (C.c_int, [C.c_void_p, C.c_int]),
    "innfer_unet_set_precision": (C.c_int, [C.c_void_p, C.c_int]),
    "innfer_unet_workspace_bytes": (C.c_size_t, [C.c_void_p, C.c_int, C.c_int, C.c_int]),
    "innfer_unet_flops": (C.c_double, [C.c_void_p, C.c_int, C.c_int, C.c_int]),
    "innfer_unet_forward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int,
                                      C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p]),
    "innfer_pan_create": (C.c_int, [C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    "innfer_pan_create_ex": (C.c_int, [C.POINTER(C.c_void_p)] + [C.c_int] * 9),
    "innfer_pan_destroy": (None, [C.c_void_p]),
    "innfer_pan_num_params": (C.c_int, [C.c_void_p]),
    "innfer_pan_param_info": (C.c_int, [C.c_void_p, C.c_int, C.c_char_p, C.c_size_t, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "innfer_pan_set_param": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p]),
    "innfer_pan_set_fused_scpa": (C.c_int, [C.c_void_p, C.c_int]),
    "innfer_pan_set_precision": (C.c_int, [C.c_void_p, C.c_int]),
    "innfer_pan_workspace_bytes": (C.c_size_t, [C.c_void_p, C.c_int, C.c_int, C.c_int]),
    "innfer_pan_forward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int,
                                     C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p]),
    "innfer_ppon_create": (C.c_int, [C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float]),
    "innfer_ppon_destroy": (None, [C.c_void_p]),
    "innfer_ppon_num_params": (C.c_int, [C.c_void_p]),
    "innfer_ppon_param_info": (C.c_int, [C.c_void_p, C.c_int, C.c_char_p, C.c_size_t, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "innfer_ppon_set_precision": (C.c_int, [C.c_void_p, C.c_int]),
    "innfer_ppon_set_param": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p]),
    "innfer_ppon_workspace_bytes": (C.c_size_t, [C.c_void_p, C.c_int, C.c_int, C.c_int]),
    "innfer_ppon_forward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                      C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p]),
    "innfer_resnet_create": (C.c_int, [C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_int, C.c_int]),
    "innfer_resnet_create_ex": (C.c_int, [C.POINTER(C.c_void_p)] + [C.c_int] * 8),
    "innfer_resnet_set_eval": (C.c_int, [C.c_void_p, C.c_int]),
    "innfer_resnet_destroy": (None, [C.c_void_p]),
    "innfer_resnet_num_params": (C.c_int, [C.c_void_p]),
    "innfer_resnet_param_info": (C.c_int, [C.c_void_p, C.c_int, C.c_char_p, C.c_size_t, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "innfer_resnet_set_precision": (C.c_int, [C.c_void_p, C.c_int]),
    "innfer_resnet_set_param": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p]),
    "innfer_resnet_workspace_bytes": (C.c_size_t, [C.c_void_p, C.c_int, C.c_int, C.c_int]),
    "innfer_resnet_forward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int,
                                        C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p]),
    "innfer_wbc_create": (C.c_int, [C.POINTER(C.c_void_p), C.c_int, C.c_int]),
    "innfer_wbc_destroy": (None, [C.c_void_p]),
    "innfer_wbc_num_params": (C.c_int, [C.c_void_p]),
    "innfer_wbc_param_info": (C.c_int, [C.c_void_p, C.c_int, C.c_char_p, C.c_size_t, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "innfer_wbc_set_precision": (C.c_int, [C.c_void_p, C.c_int]),
    "innfer_wbc_set_param": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p]),
    "innfer_wbc_workspace_bytes": (C.c_size_t, [C.c_void_p, C.c_int, C.c_int, C.c_int]),
    "innfer_wbc_forward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int,
                                     C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p]),
    "innfer_guided_filter_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int, C.c_int]),
    "innfer_guided_filter": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_void_p,
                                       C.c_void_p, C.c_size_t, C.c_void_p]),
    "innfer_conv3x3_packed_bytes": (C.c_size_t, [C.c_int, C.c_int]),
    "innfer_pack_conv3x3": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "innfer_pack_conv3x3_rows": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "innfer_pack_conv3x3_shuffle2": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "innfer_pack_convt2x_rows": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "innfer_conv3x3_f16": (C.c_int, [C.POINTER(ConvArgs), C.c_void_p]),
    "innfer_conv3x3_f16_slope": (C.c_int, [C.POINTER(ConvArgs), C.c_void_p, C.c_void_p]),
    "innfer_conv3x3_f16_grid": (C.c_int, [C.POINTER(ConvArgs), C.c_int, C.c_void_p]),
    "innfer_shuffle_add": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int] + [C.c_int] * 5 + [C.c_void_p]),
    "innfer_compact_create": (C.c_int, [C.POINTER(C.c_void_p)] + [C.c_int] * 5),
    "innfer_span_create": (C.c_int, [C.POINTER(C.c_void_p)] + [C.c_int] * 5 + [C.c_float, C.c_void_p]),
    "innfer_first_conv_map": (C.c_int, [C.c_void_p] + [C.c_int] * 7 + [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    "innfer_net_set_conv_slope": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p]),
    "innfer_plksr_create": (C.c_int, [C.POINTER(C.c_void_p)] + [C.c_int] * 8),
    "innfer_net_set_group_norm": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "innfer_swinir_create": (C.c_int, [C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_int, C.c_void_p] + [C.c_int] * 6 + [C.c_void_p]),
    "innfer_net_set_layer_norm": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "innfer_net_set_attn_bias": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p]),
    "innfer_window_attention": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p] + [C.c_int] * 6 + [C.c_void_p]),
    "innfer_layer_norm": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int64, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_float, C.c_void_p]),
    "innfer_swin2sr_create": (C.c_int, [C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_int, C.c_void_p] + [C.c_int] * 6 + [C.c_void_p]),
    "innfer_net_set_attn_scale": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p]),
    "innfer_window_attention_cos": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p] + [C.c_int] * 6 + [C.c_void_p]),
    "innfer_layer_norm_add": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int64, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_float, C.c_void_p]),
    "innfer_hat_create": (C.c_int, [C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_int, C.c_void_p] + [C.c_int] * 6 + [C.c_void_p]),
    "innfer_net_set_chan_attn": (C.c_int, [C.c_void_p, C.c_int] + [C.c_void_p] * 4),
    "innfer_net_set_conv_scale": (C.c_int, [C.c_void_p, C.c_float]),
    "innfer_window_attention16": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p] + [C.c_int] * 7 + [C.c_void_p]),
    "innfer_chan_attn_work_bytes": (C.c_size_t, [C.c_int, C.c_int64, C.c_int]),
    "innfer_chan_attn_excite": (C.c_int, [C.c_void_p, C.c_int64, C.c_int, C.c_int64, C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 7 + [C.c_size_t, C.c_void_p]),
    "innfer_chan_attn_scale_add": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_float, C.c_int, C.c_int64, C.c_int, C.c_void_p]),
    # (123, additive) the kernels of a DAT block as single launches
    "innfer_window_attention_rect": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p] + [C.c_int] * 8 + [C.c_void_p]),
    "innfer_channel_attention_work_bytes": (C.c_size_t, [C.c_int, C.c_int64, C.c_int]),
    "innfer_channel_attention_scores": (C.c_int, [C.c_void_p, C.c_int64, C.c_int, C.c_int64, C.c_int, C.c_int] + [C.c_void_p] * 4 + [C.c_size_t, C.c_void_p]),
    "innfer_channel_attention_apply": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int, C.c_int64, C.c_int, C.c_int, C.c_void_p]),
    "innfer_dwconv3x3": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64] + [C.c_int] * 5 + [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "innfer_chan_attn_excite_gelu": (C.c_int, [C.c_void_p, C.c_int64, C.c_int, C.c_int64, C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 7 + [C.c_size_t, C.c_void_p]),
    "innfer_aim_mix": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int, C.c_int64, C.c_int, C.c_int, C.c_int,
                                 C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_void_p]),
    "innfer_layer_norm_wide": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int64, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_float, C.c_void_p]),
    # (124, additive) DRCT
    "innfer_drct_create": (C.c_int, [C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "innfer_window_attention16_wide": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p] + [C.c_int] * 6 + [C.c_void_p]),
    "innfer_layer_norm_holed": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_float, C.c_void_p]),
    "innfer_dat_create": (C.c_int, [C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_int, C.c_void_p] + [C.c_int] * 8 + [C.c_void_p, C.c_void_p]),
    "innfer_dat_block_floats": (C.c_size_t, [C.c_void_p]),
    "innfer_net_set_dat_block": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t]),
    "innfer_plk_conv": (C.c_int, [C.c_void_p, C.c_void_p] + [C.c_int] * 4 + [C.c_void_p, C.c_void_p, C.c_void_p]),
    "innfer_group_norm_skip_work_bytes": (C.c_size_t, [C.c_int, C.c_int64]),
    "innfer_group_norm_skip": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int, C.c_int64, C.c_int, C.c_void_p, C.c_void_p,
                                         C.c_float, C.c_void_p, C.c_size_t, C.c_void_p]),
    "innfer_conv1x1_packed_bytes": (C.c_size_t, [C.c_int, C.c_int]),
    "innfer_pack_conv1x1": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "innfer_pack_conv1x1_split": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "innfer_pack_selfgate": (C.c_int, [C.c_void_p, C.c_void_p]),
    "innfer_conv7x7_packed_bytes": (C.c_size_t, [C.c_int, C.c_int]),
    "innfer_pack_conv7x7": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "innfer_pack_up2x_phases": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "innfer_filter2d": (C.c_int, [C.c_void_p, C.c_int, C.c_long, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "innfer_conv7x1_packed_bytes": (C.c_size_t, [C.c_int, C.c_int]),
    "innfer_pack_conv7x1": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "innfer_conv4x4s2_packed_bytes": (C.c_size_t, [C.c_int, C.c_int]),
    "innfer_pack_conv4x4s2": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "innfer_convt2x_packed_bytes": (C.c_size_t, [C.c_int, C.c_int]),
    "innfer_pack_convt2x": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "innfer_nchw_to_slab": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int64, C.c_int,
                                      C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "innfer_slab_to_nchw": (C.c_int, [C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_int,
                                      C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "innfer_chop_plan": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_double, C.POINTER(C.c_int),
                                   C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int),
                                   C.POINTER(C.c_int)]),
    "innfer_extract_tiles": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double,
                                       C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "innfer_blend_profile": (C.c_int, [C.c_int, C.c_double, C.c_int, C.POINTER(C.c_float)]),
    "innfer_recompose": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                   C.c_double, C.c_int, C.c_void_p, C.c_int, C.c_void_p]),
    "innfer_shard_tiles": (C.c_int, [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "innfer_comm_unique_id": (C.c_int, [C.c_void_p]),
    "innfer_comm_init": (C.c_int, [C.POINTER(C.c_void_p), C.c_void_p, C.c_int, C.c_int]),
    "innfer_comm_destroy": (None, [C.c_void_p]),
    "innfer_comm_rank": (C.c_int, [C.c_void_p]),
    "innfer_comm_size": (C.c_int, [C.c_void_p]),
    "innfer_gather_tiles": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]),
    "innfer_comm_broadcast": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]),
    "innfer_u8hwc_to_nchw": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p]),
    "innfer_srgb_to_linear": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "innfer_linear_to_srgb": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "innfer_color_fix_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    "innfer_color_fix": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                   C.c_void_p, C.c_size_t, C.c_void_p]),
    "innfer_color_fix_mode_workspace_bytes": (C.c_size_t, [C.c_int] * 6),
    "innfer_color_fix_mode": (C.c_int, [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                        C.c_void_p, C.c_size_t, C.c_void_p]),
    "innfer_nchw_to_u8hwc": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "innfer_linear_resize": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p]),
    "innfer_extract_tiles_u8": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p]),
    "innfer_recompose_u8": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "innfer_net_set_u8_io": (C.c_int, [C.c_void_p, C.c_int, C.c_int]),
    "innfer_guided_filter_ex": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float,
                                          C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "innfer_inthwc_to_nchw": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_void_p, C.c_int, C.c_void_p]),
    "innfer_nchw_to_inthwc": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "innfer_channel_minmax": (C.c_int, [C.c_void_p] + [C.c_int] * 5 + [C.c_void_p, C.c_void_p]),
    "innfer_extract_tiles_u8_fit": (C.c_int, [C.c_void_p] + [C.c_int] * 5 + [C.c_double] + [C.c_int] * 3 + [C.c_void_p, C.c_int, C.c_void_p]),
    "innfer_recompose_u8_fit": (C.c_int, [C.c_void_p] + [C.c_int] * 5 + [C.c_double] + [C.c_int] * 6 + [C.c_void_p, C.c_void_p]),
    "innfer_inthwc_to_nchw_fit": (C.c_int, [C.c_void_p] + [C.c_int] * 5 + [C.c_float, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "innfer_nchw_to_inthwc_fit": (C.c_int, [C.c_void_p, C.c_void_p] + [C.c_int] * 7 + [C.c_void_p, C.c_void_p]),
    "innfer_border_index": (C.c_int, [C.c_int, C.c_int, C.c_int]),
    "innfer_pad_inthwc": (C.c_int, [C.c_void_p] + [C.c_int] * 6 + [C.c_void_p, C.c_void_p]),
    "innfer_extract_tiles_u8_seamless": (C.c_int, [C.c_void_p] + [C.c_int] * 5 + [C.c_double] + [C.c_int] * 4 + [C.c_void_p, C.c_int, C.c_void_p]),
    "innfer_extract_tiles_u8_fit_seamless": (C.c_int, [C.c_void_p] + [C.c_int] * 5 + [C.c_double] + [C.c_int] * 5 + [C.c_void_p, C.c_int, C.c_void_p]),
    "innfer_recompose_u8_seamless": (C.c_int, [C.c_void_p] + [C.c_int] * 6 + [C.c_double] + [C.c_int] * 4 + [C.c_void_p, C.c_void_p]),
    "innfer_recompose_u8_fit_seamless": (C.c_int, [C.c_void_p] + [C.c_int] * 5 + [C.c_double] + [C.c_int] * 7 + [C.c_void_p, C.c_void_p]),
    "innfer_dihedral_index": (C.c_int, [C.c_int] * 5 + [C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "innfer_extract_tiles_u8_tta": (C.c_int, [C.c_void_p] + [C.c_int] * 5 + [C.c_double] + [C.c_int] * 4 + [C.c_void_p, C.c_int, C.c_void_p]),
    "innfer_recompose_u8_tta": (C.c_int, [C.c_void_p] + [C.c_int] * 6 + [C.c_double] + [C.c_int] * 7 + [C.c_void_p, C.c_void_p]),
    "innfer_resample_taps": (C.c_int, [C.c_int, C.c_int, C.c_int]),
    "innfer_resample_plan": (C.c_int, [C.c_int] * 4 + [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]),
    "innfer_resample_workspace_bytes": (C.c_size_t, [C.c_int] * 7),
    "innfer_resample_inthwc": (C.c_int, [C.c_void_p] + [C.c_int] * 4 + [C.c_void_p, C.c_int, C.c_int] + [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int] * 2
                               + [C.c_int, C.c_void_p, C.c_size_t, C.c_void_p]),
    "innfer_f32conv_packed_floats": (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    "innfer_pack_f32conv": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "innfer_f32conv": (C.c_int, [C.POINTER(F32ConvArgs), C.c_void_p]),
    "innfer_f32conv_plan": (C.c_int, [C.POINTER(F32ConvArgs), C.POINTER(C.c_int)]),
    "innfer_f32_norm": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_int64, C.c_int64, C.c_int, C.c_int, C.c_int64, C.c_int, C.c_float,
                                  C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int64, C.c_int64, C.c_int, C.c_void_p]),
    "innfer_gather_gemm_packed_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    "innfer_pack_gather_gemm": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "innfer_gather_gemm": (C.c_int, [C.POINTER(GatherGemmArgs), C.POINTER(C.c_int), C.c_void_p]),
    "innfer_gather_gemm_plan": (C.c_int, [C.POINTER(GatherGemmArgs), C.POINTER(C.c_int)]),
    "innfer_pan_attention_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    "innfer_pan_attention": (C.c_int, [C.c_void_p] * 4 + [C.c_int] * 3 + [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "innfer_pan_maxpool": (C.c_int, [C.c_void_p] + [C.c_int] * 5 + [C.c_void_p, C.c_void_p]),
    "innfer_pan_fsa_combine": (C.c_int, [C.c_void_p] + [C.c_int] * 3 + [C.c_void_p] + [C.c_int] * 4 + [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "innfer_pan_scpa_blob_bytes": (C.c_size_t, [C.c_int]),
    "innfer_pack_pan_scpa": (C.c_int, [C.c_void_p] * 8 + [C.c_int, C.c_void_p]),
    "innfer_pan_scpa_block": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p] + [C.c_int] * 6 + [C.c_void_p]),
    "innfer_pan_split_from_nchw": (C.c_int, [C.c_void_p, C.c_void_p] + [C.c_int] * 3 + [C.c_void_p]),
    "innfer_pan_split_to_nchw": (C.c_int, [C.c_void_p, C.c_void_p] + [C.c_int] * 3 + [C.c_void_p]),
    "innfer_conv_stats_records": (C.c_int, [C.c_int, C.c_int, C.c_int]),
    "innfer_norm_combine_parts": (C.c_int, [C.c_void_p, C.c_int, C.c_int64, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "innfer_norm_stats": (C.c_int, [C.c_void_p, C.c_int, C.c_int64, C.c_int, C.c_int64, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                    C.c_void_p, C.c_int64, C.c_void_p]),
    "innfer_resnet_post_slab_parts": (C.c_int, [C.c_void_p, C.c_int64, C.c_int, C.c_int64, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p,
                                                C.c_void_p, C.c_void_p]),
    "innfer_unet_post_slab_parts": (C.c_int, [C.c_void_p, C.c_int64, C.c_int, C.c_int64, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                              C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_void_p]),
    # (123) the UNet / ResNet engines' pass kernels, one launch at a time; a destination view = (pointer, group stride, channel offset, act)
    "innfer_unet_pre": (C.c_int, [C.c_void_p] + [C.c_int] * 5 + [C.c_void_p, C.c_int64, C.c_int, C.c_void_p]),
    "innfer_unet_post": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int64, C.c_int, C.c_void_p, C.c_void_p, C.c_int] +
                         [C.c_void_p, C.c_int64, C.c_int, C.c_int] * 2 + [C.c_void_p]),
    "innfer_unet_post_slab": (C.c_int, [C.c_void_p, C.c_int64, C.c_int, C.c_int64, C.c_int, C.c_void_p, C.c_void_p, C.c_int] +
                              [C.c_void_p, C.c_int64, C.c_int, C.c_int] * 2 + [C.c_void_p]),
    "innfer_unet_deep_post": (C.c_int, [C.c_void_p, C.c_int64] + [C.c_int] * 5 + [C.c_void_p] * 4 + [C.c_void_p, C.c_int64, C.c_int, C.c_int] * 2 + [C.c_void_p]),
    "innfer_unet_final": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int64, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "innfer_unet_first_packed_bytes": (C.c_size_t, []),
    "innfer_pack_unet_first": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p]),
    "innfer_unet_first_conv": (C.c_int, [C.c_void_p] + [C.c_int] * 5 + [C.c_void_p] * 4 + [C.c_int64, C.c_void_p]),
    "innfer_resnet_pre": (C.c_int, [C.c_void_p] + [C.c_int] * 5 + [C.c_void_p, C.c_int, C.c_void_p]),
    "innfer_resnet_post": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int64, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    "innfer_resnet_post_slab": (C.c_int, [C.c_void_p, C.c_int, C.c_int64, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    "innfer_resnet_post_slab_pad": (C.c_int, [C.c_void_p, C.c_int64] + [C.c_int] * 4 + [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int64, C.c_void_p]),
    "innfer_resnet_sum9_tanh": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p] + [C.c_int] * 5 + [C.c_void_p]),
    "innfer_resnet_final": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int64, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    # (124) the remaining pass kernels of PAN, PPON, the WBC UNet and the fp32 mode, one launch at a time
    "innfer_pan_pre": (C.c_int, [C.c_void_p] + [C.c_int] * 5 + [C.c_void_p, C.c_void_p]),
    "innfer_pan_upsample": (C.c_int, [C.c_void_p] + [C.c_int] * 7 + [C.c_int64, C.c_void_p, C.c_int64, C.c_void_p]),
    "innfer_pan_final": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p] + [C.c_int] * 5 + [C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "innfer_pan_slab_pair": (C.c_int, [C.c_void_p] + [C.c_int] * 4 + [C.c_void_p, C.c_int64, C.c_void_p]),
    "innfer_ppon_upsample3": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64] + [C.c_int] * 3 + [C.c_void_p]),
    "innfer_ppon_axpy": (C.c_int, [C.c_void_p] * 3 + [C.c_float, C.c_int64, C.c_int, C.c_int, C.c_void_p]),
    "innfer_wbc_pre": (C.c_int, [C.c_void_p] + [C.c_int] * 5 + [C.c_void_p, C.c_void_p]),
    "innfer_wbc_upadd": (C.c_int, [C.c_void_p, C.c_void_p] + [C.c_int] * 6 + [C.c_void_p, C.c_void_p]),
    "innfer_f32_prefix_lrelu": (C.c_int, [C.c_void_p] + [C.c_int] * 3 + [C.c_int64, C.c_void_p]),
    "innfer_f32_act_copy": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int64, C.c_int, C.c_int, C.c_void_p]),
    "innfer_tile_plan": (C.c_int, [C.c_int] * 4 + [C.POINTER(C.c_int)] * 6),
    "innfer_tile_owner": (C.c_int, [C.c_int] * 5 + [C.POINTER(C.c_int)] * 2),
    "innfer_extract_tiles_rect": (C.c_int, [C.c_void_p] + [C.c_int] * 8 + [C.c_void_p, C.c_void_p]),
    "innfer_extract_tiles_u8_rect": (C.c_int, [C.c_void_p] + [C.c_int] * 10 + [C.c_void_p, C.c_int, C.c_void_p]),
    "innfer_stitch_tiles": (C.c_int, [C.c_void_p] + [C.c_int] * 8 + [C.c_void_p, C.c_void_p]),
    "innfer_stitch_tiles_u8": (C.c_int, [C.c_void_p] + [C.c_int] * 10 + [C.c_void_p, C.c_void_p]),
    # (123, additive) many images as one tile stream: `sizes` is a host int array H_0, W_0, H_1, W_1, ...; the tables are innfer_multi_tile / innfer_multi_image
    "innfer_chop_multi_plan": (C.c_int, [C.c_int, C.c_void_p] + [C.c_int] * 3 + [C.c_double, C.c_int] + [C.c_void_p] * 7),
    "innfer_extract_tiles_u8_multi": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p] + [C.c_int] * 3 + [C.c_double, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "innfer_recompose_u8_multi": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_double] + [C.c_int] * 4 + [C.c_void_p] * 3),
}

# INNFER_ABI_ANY=1 (measurement only: scripts/evidence_r5.sh A/Bs an OLDER build of the library against the current one on one box): bind the entry points that
# library has and skip the revision check -- calls into entry points it lacks fail with AttributeError.  Never set for product use.
#  Only honoured together with INNFER_LIB pointing at a NON-default library, and loudly: struct layouts are not checked in this mode.
_ABI_ANY = os.environ.get("INNFER_ABI_ANY") == "1" and bool(os.environ.get("INNFER_LIB")) and os.path.realpath(os.environ["INNFER_LIB"]) != os.path.realpath(_DEFAULT_LIB)
if os.environ.get("INNFER_ABI_ANY") == "1":
    import warnings
    warnings.warn("INNFER_ABI_ANY=1: " + ("binding %s without the ABI revision / symbol check (measurement only; struct layouts are unchecked)" % LIB_PATH if _ABI_ANY
                  else "ignored -- it needs INNFER_LIB to name a library other than the in-tree default"), RuntimeWarning, stacklevel=2)
for _name, (_res, _args) in SIGNATURES.items():
    if _ABI_ANY and not hasattr(_lib, _name):
        continue
    _fn = getattr(_lib, _name)          # AttributeError here = header/library mismatch
    _fn.restype = _res
    _fn.argtypes = _args

lib = _lib

ABI_VERSION = 124       # the header revision this binding was written against (INNFER_ABI_VERSION)
if _lib.innfer_version() != ABI_VERSION and not _ABI_ANY:
    raise ImportError(f"{LIB_PATH} speaks ABI {_lib.innfer_version()}, this binding {ABI_VERSION}: rebuild with `make`")


def last_error():
    return _lib.innfer_last_error().decode(errors="replace")


def check(rc):
    """Map a status code to the exception the reference raises for that condition."""
    if rc == OK:
        return
    msg = last_error()
    if rc == ERR_INVALID:
        raise ValueError(msg)
    if rc == ERR_UNSUPPORTED:
        raise NotImplementedError(msg)
    if rc == ERR_NOMEM:                 # the class torch's allocator raises: parallel.run_tile_batches halves the tile batch on it
        import torch
        raise torch.OutOfMemoryError(msg)
    raise InnferError(f"innfer_amd status {rc}: {msg}")


COMM_ID_BYTES = 128


def shard_tiles(n_tiles, nranks, rank):
    first, count = C.c_int(), C.c_int()
    check(_lib.innfer_shard_tiles(n_tiles, nranks, rank, C.byref(first), C.byref(count)))
    return first.value, count.value


def chop_plan(H, W, patch=200, step=0.5):
    """(ps, ys, xs): host-side tile geometry."""
    ps, nh, nw = C.c_int(), C.c_int(), C.c_int()
    check(_lib.innfer_chop_plan(H, W, patch, step, C.byref(ps), C.byref(nh), C.byref(nw), None, None))
    ys, xs = (C.c_int * nh.value)(), (C.c_int * nw.value)()
    check(_lib.innfer_chop_plan(H, W, patch, step, C.byref(ps), C.byref(nh), C.byref(nw), ys, xs))
    return ps.value, list(ys), list(xs)


MULTI_TILE = [("img_off", "<i8"), ("H", "<i4"), ("W", "<i4"), ("oy", "<i4"), ("ox", "<i4")]                         # innfer_multi_tile
MULTI_IMAGE = [("out_off", "<i8"), ("first", "<i8"), ("FH", "<i4"), ("FW", "<i4"), ("nh", "<i4"), ("nw", "<i4")]     # innfer_multi_image


def chop_multi_plan(sizes, channels, pad=0, patch=200, step=0.5, scale=1):
    """innfer_chop_multi_plan (host only): the geometry of the images [(H, W), ...] of `channels` channels as ONE tile stream -- a dict of ps, sizes (int32 [n, 2],
    what the kernels' entry points take), counts [n], first [n + 1], in_off / out_off (int64 [n + 1], bytes; the last entry is the packed buffer's size) and
    the two tables the caller uploads: tiles (MULTI_TILE records, one per tile, for the gather) and images (MULTI_IMAGE records, for the blend at `scale`)."""
    import numpy as np
    hw = np.ascontiguousarray(np.asarray(sizes, dtype=np.int32).reshape(-1, 2))
    n = hw.shape[0]
    ps = C.c_int()
    counts, first = np.zeros(n, np.int32), np.zeros(n + 1, np.int32)
    in_off, out_off = np.zeros(n + 1, np.int64), np.zeros(n + 1, np.int64)
    images = np.zeros(n, np.dtype(MULTI_IMAGE))
    args = (n, hw.ctypes.data, int(channels), int(pad), int(patch), float(step), int(scale), C.byref(ps), counts.ctypes.data, first.ctypes.data,
            in_off.ctypes.data, out_off.ctypes.data)
    check(_lib.innfer_chop_multi_plan(*args, None, images.ctypes.data))
    tiles = np.zeros(int(first[n]), np.dtype(MULTI_TILE))
    check(_lib.innfer_chop_multi_plan(*args, tiles.ctypes.data, images.ctypes.data))
    return dict(ps=ps.value, sizes=hw, counts=counts, first=first, in_off=in_off, out_off=out_off, tiles=tiles, images=images)


def tile_plan(H, W, tile, halo=16):
    """innfer_tile_plan (host only): (ph, pw, ys, xs), the lattice of the stitched tile path (`-tile N -tile_pad P`) -- per axis of A pixels
    n = 1, P = A where A <= tile + 2 halo, else n = ceil((A - 2 halo) / tile), P = ceil((A + 2 halo (n - 1)) / n), origins min(i (P - 2 halo), A - P)."""
    ph, pw, nh, nw = C.c_int(), C.c_int(), C.c_int(), C.c_int()
    check(_lib.innfer_tile_plan(int(H), int(W), int(tile), int(halo), C.byref(ph), C.byref(pw), C.byref(nh), C.byref(nw), None, None))
    ys, xs = (C.c_int * nh.value)(), (C.c_int * nw.value)()
    check(_lib.innfer_tile_plan(int(H), int(W), int(tile), int(halo), None, None, None, None, ys, xs))
    return ph.value, pw.value, list(ys), list(xs)


def tile_owner(A, tile, halo, X, scale=1):
    """innfer_tile_owner (host only): (index, origin) of the tile that owns position X of the scale * A output axis, as the stitch kernels compute it:
    index = the largest i with i == 0 or o_i + halo <= X // scale, origin = scale * o_index."""
    index, origin = C.c_int(), C.c_int()
    check(_lib.innfer_tile_owner(int(A), int(tile), int(halo), int(scale), int(X), C.byref(index), C.byref(origin)))
    return index.value, origin.value


BORDER_MODES = {"tile": 0, "mirror": 1, "replicate": 2, "alpha_pad": 3}       # INNFER_BORDER_*: the seamless modes
BORDER_OUTSIDE = -1


def border_index(i, n, mode):
    """innfer_border_index (host only): the source index the seamless kernels read for position i (relative to the image) on an axis of n pixels;
    BORDER_OUTSIDE for alpha_pad outside the image.  mode: a name of BORDER_MODES or its code."""
    r = _lib.innfer_border_index(int(i), int(n), BORDER_MODES.get(mode, mode) if isinstance(mode, str) else int(mode))
    if r < BORDER_OUTSIDE:
        raise ValueError(last_error())
    return r


def dihedral_index(k, H, W, y, x):
    """innfer_dihedral_index (host only): (sy, sx), the pixel of an H x W image that pixel (y, x) of its orientation k shows (t_k: transpose if k & 4,
    then flip the columns if k & 1, then flip the rows if k & 2).  ValueError for k outside 0 .. 7 or a pixel outside the oriented image."""
    sy, sx = C.c_int(), C.c_int()
    check(_lib.innfer_dihedral_index(int(k), int(H), int(W), int(y), int(x), C.byref(sy), C.byref(sx)))
    return sy.value, sx.value


RESAMPLE_FILTERS = {"box": 0, "bilinear": 1, "bicubic": 2, "lanczos": 3}     # INNFER_RESAMPLE_*: the filters of the resampler (-outfilter)


def resample_filter(filter):
    """The INNFER_RESAMPLE_* code of a filter name (or the code itself); ValueError for anything else."""
    code = RESAMPLE_FILTERS.get(filter, -1) if isinstance(filter, str) else filter
    if code not in RESAMPLE_FILTERS.values():
        raise ValueError(f"resample: filter must be one of {', '.join(RESAMPLE_FILTERS)}, got {filter!r}")
    return int(code)


COLOR_FIX_MODES = {"lowfreq": 0, "wavelet": 1, "adain": 2}                    # INNFER_COLOR_FIX_*: the colour fixes (-cf_mode)


def color_fix_mode(mode):
    """The INNFER_COLOR_FIX_* code of a mode name; ValueError for anything else."""
    if not isinstance(mode, str) or mode not in COLOR_FIX_MODES:
        raise ValueError(f"color_fix: mode must be one of {', '.join(COLOR_FIX_MODES)}, got {mode!r}")
    return COLOR_FIX_MODES[mode]


def resample_taps(n_in, n_out, filter="lanczos"):
    """innfer_resample_taps (host only): the widest window of the axis n_in -> n_out, wrapped or not."""
    T = _lib.innfer_resample_taps(int(n_in), int(n_out), resample_filter(filter))
    if T < 0:
        raise ValueError(last_error())
    return T


def resample_plan(n_in, n_out, filter="lanczos", wrap=False, T=None):
    """innfer_resample_plan (host only): (start int32 [n_out], count int32 [n_out], weights float32 [n_out, T]) of one axis; T defaults to
    resample_taps.  Output i is the sum over t < count[i] of weights[i, t] * sample (start[i] + t) (mod n_in when wrapping)."""
    import numpy as np
    code = resample_filter(filter)
    T = resample_taps(n_in, n_out, code) if T is None else int(T)
    start, count = np.empty(n_out, np.int32), np.empty(n_out, np.int32)
    weights = np.empty((n_out, T), np.float32)
    check(_lib.innfer_resample_plan(int(n_in), int(n_out), code, int(bool(wrap)), start.ctypes.data, count.ctypes.data, weights.ctypes.data, T))
    return start, count, weights


F32_PLAN_KEYS = ("direct", "NKT", "NPT", "IMG", "CC", "vec4", "workgroups", "lds")


def f32conv_args(taps, **fields):
    """F32ConvArgs from keyword fields (names of the struct) and the tap list [(dy, dx)]; pointers as integers."""
    a = F32ConvArgs(**fields)
    a.ntap = len(taps)
    for i, (dy, dx) in enumerate(taps):
        a.dy[i], a.dx[i] = dy, dx
    return a


def f32conv_plan(a):
    """innfer_f32conv_plan (host only): what innfer_f32conv would launch for the F32ConvArgs `a`, as a dict of F32_PLAN_KEYS."""
    plan = (C.c_int * 8)()
    check(_lib.innfer_f32conv_plan(C.byref(a), plan))
    return dict(zip(F32_PLAN_KEYS, plan))


GATHER_GEMM_INFO_KEYS = ("shape", "ksplit", "seg", "taps", "split_bytes")


def gather_gemm_args(dy, dx, **fields):
    """GatherGemmArgs from keyword fields (names of the struct) and the tap displacements dy / dx (for g_phase: the four groups' lists back to back, ntaps per
    group given as a field); pointers as integers."""
    a = GatherGemmArgs(**fields)
    if "ntaps" not in fields:
        a.ntaps = len(dy)
    for i, (y, x) in enumerate(zip(dy, dx)):
        a.dy[i], a.dx[i] = y, x
    return a


def gather_gemm_plan(a):
    """innfer_gather_gemm_plan (host only): what innfer_gather_gemm would launch for the GatherGemmArgs `a`, as a dict of GATHER_GEMM_INFO_KEYS."""
    info = (C.c_int * 5)()
    check(_lib.innfer_gather_gemm_plan(C.byref(a), info))
    return dict(zip(GATHER_GEMM_INFO_KEYS, info))


def blend_profile(P, step=0.5, scale=1):
    import numpy as np
    buf = (C.c_float * P)()
    check(_lib.innfer_blend_profile(P, step, scale, buf))
    return np.frombuffer(buf, dtype=np.float32).copy()


def timed_launches(fn, stream=None, cap=4096, name_cap=64):
    """fn() under the library's launch timer (innfer_timer_start / innfer_timer_stop): [(kernel family, ms, algorithmic flops, algorithmic bytes)] of
    every instrumented launch fn made on this thread, in issue order.  Measurement only."""
    import torch
    if stream is None:
        stream = torch.cuda.current_stream().cuda_stream
    names = C.create_string_buffer(cap * name_cap)
    ms, fl, by, n = (C.c_float * cap)(), (C.c_double * cap)(), (C.c_double * cap)(), C.c_int()
    check(_lib.innfer_timer_start())
    try:
        fn()
    finally:
        rc = _lib.innfer_timer_stop(stream, cap, names, name_cap, ms, fl, by, C.byref(n))
    check(rc)
    raw = names.raw
    return [(raw[i * name_cap:(i + 1) * name_cap].split(b"\0", 1)[0].decode(), ms[i], fl[i], by[i]) for i in range(min(n.value, cap))]
