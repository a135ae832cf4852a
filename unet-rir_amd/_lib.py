"""ctypes binding of libunetrir.so (the C ABI declared in include/unetrir.h).

There is no CPU fallback: if the library is missing or a call fails, this raises.
"""
import ctypes as C
import os

from . import build as _build

_LIB = None

c_f32p = C.c_void_p   # device pointers travel as integers
c_stream = C.c_void_p


class CastDesc(C.Structure):
    """unetrir_cast_desc (include/unetrir.h)."""
    _fields_ = [("w", C.c_void_p), ("same", C.c_void_p), ("transposed", C.c_void_p), ("N", C.c_int), ("T", C.c_int), ("C", C.c_int),
                ("Cp", C.c_int), ("Np", C.c_int), ("reserved", C.c_int), ("packed_s2", C.c_void_p)]


class ReduceDesc(C.Structure):
    """unetrir_reduce_desc (include/unetrir.h): one deferred split-K reduction."""
    _fields_ = [("part", C.c_void_p), ("nsplit", C.c_int), ("n", C.c_size_t), ("out", C.c_void_p), ("reg", C.c_float), ("w", C.c_void_p)]


class LambSeg(C.Structure):
    """unetrir_lamb_seg (include/unetrir.h): one variable of the LAMB segment table."""
    _fields_ = [("offset", C.c_longlong), ("count", C.c_longlong), ("slot", C.c_longlong), ("flags", C.c_int), ("chunk0", C.c_int)]


class Config(C.Structure):
    """unetrir_config: kernel-selection switches (include/unetrir.h)."""
    _fields_ = [(n, C.c_int) for n in ("conv3x3", "conv3x3g", "conv3x3g_pair", "conv3x3h", "conv3x3s", "conv3x3r", "stem",
                                       "upconv3x3g", "wgrad3x3g", "wgrad3x3r", "head_mfma", "wgrad3x3d", "conv3x3d", "conv3x3p", "upconv3x3q", "dyn_tiles", "pw1x1", "igemm2")]


class ConvGeom(C.Structure):
    """unetrir_conv_geom"""
    _fields_ = [("B", C.c_int), ("H", C.c_int), ("W", C.c_int), ("Cin", C.c_int), ("Cout", C.c_int),
                ("k", C.c_int), ("stride", C.c_int)]


_SIGS = {
    "unetrir_abi_version": (C.c_int, []),
    "unetrir_get_config": (C.c_int, [C.POINTER(Config)]),
    "unetrir_set_config": (C.c_int, [C.POINTER(Config)]),
    "unetrir_conv2d_fwd_f32": (C.c_int, [C.POINTER(ConvGeom), c_f32p, C.c_int, c_f32p, c_f32p, c_f32p, C.c_int,
                                         c_f32p, C.c_int, c_stream]),
    "unetrir_conv2d_dgrad_f32": (C.c_int, [C.POINTER(ConvGeom), c_f32p, C.c_int, c_f32p, c_f32p, C.c_int, c_f32p,
                                           C.c_int, c_stream]),
    "unetrir_conv2d_wgrad_ws_bytes": (C.c_size_t, [C.POINTER(ConvGeom)]),
    "unetrir_conv2d_wgrad_f32": (C.c_int, [C.POINTER(ConvGeom), c_f32p, C.c_int, c_f32p, C.c_int, c_f32p, C.c_float,
                                           c_f32p, C.c_void_p, C.c_size_t, c_stream]),
    "unetrir_conv2d_transpose_fwd_f32": (C.c_int, [C.POINTER(ConvGeom), c_f32p, C.c_int, c_f32p, c_f32p, c_f32p,
                                                   C.c_int, c_stream]),
    "unetrir_conv2d_transpose_dgrad_f32": (C.c_int, [C.POINTER(ConvGeom), c_f32p, C.c_int, c_f32p, c_f32p, C.c_int,
                                                     c_f32p, C.c_int, c_stream]),
    "unetrir_conv2d_transpose_wgrad_ws_bytes": (C.c_size_t, [C.POINTER(ConvGeom)]),
    "unetrir_conv2d_transpose_wgrad_f32": (C.c_int, [C.POINTER(ConvGeom), c_f32p, C.c_int, c_f32p, C.c_int, c_f32p,
                                                     C.c_float, c_f32p, C.c_void_p, C.c_size_t, c_stream]),
    "unetrir_dense_fwd_ws_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    "unetrir_dense_fwd_f32": (C.c_int, [c_f32p, C.c_int, c_f32p, c_f32p, c_f32p, C.c_int, C.c_int, C.c_int, C.c_int,
                                        C.c_void_p, C.c_size_t, c_stream]),
    "unetrir_transpose_weight_f32": (C.c_int, [c_f32p, c_f32p, C.c_int, C.c_int, C.c_int, c_stream]),
    "unetrir_bn_ws_bytes": (C.c_size_t, [C.c_longlong, C.c_int]),
    "unetrir_bn_stats_f32": (C.c_int, [c_f32p, C.c_int, C.c_longlong, C.c_int, c_f32p, c_f32p, C.c_float, C.c_float,
                                       c_f32p, c_f32p, c_f32p, c_f32p, C.c_void_p, C.c_size_t, c_stream]),
    "unetrir_bn_apply_f32": (C.c_int, [c_f32p, C.c_int, C.c_longlong, C.c_int, c_f32p, C.c_int, c_f32p, C.c_int,
                                       c_stream]),
    "unetrir_bn_bwd_f32": (C.c_int, [c_f32p, C.c_int, c_f32p, C.c_int, C.c_longlong, C.c_int, c_f32p, c_f32p, c_f32p,
                                     C.c_int, c_f32p, C.c_int, c_f32p, c_f32p, C.c_void_p, C.c_size_t, c_stream]),
    "unetrir_colsum_f32": (C.c_int, [c_f32p, C.c_int, C.c_longlong, C.c_int, c_f32p, C.c_void_p, C.c_size_t,
                                     c_stream]),
    "unetrir_relu_fwd_f32": (C.c_int, [c_f32p, C.c_int, C.c_longlong, C.c_int, c_f32p, C.c_int, c_stream]),
    "unetrir_relu_bwd_f32": (C.c_int, [c_f32p, C.c_int, c_f32p, C.c_int, C.c_longlong, C.c_int, c_f32p, C.c_int,
                                       c_stream]),
    "unetrir_bn_act_add_f32": (C.c_int, [c_f32p, C.c_int, C.c_longlong, C.c_int, c_f32p, C.c_int, c_f32p, C.c_int, c_f32p,
                                         C.c_int, c_stream]),
    "unetrir_act_bwd_f32": (C.c_int, [c_f32p, C.c_int, c_f32p, C.c_int, C.c_longlong, C.c_int, C.c_int, c_f32p, C.c_int,
                                      c_stream]),
    "unetrir_add_f32": (C.c_int, [c_f32p, c_f32p, c_f32p, C.c_longlong, c_stream]),
    "unetrir_nchw_to_nhwc_pad_f32": (C.c_int, [c_f32p, C.c_int, C.c_int, C.c_int, C.c_int, c_f32p, C.c_int,
                                               c_stream]),
    "unetrir_head6x6_supported": (C.c_int, [C.c_int]),
    "unetrir_head6x6_fwd_f32": (C.c_int, [c_f32p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, c_f32p, c_f32p, c_f32p,
                                          C.c_int, c_stream]),
    "unetrir_head6x6_wgrad_ws_bytes": (C.c_size_t, [C.c_int]),
    "unetrir_head6x6_wgrad_f32": (C.c_int, [c_f32p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, c_f32p, C.c_int, c_f32p,
                                            C.c_void_p, C.c_size_t, c_stream]),
    "unetrir_loss_ws_bytes": (C.c_size_t, [C.c_longlong]),
    "unetrir_sigmoid_loss_f32": (C.c_int, [c_f32p, C.c_int, c_f32p, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float,
                                           c_f32p, c_f32p, c_f32p, C.c_void_p, C.c_size_t, c_stream]),
    "unetrir_sigmoid_nchw_f32": (C.c_int, [c_f32p, C.c_int, C.c_int, C.c_int, C.c_int, c_f32p, c_stream]),
    "unetrir_sigmoid_bwd_f32": (C.c_int, [c_f32p, c_f32p, C.c_int, C.c_int, C.c_int, c_f32p, c_stream]),
    "unetrir_embedding_fwd_f32": (C.c_int, [C.c_void_p, C.c_int, c_f32p, C.c_int, C.c_int, c_f32p, c_stream]),
    "unetrir_embedding_bwd_f32": (C.c_int, [C.c_void_p, C.c_int, c_f32p, C.c_int, C.c_int, c_f32p, c_stream]),
    "unetrir_mul_f32": (C.c_int, [c_f32p, c_f32p, c_f32p, C.c_longlong, c_stream]),
    "unetrir_sumsq_f32": (C.c_int, [c_f32p, C.c_longlong, C.c_float, c_f32p, C.c_int, C.c_void_p, C.c_size_t,
                                    c_stream]),
    "unetrir_adam_f32": (C.c_int, [c_f32p, c_f32p, c_f32p, c_f32p, C.c_longlong, C.c_float, C.c_float, C.c_float,
                                   C.c_float, C.c_float, c_stream]),
    # ---- bf16-storage variants (same argument lists; pointers are void*) ----
    "unetrir_conv2d_fwd_bf16": (C.c_int, [C.POINTER(ConvGeom), c_f32p, C.c_int, c_f32p, c_f32p, c_f32p, C.c_int,
                                          c_f32p, C.c_int, c_stream]),
    "unetrir_conv3x3s2_packed_elems": (C.c_size_t, [C.c_int, C.c_int]),
    "unetrir_conv2d_fwd_packed_bf16": (C.c_int, [C.POINTER(ConvGeom), c_f32p, C.c_int, c_f32p, c_f32p, c_f32p, c_f32p, C.c_int,
                                                 c_f32p, C.c_int, c_stream]),
    "unetrir_conv2d_transpose_dgrad_packed_bf16": (C.c_int, [C.POINTER(ConvGeom), c_f32p, C.c_int, c_f32p, c_f32p, c_f32p, C.c_int,
                                                             c_f32p, C.c_int, c_stream]),
    "unetrir_conv2d_dgrad_bf16": (C.c_int, [C.POINTER(ConvGeom), c_f32p, C.c_int, c_f32p, c_f32p, C.c_int, c_f32p,
                                            C.c_int, c_stream]),
    "unetrir_conv2d_wgrad_bf16": (C.c_int, [C.POINTER(ConvGeom), c_f32p, C.c_int, c_f32p, C.c_int, c_f32p, C.c_float,
                                            c_f32p, C.c_void_p, C.c_size_t, c_stream]),
    "unetrir_conv2d_transpose_fwd_bf16": (C.c_int, [C.POINTER(ConvGeom), c_f32p, C.c_int, c_f32p, c_f32p, c_f32p,
                                                    C.c_int, c_stream]),
    "unetrir_conv2d_transpose_dgrad_bf16": (C.c_int, [C.POINTER(ConvGeom), c_f32p, C.c_int, c_f32p, c_f32p, C.c_int,
                                                      c_f32p, C.c_int, c_stream]),
    "unetrir_conv2d_wgrad_partials_bf16": (C.c_int, [C.POINTER(ConvGeom), c_f32p, C.c_int, c_f32p, C.c_int, c_f32p, C.c_float, c_f32p,
                                                     C.c_void_p, C.c_size_t, C.POINTER(ReduceDesc), c_stream]),
    "unetrir_conv2d_transpose_wgrad_partials_bf16": (C.c_int, [C.POINTER(ConvGeom), c_f32p, C.c_int, c_f32p, C.c_int, c_f32p, C.c_float,
                                                               c_f32p, C.c_void_p, C.c_size_t, C.POINTER(ReduceDesc), c_stream]),
    "unetrir_splitk_reduce_batched": (C.c_int, [C.POINTER(ReduceDesc), C.c_int, c_stream]),
    "unetrir_conv2d_transpose_wgrad_bf16": (C.c_int, [C.POINTER(ConvGeom), c_f32p, C.c_int, c_f32p, C.c_int, c_f32p,
                                                      C.c_float, c_f32p, C.c_void_p, C.c_size_t, c_stream]),
    # the 2x2 stride-2 layers (conv2x2.hip): the argument lists of their unetrir_conv2d_* twins
    "unetrir_conv2x2s2_supported_bf16": (C.c_int, [C.POINTER(ConvGeom), C.c_int, C.c_int]),
    "unetrir_conv2x2s2_transpose_supported_bf16": (C.c_int, [C.POINTER(ConvGeom), C.c_int, C.c_int]),
    "unetrir_conv2x2s2_fwd_bf16": (C.c_int, [C.POINTER(ConvGeom), c_f32p, C.c_int, c_f32p, c_f32p, c_f32p, C.c_int, c_f32p, C.c_int,
                                             c_stream]),
    "unetrir_conv2x2s2_dgrad_bf16": (C.c_int, [C.POINTER(ConvGeom), c_f32p, C.c_int, c_f32p, c_f32p, C.c_int, c_f32p, C.c_int, c_stream]),
    "unetrir_conv2x2s2_wgrad_ws_bytes": (C.c_size_t, [C.POINTER(ConvGeom)]),
    "unetrir_conv2x2s2_wgrad_bf16": (C.c_int, [C.POINTER(ConvGeom), c_f32p, C.c_int, c_f32p, C.c_int, c_f32p, C.c_float, c_f32p,
                                               C.c_void_p, C.c_size_t, c_stream]),
    "unetrir_conv2x2s2_wgrad_partials_bf16": (C.c_int, [C.POINTER(ConvGeom), c_f32p, C.c_int, c_f32p, C.c_int, c_f32p, C.c_float, c_f32p,
                                                        C.c_void_p, C.c_size_t, C.POINTER(ReduceDesc), c_stream]),
    "unetrir_conv2x2s2_transpose_fwd_bf16": (C.c_int, [C.POINTER(ConvGeom), c_f32p, C.c_int, c_f32p, c_f32p, c_f32p, C.c_int, c_stream]),
    "unetrir_conv2x2s2_transpose_dgrad_bf16": (C.c_int, [C.POINTER(ConvGeom), c_f32p, C.c_int, c_f32p, c_f32p, C.c_int, c_f32p, C.c_int,
                                                         c_stream]),
    "unetrir_conv2x2s2_transpose_wgrad_ws_bytes": (C.c_size_t, [C.POINTER(ConvGeom)]),
    "unetrir_conv2x2s2_transpose_wgrad_bf16": (C.c_int, [C.POINTER(ConvGeom), c_f32p, C.c_int, c_f32p, C.c_int, c_f32p, C.c_float, c_f32p,
                                                         C.c_void_p, C.c_size_t, c_stream]),
    "unetrir_conv2x2s2_transpose_wgrad_partials_bf16": (C.c_int, [C.POINTER(ConvGeom), c_f32p, C.c_int, c_f32p, C.c_int, c_f32p, C.c_float,
                                                                  c_f32p, C.c_void_p, C.c_size_t, C.POINTER(ReduceDesc), c_stream]),
    "unetrir_cast_weight_bf16": (C.c_int, [c_f32p, c_f32p, C.c_int, C.c_int, C.c_int, C.c_int, c_stream]),
    "unetrir_transpose_cast_weight_bf16": (C.c_int, [c_f32p, c_f32p, C.c_int, C.c_int, C.c_int, C.c_int, c_stream]),
    "unetrir_bn_stats_bf16": (C.c_int, [c_f32p, C.c_int, C.c_longlong, C.c_int, c_f32p, c_f32p, C.c_float, C.c_float,
                                        c_f32p, c_f32p, c_f32p, c_f32p, C.c_void_p, C.c_size_t, c_stream]),
    "unetrir_bn_apply_bf16": (C.c_int, [c_f32p, C.c_int, C.c_longlong, C.c_int, c_f32p, C.c_int, c_f32p, C.c_int,
                                        c_stream]),
    "unetrir_bn_bwd_bf16": (C.c_int, [c_f32p, C.c_int, c_f32p, C.c_int, C.c_longlong, C.c_int, c_f32p, c_f32p,
                                      C.c_int, c_f32p, C.c_int, c_f32p, c_f32p, C.c_void_p, C.c_size_t, c_stream]),
    "unetrir_colsum_bf16": (C.c_int, [c_f32p, C.c_int, C.c_longlong, C.c_int, c_f32p, C.c_void_p, C.c_size_t,
                                      c_stream]),
    "unetrir_relu_bwd_bf16": (C.c_int, [c_f32p, C.c_int, c_f32p, C.c_int, C.c_longlong, C.c_int, c_f32p, C.c_int,
                                        c_stream]),
    "unetrir_nchw_to_nhwc_pad_bf16": (C.c_int, [c_f32p, C.c_int, C.c_int, C.c_int, C.c_int, c_f32p, C.c_int,
                                                c_stream]),
    "unetrir_head6x6_fwd_bf16": (C.c_int, [c_f32p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, c_f32p, c_f32p, c_f32p,
                                           C.c_int, c_stream]),
    "unetrir_head6x6_wgrad_bf16": (C.c_int, [c_f32p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, c_f32p, C.c_int,
                                             c_f32p, C.c_void_p, C.c_size_t, c_stream]),
    "unetrir_stem_composite_supported": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    "unetrir_stem_composite_ws_bytes": (C.c_size_t, [C.c_int]),
    "unetrir_stem_composite_bf16": (C.c_int, [c_f32p, C.c_int, c_f32p, C.c_int, C.c_int, C.c_int, C.c_int, c_f32p, C.c_float, c_f32p,
                                              c_f32p, C.c_int, c_f32p, C.c_void_p, C.c_size_t, c_stream]),
    "unetrir_stage_h2d": (C.c_int, [C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), c_stream]),
    "unetrir_conv2d_colstat_rows_bf16": (C.c_longlong, [C.POINTER(ConvGeom), C.c_int, C.c_int]),
    "unetrir_conv3x3_kernel_id_bf16": (C.c_int, [C.POINTER(ConvGeom), C.c_int, C.c_int]),
    "unetrir_conv2d_fwd_colstat_bf16": (C.c_int, [C.POINTER(ConvGeom), c_f32p, C.c_int, c_f32p, c_f32p, c_f32p, C.c_int, c_f32p, C.c_int,
                                                  c_f32p, c_stream]),
    "unetrir_conv2d_dgrad_colstat_bf16": (C.c_int, [C.POINTER(ConvGeom), c_f32p, C.c_int, c_f32p, c_f32p, C.c_int, c_f32p, C.c_int,
                                                    c_f32p, c_stream]),
    "unetrir_conv2d_transpose_colstat_rows_bf16": (C.c_longlong, [C.POINTER(ConvGeom), C.c_int]),
    "unetrir_conv2d_transpose_fwd_colstat_bf16": (C.c_int, [C.POINTER(ConvGeom), c_f32p, C.c_int, c_f32p, c_f32p, c_f32p, C.c_int, c_f32p,
                                                            c_stream]),
    "unetrir_bn_stats_colstat": (C.c_int, [c_f32p, C.c_longlong, C.c_longlong, C.c_int, c_f32p, c_f32p, C.c_float, C.c_float,
                                           c_f32p, c_f32p, c_f32p, c_f32p, c_stream]),
    "unetrir_bn_colstat_act_add_f32": (C.c_int, [c_f32p, C.c_longlong, c_f32p, C.c_int, C.c_longlong, C.c_int, c_f32p, c_f32p, C.c_float, C.c_float, c_f32p, c_f32p, c_f32p, c_f32p, C.c_int, c_f32p, C.c_int, c_f32p, C.c_int, c_stream]),
    "unetrir_bn_colstat_act_add_bf16": (C.c_int, [c_f32p, C.c_longlong, c_f32p, C.c_int, C.c_longlong, C.c_int, c_f32p, c_f32p, C.c_float, C.c_float, c_f32p, c_f32p, c_f32p, c_f32p, C.c_int, c_f32p, C.c_int, c_f32p, C.c_int, c_stream]),
    "unetrir_colsum_colstat": (C.c_int, [c_f32p, C.c_longlong, C.c_int, C.c_int, C.c_int, c_f32p, c_stream]),
    "unetrir_cast_weights_batched_bf16": (C.c_int, [C.c_void_p, C.c_int, c_stream]),
    "unetrir_dense_dgrad_supported": (C.c_int, [C.c_int, C.c_int, C.c_int]),
    "unetrir_dense_dgrad_ws_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    "unetrir_dense_dgrad_f32": (C.c_int, [c_f32p, C.c_int, c_f32p, c_f32p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_size_t,
                                          c_stream]),
    "unetrir_stft_frames": (C.c_int, [C.c_int, C.c_int]),
    "unetrir_stft_features_f32": (C.c_int, [c_f32p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                            c_f32p, C.c_int, C.c_int, c_stream]),
    "unetrir_istft_features_f32": (C.c_int, [c_f32p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                             C.c_int, c_f32p, c_stream]),
    # waveform-domain loss and its gradient on the prediction (waveloss.hip)
    "unetrir_wave_loss_ws_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    "unetrir_wave_loss_f32": (C.c_int, [c_f32p, c_f32p, c_f32p, c_f32p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                        C.c_int, C.c_int, C.c_double, C.c_double, c_f32p, c_f32p, C.c_float, C.c_float, c_f32p, c_f32p,
                                        C.c_void_p, c_f32p, C.c_void_p, C.c_size_t, c_stream]),
    # the vector-Jacobian product of PostProcess (istft_bwd.hip) and the loss on the energy decay curve (decayloss.hip)
    "unetrir_istft_features_bwd_f32": (C.c_int, [c_f32p, c_f32p, c_f32p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                                 C.c_int, C.c_int, c_f32p, c_stream]),
    "unetrir_decay_loss_ws_bytes": (C.c_size_t, [C.c_int, C.c_int]),
    "unetrir_decay_loss_supported": (C.c_int, [C.c_int]),
    "unetrir_decay_loss_f32": (C.c_int, [c_f32p, c_f32p, C.c_int, C.c_int, C.c_double, C.c_double, C.c_double, c_f32p, C.c_void_p,
                                         c_f32p, C.c_void_p, C.c_size_t, c_stream]),
    # the multi-resolution STFT loss on the waveform (spectralloss.hip); res is a host array of 3 R ints
    "unetrir_spectral_loss_supported": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int]),
    "unetrir_spectral_loss_ws_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int)]),
    "unetrir_spectral_loss_f32": (C.c_int, [c_f32p, c_f32p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.c_double, C.c_double,
                                            C.c_double, C.c_double, C.c_double, C.c_int, c_f32p, C.c_void_p, c_f32p, C.c_void_p,
                                            C.c_size_t, c_stream]),
    # the same loss with fp32 FFTs in LDS (spectralloss_fft.hip)
    "unetrir_spectral_loss_fft_supported": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int]),
    "unetrir_spectral_loss_fft_ws_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int)]),
    "unetrir_spectral_loss_fft_f32": (C.c_int, [c_f32p, c_f32p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.c_double, C.c_double,
                                                C.c_double, C.c_double, C.c_double, C.c_int, c_f32p, C.c_void_p, c_f32p, C.c_void_p,
                                                C.c_size_t, c_stream]),
    # y = h * x on the fp32 matrix cores (auralize.hip)
    "unetrir_auralize_supported": (C.c_int, [C.c_int]),
    "unetrir_auralize_f32": (C.c_int, [c_f32p, c_f32p, c_f32p, C.c_int, C.c_int, C.c_int, C.c_longlong, C.c_int, c_stream]),
    # the same by partitioned overlap-save, FFTs in LDS (auralize_fft.hip)
    "unetrir_auralize_fft_supported": (C.c_int, [C.c_int]),
    "unetrir_auralize_fft_block": (C.c_int, [C.c_int]),
    "unetrir_auralize_fft_ws_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int, C.c_longlong, C.c_int]),
    "unetrir_auralize_fft_f32": (C.c_int, [c_f32p, c_f32p, c_f32p, C.c_int, C.c_int, C.c_int, C.c_longlong, C.c_int, C.c_void_p,
                                           C.c_size_t, c_stream]),
    # a moving listener: the same spectra, blended per output block along a path of responses (auralize_fft.hip)
    "unetrir_auralize_path_supported": (C.c_int, [C.c_int]),
    "unetrir_auralize_path_ws_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_longlong, C.c_int]),
    "unetrir_auralize_path_f32": (C.c_int, [c_f32p, C.c_void_p, c_f32p, c_f32p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_longlong, C.c_int,
                                            C.c_void_p, C.c_size_t, c_stream]),
    "unetrir_eval_metrics_f32": (C.c_int, [c_f32p, c_f32p, c_f32p, C.c_int, C.c_int, C.c_int, c_f32p, c_f32p, C.c_int, C.c_int,
                                           C.c_void_p, c_stream]),
    "unetrir_eval_accumulate": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, c_stream]),
    # room-acoustic figures (acoustics.hip)
    "unetrir_acoustic_figures_f32": (C.c_int, [c_f32p, c_f32p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.c_void_p,
                                               c_stream]),
    "unetrir_acoustic_accumulate": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_double, C.c_void_p, C.c_void_p, c_stream]),
    "unetrir_head6x6_dgrad_supported": (C.c_int, [C.c_int, C.c_int]),
    "unetrir_head6x6_dgrad_bf16": (C.c_int, [c_f32p, C.c_int, C.c_int, C.c_int, C.c_int, c_f32p, C.c_int, c_f32p, C.c_int,
                                             c_stream]),
    "unetrir_sigmoid_loss_bf16": (C.c_int, [c_f32p, C.c_int, c_f32p, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float,
                                            c_f32p, c_f32p, c_f32p, C.c_void_p, C.c_size_t, c_stream]),
    "unetrir_sigmoid_bwd_bf16": (C.c_int, [c_f32p, c_f32p, C.c_int, C.c_int, C.c_int, c_f32p, c_stream]),
    "unetrir_add_f32_to_bf16": (C.c_int, [c_f32p, c_f32p, c_f32p, C.c_longlong, c_stream]),
    "unetrir_cast_bf16_to_f32": (C.c_int, [c_f32p, c_f32p, C.c_longlong, c_stream]),
    "unetrir_cast_f32_to_bf16": (C.c_int, [c_f32p, c_f32p, C.c_longlong, c_stream]),
    "unetrir_bn_act_add_bf16": (C.c_int, [c_f32p, C.c_int, C.c_longlong, C.c_int, c_f32p, C.c_int, c_f32p, C.c_int, c_f32p,
                                          C.c_int, c_stream]),
    "unetrir_act_bwd_bf16": (C.c_int, [c_f32p, C.c_int, c_f32p, C.c_int, C.c_longlong, C.c_int, C.c_int, c_f32p, C.c_int,
                                       c_stream]),
    "unetrir_bn_inference_affine_f32": (C.c_int, [c_f32p, c_f32p, c_f32p, c_f32p, C.c_float, C.c_int, c_f32p, c_stream]),
    "unetrir_dropout_mask_f32": (C.c_int, [c_f32p, C.c_longlong, C.c_float, C.c_ulonglong, C.c_ulonglong, c_stream]),
    "unetrir_index_to_i32": (C.c_int, [C.c_void_p, C.c_int, C.c_longlong, C.c_void_p, c_stream]),
    "unetrir_reset_tile_tickets": (C.c_int, []),
    "unetrir_bn_bwd_junction_f32": (C.c_int, [c_f32p, C.c_int, c_f32p, C.c_int, c_f32p, C.c_int, C.c_longlong, C.c_int, c_f32p, c_f32p, C.c_int, c_f32p, C.c_int, c_f32p, C.c_int, c_f32p, C.c_int, c_f32p, c_f32p, C.c_void_p, C.c_size_t, c_stream]),
    "unetrir_bn_bwd_junction_bf16": (C.c_int, [c_f32p, C.c_int, c_f32p, C.c_int, c_f32p, C.c_int, C.c_longlong, C.c_int, c_f32p, c_f32p, C.c_int, c_f32p, C.c_int, c_f32p, C.c_int, c_f32p, C.c_int, c_f32p, c_f32p, C.c_void_p, C.c_size_t, c_stream]),
    "unetrir_sigmoid_loss_ex_f32": (C.c_int, [c_f32p, C.c_int, c_f32p, c_f32p, c_f32p, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float,
                                              c_f32p, c_f32p, c_f32p, C.c_void_p, C.c_size_t, c_stream]),
    "unetrir_sigmoid_loss_ex_bf16": (C.c_int, [c_f32p, C.c_int, c_f32p, c_f32p, c_f32p, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float,
                                               c_f32p, c_f32p, c_f32p, C.c_void_p, C.c_size_t, c_stream]),
    "unetrir_relu1_loss_ex_f32": (C.c_int, [c_f32p, C.c_int, c_f32p, c_f32p, c_f32p, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float,
                                            c_f32p, c_f32p, c_f32p, C.c_void_p, C.c_size_t, c_stream]),
    "unetrir_relu1_loss_ex_bf16": (C.c_int, [c_f32p, C.c_int, c_f32p, c_f32p, c_f32p, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float,
                                             c_f32p, c_f32p, c_f32p, C.c_void_p, C.c_size_t, c_stream]),
    "unetrir_relu1_nchw_f32": (C.c_int, [c_f32p, C.c_int, C.c_int, C.c_int, C.c_int, c_f32p, c_stream]),
    "unetrir_relu1_bwd_f32": (C.c_int, [c_f32p, c_f32p, C.c_int, C.c_int, C.c_int, c_f32p, c_stream]),
    "unetrir_relu1_bwd_bf16": (C.c_int, [c_f32p, c_f32p, C.c_int, C.c_int, C.c_int, c_f32p, c_stream]),
    "unetrir_linear_loss_ex_f32": (C.c_int, [c_f32p, C.c_int, c_f32p, c_f32p, c_f32p, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float,
                                             c_f32p, c_f32p, c_f32p, C.c_void_p, C.c_size_t, c_stream]),
    "unetrir_linear_loss_ex_bf16": (C.c_int, [c_f32p, C.c_int, c_f32p, c_f32p, c_f32p, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float,
                                              c_f32p, c_f32p, c_f32p, C.c_void_p, C.c_size_t, c_stream]),
    "unetrir_linear_nchw_f32": (C.c_int, [c_f32p, C.c_int, C.c_int, C.c_int, C.c_int, c_f32p, c_stream]),
    "unetrir_linear_bwd_f32": (C.c_int, [c_f32p, c_f32p, C.c_int, C.c_int, C.c_int, c_f32p, c_stream]),
    "unetrir_linear_bwd_bf16": (C.c_int, [c_f32p, c_f32p, C.c_int, C.c_int, C.c_int, c_f32p, c_stream]),
    # Conv2D(2, (1, 1)) head of DiffUNet on a bf16 trunk (head1x1.hip)
    "unetrir_head1x1_supported": (C.c_int, [C.c_int]),
    "unetrir_head1x1_fwd_bf16": (C.c_int, [c_f32p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, c_f32p, c_f32p, c_f32p, C.c_int, c_stream]),
    "unetrir_head1x1_bwd_ws_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int, C.c_int]),
    "unetrir_head1x1_bwd_bf16": (C.c_int, [c_f32p, C.c_int, c_f32p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, c_f32p, c_f32p, C.c_int,
                                           c_f32p, c_f32p, C.c_void_p, C.c_size_t, c_stream]),
    # UpSampling2D((2, 2)) -> Conv2D(2, (6, 6)) head of the half-resolution U-Net, folded to the coarse grid (head_up2.hip)
    "unetrir_head_up2_supported_f32": (C.c_int, [C.c_int]),
    "unetrir_head_up2_supported_bf16": (C.c_int, [C.c_int]),
    "unetrir_head_up2_fold": (C.c_int, [c_f32p, C.c_int, c_f32p, C.c_int, c_stream]),
    "unetrir_head_up2_fwd_f32": (C.c_int, [c_f32p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, c_f32p, c_f32p, c_f32p, C.c_int, c_stream]),
    "unetrir_head_up2_fwd_bf16": (C.c_int, [c_f32p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, c_f32p, c_f32p, c_f32p, C.c_int, c_stream]),
    "unetrir_head_up2_dgrad_f32": (C.c_int, [c_f32p, C.c_int, C.c_int, C.c_int, C.c_int, c_f32p, C.c_int, c_f32p, C.c_int, c_stream]),
    "unetrir_head_up2_dgrad_bf16": (C.c_int, [c_f32p, C.c_int, C.c_int, C.c_int, C.c_int, c_f32p, C.c_int, c_f32p, C.c_int, c_stream]),
    "unetrir_head_up2_wgrad_ws_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int, C.c_int]),
    "unetrir_head_up2_wgrad_f32": (C.c_int, [c_f32p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, c_f32p, C.c_int, c_f32p, C.c_void_p,
                                             C.c_size_t, c_stream]),
    "unetrir_head_up2_wgrad_bf16": (C.c_int, [c_f32p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, c_f32p, C.c_int, c_f32p, C.c_void_p,
                                              C.c_size_t, c_stream]),
    "unetrir_sgd_f32": (C.c_int, [c_f32p, c_f32p, C.c_longlong, C.c_float, C.c_float, c_stream]),
    "unetrir_nadam_f32": (C.c_int, [c_f32p, c_f32p, c_f32p, c_f32p, C.c_longlong, C.c_float, C.c_float, C.c_float, C.c_float, C.c_float,
                                    C.c_float, C.c_float, C.c_float, c_stream]),
    "unetrir_step_advance": (C.c_int, [C.c_void_p, c_f32p, c_f32p, C.c_int, C.c_int, c_stream]),
    "unetrir_adam_dev_f32": (C.c_int, [c_f32p, c_f32p, c_f32p, c_f32p, C.c_longlong, c_f32p, c_stream]),
    "unetrir_dropout_mask_dev_f32": (C.c_int, [c_f32p, C.c_longlong, C.c_float, C.c_ulonglong, C.c_void_p, C.c_ulonglong, c_stream]),
    "unetrir_normal_f32": (C.c_int, [c_f32p, C.c_longlong, C.c_ulonglong, C.c_ulonglong, c_stream]),
    "unetrir_normal_dev_f32": (C.c_int, [c_f32p, C.c_longlong, C.c_ulonglong, C.c_void_p, C.c_ulonglong, c_stream]),
    "unetrir_vae_sample_kl_fwd_f32": (C.c_int, [c_f32p, C.c_int, c_f32p, C.c_int, c_f32p, C.c_int, C.c_int, C.c_float, c_f32p, C.c_int,
                                                c_f32p, c_stream]),
    "unetrir_vae_sample_kl_bwd_f32": (C.c_int, [c_f32p, C.c_int, c_f32p, C.c_int, c_f32p, c_f32p, C.c_int, C.c_int, C.c_int, C.c_float,
                                                c_f32p, C.c_int, c_f32p, C.c_int, c_stream]),
    "unetrir_vae_loss_add_f32": (C.c_int, [c_f32p, c_f32p, c_stream]),
    "unetrir_vq_ws_bytes": (C.c_size_t, []),
    "unetrir_vq_fwd_f32": (C.c_int, [c_f32p, C.c_longlong, C.c_int, C.c_int, C.c_int, c_f32p, C.c_int, C.c_float, C.c_float, C.c_void_p,
                                     c_f32p, C.c_int, c_f32p, C.c_void_p, C.c_size_t, c_stream]),
    "unetrir_vq_bwd_f32": (C.c_int, [c_f32p, C.c_longlong, C.c_int, C.c_int, C.c_int, C.c_void_p, c_f32p, C.c_int, c_f32p, C.c_int,
                                     C.c_float, C.c_float, c_f32p, C.c_int, c_f32p, c_stream]),
    "unetrir_gather_batch_f32": (C.c_int, [c_f32p, C.c_longlong, C.c_longlong, C.c_void_p, C.c_int, c_f32p, C.c_longlong, C.c_void_p,
                                           C.c_void_p, C.c_void_p, C.c_int, c_f32p, c_f32p, C.c_void_p, c_f32p, C.c_void_p, c_stream]),
    "unetrir_griffinlim_ws_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int, C.c_int]),
    "unetrir_griffinlim_f32": (C.c_int, [c_f32p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                         C.c_int, C.c_int, C.c_float, c_f32p, C.c_ulonglong, C.c_ulonglong, c_f32p, C.c_void_p,
                                         C.c_size_t, c_stream]),
    "unetrir_uniform_f32": (C.c_int, [c_f32p, C.c_longlong, C.c_ulonglong, C.c_ulonglong, c_stream]),
    "unetrir_griffinlim_fft_supported": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    "unetrir_griffinlim_fft_ws_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    "unetrir_griffinlim_fft_f32": (C.c_int, [c_f32p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                             C.c_int, C.c_int, C.c_float, c_f32p, C.c_ulonglong, C.c_ulonglong, c_f32p, C.c_void_p,
                                             C.c_size_t, c_stream]),
    # tfa.optimizers.LAMB (lamb.hip)
    "unetrir_lamb_chunk_elems": (C.c_int, []),
    "unetrir_lamb_table_init": (C.c_longlong, [C.POINTER(LambSeg), C.c_int, C.c_void_p, C.c_longlong]),
    "unetrir_lamb_ws_bytes": (C.c_size_t, [C.c_int, C.c_longlong]),
    "unetrir_lamb_f32": (C.c_int, [c_f32p, c_f32p, c_f32p, c_f32p, C.POINTER(LambSeg), C.c_void_p, C.c_void_p, C.c_int, C.c_longlong,
                                   C.c_longlong, C.c_float, C.c_float, C.c_float, C.c_float, C.c_float, C.c_float, C.c_float, C.c_float,
                                   C.c_void_p, C.c_size_t, c_stream]),
    "unetrir_lamb_dev_f32": (C.c_int, [c_f32p, c_f32p, c_f32p, c_f32p, C.POINTER(LambSeg), C.c_void_p, C.c_void_p, C.c_int, C.c_longlong,
                                       C.c_longlong, C.c_float, C.c_void_p, c_f32p, C.c_void_p, C.c_size_t, c_stream]),
    # the room classifier deep_CNN (cnn_clas.hip): 'valid' 3x3 convolution, average / global pooling, softmax + cross-entropy
    "unetrir_conv3x3_valid_fwd_f32": (C.c_int, [C.POINTER(ConvGeom), c_f32p, C.c_int, c_f32p, c_f32p, C.c_int, c_f32p, C.c_int, c_stream]),
    "unetrir_conv3x3_valid_dgrad_f32": (C.c_int, [C.POINTER(ConvGeom), c_f32p, C.c_int, c_f32p, C.c_int, C.c_int, c_f32p, c_f32p, C.c_int,
                                                  c_stream]),
    "unetrir_conv3x3_valid_wgrad_ws_bytes": (C.c_size_t, [C.POINTER(ConvGeom)]),
    "unetrir_conv3x3_valid_wgrad_f32": (C.c_int, [C.POINTER(ConvGeom), c_f32p, C.c_int, c_f32p, C.c_int, c_f32p, C.c_int, C.c_int, c_f32p,
                                                  c_f32p, C.c_void_p, C.c_size_t, c_stream]),
    "unetrir_avgpool2_fwd_f32": (C.c_int, [c_f32p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, c_f32p, c_f32p, C.c_int, c_stream]),
    "unetrir_avgpool2_bwd_f32": (C.c_int, [c_f32p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, c_f32p, C.c_int, c_stream]),
    "unetrir_gap_fwd_f32": (C.c_int, [c_f32p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, c_f32p, c_f32p, C.c_int, c_stream]),
    "unetrir_gap_bwd_f32": (C.c_int, [c_f32p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, c_f32p, C.c_int, c_stream]),
    "unetrir_softmax_ce_f32": (C.c_int, [c_f32p, C.c_int, c_f32p, C.c_int, C.c_int, C.c_float, c_f32p, c_f32p, C.c_int, c_f32p, c_f32p,
                                         c_stream]),
    "unetrir_softmax_fwd_f32": (C.c_int, [c_f32p, C.c_int, C.c_int, C.c_int, c_f32p, c_stream]),
    "unetrir_softmax_bwd_f32": (C.c_int, [c_f32p, c_f32p, C.c_int, C.c_int, c_f32p, C.c_int, c_stream]),
    "unetrir_prof_enable": (C.c_int, [C.c_int]),
    "unetrir_prof_collect": (C.c_int, [C.POINTER(C.c_int), C.POINTER(C.c_double), C.POINTER(C.c_double)]),
}

EXPORTS = tuple(_SIGS)
PROF_FAMILIES = 8


class UnetrirError(RuntimeError):
    pass


_LIB_PATH = None


def use_library(path):
    """Load another build of the library instead of libunetrir.so (scripts/: the timing-ablation build).  Before first use."""
    global _LIB_PATH
    if _LIB is not None:
        raise UnetrirError("the library is already loaded")
    _LIB_PATH = path


def lib():
    """Load (building first if the sources are newer) libunetrir.so.  Raises if it cannot."""
    global _LIB
    if _LIB is not None:
        return _LIB
    path = _LIB_PATH or _build.LIB
    if _LIB_PATH is None and _build.needs_build():
        path = _build.build()
    if not os.path.exists(path):
        raise UnetrirError(f"HIP extension missing: {path}")
    L = C.CDLL(path)
    for name, (res, args) in _SIGS.items():
        fn = getattr(L, name)      # AttributeError if the export is missing: fail loudly
        fn.restype = res
        fn.argtypes = args
    if L.unetrir_abi_version() != 1:
        raise UnetrirError("libunetrir.so ABI version mismatch")
    _LIB = L
    return L


def check(err, what):
    if err != 0:
        raise UnetrirError(f"{what} failed with code {err}")
