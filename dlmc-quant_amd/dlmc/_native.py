"""ctypes binding of the C ABI in include/dlmcq.h (libdlmcq.so, built by csrc/Makefile).

There is NO fallback: if the shared library is missing or a symbol is absent the import fails,
and every call on a non-GPU tensor raises.  The product path is the HIP path or nothing.
"""
import ctypes
import os

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
import sys

_PRODUCT = os.path.join(os.path.dirname(_HERE), "libdlmcq.so")
# Another build of the library (same-box A/B timing, the lab library of tools/) is loaded ONLY when the caller names it AND
# declares itself a lab tool (DLMCQ_LAB_TOOLS=1; tools/*.py and tools/*.sh set both), and the path is printed: a stale
# DLMCQ_LIBRARY in a user's environment does not swap the product library silently - it is reported and ignored.
_OVERRIDE = os.environ.get("DLMCQ_LIBRARY")
LAB_OVERRIDE = bool(_OVERRIDE) and os.environ.get("DLMCQ_LAB_TOOLS") == "1"
if _OVERRIDE and not LAB_OVERRIDE:
    print(f"[dlmc] DLMCQ_LIBRARY={_OVERRIDE} ignored (set DLMCQ_LAB_TOOLS=1 to load a lab / A-B build); loading {_PRODUCT}", file=sys.stderr)
LIB_PATH = _OVERRIDE if LAB_OVERRIDE else _PRODUCT
if LAB_OVERRIDE:
    print(f"[dlmc] lab override: loading {LIB_PATH} instead of the product library", file=sys.stderr)

# enums of include/dlmcq.h
FORM_EMULATE, FORM_QBASE, FORM_ZEROPOINT, FORM_SYMMETRIC, FORM_ROOTQ_ACT = range(5)
EMIT_SHIFT128 = 0x100    # DLMCQ_EMIT_SHIFT128: OR-able into q_form (include/dlmcq.h)
W2_CHUNK_MAJOR = 0x200   # DLMCQ_W2_CHUNK_MAJOR: OR-able into the chain entry points' last quantiser form
FORCE_TILED = 0x400      # DLMCQ_FORCE_TILED: OR-able into q_form of conv2d_i8_nhwc_fused / _asym / _dual / conv2d_dw_i8_nhwc: the family's generic kernel
ROUTE_ONLY = 0x800       # DLMCQ_ROUTE_ONLY: launch nothing, return which kernel the dispatch picks (ROUTE_*)
FP32_IN_CHUNK_MAJOR = 0x2000   # DLMCQ_FP32_IN_CHUNK_MAJOR: a chain call's fp32 shortcut is [K / 64][M][64] (kernels.ChunkMajor)
FP32_OUT_CHUNK_MAJOR = 0x4000  # DLMCQ_FP32_OUT_CHUNK_MAJOR: ... and / or its fp32 block output
PAD_CODE0 = 0x8000       # DLMCQ_PAD_CODE0: quantize_pad_nhwc4's border holds code 0 (a float-offset quantiser's padding)
PIPELINED = 0x1000       # DLMCQ_PIPELINED (opt-in): the persistent, software-pipelined halo-tile 3x3 kernel where it applies
ROUTE_VARIANT = 0x10000  # DLMCQ_ROUTE_VARIANT: with ROUTE_ONLY, a ROUTE_TILED answer names the tiled kernel's instantiation instead (decode_variant)
ROUTE_VARIANT_TAG = 1 << 24
ROUTE_HALO_VARIANT = 0x20000  # DLMCQ_ROUTE_HALO_VARIANT: with ROUTE_ONLY, a ROUTE_HALO3X3 / ROUTE_HALO3X3_PIPE answer names the instantiation instead (decode_halo_variant)
ROUTE_HALO_VARIANT_TAG, ROUTE_PIPE_VARIANT_TAG = 1 << 25, 1 << 26
HV_PLAIN, HV_XS, HV_S2 = 1, 2, 4   # the flags of such an answer (include/dlmcq.h)
ROUTE_HALO_ROWS = 0x200000  # DLMCQ_ROUTE_HALO_ROWS: with ROUTE_ONLY | ROUTE_HALO_VARIANT, a halo answer also carries HV_DENSE when the launch's rows are real pixels only
HV_DENSE = 8
ROUTE_DW_VARIANT = 0x40000  # DLMCQ_ROUTE_DW_VARIANT: with ROUTE_ONLY, a ROUTE_DW / ROUTE_DWM answer of the depthwise entry points names the instantiation instead (decode_dw_variant)
ROUTE_DW_VARIANT_TAG, ROUTE_DWM_VARIANT_TAG = 1 << 27, 1 << 28
ROUTE_CHAIN_VARIANT = 0x80000  # DLMCQ_ROUTE_CHAIN_VARIANT: with ROUTE_ONLY, in the chain entry points' last form: which conv_chain_i8_kernel instantiation, tile height and layouts (decode_chain_variant)
ROUTE_CHAIN_VARIANT_TAG = 1 << 30
CHAIN_FL = (3, 1, -1)              # the FL slot of such an answer -> the first epilogue's compile-time form (csrc/conv_chain_i8.hip)
DV_R6, DV_XOFF, DV_XS = 1, 2, 2    # the flags of such an answer: R6 in both, XOFF in a DW_TABLE answer, XS in a DWM_TABLE one (include/dlmcq.h)
DW_FAMILIES = ("p2", "dw3", "generic")   # conv_dw3p2_i8_kernel, conv_dw3_i8_kernel, conv_dw_i8_kernel: the family field of a DW_TABLE answer
# the `flags` of a ROUTE_VARIANT answer: conv_i8_mfma_kernel's boolean template parameters (include/dlmcq.h)
CV_DUAL, CV_ADIR, CV_ASYM, CV_SWAP, CV_R6, CV_XOFF, CV_NARROW, CV_PADRES = 1, 2, 4, 8, 16, 32, 64, 128
ROUTE_TILED, ROUTE_HALO3X3, ROUTE_PW, ROUTE_PWR, ROUTE_DW, ROUTE_DWM, ROUTE_HALO3X3_PIPE, ROUTE_GAP = 1, 2, 3, 4, 5, 6, 7, 8
ROUTE_TAG = {ROUTE_TILED: "conv_i8", ROUTE_HALO3X3: "conv3x3_halo", ROUTE_PW: "conv_pw", ROUTE_PWR: "conv_pwr", ROUTE_DW: "conv_dw",
             ROUTE_DWM: "conv_dwm", ROUTE_HALO3X3_PIPE: "conv3x3_pipe", ROUTE_GAP: "conv_gap"}     # the profile tag (bench.py's kernel families) of each route
ACT_NONE, ACT_RELU, ACT_RELU6 = 0, 1, 2   # DLMCQ_ACT_*: the `relu` argument of the fused convolution entry points
SQUEEZE_NONE, SQUEEZE_RELU, SQUEEZE_SWISH = 0, 1, 2   # DLMCQ_SQUEEZE_*: dlmcq_squeeze_gate_i8's activation between its two layers
GATE_NONE, GATE_SIGMOID, GATE_HARDSIGMOID = 0, 1, 2   # DLMCQ_GATE_*: ... and its gate function
HSWISH_MUL_FIRST, HSWISH_GATE_FIRST = 0, 1   # DLMCQ_HSWISH_*: dlmcq_hardswish_nhwc_f32's order of the two multiplies
SQUEEZE_MAX_C, SQUEEZE_MAX_R, SQUEEZE_IMAGES = 2048, 512, 4  # DLMCQ_SQUEEZE_MAX_C / _MAX_R / _IMAGES
Y_DEQUANT, Y_CODES = 0, 1
CODES_NONE, CODES_I8, CODES_P4 = 0, 1, 2
MINMAX_ABSMAX, MINMAX_MINMAX, MINMAX_NEGMIN = 0, 1, 2

_p, _i64, _i32, _f32, _sz = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32, ctypes.c_float, ctypes.c_size_t

# symbol -> (restype, argtypes); must list every function include/dlmcq.h declares
SIGNATURES = {
    "dlmcq_version": (ctypes.c_int, []),
    "dlmcq_strerror": (ctypes.c_char_p, [ctypes.c_int]),
    "dlmcq_fake_quant_f32": (ctypes.c_int, [_p, _p, _p, _p, _p, _i64, _i64, _i64, _i32, _i32, _i32, _i32, _i32, _f32, _p]),
    "dlmcq_dequant_codes_f32": (ctypes.c_int, [_p, _p, _p, _p, _i64, _i64, _i64, _i32, _i32, _i32, _f32, _p]),
    "dlmcq_dequant_f32": (ctypes.c_int, [_p, _p, _p, _p, _i64, _i64, _i64, _p]),
    "dlmcq_minmax_scratch_bytes": (_sz, [_i64, _i64, _i64]),
    "dlmcq_minmax_f32": (ctypes.c_int, [_p, _p, _p, _i64, _i64, _i64, _i32, _p, _sz, _p]),
    "dlmcq_minmax_finalize_f32": (ctypes.c_int, [_p, _i64, _i64, _p, _p, _i32, _p]),
    "dlmcq_conv2d_i8_observed_partials": (_sz, [_i64, _i64]),
    "dlmcq_conv2d_i8_nhwc_fused_observed": (ctypes.c_int, [_p, _p, _p, _p, _p, _p, _p, _p, _i64, _i64, _i64, _i64, _i64, _i64, _i64, _i32, _i32,
                                                            _i32, _i32, _p, _i32, _p, _p, _p, _i32, _i32, _i32, _f32, _p, _i64, _p, _p]),
    "dlmcq_qparams_from_minmax": (ctypes.c_int, [_p, _p, _p, _p, _i64, _i32, _i32, _i32, _i32, _f32, _p]),
    "dlmcq_span_scale_f32": (ctypes.c_int, [_p, _p, _p, _i64, _f32, _i32, _p]),
    "dlmcq_lsq_init_scratch_bytes": (_sz, [_i64]),
    "dlmcq_lsq_init_f32": (ctypes.c_int, [_p, _p, _i64, _f32, _p, _sz, _p]),
    "dlmcq_observe_qparams_f32": (ctypes.c_int, [_p, _p, _p, _i64, _i64, _i64, _i32, _i32, _i32, _f32, _p, _sz, _p]),
    "dlmcq_pack_int4": (ctypes.c_int, [_p, _p, _i64, _p]),
    "dlmcq_unpack_int4": (ctypes.c_int, [_p, _p, _i64, _i32, _p]),
    "dlmcq_fq_bwd_scratch_bytes": (_sz, [_i64, _i64, _i64]),
    "dlmcq_fake_quant_bwd_f32": (ctypes.c_int, [_p, _p, _p, _p, _p, _p, _i64, _i64, _i64, _i32, _i32, _f32, _p, _sz, _p]),
    "dlmcq_rootq_bwd_scratch_bytes": (ctypes.c_size_t, [_i64]),
    "dlmcq_rootq_weight_bwd_f32": (ctypes.c_int, [_p, _p, _p, _p, _p, _p, _i64, _i32, _i32, _p, _sz, _p]),
    "dlmcq_fake_quant_bwd_form_f32": (ctypes.c_int, [_p, _p, _p, _p, _p, _p, _i64, _i64, _i64, _i32, _i32, _i32, _f32, _p, _sz, _p]),
    "dlmcq_fq_segment_bytes": (_sz, []),
    "dlmcq_fq_multi_prepare": (ctypes.c_int, [_p, _i64, _p, _p, _p, _p]),
    "dlmcq_fake_quant_multi_f32": (ctypes.c_int, [_p, _i64, _i64, _p]),
    "dlmcq_fake_quant_multi_bwd_f32": (ctypes.c_int, [_p, _i64, _i64, _i64, _p, _sz, _p]),
    "dlmcq_rootq_weight_f32": (ctypes.c_int, [_p, _p, _p, _i64, _i32, _i32, _p]),
    "dlmcq_l2norm_scratch_bytes": (_sz, [_i64, _i64, _i64]),
    "dlmcq_l2norm_step_f32": (ctypes.c_int, [_p, _p, _p, _p, _i64, _i64, _i64, _i32, _i32, _p, _sz, _p]),
    "dlmcq_l2norm_iterate_f32": (ctypes.c_int, [_p, _p, _p, _p, _i64, _i64, _i64, _i32, _i32, _i32, _f32, _p, _sz, _p]),
    "dlmcq_l2out_scratch_bytes": (_sz, [_i64, _i64, _i64]),
    "dlmcq_l2out_update_f32": (ctypes.c_int, [_p, _p, _p, _p, _p, _i64, _i64, _i64, _i32, _f32, _f32, _p, _sz, _p]),
    "dlmcq_l2loss_scratch_bytes": (_sz, [_i64]),
    "dlmcq_l2loss_tensor_f32": (ctypes.c_int, [_p, _p, _p, _p, _p, _i64, _i32, _f32, _p, _sz, _p]),
    "dlmcq_l2loss_rows_f32": (ctypes.c_int, [_p, _p, _p, _i64, _i64, _i32, _p]),
    "dlmcq_adaround_weight_f32": (ctypes.c_int, [_p, _p, _p, _p, _i64, _i64, _i32, _i32, _i32, _p]),
    "dlmcq_adaround_weight_bwd_f32": (ctypes.c_int, [_p, _p, _p, _p, _p, _p, _i64, _i64, _i32, _i32, _p]),
    "dlmcq_quantize_weight_krsc_i8": (ctypes.c_int, [_p, _p, _p, _p, _i64, _i64, _i64, _i64, _i32, _i32, _p]),
    "dlmcq_conv2d_i8_nhwc_f32": (ctypes.c_int, [_p, _p, _p, _p, _p, _p, _p, _p, _i64, _i64, _i64, _i64, _i64, _i64, _i64,
                                               _i32, _i32, _i32, _i32, _p]),
    "dlmcq_conv2d_i8_nhwc_fused": (ctypes.c_int, [_p, _p, _p, _p, _p, _p, _p, _p, _i64, _i64, _i64, _i64, _i64, _i64, _i64,
                                                 _i32, _i32, _i32, _i32, _p, _i32, _p, _p, _p, _i32, _i32, _i32, _f32, _p]),
    "dlmcq_conv2d_i8_nhwc_asym": (ctypes.c_int, [_p, _p, _p, _p, _p, _p, _p, _p, _p, _i64, _i64, _i64, _i64, _i64, _i64, _i64,
                                                _i32, _i32, _i32, _i32, _p, _i32, _p, _p, _p, _i32, _i32, _i32, _f32, _p]),
    "dlmcq_conv2d_i8_nhwc_narrow": (ctypes.c_int, [_p, _p, _p, _p, _p, _p, _p, _p, _p, _i64, _i64, _i64, _i64, _i64, _i64, _i64,
                                                  _i32, _i32, _i32, _i32, _p, _i32, _p, _p, _p, _i32, _i32, _i32, _f32, _i64, _p]),
    "dlmcq_conv2d_i8_nhwc_padres": (ctypes.c_int, [_p, _p, _p, _p, _p, _p, _p, _p, _p, _i64, _i64, _i64, _i64, _i64, _i64, _i64,
                                                  _i32, _i32, _i32, _i32, _p, _i64, _i64, _i64, _i32, _i64, _i32, _p, _p, _p, _i32, _i32, _i32,
                                                  _f32, _i64, _p]),
    "dlmcq_conv2d_dw_i8_nhwc": (ctypes.c_int, [_p, _p, _p, _p, _p, _p, _p, _p, _i64, _i64, _i64, _i64, _i64, _i64, _i32, _i32, _i32,
                                              _i32, _p, _p, _p, _i32, _i32, _i32, _f32, _p]),
    "dlmcq_conv2d_dw5_i8_nhwc": (ctypes.c_int, [_p, _p, _p, _p, _p, _p, _p, _p, _i64, _i64, _i64, _i64, _i32, _i32, _i32,
                                               _i32, _p, _p, _p, _i32, _i32, _i32, _f32, _p]),
    "dlmcq_conv2d_i8_nhwc_xoff": (ctypes.c_int, [_p, _p, _p, _p, _p, _p, _p, _p, _p, _i64, _i64, _i64, _i64, _i64, _i64, _i64,
                                                _i32, _i32, _i32, _i32, _p, _i32, _p, _p, _p, _i32, _i32, _i32, _f32, _p, _p, _p]),
    "dlmcq_conv2d_dw_i8_nhwc_xoff": (ctypes.c_int, [_p, _p, _p, _p, _p, _p, _p, _p, _i64, _i64, _i64, _i64, _i64, _i64, _i32, _i32, _i32,
                                                   _i32, _p, _p, _p, _i32, _i32, _i32, _f32, _p, _p, _p]),
    "dlmcq_conv2d_i8_stem_xoff": (ctypes.c_int, [_p, _p, _p, _p, _p, _p, _p, _p, _p, _i64, _i64, _i64, _i64, _i64, _i64, _i64, _i32, _i32,
                                                _i32, _i32, _p, _p, _p, _i32, _i32, _i32, _f32, _p, _p, _p]),
    "dlmcq_dwpw_pack_table": (ctypes.c_int, [_p, _p, _p, _p, _p, _p, _i64, _i32, _p, _p]),
    "dlmcq_conv2d_dwpw_i8_nhwc": (ctypes.c_int, [_p, _p, _i32, _i32, _i32, _p, _i64, _i64, _i64, _i64, _i32, _p, _p, _i32, _i32, _i32, _f32,
                                                _p, _p, _p, _p, _p, _p, _i64, _i32, _p, _p, _p, _i32, _i32, _i32, _f32, _p]),
    "dlmcq_conv2d_i8_nhwc_dual": (ctypes.c_int, [_p, _p, _p, _p, _p, _p, _p, _p, _i64, _i64, _i64, _i64, _i64, _i64, _i64,
                                                _i32, _i32, _i32, _i32,
                                                _p, _p, _p, _p, _p, _p, _p, _i64, _i64, _i64, _i64, _i64, _i32, _i32, _i32, _i32,
                                                _i32, _p, _p, _p, _i32, _i32, _i32, _f32, _p]),
    "dlmcq_conv2d_i8_nhwc_chain": (ctypes.c_int, [_p, _p, _p, _p, _p, _p, _p, _p, _i64, _i64, _i64, _i32, _p, _i32, _p, _p, _p, _i32,
                                                 _i32, _i32, _f32, _p, _p, _p, _p, _i64, _i32, _p, _p, _p, _i32, _i32, _i32, _f32,
                                                 _i32, _p]),
    "dlmcq_conv2d_i8_nhwc_dual_chain": (ctypes.c_int, [_p, _p, _p, _p, _p, _p, _p, _p, _i64, _i64, _i64, _i64, _i64, _i32,
                                                      _p, _p, _p, _p, _p, _p, _p, _i64, _i64, _i64, _i32, _i32,
                                                      _i32, _p, _p, _p, _i32, _i32, _i32, _f32,
                                                      _p, _p, _p, _p, _i64, _i32, _p, _p, _p, _i32, _i32, _i32, _f32, _i32, _p]),
    "dlmcq_conv2d_i8_nhwc_recompute_chain": (ctypes.c_int, [_p, _p, _p, _p, _p, _p, _p, _p, _i64, _i64, _i64, _i64, _i64, _i32,
                                                           _p, _p, _p, _p, _p, _p, _p, _i64, _i32,
                                                           _p, _p, _p, _p, _p, _p, _p, _i64, _i64, _i64, _i32, _i32,
                                                           _i32, _i32, _p, _p, _p, _i32, _i32, _i32, _f32,
                                                           _p, _p, _p, _p, _i64, _i32, _p, _p, _p, _i32, _i32, _i32, _f32, _i32, _p]),
    "dlmcq_quantize_pad_nhwc4": (ctypes.c_int, [_p, _p, _p, _p, _i64, _i64, _i64, _i64, _i64, _i64, _i64, _i64, _i32, _i32, _i32,
                                               _i32, _f32, _p]),
    "dlmcq_quantize_weight_stem_i8": (ctypes.c_int, [_p, _p, _p, _p, _i64, _i64, _i64, _i64, _i32, _i32, _p]),
    "dlmcq_conv2d_i8_stem_fused": (ctypes.c_int, [_p, _p, _p, _p, _p, _p, _p, _p, _i64, _i64, _i64, _i64, _i64, _i64, _i32, _i32,
                                                 _i32, _p, _p, _p, _i32, _i32, _i32, _f32, _p]),
    "dlmcq_conv2d_i8_stem_asym": (ctypes.c_int, [_p, _p, _p, _p, _p, _p, _p, _p, _p, _i64, _i64, _i64, _i64, _i64, _i64, _i64, _i32, _i32,
                                                _i32, _p, _p, _p, _i32, _i32, _i32, _f32, _p]),
    "dlmcq_conv2d_i8_stem_pool_fused": (ctypes.c_int, [_p, _p, _p, _p, _p, _p, _p, _p, _i64, _i64, _i64, _i64, _i64, _i64, _i32, _i32,
                                                      _i32, _p, _p, _p, _i32, _i32, _i32, _f32, _p]),
    "dlmcq_maxpool_codes_nhwc": (ctypes.c_int, [_p, _p, _i64, _i64, _i64, _i64, _i32, _i32, _i32, _i32, _p]),
    "dlmcq_gap_nhwc_f32": (ctypes.c_int, [_p, _p, _p, _i64, _i64, _i64, _p, _p, _i32, _i32, _i32, _f32, _p]),
    "dlmcq_avgpool_nhwc_f32": (ctypes.c_int, [_p, _p, _p, _i64, _i64, _i64, _i64, _i64, _i64, _i64, _i32, _p, _p, _i32, _i32, _i32, _f32, _p]),
    "dlmcq_gate_nhwc_f32": (ctypes.c_int, [_p, _p, _p, _p, _i64, _i64, _i64, _i64, _i64, _i64, _i32, _i32, _p, _p, _i32, _i32, _i32, _f32, _p]),
    "dlmcq_swish_nhwc_f32": (ctypes.c_int, [_p, _p, _p, _i64, _i64, _i64, _i64, _i64, _i64, _i32, _p, _p, _i32, _i32, _i32, _f32, _p]),
    "dlmcq_hardswish_nhwc_f32": (ctypes.c_int, [_p, _p, _p, _i64, _i64, _i64, _i64, _i64, _i64, _i32, _p, _p, _i32, _i32, _i32, _f32, _i32, _p]),
    "dlmcq_squeeze_gate_i8": (ctypes.c_int, [_p] * 7 + [_i32] + [_p] * 4 + [_i32, _p, _p, _i64, _i64, _i64, _i32, _p, _p, _i32, _i32, _i32, _f32, _p]),
    "dlmcq_gelu_nhwc_f32": (ctypes.c_int, [_p, _p, _p, _i64, _i64, _i64, _i64, _i64, _i64, _i32, _p, _p, _i32, _i32, _i32, _f32, _p]),
    "dlmcq_layernorm_rows_f32": (ctypes.c_int, [_p, _p, _p, _p, _p, _i64, _i64, _f32, _p, _p, _i32, _i32, _i32, _f32, _p]),
    "dlmcq_attention_f32": (ctypes.c_int, [_p, _p, _p, _p, _p] + [_i64] * 17 + [_f32, _p, _p, _i32, _i32, _i32, _f32, _p]),
    "dlmcq_patch_rows_f32": (ctypes.c_int, [_p, _p, _p] + [_i64] * 8 + [_p, _p, _i32, _i32, _i32, _f32, _p]),
    "dlmcq_tokens_assemble_f32": (ctypes.c_int, [_p, _p, _p, _p] + [_i64] * 6 + [_p]),
    "dlmcq_conv2d_i8_nhwc_gap": (ctypes.c_int, [_p, _p, _p, _p, _p, _p, _p, _p, _i64, _i64, _i64, _i64, _i64, _i32, _p, _i32, _p, _p, _p,
                                               _i32, _i32, _i32, _f32, _p]),
    "dlmcq_fold_bn_f32": (ctypes.c_int, [_p, _p, _p, _p, _p, _p, _i64, _i64, _f32, _p]),
    "dlmcq_repvgg_fuse_f32": (ctypes.c_int, [_p, _p, _p, _p, _p, _p, _p, _f32, _f32, _f32, _i64, _i64, _p]),
}


class FqSegment(ctypes.Structure):
    """dlmcq_fq_segment of include/dlmcq.h: 17 fields of 8 bytes (checked against dlmcq_fq_segment_bytes() on load)."""
    _fields_ = [("x", _p), ("y", _p), ("gy", _p), ("gx", _p), ("scale", _p), ("offset", _p), ("gscale", _p),
                ("n", _i64), ("channels", _i64), ("inner", _i64), ("lo", _i64), ("hi", _i64), ("ste_g", ctypes.c_double),
                ("form", _i64), ("fwd_chunk0", _i64), ("bwd_wg0", _i64), ("part0", _i64)]


FQ_MULTI_MAX_ELEMENTS = 8192 * 1024      # a segment's cap: 8192 backward chunks of 1024 elements (include/dlmcq.h)


def _load():
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} not found: build it with `make -C dlmc-quant_amd/csrc` (or "
            "`python -c 'import __graft_entry__ as g; g.build()'`).  There is no CPU fallback.")
    # torch ships its own libamdhip64 (soname libamdhip64.so.7); load it first so that libdlmcq's
    # DT_NEEDED resolves to the SAME runtime instance torch uses (pointers and streams are shared).
    tlib = os.path.join(os.path.dirname(torch.__file__), "lib", "libamdhip64.so")
    if os.path.exists(tlib):
        ctypes.CDLL(tlib, mode=ctypes.RTLD_GLOBAL)
    lib = ctypes.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        try:
            fn = getattr(lib, name)  # AttributeError if the library lacks a declared symbol
        except AttributeError:
            if LAB_OVERRIDE:   # an older build named for an A/B run: calls to what it lacks fail there
                continue
            raise
        fn.restype, fn.argtypes = res, args
    if hasattr(lib, "dlmcq_fq_segment_bytes") and lib.dlmcq_fq_segment_bytes() != ctypes.sizeof(FqSegment):
        raise ImportError(f"{LIB_PATH}: dlmcq_fq_segment is {lib.dlmcq_fq_segment_bytes()} bytes, the ctypes mirror {ctypes.sizeof(FqSegment)}")
    return lib


lib = _load()


def experimental(name, argtypes):
    """A symbol exported by the library but deliberately absent from include/dlmcq.h (tests / tuning only)."""
    fn = getattr(lib, name)
    fn.restype, fn.argtypes = ctypes.c_int, argtypes
    return fn


class DlmcqError(RuntimeError):
    pass


def check(rc):
    if rc != 0:
        raise DlmcqError(f"{lib.dlmcq_strerror(rc).decode()} (code {rc})")


def route(rc):
    """Return value of an entry point called with ROUTE_ONLY: the route (> 0), or an error like any other call."""
    if rc <= 0:
        raise DlmcqError(f"{lib.dlmcq_strerror(rc).decode()} (code {rc})" if rc < 0 else "route query returned DLMCQ_OK (an empty problem)")
    return rc


def decode_variant(rc):
    """Answer of a ROUTE_ONLY | ROUTE_VARIANT call -> (tile width, flags) of the conv_i8_mfma_kernel instantiation, or None when the
    answer is no variant (another kernel's ROUTE_*, DLMCQ_OK, a refusal)."""
    if rc < ROUTE_VARIANT_TAG or rc >> 25:
        return None
    return (rc >> 8) & 0xffff, rc & 0xff


def conv_variant_table():
    """[(tile width, flags)]: the instantiations of conv_i8_mfma_kernel the library holds, as its own launcher lists them."""
    fn = experimental("dlmcq_x_conv_variant_table", [ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_uint32), ctypes.c_int])
    n = fn(None, None, 0)
    bn, flags = (ctypes.c_int32 * n)(), (ctypes.c_uint32 * n)()
    assert fn(bn, flags, n) == n
    return [(int(b), int(f)) for b, f in zip(bn, flags)]


def decode_halo_variant(rc):
    """Answer of a ROUTE_ONLY | ROUTE_HALO_VARIANT call -> ("halo", column width, stride 2, halo pieces per buffer, halo buffers, XS, PLAIN) of the
    conv3x3_halo_i8_kernel instantiation, ("pipe", chunks, XS) of the conv3x3_pipe_i8_kernel one, or None when the answer is neither (another
    kernel's ROUTE_*, a tiled variant, DLMCQ_OK, a refusal)."""
    if rc >> 27 or rc < ROUTE_HALO_VARIANT_TAG:
        return None
    if rc & ROUTE_PIPE_VARIANT_TAG:
        return None if rc & ROUTE_HALO_VARIANT_TAG else ("pipe", (rc >> 8) & 0xff, bool(rc & HV_XS))
    return ("halo", (rc >> 16) & 0x1ff, bool(rc & HV_S2), (rc >> 8) & 0xff, (rc >> 4) & 0xf, bool(rc & HV_XS), bool(rc & HV_PLAIN))


def conv3x3_variant_tables():
    """(halo records, pipe records), decoded: the instantiations of the two 3x3 kernels the library holds, as its own launchers list them."""
    fn = experimental("dlmcq_x_conv3x3_variant_table", [ctypes.c_int, ctypes.POINTER(ctypes.c_int32), ctypes.c_int])
    out = []
    for which in (0, 1):
        n = fn(which, None, 0)
        answers = (ctypes.c_int32 * n)()
        assert fn(which, answers, n) == n
        out.append([decode_halo_variant(int(a)) for a in answers])
    return tuple(out)


def decode_dw_variant(rc):
    """Answer of a ROUTE_ONLY | ROUTE_DW_VARIANT call of a depthwise entry point -> ("dw", family ("p2" / "dw3" / "generic"), FAST, R6, XOFF) of the
    csrc/conv_dw_i8.hip instantiation, ("dwm", halo pieces per wave, XS, R6) of the conv_dwm_i8_kernel one, or None when the answer is neither
    (a ROUTE_*, another kernel's variant, DLMCQ_OK, a refusal)."""
    if rc >> 29 or rc < ROUTE_DW_VARIANT_TAG:
        return None
    if rc & ROUTE_DWM_VARIANT_TAG:
        return None if rc & ROUTE_DW_VARIANT_TAG else ("dwm", (rc >> 8) & 0xff, bool(rc & DV_XS), bool(rc & DV_R6))
    family = (rc >> 8) & 0xff
    return None if family >= len(DW_FAMILIES) else ("dw", DW_FAMILIES[family], (rc >> 4) & 0xf, bool(rc & DV_R6), bool(rc & DV_XOFF))


ROUTE_DW5_VARIANT_TAG = 1 << 29      # DLMCQ_ROUTE_DW5_VARIANT_TAG: dlmcq_conv2d_dw5_i8_nhwc's answer to ROUTE_ONLY | ROUTE_DW_VARIANT


def decode_dw5_variant(rc):
    """Answer of a ROUTE_ONLY | ROUTE_DW_VARIANT call of dlmcq_conv2d_dw5_i8_nhwc -> ("dw5", FAST, R6) of the conv_dw5_i8_kernel
    instantiation, or None when the answer is none (DLMCQ_OK, a refusal, another entry point's answer)."""
    if rc < ROUTE_DW5_VARIANT_TAG or rc >> 30 or rc & ~(ROUTE_DW5_VARIANT_TAG | 0x31) or (rc >> 4) & 3 == 3:
        return None
    return ("dw5", (rc >> 4) & 3, bool(rc & DV_R6))


def dw5_variant_table():
    """The conv_dw5_i8_kernel instantiations the library holds, decoded, as its own launcher lists them (csrc/conv_dw5_i8.hip: DW5_TABLE)."""
    fn = experimental("dlmcq_x_dw5_variant_table", [ctypes.POINTER(ctypes.c_int32), ctypes.c_int])
    n = fn(None, 0)
    answers = (ctypes.c_int32 * n)()
    assert fn(answers, n) == n
    return [decode_dw5_variant(int(a)) for a in answers]


def dw_variant_tables():
    """(DW_TABLE records, DWM_TABLE records), decoded: the depthwise instantiations the library holds, as its own launchers list them."""
    fn = experimental("dlmcq_x_dw_variant_table", [ctypes.c_int, ctypes.POINTER(ctypes.c_int32), ctypes.c_int])
    out = []
    for which in (0, 1):
        n = fn(which, None, 0)
        answers = (ctypes.c_int32 * n)()
        assert fn(which, answers, n) == n
        out.append([decode_dw_variant(int(a)) for a in answers])
    return tuple(out)


def decode_chain_variant(rc):
    """Answer of a ROUTE_ONLY | ROUTE_CHAIN_VARIANT call of a chain entry point -> ("chain", table row, FL (3 / 1 / -1), rows per tile, icm, ocm) -
    the conv_chain_i8_kernel instantiation the call launches (row: its index in chain_variant_table()), the tile height and the resolved
    layouts of the fp32 shortcut read / block output written - or None when the answer is none (DLMCQ_OK, a refusal, another entry point's)."""
    if rc < ROUTE_CHAIN_VARIANT_TAG or rc & 0x3ff0c80c or (rc >> 12) & 3 == 3:
        return None
    return ("chain", (rc >> 16) & 0xf, CHAIN_FL[(rc >> 12) & 3], (rc >> 4) & 0x7f, bool(rc & 1), bool(rc & 2))


def chain_variant_table():
    """[(C1, KB, C2, CA, CB, (FL, ...))]: the rows of the chain launcher's table (csrc/conv_chain_i8.hip: CHAIN_TABLE) in its order, each with
    the first-epilogue forms it holds a kernel for."""
    fn = experimental("dlmcq_x_chain_variant_table", [ctypes.POINTER(ctypes.c_int32), ctypes.c_int])
    n = fn(None, 0)
    rows = (ctypes.c_int32 * (6 * n))()
    assert fn(rows, n) == n
    return [tuple(int(v) for v in rows[6 * i:6 * i + 5]) + (tuple(f for b, f in enumerate(CHAIN_FL) if rows[6 * i + 5] >> b & 1),) for i in range(n)]


ROUTE_PW_VARIANT = 0x100000  # DLMCQ_ROUTE_PW_VARIANT: with ROUTE_ONLY, a ROUTE_PW / ROUTE_PWR answer names the instantiation instead (decode_pw_variant); the first-layer entry points answer theirs (decode_stem_variant)
ROUTE_STEM_VARIANT_TAG, ROUTE_PW_VARIANT_TAG, ROUTE_PWR_VARIANT_TAG = 1 << 21, 1 << 22, 1 << 23
STEM_KERNELS = ("stem", "pool", "pool7")   # conv_stem_i8_kernel, conv_stem_pool_i8_kernel, conv_stem_pool7_i8_kernel: the kernel field of a first-layer answer


def decode_stem_variant(rc):
    """Answer of a ROUTE_ONLY | ROUTE_PW_VARIANT call of a first-layer entry point -> ("stem", R, ASYM, SWAP, R6, XOFF) of the conv_stem_i8_kernel
    instantiation, ("pool", R) of the conv_stem_pool_i8_kernel one, ("pool7", XS) of the conv_stem_pool7_i8_kernel one, or None when the answer
    is none (DLMCQ_OK, a refusal, another entry point's answer)."""
    if rc < ROUTE_STEM_VARIANT_TAG or rc >> 22 or rc & 0x1fc000 or rc & 0xf80:
        return None
    kernel, r, flags = (rc >> 12) & 3, (rc >> 4) & 7, rc & 15
    if kernel == 0:
        return ("stem", r, bool(flags & 2), bool(flags & 4), bool(flags & 1), bool(flags & 8)) if 1 <= r <= 7 else None
    if kernel == 1:
        return ("pool", r) if 1 <= r <= 7 and not flags else None
    return ("pool7", bool(flags & 1)) if kernel == 2 and r == 0 and flags < 2 else None


def decode_pw_variant(rc):
    """Answer of a ROUTE_ONLY | ROUTE_PW_VARIANT call of the tiled entry points -> ("pw", input channels, slice width, ASYM, R6) of the
    conv_pw_i8_kernel instantiation, ("pwr", C, fp32 output, codes, dual form, SWP) of the conv_pwr_i8_kernel one, or None when the answer is
    neither (a ROUTE_*, another kernel's variant, DLMCQ_OK, a refusal)."""
    if rc < ROUTE_PW_VARIANT_TAG or rc >> 24:
        return None
    if rc & ROUTE_PWR_VARIANT_TAG:
        if rc & ROUTE_PW_VARIANT_TAG or rc & 0x3fffc0:
            return None
        return ("pwr", 256 * ((rc >> 4) & 3), bool(rc & 2), bool(rc & 1), bool(rc & 4), bool(rc & 8))
    if rc & 0x3fe00c:
        return None
    return ("pw", 64 * ((rc >> 8) & 0x1f), 64 * ((rc >> 4) & 0xf), bool(rc & 2), bool(rc & 1))


def stem_variant_table():
    """The first-layer instantiations the library holds, decoded, as its own launchers list them (csrc/conv_stem_i8.hip: STEM_TABLE, STEM_POOL_TABLE,
    and the two of csrc/conv_stem_pool7_i8.hip)."""
    fn = experimental("dlmcq_x_stem_variant_table", [ctypes.POINTER(ctypes.c_int32), ctypes.c_int])
    n = fn(None, 0)
    answers = (ctypes.c_int32 * n)()
    assert fn(answers, n) == n
    return [decode_stem_variant(int(a)) for a in answers]


def pw_variant_tables():
    """(conv_pw_i8_kernel records, conv_pwr_i8_kernel records), decoded: the instantiations the library holds, as its own launchers list them."""
    fn = experimental("dlmcq_x_pw_variant_table", [ctypes.c_int, ctypes.POINTER(ctypes.c_int32), ctypes.c_int])
    out = []
    for which in (0, 1):
        n = fn(which, None, 0)
        answers = (ctypes.c_int32 * n)()
        assert fn(which, answers, n) == n
        out.append([decode_pw_variant(int(a)) for a in answers])
    return tuple(out)


def gap_launch_record(n, c, k):
    """(slice width, nslice, ngroups, dynamic LDS bytes) of the launch dlmcq_conv2d_i8_nhwc_gap makes for n images and c -> k channels on this
    process's device (256 CUs without one) - the launcher's own record (csrc/conv_gap_i8.hip: gap_launch_record).  A workgroup owns one
    slice and the images group, group + ngroups, ...; shapes the entry point refuses raise DlmcqError."""
    fn = experimental("dlmcq_x_gap_launch_record", [_i64, _i64, _i64, ctypes.POINTER(ctypes.c_int64)])
    answer = (ctypes.c_int64 * 4)()
    check(fn(n, c, k, answer))
    return tuple(int(v) for v in answer)


def stream_ptr():
    """The hipStream_t torch is currently launching on (kernels are enqueued there, asynchronously)."""
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def require_gpu(*tensors):
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise DlmcqError(
                "dlmc (MI355X build) runs on the GPU only: got a tensor on "
                f"'{t.device}'.  There is no CPU fallback in this package.")
