/*
 * dlmcq.h - C ABI of the MI355X (gfx950) fake-quantize path.
 *
 * This is the drop-in boundary for DLMC-QUANT's fake-quantize hot path.  The reference has no
 * FFI of its own: the path is a chain of ATen elementwise/reduction ops issued from Python
 * (reference files cited per entry point below, relative to the reference checkout).  Each entry
 * point here replaces one such chain with ONE hand-written HIP kernel (or a two-launch
 * reduce/finalize pair); the Python layer in `dlmc-quant_amd/dlmc/` binds them with ctypes and
 * re-exports the reference's own names (`quantize`, `emulate_quantize`, `get_qparams_tensor`,
 * `QConv2d`, ... see INTEGRATION.md).
 *
 * Contract:
 *   - plain pointers and sizes only; no torch / C++ types cross the boundary;
 *   - every buffer (x, y, codes, scale, offset, scratch) is caller-allocated DEVICE memory; the
 *     library owns nothing and keeps no global mutable state (all functions are re-entrant);
 *   - all work is enqueued asynchronously on the caller's `stream` (a hipStream_t passed as
 *     void*), on the caller's current device; nothing here synchronises the device or allocates,
 *     so every entry point is hipGraph-capturable;
 *   - return value: 0 = success; < 0 = a DLMCQ_E* argument error (nothing was launched);
 *     > 0 = the hipError_t of the failed launch.  No exception or abort crosses the boundary.
 *
 * Tensor addressing.  Every elementwise entry point sees its tensor as (outer, channels, inner),
 * contiguous, with one (scale, offset) pair per channel:
 *     per-tensor            : outer = 1, channels = 1, inner = numel
 *     KCRS weights, axis 0  : outer = 1, channels = K, inner = C*R*S      (scale [K,1,1,1])
 *     NCHW activations, ax 1: outer = N, channels = C, inner = H*W        (scale [1,C,1,1])
 *     (N,C) activations     : outer = N, channels = C, inner = 1
 * No transpose copy is ever made (the reference materialises one: ops.py:112-118).
 */
#ifndef DLMCQ_H
#define DLMCQ_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DLMCQ_VERSION 100 /* 0.1.0 */

typedef void* dlmcq_stream_t; /* hipStream_t */

/* ---- error codes (negative; positive values are hipError_t) ---- */
#define DLMCQ_OK 0
#define DLMCQ_EINVAL (-1)       /* null pointer, negative size, lo > hi, unknown enum value */
#define DLMCQ_ERANGE (-2)       /* a size exceeds what the kernels index (see each function) */
#define DLMCQ_ESCRATCH (-3)     /* scratch buffer too small or missing */
#define DLMCQ_EALIGN (-4)       /* a pointer violates its stated alignment */

/* ---- fake-quant forms: the five clamp-round-dequant expressions of the reference ----
 * r(v) = rint(v) (round half to even); R(v) = (r(v) - v) + v, the forward value of the
 * reference's `round_pass` (utils.py:29-32): equal to r(v) but -0 -> +0 and +-inf -> NaN.
 * clamp() propagates NaN like torch.clamp.  All arithmetic is IEEE fp32, no FMA contraction. */
#define DLMCQ_FORM_EMULATE 0   /* utils.py:1-11 emulate_quantize:
                                  q = clamp(r((x-o)/(s+1e-7)), lo, hi);       y = q*s + o       */
#define DLMCQ_FORM_QBASE 1     /* modules/base.py:96-102,131-133 (QBase.forward):
                                  s^ = (s - s*g) + s*g  (grad_scale, utils.py:24-27)
                                  q = R(clamp((x-o)/s^, lo, hi));              y = q*s^ + o      */
#define DLMCQ_FORM_ZEROPOINT 2 /* FSPTQuant/base.py:108-109 (FSPTQ activations):
                                  q = clamp(R(x/s) + zp, lo, hi);              y = (q - zp)*s    */
#define DLMCQ_FORM_SYMMETRIC 3 /* FSPTQuant/base.py:149-152 (FSPTQ weights; offset unused):
                                  q = clamp(R(x/s), lo, hi);                   y = q*s           */
#define DLMCQ_FORM_ROOTQ_ACT 4 /* RootQ/base.py:106-111 + RootQ/function.py:15-20 (offset unused):
                                  u = s*(hi-lo); t = x + relu(0-x); t = t - relu(t-u)
                                  q = R(t/s);                                  y = q*s           */
#define DLMCQ_FORM_COUNT 5
/* OR-able into the `q_form` argument of the int8 convolution entry points (the consumer's quantiser evaluated in the
 * epilogue) when its range is an unsigned byte (0 <= q_lo, q_hi <= 255): the codes are stored as int8 `code - 128`
 * (each byte ^ 0x80) instead of uint8 `code`.  A consumer then takes them as signed codes (x_is_unsigned = 0) with the
 * zero point `zp - 128`: the same integers reach the matrix cores (they multiply signed bytes, so uint8 codes are
 * re-centred on every operand read otherwise), hence the same results.  Accepted by dlmcq_conv2d_i8_nhwc_fused / _asym /
 * _dual, by dlmcq_quantize_pad_nhwc4 (its `form`: the padded image buffer then holds `code - 128`, border included) and for
 * the SECOND quantiser of the chain entry points (the first one's codes are read in place by the second GEMM);
 * every other entry point returns DLMCQ_EINVAL for it. */
#define DLMCQ_EMIT_SHIFT128 0x100
/* OR-able into the LAST quantiser form argument of the chain entry points (`q2_form` of dlmcq_conv2d_i8_nhwc_chain, `q3_form` of
 * dlmcq_conv2d_i8_nhwc_dual_chain): the second 1x1 layer's weight codes are handed over CHUNK-MAJOR, int8 [K / 64][K2][64]
 * (element [n][k2][j] = KRSC element [k2][64 n + j]), so that the 64-column chunk the kernel stages per step is one contiguous
 * K2 x 64 byte block (whole cache lines per LDS-DMA instruction instead of 64-byte pieces of K-byte rows).  Same results. */
#define DLMCQ_W2_CHUNK_MAJOR 0x200
/* DLMCQ_FP32_IN_CHUNK_MAJOR / DLMCQ_FP32_OUT_CHUNK_MAJOR (OR-able into the LAST quantiser form - `q2_form` / `q3_form` - of the two chain
 * entry points): the fp32 shortcut the call reads / the fp32 block output it writes, [M][K], is CHUNK-MAJOR: [K / 64][M][64], every
 * 64-channel chunk a plane of M rows x 256 bytes (K a multiple of 64).  The kernels walk a tile of rows chunk by chunk; with row-major
 * tensors the chip's workgroups then touch 256-byte pieces K * 4 bytes apart, spread over hundreds of megabytes, and HBM serves that
 * pattern at 4.6 - 5.8 TB/s where the same loads and stores reach 5.9 - 6.0 on planes in which neighbouring workgroups' pieces are
 * neighbours (tools/probes/stream_pattern_probe.hip, round 5; the chain launches themselves: -11 ... -18 % at 14^2 and 56^2).  A private
 * layout between two of these calls: same values, another place in the buffer.  The two tensors of a call may differ in layout, except
 * for the 128 -> K -> 128 instantiation (DLMCQ_EINVAL).  A call with one fp32 tensor takes either bit for it.
 * The same two bits in `q_form` of dlmcq_conv2d_i8_nhwc_fused (its `residual` / `out`) and dlmcq_conv2d_i8_nhwc_dual (`out`): honoured where
 * the block-end kernel takes the call (DLMCQ_ROUTE_PWR - ask with DLMCQ_ROUTE_ONLY, without the bits), one layout per call; anywhere else the
 * call is refused with DLMCQ_EINVAL rather than run on a kernel that would read or write the tensor row-major. */
#define DLMCQ_FP32_IN_CHUNK_MAJOR 0x2000
#define DLMCQ_FP32_OUT_CHUNK_MAJOR 0x4000
/* Two control bits, OR-able into the `q_form` argument of dlmcq_conv2d_i8_nhwc_fused / _asym / _dual and dlmcq_conv2d_dw_i8_nhwc.
 * The chain, dual-chain, dwpw and quantize_pad_nhwc4 entry points return DLMCQ_EINVAL for them and for DLMCQ_PIPELINED in any form argument.
 * DLMCQ_FORCE_TILED: the call runs on the generic kernel of its family (conv_i8_mfma_kernel; conv_dw3*_i8_kernel for the
 * depthwise entry point) even where the library's dispatch would hand it to a specialised one (halo-tile 3x3, weight-resident
 * pointwise, block-end pointwise, matrix-core depthwise).  Same results bit for bit; it exists so that a specialised kernel and
 * the kernel it replaces can be compared on ONE tensor at any size (tests/, tools/) and for same-box A/B timing.
 * DLMCQ_ROUTE_ONLY: nothing is launched; the call validates its arguments exactly as the real call does and returns WHICH kernel
 * the dispatch picks for them (DLMCQ_ROUTE_*, all > 0; errors stay negative) - the dispatch code itself answers, so a caller's
 * bookkeeping (bench.py's per-kernel-family rooflines) cannot drift from what runs. */
#define DLMCQ_FORCE_TILED 0x400
#define DLMCQ_ROUTE_ONLY 0x800
/* DLMCQ_PIPELINED (dlmcq_conv2d_i8_nhwc_fused; opt-in): a 3x3 / stride 1 layer of 128, 256 or 512 input channels with enough tiles runs on the
 * persistent halo kernel that is software-pipelined across tiles (csrc/conv3x3_pipe_i8.hip: tile t's quantising epilogue under tile t + 1's
 * K loop) instead of the plain halo-tile kernel.  Same bytes; measured 12 - 20 % SLOWER than the plain kernel (round 5, LABNOTES 15), hence
 * not the default - kept built and tested for same-box A/B timing. */
#define DLMCQ_PIPELINED 0x1000
/* DLMCQ_PAD_CODE0 (the `form` of dlmcq_quantize_pad_nhwc4 only; every other entry point returns DLMCQ_EINVAL for it): the padded border
 * holds code 0 (with DLMCQ_EMIT_SHIFT128: the byte 0x80) instead of the code of x' = 0.  The padding of a float-offset quantiser
 * (x^ = q * s^ + o, o no code) for dlmcq_conv2d_i8_stem_xoff with a zero point of 0. */
#define DLMCQ_PAD_CODE0 0x8000
/* DLMCQ_ROUTE_VARIANT (the dlmcq_conv2d_i8_nhwc_* entry points that take DLMCQ_ROUTE_ONLY; OR-able only TOGETHER with DLMCQ_ROUTE_ONLY -
 * alone it is DLMCQ_EINVAL): where the route query would answer DLMCQ_ROUTE_TILED it answers WHICH instantiation of conv_i8_mfma_kernel the
 * call launches instead:  DLMCQ_ROUTE_VARIANT_TAG | (tile width << 8) | flags,  with the tile width in channels (64, 128, 192 or 256) and
 * `flags` the kernel's boolean template parameters: 1 DUAL (two operand pairs), 2 ADIR (activations straight to registers), 4 ASYM
 * (per-channel weight offsets), 8 SWAP (the codes-only epilogue in the swapped accumulator layout), 16 R6 (ReLU6), 32 XOFF (float
 * activation offset), 64 NARROW (narrow fp32 rows), 128 PADRES (pad shortcut).  Always above every DLMCQ_ROUTE_*; every other answer -
 * another kernel's route, DLMCQ_OK for an empty problem, a refusal - is what it is without the bit.  (tests/: which of the library's
 * instantiations a case really runs.) */
#define DLMCQ_ROUTE_VARIANT 0x10000
#define DLMCQ_ROUTE_VARIANT_TAG (1 << 24)
/* DLMCQ_ROUTE_HALO_VARIANT (as DLMCQ_ROUTE_VARIANT: OR-able only TOGETHER with DLMCQ_ROUTE_ONLY, alone it is DLMCQ_EINVAL for every entry point):
 * where the route query would answer DLMCQ_ROUTE_HALO3X3 or DLMCQ_ROUTE_HALO3X3_PIPE it answers WHICH instantiation of the 3x3 kernel the call
 * launches instead - the record the launcher itself picks the kernel from:
 *   conv3x3_halo_i8_kernel:  DLMCQ_ROUTE_HALO_VARIANT_TAG | (column width << 16) | (halo pieces per buffer << 8) | (halo buffers << 4) | flags
 *     column width 64 or 128 channels; halo pieces of 16 frame positions allocated per buffer: 24 or 32 (stride 1), 18 or 20 (stride 2);
 *     halo buffers 1, 2, or 3 (stride 2);  flags: 4 S2 (stride 2), 2 XS (uint8 codes, re-centred on read), 1 PLAIN (the compile-time plain
 *     unsigned-byte quantiser);
 *   conv3x3_pipe_i8_kernel:  DLMCQ_ROUTE_PIPE_VARIANT_TAG | (chunks of 64 input channels << 8) | flags      chunks 2, 4 or 8; flags: 2 XS.
 * Both above every DLMCQ_ROUTE_* and every DLMCQ_ROUTE_VARIANT answer; what DLMCQ_ROUTE_VARIANT means is untouched, the two bits may be
 * passed together, and every other answer - another kernel's route, a tiled variant, DLMCQ_OK for an empty problem, a refusal - is what it
 * is without the bit. */
#define DLMCQ_ROUTE_HALO_VARIANT 0x20000
/* DLMCQ_ROUTE_HALO_ROWS (only TOGETHER with DLMCQ_ROUTE_ONLY | DLMCQ_ROUTE_HALO_VARIANT, otherwise DLMCQ_EINVAL): a conv3x3_halo_i8_kernel answer
 * also names the launch's ROW MAPPING - flag 8 DENSE: a tile's rows are consecutive real pixels (no junk row of the frame is multiplied), which
 * the launcher takes for stride-1 layers whose longer halo span fits the 24-piece buffers; without the flag the rows are the frame's positions.
 * Every answer without this bit, and every other answer with it, is what it was. */
#define DLMCQ_ROUTE_HALO_ROWS 0x200000
#define DLMCQ_ROUTE_HALO_VARIANT_TAG (1 << 25)
#define DLMCQ_ROUTE_PIPE_VARIANT_TAG (1 << 26)
/* DLMCQ_ROUTE_DW_VARIANT (dlmcq_conv2d_dw_i8_nhwc and dlmcq_conv2d_dw_i8_nhwc_xoff; as the two bits above: OR-able only TOGETHER with
 * DLMCQ_ROUTE_ONLY, alone it is DLMCQ_EINVAL; every entry point that takes no route query refuses it as it refuses any bit it does not
 * know): where the route query would answer DLMCQ_ROUTE_DW or DLMCQ_ROUTE_DWM it answers WHICH instantiation the call launches instead -
 * the record the launcher itself picks the kernel from:
 *   csrc/conv_dw_i8.hip:   DLMCQ_ROUTE_DW_VARIANT_TAG | (family << 8) | (FAST << 4) | flags
 *     family 0 conv_dw3p2_i8_kernel (3x3 / 1 / 1, two pixels per thread), 1 conv_dw3_i8_kernel (any other 3x3), 2 conv_dw_i8_kernel (any
 *     filter up to 7x7); FAST 0 (any epilogue), 1 / 2 (codes only with the plain quantiser, asymmetric / symmetric weights);
 *     flags: 2 XOFF (float activation offset), 1 R6 (ReLU6);
 *   conv_dwm_i8_kernel:    DLMCQ_ROUTE_DWM_VARIANT_TAG | (halo pieces per wave << 8) | flags        pieces 4 or 5; flags: 2 XS (int8
 *     codes: no re-centring), 1 R6.
 * Both above every other answer; every other answer - DLMCQ_OK for an empty problem, a refusal - is what it is without the bit. */
#define DLMCQ_ROUTE_DW_VARIANT 0x40000
#define DLMCQ_ROUTE_DW_VARIANT_TAG (1 << 27)
#define DLMCQ_ROUTE_DWM_VARIANT_TAG (1 << 28)
/* dlmcq_conv2d_dw5_i8_nhwc's answer to DLMCQ_ROUTE_ONLY | DLMCQ_ROUTE_DW_VARIANT (the only control bits it takes, and only together): WHICH
 * instantiation of conv_dw5_i8_kernel (csrc/conv_dw5_i8.hip) the call launches,  DLMCQ_ROUTE_DW5_VARIANT_TAG | (FAST << 4) | flags,  FAST 0 / 1 / 2
 * and flags: 1 R6 as above.  Above every other answer. */
#define DLMCQ_ROUTE_DW5_VARIANT_TAG (1 << 29)
/* DLMCQ_ROUTE_CHAIN_VARIANT (the last form argument - `q2_form` / `q3_form` - of dlmcq_conv2d_i8_nhwc_chain, _dual_chain and _recompute_chain
 * only; honoured only TOGETHER with DLMCQ_ROUTE_ONLY: either bit alone stays DLMCQ_EINVAL there, and every other entry point refuses it as it
 * refuses any bit it does not know): nothing is launched; the call is validated exactly as the real call is and answers WHICH instantiation
 * of conv_chain_i8_kernel (csrc/conv_chain_i8.hip) it would launch and how - the record the launcher itself reads:
 *   DLMCQ_ROUTE_CHAIN_VARIANT_TAG | (row << 16) | (FL slot << 12) | (rows per tile << 4) | (ocm << 1) | icm
 *     row: the index of the (C1, KB, C2, CA, CB) row in the launcher's table (dlmcq_x_chain_variant_table lists it, for tests);
 *     FL slot: 0, 1, 2 for the first epilogue's compile-time form FL = 3 (ReLU + fp32 output), 1 (ReLU), -1 (read at run time);
 *     rows per tile: the tile height the launch uses, 1 .. 64 - `rows_per_tile` as passed, or what the automatic rule picks for 0;
 *     icm / ocm: the resolved layouts of the fp32 shortcut read / the fp32 block output (1: chunk-major), as the kernel is handed them -
 *     a call with one fp32 tensor has one layout, and both bits carry it.
 * Above every other answer; DLMCQ_OK for an empty problem and every refusal are what they are without the bits. */
#define DLMCQ_ROUTE_CHAIN_VARIANT 0x80000
#define DLMCQ_ROUTE_CHAIN_VARIANT_TAG (1 << 30)
/* DLMCQ_ROUTE_PW_VARIANT (as the four bits above: honoured only TOGETHER with DLMCQ_ROUTE_ONLY, alone it is DLMCQ_EINVAL for every entry
 * point, and every entry point that does not take it refuses it as it refuses any bit it does not know).  Two families take it:
 *   dlmcq_conv2d_i8_nhwc_fused / _dual (and the other entry points in front of the same dispatch: _asym carries the pointwise kernel's
 *   asymmetric weights): where the route query would answer DLMCQ_ROUTE_PW or DLMCQ_ROUTE_PWR it answers WHICH instantiation the call
 *   launches instead - the record the launcher itself picks the kernel from:
 *     conv_pw_i8_kernel:   DLMCQ_ROUTE_PW_VARIANT_TAG | (input channels / 64 << 8) | (slice width / 64 << 4) | flags
 *       the nine (input channels, slice width) pairs of csrc/conv_pw_i8.hip; flags: 2 ASYM (per-channel weight offsets), 1 R6 (ReLU6);
 *     conv_pwr_i8_kernel:  DLMCQ_ROUTE_PWR_VARIANT_TAG | (C / 256 << 4) | flags
 *       C 256 or 512: the depth of the reduction read row by row; flags: 8 SWP (dual form: the sampled pair is the call's first), 4 DUAL
 *       (the shortcut is a second, sampled 512-deep reduction), 2 OUTF (the fp32 output is stored), 1 CODES (the consumer's codes are);
 *     every other answer - the tiled route, a 3x3 route, DLMCQ_OK for an empty problem, a refusal - is what it is without the bit.
 *   dlmcq_conv2d_i8_stem_fused / _stem_asym / _stem_xoff / _stem_pool_fused (which take no other control bit, DLMCQ_ROUTE_ONLY alone
 *   included): the call is validated exactly as the real call is, nothing is launched, and the answer is the instantiation:
 *     DLMCQ_ROUTE_STEM_VARIANT_TAG | (kernel << 12) | (R << 4) | flags
 *       kernel 0 conv_stem_i8_kernel: R 1 .. 7 filter rows; flags: 8 XOFF (float activation offset), 4 SWAP (codes-only swapped epilogue),
 *       2 ASYM, 1 R6;  kernel 1 conv_stem_pool_i8_kernel: R 1 .. 7, no flags;  kernel 2 conv_stem_pool7_i8_kernel: R field 0, flags: 1 XS
 *       (uint8 codes, re-centred on read).
 * All three tags lie below every other variant tag and above every DLMCQ_ROUTE_*: no answer equals another family's. */
#define DLMCQ_ROUTE_PW_VARIANT 0x100000
#define DLMCQ_ROUTE_STEM_VARIANT_TAG (1 << 21)
#define DLMCQ_ROUTE_PW_VARIANT_TAG (1 << 22)
#define DLMCQ_ROUTE_PWR_VARIANT_TAG (1 << 23)
#define DLMCQ_ROUTE_TILED 1   /* conv_i8_mfma_kernel (csrc/conv_i8.hip) */
#define DLMCQ_ROUTE_HALO3X3 2 /* conv3x3_halo_i8_kernel (csrc/conv3x3_i8.hip) */
#define DLMCQ_ROUTE_PW 3      /* conv_pw_i8_kernel (csrc/conv_pw_i8.hip) */
#define DLMCQ_ROUTE_PWR 4     /* conv_pwr_i8_kernel (csrc/conv_pwr_i8.hip) */
#define DLMCQ_ROUTE_DW 5      /* conv_dw_i8_kernel / conv_dw3_i8_kernel / conv_dw3p2_i8_kernel (csrc/conv_dw_i8.hip) */
#define DLMCQ_ROUTE_DWM 6     /* conv_dwm_i8_kernel (csrc/conv_dwm_i8.hip) */
#define DLMCQ_ROUTE_HALO3X3_PIPE 7 /* conv3x3_pipe_i8_kernel (csrc/conv3x3_pipe_i8.hip) */
#define DLMCQ_ROUTE_GAP 8     /* conv_gap_i8_kernel (csrc/conv_gap_i8.hip): the answer of dlmcq_conv2d_i8_nhwc_gap */

/* ---- the activation of a fused epilogue: the `relu` / `relu2` / `relu3` / `dw_relu` arguments of the convolution entry points ----
 * DLMCQ_ACT_RELU6 is  v = v < 0 ? 0 : (v > 6 ? 6 : v)  (torch.nn.functional.relu6; NaN stays NaN, -0 stays -0), applied in fp32
 * before the value is stored or quantised.  It is implemented by dlmcq_conv2d_i8_nhwc_fused / _fused_observed / _asym,
 * dlmcq_conv2d_dw_i8_nhwc and dlmcq_conv2d_i8_stem_fused / _stem_asym; every other entry point with an activation argument
 * returns DLMCQ_EINVAL for it before anything is launched (dual, chain, dual-chain, dwpw, stem_pool_fused).  Every other
 * non-zero value keeps its earlier meaning, ReLU. */
#define DLMCQ_ACT_NONE 0
#define DLMCQ_ACT_RELU 1
#define DLMCQ_ACT_RELU6 2

/* ---- what is written to `y` ---- */
#define DLMCQ_Y_DEQUANT 0 /* the fake-quantised value y */
#define DLMCQ_Y_CODES 1   /* the integer code q as fp32 (reference `quantize`, utils.py:1-2) */

/* ---- integer code emission (no reference counterpart: it keeps codes in fp32) ---- */
#define DLMCQ_CODES_NONE 0
#define DLMCQ_CODES_I8 1  /* one byte per element: int8 when lo < 0, uint8 otherwise */
#define DLMCQ_CODES_P4 2  /* two codes per byte, element 2i in the low nibble, 2i+1 in the high
                             nibble; two's-complement nibbles when lo < 0.  Needs -8<=lo, hi<=15 */

int dlmcq_version(void);
const char* dlmcq_strerror(int code);

/*
 * Fake-quantise x -> y (and/or integer codes) in one pass: 4 B read + 4 B written per element
 * (+1 B int8 codes, +0.5 B packed int4).  Replaces the 6-9 separate ATen passes of
 * utils.py:9-11 / modules/base.py:102,133 / FSPTQuant/base.py:108-109,149-152 / RootQ/base.py:108-111.
 *   x, y     : fp32 [outer*channels*inner]; y may alias x; y may be NULL when only codes are wanted
 *   codes    : NULL or the buffer selected by codes_kind (4-byte aligned)
 *   scale    : fp32 [channels]        offset: fp32 [channels] or NULL (= 0)
 *   ste_g    : DLMCQ_FORM_QBASE only - the `g` of grad_scale; 0 gives s^ = s
 * Any pointer alignment is accepted (16-byte aligned x/y take the 128-bit path).
 * DLMCQ_ERANGE if channels*inner >= 2^31 with channels > 1, or the launch would exceed 2^31 blocks.
 */
int dlmcq_fake_quant_f32(const float* x, float* y, void* codes, const float* scale,
                         const float* offset, int64_t outer, int64_t channels, int64_t inner,
                         int32_t lo, int32_t hi, int32_t form, int32_t y_kind, int32_t codes_kind,
                         float ste_g, dlmcq_stream_t stream);

/*
 * Dequantise stored integer codes: the second half of every form above (reference `dequantize`,
 * utils.py:5-6, for forms EMULATE/QBASE).  codes_kind I8 or P4; `is_signed` selects int8/uint8 or
 * the nibble sign extension.  For DLMCQ_FORM_QBASE pass the same ste_g as at quantisation.
 */
int dlmcq_dequant_codes_f32(const void* codes, float* y, const float* scale, const float* offset,
                            int64_t outer, int64_t channels, int64_t inner, int32_t form,
                            int32_t codes_kind, int32_t is_signed, float ste_g,
                            dlmcq_stream_t stream);

/* Reference `dequantize` on fp32 codes (utils.py:5-6): y = q*s + o. */
int dlmcq_dequant_f32(const float* q, float* y, const float* scale, const float* offset,
                      int64_t outer, int64_t channels, int64_t inner, dlmcq_stream_t stream);

/* ---- observer (ops.py:20-34 per tensor, ops.py:112-140 per channel) ---- */
#define DLMCQ_MINMAX_ABSMAX 0 /* out_max[c] = max|x|;             out_min untouched (may be NULL) */
#define DLMCQ_MINMAX_MINMAX 1 /* out_max[c] = max x, out_min[c] = min x                           */
#define DLMCQ_MINMAX_NEGMIN 2 /* out_max[c] = max x, out_min[c] = -min x: [max | -min] is then one
                                 flat vector for a single all_reduce(MAX) across ranks (C2)       */

/* Bytes of device scratch the observer needs for this shape (partials of the first stage). */
size_t dlmcq_minmax_scratch_bytes(int64_t outer, int64_t channels, int64_t inner);

/*
 * One read of x (4 B per element), NaN-propagating like torch.max/min.  Two launches: a partial
 * reduction (wave shuffles -> LDS -> one partial per block) and a finalize over the partials.
 * Deterministic (no atomics); results do not depend on the launch geometry.
 */
int dlmcq_minmax_f32(const float* x, float* out_max, float* out_min, int64_t outer,
                     int64_t channels, int64_t inner, int32_t mode, void* scratch,
                     size_t scratch_bytes, dlmcq_stream_t stream);

/* The second stage of dlmcq_minmax_f32 alone, per tensor: `count` partials in three planes `plane_stride` floats apart ([max | min |
 * bits of max |x|]: what a stage-1 kernel or dlmcq_conv2d_i8_nhwc_fused_observed wrote) -> out_max[0], out_min[0] as `mode` says. */
int dlmcq_minmax_finalize_f32(const float* partials, int64_t count, int64_t plane_stride, float* out_max, float* out_min,
                              int32_t mode, dlmcq_stream_t stream);

/*
 * The arithmetic tail of quantize_minmax_{tensor,channel} on device (no host sync):
 *   signed  : scale = vmax / (2^(b-1)-1)              offset = 0         (vmax = max|x|)
 *   unsigned: scale = (vmax - vmin) / (2^b-1)         offset = vmin      (allow_offset != 0)
 *             scale = (vmax - 0) / (2^b-1)            offset = 0         (allow_offset == 0)
 * then scale += scale_eps when scale_eps != 0 (FSPTQuant/base.py:129 adds 1e-6).
 * `min_is_negated` != 0 when vmin holds -min (DLMCQ_MINMAX_NEGMIN, after the all-reduce).
 */
int dlmcq_qparams_from_minmax(const float* vmax, const float* vmin, float* scale, float* offset,
                              int64_t channels, int32_t n_bits, int32_t is_signed,
                              int32_t allow_offset, int32_t min_is_negated, float scale_eps,
                              dlmcq_stream_t stream);

/*
 * RootQ activation initialisation (RootQ/base.py:80): scale[c] = (vmax[c] - vmin[c]) / span with a true
 * IEEE division (span = hi - lo of the format).  `min_is_negated` as above.
 */
int dlmcq_span_scale_f32(const float* vmax, const float* vmin, float* scale, int64_t channels, float span,
                         int32_t min_is_negated, dlmcq_stream_t stream);

/*
 * LSQ initialisation (modules/base.py:84-85 input, :118-121 weight): scale[0] = 2 * mean|x| / sqrt(Qp), the QAT flow's default
 * first-call initialiser (example/quantization/LSQ_config.yaml, `type: "LSQ"`).  One read of x (4 B per element); per-lane
 * double partials, a fixed-order tree over one double per workgroup (no atomics: deterministic), then the reference's own
 * fp32 chain on the device: mean = fl32(sum) / n, 2 * mean, true IEEE division by `sqrt_qmax` (= the fp32 value of
 * math.sqrt(Qp) the caller computed).  The only difference from the reference's CPU result is the summation order of the mean
 * (<= a few ulp; tests state 2e-6 relative).  `scratch`: dlmcq_lsq_init_scratch_bytes() bytes, 8-byte aligned.
 */
size_t dlmcq_lsq_init_scratch_bytes(int64_t n);
int dlmcq_lsq_init_f32(const float* x, float* scale, int64_t n, float sqrt_qmax, void* scratch, size_t scratch_bytes,
                       dlmcq_stream_t stream);

/* dlmcq_minmax_f32 + dlmcq_qparams_from_minmax fused into the same two launches. */
int dlmcq_observe_qparams_f32(const float* x, float* scale, float* offset, int64_t outer,
                              int64_t channels, int64_t inner, int32_t n_bits, int32_t is_signed,
                              int32_t allow_offset, float scale_eps, void* scratch,
                              size_t scratch_bytes, dlmcq_stream_t stream);

/* ---- sub-byte pack / unpack (BASELINE config 5; layout as DLMCQ_CODES_P4) ---- */
int dlmcq_pack_int4(const int8_t* codes, uint8_t* packed, int64_t n, dlmcq_stream_t stream);
int dlmcq_unpack_int4(const uint8_t* packed, int8_t* codes, int64_t n, int32_t is_signed,
                      dlmcq_stream_t stream);

/*
 * Backward of DLMCQ_FORM_QBASE as autograd executes it through modules/base.py:96-102 (closed
 * form: modules/function.py:37-49).  With v = (x-o)/s^, inside = [lo <= v <= hi]:
 *   gx       = inside ? (gy*s^)/s^ : +0                      (bit-exact with autograd)
 *   gscale[c]= g * sum(gy*q - inside*(gy*s^)*(v/s^))          (fp32 tree sum, deterministic)
 * gx may alias gy; gx or gscale may be NULL.  scratch: dlmcq_fq_bwd_scratch_bytes().
 */
size_t dlmcq_fq_bwd_scratch_bytes(int64_t outer, int64_t channels, int64_t inner);
int dlmcq_fake_quant_bwd_f32(const float* x, const float* gy, float* gx, float* gscale,
                             const float* scale, const float* offset, int64_t outer,
                             int64_t channels, int64_t inner, int32_t lo, int32_t hi, float ste_g,
                             void* scratch, size_t scratch_bytes, dlmcq_stream_t stream);
/*
 * The same for the FSPTQ forms, as autograd executes FSPTQuant/base.py:108-109 (DLMCQ_FORM_ZEROPOINT, offset = zero
 * point: u = x/s, a = R(u) + zp, inside = [lo <= a <= hi], gscale = sum gy*((clamp(a) - zp) - inside*u)) and :149-152
 * (DLMCQ_FORM_SYMMETRIC, per-channel weight scale, no offset), and for the RootQ activation form
 * (DLMCQ_FORM_ROOTQ_ACT, RootQ/base.py:106-111: clipped elements pass nothing to x; the scale also collects
 * gy*(hi - lo) from every element clipped above); DLMCQ_FORM_QBASE is the call above.  ste_g is used by QBASE only.
 */
int dlmcq_fake_quant_bwd_form_f32(const float* x, const float* gy, float* gx, float* gscale,
                                  const float* scale, const float* offset, int64_t outer,
                                  int64_t channels, int64_t inner, int32_t lo, int32_t hi, int32_t form,
                                  float ste_g, void* scratch, size_t scratch_bytes,
                                  dlmcq_stream_t stream);

/*
 * ---- fake-quant of MANY weight tensors in one launch, forward and backward (csrc/fake_quant_multi.hip) ----
 * A segment is one tensor with its quantiser; a device-resident table of segments drives one forward launch
 * (dlmcq_fake_quant_multi_f32) and one backward launch plus one finalize (dlmcq_fake_quant_multi_bwd_f32).  For every
 * segment y, gx and gscale are bit-identical to dlmcq_fake_quant_f32 (y_kind = DLMCQ_Y_DEQUANT, no codes) and
 * dlmcq_fake_quant_bwd_form_f32 on that tensor alone: both families run the same per-workgroup bodies (csrc/fq_bodies.h).
 *
 * Layout: 17 fields of 8 bytes, no padding (sizeof = dlmcq_fq_segment_bytes() = 136).  The caller fills the first 14
 * on the host, dlmcq_fq_multi_prepare fills the last three, and the caller copies the table to the device.
 *
 * Eligibility (everything else keeps its own launches):
 *   - fp32, contiguous; x, y, gy and gx 16-byte aligned (DLMCQ_EALIGN otherwise);
 *   - form is DLMCQ_FORM_QBASE, DLMCQ_FORM_ZEROPOINT or DLMCQ_FORM_SYMMETRIC (DLMCQ_EINVAL otherwise);
 *   - per tensor (channels == 1; inner is ignored) or per channel on axis 0 (n == channels * inner, rows of `inner`
 *     elements; DLMCQ_EINVAL otherwise);
 *   - at most 8192 backward chunks of 1024 elements, n <= 8 388 608 (DLMCQ_ERANGE otherwise): above that the one-tensor
 *     backward grid-strides and one chunk per workgroup cannot reproduce its summation order;
 *   - lo <= hi (DLMCQ_EINVAL), both within int32 (DLMCQ_ERANGE); n, channels >= 0 ... see dlmcq_fq_multi_prepare.
 */
typedef struct dlmcq_fq_segment {
  const float* x;       /* input, n elements */
  float* y;             /* forward output (dequantised fp32); NULL: the segment takes no part in the forward */
  const float* gy;      /* backward: gradient of y; NULL (n > 0): the segment takes no part in the backward */
  float* gx;            /* backward: gradient of x, or NULL (not wanted); may alias gy */
  const float* scale;   /* [channels] */
  const float* offset;  /* [channels] or NULL (= 0): QBASE offset / ZEROPOINT zero point; SYMMETRIC ignores it */
  float* gscale;        /* backward: [channels] gradient of scale, or NULL (not wanted) */
  int64_t n;            /* elements; 0 is legal: no workgroups (the backward zero-fills gscale, as the one-tensor call does) */
  int64_t channels;     /* 1: per tensor;  > 1: per channel on axis 0 */
  int64_t inner;        /* elements per channel row (channels > 1) */
  int64_t lo, hi;       /* integer code range */
  double ste_g;         /* DLMCQ_FORM_QBASE only: the `g` of grad_scale (rounded to fp32, as the one-tensor calls take it) */
  int64_t form;         /* DLMCQ_FORM_QBASE / _ZEROPOINT / _SYMMETRIC */
  /* filled in by dlmcq_fq_multi_prepare: */
  int64_t fwd_chunk0;   /* first forward workgroup (one 256-element chunk each) */
  int64_t bwd_wg0;      /* first backward workgroup (per tensor: one 1024-element chunk each; per channel: one row each) */
  int64_t part0;        /* first of this segment's fp32 partial sums in the scratch (one per backward workgroup) */
} dlmcq_fq_segment;

size_t dlmcq_fq_segment_bytes(void);
/*
 * Host only (no HIP call): validates every segment of the HOST table `segs` (the codes above; nseg < 0 or a NULL output pointer:
 * DLMCQ_EINVAL; n > 0 with x or scale NULL: DLMCQ_EINVAL), fills fwd_chunk0 / bwd_wg0 / part0 and returns the grids:
 *   *fwd_workgroups      sum over segments with y != NULL of max(1, ceil((n / 4) / 64))      (n > 0)
 *   *bwd_workgroups      sum over segments with gy != NULL and (gx or gscale) of: channels == 1 ? max(1, ceil((n / 4) / 256))
 *                        : channels                                                          (n > 0)
 *   *finalize_workgroups nseg when any segment has a gscale, else 0: the finalize is indexed by segment, and the workgroup
 *                        of a segment with nothing to fold returns at once
 *   *scratch_bytes       4 bytes per backward workgroup when any segment has a gscale, else 0
 * Empty segments get no forward or backward workgroups.
 */
int dlmcq_fq_multi_prepare(dlmcq_fq_segment* segs, int64_t nseg, int64_t* fwd_workgroups, int64_t* bwd_workgroups,
                           int64_t* finalize_workgroups, size_t* scratch_bytes);
/* One launch for every segment with y != NULL.  `table` is the prepared table in DEVICE memory (8-byte aligned). */
int dlmcq_fake_quant_multi_f32(const dlmcq_fq_segment* table, int64_t nseg, int64_t fwd_workgroups,
                               dlmcq_stream_t stream);
/* One backward launch and (finalize_workgroups > 0) one finalize launch.  scratch_bytes below what prepare returned
 * (or a NULL scratch when it returned more than 0): DLMCQ_ESCRATCH.  Buffers of segments that take no part, and a NULL gx / gscale, are not touched. */
int dlmcq_fake_quant_multi_bwd_f32(const dlmcq_fq_segment* table, int64_t nseg, int64_t bwd_workgroups,
                                   int64_t finalize_workgroups, void* scratch, size_t scratch_bytes,
                                   dlmcq_stream_t stream);

/*
 * RootQ weight forward (RootQ/base.py:146-155 + RootQ/function.py:15-32,58-67), per tensor.
 * `bounds` is a device array {upper, lower}.  The forward value does not depend on alpha (it only
 * shapes the gradient), so alpha is not an input.  y = ((sgn+1)/2 + interval)*delta + lower.
 */
int dlmcq_rootq_weight_f32(const float* w, float* y, const float* bounds, int64_t n, int32_t lo,
                           int32_t hi, dlmcq_stream_t stream);

/*
 * Backward of that transform as autograd runs the reference's op chain (RootQ/base.py:146-155 + function.py:15-32,58-67;
 * the sign and the floor are straight-through): gw[n] (nullable) and g_bounds_alpha = {g_upper, g_lower, g_alpha}.
 * alpha: device scalar.  scratch: dlmcq_rootq_bwd_scratch_bytes(n).  Two launches instead of the ~35 elementwise ones
 * the op chain costs per layer per step.
 */
size_t dlmcq_rootq_bwd_scratch_bytes(int64_t n);
int dlmcq_rootq_weight_bwd_f32(const float* w, const float* gy, float* gw, float* g_bounds_alpha,
                               const float* bounds, const float* alpha, int64_t n, int32_t lo, int32_t hi,
                               void* scratch, size_t scratch_bytes, dlmcq_stream_t stream);

/* ---- weight transforms that precede the path in the few-shot PTQ flow (FSPTQuant.py:65-67) ---- */

/*
 * BatchNorm folding, in place (dlmc/utils/merge_bn.py:85-101): with sd = sqrt(var + var_eps)
 *   weight[k, :] <- (weight[k, :] * gamma[k]) / sd[k];   bias[k] <- (gamma[k]*(bias[k] - mean[k])) / sd[k] + beta[k]
 * The reference adds 1e-7 to the running variance here (not the layer's eps): pass var_eps = 1e-7f.
 * weight is [out_channels, inner]; bias must exist ([out_channels], zeros when the conv had none).
 */
int dlmcq_fold_bn_f32(float* weight, float* bias, const float* gamma, const float* beta,
                      const float* mean, const float* var, int64_t out_channels, int64_t inner,
                      float var_eps, dlmcq_stream_t stream);

/*
 * RepVGG re-parameterisation (model/classification/repvgg.py:92-147): the 3x3 branch, the 1x1 branch and
 * the optional identity branch, each followed by BatchNorm, fused into one 3x3 kernel + bias.
 * bn3 / bn1 / bnid are HOST arrays of 4 device pointers {gamma, beta, running_mean, running_var}; bnid is
 * NULL when the block has no identity branch.  k3 is [K, cin_per_group, 3, 3], k1 is [K, cin_per_group, 1, 1].
 */
int dlmcq_repvgg_fuse_f32(const float* k3, const float* k1, float* out_kernel, float* out_bias,
                          const float* const* bn3, const float* const* bn1, const float* const* bnid,
                          float eps3, float eps1, float epsid, int64_t out_channels,
                          int64_t cin_per_group, dlmcq_stream_t stream);

/* ---- calibration-time estimators (ops.py:71-83, :198-215) ---- */

/*
 * One iteration of the l2norm scale refinement, fused: q = clamp(r((x-o)/(s+1e-7)), lo, hi),
 * new_scale[c] = SUM x*q / SUM (q*q + 1e-7), one read of x.  Order-dependent fp32/fp64 sums: equal to the
 * reference to summation tolerance.  scratch: dlmcq_l2norm_scratch_bytes().
 */
size_t dlmcq_l2norm_scratch_bytes(int64_t outer, int64_t channels, int64_t inner);
int dlmcq_l2norm_step_f32(const float* x, const float* scale, const float* offset, float* new_scale,
                          int64_t outer, int64_t channels, int64_t inner, int32_t lo, int32_t hi,
                          void* scratch, size_t scratch_bytes, dlmcq_stream_t stream);

/* The same refinement run to convergence WITHOUT host round trips: `iterations` iterations are enqueued; each one does
 * nothing once state[0] != 0 (converged: |new - s| / s <= eps per tensor, ||new - s|| / ||s|| <= eps per channel,
 * ops.py:77-81 / :205-210), so the caller reads the flag once per batch instead of syncing on `diff` every step.
 * scale (in/out) [channels]; state = {done, iterations run, unused} (3 floats, zero-initialised by the caller). */
int dlmcq_l2norm_iterate_f32(const float* x, float* scale, const float* offset, float* state, int64_t outer,
                             int64_t channels, int64_t inner, int32_t lo, int32_t hi, int32_t iterations, float eps,
                             void* scratch, size_t scratch_bytes, dlmcq_stream_t stream);

/* One output-aware refinement step (ops.py:96-108 per tensor, :268-284 per output channel), fused: in ONE read of the
 * layer output `out` and of `out_q` = the layer applied to the quantised weight ([outer, channels, inner] both),
 *   s_new = SUM out*out_q / SUM (out_q*out_q + 1e-7),   mse = SUM (out - out_q)^2 / mse_div   (l2_loss, loss.py:22-24)
 * then on device: the reference's best-scale bookkeeping (per tensor: scale <- s_new, best <- scale if mse improved;
 * per channel: best <- OLD scale if mse improved, scale <- s_new) and the convergence flag as above.
 * scale (in/out) [1 or channels]; best_scale [2 x that] (second half: staging); state = {done, iterations, best mse}. */
size_t dlmcq_l2out_scratch_bytes(int64_t outer, int64_t channels, int64_t inner);
int dlmcq_l2out_update_f32(const float* out, const float* out_q, float* scale, float* best_scale, float* state,
                           int64_t outer, int64_t channels, int64_t inner, int32_t per_channel, float mse_div, float eps,
                           void* scratch, size_t scratch_bytes, dlmcq_stream_t stream);

/* quantize_l2loss_tensor (ops.py:36-68, unsigned): the 80-step shrink search in ONE read of x - 80 running squared errors
 * per thread, candidates (scale_i, round(-min_i / scale_i)) derived on device from (vmax, vmin) - and the reference's
 * selection (first loss below 1000, then strictly better ones).  loss_div = numel / shape[1] (l2_loss sums axis 1 and
 * averages the rest).  vmin may be NULL (allow_offset = False).  scale / offset: one float each. */
size_t dlmcq_l2loss_scratch_bytes(int64_t n);
int dlmcq_l2loss_tensor_f32(const float* x, const float* vmax, const float* vmin, float* scale, float* offset, int64_t n,
                            int32_t n_bits, float loss_div, void* scratch, size_t scratch_bytes, dlmcq_stream_t stream);

/* quantize_l2loss_channel (ops.py:169-196) for [rows, inner] rows: one workgroup per row (cached in LDS up to 8192
 * elements), the 80 steps in order with the reference's aliasing quirk (`min_val` is `offset`: an accepted step replaces
 * the minimum by its zero point).  scale / offset [rows]: in = quantize_minmax_channel's result, out = the search's. */
int dlmcq_l2loss_rows_f32(const float* x, float* scale, float* offset, int64_t rows, int64_t inner, int32_t n_bits,
                          dlmcq_stream_t stream);

/*
 * AdaRound weight path of the few-shot PTQ wrapper (FSPTQuant/base.py:69-79,136-141,151-152), per output channel:
 *   y = clamp(floor(w/s_k) + r, lo, hi) * s_k,  r = clamp(sigmoid(alpha)*1.2 - 0.1, 0, 1) when `training`, else [alpha >= 0]
 * and its backward w.r.t. alpha and s_k (w receives no gradient through floor):
 *   g_alpha = gy*s_k*[lo<=q<=hi]*1.2*sig*(1-sig)*[0<=1.2*sig-0.1<=1],   g_scale[k] = sum gy*clamp(q, lo, hi)
 * w / alpha / y / gy / g_alpha are [out_channels, inner]; g_alpha or g_scale may be NULL.
 */
int dlmcq_adaround_weight_f32(const float* w, const float* alpha, const float* scale, float* y,
                              int64_t out_channels, int64_t inner, int32_t lo, int32_t hi,
                              int32_t training, dlmcq_stream_t stream);
int dlmcq_adaround_weight_bwd_f32(const float* w, const float* alpha, const float* scale,
                                  const float* gy, float* g_alpha, float* g_scale,
                                  int64_t out_channels, int64_t inner, int32_t lo, int32_t hi,
                                  dlmcq_stream_t stream);

/* ---- fused int8-dequant x GEMM convolution / linear on the matrix cores ---- */

/*
 * Weights fp32 KCRS -> int8 codes in KRSC order (the reduction order of the implicit GEMM) with the
 * SYMMETRIC form (q = clamp(R(w / scale[k]), lo, hi), FSPTQuant/base.py:149-152), plus wsum[k] = sum of the
 * codes of output channel k (needed for the activation zero-point / uint8 shift correction).
 */
int dlmcq_quantize_weight_krsc_i8(const float* w, int8_t* wq, int32_t* wsum, const float* scale,
                                  int64_t K, int64_t C, int64_t R, int64_t S, int32_t lo, int32_t hi,
                                  dlmcq_stream_t stream);

/*
 * out[n,p,q,k] = in_scale * w_scale[k] * SUM_{r,s,c} (x[n,h,w,c] - zp) * wq[k,r,s,c]  + bias[k]
 * i.e. F.conv2d(x', w', bias) of modules/conv.py:18-19 on the fake-quantised operands, with exact int32
 * accumulation on v_mfma_i32_32x32x32_i8 (groups = 1).  Zero padding is padding of x' = 0, i.e. of x = zp.
 *   x        integer codes, NHWC (uint8 when x_is_unsigned, else int8), 16-byte aligned, C % 64 == 0
 *   w, wsum  from dlmcq_quantize_weight_krsc_i8
 *   out      fp32 NHWC [N, P, Q, K];  bias [K] or NULL
 *   in_scale, in_zero_point: device scalars (zero point must hold an integer value; NULL = 0); w_scale [K]
 * A linear layer is the case H = W = R = S = 1.
 */
int dlmcq_conv2d_i8_nhwc_f32(const void* x, const int8_t* w, float* out, const float* bias,
                             const int32_t* wsum, const float* in_scale, const float* in_zero_point,
                             const float* w_scale, int64_t N, int64_t H, int64_t W, int64_t C, int64_t K,
                             int64_t R, int64_t S, int32_t stride, int32_t pad, int32_t dilation,
                             int32_t x_is_unsigned, dlmcq_stream_t stream);

/*
 * The same contraction with the work that FOLLOWS a quantised layer in a frozen (inference) network folded
 * into the epilogue, so the fp32 output, the ReLU pass, the residual add and the consumer's quantise pass stop
 * being separate trips through HBM.  In order, per output element v = in_scale*w_scale[k]*SUM + bias[k]:
 *   residual != NULL : v = v + residual[n,p,q,k]          (fp32 NHWC, the output's shape: the block's shortcut)
 *   relu == 1        : v = v < 0 ? 0 : v                  (DLMCQ_ACT_RELU: torch.relu; NaN stays NaN)
 *   relu == 2        : v = v < 0 ? 0 : (v > 6 ? 6 : v)    (DLMCQ_ACT_RELU6: F.relu6; the specialised kernels without the bound
 *                                                          - halo-tile 3x3, pipelined 3x3, block-end pointwise - are not chosen)
 *   out != NULL      : out[n,p,q,k] = v
 *   codes != NULL    : codes[n,p,q,k] = the consumer's activation code of v: forms EMULATE / QBASE /
 *                      ZEROPOINT / SYMMETRIC of dlmcq_fake_quant_f32 with (q_scale, q_zero_point, q_lo, q_hi,
 *                      q_ste_g) - the same arithmetic in the same order, hence the bytes that
 *                      dlmcq_fake_quant_f32(..., DLMCQ_CODES_I8) would write for the stored fp32 tensor.
 *                      uint8 when q_lo >= 0, else int8; -128 <= q_lo <= q_hi <= 255, q_hi - q_lo <= 255.
 * At least one of out / codes must be given.  Replaces, for a frozen network, the chain
 * F.conv2d -> (+ identity) -> ReLU -> next FSPTQBase.forward activation branch (FSPTQuant/base.py:108-109).
 */
int dlmcq_conv2d_i8_nhwc_fused(const void* x, const int8_t* w, float* out, const float* bias,
                               const int32_t* wsum, const float* in_scale, const float* in_zero_point,
                               const float* w_scale, int64_t N, int64_t H, int64_t W, int64_t C, int64_t K,
                               int64_t R, int64_t S, int32_t stride, int32_t pad, int32_t dilation,
                               int32_t x_is_unsigned, const float* residual, int32_t relu, void* codes,
                               const float* q_scale, const float* q_zero_point, int32_t q_lo, int32_t q_hi,
                               int32_t q_form, float q_ste_g, dlmcq_stream_t stream);

/* dlmcq_conv2d_i8_nhwc_fused (out != NULL) that also OBSERVES its fp32 output - the calibrating first batch (round 5): the min/max pass
 * of the consumer's activation observer (modules/base.py:82-94 / FSPTQuant/base.py:99-103 -> ops.py:20-34: one more read of the tensor) comes
 * out of the epilogue of the launch that writes the tensor.  Every workgroup of the tiled kernel stores the (max, min, unsigned max of the
 * bits of |v| - the NaN detector) of the values it wrote as entry i of three planes of `*partials_count` floats each in `partials`
 * (observer.hip's partial layout; capacity >= 3 * dlmcq_conv2d_i8_observed_partials(N P Q, K) floats, else DLMCQ_ESCRATCH);
 * dlmcq_minmax_finalize_f32 reduces them to what dlmcq_minmax_f32 gives for the tensor - max and min are exact, so bit for bit.
 * `*partials_count` (written on the host before the call returns) is 0 when the dispatch hands the call to a kernel without the
 * observing epilogue (the block-end pointwise kernel): observe the tensor with dlmcq_minmax_f32 then.  K < 1 or N P Q < 1: DLMCQ_EINVAL. */
size_t dlmcq_conv2d_i8_observed_partials(int64_t M, int64_t K);
int dlmcq_conv2d_i8_nhwc_fused_observed(const void* x, const int8_t* w, float* out, const float* bias, const int32_t* wsum,
                                        const float* in_scale, const float* in_zero_point, const float* w_scale, int64_t N,
                                        int64_t H, int64_t W, int64_t C, int64_t K, int64_t R, int64_t S, int32_t stride,
                                        int32_t pad, int32_t dilation, int32_t x_is_unsigned, const float* residual,
                                        int32_t relu, void* codes, const float* q_scale, const float* q_zero_point,
                                        int32_t q_lo, int32_t q_hi, int32_t q_form, float q_ste_g, float* partials,
                                        int64_t partials_capacity, int64_t* partials_count, dlmcq_stream_t stream);

/* dlmcq_conv2d_i8_nhwc_fused for ASYMMETRIC per-output-channel weights (ops.py:129-136, unsigned `minmax_channel`:
 * w' = qw * s_w[k] + o_w[k], the offset being the channel minimum; BASELINE configs[4], W4A8): the convolution gains the
 * term  o_w[k] * SUM x'  over the receptive field, which the kernel evaluates from a per-pixel sum of the activation
 * codes (v_dot4_i32_i8 on the operand fragments it multiplies anyway):
 *     out = s_in * ( s_w[k] * (SUM q'*qw + (shift - zp) * SUM qw)  +  o_w[k] * SUM (q - zp) ) + bias[k].
 * `w` holds int8 codes; codes above 127 (8-bit unsigned weights) are stored minus 128 with w_offset += 128 * s_w[k]. */
int dlmcq_conv2d_i8_nhwc_asym(const void* x, const int8_t* w, float* out, const float* bias, const int32_t* wsum,
                              const float* in_scale, const float* in_zero_point, const float* w_scale, const float* w_offset,
                              int64_t N, int64_t H, int64_t W, int64_t C, int64_t K, int64_t R, int64_t S, int32_t stride,
                              int32_t pad, int32_t dilation, int32_t x_is_unsigned, const float* residual, int32_t relu,
                              void* codes, const float* q_scale, const float* q_zero_point, int32_t q_lo, int32_t q_hi,
                              int32_t q_form, float q_ste_g, dlmcq_stream_t stream);

/* Narrow fp32 rows: dlmcq_conv2d_i8_nhwc_fused (w_offset == NULL) / dlmcq_conv2d_i8_nhwc_asym (w_offset != NULL) for a layer whose
 * K is its real channel count Kf zero-padded to the K step of its consumer (K % 64 == 0, Kf % 4 == 0, K - 64 < Kf <= K; anything
 * else DLMCQ_EINVAL): the two fp32 tensors have rows of the REAL width, the codes rows of the padded one.
 *   residual  fp32 [N, P, Q, Kf] or NULL, out  fp32 [N, P, Q, Kf] or NULL: columns Kf .. K - 1 are neither read nor written
 *   codes     [N, P, Q, K] or NULL: every column is written; for a column in Kf .. K - 1 no shortcut is added - the code is the
 *             consumer's code of what the (zero) padded weights, bias and weight offset give
 *   w, wsum, w_scale, bias, w_offset: [K] entries / rows, the padded ones included
 * Per element the order of dlmcq_conv2d_i8_nhwc_fused: dequantise, weight-offset term, shortcut, ReLU / ReLU6, store, quantiser; with
 * Kf == K the call gives, bit for bit, what _fused / _asym gives.  out, residual AND codes 16-byte aligned (DLMCQ_EALIGN otherwise).
 * Always conv_i8_mfma_kernel (64-wide tiles, unswapped epilogue): the halo-tile, pointwise and block-end kernels are never chosen, so
 * DLMCQ_FORCE_TILED changes nothing and DLMCQ_ROUTE_ONLY answers DLMCQ_ROUTE_TILED; DLMCQ_EMIT_SHIFT128 as in _fused; DLMCQ_PIPELINED and
 * the two DLMCQ_FP32_*_CHUNK_MAJOR bits are DLMCQ_EINVAL.  No dual, observing or float-offset (_xoff) form. */
int dlmcq_conv2d_i8_nhwc_narrow(const void* x, const int8_t* w, float* out, const float* bias, const int32_t* wsum,
                                const float* in_scale, const float* in_zero_point, const float* w_scale, const float* w_offset,
                                int64_t N, int64_t H, int64_t W, int64_t C, int64_t K, int64_t R, int64_t S, int32_t stride,
                                int32_t pad, int32_t dilation, int32_t x_is_unsigned, const float* residual, int32_t relu,
                                void* codes, const float* q_scale, const float* q_zero_point, int32_t q_lo, int32_t q_hi,
                                int32_t q_form, float q_ste_g, int64_t Kf, dlmcq_stream_t stream);

/* Pad shortcut: dlmcq_conv2d_i8_nhwc_narrow whose shortcut is not a tensor of the output's shape but the SOURCE of a parameter-free
 * "option A" shortcut (He et al. 2016, section 4.2: subsample, zero-pad the channels)
 *     shortcut = pad(res_src[:, ::res_stride, ::res_stride, :], res_clo zero channels in front, Kf - res_clo - res_c behind)
 * read in place by the epilogue - the padded tensor is never written or read back.
 *   res_src   fp32 [N, res_h, res_w, res_c], DENSE (rows of res_c floats, no gaps), 16-byte aligned (DLMCQ_EALIGN otherwise), not NULL
 *   output row (n, p, q), fp32 column col < Kf:   r = res_src[n, p * res_stride, q * res_stride, col - res_clo]
 *             where res_clo <= col < res_clo + res_c, and r = +0.0f elsewhere.  The addition v + r IS performed for the zero columns as
 *             well (-0 + +0 = +0, exactly what adding the materialised padding gives); columns Kf .. K - 1 get no addition and no
 *             fp32 store, as in _narrow.  Everything behind the addition is _narrow's order: ReLU / ReLU6, store, quantiser.
 * DLMCQ_EINVAL for anything _narrow refuses and for: res_src == NULL; res_stride < 1; res_h or res_w < 1; P != ceil(res_h / res_stride)
 * or Q != ceil(res_w / res_stride) (the condition under which no output pixel reads outside the source); res_c < 4; res_c % 4 != 0;
 * res_clo % 4 != 0; res_clo < 0; res_clo + res_c > Kf (multiples of 4 keep every shortcut access a 16-byte one: a quad is wholly inside
 * the source or wholly zero); DLMCQ_PIPELINED or either DLMCQ_FP32_*_CHUNK_MAJOR bit.  w_offset == NULL selects symmetric weights.
 * Always conv_i8_mfma_kernel (its PADRES instantiations): DLMCQ_ROUTE_ONLY answers DLMCQ_ROUTE_TILED and launches nothing,
 * DLMCQ_FORCE_TILED changes nothing, DLMCQ_EMIT_SHIFT128 as in _fused.  Bit for bit what _narrow gives on the materialised shortcut. */
int dlmcq_conv2d_i8_nhwc_padres(const void* x, const int8_t* w, float* out, const float* bias, const int32_t* wsum,
                                const float* in_scale, const float* in_zero_point, const float* w_scale, const float* w_offset,
                                int64_t N, int64_t H, int64_t W, int64_t C, int64_t K, int64_t R, int64_t S, int32_t stride,
                                int32_t pad, int32_t dilation, int32_t x_is_unsigned, const float* res_src, int64_t res_h,
                                int64_t res_w, int64_t res_c, int32_t res_stride, int64_t res_clo, int32_t relu, void* codes,
                                const float* q_scale, const float* q_zero_point, int32_t q_lo, int32_t q_hi, int32_t q_form,
                                float q_ste_g, int64_t Kf, dlmcq_stream_t stream);

/* Depthwise 3x3 convolution (groups = channels; the MobileOne / MobileNet unit, modules/conv.py:13-19 with `groups`) on
 * activation codes, HBM-bound (1 byte in, 1 byte out): plain vector arithmetic, no matrix cores.  x: NHWC codes (uint8 if
 * x_is_unsigned), C % 4 == 0; w: int8 codes [R*S][C] (tap-major); per-channel w_scale and optional w_offset (asymmetric
 * weights as above), bias; zero padding (x' = 0).  Epilogue as dlmcq_conv2d_i8_nhwc_fused: ReLU or ReLU6, fp32 NHWC out and / or the
 * consumer's codes.   out = s_in * ( s_w[c] * SUM (q - zp) * qw  +  o_w[c] * SUM (q - zp) ) + bias[c]   (exact integer sums). */
int dlmcq_conv2d_dw_i8_nhwc(const void* x, const int8_t* w, float* out, const float* bias, const float* in_scale,
                            const float* in_zero_point, const float* w_scale, const float* w_offset, int64_t N, int64_t H,
                            int64_t W, int64_t C, int64_t R, int64_t S, int32_t stride, int32_t pad, int32_t x_is_unsigned,
                            int32_t relu, void* codes, const float* q_scale, const float* q_zero_point, int32_t q_lo,
                            int32_t q_hi, int32_t q_form, float q_ste_g, dlmcq_stream_t stream);

/* Depthwise 5x5 convolution with padding 2 and stride 1 or 2 (the 5x5 layers of the MBConv family) on the integer dot-product path
 * (csrc/conv_dw5_i8.hip): the arguments of dlmcq_conv2d_dw_i8_nhwc without R, S, the same arithmetic, and bit for bit the result that call gives
 * for R = S = 5 - for an INTEGER input zero point in the byte range (the kernel reads (int)in_zero_point[0], as the 3x3 kernels do).
 * C % 16 == 0, C <= 2048, stride 1 or 2, pad == 2 (DLMCQ_EINVAL otherwise); x and codes 16-byte aligned, the per-channel arrays and out as in
 * dlmcq_conv2d_dw_i8_nhwc (DLMCQ_EALIGN otherwise); the other checks are that entry point's, in its order (N == 0: DLMCQ_OK, nothing launched).
 * Control bits in q_form: DLMCQ_ROUTE_ONLY | DLMCQ_ROUTE_DW_VARIANT together validate, launch nothing and answer the instantiation
 * (DLMCQ_ROUTE_DW5_VARIANT_TAG); either alone, DLMCQ_FORCE_TILED and every other bit are DLMCQ_EINVAL.  No float activation offset. */
int dlmcq_conv2d_dw5_i8_nhwc(const void* x, const int8_t* w, float* out, const float* bias, const float* in_scale,
                             const float* in_zero_point, const float* w_scale, const float* w_offset, int64_t N, int64_t H,
                             int64_t W, int64_t C, int32_t stride, int32_t pad, int32_t x_is_unsigned, int32_t relu, void* codes,
                             const float* q_scale, const float* q_zero_point, int32_t q_lo, int32_t q_hi, int32_t q_form, float q_ste_g,
                             dlmcq_stream_t stream);

/*
 * A MobileOne / MobileNet unit as ONE launch (round 4): depthwise 3x3 / stride 1 / pad 1 (+ ReLU + quantiser) followed by the
 * pointwise 1x1 convolution that reads nothing but its codes (+ ReLU + the consumer's quantiser): dlmcq_conv2d_dw_i8_nhwc followed
 * by dlmcq_conv2d_i8_nhwc_asym / _fused with codes-only output, same integers, same fp32 chains, same quantisers - bit-identical -
 * but the wide code tensor between the two layers stays in LDS (csrc/conv_dwpw_i8.hip).
 *   dlmcq_dwpw_pack_table   the depthwise layer's constants (w: int8 codes [9][C] tap-major, per-channel w_scale, optional w_offset
 *                           and bias, the layer's input scale / zero point) -> `table`: C * 32 bytes, 16-byte aligned, C % 64 == 0.
 *                           Made once per (layer, input scale): what conv_dw3_i8_kernel builds per workgroup.
 *   dlmcq_conv2d_dwpw_i8_nhwc   x: NHWC codes [N][H][W][C] (uint8 if x_is_unsigned), W <= 61; (q_*): the depthwise output's
 *                           quantiser = the pointwise layer's input quantiser, range [0, 255]; pw_in_scale: the scale the pointwise
 *                           layer dequantises with (= q_scale, or its grad_scale value for QBase); w: int8 [K][C], K in {128, 192,
 *                           512}, with wsum / w_scale / optional w_offset / bias [K]; codes: [N][H][W][K] under (q2_*).
 *                           dw_relu or relu = DLMCQ_ACT_RELU6: DLMCQ_EINVAL.
 */
int dlmcq_dwpw_pack_table(const int8_t* w, const float* bias, const float* in_scale, const float* in_zero_point,
                          const float* w_scale, const float* w_offset, int64_t C, int32_t x_is_unsigned, void* table,
                          dlmcq_stream_t stream);
int dlmcq_conv2d_dwpw_i8_nhwc(const void* x, const void* dw_table, int32_t dw_asym, int32_t dw_bias, int32_t dw_relu,
                              const float* in_zero_point, int64_t N, int64_t H, int64_t W, int64_t C, int32_t x_is_unsigned,
                              const float* q_scale, const float* q_zero_point, int32_t q_lo, int32_t q_hi, int32_t q_form,
                              float q_ste_g, const int8_t* w, const float* bias, const int32_t* wsum, const float* pw_in_scale,
                              const float* w_scale, const float* w_offset, int64_t K, int32_t relu, void* codes,
                              const float* q2_scale, const float* q2_zero_point, int32_t q2_lo, int32_t q2_hi, int32_t q2_form,
                              float q2_ste_g, dlmcq_stream_t stream);

/*
 * Two convolutions into ONE output: out = conv(x, w) + conv(x2, w2), each dequantised with its own scales and bias
 * and summed in fp32 (one addition, as `out += identity` does it in a residual block whose shortcut is a
 * convolution), then the epilogue of dlmcq_conv2d_i8_nhwc_fused (relu = DLMCQ_ACT_RELU6: DLMCQ_EINVAL).  Both pairs must give the same [N, P, Q, K] output;
 * the second pair has its own input size, channel count, filter size, stride, padding and dilation (the 1x1/2
 * downsample next to the block's last 1x1).  Neither addend is written to memory.
 */
int dlmcq_conv2d_i8_nhwc_dual(const void* x, const int8_t* w, float* out, const float* bias,
                              const int32_t* wsum, const float* in_scale, const float* in_zero_point,
                              const float* w_scale, int64_t N, int64_t H, int64_t W, int64_t C, int64_t K,
                              int64_t R, int64_t S, int32_t stride, int32_t pad, int32_t dilation,
                              int32_t x_is_unsigned, const void* x2, const int8_t* w2, const float* bias2,
                              const int32_t* wsum2, const float* in_scale2, const float* in_zero_point2,
                              const float* w_scale2, int64_t H2, int64_t W2, int64_t C2, int64_t R2,
                              int64_t S2, int32_t stride2, int32_t pad2, int32_t dilation2,
                              int32_t x2_is_unsigned, int32_t relu, void* codes, const float* q_scale,
                              const float* q_zero_point, int32_t q_lo, int32_t q_hi, int32_t q_form,
                              float q_ste_g, dlmcq_stream_t stream);

/*
 * A residual block's LAST 1x1 convolution and the NEXT block's FIRST 1x1 convolution as one kernel
 * (csrc/conv_chain_i8.hip):
 *     v      = conv1x1(x, w) + bias + residual;  ReLU (if relu);  out = v (optional);  codes = Q(v) (optional)
 *     codes2 = Q2( ReLU?( conv1x1( Q(v), w2 ) + bias2 ) )
 * i.e. dlmcq_conv2d_i8_nhwc_fused on [M, C] -> [M, K] (stride 1, no padding) followed by the same call on its `codes`
 * with [K2, K] weights, `relu2` and the second consumer's quantiser Q2 - bit-identical to those two calls - but the
 * [M, K] code tensor stays in LDS: it is not read back, and not written unless `codes` is given.  M = N*H*W pixels;
 * x: [M][C] codes; w: [K][C]; residual (required) / out: fp32 [M][K]; w2: [K2][K]; codes2: [M][K2].
 * Q must be an unsigned 8-bit quantiser (q_lo = 0, q_hi = 255: the second reduction reads uint8 codes).
 * Supported: (C, K2) in {(64,64), (64,128), (128,128), (128,256), (256,256)}, K % 64 == 0, M*K*4 < 2^31 - 64 Ki
 * (anything else: DLMCQ_EINVAL / DLMCQ_ERANGE; callers fall back to the two separate calls).  relu or relu2 = DLMCQ_ACT_RELU6: DLMCQ_EINVAL.
 * rows_per_tile: pixels per workgroup, 1..64; <= 0: 64.  x, w, w2, residual, out, codes and codes2 must be 16-byte aligned
 * (DLMCQ_EALIGN otherwise).
 */
int dlmcq_conv2d_i8_nhwc_chain(const void* x, const int8_t* w, float* out, const float* bias, const int32_t* wsum,
                               const float* in_scale, const float* in_zero_point, const float* w_scale, int64_t M,
                               int64_t C, int64_t K, int32_t x_is_unsigned, const float* residual, int32_t relu,
                               void* codes, const float* q_scale, const float* q_zero_point, int32_t q_lo,
                               int32_t q_hi, int32_t q_form, float q_ste_g, const int8_t* w2, const float* bias2,
                               const int32_t* wsum2, const float* w_scale2, int64_t K2, int32_t relu2, void* codes2,
                               const float* q2_scale, const float* q2_zero_point, int32_t q2_lo, int32_t q2_hi,
                               int32_t q2_form, float q2_ste_g, int32_t rows_per_tile, dlmcq_stream_t stream);

/*
 * dlmcq_conv2d_i8_nhwc_chain for a block whose shortcut is itself a 1x1 convolution (the first block of a stage): the
 * first layer is dlmcq_conv2d_i8_nhwc_dual restricted to two 1x1 convolutions,
 *     v = conv1x1(x, w) + bias  +  conv1x1(x2 sampled at stride2, w2) + bias2;  ReLU;  out = v (optional);  codes = Q(v) (optional)
 *     codes3 = Q3( ReLU?( conv1x1( Q(v), w3 ) + bias3 ) )
 * bit-identical to dlmcq_conv2d_i8_nhwc_dual followed by dlmcq_conv2d_i8_nhwc_fused on its codes.  x: [N][H][W][C] codes
 * (stride 1); x2: [N][H2][W2][C2] codes with (H2 - 1) / stride2 + 1 == H (likewise W); w: [K][C]; w2: [K][C2]; w3: [K3][K].
 * Supported: (C, C2, K3) in {(64, 64, 64), (128, 256, 128)}; K % 64 == 0; N*H*W*K*4 < 2^31 - 64 Ki.  relu or relu3 = DLMCQ_ACT_RELU6: DLMCQ_EINVAL.
 */
int dlmcq_conv2d_i8_nhwc_dual_chain(const void* x, const int8_t* w, float* out, const float* bias, const int32_t* wsum,
                                    const float* in_scale, const float* in_zero_point, const float* w_scale, int64_t N,
                                    int64_t H, int64_t W, int64_t C, int64_t K, int32_t x_is_unsigned, const void* x2,
                                    const int8_t* w2, const float* bias2, const int32_t* wsum2, const float* in_scale2,
                                    const float* in_zero_point2, const float* w_scale2, int64_t H2, int64_t W2, int64_t C2,
                                    int32_t stride2, int32_t x2_is_unsigned, int32_t relu, void* codes, const float* q_scale,
                                    const float* q_zero_point, int32_t q_lo, int32_t q_hi, int32_t q_form, float q_ste_g,
                                    const int8_t* w3, const float* bias3, const int32_t* wsum3, const float* w_scale3,
                                    int64_t K3, int32_t relu3, void* codes3, const float* q3_scale, const float* q3_zero_point,
                                    int32_t q3_lo, int32_t q3_hi, int32_t q3_form, float q3_ste_g, int32_t rows_per_tile,
                                    dlmcq_stream_t stream);

/*
 * dlmcq_conv2d_i8_nhwc_chain whose fp32 shortcut is not read but RECOMPUTED: the shortcut is the output of a block of the
 * dlmcq_conv2d_i8_nhwc_dual_chain kind (the first block of a stage), handed over as that block's operands,
 *     r      = conv1x1(xa, wa) + biasa  +  conv1x1(xb sampled at strideb, wb) + biasb;  ReLU (if relu_shortcut)
 *     v      = conv1x1(x, w) + bias + r;  ReLU (if relu);  out = v (optional);  codes = Q(v) (optional)
 *     codes2 = Q2( ReLU?( conv1x1( Q(v), w2 ) + bias2 ) )
 * r is computed per 64-channel chunk by the instructions dlmcq_conv2d_i8_nhwc_dual_chain computes its fp32 output with, in their order,
 * so the call is bit-identical to dlmcq_conv2d_i8_nhwc_chain reading that call's `out` as `residual` - for Ca + Cb bytes of codes per pixel
 * instead of 4 K bytes of fp32, and the first call then needs no fp32 output.  x: [N][H][W][C] codes; xa: [N][H][W][Ca]; xb: [N][Hb][Wb][Cb]
 * with (Hb - 1) / strideb + 1 == H (likewise Wb); w: [K][C]; wa: [K][Ca]; wb: [K][Cb]; w2: [K2][K].  out is chunk-major under
 * DLMCQ_FP32_OUT_CHUNK_MAJOR in q2_form (DLMCQ_W2_CHUNK_MAJOR as in the other chain calls).
 * Supported: (C, Ca, Cb, K2) = (64, 64, 64, 64) (ResNet-50's stage 1), K % 64 == 0, N*H*W*K*4 < 2^31 - 64 Ki, relu != 0, and both quantisers
 * plain ones (forms ZEROPOINT / SYMMETRIC with an integer zero point, as the plan's are; there is no run-time-flag form of this kernel) -
 * anything else: DLMCQ_EINVAL / DLMCQ_ERANGE, and callers run dlmcq_conv2d_i8_nhwc_chain on the stored tensor.  relu_shortcut, relu or
 * relu2 = DLMCQ_ACT_RELU6: DLMCQ_EINVAL.  Pointer and alignment rules as for the other two chain calls.
 */
int dlmcq_conv2d_i8_nhwc_recompute_chain(
    const void* x, const int8_t* w, float* out, const float* bias, const int32_t* wsum, const float* in_scale, const float* in_zero_point,
    const float* w_scale, int64_t N, int64_t H, int64_t W, int64_t C, int64_t K, int32_t x_is_unsigned, const void* xa, const int8_t* wa,
    const float* biasa, const int32_t* wsuma, const float* in_scalea, const float* in_zero_pointa, const float* w_scalea, int64_t Ca,
    int32_t xa_is_unsigned, const void* xb, const int8_t* wb, const float* biasb, const int32_t* wsumb, const float* in_scaleb,
    const float* in_zero_pointb, const float* w_scaleb, int64_t Hb, int64_t Wb, int64_t Cb, int32_t strideb, int32_t xb_is_unsigned,
    int32_t relu_shortcut, int32_t relu, void* codes, const float* q_scale, const float* q_zero_point, int32_t q_lo, int32_t q_hi,
    int32_t q_form, float q_ste_g, const int8_t* w2, const float* bias2, const int32_t* wsum2, const float* w_scale2, int64_t K2,
    int32_t relu2, void* codes2, const float* q2_scale, const float* q2_zero_point, int32_t q2_lo, int32_t q2_hi, int32_t q2_form,
    float q2_ste_g, int32_t rows_per_tile, dlmcq_stream_t stream);

/* ---- the 3-channel first layer and its max-pool, in the integer-code domain (csrc/conv_stem_i8.hip) ---- */

/*
 * Quantise an image batch (C <= 4 channels, any memory format: element strides given) to activation codes in a
 * zero-point-PADDED NHWC buffer with 4 bytes per pixel: out[N][H+2*pad][W+2*pad][4], border = the code of
 * x' = 0 (zero padding of the fake-quantised image, modules/conv.py:18-19), bytes c >= C unspecified.
 * Forms EMULATE / QBASE / ZEROPOINT / SYMMETRIC as in dlmcq_fake_quant_f32 (same arithmetic, same codes).
 * The consumer over-reads up to 32 bytes past the last pixel: allocate N*(H+2*pad)*(W+2*pad)*4 + 32 bytes.
 */
int dlmcq_quantize_pad_nhwc4(const float* x, void* out, const float* scale, const float* zero_point, int64_t N,
                             int64_t C, int64_t H, int64_t W, int64_t stride_n, int64_t stride_c, int64_t stride_h,
                             int64_t stride_w, int32_t pad, int32_t lo, int32_t hi, int32_t form, float ste_g,
                             dlmcq_stream_t stream);

/* Weights fp32 KCRS (C <= 4, R <= 7, S <= 8) -> int8 [K][R][8][4] zero-filled, SYMMETRIC form, + wsum[K]. */
int dlmcq_quantize_weight_stem_i8(const float* w, int8_t* wq, int32_t* wsum, const float* scale, int64_t K,
                                  int64_t C, int64_t R, int64_t S, int32_t lo, int32_t hi, dlmcq_stream_t stream);

/*
 * The convolution of modules/conv.py:18-19 for such a layer: out[n,p,q,k] = in_scale*w_scale[k]*SUM (x - zp)*wq
 * + bias[k] over the padded codes (P = (Hp - R)/stride + 1, Q = (Wp - S)/stride + 1, dilation 1), then the
 * epilogue of dlmcq_conv2d_i8_nhwc_fused (ReLU or ReLU6, fp32 NHWC output and / or the consumer's codes).  K % 4 == 0.
 */
int dlmcq_conv2d_i8_stem_fused(const void* xpad, const int8_t* w, float* out, const float* bias,
                               const int32_t* wsum, const float* in_scale, const float* in_zero_point,
                               const float* w_scale, int64_t N, int64_t Hp, int64_t Wp, int64_t K, int64_t R,
                               int64_t S, int32_t stride, int32_t x_is_unsigned, int32_t relu, void* codes,
                               const float* q_scale, const float* q_zero_point, int32_t q_lo, int32_t q_hi,
                               int32_t q_form, float q_ste_g, dlmcq_stream_t stream);

/* dlmcq_conv2d_i8_stem_fused for ASYMMETRIC per-output-channel weights (as dlmcq_conv2d_i8_nhwc_asym: w' = qw * s_w[k] + o_w[k]):
 * the term o_w[k] * SUM x' comes from a per-pixel sum of the operand codes over the R x S taps and the C real channels
 * (C <= 4: the 4th byte of a pixel and the taps beyond S are excluded by a 0/1 byte mask). */
int dlmcq_conv2d_i8_stem_asym(const void* xpad, const int8_t* w, float* out, const float* bias, const int32_t* wsum,
                              const float* in_scale, const float* in_zero_point, const float* w_scale, const float* w_offset,
                              int64_t C, int64_t N, int64_t Hp, int64_t Wp, int64_t K, int64_t R, int64_t S, int32_t stride,
                              int32_t x_is_unsigned, int32_t relu, void* codes, const float* q_scale, const float* q_zero_point,
                              int32_t q_lo, int32_t q_hi, int32_t q_form, float q_ste_g, dlmcq_stream_t stream);

/*
 * dlmcq_conv2d_i8_stem_fused followed by ReLU (if asked) and nn.MaxPool2d(3, 2, 1) in ONE kernel, K <= 64: out / codes
 * are the POOLED tensor [N, (P+1)/2.., (Q+1)/2.., K]; relu = DLMCQ_ACT_RELU6: DLMCQ_EINVAL.  The pool runs on the fp32 values (the reference's order: ReLU,
 * max-pool, fake-quant; NaN propagates as in torch), so only the pooled quarter of the outputs is quantised and
 * nothing un-pooled is ever written.
 */
int dlmcq_conv2d_i8_stem_pool_fused(const void* xpad, const int8_t* w, float* out, const float* bias,
                                    const int32_t* wsum, const float* in_scale, const float* in_zero_point,
                                    const float* w_scale, int64_t N, int64_t Hp, int64_t Wp, int64_t K, int64_t R,
                                    int64_t S, int32_t stride, int32_t x_is_unsigned, int32_t relu, void* codes,
                                    const float* q_scale, const float* q_zero_point, int32_t q_lo, int32_t q_hi,
                                    int32_t q_form, float q_ste_g, dlmcq_stream_t stream);

/*
 * nn.MaxPool2d (square window, dilation 1, floor mode) on NHWC activation codes.  The quantisers of this library
 * are monotone, so  code(maxpool(v)) == maxpool(code(v)):  pooling the 1-byte codes replaces pooling the fp32
 * tensor and quantising the result.  C % 4 == 0; padding never wins (torch pads with -inf).
 */
int dlmcq_maxpool_codes_nhwc(const void* x, void* y, int64_t N, int64_t H, int64_t W, int64_t C, int32_t kernel,
                             int32_t stride, int32_t pad, int32_t x_is_unsigned, dlmcq_stream_t stream);

/* ---- float activation offsets: the *_xoff convolution entry points ----
 * A QBase activation quantiser with a per-tensor FLOAT offset o (x^ = q * s^ + o, modules/base.py:96-102; ops.py:20-34 sets
 * o = min(x) for unsigned ranges) has no integer zero point, and zero padding pads x^ with 0, which is no code.  With
 * T[k](p,q) = SUM over the IN-BOUNDS taps (r,s) of tap[k][r][s], tap[k][r][s] = SUM_c (real channels) w^[k,c,r,s]:
 *     out[n,p,q,k] = s^ * SUM_in q * w^  +  o * T[k](p,q)  +  bias[k]
 * The first term is what the fused / _asym calls compute (the caller passes `in_zero_point` as for integer codes - usually NULL - and
 * pads with that zero point's code: padded taps then add exactly 0).  The caller folds o * SUM_{all taps} tap[k] into `bias` (build
 * time; `bias` must not be NULL then), and these entry points subtract  o * SUM_{out-of-bounds taps} tap[k][r][s]  at border pixels
 * only, as ONE fused multiply-add after the bias and weight-offset terms, before residual / activation / quantiser.  The border sum
 * is taken in fp32, r-major, s ascending.
 *   in_offset: device fp32 scalar o.  tap_sums: device fp32 [R * S][K] (16-byte aligned), tap-major.  Both non-NULL (else EINVAL).
 *   w_offset: NULL for symmetric weights, else as in the _asym calls.
 * Unpadded layers (pad = 0) have no border: the call is then the fused / _asym call itself (in_offset and tap_sums unused).
 * Routes: dlmcq_conv2d_i8_nhwc_xoff runs on conv_i8_mfma_kernel (unswapped epilogue, 64 / 128-channel tiles): the halo-tile, pipelined
 * 3x3 and pointwise kernels decline it (DLMCQ_ROUTE_ONLY answers DLMCQ_ROUTE_TILED); no dual form.  dlmcq_conv2d_dw_i8_nhwc_xoff:
 * 3 x 3 layers with C % 16 == 0, C <= 2048, 16-byte-aligned codes (the two vector kernels; the matrix-core depthwise kernel
 * declines: DLMCQ_ROUTE_DW), anything else EINVAL.  dlmcq_conv2d_i8_stem_xoff: R = 3 or 7 (unswapped epilogue), `pad` = the padding
 * of the NHWC4 buffer (dlmcq_quantize_pad_nhwc4 with DLMCQ_PAD_CODE0), `C` the image's real channels; no pooling form.  DLMCQ_ACT_*
 * as in the fused calls.  No offset variant exists for the pooling first layer, dwpw, chain, dual or dual-chain calls. */
int dlmcq_conv2d_i8_nhwc_xoff(const void* x, const int8_t* w, float* out, const float* bias, const int32_t* wsum,
                              const float* in_scale, const float* in_zero_point, const float* w_scale, const float* w_offset,
                              int64_t N, int64_t H, int64_t W, int64_t C, int64_t K, int64_t R, int64_t S, int32_t stride,
                              int32_t pad, int32_t dilation, int32_t x_is_unsigned, const float* residual, int32_t relu, void* codes,
                              const float* q_scale, const float* q_zero_point, int32_t q_lo, int32_t q_hi, int32_t q_form,
                              float q_ste_g, const float* in_offset, const float* tap_sums, dlmcq_stream_t stream);
int dlmcq_conv2d_dw_i8_nhwc_xoff(const void* x, const int8_t* w, float* out, const float* bias, const float* in_scale,
                                 const float* in_zero_point, const float* w_scale, const float* w_offset, int64_t N, int64_t H,
                                 int64_t W, int64_t C, int64_t R, int64_t S, int32_t stride, int32_t pad, int32_t x_is_unsigned,
                                 int32_t relu, void* codes, const float* q_scale, const float* q_zero_point, int32_t q_lo,
                                 int32_t q_hi, int32_t q_form, float q_ste_g, const float* in_offset, const float* tap_sums,
                                 dlmcq_stream_t stream);
int dlmcq_conv2d_i8_stem_xoff(const void* xpad, const int8_t* w, float* out, const float* bias, const int32_t* wsum,
                              const float* in_scale, const float* in_zero_point, const float* w_scale, const float* w_offset,
                              int64_t C, int64_t N, int64_t Hp, int64_t Wp, int64_t K, int64_t R, int64_t S, int32_t stride,
                              int32_t pad, int32_t x_is_unsigned, int32_t relu, void* codes, const float* q_scale,
                              const float* q_zero_point, int32_t q_lo, int32_t q_hi, int32_t q_form, float q_ste_g,
                              const float* in_offset, const float* tap_sums, dlmcq_stream_t stream);

/* ---- global-average-pool heads: the pooled output as fp32 and / or the classifier's activation codes ----
 * One arithmetic for both entry points.  For image n and channel k, over the HW pixels p = 0 .. HW - 1 in NHWC row order:
 *     s = v[n,0,k];  for p = 1 .. HW - 1: s = fl32(s + v[n,p,k]);  pooled[n,k] = fl32(s / fl32(HW))  (true IEEE division)
 *     code[n,k] = the quantiser (q_scale .. q_ste_g, as in dlmcq_conv2d_i8_nhwc_fused; DLMCQ_EMIT_SHIFT128 accepted) of pooled[n,k] -
 *                 the code dlmcq_fake_quant_f32 gives for it
 * A sequential fp32 sum, no atomics: the result depends neither on the launch geometry nor on the run.  (torch.mean sums in another
 * order: equal to it only within HW * 2^-24 * mean|v|.)  `pooled` (fp32 [N, C]) and `codes` ([N, C] bytes) are optional, at least one
 * is required; `codes` needs q_scale.
 *
 * dlmcq_gap_nhwc_f32: x fp32 [N, HW, C] row-major NHWC (16-byte aligned), C % 4 == 0, HW >= 1.  One read of the map, no scratch.
 * Every control / layout bit in q_form (a chunk-major input, DLMCQ_ROUTE_ONLY, ...) is DLMCQ_EINVAL.
 *
 * dlmcq_conv2d_i8_nhwc_gap: v is the output of the 1 x 1 / stride 1 / unpadded convolution of dlmcq_conv2d_i8_nhwc_fused (same
 * operands: codes x [N, H, W, C], weights [K, C], symmetric; in_zero_point as there - also the `zp - 128` of shifted codes passed as
 * signed; a float activation offset is folded into `bias` by the caller, an unpadded layer has no border term) + `residual` (fp32
 * [N, H, W, K] row-major or NULL) + `act` (DLMCQ_ACT_NONE / RELU / RELU6), bit for bit the value that call stores - but the
 * [N, H, W, K] map is never written: one launch produces pooled / codes.  Supported: C % 64 == 0, C <= DLMCQ_GAP_MAX_C (the slice's
 * weights stay in LDS), K % 64 == 0, H * W <= 64; anything else DLMCQ_EINVAL.  DLMCQ_ROUTE_ONLY in q_form: validates, launches
 * nothing, returns DLMCQ_ROUTE_GAP; every other control / layout bit is DLMCQ_EINVAL (refused, not stripped). */
#define DLMCQ_GAP_MAX_C 2048
int dlmcq_gap_nhwc_f32(const float* x, float* pooled, void* codes, int64_t N, int64_t HW, int64_t C, const float* q_scale,
                       const float* q_zero_point, int32_t q_lo, int32_t q_hi, int32_t q_form, float q_ste_g, dlmcq_stream_t stream);
int dlmcq_conv2d_i8_nhwc_gap(const void* x, const int8_t* w, float* pooled, const float* bias, const int32_t* wsum,
                             const float* in_scale, const float* in_zero_point, const float* w_scale, int64_t N, int64_t H,
                             int64_t W, int64_t C, int64_t K, int32_t x_is_unsigned, const float* residual, int32_t act,
                             void* codes, const float* q_scale, const float* q_zero_point, int32_t q_lo, int32_t q_hi,
                             int32_t q_form, float q_ste_g, dlmcq_stream_t stream);

/* ---- windowed average pool (nn.AvgPool2d(s, s): window = stride, no padding, floor): fp32 and / or the consumer's activation codes ----
 * For image n, output pixel (p, q), channel c, with s = window, P = H / s, Q = W / s (floor: trailing rows / columns are dropped):
 *     a = +0.0f;  for dy = 0 .. s-1: for dx = 0 .. s-1: a = fl32(a + x[n, p*s + dy, q*s + dx, c]);  pooled = fl32(a / fl32(s*s))
 *     code = the quantiser (q_scale .. q_ste_g, as in dlmcq_conv2d_i8_nhwc_fused; DLMCQ_EMIT_SHIFT128 accepted) of pooled - the code
 *            dlmcq_fake_quant_f32 gives for it
 * A sequential fp32 sum from +0 in row-major window order and a true IEEE division - the loop of torch's avg_pool2d, bit for bit; no
 * atomics, no scratch: the result depends neither on the launch geometry nor on the run.
 *   x        fp32 [N, H, W, x_stride] row-major, of which channels 0 .. C - 1 are read (x_stride >= C, x_stride % 4 == 0: the channel
 *            slice of a wider NHWC tensor is read in place), 16-byte aligned
 *   pooled   fp32 [N, P, Q, C] dense, 16-byte aligned, or NULL
 *   codes    bytes [N, P, Q, c_pad], 4-byte aligned, or NULL (needs q_scale); c_pad >= C, c_pad % 4 == 0; channels C .. c_pad - 1 receive
 *            the byte `pad_code` (-128 .. 255, its low 8 bits are stored as given: the caller passes the consumer's zero point, code 0
 *            under a float activation offset, or either minus 128 beside DLMCQ_EMIT_SHIFT128)
 * DLMCQ_EINVAL: window < 2, window > 8, H < window, W < window, C < 4, C % 4, x_stride < C, x_stride % 4, c_pad < C, c_pad % 4, pad_code
 * outside -128 .. 255, both outputs NULL, c_pad != C without codes, an invalid quantiser, any control or layout bit in q_form (refused,
 * not stripped).  DLMCQ_EALIGN: x / pooled not 16-byte aligned, codes not 4-byte aligned.  DLMCQ_ERANGE: N * P * Q * c_pad / 4 or H * W
 * reaches 2^31.  N == 0: DLMCQ_OK, nothing launched. */
int dlmcq_avgpool_nhwc_f32(const float* x, float* pooled, void* codes, int64_t N, int64_t H, int64_t W, int64_t C, int64_t x_stride,
                           int64_t window, int64_t c_pad, int32_t pad_code, const float* q_scale, const float* q_zero_point,
                           int32_t q_lo, int32_t q_hi, int32_t q_form, float q_ste_g, dlmcq_stream_t stream);

/* ---- squeeze-excite channel gate x * g (+ ReLU / ReLU6): fp32 and / or the consumer's activation codes ----
 * For image n, pixel (h, w), channel c:
 *     v = fl32(x[n, h, w, c] * gate[n, c])    one IEEE multiply, rounded to fp32 before anything else reads it (never contracted into
 *                                             the quantiser's arithmetic)
 *     v = act(v)                              DLMCQ_ACT_NONE / DLMCQ_ACT_RELU / DLMCQ_ACT_RELU6: NaN stays NaN; -0 becomes +0 under ReLU and
 *                                             ReLU6 - torch's clamp kernels ON THE DEVICE (isnan(v) ? v : max(v, 0)), whose op this call
 *                                             replaces, not the CPU's v < 0 ? 0 : v of the convolution epilogues above
 *     out = v;  code = the quantiser (q_scale .. q_ste_g, as in dlmcq_conv2d_i8_nhwc_fused; DLMCQ_EMIT_SHIFT128 accepted) of v - the
 *                      code dlmcq_fake_quant_f32 gives for it
 * - torch's x * g.view(N, C, 1, 1) and its relu / relu6, element by element.  No atomics, no scratch: the result depends neither on the
 * launch geometry nor on the run.
 *   x        fp32 [N, H, W, x_stride] row-major, of which channels 0 .. C - 1 are read (x_stride >= C, x_stride % 4 == 0: the channel
 *            slice of a wider NHWC tensor is read in place), 16-byte aligned
 *   gate     fp32 [N, C] dense, 16-byte aligned
 *   out      fp32 [N, H, W, C] dense, 16-byte aligned, or NULL
 *   codes    bytes [N, H, W, c_pad], 4-byte aligned, or NULL (needs q_scale); c_pad >= C, c_pad % 4 == 0; channels C .. c_pad - 1 receive
 *            the byte `pad_code` (-128 .. 255, its low 8 bits are stored as given: the caller passes the consumer's zero point, code 0
 *            under a float activation offset, or either minus 128 beside DLMCQ_EMIT_SHIFT128)
 * DLMCQ_EINVAL: H < 1, W < 1, C < 4, C % 4, x_stride < C, x_stride % 4, c_pad < C, c_pad % 4, pad_code outside -128 .. 255, act outside
 * 0 .. 2, x or gate NULL, both outputs NULL, c_pad != C without codes, an invalid quantiser, any control or layout bit in q_form
 * (refused, not stripped).  DLMCQ_EALIGN: x / gate / out not 16-byte aligned, codes not 4-byte aligned.  DLMCQ_ERANGE: N * H * W *
 * c_pad / 4 reaches 2^31.  N == 0: DLMCQ_OK, nothing launched.  A refused call writes nothing. */
int dlmcq_gate_nhwc_f32(const float* x, const float* gate, float* out, void* codes, int64_t N, int64_t H, int64_t W, int64_t C,
                        int64_t x_stride, int64_t c_pad, int32_t pad_code, int32_t act, const float* q_scale, const float* q_zero_point,
                        int32_t q_lo, int32_t q_hi, int32_t q_form, float q_ste_g, dlmcq_stream_t stream);

/* ---- swish / SiLU x * sigmoid(x): fp32 and / or the consumer's activation codes ----
 * For image n, pixel (h, w), channel c, with x = x[n, h, w, c]:
 *     e = expf(-x)          the device library's accurate expf
 *     d = fl32(1 + e)       one IEEE add
 *     s = fl32(1 / d)       one IEEE division, correctly rounded
 *     v = fl32(x * s)       one IEEE multiply, rounded to fp32 before anything else reads it (never contracted into the quantiser's
 *                           arithmetic)
 *     out = v;  code = the quantiser (q_scale .. q_ste_g, as in dlmcq_conv2d_i8_nhwc_fused; DLMCQ_EMIT_SHIFT128 accepted) of v - the
 *                      code dlmcq_fake_quant_f32 gives for it
 * - the operation sequence of torch's x * torch.sigmoid(x), element by element; within 3 * 2^-23 relative of the real x * sigmoid(x) for
 * |x| <= 80.  x <= -88.8: v = -0; x = -inf: NaN (as -inf * 0); x = +inf: +inf; NaN stays NaN; denormals are kept.  There is no
 * activation argument.  No atomics, no scratch: the result depends neither on the launch geometry nor on the run.
 *   x        fp32 [N, H, W, x_stride] row-major, of which channels 0 .. C - 1 are read (x_stride >= C, x_stride % 4 == 0: the channel
 *            slice of a wider NHWC tensor is read in place), 16-byte aligned
 *   out      fp32 [N, H, W, C] dense, 16-byte aligned, or NULL
 *   codes    bytes [N, H, W, c_pad], 4-byte aligned, or NULL (needs q_scale); c_pad >= C, c_pad % 4 == 0; channels C .. c_pad - 1 receive
 *            the byte `pad_code` (-128 .. 255, its low 8 bits are stored as given: the caller passes the consumer's zero point, code 0
 *            under a float activation offset, or either minus 128 beside DLMCQ_EMIT_SHIFT128)
 * DLMCQ_EINVAL: H < 1, W < 1, C < 4, C % 4, x_stride < C, x_stride % 4, c_pad < C, c_pad % 4, pad_code outside -128 .. 255, x NULL, both
 * outputs NULL, c_pad != C without codes, an invalid quantiser, any control or layout bit in q_form (refused, not stripped).
 * DLMCQ_EALIGN: x / out not 16-byte aligned, codes not 4-byte aligned.  DLMCQ_ERANGE: N * H * W * c_pad / 4 reaches 2^31.  N == 0:
 * DLMCQ_OK, nothing launched.  A refused call writes nothing. */
int dlmcq_swish_nhwc_f32(const float* x, float* out, void* codes, int64_t N, int64_t H, int64_t W, int64_t C, int64_t x_stride,
                         int64_t c_pad, int32_t pad_code, const float* q_scale, const float* q_zero_point, int32_t q_lo, int32_t q_hi,
                         int32_t q_form, float q_ste_g, dlmcq_stream_t stream);

/* ---- hard swish x * relu6(x + 3) / 6: fp32 and / or the consumer's activation codes ----
 * For image n, pixel (h, w), channel c, with x = x[n, h, w, c]:
 *     t = fl32(x + 3)       one IEEE add
 *     r = relu6(t)          t > 0 ? t : (t is NaN ? t : +0), then r > 6 ? 6 : r - the device's clamp (NaN passes, -0 becomes +0), as
 *                           dlmcq_squeeze_gate_i8's DLMCQ_GATE_HARDSIGMOID
 *     c = fl32(1 / 6)       the constant 0x3E2AAAAB: a division by the host scalar 6 is this multiplication on the device
 *     order DLMCQ_HSWISH_MUL_FIRST:   v = fl32(fl32(x * r) * c)    nn.Hardswish, F.hardswish, (x * relu6(x + 3)) / 6
 *     order DLMCQ_HSWISH_GATE_FIRST:  v = fl32(x * fl32(r * c))    x * (relu6(x + 3) / 6), x * hardsigmoid(x)
 *     out = v;  code = the quantiser (q_scale .. q_ste_g, as in dlmcq_conv2d_i8_nhwc_fused; DLMCQ_EMIT_SHIFT128 accepted) of v - the
 *                      code dlmcq_fake_quant_f32 gives for it
 * - every step rounded to fp32 by itself, never contracted.  The two orders differ in the last bit of about a quarter of the elements;
 * either is within 5 * 2^-24 relative of the real x * clip(x + 3, 0, 6) / 6, and exactly 0 where that is 0.  x <= -3: v = -0; x = -0:
 * -0; x = -inf: NaN (as -inf * 0); x = +inf: +inf; NaN stays NaN; x >= 3: (x * 6) * c or x * (6 * c), which need not equal x;
 * x > FLT_MAX / 6: +inf under DLMCQ_HSWISH_MUL_FIRST (x * 6 overflows), finite under DLMCQ_HSWISH_GATE_FIRST; denormals are kept.
 * No atomics, no scratch: the result depends neither on the launch geometry nor on the run.
 * Arguments, layouts and return codes: exactly those of dlmcq_swish_nhwc_f32, plus `order`.  DLMCQ_EINVAL first of all for an order
 * outside 0 .. 1. */
#define DLMCQ_HSWISH_MUL_FIRST 0
#define DLMCQ_HSWISH_GATE_FIRST 1
int dlmcq_hardswish_nhwc_f32(const float* x, float* out, void* codes, int64_t N, int64_t H, int64_t W, int64_t C, int64_t x_stride,
                             int64_t c_pad, int32_t pad_code, const float* q_scale, const float* q_zero_point, int32_t q_lo, int32_t q_hi,
                             int32_t q_form, float q_ste_g, int32_t order, dlmcq_stream_t stream);

/* ---- the squeeze path of a squeeze-excite block: pooled activation codes [N, C] -> the fp32 gate [N, C], one launch ----
 * Two int8 layers on rows with an activation between them and the gate function behind them; the hidden vector stays on the chip.
 * For image n, hidden unit r (0 .. R4 - 1) and channel c (0 .. C - 1):
 *     S1 = SUM_c (x[n, c] - zp1) * w1[r, c]                 exact in int32; zp1 = in_zero_point1 (an integer value; NULL = 0)
 *     h  = fma(fl32(S1), fl32(in_scale1 * w_scale1[r]), bias1[r])      the rounding chain of dlmcq_conv2d_i8_nhwc_fused: ONE fused
 *                                                           multiply-add (bias1 NULL: + 0)
 *     h  = inner_act(h)     DLMCQ_SQUEEZE_NONE | DLMCQ_SQUEEZE_RELU: h < 0 ? 0 : h (NaN and -0 pass, as that entry point's ReLU) |
 *                           DLMCQ_SQUEEZE_SWISH: e = expf(-h), d = fl32(1 + e), s = fl32(1 / d), h = fl32(h * s) (dlmcq_swish_nhwc_f32's steps)
 *     hidden[n, r] = h
 *     qh = the quantiser (q_scale .. q_ste_g, forms EMULATE / QBASE / ZEROPOINT / SYMMETRIC as in dlmcq_conv2d_i8_nhwc_fused) of h - the
 *          code dlmcq_fake_quant_f32 gives for it; uint8 when q_lo >= 0, else int8
 *     S2 = SUM_r (qh - zp2) * w2[c, r]                      exact in int32; zp2 = q_zero_point as an integer zero point (NULL = 0) in
 *                                                           every form
 *     v  = fma(fl32(S2), fl32(s_h * w_scale2[c]), bias2[c])  s_h = the scale the form dequantises with: QBASE (s - s g) + s g, else q_scale
 *     gate[n, c] = gate_fn(v)   DLMCQ_GATE_NONE: v | DLMCQ_GATE_SIGMOID: e = expf(-v), d = fl32(1 + e), g = fl32(1 / d) - the accurate expf and
 *                           a correctly rounded division | DLMCQ_GATE_HARDSIGMOID: t = fl32(v + 3); t = t > 0 ? t : (t is NaN ? t : +0);
 *                           t = t > 6 ? 6 : t (relu6 as the device's clamp has it: NaN passes, -0 becomes +0); g = fl32(t * fl32(1 / 6)) -
 *                           `F.relu6(v + 3) / 6` as the device evaluates it, where a division by a host scalar is a multiplication by
 *                           its rounded reciprocal
 * - every step rounded to fp32 by itself; no atomics, no scratch: the result depends neither on the launch geometry nor on the run.
 * It is dlmcq_conv2d_i8_nhwc_fused (H = W = R = S = 1) on x, the activation, dlmcq_fake_quant_f32 and the same entry point again, bit
 * for bit, for layers too narrow for that entry point's 64-channel step.
 *   x          activation codes [N, C] (uint8 when x_is_unsigned, else int8), 4-byte aligned
 *   w1, wsum1  int8 [R4, C] (16-byte aligned) and its row sums [R4]; w2, wsum2: int8 [C, R4] (16-byte aligned) and its row sums [C].
 *              Symmetric weights.  R4 is the hidden width rounded up to a multiple of 4: the caller pads w1's rows, wsum1, bias1 and
 *              w2's columns with 0 (and w_scale1 with anything finite); a padded unit's code is multiplied by 0.
 *   bias1 [R4], bias2 [C] or NULL; in_scale1, in_zero_point1, q_scale, q_zero_point: device scalars; w_scale1 [R4], w_scale2 [C]
 *   gate       fp32 [N, C], hidden fp32 [N, R4] (the values behind inner_act), each 16-byte aligned or NULL; one of them is required.
 *              Without `gate` layer 2 is not computed.
 * DLMCQ_EINVAL: N < 0, C < 4, C > DLMCQ_SQUEEZE_MAX_C, C % 4, R4 < 1, R4 > DLMCQ_SQUEEZE_MAX_R, R4 % 4, inner_act or gate_fn outside
 * 0 .. 2; then an invalid quantiser (q_scale NULL included), any control or layout bit or DLMCQ_EMIT_SHIFT128 in q_form (refused, not
 * stripped), a code range that is neither a uint8 nor an int8 one (q_lo < 0 and q_hi > 127: the hidden codes are bytes that layer 2
 * reads as one or the other); then, unless N == 0 (DLMCQ_OK, nothing launched, null pointers included): both outputs NULL, a required input NULL.
 * DLMCQ_EALIGN: w1 / w2 / gate / hidden not 16-byte aligned, any other pointer not 4-byte aligned.  DLMCQ_ERANGE: N * C or N * R4
 * reaches 2^31.  A refused call writes nothing.  One workgroup computes DLMCQ_SQUEEZE_IMAGES images. */
#define DLMCQ_SQUEEZE_MAX_C 2048
#define DLMCQ_SQUEEZE_MAX_R 512
#define DLMCQ_SQUEEZE_IMAGES 4
#define DLMCQ_SQUEEZE_NONE 0
#define DLMCQ_SQUEEZE_RELU 1
#define DLMCQ_SQUEEZE_SWISH 2
#define DLMCQ_GATE_NONE 0
#define DLMCQ_GATE_SIGMOID 1
#define DLMCQ_GATE_HARDSIGMOID 2
int dlmcq_squeeze_gate_i8(const void* x, const int8_t* w1, const int32_t* wsum1, const float* bias1, const float* in_scale1,
                          const float* in_zero_point1, const float* w_scale1, int32_t inner_act, const int8_t* w2, const int32_t* wsum2,
                          const float* bias2, const float* w_scale2, int32_t gate_fn, float* gate, float* hidden, int64_t N, int64_t C,
                          int64_t R4, int32_t x_is_unsigned, const float* q_scale, const float* q_zero_point, int32_t q_lo, int32_t q_hi,
                          int32_t q_form, float q_ste_g, dlmcq_stream_t stream);

/* ---- GELU (erf form) 0.5 x (1 + erf(x / sqrt(2))): fp32 and / or the consumer's activation codes ----
 * For image n, pixel (h, w), channel c, with x = x[n, h, w, c] (dense rows [M, C]: N = M, H = W = 1):
 *     z = fl32(x * 0.70710678118654752440f)   one IEEE multiply by fl32(1 / sqrt(2))
 *     e = erff(z)                             the device library's accurate erff
 *     f = fl32(1 + e)                         one IEEE add
 *     h = fl32(x * 0.5f)
 *     v = fl32(h * f)                         one IEEE multiply, rounded to fp32 before anything else reads it (never contracted into
 *                                             the quantiser's arithmetic)
 *     out = v;  code = the quantiser (q_scale .. q_ste_g, as in dlmcq_conv2d_i8_nhwc_fused; DLMCQ_EMIT_SHIFT128 accepted) of v - the
 *                      code dlmcq_fake_quant_f32 gives for it
 * - the operation order of torch's device GELU kernel for approximate="none", element by element; with u = 2^-23 (|x| + |v*|) within
 * 2 u of the real v* = x Phi(x).  x <= about -5.9: v = -0; x = -inf: NaN (as -inf * 0); x = +inf: +inf; NaN stays NaN; denormals are
 * kept.  There is no tanh form.  No atomics, no scratch: the result depends neither on the launch geometry nor on the run.
 * Arguments, layouts and return codes: exactly those of dlmcq_swish_nhwc_f32. */
int dlmcq_gelu_nhwc_f32(const float* x, float* out, void* codes, int64_t N, int64_t H, int64_t W, int64_t C, int64_t x_stride,
                        int64_t c_pad, int32_t pad_code, const float* q_scale, const float* q_zero_point, int32_t q_lo, int32_t q_hi,
                        int32_t q_form, float q_ste_g, dlmcq_stream_t stream);

/* ---- LayerNorm over the last dimension of dense fp32 rows: fp32 and / or the consumer's activation codes ----
 * For row m, with x = x[m, 0 .. C - 1] as C / 4 quads of 4 floats, lane l (0 .. 63) owning quads l, l + 64, ...:
 *     q_j  = fl32(fl32(x0 + x1) + fl32(x2 + x3))   the lane's j-th quad (a quad past the row's end: +0)
 *     s_l  = the lane's q_j added pairwise in memory order, (q0 + q1) + (q2 + q3), ...: a balanced tree (1, 2, 4 or 8 quads: C <= 256,
 *            512, 1024, 2048), not a running sum - 32 equal values added one by one drift by several ulp, which the bound below has no
 *            room for
 *     S    =the 64 lane sums combined by an xor butterfly with strides 32, 16, 8, 4, 2, 1
 *     mean = fl32(S / (float)C)               a true division
 *     d    = fl32(x - mean)
 *     S2   = the same two-level sum of fl32(d * d)
 *     var  = fl32(S2 / (float)C)              the biased variance
 *     r    = fl32(1 / sqrtf(fl32(var + eps))) square root and division correctly rounded
 *     v    = fl32(fl32(fl32(d * r) * gamma[c]) + beta[c])      gamma NULL: no multiply; beta NULL: no add
 *     out = v;  code = the quantiser (q_scale .. q_ste_g, as in dlmcq_conv2d_i8_nhwc_fused) of v - the code dlmcq_fake_quant_f32 gives
 *                      for it.  The shifted emission is NOT accepted: the readers are Linear layers, which take plain codes.
 * - nn.LayerNorm((C,)) up to the summation order: with n = (x - mean) / sqrt(var + eps) in real arithmetic on the same fp32 inputs and
 * u = 2^-23 (|n gamma| + |beta| + |gamma| max_row|x| / sqrt(var + eps)), |v - (n gamma + beta)| <= 2 u.  A NaN or an infinity in a row
 * makes the whole row NaN.  No LDS, no atomics, no scratch: a row's result depends neither on M nor on its index nor on the launch.
 *   x        fp32 [M, C] dense, 16-byte aligned
 *   gamma    fp32 [C], 16-byte aligned, or NULL (no scale)
 *   beta     fp32 [C], 16-byte aligned, or NULL (no shift)
 *   out      fp32 [M, C] dense, 16-byte aligned, or NULL
 *   codes    bytes [M, C], 4-byte aligned, or NULL (needs q_scale)
 * DLMCQ_EINVAL: M < 0, C < 4, C % 4, C > 2048, eps not finite or not > 0, x NULL, both outputs NULL, an invalid quantiser, any control
 * or layout bit or DLMCQ_EMIT_SHIFT128 in q_form (refused, not stripped).  DLMCQ_EALIGN: x / gamma / beta / out not 16-byte aligned,
 * codes not 4-byte aligned.  DLMCQ_ERANGE: M or M * C / 4 reaches 2^31.  M == 0: DLMCQ_OK, nothing launched.  A refused call writes
 * nothing. */
int dlmcq_layernorm_rows_f32(const float* x, const float* gamma, const float* beta, float* out, void* codes, int64_t M, int64_t C,
                             float eps, const float* q_scale, const float* q_zero_point, int32_t q_lo, int32_t q_hi, int32_t q_form,
                             float q_ste_g, dlmcq_stream_t stream);

/* ---- Scaled dot-product attention softmax(scale q k^T) v: fp32 and / or the activation codes of the projection behind it ----
 * One flash forward per query tile (csrc/attention.hip): nothing of size Tq x Tk touches memory.  No mask, no causal flag, no dropout.
 * For query row i of one (b, h), keys j = 0 .. Tk - 1 in blocks of 32 (the online softmax's key block), u = 2^-24:
 *     a_ij = the k-ordered fmaf chain over D from +0 (v_mfma_f32_32x32x2_f32: bit for bit fmaf(q[D-1], k[D-1], ... fmaf(q[0], k[0], +0)))
 *     s_ij = fl32(a_ij * scale)               one IEEE multiply
 *     per key block, m the running maximum (-inf at first), keys past Tk - 1 holding s = -inf:
 *     m'   = max(m, max_j s_ij)               NaNs dropped by the maximum: a NaN score reaches p instead
 *     m~   = m', or 0 where m' = -inf
 *     al   = expf(fl32(m - m~))               the device library's accurate expf (1 ulp), not v_exp_f32
 *     p_ij = expf(fl32(s_ij - m~))
 *     l_h  = fl32(fl32(l_h * al) + t_h)       h = bit 2 of the key index; t_h: the half's 16 p_ij added one by one in ascending key order
 *     w_g  = the chain fmaf(v_j[c], p_ij, w_g) from +0 over the block's keys 8 g .. 8 g + 7 in the order 0 4 1 5 2 6 3 7 (+ 8 g), g = 0 .. 3
 *     o_ic = fl32(fl32(o_ic * al) + fl32(fl32(w_0 + w_1) + fl32(w_2 + w_3)))      chains of 8 and a tree: one chain over alike summands drifts
 *     at the end: l = fl32(l_0 + l_1), out_ic = fl32(o_ic / l)      a true division, correctly rounded
 *     out = out_ic;  code = the quantiser (q_scale .. q_ste_g, as in dlmcq_conv2d_i8_nhwc_fused) of out_ic - the code dlmcq_fake_quant_f32
 *                    gives for it.  The shifted emission is NOT accepted: the reader is a Linear layer, which takes plain codes.
 * Non-finite inputs give the NaNs of the unfused graph (matmul, multiply, softmax, matmul), element for element: a NaN in q_i makes
 * row i NaN and no other; a NaN in any k_j makes every row of the head NaN; a +inf score makes its row NaN; a NaN in v_j[c] makes
 * column c of every row of the head NaN and leaves the other columns finite.
 * Against real arithmetic on the same fp32 inputs (p*, o* real), with delta_i = (D + 1) u scale max_j sum_k |q_ik k_jk|, nb = ceil(Tk / 32)
 * and kappa = 2 (104 + 2 + 3 nb + 32 nb) + 1:
 *     |out_ic - o*_ic| <= (2 delta_i + kappa u) sum_j p*_ij |v_jc| + 2^-126 max_j |v_jc|
 * (csrc/attention.hip derives it: 104 is the largest m - s whose term is not 0 in fp32, the last summand stands for such terms).
 * No atomics, no scratch: a row's result depends neither on B, H, its (b, h) nor on the launch.
 *   q        fp32 view [B, H, Tq, D]: element strides q_sb, q_sh, q_st (batch, head, token), unit stride in D, 16-byte aligned
 *   k, v     fp32 views [B, H, Tk, D], strides k_* / v_*, likewise - the packed [B, T, 3, H, D] output of one projection is three such
 *            views, read in place
 *   out      fp32, written at b o_sb + h o_sh + t o_st + c (o_sb = Tq H D, o_sh = D, o_st = H D: [B, Tq, H D], the merged heads), 16-byte
 *            aligned, or NULL
 *   codes    bytes at the same element offsets, 4-byte aligned, or NULL (needs q_scale)
 * DLMCQ_EINVAL: B, H or Tq < 0, Tk < 1, D not 32 or 64, scale not finite, a stride negative or no multiple of 4, a token stride below D,
 * q / k / v NULL, both outputs NULL, an invalid quantiser, any control or layout bit or DLMCQ_EMIT_SHIFT128 in q_form (refused, not
 * stripped).  DLMCQ_EALIGN: q / k / v / out not 16-byte aligned, codes not 4-byte aligned.  DLMCQ_ERANGE: B, H, Tq, Tk, B * H or
 * B * H * ceil(Tq / 128) reaches 2^31.  B * H * Tq == 0: DLMCQ_OK, nothing launched.  A refused call writes nothing. */
int dlmcq_attention_f32(const float* q, const float* k, const float* v, float* out, void* codes, int64_t B, int64_t H, int64_t Tq,
                        int64_t Tk, int64_t D, int64_t q_sb, int64_t q_sh, int64_t q_st, int64_t k_sb, int64_t k_sh, int64_t k_st,
                        int64_t v_sb, int64_t v_sh, int64_t v_st, int64_t o_sb, int64_t o_sh, int64_t o_st, float scale,
                        const float* q_scale, const float* q_zero_point, int32_t q_lo, int32_t q_hi, int32_t q_form, float q_ste_g,
                        dlmcq_stream_t stream);

/* ---- A vision transformer's patch rows: an fp32 image batch to fp32 rows and / or the activation codes of the embedding ----
 * The rearrangement 'b c (h p1) (w p2) -> b (h w) (p1 p2 c)' of an image batch [B, C, gh p, gw p] into rows [B gh gw, p p C]:
 *     row (b gh + gy) gw + gx, column (py p + px) C + c  =  img[b sb + c sc + (gy p + py) sh + gx p + px]
 *     out = that value;  code = the quantiser (q_scale .. q_ste_g, as in dlmcq_gelu_nhwc_f32) of it - the code dlmcq_fake_quant_f32
 *                        gives for it (NaN, infinities, -0 as there).  The shifted emission is NOT accepted: the reader is a Linear
 *                        layer, which takes plain codes.
 * No arithmetic but the quantiser's: every element is read once, moved and, for the codes, quantised once.  One workgroup per (b, gy)
 * strip, whose codes - gw p p C consecutive bytes of the output - are staged in LDS (csrc/patch_rows.hip).  No atomics, no scratch:
 * a row's result depends neither on B nor on the launch.
 *   img      fp32 view [B, C, gh p, gw p]: element strides sb, sc, sh (batch, channel, image line), unit stride along a line,
 *            16-byte aligned
 *   out      fp32 [B gh gw, p p C] dense, 16-byte aligned, or NULL
 *   codes    bytes [B gh gw, p p C] dense, 16-byte aligned, or NULL (needs q_scale)
 * DLMCQ_EINVAL: B < 0, C, gh or gw < 1, p < 4 or p % 4, a stride negative or no multiple of 4, a strip of more than 65536 elements
 * (gw p p C: the LDS a launch may ask for), img NULL, both outputs NULL, an invalid quantiser, any control or layout bit or
 * DLMCQ_EMIT_SHIFT128 in q_form (refused, not stripped).  DLMCQ_EALIGN: img / out / codes not 16-byte aligned.  DLMCQ_ERANGE: B, gh,
 * B gh, B gh gw or gh p reaches 2^31.  B == 0: DLMCQ_OK, nothing launched.  A refused call writes nothing. */
int dlmcq_patch_rows_f32(const float* img, float* out, void* codes, int64_t B, int64_t C, int64_t gh, int64_t gw, int64_t p, int64_t sb,
                         int64_t sc, int64_t sh, const float* q_scale, const float* q_zero_point, int32_t q_lo, int32_t q_hi,
                         int32_t q_form, float q_ste_g, dlmcq_stream_t stream);

/* ---- A transformer's token tensor: the class token in front of the embedded patches, the position embedding added ----
 *     out[b, 0, :]     = fl32(cls[:] + pos[0, :])
 *     out[b, 1 + i, :] = fl32(e[b, i, :] + pos[1 + i, :])      i = 0 .. T - 1
 * - one IEEE add per element: the bits of `torch.cat((cls.expand(B, -1, -1), e), 1) + pos` in either operand order.  fp32 only (the
 * readers are the residual stream and a LayerNorm node).  No LDS, no atomics, no scratch (csrc/tokens.hip).
 *   e        fp32 rows [B T, C], row b T + i e_stride floats after the first, 16-byte aligned
 *   cls      fp32 [C], 16-byte aligned
 *   pos      fp32 [T + 1, C] dense, 16-byte aligned
 *   out      fp32 [B, T + 1, C]: element strides o_sb (image) and o_st (token), 16-byte aligned
 * DLMCQ_EINVAL: B < 0, T < 1, C < 4, C % 4, e_stride or o_st below C or no multiple of 4, o_sb no multiple of 4 or below
 * T o_st + C (two images' rows would meet), a NULL pointer.  DLMCQ_EALIGN: a pointer not 16-byte aligned.  DLMCQ_ERANGE: B, T + 1, C,
 * a row stride, B (T + 1) or B (T + 1) C / 4 reaches 2^31.  B == 0: DLMCQ_OK, nothing launched.  A refused call writes nothing. */
int dlmcq_tokens_assemble_f32(const float* e, const float* cls, const float* pos, float* out, int64_t B, int64_t T, int64_t C,
                              int64_t e_stride, int64_t o_sb, int64_t o_st, dlmcq_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* DLMCQ_H */
