// What the depthwise vector kernels' files (conv_dw_i8.hip, conv_dw5_i8.hip) share: the geometry record their kernels take, the small device
// helpers of the integer path, the ABI arguments -> DwCall, and THE argument checks of a depthwise entry point, in their one order.
// Not part of the ABI.
#pragma once

#include "conv_i8_common.h"

namespace dlmcq {

struct DwGeom {
  int N, H, W, C4, R, S, stride, pad, P, Q;    // C4 = C / 4
  FastDiv cdiv, qdiv, pdiv;
};

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// the first v_dot4_i32_i8 of a chain in its three-address form: the compiler renders __builtin_amdgcn_sdot4 as the accumulating
// v_dot4c_i32_i8, which needs a v_mov of the start value whenever that value is shared between chains (it always is here)
__device__ __forceinline__ int dot4_from(uint32_t a, uint32_t b, int c) {
  int d;
  asm("v_dot4_i32_i8 %0, %1, %2, %3" : "=v"(d) : "v"(a), "v"(b), "v"(c));
  return d;
}
constexpr int DW_BIG = 0x7fff0000;      // a byte offset beyond every tensor the buffer-addressed tap loads accept

// 4 x 4 bytes transposed (8 v_perm_b32): a0..a3 hold bytes [tap k][channel j]; t[j] = the four taps of channel j
__device__ __forceinline__ void transpose4x4(uint32_t a0, uint32_t a1, uint32_t a2, uint32_t a3, uint32_t (&t)[4]) {
  const uint32_t l01 = __builtin_amdgcn_perm(a1, a0, 0x05010400u), h01 = __builtin_amdgcn_perm(a1, a0, 0x07030602u);
  const uint32_t l23 = __builtin_amdgcn_perm(a3, a2, 0x05010400u), h23 = __builtin_amdgcn_perm(a3, a2, 0x07030602u);
  t[0] = __builtin_amdgcn_perm(l23, l01, 0x05040100u);
  t[1] = __builtin_amdgcn_perm(l23, l01, 0x07060302u);
  t[2] = __builtin_amdgcn_perm(h23, h01, 0x05040100u);
  t[3] = __builtin_amdgcn_perm(h23, h01, 0x07060302u);
}

constexpr int32_t DW_CTL = DLMCQ_FORCE_TILED | DLMCQ_ROUTE_ONLY | DLMCQ_ROUTE_DW_VARIANT;     // (include/dlmcq.h: control bits of `q_form`)

// the record of a depthwise entry point's ABI arguments; ep.x_off / ep.x_tap are the caller's to set.  Of `q_form`'s flag bits only the
// three control bits are taken (dw_checks): the rest of it goes into the epilogue as it came.
static inline DwCall dw_call(const void* x, const int8_t* w, float* out, const float* bias, const float* in_scale, const float* in_zero_point,
                             const float* w_scale, const float* w_offset, int64_t N, int64_t H, int64_t W, int64_t C, int64_t R, int64_t S,
                             int32_t stride, int32_t pad, int32_t x_is_unsigned, int32_t relu, void* codes, const float* q_scale,
                             const float* q_zero_point, int32_t q_lo, int32_t q_hi, int32_t q_form, float q_ste_g, dlmcq_stream_t stream) {
  DwCall c{};
  c.x = x; c.w = w; c.out = out; c.bias = bias; c.s_in = in_scale; c.zp_in = in_zero_point; c.s_w = w_scale; c.w_off = w_offset;
  c.N = N; c.H = H; c.W = W; c.C = C; c.R = R; c.S = S; c.stride = stride; c.pad = pad;
  c.x_signed = x_is_unsigned ? 0 : 1;
  c.st = reinterpret_cast<hipStream_t>(stream);
  c.ep = make_epi_form(nullptr, relu, codes, q_scale, q_zero_point, q_lo, q_hi, q_form & ~DW_CTL, q_ste_g);
  c.ctl = (uint32_t)q_form & DW_CTL;
  c.q_lo = q_lo; c.q_hi = q_hi; c.q_form = q_form;
  c.P = conv_out_size(H, R, stride, pad, 1);
  c.Q = conv_out_size(W, S, stride, pad, 1);
  return c;
}

// THE checks of a depthwise entry point, in their one order: false = the call is answered, with `status` (a refusal, or DLMCQ_OK for an
// empty problem); true = the dispatch goes on.  `vec16`: the entry point reads `x` and writes `codes` 16 bytes at a time (else 4).
static inline bool dw_checks(const DwCall& c, bool vec16, int& status) {
  status = DLMCQ_EINVAL;
  if ((c.ctl & DLMCQ_ROUTE_DW_VARIANT) && !(c.ctl & DLMCQ_ROUTE_ONLY)) return false;     // (a question about the route, never a launch)
  if (c.N < 0 || c.H < 1 || c.W < 1 || c.C < 4 || (c.C & 3) || c.R < 1 || c.S < 1 || c.R > 7 || c.S > 7 || c.stride < 1 || c.pad < 0)
    return false;
  if (c.P < 1 || c.Q < 1) return false;
  if (c.N == 0) {
    status = DLMCQ_OK;
    return false;
  }
  if (!c.x || !c.w || !(c.out || c.ep.codes) || !c.s_in || !c.s_w) return false;
  if (quantiser_check(c.ep.codes, c.ep.q_scale, c.q_lo, c.q_hi, c.q_form, DW_CTL) != DLMCQ_OK) return false;
  status = DLMCQ_EALIGN;
  if (!aligned4(c.x) || !aligned4(c.w) || !aligned16(c.s_w) || (c.w_off && !aligned16(c.w_off)) || (c.bias && !aligned16(c.bias)) ||
      (c.out && !aligned16(c.out)) || (c.ep.codes && !aligned4(c.ep.codes)))
    return false;
  if (vec16 && (!aligned16(c.x) || (c.ep.codes && !aligned16(c.ep.codes)))) return false;
  status = DLMCQ_ERANGE;
  if (c.N * c.P * c.Q * (c.C / 4) >= (1ll << 31) || c.N * c.H * c.W * (c.C / 4) >= (1ll << 31)) return false;
  status = DLMCQ_OK;
  return true;
}

}  // namespace dlmcq
