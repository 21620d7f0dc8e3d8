// What the map-to-codes kernels (avgpool.hip, gate.hip, swish.hip, hardswish.hip) share: one read of an fp32 NHWC map, the op's own
// value per element, then fp32 [N, P, Q, C] and / or the consumer's activation codes [N, P, Q, c_pad].  Not part of the ABI.
// One thread per (output pixel, 4 channels of the code row): one optional float4 store, four code bytes as one 32-bit word.  No LDS, no
// atomics, no scratch: the result depends neither on the launch geometry nor on the run.  Input rows may be wider than the data
// (`x_stride` floats per pixel: the channel-sliced fp32 view of a channel-padded plan layer is read in place); code rows are c_pad wide,
// channels C .. c_pad - 1 holding `pad_code`.  An op: `f32x4 operator()(x, m, c4, rows, ep) const`, quad c4 of output pixel m.
#pragma once

#include <initializer_list>

#include "conv_gap.h"

namespace dlmcq {

// the row geometry in quads of 4 channels: data, code row and input row widths; threads of the launch; four pad codes as one word
struct MapRows {
  int C4, CP4, XS4;
  uint32_t total, pad_word;
};

// NT: the fp32 store goes around the cache like the load (a map as large as the input, read by whoever asked for it in a later launch)
template <class Op, bool NT>
__global__ __launch_bounds__(DLMCQ_BLOCK) void map_codes_kernel(const float* __restrict__ x, float* __restrict__ out, Op op, MapRows g,
                                                                ConvEpi ep) {
  const uint32_t idx = blockIdx.x * (uint32_t)DLMCQ_BLOCK + threadIdx.x;
  if (idx >= g.total) return;
  const uint32_t m = idx / (uint32_t)g.CP4, c4 = idx - m * (uint32_t)g.CP4;
  if (c4 >= (uint32_t)g.C4) {     // a padding quad of the code row (c_pad > C only with codes: checked on the host)
    *reinterpret_cast<uint32_t*>(ep.codes + ((int64_t)m * g.CP4 + c4) * 4) = g.pad_word;
    return;
  }
  const f32x4 v = op(reinterpret_cast<const f32x4*>(x), m, c4, g, ep);
  if (out) {
    f32x4* o = reinterpret_cast<f32x4*>(out) + (int64_t)m * g.C4 + c4;
    if (NT) __builtin_nontemporal_store(v, o);
    else *o = v;
  }
  if (ep.codes) {
    const EpiQuant eq(ep);
    *reinterpret_cast<uint32_t*>(ep.codes + ((int64_t)m * g.CP4 + c4) * 4) = eq.code4(v);
  }
}

// Everything the entry points share, in the order that decides which code an argument set with two faults gets (the op's own EINVAL
// checks come before the call): geometry, the seven quantiser arguments -> ep (emit_set_quantiser, conv_gap.h), N == 0, null pointers
// and alignment (emit_check_pointers), the 2^31 limits (thread and pixel indices are 32-bit; element offsets are 64-bit).
// `in`: the fp32 inputs, the map first; H x W: the input map; P x Q: the output.  DLMCQ_OK with g.total == 0: nothing to launch.
static inline int map_codes_call(MapRows& g, ConvEpi& ep, std::initializer_list<const void*> in, const float* out, void* codes, int64_t N,
                                 int64_t H, int64_t W, int64_t P, int64_t Q, int64_t C, int64_t x_stride, int64_t c_pad, int32_t pad_code,
                                 const float* q_scale, const float* q_zero_point, int32_t q_lo, int32_t q_hi, int32_t q_form,
                                 float q_ste_g) {
  g = MapRows{};
  if (N < 0 || H < 1 || W < 1 || C < 4 || C % 4 != 0) return DLMCQ_EINVAL;
  if (x_stride < C || x_stride % 4 != 0 || c_pad < C || c_pad % 4 != 0 || pad_code < -128 || pad_code > 255) return DLMCQ_EINVAL;
  int rc = emit_set_quantiser(ep, codes, q_scale, q_zero_point, q_lo, q_hi, q_form, q_ste_g, false);
  if (rc != DLMCQ_OK) return rc;
  if (!codes && c_pad != C) return DLMCQ_EINVAL;
  if (N == 0) return DLMCQ_OK;
  rc = emit_check_pointers(in, {}, out, codes, 4);
  if (rc != DLMCQ_OK) return rc;
  constexpr int64_t LIM = 1ll << 31;
  if (H >= LIM || W >= LIM || x_stride >= LIM || c_pad >= LIM || N >= LIM || N * P >= LIM || N * P * Q >= LIM ||
      N * P * Q * (c_pad / 4) >= LIM)
    return DLMCQ_ERANGE;
  g = MapRows{(int)(C / 4), (int)(c_pad / 4), (int)(x_stride / 4), (uint32_t)(N * P * Q * (c_pad / 4)),
              (uint32_t)(pad_code & 0xff) * 0x01010101u};
  return DLMCQ_OK;
}

template <bool NT, class Op>
static inline int map_codes_launch(const Op& op, const float* x, float* out, const MapRows& g, const ConvEpi& ep, dlmcq_stream_t stream) {
  hipLaunchKernelGGL((map_codes_kernel<Op, NT>), dim3((g.total + DLMCQ_BLOCK - 1) / DLMCQ_BLOCK), dim3(DLMCQ_BLOCK), 0,
                     reinterpret_cast<hipStream_t>(stream), x, out, op, g, ep);
  return launch_status();
}

}  // namespace dlmcq
