// Hard swish x * relu6(x + 3) / 6 of an fp32 NHWC map [N, H, W, C] to fp32 [N, H, W, C] and / or the consumer's activation codes
// [N, H, W, c_pad]: the add, the clamp, the two multiplies and the quantise pass of the plan layer that reads the activated map as ONE
// read of the map - 4 B in, 1 B out per element, where torch's add, relu6, multiply, divide and the consumer's own quantise pass move
// 20 to 25.  The arithmetic, once:
//     t = fl32(x + 3.0f)                     (one IEEE add)
//     r = relu6(t)                           (the device's clamp, as squeeze_i8.hip's hard sigmoid has it: t > 0 ? t : (t is NaN ? t : +0),
//                                             then cap6_nan - NaN passes, -0 becomes +0; both exact)
//     c = fl32(1.0f / 6.0f)                  (a constant, 0x3E2AAAAB: a division by the host scalar 6 IS this multiplication on the device)
//     DLMCQ_HSWISH_MUL_FIRST  (0):  v = fl32(fl32(x * r) * c)      nn.Hardswish / F.hardswish, (x * relu6(x + 3)) / 6
//     DLMCQ_HSWISH_GATE_FIRST (1):  v = fl32(x * fl32(r * c))      x * (relu6(x + 3) / 6), x * hardsigmoid(x)
//     code = the consumer's quantiser of v   (EpiQuant::code4: the codes every emitting epilogue produces)
// - each step rounded to fp32 by itself under the library's flags (-ffp-contract=off, -fno-fast-math, denormals kept).  The two orders
// round differently in about a quarter of the elements, and a plan computes what the ops it replaces compute: hence both.  Special
// values follow from the steps: x <= -3 makes r = 0 and v = -0; x = -0 gives -0; x = -inf gives -inf * 0 = NaN; x = +inf gives +inf; NaN
// stays NaN; for x >= 3, v = (x * 6) * c or x * (6 * c), which need not equal x; x * 6 overflows to +inf above FLT_MAX / 6 under
// mul-first and does not under gate-first.  Against the real x * clip(x + 3, 0, 6) / 6: |v - v*| <= 5 * 2^-24 |v*|.
// The map is read once with a non-temporal float4 load; threads, stores and row layout: map_codes.h.
#include "map_codes.h"

namespace dlmcq {

// relu6 as the device's clamp has it (squeeze_i8.hip: sq_relu_device + cap6_nan)
__device__ __forceinline__ float hsw_relu6(float t) { return cap6_nan(t > 0.0f ? t : (t != t ? t : 0.0f)); }

template <int ORDER>
__device__ __forceinline__ float hardswish1(float x) {
  const float r = hsw_relu6(x + 3.0f);
  constexpr float c = 1.0f / 6.0f;
  if constexpr (ORDER == DLMCQ_HSWISH_MUL_FIRST) {
    const float p = x * r;
    return p * c;
  } else {
    const float g = r * c;
    return x * g;
  }
}

template <int ORDER>
struct HardswishOp {
  __device__ __forceinline__ f32x4 operator()(const f32x4* x, uint32_t m, uint32_t c4, const MapRows& g, const ConvEpi&) const {
    const f32x4 a = __builtin_nontemporal_load(x + (int64_t)m * g.XS4 + c4);
    return f32x4{hardswish1<ORDER>(a.x), hardswish1<ORDER>(a.y), hardswish1<ORDER>(a.z), hardswish1<ORDER>(a.w)};
  }
};

}  // namespace dlmcq

using namespace dlmcq;

extern "C" int dlmcq_hardswish_nhwc_f32(const float* x, float* out, void* codes, int64_t N, int64_t H, int64_t W, int64_t C,
                                        int64_t x_stride, int64_t c_pad, int32_t pad_code, const float* q_scale, const float* q_zero_point,
                                        int32_t q_lo, int32_t q_hi, int32_t q_form, float q_ste_g, int32_t order, dlmcq_stream_t stream) {
  if (order != DLMCQ_HSWISH_MUL_FIRST && order != DLMCQ_HSWISH_GATE_FIRST) return DLMCQ_EINVAL;
  MapRows g;
  ConvEpi ep{};
  const int rc = map_codes_call(g, ep, {x}, out, codes, N, H, W, H, W, C, x_stride, c_pad, pad_code, q_scale, q_zero_point, q_lo, q_hi,
                                q_form, q_ste_g);
  if (rc != DLMCQ_OK || !g.total) return rc;
  if (order == DLMCQ_HSWISH_MUL_FIRST) return map_codes_launch<true>(HardswishOp<DLMCQ_HSWISH_MUL_FIRST>{}, x, out, g, ep, stream);
  return map_codes_launch<true>(HardswishOp<DLMCQ_HSWISH_GATE_FIRST>{}, x, out, g, ep, stream);
}
