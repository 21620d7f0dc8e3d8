// Swish (SiLU) x * sigmoid(x) of an fp32 NHWC map [N, H, W, C] to fp32 [N, H, W, C] and / or the consumer's activation codes
// [N, H, W, c_pad]: the sigmoid, the multiply and the quantise pass of the plan layer that reads the activated map as ONE read of the
// map - 4 B in, 1 B out per element, where torch's sigmoid, multiply and the consumer's own quantise pass move 25.  The arithmetic, once:
//     e = expf(-x)                           (the device library's accurate expf, not __expf; the negation is exact)
//     d = fl32(1.0f + e)                     (one IEEE add)
//     s = fl32(1.0f / d)                     (one IEEE division, correctly rounded: -fhip-fp32-correctly-rounded-divide-sqrt)
//     v = fl32(x * s)                        (one IEEE multiply, a value of its own: never folded into the quantiser's v - of or fma)
//     code = the consumer's quantiser of v   (EpiQuant::code4: the codes every emitting epilogue produces)
// - each step rounded to fp32 by itself under the library's flags (-ffp-contract=off, -fno-fast-math, denormals kept).  It is the
// operation sequence of torch's x * torch.sigmoid(x); F.silu divides x by d instead and may differ in the last bit.  Special values
// follow from the steps: x <= -88.8 makes e = +inf, s = 0 and v = -0; x = -inf gives -inf * 0 = NaN; x = +inf gives +inf; NaN stays NaN;
// a denormal x gives s = 0.5 and v = x / 2 (rounded to even).  Against the real x * sigmoid(x): |v - v*| <= 3 * 2^-23 |v*| for
// |x| <= 80.
// The map is read once with a non-temporal float4 load; threads, stores and row layout: map_codes.h.
#include "map_codes.h"

namespace dlmcq {

__device__ __forceinline__ float swish1(float x) {
  const float d = 1.0f + expf(-x);
  const float s = 1.0f / d;
  return x * s;
}

struct SwishOp {
  __device__ __forceinline__ f32x4 operator()(const f32x4* x, uint32_t m, uint32_t c4, const MapRows& g, const ConvEpi&) const {
    const f32x4 a = __builtin_nontemporal_load(x + (int64_t)m * g.XS4 + c4);
    return f32x4{swish1(a.x), swish1(a.y), swish1(a.z), swish1(a.w)};
  }
};

}  // namespace dlmcq

using namespace dlmcq;

extern "C" int dlmcq_swish_nhwc_f32(const float* x, float* out, void* codes, int64_t N, int64_t H, int64_t W, int64_t C, int64_t x_stride,
                                    int64_t c_pad, int32_t pad_code, const float* q_scale, const float* q_zero_point, int32_t q_lo,
                                    int32_t q_hi, int32_t q_form, float q_ste_g, dlmcq_stream_t stream) {
  MapRows g;
  ConvEpi ep{};
  const int rc = map_codes_call(g, ep, {x}, out, codes, N, H, W, H, W, C, x_stride, c_pad, pad_code, q_scale, q_zero_point, q_lo, q_hi,
                                q_form, q_ste_g);
  if (rc != DLMCQ_OK || !g.total) return rc;
  return map_codes_launch<true>(SwishOp{}, x, out, g, ep, stream);
}
