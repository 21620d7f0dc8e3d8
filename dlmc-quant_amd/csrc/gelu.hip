// GELU (the erf form, approximate="none") x * Phi(x) of an fp32 NHWC map [N, H, W, C] - or of dense rows [M, C], passed as N = M,
// H = W = 1 - to fp32 [N, H, W, C] and / or the consumer's activation codes [N, H, W, c_pad]: the activation and the quantise pass of
// the plan layer that reads the activated tensor as ONE read - 4 B in, 1 B out per element, where torch's GELU pass and the consumer's
// own quantise pass move 13.  The arithmetic, once:
//     z = fl32(x * 0.70710678118654752440f)  (one IEEE multiply by fl32(1 / sqrt(2)))
//     e = erff(z)                            (the device library's accurate erff)
//     f = fl32(1.0f + e)                     (one IEEE add)
//     h = fl32(x * 0.5f)                     (exact, but for a denormal result)
//     v = fl32(h * f)                        (one IEEE multiply, a value of its own: never folded into the quantiser's v - of or fma)
//     code = the consumer's quantiser of v   (EpiQuant::code4: the codes every emitting epilogue produces)
// - each step rounded to fp32 by itself under the library's flags (-ffp-contract=off, -fno-fast-math, denormals kept).  It is the
// operation order of torch's device GELU kernel for approximate="none".  Special values follow from the steps: x <= about -5.9 makes
// e = -1, f = 0 and v = -0; x = -inf gives -inf * 0 = NaN; x = +inf gives +inf * 2 = +inf; NaN stays NaN; -0 gives -0; a denormal x
// gives f = 1 and v = x / 2 (rounded to even).
// Against the real v* = x * Phi(x) = 0.5 x (1 + erf(x / sqrt(2))), with u = 2^-23 (|x| + |v*|): |v - v*| <= 2 u.  erff is within 2 ulp
// (the device library's documented bound: ROCm "HIP math API", single-precision table, erff: 2 ulp - the bound CUDA's table gives too),
// and |e| <= 1, so e carries at most about 2^-23 + 2^-24 absolute; z's rounding moves erf by at most 2^-24 |z| erf'(z) <= 2^-24 * 0.5
// (|t| exp(-t^2) * 2 / sqrt(pi) <= 0.49); the add rounds by 2^-24 f <= 2^-23.  Together at most about 2^-22 absolute on f, which h =
// x / 2 scales to 2^-23 |x|.  The last multiply (and h's rounding, exact outside the denormals) adds 2^-24 |v*| each at most: 2^-23 |v*|
// covers them.  The factor 2 covers the second-order terms and the deep negative tail, where f itself is of the size of its error.
// (The same five steps in torch fp32 on the CPU stay within 0.46 u over randn * 3 and a sweep of [-12, 12])
// The map is read once with a non-temporal float4 load; threads, stores and row layout: map_codes.h.
#include "map_codes.h"

namespace dlmcq {

__device__ __forceinline__ float gelu1(float x) {
  const float z = x * 0.70710678118654752440f;
  const float f = 1.0f + erff(z);
  const float h = x * 0.5f;
  return h * f;
}

struct GeluOp {
  __device__ __forceinline__ f32x4 operator()(const f32x4* x, uint32_t m, uint32_t c4, const MapRows& g, const ConvEpi&) const {
    const f32x4 a = __builtin_nontemporal_load(x + (int64_t)m * g.XS4 + c4);
    return f32x4{gelu1(a.x), gelu1(a.y), gelu1(a.z), gelu1(a.w)};
  }
};

}  // namespace dlmcq

using namespace dlmcq;

extern "C" int dlmcq_gelu_nhwc_f32(const float* x, float* out, void* codes, int64_t N, int64_t H, int64_t W, int64_t C, int64_t x_stride,
                                   int64_t c_pad, int32_t pad_code, const float* q_scale, const float* q_zero_point, int32_t q_lo,
                                   int32_t q_hi, int32_t q_form, float q_ste_g, dlmcq_stream_t stream) {
  MapRows g;
  ConvEpi ep{};
  const int rc = map_codes_call(g, ep, {x}, out, codes, N, H, W, H, W, C, x_stride, c_pad, pad_code, q_scale, q_zero_point, q_lo, q_hi,
                                q_form, q_ste_g);
  if (rc != DLMCQ_OK || !g.total) return rc;
  return map_codes_launch<true>(GeluOp{}, x, out, g, ep, stream);
}
