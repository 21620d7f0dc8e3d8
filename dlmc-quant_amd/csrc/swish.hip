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
// One thread per (pixel, 4 channels of the code row): the map is read once with a non-temporal float4 load, one optional non-temporal
// float4 store, four code bytes as one 32-bit word.  No LDS, no atomics, no scratch.  Input rows may be wider than the data (`x_stride`
// floats per pixel: the channel-sliced fp32 view of a channel-padded plan layer is read in place); code rows are c_pad wide, channels
// C .. c_pad - 1 holding `pad_code`.
#include "conv_gap.h"

namespace dlmcq {

__device__ __forceinline__ float swish1(float x) {
  const float d = 1.0f + expf(-x);
  const float s = 1.0f / d;
  return x * s;
}

__global__ __launch_bounds__(DLMCQ_BLOCK) void swish_nhwc_kernel(const float* __restrict__ x, float* __restrict__ out, int C4, int CP4,
                                                                 int XS4, uint32_t total, uint32_t pad_word, ConvEpi ep) {
  const uint32_t idx = blockIdx.x * (uint32_t)DLMCQ_BLOCK + threadIdx.x;
  if (idx >= total) return;
  const uint32_t m = idx / (uint32_t)CP4, c4 = idx - m * (uint32_t)CP4;
  if (c4 >= (uint32_t)C4) {     // a padding quad of the code row (c_pad > C only with codes: checked on the host)
    *reinterpret_cast<uint32_t*>(ep.codes + ((int64_t)m * CP4 + c4) * 4) = pad_word;
    return;
  }
  const f32x4 a = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(x) + (int64_t)m * XS4 + c4);
  const f32x4 v = f32x4{swish1(a.x), swish1(a.y), swish1(a.z), swish1(a.w)};
  // (the fp32 map is as large as the input and read by whoever asked for it in a later launch: written around the cache like the load)
  if (out) __builtin_nontemporal_store(v, reinterpret_cast<f32x4*>(out) + (int64_t)m * C4 + c4);
  if (ep.codes) {
    const EpiQuant eq(ep);
    *reinterpret_cast<uint32_t*>(ep.codes + ((int64_t)m * CP4 + c4) * 4) = eq.code4(v);
  }
}

}  // namespace dlmcq

using namespace dlmcq;

extern "C" int dlmcq_swish_nhwc_f32(const float* x, float* out, void* codes, int64_t N, int64_t H, int64_t W, int64_t C, int64_t x_stride,
                                    int64_t c_pad, int32_t pad_code, const float* q_scale, const float* q_zero_point, int32_t q_lo,
                                    int32_t q_hi, int32_t q_form, float q_ste_g, dlmcq_stream_t stream) {
  if (N < 0 || H < 1 || W < 1 || C < 4 || C % 4 != 0) return DLMCQ_EINVAL;
  if (x_stride < C || x_stride % 4 != 0 || c_pad < C || c_pad % 4 != 0 || pad_code < -128 || pad_code > 255) return DLMCQ_EINVAL;
  ConvEpi ep{};
  const int rc = gap_set_quantiser(ep, codes, q_scale, q_zero_point, q_lo, q_hi, q_form, q_ste_g);
  if (rc != DLMCQ_OK) return rc;
  if (ep.ctl) return DLMCQ_EINVAL;           // (row-major NHWC only: every control / layout bit is refused, not stripped)
  if (!codes && c_pad != C) return DLMCQ_EINVAL;
  if (N == 0) return DLMCQ_OK;
  if (!x || !(out || codes)) return DLMCQ_EINVAL;
  if (!aligned16(x) || (out && !aligned16(out)) || (codes && !aligned4(codes))) return DLMCQ_EALIGN;
  constexpr int64_t LIM = 1ll << 31;
  if (H >= LIM || W >= LIM || x_stride >= LIM || c_pad >= LIM || N >= LIM || N * H >= LIM || N * H * W >= LIM ||
      N * H * W * (c_pad / 4) >= LIM)        // (thread and pixel indices are 32-bit; element offsets are 64-bit)
    return DLMCQ_ERANGE;
  const int64_t threads = N * H * W * (c_pad / 4);
  const uint32_t pad_word = (uint32_t)(pad_code & 0xff) * 0x01010101u;
  hipLaunchKernelGGL(swish_nhwc_kernel, dim3((uint32_t)((threads + DLMCQ_BLOCK - 1) / DLMCQ_BLOCK)), dim3(DLMCQ_BLOCK), 0,
                     reinterpret_cast<hipStream_t>(stream), x, out, (int)(C / 4), (int)(c_pad / 4), (int)(x_stride / 4), (uint32_t)threads,
                     pad_word, ep);
  return launch_status();
}
