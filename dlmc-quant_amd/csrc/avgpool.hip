// Windowed average pool (nn.AvgPool2d(s, s): window = stride, no padding, floor) of an fp32 NHWC map to fp32 [N, P, Q, C] and / or the
// consumer's activation codes [N, P, Q, c_pad] - the shortcut of a ResNet-C / -D block, a DenseNet transition, an "anti-aliased"
// downsample: avg pool -> 1x1 convolution, whose quantise pass and the pooled fp32 tensor between the two disappear.  The arithmetic, once:
//     a = +0.0f
//     for dy in 0 .. s-1: for dx in 0 .. s-1: a = fl32(a + x[n, p*s + dy, q*s + dx, c])
//     pooled = fl32(a / fl32(s*s))       (a true IEEE division: no reciprocal multiply, no contraction)
//     code = the consumer's quantiser of pooled (EpiQuant::code4: the codes every emitting epilogue produces)
// P = H / s, Q = W / s (floor: trailing rows and columns are dropped, as torch does with ceil_mode=False).  It is the loop torch's
// avg_pool2d runs (sum from +0 in row-major window order, then one division), hence bit-identical pooled values.
// One thread per (output pixel, 4 channels of the code row): float4 loads coalesced over channels and non-temporal (the map is read
// once), one optional float4 store, four code bytes as one 32-bit word.  No LDS, no atomics, no scratch: the result depends neither on
// the launch geometry nor on the run.  Input rows may be wider than the data (`x_stride` floats per pixel: the channel-sliced fp32 view
// of a channel-padded plan layer is read in place); code rows are c_pad wide, channels C .. c_pad - 1 holding `pad_code`.
#include "conv_gap.h"

namespace dlmcq {

__global__ __launch_bounds__(DLMCQ_BLOCK) void avgpool_nhwc_kernel(const float* __restrict__ x, float* __restrict__ pooled, int P, int Q,
                                                                   int W, int C4, int CP4, int XS4, int s, int64_t img4, uint32_t total,
                                                                   uint32_t pad_word, ConvEpi ep) {
  const uint32_t idx = blockIdx.x * (uint32_t)DLMCQ_BLOCK + threadIdx.x;
  if (idx >= total) return;
  const uint32_t m = idx / (uint32_t)CP4, c4 = idx - m * (uint32_t)CP4;
  if (c4 >= (uint32_t)C4) {     // a padding quad of the code row (c_pad > C only with codes: checked on the host)
    *reinterpret_cast<uint32_t*>(ep.codes + ((int64_t)m * CP4 + c4) * 4) = pad_word;
    return;
  }
  const uint32_t q = m % (uint32_t)Q, t = m / (uint32_t)Q, p = t % (uint32_t)P, n = t / (uint32_t)P;
  const f32x4* base = reinterpret_cast<const f32x4*>(x) + (int64_t)n * img4 + ((int64_t)(p * s) * W + (int64_t)(q * s)) * XS4 + c4;
  f32x4 a = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
  for (int dy = 0; dy < s; ++dy) {
    const f32x4* row = base + (int64_t)dy * W * XS4;
    for (int dx = 0; dx < s; ++dx) {
      const f32x4 v = __builtin_nontemporal_load(row + (int64_t)dx * XS4);
      a = f32x4{a.x + v.x, a.y + v.y, a.z + v.z, a.w + v.w};
    }
  }
  const float d = (float)(s * s);
  const f32x4 mean = f32x4{a.x / d, a.y / d, a.z / d, a.w / d};
  if (pooled) *reinterpret_cast<f32x4*>(pooled + ((int64_t)m * C4 + c4) * 4) = mean;
  if (ep.codes) {
    const EpiQuant eq(ep);
    *reinterpret_cast<uint32_t*>(ep.codes + ((int64_t)m * CP4 + c4) * 4) = eq.code4(mean);
  }
}

}  // namespace dlmcq

using namespace dlmcq;

extern "C" int dlmcq_avgpool_nhwc_f32(const float* x, float* pooled, void* codes, int64_t N, int64_t H, int64_t W, int64_t C,
                                      int64_t x_stride, int64_t window, int64_t c_pad, int32_t pad_code, const float* q_scale,
                                      const float* q_zero_point, int32_t q_lo, int32_t q_hi, int32_t q_form, float q_ste_g,
                                      dlmcq_stream_t stream) {
  if (N < 0 || window < 2 || window > 8 || H < window || W < window || C < 4 || C % 4 != 0) return DLMCQ_EINVAL;
  if (x_stride < C || x_stride % 4 != 0 || c_pad < C || c_pad % 4 != 0 || pad_code < -128 || pad_code > 255) return DLMCQ_EINVAL;
  ConvEpi ep{};
  const int rc = gap_set_quantiser(ep, codes, q_scale, q_zero_point, q_lo, q_hi, q_form, q_ste_g);
  if (rc != DLMCQ_OK) return rc;
  if (ep.ctl) return DLMCQ_EINVAL;           // (row-major NHWC only: every control / layout bit is refused, not stripped)
  if (!codes && c_pad != C) return DLMCQ_EINVAL;
  if (N == 0) return DLMCQ_OK;
  if (!x || !(pooled || codes)) return DLMCQ_EINVAL;
  if (!aligned16(x) || (pooled && !aligned16(pooled)) || (codes && !aligned4(codes))) return DLMCQ_EALIGN;
  const int64_t P = H / window, Q = W / window;
  constexpr int64_t LIM = 1ll << 31;
  if (H >= LIM || W >= LIM || x_stride >= LIM || c_pad >= LIM || N >= LIM || N * P >= LIM || N * P * Q >= LIM ||
      N * P * Q * (c_pad / 4) >= LIM || H * W >= LIM)      // (thread and pixel indices are 32-bit; element offsets are 64-bit)
    return DLMCQ_ERANGE;
  const int64_t threads = N * P * Q * (c_pad / 4);
  const uint32_t pad_word = (uint32_t)(pad_code & 0xff) * 0x01010101u;
  hipLaunchKernelGGL(avgpool_nhwc_kernel, dim3((uint32_t)((threads + DLMCQ_BLOCK - 1) / DLMCQ_BLOCK)), dim3(DLMCQ_BLOCK), 0,
                     reinterpret_cast<hipStream_t>(stream), x, pooled, (int)P, (int)Q, (int)W, (int)(C / 4), (int)(c_pad / 4),
                     (int)(x_stride / 4), (int)window, H * W * (x_stride / 4), (uint32_t)threads, pad_word, ep);
  return launch_status();
}
