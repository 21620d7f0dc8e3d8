// Windowed average pool (nn.AvgPool2d(s, s): window = stride, no padding, floor) of an fp32 NHWC map to fp32 [N, P, Q, C] and / or the
// consumer's activation codes [N, P, Q, c_pad] - the shortcut of a ResNet-C / -D block, a DenseNet transition, an "anti-aliased"
// downsample: avg pool -> 1x1 convolution, whose quantise pass and the pooled fp32 tensor between the two disappear.  The arithmetic, once:
//     a = +0.0f
//     for dy in 0 .. s-1: for dx in 0 .. s-1: a = fl32(a + x[n, p*s + dy, q*s + dx, c])
//     pooled = fl32(a / fl32(s*s))       (a true IEEE division: no reciprocal multiply, no contraction)
//     code = the consumer's quantiser of pooled (EpiQuant::code4: the codes every emitting epilogue produces)
// P = H / s, Q = W / s (floor: trailing rows and columns are dropped, as torch does with ceil_mode=False).  It is the loop torch's
// avg_pool2d runs (sum from +0 in row-major window order, then one division), hence bit-identical pooled values.
// float4 loads coalesced over channels and non-temporal (the map is read once); threads, stores and row layout: map_codes.h.
#include "map_codes.h"

namespace dlmcq {

struct AvgPoolOp {
  int P, Q, W, s;
  int64_t img4;      // quads per input image
  __device__ __forceinline__ f32x4 operator()(const f32x4* x, uint32_t m, uint32_t c4, const MapRows& g, const ConvEpi&) const {
    const int XS4 = g.XS4;
    const uint32_t q = m % (uint32_t)Q, t = m / (uint32_t)Q, p = t % (uint32_t)P, n = t / (uint32_t)P;
    const f32x4* base = x + (int64_t)n * img4 + ((int64_t)(p * s) * W + (int64_t)(q * s)) * XS4 + c4;
    f32x4 a = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    for (int dy = 0; dy < s; ++dy) {
      const f32x4* row = base + (int64_t)dy * W * XS4;
      for (int dx = 0; dx < s; ++dx) {
        const f32x4 v = __builtin_nontemporal_load(row + (int64_t)dx * XS4);
        a = f32x4{a.x + v.x, a.y + v.y, a.z + v.z, a.w + v.w};
      }
    }
    const float d = (float)(s * s);
    return f32x4{a.x / d, a.y / d, a.z / d, a.w / d};
  }
};

}  // namespace dlmcq

using namespace dlmcq;

extern "C" int dlmcq_avgpool_nhwc_f32(const float* x, float* pooled, void* codes, int64_t N, int64_t H, int64_t W, int64_t C,
                                      int64_t x_stride, int64_t window, int64_t c_pad, int32_t pad_code, const float* q_scale,
                                      const float* q_zero_point, int32_t q_lo, int32_t q_hi, int32_t q_form, float q_ste_g,
                                      dlmcq_stream_t stream) {
  if (window < 2 || window > 8 || H < window || W < window) return DLMCQ_EINVAL;
  const int64_t P = H / window, Q = W / window;
  MapRows g;
  ConvEpi ep{};
  const int rc = map_codes_call(g, ep, {x}, pooled, codes, N, H, W, P, Q, C, x_stride, c_pad, pad_code, q_scale, q_zero_point, q_lo, q_hi,
                                q_form, q_ste_g);
  if (rc != DLMCQ_OK || !g.total) return rc;
  if (H * W >= (1ll << 31)) return DLMCQ_ERANGE;      // (the pixel offset inside an image is formed in 64 bits from 32-bit factors)
  return map_codes_launch<false>(AvgPoolOp{(int)P, (int)Q, (int)W, (int)window, H * W * (x_stride / 4)}, x, pooled, g, ep, stream);
}
