// A squeeze-excite channel gate x * g (x fp32 NHWC [N, H, W, C], g fp32 [N, C] broadcast over the pixels) (+ ReLU / ReLU6) to fp32
// [N, H, W, C] and / or the consumer's activation codes [N, H, W, c_pad]: the multiply, the activation behind it and the quantise pass
// of the plan convolution that reads the gated map as ONE read of the map - 4 B in, 1 B out per element.  The arithmetic, once:
//     v = fl32(x[n, h, w, c] * g[n, c])      (one IEEE multiply, a value of its own: never folded into the quantiser's v - of or fma)
//     v = act(v)                             (ReLU as torch runs it ON THE DEVICE: clamp_min(0) = isnan(v) ? v : max(v, 0) - NaN passes and
//                                             -0 becomes +0, where relu_nan, the CPU's, keeps -0; ReLU6 adds cap6_nan)
//     code = the consumer's quantiser of v   (EpiQuant::code4: the codes every emitting epilogue produces)
// It is torch's own x * g.view(N, C, 1, 1) followed by its relu / relu6, element by element, hence bit-identical values.
// The map is read once with a non-temporal float4 load, the gate with an ordinary one (N * C floats stay in cache).  The gate row is
// that of the thread's own image - a workgroup may span several.  Threads, stores and row layout: map_codes.h.
#include "map_codes.h"

namespace dlmcq {

// torch.relu / F.relu6 on the device (ATen's clamp kernels: `isnan(v) ? v : max(v, 0)`, the hardware maximum of -0 and +0 being +0).
// The node replaces exactly that op of the plan without gates, so that is the value to store - sign of a zero included.
__device__ __forceinline__ float relu_device(float v) { return v > 0.0f ? v : (v != v ? v : 0.0f); }

struct GateOp {
  const float* gate;
  uint32_t HW;
  __device__ __forceinline__ f32x4 operator()(const f32x4* x, uint32_t m, uint32_t c4, const MapRows& r, const ConvEpi& ep) const {
    const uint32_t n = m / HW;
    const f32x4 a = __builtin_nontemporal_load(x + (int64_t)m * r.XS4 + c4);
    const f32x4 g = *(reinterpret_cast<const f32x4*>(gate) + (int64_t)n * r.C4 + c4);
    f32x4 v = f32x4{a.x * g.x, a.y * g.y, a.z * g.z, a.w * g.w};
    if (ep.relu) {
      v = f32x4{relu_device(v.x), relu_device(v.y), relu_device(v.z), relu_device(v.w)};
      if (ep.relu == DLMCQ_ACT_RELU6) v = cap6_nan4(v);
    }
    return v;
  }
};

}  // namespace dlmcq

using namespace dlmcq;

extern "C" int dlmcq_gate_nhwc_f32(const float* x, const float* gate, float* out, void* codes, int64_t N, int64_t H, int64_t W, int64_t C,
                                   int64_t x_stride, int64_t c_pad, int32_t pad_code, int32_t act, const float* q_scale,
                                   const float* q_zero_point, int32_t q_lo, int32_t q_hi, int32_t q_form, float q_ste_g,
                                   dlmcq_stream_t stream) {
  if (act != DLMCQ_ACT_NONE && act != DLMCQ_ACT_RELU && act != DLMCQ_ACT_RELU6) return DLMCQ_EINVAL;
  MapRows g;
  ConvEpi ep{};
  const int rc = map_codes_call(g, ep, {x, gate}, out, codes, N, H, W, H, W, C, x_stride, c_pad, pad_code, q_scale, q_zero_point, q_lo,
                                q_hi, q_form, q_ste_g);
  if (rc != DLMCQ_OK || !g.total) return rc;
  ep.relu = act;
  return map_codes_launch<true>(GateOp{gate, (uint32_t)(H * W)}, x, out, g, ep, stream);
}
