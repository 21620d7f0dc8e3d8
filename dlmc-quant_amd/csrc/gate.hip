// A squeeze-excite channel gate x * g (x fp32 NHWC [N, H, W, C], g fp32 [N, C] broadcast over the pixels) (+ ReLU / ReLU6) to fp32
// [N, H, W, C] and / or the consumer's activation codes [N, H, W, c_pad]: the multiply, the activation behind it and the quantise pass
// of the plan convolution that reads the gated map as ONE read of the map - 4 B in, 1 B out per element.  The arithmetic, once:
//     v = fl32(x[n, h, w, c] * g[n, c])      (one IEEE multiply, a value of its own: never folded into the quantiser's v - of or fma)
//     v = act(v)                             (ReLU as torch runs it ON THE DEVICE: clamp_min(0) = isnan(v) ? v : max(v, 0) - NaN passes and
//                                             -0 becomes +0, where relu_nan, the CPU's, keeps -0; ReLU6 adds cap6_nan)
//     code = the consumer's quantiser of v   (EpiQuant::code4: the codes every emitting epilogue produces)
// It is torch's own x * g.view(N, C, 1, 1) followed by its relu / relu6, element by element, hence bit-identical values.
// One thread per (pixel, 4 channels of the code row): the map is read once with a non-temporal float4 load, the gate with an ordinary
// one (N * C floats stay in cache), one optional float4 store, four code bytes as one 32-bit word.  The gate row is that of the
// thread's own image - a workgroup may span several.  No LDS, no atomics, no scratch.  Input rows may be wider than the data (`x_stride`
// floats per pixel: the channel-sliced fp32 view of a channel-padded plan layer is read in place); code rows are c_pad wide, channels
// C .. c_pad - 1 holding `pad_code`.
#include "conv_gap.h"

namespace dlmcq {

// torch.relu / F.relu6 on the device (ATen's clamp kernels: `isnan(v) ? v : max(v, 0)`, the hardware maximum of -0 and +0 being +0).
// The node replaces exactly that op of the plan without gates, so that is the value to store - sign of a zero included.
__device__ __forceinline__ float relu_device(float v) { return v > 0.0f ? v : (v != v ? v : 0.0f); }

__global__ __launch_bounds__(DLMCQ_BLOCK) void gate_nhwc_kernel(const float* __restrict__ x, const float* __restrict__ gate,
                                                                float* __restrict__ out, uint32_t HW, int C4, int CP4, int XS4,
                                                                uint32_t total, uint32_t pad_word, ConvEpi ep) {
  const uint32_t idx = blockIdx.x * (uint32_t)DLMCQ_BLOCK + threadIdx.x;
  if (idx >= total) return;
  const uint32_t m = idx / (uint32_t)CP4, c4 = idx - m * (uint32_t)CP4;
  if (c4 >= (uint32_t)C4) {     // a padding quad of the code row (c_pad > C only with codes: checked on the host)
    *reinterpret_cast<uint32_t*>(ep.codes + ((int64_t)m * CP4 + c4) * 4) = pad_word;
    return;
  }
  const uint32_t n = m / HW;
  const f32x4 a = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(x) + (int64_t)m * XS4 + c4);
  const f32x4 g = *(reinterpret_cast<const f32x4*>(gate) + (int64_t)n * C4 + c4);
  f32x4 v = f32x4{a.x * g.x, a.y * g.y, a.z * g.z, a.w * g.w};
  if (ep.relu) {
    v = f32x4{relu_device(v.x), relu_device(v.y), relu_device(v.z), relu_device(v.w)};
    if (ep.relu == DLMCQ_ACT_RELU6) v = cap6_nan4(v);
  }
  // (the fp32 map is as large as the input and read by whoever asked for it in a later launch: written around the cache like the load)
  if (out) __builtin_nontemporal_store(v, reinterpret_cast<f32x4*>(out) + (int64_t)m * C4 + c4);
  if (ep.codes) {
    const EpiQuant eq(ep);
    *reinterpret_cast<uint32_t*>(ep.codes + ((int64_t)m * CP4 + c4) * 4) = eq.code4(v);
  }
}

}  // namespace dlmcq

using namespace dlmcq;

extern "C" int dlmcq_gate_nhwc_f32(const float* x, const float* gate, float* out, void* codes, int64_t N, int64_t H, int64_t W, int64_t C,
                                   int64_t x_stride, int64_t c_pad, int32_t pad_code, int32_t act, const float* q_scale,
                                   const float* q_zero_point, int32_t q_lo, int32_t q_hi, int32_t q_form, float q_ste_g,
                                   dlmcq_stream_t stream) {
  if (N < 0 || H < 1 || W < 1 || C < 4 || C % 4 != 0) return DLMCQ_EINVAL;
  if (x_stride < C || x_stride % 4 != 0 || c_pad < C || c_pad % 4 != 0 || pad_code < -128 || pad_code > 255) return DLMCQ_EINVAL;
  if (act != DLMCQ_ACT_NONE && act != DLMCQ_ACT_RELU && act != DLMCQ_ACT_RELU6) return DLMCQ_EINVAL;
  ConvEpi ep{};
  const int rc = gap_set_quantiser(ep, codes, q_scale, q_zero_point, q_lo, q_hi, q_form, q_ste_g);
  if (rc != DLMCQ_OK) return rc;
  if (ep.ctl) return DLMCQ_EINVAL;           // (row-major NHWC only: every control / layout bit is refused, not stripped)
  if (!codes && c_pad != C) return DLMCQ_EINVAL;
  if (N == 0) return DLMCQ_OK;
  if (!x || !gate || !(out || codes)) return DLMCQ_EINVAL;
  if (!aligned16(x) || !aligned16(gate) || (out && !aligned16(out)) || (codes && !aligned4(codes))) return DLMCQ_EALIGN;
  constexpr int64_t LIM = 1ll << 31;
  if (H >= LIM || W >= LIM || x_stride >= LIM || c_pad >= LIM || N >= LIM || N * H >= LIM || N * H * W >= LIM ||
      N * H * W * (c_pad / 4) >= LIM)        // (thread and pixel indices are 32-bit; element offsets are 64-bit)
    return DLMCQ_ERANGE;
  ep.relu = act;
  const int64_t threads = N * H * W * (c_pad / 4);
  const uint32_t pad_word = (uint32_t)(pad_code & 0xff) * 0x01010101u;
  hipLaunchKernelGGL(gate_nhwc_kernel, dim3((uint32_t)((threads + DLMCQ_BLOCK - 1) / DLMCQ_BLOCK)), dim3(DLMCQ_BLOCK), 0,
                     reinterpret_cast<hipStream_t>(stream), x, gate, out, (uint32_t)(H * W), (int)(C / 4), (int)(c_pad / 4),
                     (int)(x_stride / 4), (uint32_t)threads, pad_word, ep);
  return launch_status();
}
