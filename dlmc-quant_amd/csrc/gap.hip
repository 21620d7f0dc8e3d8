// Global average pool of an fp32 NHWC map to fp32 [N, C] and / or the consumer's activation codes [N, C] (the tail of every network
// the plan runs: last layer -> ReLU -> pool -> flatten -> quantised Linear).  One definition of the arithmetic, shared with the fused
// head kernel (conv_gap_i8.hip) through gap_finish4 below:
//     s = v[n, 0, k];  for p = 1 .. HW - 1: s = fl32(s + v[n, p, k]);  pooled = fl32(s / fl32(HW));  code = the consumer's quantiser
// A sequential fp32 sum in pixel order, no atomics, a true IEEE division: the result depends neither on the launch geometry nor on
// the run.  (torch's mean sums in another order; the plan with this node is compared against a restatement of the lines above.)
// One thread per (image, 4 channels): float4 loads coalesced over channels, one read of the map, no scratch.
#include "conv_gap.h"

namespace dlmcq {

__global__ __launch_bounds__(DLMCQ_BLOCK) void gap_nhwc_kernel(const float* __restrict__ x, float* __restrict__ pooled, int N, int HW,
                                                               int C4, ConvEpi ep) {
  const uint32_t idx = blockIdx.x * (uint32_t)DLMCQ_BLOCK + threadIdx.x;
  if (idx >= (uint32_t)N * (uint32_t)C4) return;
  const uint32_t n = idx / (uint32_t)C4, c4 = idx - n * (uint32_t)C4;
  const f32x4* p = reinterpret_cast<const f32x4*>(x) + (int64_t)n * HW * C4 + c4;
  f32x4 s = __builtin_nontemporal_load(p);
#pragma unroll 8
  for (int i = 1; i < HW; ++i) {
    const f32x4 v = __builtin_nontemporal_load(p + (int64_t)i * C4);
    s = f32x4{s.x + v.x, s.y + v.y, s.z + v.z, s.w + v.w};
  }
  const EpiQuant eq(ep);
  gap_finish4(s, HW, eq, pooled, ep.codes, (int64_t)idx * 4);
}

}  // namespace dlmcq

using namespace dlmcq;

extern "C" int dlmcq_gap_nhwc_f32(const float* x, float* pooled, void* codes, int64_t N, int64_t HW, int64_t C, const float* q_scale,
                                  const float* q_zero_point, int32_t q_lo, int32_t q_hi, int32_t q_form, float q_ste_g,
                                  dlmcq_stream_t stream) {
  if (N < 0 || HW < 1 || C < 4 || C % 4 != 0) return DLMCQ_EINVAL;
  ConvEpi ep{};
  int rc = emit_set_quantiser(ep, codes, q_scale, q_zero_point, q_lo, q_hi, q_form, q_ste_g, false);
  if (rc != DLMCQ_OK) return rc;
  if (N == 0) return DLMCQ_OK;
  rc = emit_check_pointers({x}, {}, pooled, codes, 4);
  if (rc != DLMCQ_OK) return rc;
  if (N * (C / 4) >= (1ll << 31) || HW >= (1ll << 31)) return DLMCQ_ERANGE;
  const int64_t threads = N * (C / 4);
  hipLaunchKernelGGL(gap_nhwc_kernel, dim3((uint32_t)((threads + DLMCQ_BLOCK - 1) / DLMCQ_BLOCK)), dim3(DLMCQ_BLOCK), 0,
                     reinterpret_cast<hipStream_t>(stream), x, pooled, (int)N, (int)HW, (int)(C / 4), ep);
  return launch_status();
}
