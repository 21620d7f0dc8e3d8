// The summation steps the LayerNorm row kernels (layernorm.hip, swin_rows.hip) share: a quad's sum, the lane's tree over its quads, the
// wave's xor butterfly - the order layernorm.hip's header states and its error bound rests on.  Not part of the ABI.
#pragma once

#include "conv_gap.h"

namespace dlmcq {

#define DLMCQ_LN_MAX_C 2048

// the sum of one fp32 per lane over the wave: the same bits in all 64 lanes (a + b = b + a)
__device__ __forceinline__ float ln_wave_sum(float t) {
#pragma unroll
  for (int off = DLMCQ_WAVE / 2; off > 0; off >>= 1) t = t + __shfl_xor(t, off, DLMCQ_WAVE);
  return t;
}

// one quad's sum, and the lane's quad sums added pairwise in memory order (N a power of two): a balanced tree over the lane's elements
__device__ __forceinline__ float ln_quad_sum(float x0, float x1, float x2, float x3) { return (x0 + x1) + (x2 + x3); }

template <int N>
__device__ __forceinline__ float ln_tree_sum(float (&t)[N]) {
#pragma unroll
  for (int w = N / 2; w > 0; w >>= 1) {
#pragma unroll
    for (int i = 0; i < w; ++i) t[i] = t[2 * i] + t[2 * i + 1];
  }
  return t[0];
}

}  // namespace dlmcq
