// LayerNorm over the last dimension of dense fp32 rows [M, C] to fp32 [M, C] and / or the consumer's activation codes [M, C]: the
// normalisation and the quantise pass of the Linear layer that reads the normalised rows as ONE read of the rows - 4 B in, 1 B out per
// element, where a LayerNorm launch and the consumer's own quantise pass move 13.  The arithmetic, once, for a row x[0 .. C - 1] held
// as C / 4 quads of 4 floats, lane l of the row's wave owning quads l, l + 64, l + 128, ...:
//     q_j  = fl32(fl32(x0 + x1) + fl32(x2 + x3)) of the lane's j-th quad                  (a quad past the row's end: +0)
//     s_l  = the lane's q_j added pairwise in memory order: (q0 + q1) + (q2 + q3), ... - a balanced tree over the lane's elements
//     S    = the 64 lane sums combined by an xor butterfly, strides 32, 16, 8, 4, 2, 1 (t += the partner's t; the same bits in every lane)
//     mean = fl32(S / (float)C)                                                       (a true division, correctly rounded)
//     d    = fl32(x - mean)
//     S2   = the same two-level sum of fl32(d * d)
//     var  = fl32(S2 / (float)C)                                                      (the biased variance, as nn.LayerNorm)
//     r    = fl32(1.0f / sqrtf(fl32(var + eps)))                                      (sqrt and division both correctly rounded)
//     v    = fl32(fl32(fl32(d * r) * gamma) + beta)                                   (no gamma: no multiply; no beta: no add)
//     code = the consumer's quantiser of v                                            (EpiQuant::code4)
// - each step rounded to fp32 by itself under the library's flags (-ffp-contract=off, -fno-fast-math, correctly rounded division and
// square root, denormals kept).  The two-pass form (deviations from the rounded mean) keeps var >= 0 and makes a constant row whose
// sum is exact (100.0) come out as d = 0, v = beta exactly.  A NaN or an infinity anywhere in a row makes mean NaN (inf - inf for an
// infinity: d = x - mean is NaN at the infinity itself, and S2 with it), hence every v of the row NaN.
// Against the real n * gamma + beta, n = (x - mean) / sqrt(var + eps) of the same fp32 inputs, with
// u = 2^-23 (|n gamma| + |beta| + |gamma| max_row|x| / sqrt(var + eps)): |v - ref| <= 2 u (the first two terms are the
// roundings of d * r * gamma + beta, the third the rounding of the mean carried through d; the factor 2 is the margin for the second
// order).  The lane sum is a tree, not a running sum, because the running sum misses that bound: a lane of a 2048-wide row of the
// constant 0.1 would add 32 equal values one by one, every add above 1.6 rounding the same way, and the mean would come out 4 ulp low
// (2.5 u; 1.25 u at 768).  The tree has 5 levels where the running sum has 32 steps, adds equal values exactly wherever the lane's quad
// count is a power of two, and costs the same adds.  Measured: at most 0.85 u over the tests' rows.
// One wave owns one row, four rows per 256-thread workgroup; a row is loaded once, as float4, into at most 32 registers per lane
// (kernels for 1, 2, 4 and 8 quads per lane: C <= 256, 512, 1024, 2048) with PLAIN loads - the rows are the residual stream, which the
// block's add reads again.  No LDS, no atomics, no scratch: a row's result depends neither on M nor on the row's index nor on the launch.
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

// QPL: quads per lane; C4 <= 64 * QPL (the host picks the smallest that fits)
template <int QPL>
__global__ __launch_bounds__(DLMCQ_BLOCK) void layernorm_rows_kernel(const float* __restrict__ x, const float* __restrict__ gamma,
                                                                     const float* __restrict__ beta, float* __restrict__ out, int M, int C4,
                                                                     float eps, ConvEpi ep) {
  const int lane = threadIdx.x & (DLMCQ_WAVE - 1);
  const int64_t row = (int64_t)blockIdx.x * (DLMCQ_BLOCK / DLMCQ_WAVE) + (threadIdx.x / DLMCQ_WAVE);
  if (row >= M) return;      // (wave-uniform: a wave is one row; there is no barrier below)
  const f32x4* xr = reinterpret_cast<const f32x4*>(x) + row * C4;
  // every load is issued before the first add, none under a branch: a quad past the row's end reads the row's last quad again (one
  // cache line for all such lanes) and is replaced by +0, which the sums do not see (t + (+0) = t; a -0 partial sum becomes +0, the same mean)
  f32x4 a[QPL];
#pragma unroll
  for (int j = 0; j < QPL; ++j) {
    const int q = lane + j * DLMCQ_WAVE;
    a[j] = xr[q < C4 ? q : C4 - 1];
  }
  float t[QPL];
#pragma unroll
  for (int j = 0; j < QPL; ++j) {
    if (!(lane + j * DLMCQ_WAVE < C4)) a[j] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    t[j] = ln_quad_sum(a[j].x, a[j].y, a[j].z, a[j].w);
  }
  const float s = ln_tree_sum<QPL>(t);
  const float fc = (float)(C4 * 4);
  const float mean = ln_wave_sum(s) / fc;
#pragma unroll
  for (int j = 0; j < QPL; ++j) {
    const bool in = lane + j * DLMCQ_WAVE < C4;      // (d = +0 past the row's end, whatever the mean: a NaN mean stays out of it)
    a[j] = f32x4{in ? a[j].x - mean : 0.0f, in ? a[j].y - mean : 0.0f, in ? a[j].z - mean : 0.0f, in ? a[j].w - mean : 0.0f};
    t[j] = ln_quad_sum(a[j].x * a[j].x, a[j].y * a[j].y, a[j].z * a[j].z, a[j].w * a[j].w);
  }
  const float s2 = ln_tree_sum<QPL>(t);
  const float var = ln_wave_sum(s2) / fc;
  const float r = 1.0f / sqrtf(var + eps);
  const EpiQuant eq(ep);
#pragma unroll
  for (int j = 0; j < QPL; ++j) {
    const int q = lane + j * DLMCQ_WAVE;
    if (q >= C4) continue;
    f32x4 v = f32x4{a[j].x * r, a[j].y * r, a[j].z * r, a[j].w * r};
    if (gamma) {
      const f32x4 g = reinterpret_cast<const f32x4*>(gamma)[q];
      v = f32x4{v.x * g.x, v.y * g.y, v.z * g.z, v.w * g.w};
    }
    if (beta) {
      const f32x4 b = reinterpret_cast<const f32x4*>(beta)[q];
      v = f32x4{v.x + b.x, v.y + b.y, v.z + b.z, v.w + b.w};
    }
    if (out) reinterpret_cast<f32x4*>(out)[row * C4 + q] = v;
    if (ep.codes) *reinterpret_cast<uint32_t*>(ep.codes + (row * C4 + q) * 4) = eq.code4(v);
  }
}

template <int QPL>
static inline void layernorm_launch(const float* x, const float* gamma, const float* beta, float* out, int M, int C4, float eps,
                                    const ConvEpi& ep, dlmcq_stream_t stream) {
  constexpr int ROWS = DLMCQ_BLOCK / DLMCQ_WAVE;
  hipLaunchKernelGGL((layernorm_rows_kernel<QPL>), dim3((uint32_t)((M + ROWS - 1) / ROWS)), dim3(DLMCQ_BLOCK), 0,
                     reinterpret_cast<hipStream_t>(stream), x, gamma, beta, out, M, C4, eps, ep);
}

}  // namespace dlmcq

using namespace dlmcq;

// The checks: geometry and eps, emit_set_quantiser (csrc/conv_gap.h; plain codes only), M == 0, emit_check_pointers, the 2^31 limits.
extern "C" int dlmcq_layernorm_rows_f32(const float* x, const float* gamma, const float* beta, float* out, void* codes, int64_t M, int64_t C,
                                        float eps, const float* q_scale, const float* q_zero_point, int32_t q_lo, int32_t q_hi,
                                        int32_t q_form, float q_ste_g, dlmcq_stream_t stream) {
  if (M < 0 || C < 4 || C % 4 != 0 || C > DLMCQ_LN_MAX_C || !(eps > 0.0f) || !(eps <= 3.402823466e+38f)) return DLMCQ_EINVAL;
  ConvEpi ep{};
  int rc = emit_set_quantiser(ep, codes, q_scale, q_zero_point, q_lo, q_hi, q_form, q_ste_g, true);
  if (rc != DLMCQ_OK) return rc;
  if (M == 0) return DLMCQ_OK;
  rc = emit_check_pointers({x}, {gamma, beta}, out, codes, 4);
  if (rc != DLMCQ_OK) return rc;
  constexpr int64_t LIM = 1ll << 31;
  if (M >= LIM || M * (C / 4) >= LIM) return DLMCQ_ERANGE;
  const int m = (int)M, c4 = (int)(C / 4);
  if (c4 <= 64) layernorm_launch<1>(x, gamma, beta, out, m, c4, eps, ep, stream);
  else if (c4 <= 128) layernorm_launch<2>(x, gamma, beta, out, m, c4, eps, ep, stream);
  else if (c4 <= 256) layernorm_launch<4>(x, gamma, beta, out, m, c4, eps, ep, stream);
  else layernorm_launch<8>(x, gamma, beta, out, m, c4, eps, ep, stream);
  return launch_status();
}
