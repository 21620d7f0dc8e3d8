// The token tensor in front of a transformer's first block: the class token put before the embedded patches and the position embedding
// added, `torch.cat((cls.expand(B, -1, -1), e), 1) + pos`, as ONE pass - 8 B read and 4 B written per element (pos stays in the cache:
// every image reads the same rows), where the concatenation and the add move 20.  For image b:
//     out[b, 0, :]     = fl32(cls[:] + pos[0, :])
//     out[b, 1 + i, :] = fl32(e[b, i, :] + pos[1 + i, :])      i = 0 .. T - 1
// - one IEEE add per element, the bits of torch's add in either operand order (a + b = b + a; a NaN's payload aside).  fp32 only: the
// readers are the residual stream and the first block's LayerNorm node, which read fp32.
// One thread per float4 of the output; e is read once (non-temporal), out is read again by the block behind it (plain stores).  No
// LDS, no atomics, no scratch.
#include "dlmcq_internal.h"

namespace dlmcq {

// C4 = C / 4; R = T + 1 rows per image; the strides in float4: e's rows, out's images and rows; total = B R C4 threads
struct TokenGeom {
  int C4, R;
  uint32_t total;
  int64_t es4, ob4, or4;
};

__global__ __launch_bounds__(DLMCQ_BLOCK) void tokens_assemble_kernel(const f32x4* __restrict__ e, const f32x4* __restrict__ cls,
                                                                      const f32x4* __restrict__ pos, f32x4* __restrict__ out, TokenGeom g) {
  const uint32_t idx = blockIdx.x * (uint32_t)DLMCQ_BLOCK + threadIdx.x;
  if (idx >= g.total) return;
  const uint32_t m = idx / (uint32_t)g.C4, c4 = idx - m * (uint32_t)g.C4;      // m: the output row b R + r
  const uint32_t b = m / (uint32_t)g.R, r = m - b * (uint32_t)g.R;
  const f32x4 t = pos[(int64_t)r * g.C4 + c4];
  // (e's rows are [B T] with one stride: row b T + r - 1)
  const f32x4 a = r == 0 ? cls[c4] : __builtin_nontemporal_load(e + ((int64_t)b * (g.R - 1) + (r - 1)) * g.es4 + c4);
  out[(int64_t)b * g.ob4 + (int64_t)r * g.or4 + c4] = f32x4{a.x + t.x, a.y + t.y, a.z + t.z, a.w + t.w};
}

}  // namespace dlmcq

using namespace dlmcq;

// The checks, in the order of csrc/conv_gap.h's helpers (no quantiser, `out` required): geometry, B == 0, null pointers, alignment, 2^31 limits.
extern "C" int dlmcq_tokens_assemble_f32(const float* e, const float* cls, const float* pos, float* out, int64_t B, int64_t T, int64_t C,
                                         int64_t e_stride, int64_t o_sb, int64_t o_st, dlmcq_stream_t stream) {
  constexpr int64_t LIM = 1ll << 31;
  if (B < 0 || T < 1 || C < 4 || C % 4 != 0) return DLMCQ_EINVAL;
  if (e_stride < C || e_stride % 4 != 0 || o_st < C || o_st % 4 != 0 || o_sb % 4 != 0) return DLMCQ_EINVAL;
  // an image's rows end before the next image's begin (the writes of two images never meet)
  if (T < LIM && o_st < LIM && C < LIM && o_sb < T * o_st + C) return DLMCQ_EINVAL;
  if (B == 0) return DLMCQ_OK;
  if (!e || !cls || !pos || !out) return DLMCQ_EINVAL;
  if (!aligned16(e) || !aligned16(cls) || !aligned16(pos) || !aligned16(out)) return DLMCQ_EALIGN;
  if (B >= LIM || T + 1 >= LIM || C >= LIM || e_stride >= LIM || o_st >= LIM || B * (T + 1) >= LIM || B * (T + 1) * (C / 4) >= LIM) return DLMCQ_ERANGE;
  const TokenGeom g{(int)(C / 4), (int)(T + 1), (uint32_t)(B * (T + 1) * (C / 4)), e_stride / 4, o_sb / 4, o_st / 4};
  hipLaunchKernelGGL(tokens_assemble_kernel, dim3((g.total + DLMCQ_BLOCK - 1) / DLMCQ_BLOCK), dim3(DLMCQ_BLOCK), 0,
                     reinterpret_cast<hipStream_t>(stream), reinterpret_cast<const f32x4*>(e), reinterpret_cast<const f32x4*>(cls),
                     reinterpret_cast<const f32x4*>(pos), reinterpret_cast<f32x4*>(out), g);
  return launch_status();
}
