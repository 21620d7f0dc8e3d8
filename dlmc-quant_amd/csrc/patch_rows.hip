// The front of a vision transformer: an fp32 image batch [B, C, gh p, gw p] (element strides sb, sc, sh; unit stride along w) to the
// patch rows [B gh gw, p p C] - row (b, gy, gx), column (py p + px) C + c holds img[b, c, gy p + py, gx p + px], the rearrangement
// 'b c (h p1) (w p2) -> b (h w) (p1 p2 c)' - as fp32 and / or as the activation codes of the Linear layer that embeds them: the strided
// copy and the consumer's quantise pass as ONE read of the image - 4 B in, 1 B out per element, where the copy and the quantise pass
// move 13.  There is no arithmetic but the quantiser's (EpiQuant::code4: the code dlmcq_fake_quant_f32 gives for the value; NaN,
// infinities and -0 as there): every element is moved and, for the codes, quantised once.
// One 256-thread workgroup owns one (b, gy) strip: C p image lines of gw p floats in, gw consecutive rows out - the strip's codes are
// ONE contiguous block of gw p p C bytes.  A wave takes a line at a time (four lines in flight: every load is issued before the first
// value is used), lane l the line's float4 l, l + 64, ...: coalesced along w, read once, non-temporal.  A float4 lies inside one patch
// (p % 4 == 0) and its four codes belong to columns C apart, so they are staged as four bytes in LDS in output order (consecutive lanes
// 4 C bytes apart: no bank is hit twice by one store while C is odd - C = 3, C = 1 -, twice at C = 2, four times at C = 4) and, after
// one barrier, the block is copied out as contiguous 16-byte pieces (4-byte pieces where gw p p C is no multiple of 16).  LDS:
// gw p p C bytes, 10.5 KiB at 224^2 / 16 / 3 - eight workgroups per CU, the thread limit.
// The fp32 rows, when asked for, are stored from the registers directly, four 4-byte stores C floats apart: staging them like the
// codes would take four times the LDS (42 KiB at 224^2 / 16 / 3: three workgroups per CU for the codes too, were it one kernel) and
// the plan never asks - the rows' only reader there is the embedding, which takes the codes.  No atomics, no scratch: a row's result
// depends neither on B nor on the launch.
#include "conv_gap.h"

namespace dlmcq {

#define DLMCQ_PATCH_MAX_STRIP 65536      // bytes of LDS a strip's codes may take: what a launch may ask for without raising the limit
#define DLMCQ_PATCH_LINES 4              // lines a wave has in flight

// C, p, gh, gw; W4 = gw p / 4 (float4 per line); K = p p C (a row); lines = C p (of a strip); the image's element strides
struct PatchGeom {
  int C, p, gh, gw, W4, K, lines;
  int64_t sb, sc, sh;
};

// VEC16: gw K % 16 == 0 - every strip's block of codes starts and ends on a 16-byte boundary (the base is 16-byte aligned)
template <bool VEC16>
__global__ __launch_bounds__(DLMCQ_BLOCK) void patch_rows_kernel(const float* __restrict__ img, float* __restrict__ out, PatchGeom g,
                                                                 ConvEpi ep) {
  extern __shared__ __attribute__((aligned(16))) uint8_t strip[];      // [gw][K]: the strip's codes in output order
  const int b = blockIdx.x / g.gh, gy = blockIdx.x - b * g.gh;
  const int lane = threadIdx.x & (DLMCQ_WAVE - 1);
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / DLMCQ_WAVE);
  constexpr int WAVES = DLMCQ_BLOCK / DLMCQ_WAVE;
  const float* base = img + (int64_t)b * g.sb + (int64_t)gy * g.p * g.sh;
  const int64_t row0 = (int64_t)blockIdx.x * g.gw;      // the strip's first row
  const EpiQuant eq(ep);
  for (int l0 = wave; l0 < g.lines; l0 += WAVES * DLMCQ_PATCH_LINES) {
    // (everything about a line is wave-uniform: the line, its channel and patch row, whether it exists)
    int at[DLMCQ_PATCH_LINES];           // column of the line's pixel px = 0: (py p) C + c
    const f32x4* src[DLMCQ_PATCH_LINES];
#pragma unroll
    for (int u = 0; u < DLMCQ_PATCH_LINES; ++u) {
      const int line = l0 + u * WAVES < g.lines ? l0 + u * WAVES : l0;      // (a line past the strip's end: the first one again, not used)
      const int c = line / g.p, py = line - c * g.p;
      at[u] = py * g.p * g.C + c;
      src[u] = reinterpret_cast<const f32x4*>(base + (int64_t)c * g.sc + (int64_t)py * g.sh);
    }
    for (int x4 = lane; x4 < g.W4; x4 += DLMCQ_WAVE) {
      f32x4 v[DLMCQ_PATCH_LINES];
#pragma unroll
      for (int u = 0; u < DLMCQ_PATCH_LINES; ++u) v[u] = __builtin_nontemporal_load(src[u] + x4);
      const int gx = (4 * x4) / g.p, px = 4 * x4 - gx * g.p;
#pragma unroll
      for (int u = 0; u < DLMCQ_PATCH_LINES; ++u) {
        if (l0 + u * WAVES >= g.lines) break;
        const int col = at[u] + px * g.C;      // of v.x; v.y, v.z, v.w: C, 2 C, 3 C further
        if (out) {
          float* o = out + (row0 + gx) * g.K + col;
          o[0] = v[u].x;
          o[g.C] = v[u].y;
          o[2 * g.C] = v[u].z;
          o[3 * g.C] = v[u].w;
        }
        if (ep.codes) {
          const uint32_t w = eq.code4(v[u]);
          uint8_t* s = strip + gx * g.K + col;
          s[0] = (uint8_t)w;
          s[g.C] = (uint8_t)(w >> 8);
          s[2 * g.C] = (uint8_t)(w >> 16);
          s[3 * g.C] = (uint8_t)(w >> 24);
        }
      }
    }
  }
  if (!ep.codes) return;      // (uniform over the launch)
  __syncthreads();
  uint8_t* dst = ep.codes + row0 * g.K;
  const int bytes = g.gw * g.K;
  if (VEC16) {
    for (int i = threadIdx.x; i < bytes / 16; i += DLMCQ_BLOCK) reinterpret_cast<uint4*>(dst)[i] = reinterpret_cast<const uint4*>(strip)[i];
  } else {
    for (int i = threadIdx.x; i < bytes / 4; i += DLMCQ_BLOCK) reinterpret_cast<uint32_t*>(dst)[i] = reinterpret_cast<const uint32_t*>(strip)[i];
  }
}

}  // namespace dlmcq

using namespace dlmcq;

// The checks: geometry, emit_set_quantiser (csrc/conv_gap.h; plain codes only), B == 0, emit_check_pointers (the code rows are written
// 16 bytes at a time), the 2^31 limits.
extern "C" int dlmcq_patch_rows_f32(const float* img, float* out, void* codes, int64_t B, int64_t C, int64_t gh, int64_t gw, int64_t p,
                                    int64_t sb, int64_t sc, int64_t sh, const float* q_scale, const float* q_zero_point, int32_t q_lo,
                                    int32_t q_hi, int32_t q_form, float q_ste_g, dlmcq_stream_t stream) {
  constexpr int64_t LIM = 1ll << 31;
  if (B < 0 || C < 1 || gh < 1 || gw < 1 || p < 4 || p % 4 != 0) return DLMCQ_EINVAL;
  if (sb < 0 || sc < 0 || sh < 0 || sb % 4 != 0 || sc % 4 != 0 || sh % 4 != 0) return DLMCQ_EINVAL;
  // the strip's codes fit the LDS a launch may ask for (p p C % 4 == 0 follows from p % 4 == 0; each factor is bounded by the limit
  // before it is multiplied: no overflow) - which also keeps W = gw p, K = p p C and the strip's line count far below 2^31
  if (C > DLMCQ_PATCH_MAX_STRIP || gw > DLMCQ_PATCH_MAX_STRIP || p > 256 ||gw * (p * p * C) > DLMCQ_PATCH_MAX_STRIP)
    return DLMCQ_EINVAL;
  ConvEpi ep{};
  int rc = emit_set_quantiser(ep, codes, q_scale, q_zero_point, q_lo, q_hi, q_form, q_ste_g, true);
  if (rc != DLMCQ_OK) return rc;
  if (B == 0) return DLMCQ_OK;
  rc = emit_check_pointers({img}, {}, out, codes, 16);
  if (rc != DLMCQ_OK) return rc;
  if (B >= LIM || gh >= LIM || B * gh >= LIM || B * gh * gw >= LIM || gh * p >= LIM) return DLMCQ_ERANGE;
  const int k = (int)(p * p * C);
  const PatchGeom g{(int)C, (int)p, (int)gh, (int)gw, (int)(gw * p / 4), k, (int)(C * p), sb, sc, sh};
  const size_t lds = codes ? (size_t)(gw * k) : 0;
  const dim3 grid((uint32_t)(B * gh)), block(DLMCQ_BLOCK);
  if ((gw * k) % 16 == 0)
    hipLaunchKernelGGL((patch_rows_kernel<true>), grid, block, lds, reinterpret_cast<hipStream_t>(stream), img, out, g, ep);
  else
    hipLaunchKernelGGL((patch_rows_kernel<false>), grid, block, lds, reinterpret_cast<hipStream_t>(stream), img, out, g, ep);
  return launch_status();
}
