// The row geometry around a Swin block's two Linear layers, as addresses instead of copies.  Between `norm1` and `to_qkv` stand a
// roll and a window partition, behind `to_out` the window reverse, the roll back and the residual add, and between two stages the 2 x 2
// patch merge in front of a LayerNorm: none of it is arithmetic, all of it is a permutation of row addresses of the fp32 token map
// x[B, Hm, Wm, C] (a pointer and strides in floats for b, y and x; channel stride 1 - the contiguous [B, L, C] residual stream is such a
// view, and so is a row-padded buffer).  Two kernels:
//
// layernorm_gather_rows_kernel - nn.LayerNorm of rows GATHERED from the map, to dense rows [M, W] as fp32 and / or the consumer's
// activation codes.  Output row m reads, with the shifts sy, sx and windows of ws x ws tokens (nWy x nWx windows per image):
//     window:  m = ((b nWy + wy) nWx + wx) ws^2 + ty ws + tx  <-  pixel ((wy ws + ty + sy) mod Hm, (wx ws + tx + sx) mod Wm), W = C
//              - torch.roll(x, (-sy, -sx), (1, 2)) followed by the window partition reshape / permute / reshape
//     merge:   m = (b Hm/2 + y2) Wm/2 + x2, four C-wide segments, segment k  <-  pixel (2 y2 + (k & 1), 2 x2 + (k >> 1)), W = 4 C
//              - Swin's cat([x[:, 0::2, 0::2], x[:, 1::2, 0::2], x[:, 0::2, 1::2], x[:, 1::2, 1::2]], -1)
// The arithmetic is layernorm.hip's, step for step - quad sum, lane tree in the GATHERED row's memory order, xor butterfly, true
// division, 1.0f / sqrtf, fl32(fl32(fl32(d r) gamma) + beta), EpiQuant::code4 - so a gathered row's result has the same bits as
// dlmcq_layernorm_rows_f32 on that row materialised; the operation order and the error bound are stated there (layernorm.hip's header,
// DESIGN.md 5.23) and hold here unchanged.  One wave per output row, four consecutive rows (tokens of one window row, neighbouring
// merged pixels) per 256-thread workgroup; the row index is decomposed once per wave on the scalar side (readfirstlane), not per lane;
// lane l owns quads l, l + 64, ... of the gathered row (1, 2, 4 or 8 per lane), a quad's source being its segment's pixel base plus its
// offset inside the segment; every load is 16 bytes, issued before the first add, none under a branch (a quad past the row's end reads
// the last valid quad again and is replaced by +0).  4 B read and 1 B written per element where the LayerNorm, the two permuting copies
// and the consumer's quantise pass move 25.
//
// window_reverse_add_kernel - out[b, y, x, :] = fl32(shortcut[b, y, x, :] + yw[row(b, y, x), :]): the window reverse, the roll back by
// (+sy, +sx) and the residual add as one pass, `row` the window-order row whose token sits at rolled position ((y - sy) mod Hm,
// (x - sx) mod Wm) - the inverse of the window geometry above.  Work is laid out in OUTPUT order: a wave owns four consecutive pixels,
// whose index arithmetic is wave-uniform; the shortcut loads and the stores are coalesced 16-byte pieces of a pixel's channels, and a
// pixel's window row is one contiguous C-row of yw.  One IEEE add per element, the bits of torch's add; fp32 only.  8 B read and 4 B
// written per element where the two copies and the add move 28.
// Neither kernel uses LDS, atomics or scratch: a result depends neither on the launch nor on the row's index.
#include "ln_sums.h"

namespace dlmcq {

// C4: quads per segment (a pixel's channels); W4: quads per gathered row (C4, or 4 C4 merged); nWy x nWx: windows per image, or merged
// pixels per image; the map's strides in quads
struct GatherGeom {
  int C4, W4, Hm, Wm, ws, sy, sx, nWy, nWx;
  int64_t sb4, sy4, sx4;
};

// QPL: quads per lane; W4 <= 64 * QPL (the host picks the smallest that fits)
template <int QPL, bool MERGE>
__global__ __launch_bounds__(DLMCQ_BLOCK) void layernorm_gather_rows_kernel(const float* __restrict__ x, const float* __restrict__ gamma,
                                                                            const float* __restrict__ beta, float* __restrict__ out, int M,
                                                                            float eps, GatherGeom g, ConvEpi ep) {
  const int lane = threadIdx.x & (DLMCQ_WAVE - 1);
  const uint32_t row = __builtin_amdgcn_readfirstlane(blockIdx.x * (DLMCQ_BLOCK / DLMCQ_WAVE) + threadIdx.x / DLMCQ_WAVE);
  if (row >= (uint32_t)M) return;      // (wave-uniform: a wave is one row; there is no barrier below)
  // the row's first pixel, on the scalar side
  uint32_t b, py, px;
  if (MERGE) {
    const uint32_t r = row / (uint32_t)g.nWx;
    px = 2 * (row - r * (uint32_t)g.nWx);
    b = r / (uint32_t)g.nWy;
    py = 2 * (r - b * (uint32_t)g.nWy);
  } else {
    const uint32_t ws = (uint32_t)g.ws, win = row / (ws * ws), t = row - win * ws * ws;
    const uint32_t ty = t / ws, tx = t - ty * ws;
    const uint32_t r = win / (uint32_t)g.nWx, wx = win - r * (uint32_t)g.nWx;
    b = r / (uint32_t)g.nWy;
    py = (r - b * (uint32_t)g.nWy) * ws + ty + (uint32_t)g.sy;      // (< 2 Hm: one conditional subtract is the modulo)
    px = wx * ws + tx + (uint32_t)g.sx;
    py -= py >= (uint32_t)g.Hm ? (uint32_t)g.Hm : 0u;
    px -= px >= (uint32_t)g.Wm ? (uint32_t)g.Wm : 0u;
  }
  const f32x4* xr = reinterpret_cast<const f32x4*>(x) + ((int64_t)b * g.sb4 + (int64_t)py * g.sy4 + (int64_t)px * g.sx4);
  const int W4 = g.W4;
  // every load is issued before the first add, none under a branch: a quad past the row's end reads the row's last quad again and is
  // replaced by +0, as in layernorm_rows_kernel
  f32x4 a[QPL];
#pragma unroll
  for (int j = 0; j < QPL; ++j) {
    const int q = lane + j * DLMCQ_WAVE, qc = q < W4 ? q : W4 - 1;
    if (MERGE) {      // segment k = qc / C4 (0 .. 3) without a division; pixel (+ (k & 1), + (k >> 1))
      const int k = (qc >= g.C4) + (qc >= 2 * g.C4) + (qc >= 3 * g.C4);
      a[j] = xr[(k & 1 ? g.sy4 : 0) + (k >> 1 ? g.sx4 : 0) + (qc - k * g.C4)];
    } else {
      a[j] = xr[qc];
    }
  }
  float t[QPL];
#pragma unroll
  for (int j = 0; j < QPL; ++j) {
    if (!(lane + j * DLMCQ_WAVE < W4)) a[j] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    t[j] = ln_quad_sum(a[j].x, a[j].y, a[j].z, a[j].w);
  }
  const float s = ln_tree_sum<QPL>(t);
  const float fc = (float)(W4 * 4);
  const float mean = ln_wave_sum(s) / fc;
#pragma unroll
  for (int j = 0; j < QPL; ++j) {
    const bool in = lane + j * DLMCQ_WAVE < W4;      // (d = +0 past the row's end, whatever the mean: a NaN mean stays out of it)
    a[j] = f32x4{in ? a[j].x - mean : 0.0f, in ? a[j].y - mean : 0.0f, in ? a[j].z - mean : 0.0f, in ? a[j].w - mean : 0.0f};
    t[j] = ln_quad_sum(a[j].x * a[j].x, a[j].y * a[j].y, a[j].z * a[j].z, a[j].w * a[j].w);
  }
  const float s2 = ln_tree_sum<QPL>(t);
  const float var = ln_wave_sum(s2) / fc;
  const float r = 1.0f / sqrtf(var + eps);
  const EpiQuant eq(ep);
  const int64_t at = (int64_t)row * W4;
#pragma unroll
  for (int j = 0; j < QPL; ++j) {
    const int q = lane + j * DLMCQ_WAVE;
    if (q >= W4) continue;
    f32x4 v = f32x4{a[j].x * r, a[j].y * r, a[j].z * r, a[j].w * r};
    if (gamma) {
      const f32x4 gq = reinterpret_cast<const f32x4*>(gamma)[q];
      v = f32x4{v.x * gq.x, v.y * gq.y, v.z * gq.z, v.w * gq.w};
    }
    if (beta) {
      const f32x4 bq = reinterpret_cast<const f32x4*>(beta)[q];
      v = f32x4{v.x + bq.x, v.y + bq.y, v.z + bq.z, v.w + bq.w};
    }
    if (out) reinterpret_cast<f32x4*>(out)[at + q] = v;
    if (ep.codes) *reinterpret_cast<uint32_t*>(ep.codes + (at + q) * 4) = eq.code4(v);
  }
}

template <int QPL, bool MERGE>
static inline void gather_launch(const float* x, const float* gamma, const float* beta, float* out, int M, float eps, const GatherGeom& g,
                                 const ConvEpi& ep, dlmcq_stream_t stream) {
  constexpr int ROWS = DLMCQ_BLOCK / DLMCQ_WAVE;
  hipLaunchKernelGGL((layernorm_gather_rows_kernel<QPL, MERGE>), dim3((uint32_t)((M + ROWS - 1) / ROWS)), dim3(DLMCQ_BLOCK), 0,
                     reinterpret_cast<hipStream_t>(stream), x, gamma, beta, out, M, eps, g, ep);
}

template <bool MERGE>
static inline void gather_dispatch(const float* x, const float* gamma, const float* beta, float* out, int M, float eps, const GatherGeom& g,
                                   const ConvEpi& ep, dlmcq_stream_t stream) {
  if (g.W4 <= 64) gather_launch<1, MERGE>(x, gamma, beta, out, M, eps, g, ep, stream);
  else if (g.W4 <= 128) gather_launch<2, MERGE>(x, gamma, beta, out, M, eps, g, ep, stream);
  else if (g.W4 <= 256) gather_launch<4, MERGE>(x, gamma, beta, out, M, eps, g, ep, stream);
  else gather_launch<8, MERGE>(x, gamma, beta, out, M, eps, g, ep, stream);
}

#define DLMCQ_WRA_PIXELS 4      // output pixels per wave of window_reverse_add_kernel

// the window geometry of GatherGeom; pixels = B Hm Wm; the strides in quads of the shortcut and of the output
struct ReverseGeom {
  int C4, Hm, Wm, ws, sy, sx, nWy, nWx;
  uint32_t pixels;
  int64_t sb4, sy4, sx4, ob4, oy4, ox4;
};

__global__ __launch_bounds__(DLMCQ_BLOCK) void window_reverse_add_kernel(const f32x4* __restrict__ yw, const f32x4* __restrict__ shortcut,
                                                                         f32x4* __restrict__ out, ReverseGeom g) {
  const int lane = threadIdx.x & (DLMCQ_WAVE - 1);
  const uint32_t p0 = __builtin_amdgcn_readfirstlane(blockIdx.x * (DLMCQ_BLOCK / DLMCQ_WAVE) + threadIdx.x / DLMCQ_WAVE) * DLMCQ_WRA_PIXELS;
  if (p0 >= g.pixels) return;      // (wave-uniform; there is no barrier below)
  // per pixel, on the scalar side: where the shortcut, the output and the window row begin.  A pixel past the last reads the last
  // one's addresses again and stores nothing.
  const f32x4 *sp[DLMCQ_WRA_PIXELS], *yp[DLMCQ_WRA_PIXELS];
  f32x4* op[DLMCQ_WRA_PIXELS];
  const uint32_t ws = (uint32_t)g.ws;
#pragma unroll
  for (int i = 0; i < DLMCQ_WRA_PIXELS; ++i) {
    const uint32_t p = p0 + i < g.pixels ? p0 + i : g.pixels - 1;
    const uint32_t r = p / (uint32_t)g.Wm, x_ = p - r * (uint32_t)g.Wm;
    const uint32_t b = r / (uint32_t)g.Hm, y_ = r - b * (uint32_t)g.Hm;
    const uint32_t ry = y_ >= (uint32_t)g.sy ? y_ - (uint32_t)g.sy : y_ + (uint32_t)(g.Hm - g.sy);      // the rolled position
    const uint32_t rx = x_ >= (uint32_t)g.sx ? x_ - (uint32_t)g.sx : x_ + (uint32_t)(g.Wm - g.sx);
    const uint32_t wy = ry / ws, ty = ry - wy * ws, wx = rx / ws, tx = rx - wx * ws;
    const uint32_t row = ((b * (uint32_t)g.nWy + wy) * (uint32_t)g.nWx + wx) * ws * ws + ty * ws + tx;
    sp[i] = shortcut + ((int64_t)b * g.sb4 + (int64_t)y_ * g.sy4 + (int64_t)x_ * g.sx4);
    op[i] = out + ((int64_t)b * g.ob4 + (int64_t)y_ * g.oy4 + (int64_t)x_ * g.ox4);
    yp[i] = yw + (int64_t)row * g.C4;
  }
  for (int q = lane; q < g.C4; q += DLMCQ_WAVE) {
    f32x4 a[DLMCQ_WRA_PIXELS], t[DLMCQ_WRA_PIXELS];
#pragma unroll
    for (int i = 0; i < DLMCQ_WRA_PIXELS; ++i) {      // (yw is read once: around the cache; the shortcut and out are the residual stream)
      a[i] = sp[i][q];
      t[i] = __builtin_nontemporal_load(yp[i] + q);
    }
#pragma unroll
    for (int i = 0; i < DLMCQ_WRA_PIXELS; ++i)
      if (p0 + i < g.pixels) op[i][q] = f32x4{a[i].x + t[i].x, a[i].y + t[i].y, a[i].z + t[i].z, a[i].w + t[i].w};
  }
}

// What the two entry points' geometry checks share: the map, its channels, the windows and the shifts (DLMCQ_EINVAL else)
static inline bool window_geometry_ok(int64_t B, int64_t Hm, int64_t Wm, int64_t C, int64_t ws, int64_t sy, int64_t sx) {
  return B >= 0 && Hm >= 1 && Wm >= 1 && C >= 4 && C % 4 == 0 && ws >= 1 && Hm % ws == 0 && Wm % ws == 0 && sy >= 0 && sy < Hm && sx >= 0 &&
         sx < Wm;
}

// a map view's strides in floats: multiples of 4, a pixel's channels, a line's pixels and an image's lines not overlapping the next
static inline bool map_strides_ok(int64_t sb, int64_t sy, int64_t sx, int64_t Hm, int64_t Wm, int64_t C) {
  if (sb < 0 || sy < 0 || sx < C || sb % 4 != 0 || sy % 4 != 0 || sx % 4 != 0) return false;
  return (__int128)sy >= (__int128)Wm * sx && (__int128)sb >= (__int128)Hm * sy;
}

}  // namespace dlmcq

using namespace dlmcq;

// The checks, in dlmcq_layernorm_rows_f32's order: geometry (mode, map, channels, row width, windows and shifts, strides) and eps,
// emit_set_quantiser (csrc/conv_gap.h; plain codes only), M == 0, emit_check_pointers, the 2^31 limits.
extern "C" int dlmcq_layernorm_gather_rows_f32(const float* x, const float* gamma, const float* beta, float* out, void* codes, int32_t mode,
                                               int64_t B, int64_t Hm, int64_t Wm, int64_t C, int64_t stride_b, int64_t stride_y,
                                               int64_t stride_x, int64_t ws, int64_t sy, int64_t sx, float eps, const float* q_scale,
                                               const float* q_zero_point, int32_t q_lo, int32_t q_hi, int32_t q_form, float q_ste_g,
                                               dlmcq_stream_t stream) {
  if (mode != DLMCQ_GATHER_WINDOW && mode != DLMCQ_GATHER_MERGE) return DLMCQ_EINVAL;
  const bool merge = mode == DLMCQ_GATHER_MERGE;
  if (merge ? !(window_geometry_ok(B, Hm, Wm, C, 1, 0, 0) && Hm % 2 == 0 && Wm % 2 == 0 && sy == 0 && sx == 0)
            : !window_geometry_ok(B, Hm, Wm, C, ws, sy, sx))
    return DLMCQ_EINVAL;
  const int64_t W = merge ? 4 * C : C;
  if (W > DLMCQ_LN_MAX_C || !map_strides_ok(stride_b, stride_y, stride_x, Hm, Wm, C) || !(eps > 0.0f) || !(eps <= 3.402823466e+38f))
    return DLMCQ_EINVAL;
  ConvEpi ep{};
  int rc = emit_set_quantiser(ep, codes, q_scale, q_zero_point, q_lo, q_hi, q_form, q_ste_g, true);
  if (rc != DLMCQ_OK) return rc;
  if (B == 0) return DLMCQ_OK;
  rc = emit_check_pointers({x}, {gamma, beta}, out, codes, 4);
  if (rc != DLMCQ_OK) return rc;
  constexpr int64_t LIM = 1ll << 31;
  if (B >= LIM || Hm >= LIM || Wm >= LIM || Hm * Wm >= LIM) return DLMCQ_ERANGE;
  const int64_t M = B * (merge ? (Hm / 2) * (Wm / 2) : Hm * Wm);
  if (M >= LIM || M * (W / 4) >= LIM) return DLMCQ_ERANGE;
  const int wsz = merge ? 2 : (int)ws;
  const GatherGeom g{(int)(C / 4), (int)(W / 4), (int)Hm,        (int)Wm,      wsz,         (int)sy,
                     (int)sx,      (int)(Hm / wsz), (int)(Wm / wsz), stride_b / 4, stride_y / 4, stride_x / 4};
  if (merge) gather_dispatch<true>(x, gamma, beta, out, (int)M, eps, g, ep, stream);
  else gather_dispatch<false>(x, gamma, beta, out, (int)M, eps, g, ep, stream);
  return launch_status();
}

// The checks, in the same order without a quantiser (`out` required): geometry and strides, B == 0, null pointers, alignment, the 2^31
// limits, and `out` apart from both inputs.
extern "C" int dlmcq_window_reverse_add_f32(const float* yw, const float* shortcut, float* out, int64_t B, int64_t Hm, int64_t Wm, int64_t C,
                                            int64_t sc_stride_b, int64_t sc_stride_y, int64_t sc_stride_x, int64_t out_stride_b,
                                            int64_t out_stride_y, int64_t out_stride_x, int64_t ws, int64_t sy, int64_t sx,
                                            dlmcq_stream_t stream) {
  if (!window_geometry_ok(B, Hm, Wm, C, ws, sy, sx)) return DLMCQ_EINVAL;
  if (!map_strides_ok(sc_stride_b, sc_stride_y, sc_stride_x, Hm, Wm, C) || !map_strides_ok(out_stride_b, out_stride_y, out_stride_x, Hm, Wm, C))
    return DLMCQ_EINVAL;
  if (B == 0) return DLMCQ_OK;
  if (!yw || !shortcut || !out) return DLMCQ_EINVAL;
  if (!aligned16(yw) || !aligned16(shortcut) || !aligned16(out)) return DLMCQ_EALIGN;
  constexpr int64_t LIM = 1ll << 31;
  if (B >= LIM || Hm >= LIM || Wm >= LIM || Hm * Wm >= LIM) return DLMCQ_ERANGE;
  const int64_t M = B * Hm * Wm;
  if (M >= LIM || M * (C / 4) >= LIM) return DLMCQ_ERANGE;
  // the floats `out` spans against yw's and the shortcut's: an overlap would let one wave read what another has written
  const auto span = [&](int64_t sb, int64_t sy_, int64_t sx_) { return (B - 1) * sb + (Hm - 1) * sy_ + (Wm - 1) * sx_ + C; };
  const auto meet = [](const float* p, int64_t n, const float* q, int64_t m) {
    const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q;
    return a < b + 4 * (uintptr_t)m && b < a + 4 * (uintptr_t)n;
  };
  const int64_t on = span(out_stride_b, out_stride_y, out_stride_x);
  if (meet(out, on, yw, M * C) || meet(out, on, shortcut, span(sc_stride_b, sc_stride_y, sc_stride_x))) return DLMCQ_EINVAL;
  const ReverseGeom g{(int)(C / 4),     (int)Hm,          (int)Wm,          (int)ws,          (int)sy,          (int)sx,         (int)(Hm / ws),
                      (int)(Wm / ws),   (uint32_t)M,      sc_stride_b / 4,  sc_stride_y / 4,  sc_stride_x / 4,  out_stride_b / 4,
                      out_stride_y / 4, out_stride_x / 4};
  const int64_t waves = (M + DLMCQ_WRA_PIXELS - 1) / DLMCQ_WRA_PIXELS;
  constexpr int WAVES = DLMCQ_BLOCK / DLMCQ_WAVE;
  hipLaunchKernelGGL(window_reverse_add_kernel, dim3((uint32_t)((waves + WAVES - 1) / WAVES)), dim3(DLMCQ_BLOCK), 0,
                     reinterpret_cast<hipStream_t>(stream), reinterpret_cast<const f32x4*>(yw), reinterpret_cast<const f32x4*>(shortcut),
                     reinterpret_cast<f32x4*>(out), g);
  return launch_status();
}
