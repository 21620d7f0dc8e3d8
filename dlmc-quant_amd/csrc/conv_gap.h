// What the two global-average-pool kernels (gap.hip, conv_gap_i8.hip) share: the tail of the pooling arithmetic and the host-side
// reading of the quantiser arguments - and, for every entry point that hands its readers codes, the quantiser and pointer checks
// (emit_set_quantiser, emit_check_pointers).  Not part of the ABI.
#pragma once

#include <initializer_list>

#include "conv_epilogue.h"

namespace dlmcq {

// s = the sequential fp32 sum of 4 channels over HW pixels -> pooled = s / HW (true division) -> fp32 and / or the consumer's codes at
// element offset `at` (a multiple of 4) of the [N, C] outputs
__device__ __forceinline__ void gap_finish4(const f32x4& s, int HW, const EpiQuant& eq, float* pooled, uint8_t* codes, int64_t at) {
  const float d = (float)HW;
  const f32x4 m = f32x4{s.x / d, s.y / d, s.z / d, s.w / d};
  if (pooled) *reinterpret_cast<f32x4*>(pooled + at) = m;
  if (codes) *reinterpret_cast<uint32_t*>(codes + at) = eq.code4(m);
}

// the seven quantiser arguments of an entry point -> ep (codes, constants, form, shifted emission, control bits in ep.ctl), checked
// as conv_launch (csrc/conv_i8.hip) checks them; which control bits it takes is the caller's to say
static inline int gap_set_quantiser(ConvEpi& ep, void* codes, const float* q_scale, const float* q_zero_point, int32_t q_lo, int32_t q_hi,
                                    int32_t q_form, float q_ste_g) {
  ep = make_epi(nullptr, 0, codes, q_scale, q_zero_point, q_lo, q_hi, q_form, q_ste_g);
  if (ep.q_form < 0) return DLMCQ_EINVAL;
  return quantiser_check(codes, q_scale, q_lo, q_hi, ep.q_form, 0);     // (the form: already without its flags)
}

// The two steps every entry point that hands its readers codes shares (map_codes.h, layernorm.hip, patch_rows.hip, attention.hip,
// gap.hip) - between them stands the caller's own empty-problem return, in front its geometry check, behind its 2^31 limits: that
// order decides which code an argument set with two faults gets.
// One: gap_set_quantiser, then every control / layout bit refused, not stripped (row-major only, no route query) and - `plain_only`:
// the readers are Linear layers, which take plain codes - the shifted emission too.
static inline int emit_set_quantiser(ConvEpi& ep, void* codes, const float* q_scale, const float* q_zero_point, int32_t q_lo, int32_t q_hi,
                                     int32_t q_form, float q_ste_g, bool plain_only) {
  const int rc = gap_set_quantiser(ep, codes, q_scale, q_zero_point, q_lo, q_hi, q_form, q_ste_g);
  if (rc != DLMCQ_OK) return rc;
  return (ep.ctl || (plain_only && ep.q_xor)) ? DLMCQ_EINVAL : DLMCQ_OK;
}

// Two: something to produce and every `required` input there, else DLMCQ_EINVAL; then the alignment, else DLMCQ_EALIGN: the fp32
// pointers (`required`, `optional`, `out`) at 16 bytes, `codes` at `codes_align` (4 or 16) bytes.  NULL is aligned.
static inline int emit_check_pointers(std::initializer_list<const void*> required, std::initializer_list<const void*> optional,
                                      const void* out, const void* codes, uintptr_t codes_align) {
  if (!(out || codes)) return DLMCQ_EINVAL;
  for (const void* p : required)
    if (!p) return DLMCQ_EINVAL;
  for (const void* p : required)
    if (!aligned16(p)) return DLMCQ_EALIGN;
  for (const void* p : optional)
    if (!aligned16(p)) return DLMCQ_EALIGN;
  return (!aligned16(out) || ((uintptr_t)codes & (codes_align - 1))) ? DLMCQ_EALIGN : DLMCQ_OK;
}

// What the two attention entry points (attention.hip, attention_f16.hip) share: the kernel arguments and the host checks in front of
// the launch.  A workgroup of either kernel owns DLMCQ_AT_ROWS query rows of one (b, h).
#define DLMCQ_AT_WAVES 4
#define DLMCQ_AT_ROWS (32 * DLMCQ_AT_WAVES)      // query rows per workgroup
#define DLMCQ_AT_KB 32                           // keys per block

struct AttnArgs {
  const float *q, *k, *v;
  float* out;
  int64_t qs[3], ks[3], vs[3], os[3];      // element strides (batch, head, token)
  int H, Tq, Tk, tiles;
  float scale;
};

// The checks: geometry (sizes, D, strides, scale), emit_set_quantiser (plain codes only: the reader is a Linear layer), an empty
// problem (DLMCQ_OK with *grid = 0: nothing to launch), emit_check_pointers, the 2^31 limits.  Else `a`, `ep` and *grid are set.
static inline int attention_args(AttnArgs& a, ConvEpi& ep, int64_t* grid, const float* q, const float* k, const float* v, float* out,
                                 void* codes, int64_t B, int64_t H, int64_t Tq, int64_t Tk, int64_t D, const int64_t (&strides)[12],
                                 float scale, const float* q_scale, const float* q_zero_point, int32_t q_lo, int32_t q_hi, int32_t q_form,
                                 float q_ste_g) {
  *grid = 0;
  if (B < 0 || H < 0 || Tq < 0 || Tk < 1 || (D != 32 && D != 64) || !(scale == scale) || !(scale > -3.402823466e+38f && scale < 3.402823466e+38f))
    return DLMCQ_EINVAL;
  for (int i = 0; i < 12; ++i)
    if (strides[i] < 0 || strides[i] % 4 != 0) return DLMCQ_EINVAL;
  for (int i = 2; i < 12; i += 3)
    if (strides[i] < D) return DLMCQ_EINVAL;      // (unit stride in D: a token's row does not overlap the next)
  ep = ConvEpi{};
  int rc = emit_set_quantiser(ep, codes, q_scale, q_zero_point, q_lo, q_hi, q_form, q_ste_g, true);
  if (rc != DLMCQ_OK) return rc;
  if (B == 0 || H == 0 || Tq == 0) return DLMCQ_OK;
  rc = emit_check_pointers({q, k, v}, {}, out, codes, 4);
  if (rc != DLMCQ_OK) return rc;
  constexpr int64_t LIM = 1ll << 31;
  const int64_t tiles = (Tq + DLMCQ_AT_ROWS - 1) / DLMCQ_AT_ROWS;
  if (B >= LIM || H >= LIM || Tq >= LIM || Tk >= LIM || B * H >= LIM || B * H * tiles >= LIM) return DLMCQ_ERANGE;
  a = AttnArgs{q, k, v, out, {strides[0], strides[1], strides[2]}, {strides[3], strides[4], strides[5]}, {strides[6], strides[7], strides[8]},
               {strides[9], strides[10], strides[11]}, (int)H, (int)Tq, (int)Tk, (int)tiles, scale};
  *grid = B * H * tiles;
  return DLMCQ_OK;
}

// What the two window attention entry points (window_attention.hip, window_attention_f16.hip) share: the kernel arguments, the
// additive term's read and the host checks in front of the launch.  A workgroup of either kernel is DLMCQ_WA_WAVES waves, one (b, h) each.
#define DLMCQ_WA_WAVES 4      // (b, h) pairs per workgroup
#define DLMCQ_WA_TMAX 64

typedef float f32x16 __attribute__((ext_vector_type(16)));

struct WinAttnArgs {
  const float *q, *k, *v, *bias, *mask;
  float* out;
  int64_t qs[3], ks[3], vs[3], os[3];      // element strides (batch, head, token)
  int64_t bias_sh, bias_st, mask_sw, mask_st;
  int H, T, nW, pairs;
  float scale;
};

// s += the additive term's row `row` (this lane's query), keys key0 + 8 g .. + 3 in registers 4 g .. 4 g + 3: four 16-byte pieces
__device__ __forceinline__ void add_term(f32x16& s, const float* row, int key0, int T) {
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    const int j = key0 + 8 * g;
    const f32x4 t = *reinterpret_cast<const f32x4*>(row + (j < T ? j : 0));
    s[4 * g] += t.x, s[4 * g + 1] += t.y, s[4 * g + 2] += t.z, s[4 * g + 3] += t.w;
  }
}

// The checks, in map_codes_call's order: geometry (sizes, D, T, strides, scale, the additive terms' layout), emit_set_quantiser
// (plain codes only: the reader is a Linear layer), an empty problem (DLMCQ_OK with *grid = 0: nothing to launch),
// emit_check_pointers, the 2^31 limits.  Else `a`, `ep` and *grid (workgroups) are set.
static inline int window_attention_args(WinAttnArgs& a, ConvEpi& ep, int64_t* grid, const float* q, const float* k, const float* v,
                                        const float* bias, const float* mask, float* out, void* codes, int64_t B, int64_t H, int64_t T,
                                        int64_t D, int64_t nW, const int64_t (&strides)[12], int64_t bias_sh, int64_t bias_st,
                                        int64_t mask_sw, int64_t mask_st, float scale, const float* q_scale, const float* q_zero_point,
                                        int32_t q_lo, int32_t q_hi, int32_t q_form, float q_ste_g) {
  *grid = 0;
  if (B < 0 || H < 0 || T < 1 || T > DLMCQ_WA_TMAX || (D != 32 && D != 64) || !(scale == scale) ||
      !(scale > -3.402823466e+38f && scale < 3.402823466e+38f))
    return DLMCQ_EINVAL;
  for (int i = 0; i < 12; ++i)
    if (strides[i] < 0 || strides[i] % 4 != 0) return DLMCQ_EINVAL;
  for (int i = 2; i < 12; i += 3)
    if (strides[i] < D) return DLMCQ_EINVAL;      // (unit stride in D: a token's row does not overlap the next)
  if (bias && (bias_sh < 0 || bias_sh % 4 != 0 || bias_st < T || bias_st % 4 != 0)) return DLMCQ_EINVAL;
  if (mask && (nW < 1 || B % nW != 0 || mask_sw < 0 || mask_sw % 4 != 0 || mask_st < T || mask_st % 4 != 0)) return DLMCQ_EINVAL;
  ep = ConvEpi{};
  int rc = emit_set_quantiser(ep, codes, q_scale, q_zero_point, q_lo, q_hi, q_form, q_ste_g, true);
  if (rc != DLMCQ_OK) return rc;
  if (B == 0 || H == 0) return DLMCQ_OK;
  rc = emit_check_pointers({q, k, v}, {bias, mask}, out, codes, 4);
  if (rc != DLMCQ_OK) return rc;
  constexpr int64_t LIM = 1ll << 31;
  if (B >= LIM || H >= LIM || B * H >= LIM - DLMCQ_WA_WAVES) return DLMCQ_ERANGE;
  a = WinAttnArgs{q, k, v, bias, mask, out, {strides[0], strides[1], strides[2]}, {strides[3], strides[4], strides[5]},
                  {strides[6], strides[7], strides[8]}, {strides[9], strides[10], strides[11]}, bias_sh, bias_st, mask_sw, mask_st,
                  (int)H, (int)T, (int)(mask ? nW : 1), (int)(B * H), scale};
  *grid = (B * H + DLMCQ_WA_WAVES - 1) / DLMCQ_WA_WAVES;
  return DLMCQ_OK;
}

}  // namespace dlmcq
