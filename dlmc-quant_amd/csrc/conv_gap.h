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

}  // namespace dlmcq
