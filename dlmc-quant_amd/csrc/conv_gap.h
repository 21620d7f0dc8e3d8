// What the two global-average-pool kernels (gap.hip, conv_gap_i8.hip) share: the tail of the pooling arithmetic and the host-side
// reading of the quantiser arguments.  Not part of the ABI.
#pragma once

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

}  // namespace dlmcq
