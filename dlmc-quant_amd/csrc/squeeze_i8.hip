// The squeeze path of a squeeze-excite block from the pooled activation codes [N, C] (the rows dlmcq_gap_nhwc_f32 writes) to the fp32
// gate [N, C]: two small int8 layers with an activation between them and the gate function behind them, ONE launch, the hidden vector
// never leaving the chip.  The arithmetic, once (include/dlmcq.h restates it):
//     S1 = SUM_c (q[n, c] - zp1) * w1[r, c]            exact in int32 (v_dot4_i32_i8 on re-centred bytes + (shift - zp1) * wsum1[r])
//     h  = fma(fl32(S1), fl32(s_in1 * s_w1[r]), b1[r])  dequant1: the one rounding chain of dlmcq_conv2d_i8_nhwc_fused
//     h  = inner_act(h)                                 none | relu_nan (v < 0 ? 0 : v) | swish.hip's e = expf(-h), d = 1 + e, s = 1 / d, h * s
//     qh = the hidden quantiser's code of h             EpiQuant::code4 (q_scale .. q_ste_g)
//     S2 = SUM_r (qh[n, r] - zp2) * w2[c, r]            exact in int32; zp2 = the quantiser's zero point
//     v  = fma(fl32(S2), fl32(s_h * s_w2[c]), b2[c])    s_h = the quantiser's dequantising scale (QBASE: grad_scale(s, g), else s)
//     g  = gate_fn(v)                                   none | e = expf(-v), d = 1 + e, g = 1 / d | t = v + 3, relu6 as the device has it,
//                                                       g = t * fl32(1 / 6) (how the device divides by the host scalar 6)
// - each step rounded to fp32 by itself under the library's flags (-ffp-contract=off, accurate expf, the correctly rounded division).
// One workgroup per SQ_IMGS images: their code rows are staged in LDS (re-centred to signed bytes); layer 1 gives every hidden unit to
// SQ_LANES lanes, which walk the weight row once in 16-byte pieces (4-byte ones where C % 16 != 0), multiply it with all images' rows and
// add up over the lanes in a fixed order (integers: any order gives the same sum); the hidden values go to LDS, are quantised four at a
// time, and layer 2 runs one output channel per thread over the hidden codes in LDS.  No atomics, no scratch; the result depends
// neither on the launch geometry nor on the run.
#include "conv_gap.h"

namespace dlmcq {

constexpr int SQ_IMGS = DLMCQ_SQUEEZE_IMAGES;      // images per workgroup (include/dlmcq.h)
constexpr int SQ_LANES = 16;                       // lanes per hidden unit in layer 1
static_assert(SQ_IMGS == 4, "the layer-1 epilogue picks an image's sum by lane (lane < SQ_IMGS <= SQ_LANES) with four selects");

struct SqueezeArgs {
  const uint32_t* x;
  const int8_t* w1;
  const int32_t* wsum1;
  const float* bias1;
  const float* s_in1;
  const float* zp1;
  const float* s_w1;
  const int8_t* w2;
  const int32_t* wsum2;
  const float* bias2;
  const float* s_w2;
  float* gate;
  float* hidden;
  int N, C, R4;
  int x_shift;       // 128: unsigned input codes, re-centred with xor 0x80
  int inner_act, gate_fn;
};

// torch.relu / F.relu6 on the device (ATen's clamp kernels; csrc/gate.hip has the same function)
__device__ __forceinline__ float sq_relu_device(float v) { return v > 0.0f ? v : (v != v ? v : 0.0f); }

// swish.hip's first three steps
__device__ __forceinline__ float sq_sigmoid(float v) {
  const float d = 1.0f + expf(-v);
  return 1.0f / d;
}

__device__ __forceinline__ float sq_inner(float v, int act) {
  if (act == DLMCQ_SQUEEZE_RELU) return relu_nan(v);
  if (act == DLMCQ_SQUEEZE_SWISH) return v * sq_sigmoid(v);
  return v;
}

__device__ __forceinline__ float sq_gate(float v, int fn) {
  if (fn == DLMCQ_GATE_SIGMOID) return sq_sigmoid(v);
  if (fn == DLMCQ_GATE_HARDSIGMOID) {
    const float t = cap6_nan(sq_relu_device(v + 3.0f));
    return t * (1.0f / 6.0f);
  }
  return v;
}

// SUM over the bytes of one piece (V: 16 bytes, else 4) of signed weights x signed codes, for all SQ_IMGS rows (`rows` in LDS, `stride`
// bytes apart, the piece at byte `at`)
template <bool V>
__device__ __forceinline__ void sq_dot(const int8_t* __restrict__ w, const uint8_t* rows, int stride, int at, int (&acc)[SQ_IMGS]) {
  if constexpr (V) {
    const i32x4 ww = *reinterpret_cast<const i32x4*>(w + at);
#pragma unroll
    for (int i = 0; i < SQ_IMGS; ++i) {
      const i32x4 xx = *reinterpret_cast<const i32x4*>(rows + i * stride + at);
      acc[i] = __builtin_amdgcn_sdot4(xx.x, ww.x, acc[i], false);
      acc[i] = __builtin_amdgcn_sdot4(xx.y, ww.y, acc[i], false);
      acc[i] = __builtin_amdgcn_sdot4(xx.z, ww.z, acc[i], false);
      acc[i] = __builtin_amdgcn_sdot4(xx.w, ww.w, acc[i], false);
    }
  } else {
    const int ww = *reinterpret_cast<const int*>(w + at);
#pragma unroll
    for (int i = 0; i < SQ_IMGS; ++i)
      acc[i] = __builtin_amdgcn_sdot4(*reinterpret_cast<const int*>(rows + i * stride + at), ww, acc[i], false);
  }
}

// V1 / V2: layer 1's / layer 2's rows are read in 16-byte pieces (C % 16 == 0 / R4 % 16 == 0)
template <bool V1, bool V2>
__global__ __launch_bounds__(DLMCQ_BLOCK) void squeeze_gate_kernel(SqueezeArgs a, ConvEpi ep) {
  extern __shared__ __attribute__((aligned(16))) uint8_t sq_lds[];
  const int C = a.C, R4 = a.R4;
  uint8_t* xs = sq_lds;                                             // [SQ_IMGS][C] signed code bytes
  float* hf = reinterpret_cast<float*>(sq_lds + SQ_IMGS * C);       // [SQ_IMGS][R4] hidden values
  uint8_t* hc = reinterpret_cast<uint8_t*>(hf + SQ_IMGS * R4);      // [SQ_IMGS][R4] signed hidden code bytes
  const int tid = threadIdx.x;
  const int64_t n0 = (int64_t)blockIdx.x * SQ_IMGS;
  const int ni = a.N - n0 < SQ_IMGS ? (int)(a.N - n0) : SQ_IMGS;    // images of this workgroup; the other rows hold zeros

  // ---- the group's code rows -> LDS, re-centred
  {
    const uint32_t xw = a.x_shift ? 0x80808080u : 0u;
    const int words = SQ_IMGS * C / 4, real = ni * (C / 4);
    const uint32_t* src = a.x + n0 * (C / 4);
    for (int i = tid; i < words; i += DLMCQ_BLOCK) reinterpret_cast<uint32_t*>(xs)[i] = i < real ? (src[i] ^ xw) : 0u;
  }
  __syncthreads();

  // ---- layer 1: hidden unit r on the SQ_LANES lanes of one group
  {
    const int group = tid / SQ_LANES, lane = tid % SQ_LANES;
    const int zpi = a.zp1 ? (int)__builtin_rintf(a.zp1[0]) : 0;
    const float sin = a.s_in1[0];
    constexpr int PB = V1 ? 16 : 4;
    for (int r = group; r < R4; r += DLMCQ_BLOCK / SQ_LANES) {
      int acc[SQ_IMGS] = {};
      const int8_t* row = a.w1 + (int64_t)r * C;
      for (int at = lane * PB; at < C; at += SQ_LANES * PB) sq_dot<V1>(row, xs, C, at, acc);
#pragma unroll
      for (int off = SQ_LANES / 2; off; off >>= 1) {
#pragma unroll
        for (int i = 0; i < SQ_IMGS; ++i) acc[i] += __shfl_xor(acc[i], off, SQ_LANES);
      }
      if (lane < SQ_IMGS) {
        const int s = lane == 0 ? acc[0] : (lane == 1 ? acc[1] : (lane == 2 ? acc[2] : acc[3]));
        const float v = dequant1(s + (a.x_shift - zpi) * a.wsum1[r], sin * a.s_w1[r], a.bias1 ? a.bias1[r] : 0.0f);
        hf[lane * R4 + r] = sq_inner(v, a.inner_act);
      }
    }
  }
  __syncthreads();

  // ---- the hidden values: fp32 out (optional), codes -> LDS as signed bytes
  const EpiQuant eq(ep);
  const bool h_unsigned = ep.q_lo >= 0.0f;
  {
    const uint32_t hx = h_unsigned ? 0x80808080u : 0u;
    const int quads = SQ_IMGS * R4 / 4, real = ni * (R4 / 4);
    f32x4* dst = a.hidden ? reinterpret_cast<f32x4*>(a.hidden) + n0 * (R4 / 4) : nullptr;
    for (int i = tid; i < quads; i += DLMCQ_BLOCK) {
      const f32x4 v = reinterpret_cast<const f32x4*>(hf)[i];
      reinterpret_cast<uint32_t*>(hc)[i] = eq.code4(v) ^ hx;
      if (dst && i < real) dst[i] = v;
    }
  }
  if (!a.gate) return;
  __syncthreads();

  // ---- layer 2 and the gate function: one output channel per thread
  {
    const float sq = ep.q_scale[0];
    const float sh = ep.q_form == DLMCQ_FORM_QBASE ? ste_scale(sq, ep.q_g) : sq;
    const int zpi = ep.q_zp ? (int)__builtin_rintf(ep.q_zp[0]) : 0;
    const int shift = h_unsigned ? 128 : 0;
    constexpr int PB = V2 ? 16 : 4;
    for (int c = tid; c < C; c += DLMCQ_BLOCK) {
      int acc[SQ_IMGS] = {};
      const int8_t* row = a.w2 + (int64_t)c * R4;
      for (int at = 0; at < R4; at += PB) sq_dot<V2>(row, hc, R4, at, acc);
      const int corr = (shift - zpi) * a.wsum2[c];
      const float mult = sh * a.s_w2[c], b = a.bias2 ? a.bias2[c] : 0.0f;
#pragma unroll
      for (int i = 0; i < SQ_IMGS; ++i)
        if (i < ni) a.gate[(n0 + i) * C + c] = sq_gate(dequant1(acc[i] + corr, mult, b), a.gate_fn);
    }
  }
}

}  // namespace dlmcq

using namespace dlmcq;

extern "C" int dlmcq_squeeze_gate_i8(const void* x, const int8_t* w1, const int32_t* wsum1, const float* bias1, const float* in_scale1,
                                     const float* in_zero_point1, const float* w_scale1, int32_t inner_act, const int8_t* w2,
                                     const int32_t* wsum2, const float* bias2, const float* w_scale2, int32_t gate_fn, float* gate,
                                     float* hidden, int64_t N, int64_t C, int64_t R4, int32_t x_is_unsigned, const float* q_scale,
                                     const float* q_zero_point, int32_t q_lo, int32_t q_hi, int32_t q_form, float q_ste_g,
                                     dlmcq_stream_t stream) {
  if (N < 0 || C < 4 || C > DLMCQ_SQUEEZE_MAX_C || C % 4 != 0 || R4 < 1 || R4 > DLMCQ_SQUEEZE_MAX_R || R4 % 4 != 0) return DLMCQ_EINVAL;
  if (inner_act < DLMCQ_SQUEEZE_NONE || inner_act > DLMCQ_SQUEEZE_SWISH || gate_fn < DLMCQ_GATE_NONE || gate_fn > DLMCQ_GATE_HARDSIGMOID)
    return DLMCQ_EINVAL;
  ConvEpi ep{};
  // (the hidden codes stay in LDS: `ep.codes` is the "there is a quantiser" mark EpiQuant and the checks key on, never dereferenced)
  int rc = emit_set_quantiser(ep, &ep, q_scale, q_zero_point, q_lo, q_hi, q_form, q_ste_g, true);
  if (rc != DLMCQ_OK) return rc;
  // (layer 2 re-reads the hidden bytes as uint8 or as int8: a range that is neither has no byte for its codes above 127)
  if (q_lo < 0 && q_hi > 127) return DLMCQ_EINVAL;
  if (N == 0) return DLMCQ_OK;
  if (!(gate || hidden)) return DLMCQ_EINVAL;
  for (const void* p : {x, (const void*)w1, (const void*)wsum1, (const void*)in_scale1, (const void*)w_scale1, (const void*)w2,
                        (const void*)wsum2, (const void*)w_scale2})
    if (!p) return DLMCQ_EINVAL;
  if (!aligned16(w1) || !aligned16(w2) || !aligned16(gate) || !aligned16(hidden)) return DLMCQ_EALIGN;
  for (const void* p : {x, (const void*)wsum1, (const void*)bias1, (const void*)in_scale1, (const void*)in_zero_point1, (const void*)w_scale1,
                        (const void*)wsum2, (const void*)bias2, (const void*)w_scale2, (const void*)q_scale, (const void*)q_zero_point})
    if (!aligned4(p)) return DLMCQ_EALIGN;
  if (N * C >= (1ll << 31) || N * R4 >= (1ll << 31)) return DLMCQ_ERANGE;
  SqueezeArgs a{static_cast<const uint32_t*>(x), w1, wsum1, bias1, in_scale1, in_zero_point1, w_scale1, w2, wsum2, bias2, w_scale2, gate, hidden,
                (int)N, (int)C, (int)R4, x_is_unsigned ? 128 : 0, inner_act, gate_fn};
  const dim3 grid((uint32_t)((N + SQ_IMGS - 1) / SQ_IMGS)), block(DLMCQ_BLOCK);
  const size_t lds = (size_t)SQ_IMGS * (C + 5 * R4);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const bool v1 = C % 16 == 0, v2 = R4 % 16 == 0;
  if (v1 && v2) hipLaunchKernelGGL((squeeze_gate_kernel<true, true>), grid, block, lds, st, a, ep);
  else if (v1) hipLaunchKernelGGL((squeeze_gate_kernel<true, false>), grid, block, lds, st, a, ep);
  else if (v2) hipLaunchKernelGGL((squeeze_gate_kernel<false, true>), grid, block, lds, st, a, ep);
  else hipLaunchKernelGGL((squeeze_gate_kernel<false, false>), grid, block, lds, st, a, ep);
  return launch_status();
}
