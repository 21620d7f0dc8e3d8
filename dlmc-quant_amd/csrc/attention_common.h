// What the five attention kernels (attention.hip, attention_f16.hip, window_attention.hip, window_attention_f16.hip,
// window_attention_stream.hip) share: the kernel
// arguments, the host checks and the launch behind them, and the device steps that are the same code in more than one of them - the
// lane map, the operand loads, the f16 conversions and v's transposing pair stores, the f16 P step, the normalised store.  (The fp32
// P V step is NOT here: as a helper it left the window kernel's code as good but cost the streaming kernel 0.4 % at ViT-S's shape,
// twice the run-to-run spread - DESIGN.md 5.35 - so each fp32 kernel keeps its own copy.)  The arithmetic of every step is stated in
// the header comment of the kernel that uses it; here stands the code, once.  Five translation units, not one: their per-file flags
// differ (csrc/Makefile).  Not part of the ABI.
#pragma once

#include "conv_gap.h"

namespace dlmcq {

// A workgroup of a streaming kernel (attention.hip, attention_f16.hip) owns DLMCQ_AT_ROWS query rows of one (b, h)
#define DLMCQ_AT_WAVES 4
#define DLMCQ_AT_ROWS (32 * DLMCQ_AT_WAVES)      // query rows per workgroup
#define DLMCQ_AT_KB 32                           // keys per block
// A workgroup of a window kernel (window_attention.hip, window_attention_f16.hip) is DLMCQ_WA_WAVES waves, one (b, h) each
#define DLMCQ_WA_WAVES 4      // (b, h) pairs per workgroup
#define DLMCQ_WA_TMAX 64
// A workgroup of the streamed window kernel (window_attention_stream.hip) owns one (b, h) whole: ceil(T / 32) waves, a 32-query tile each
#define DLMCQ_WS_TMAX 256

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

struct AttnArgs {
  const float *q, *k, *v;
  float* out;
  int64_t qs[3], ks[3], vs[3], os[3];      // element strides (batch, head, token)
  int H, Tq, Tk, tiles;
  float scale;
};

struct WinAttnArgs {
  const float *q, *k, *v, *bias, *mask;
  float* out;
  int64_t qs[3], ks[3], vs[3], os[3];      // element strides (batch, head, token)
  int64_t bias_sh, bias_st, mask_sw, mask_st;
  int H, T, nW, pairs;
  float scale;
};

// ---- device: the lane map.  S^T = k q^T: a lane holds ONE query (lane & 31) and, of a 32-key block, the 16 keys acc_key(r, lane >> 5)
__device__ __forceinline__ constexpr int acc_key(int r, int half) { return (r & 3) + 8 * (r >> 2) + 4 * half; }

// keys past T - 1 hold s = -inf (a select, no branch); key0 = the block's first key + 4 half
__device__ __forceinline__ void mask_tail(f32x16& s, int key0, int T) {
#pragma unroll
  for (int r = 0; r < 16; ++r) s[r] = key0 + acc_key(r, 0) >= T ? -__builtin_inff() : s[r];
}

// max(m, the lane's 16 scores), registers in ascending order (v_max_f32: a NaN is dropped)
__device__ __forceinline__ float acc_max(float m, const f32x16& s) {
#pragma unroll
  for (int r = 0; r < 16; ++r) m = fmaxf(m, s[r]);
  return m;
}

// a query's value in the other lane half (lane ^ 32): the row maximum is fmaxf(m, other_half(m)), l is l + other_half(l)
__device__ __forceinline__ float other_half(float x) { return __shfl_xor(x, 32, 64); }

// s += the additive term's row `row` (this lane's query), keys key0 + 8 g .. + 3 in registers 4 g .. 4 g + 3: four 16-byte pieces
__device__ __forceinline__ void add_term(f32x16& s, const float* row, int key0, int T) {
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    const int j = key0 + 8 * g;
    const f32x4 t = *reinterpret_cast<const f32x4*>(row + (j < T ? j : 0));
    s[4 * g] += t.x, s[4 * g + 1] += t.y, s[4 * g + 2] += t.z, s[4 * g + 3] += t.w;
  }
}

// ---- device: operands.  fp32: row `row` of a [T, D] view as the operand of the 32x32x2 MFMA whose k steps walk D: element
// 2 s + half of the row in register s
template <int D>
__device__ __forceinline__ void load_operand_row(const float* base, int64_t row_stride, int row, int half, float (&r)[D / 2]) {
  const f32x4* p = reinterpret_cast<const f32x4*>(base + (int64_t)row * row_stride);
#pragma unroll
  for (int f = 0; f < D / 4; ++f) {
    const f32x4 t = p[f];
    r[2 * f] = half ? t.y : t.x;
    r[2 * f + 1] = half ? t.w : t.z;
  }
}

__device__ __forceinline__ f16x2 h2(float a, float b) { return __builtin_convertvector(f32x2{a, b}, f16x2); }      // RNE, packed
__device__ __forceinline__ f16x8 h8(const f32x4& a, const f32x4& b) {
  const f16x2 p0 = h2(a.x, a.y), p1 = h2(a.z, a.w), p2 = h2(b.x, b.y), p3 = h2(b.z, b.w);
  return f16x8{p0.x, p0.y, p1.x, p1.y, p2.x, p2.y, p3.x, p3.y};
}

// f16: h(row[16 s + 8 half .. + 7]), s = 0 .. QS - 1: this lane's operand of the 32x32x16 score MFMA
template <int QS>
__device__ __forceinline__ void load_operand_f16(const float* row, int half, f16x8 (&r)[QS]) {
  const f32x4* p = reinterpret_cast<const f32x4*>(row);
#pragma unroll
  for (int s = 0; s < QS; ++s) r[s] = h8(p[4 * s + 2 * half], p[4 * s + 2 * half + 1]);
}

// v^T is staged with the keys of a 32-block in the f16 P operand's order: key j stands at position j with bits 2 and 3 exchanged
__device__ __forceinline__ constexpr int swap23(int x) { return (x & ~12) | ((x & 4) << 1) | ((x & 8) >> 1); }

// the transposing write of that staging: 4 channels of the two keys at neighbouring positions pos, pos + 1 -> 4 packed pair stores
// into the channel rows r0 .. r3 (offsets in halves) of `lv`
__device__ __forceinline__ void store_v_pairs(_Float16* lv, int r0, int r1, int r2, int r3, int pos, const f32x4& v0, const f32x4& v1) {
  *reinterpret_cast<f16x2*>(&lv[r0 + pos]) = h2(v0.x, v1.x);
  *reinterpret_cast<f16x2*>(&lv[r1 + pos]) = h2(v0.y, v1.y);
  *reinterpret_cast<f16x2*>(&lv[r2 + pos]) = h2(v0.z, v1.z);
  *reinterpret_cast<f16x2*>(&lv[r3 + pos]) = h2(v0.w, v1.w);
}

// ---- device: the f16 P step of one 32-key block.  p = exp2(x) (v_exp_f32) of x = s - m~ where the scores are in base-2 units
// (FOLDED: the streaming kernel's scale holds log2 e), else of fl32(fl32(s - m~) * fl32(log2 e)) (the window kernel: natural units);
// P = h(p), packed in place into the two B operands of O^T = v^T P^T; returns t0 + t1, the two balanced trees over the fp32 values
// of the ROUNDED weights of registers 0 .. 7 and 8 .. 15
template <bool FOLDED>
__device__ __forceinline__ float p_step_f16(const f32x16& s, float mu, f16x8 (&ph)[2]) {
  const float L = 1.44269502162933349609375f;      // fl32(log2 e)
  float x[16];
#pragma unroll
  for (int r = 0; r < 16; r += 2) {
    const float a0 = FOLDED ? s[r] - mu : (s[r] - mu) * L, a1 = FOLDED ? s[r + 1] - mu : (s[r + 1] - mu) * L;
    const f16x2 p = h2(__builtin_amdgcn_exp2f(a0), __builtin_amdgcn_exp2f(a1));
    ph[r >> 3][r & 7] = p.x;
    ph[r >> 3][(r & 7) + 1] = p.y;
    x[r] = (float)p.x;
    x[r + 1] = (float)p.y;
  }
  const float t0 = ((x[0] + x[1]) + (x[2] + x[3])) + ((x[4] + x[5]) + (x[6] + x[7]));
  const float t1 = ((x[8] + x[9]) + (x[10] + x[11])) + ((x[12] + x[13]) + (x[14] + x[15]));
  return t0 + t1;
}

// ---- device: the normalised store of CB channel blocks of one query: out = o / l (a true division) as fp32 and / or the consumer's
// codes, 4 consecutive channels per register quad, at element offset `at` (channel 0 of the first block) of either output
template <int CB>
__device__ __forceinline__ void store_normalised(const f32x16* o, float l, float* out, const ConvEpi& ep, const EpiQuant& eq,
                                                 int64_t at, int half) {
#pragma unroll
  for (int cb = 0; cb < CB; ++cb) {
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const f32x4 v = f32x4{o[cb][4 * g] / l, o[cb][4 * g + 1] / l, o[cb][4 * g + 2] / l, o[cb][4 * g + 3] / l};
      const int64_t e = at + cb * 32 + 8 * g + 4 * half;
      if (out) *reinterpret_cast<f32x4*>(out + e) = v;
      if (ep.codes) *reinterpret_cast<uint32_t*>(ep.codes + e) = eq.code4(v);
    }
  }
}

// ---- host.  The checks the four entry points share, in the order that decides which code a call with two faults gets: geometry
// (`own_geometry`: the caller's sizes and term layout; here B, H, D, the scale, the twelve strides), emit_set_quantiser (plain codes
// only: the reader is a Linear layer), an empty problem (`own_empty`, or B or H zero: DLMCQ_OK, *launch stays false), emit_check_pointers,
// the 2^31 limits of B and H (the caller's own limits follow).  Else `ep` is set and *launch is true.
static inline int attention_checks(ConvEpi& ep, bool* launch, bool own_geometry, bool own_empty, const float* q, const float* k,
                                   const float* v, const float* bias, const float* mask, const float* out, void* codes, int64_t B, int64_t H,
                                   int64_t D, const int64_t (&strides)[12], float scale, const float* q_scale, const float* q_zero_point,
                                   int32_t q_lo, int32_t q_hi, int32_t q_form, float q_ste_g) {
  *launch = false;
  if (!own_geometry || B < 0 || H < 0 || (D != 32 && D != 64) || !(scale == scale) || !(scale > -3.402823466e+38f && scale < 3.402823466e+38f))
    return DLMCQ_EINVAL;
  for (int i = 0; i < 12; ++i)
    if (strides[i] < 0 || strides[i] % 4 != 0) return DLMCQ_EINVAL;
  for (int i = 2; i < 12; i += 3)
    if (strides[i] < D) return DLMCQ_EINVAL;      // (unit stride in D: a token's row does not overlap the next)
  ep = ConvEpi{};
  int rc = emit_set_quantiser(ep, codes, q_scale, q_zero_point, q_lo, q_hi, q_form, q_ste_g, true);
  if (rc != DLMCQ_OK) return rc;
  if (own_empty || B == 0 || H == 0) return DLMCQ_OK;
  rc = emit_check_pointers({q, k, v}, {bias, mask}, out, codes, 4);
  if (rc != DLMCQ_OK) return rc;
  constexpr int64_t LIM = 1ll << 31;
  if (B >= LIM || H >= LIM || B * H >= LIM) return DLMCQ_ERANGE;
  *launch = true;
  return DLMCQ_OK;
}

// The streaming entry points' checks (attention_checks; Tq >= 0, Tk >= 1; Tq = 0 is empty).  DLMCQ_OK with *grid = 0: nothing to
// launch.  Else `a`, `ep` and *grid (workgroups) are set.
static inline int attention_args(AttnArgs& a, ConvEpi& ep, int64_t* grid, const float* q, const float* k, const float* v, float* out,
                                 void* codes, int64_t B, int64_t H, int64_t Tq, int64_t Tk, int64_t D, const int64_t (&strides)[12],
                                 float scale, const float* q_scale, const float* q_zero_point, int32_t q_lo, int32_t q_hi, int32_t q_form,
                                 float q_ste_g) {
  *grid = 0;
  bool launch;
  const int rc = attention_checks(ep, &launch, Tq >= 0 && Tk >= 1, Tq == 0, q, k, v, nullptr, nullptr, out, codes, B, H, D, strides, scale,
                                  q_scale, q_zero_point, q_lo, q_hi, q_form, q_ste_g);
  if (!launch) return rc;
  constexpr int64_t LIM = 1ll << 31;
  const int64_t tiles = (Tq + DLMCQ_AT_ROWS - 1) / DLMCQ_AT_ROWS;
  if (Tq >= LIM || Tk >= LIM || B * H * tiles >= LIM) return DLMCQ_ERANGE;
  a = AttnArgs{q, k, v, out, {strides[0], strides[1], strides[2]}, {strides[3], strides[4], strides[5]}, {strides[6], strides[7], strides[8]},
               {strides[9], strides[10], strides[11]}, (int)H, (int)Tq, (int)Tk, (int)tiles, scale};
  *grid = B * H * tiles;
  return DLMCQ_OK;
}

// The window entry points' checks (attention_checks; 1 <= T <= `tmax` - DLMCQ_WA_TMAX for the one-wave kernels, DLMCQ_WS_TMAX for the
// streamed one - and the additive terms' layout).  DLMCQ_OK with *grid = 0: nothing to launch.  Else `a`, `ep` and *grid (workgroups
// of DLMCQ_WA_WAVES pairs; the streamed kernel launches a.pairs instead) are set.
static inline int window_attention_args(WinAttnArgs& a, ConvEpi& ep, int64_t* grid, const float* q, const float* k, const float* v,
                                        const float* bias, const float* mask, float* out, void* codes, int64_t B, int64_t H, int64_t T,
                                        int64_t D, int64_t nW, const int64_t (&strides)[12], int64_t bias_sh, int64_t bias_st,
                                        int64_t mask_sw, int64_t mask_st, float scale, const float* q_scale, const float* q_zero_point,
                                        int32_t q_lo, int32_t q_hi, int32_t q_form, float q_ste_g, int64_t tmax = DLMCQ_WA_TMAX) {
  *grid = 0;
  const bool bias_ok = !bias || (bias_sh >= 0 && bias_sh % 4 == 0 && bias_st >= T && bias_st % 4 == 0);
  const bool mask_ok = !mask || (nW >= 1 && B % nW == 0 && mask_sw >= 0 && mask_sw % 4 == 0 && mask_st >= T && mask_st % 4 == 0);
  bool launch;
  const int rc = attention_checks(ep, &launch, T >= 1 && T <= tmax && bias_ok && mask_ok, false, q, k, v, bias, mask, out, codes, B, H, D,
                                  strides, scale, q_scale, q_zero_point, q_lo, q_hi, q_form, q_ste_g);
  if (!launch) return rc;
  if (B * H >= (1ll << 31) - DLMCQ_WA_WAVES) return DLMCQ_ERANGE;
  a = WinAttnArgs{q, k, v, bias, mask, out, {strides[0], strides[1], strides[2]}, {strides[3], strides[4], strides[5]},
                  {strides[6], strides[7], strides[8]}, {strides[9], strides[10], strides[11]}, bias_sh, bias_st, mask_sw, mask_st,
                  (int)H, (int)T, (int)(mask ? nW : 1), (int)(B * H), scale};
  *grid = (B * H + DLMCQ_WA_WAVES - 1) / DLMCQ_WA_WAVES;
  return DLMCQ_OK;
}

// The launch behind the checks: `blocks` workgroups of `threads` of the D = 64 or the D = 32 instantiation
template <class Args>
static inline int attention_launch(void (*kernel64)(Args, ConvEpi), void (*kernel32)(Args, ConvEpi), const Args& a, const ConvEpi& ep,
                                   int64_t blocks, int threads, int64_t D, dlmcq_stream_t stream) {
  hipLaunchKernelGGL(D == 64 ? kernel64 : kernel32, dim3((uint32_t)blocks), dim3(threads), 0, reinterpret_cast<hipStream_t>(stream), a, ep);
  return launch_status();
}

}  // namespace dlmcq
