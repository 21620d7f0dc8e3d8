// Scaled dot-product attention softmax(scale q k^T) v of fp32 [B, H, T, D] views, D in {32, 64}, to fp32 and / or the activation codes of
// the projection that reads the merged heads, as ONE flash forward: q, k and v are read once, nothing of size Tq x Tk touches memory,
// and the projection's quantise pass is the kernel's store.  No mask, no causal flag, no dropout.  The arithmetic, once, for query row
// i of one (b, h), keys j = 0 .. Tk - 1 taken in blocks of 32 (the online softmax's key block), u = 2^-24:
//     a_ij = fmaf(q_i[D-1], k_j[D-1], ... fmaf(q_i[1], k_j[1], fmaf(q_i[0], k_j[0], +0)))   the k-ordered chain of v_mfma_f32_32x32x2_f32
//     s_ij = fl32(a_ij * scale)                                                              one IEEE multiply
//     per key block b, with m the running maximum (-inf before the first block) and the block's keys past Tk - 1 holding s = -inf:
//     m'   = max(m, max_j s_ij)            v_max_f32, which drops NaNs: a NaN score never becomes the maximum (it reaches p, below)
//     m~   = m', or 0 where m' = -inf      (a row that has met only -inf scores so far: no inf - inf)
//     al   = expf(fl32(m - m~))            the device library's accurate expf (1 ulp), not v_exp_f32; 0 in the first block
//     p_ij = expf(fl32(s_ij - m~))
//     l_h  = fl32(fl32(l_h * al) + t_h)    per half h of the block's keys (keys with bit 2 clear / set: the two lane halves), t_h the
//                                          half's 16 p_ij added one by one from p of the lowest key, in ascending key order
//     w_g  = the fmaf chain fmaf(v_j[c], p_ij, w_g) from +0 over the 8 keys 8 g .. 8 g + 7 of the block (g = 0 .. 3) in the order
//            0 4 1 5 2 6 3 7  (+ 8 g + 32 b: the accumulator rows of the 32x32 MFMA tile as its k steps)
//     o_ic = fl32(fl32(o_ic * al) + fl32(fl32(w_0 + w_1) + fl32(w_2 + w_3)))      chains of 8 and a tree, not one chain over the keys:
//            a chain over alike summands drifts (q = 0, constant v: 4 ulp after 32 keys, 31 ulp after 257; this order: at most 2)
//     after the last block: l = fl32(l_0 + l_1), out_ic = fl32(o_ic / l) - a true division, correctly rounded, not a multiply by 1 / l
//     code = the consumer's quantiser of out_ic (EpiQuant::code4, plain codes)
// - each step rounded to fp32 by itself under the library's flags.  S^T = k q^T is what the MFMA computes (A = k, B = q^T), so a lane
// holds ONE query (lane & 31) and 16 of the block's 32 keys in its accumulator registers (rows (r & 3) + 8 (r >> 2) + 4 (lane >> 5));
// the row maximum is 15 v_max and one exchange with lane ^ 32, and P^T register r is, as it stands, the B operand of k step r of
// O^T = v^T P^T - no lane movement, no LDS for P.  O^T has the query on the lane and 4 consecutive channels per register quad: one
// 16-byte store (4 codes) per quad.
// Non-finite inputs: the NaNs of torch's unfused graph, element for element.  A NaN in q_i makes row i NaN (and no other: a query lives
// in its own two lanes); a NaN in any k_j makes s_ij, hence p_ij and l, NaN for every i of the head; a +inf score gives m~ = +inf,
// p = expf(inf - inf) = NaN: the row is NaN; a NaN in v_j[c] makes column c of every row of the head NaN (0 * NaN = NaN in the fmaf
// chain, as in torch's matmul) and leaves the other columns finite.  Rows past Tk / Tq are never read: the last valid row is read again
// and replaced by +0 (k, v) or not stored (q), under selects, not branches.
// Error bound against real arithmetic on the same fp32 inputs (s*, p*, o* real; delta_i = (D + 1) u scale max_j sum_k |q_ik k_jk|):
//     |o_ic - o*_ic| <= (2 delta_i + kappa u) sum_j p*_ij |v_jc| + 2^-126 max_j |v_jc|,   kappa = 2 (104 + 2 + 3 nb + 32 nb) + 1,
// nb = ceil(Tk / 32).  delta_i bounds a score's error (D roundings of the chain, one of the multiply); scores enter only through
// differences, hence 2 delta_i.  Per term of the numerator and of l: the subtractions s - m~ and m - m~ round their results, in total
// (telescoped over the blocks: m only rises) at most u (m_final - s_ij), and a term with m_final - s_ij > 104 is 0 in fp32 and below
// 2^-149 in real arithmetic (the last summand: an output that small is not resolved) - 104; expf 1 ulp = 2 u; per later block one ulp
// of al and one multiply, 3 u; the sum of l at most one rounding per key, 32 nb (the chains, the tree and the block adds of o: fewer);
// twice, for numerator and denominator; one division.  Measured ratios: DESIGN.md 5.24.
// One workgroup of 4 waves owns 128 query rows of one (b, h), a wave 32 of them (q in D / 2 registers); k and v stream through LDS in
// key blocks of 32 rows (17.3 KiB at D = 64, rows padded by 2 and 8 floats against bank conflicts).  A wave whose 32 rows lie past Tq
// only loads; which wave that is rotates with the head index, so the idle waves spread over the SIMDs.  No atomics, no scratch: a
// row's result depends neither on B, H, its (b, h) nor on the launch.
#include "conv_gap.h"

namespace dlmcq {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x2 __attribute__((ext_vector_type(2)));

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

template <int D>
__global__ __launch_bounds__(64 * DLMCQ_AT_WAVES) void attention_kernel(AttnArgs a, ConvEpi ep) {
  constexpr int KS = D + 2, VS = D + 8, D4 = D / 4, CB = D / 32;
  constexpr int THREADS = 64 * DLMCQ_AT_WAVES;
  __shared__ __attribute__((aligned(16))) float lds_k[DLMCQ_AT_KB * KS];
  __shared__ __attribute__((aligned(16))) float lds_v[DLMCQ_AT_KB * VS];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, col = lane & 31, half = lane >> 5;
  const int bh = (int)(blockIdx.x / (uint32_t)a.tiles), tile = (int)(blockIdx.x % (uint32_t)a.tiles);
  const int b = bh / a.H, h = bh % a.H;
  const int q0 = tile * DLMCQ_AT_ROWS + ((wave + bh) & (DLMCQ_AT_WAVES - 1)) * 32;
  const bool active = q0 < a.Tq;      // (wave-uniform)
  const int qi = q0 + col;
  const float* kb_ = a.k + b * a.ks[0] + h * a.ks[1];
  const float* vb_ = a.v + b * a.vs[0] + h * a.vs[1];

  float qr[D / 2];      // q_i[2 s + half]: the B operand of k step s
  if (active) {
    const f32x4* qp = reinterpret_cast<const f32x4*>(a.q + b * a.qs[0] + h * a.qs[1] + (int64_t)(qi < a.Tq ? qi : a.Tq - 1) * a.qs[2]);
#pragma unroll
    for (int f = 0; f < D4; ++f) {
      const f32x4 t = qp[f];
      qr[2 * f] = half ? t.y : t.x;
      qr[2 * f + 1] = half ? t.w : t.z;
    }
  }
  f32x16 o[CB];
#pragma unroll
  for (int cb = 0; cb < CB; ++cb)
#pragma unroll
    for (int r = 0; r < 16; ++r) o[cb][r] = 0.0f;
  float m = -__builtin_inff(), l = 0.0f;
  const int nkb = (a.Tk + DLMCQ_AT_KB - 1) / DLMCQ_AT_KB;
  for (int kb = 0; kb < nkb; ++kb) {
    __syncthreads();      // (the previous block has been read)
#pragma unroll
    for (int it = 0; it < DLMCQ_AT_KB * D4 / THREADS; ++it) {
      const int idx = tid + it * THREADS, row = idx / D4, c4 = idx % D4;
      const int key = kb * DLMCQ_AT_KB + row;
      const bool in = key < a.Tk;
      const int64_t kr = in ? key : a.Tk - 1;
      f32x4 kk = *reinterpret_cast<const f32x4*>(kb_ + kr * a.ks[2] + c4 * 4);
      f32x4 vv = *reinterpret_cast<const f32x4*>(vb_ + kr * a.vs[2] + c4 * 4);
      if (!in) kk = f32x4{0.0f, 0.0f, 0.0f, 0.0f}, vv = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
      *reinterpret_cast<f32x2*>(&lds_k[row * KS + c4 * 4]) = f32x2{kk.x, kk.y};
      *reinterpret_cast<f32x2*>(&lds_k[row * KS + c4 * 4 + 2]) = f32x2{kk.z, kk.w};
      *reinterpret_cast<f32x4*>(&lds_v[row * VS + c4 * 4]) = vv;
    }
    __syncthreads();
    if (!active) continue;      // (wave-uniform; the barriers are above)
    f32x16 s;
#pragma unroll
    for (int r = 0; r < 16; ++r) s[r] = 0.0f;
#pragma unroll
    for (int st = 0; st < D / 2; ++st) s = __builtin_amdgcn_mfma_f32_32x32x2f32(lds_k[col * KS + 2 * st + half], qr[st], s, 0, 0, 0);
    const int key0 = kb * DLMCQ_AT_KB + 4 * half;
    float bm = -__builtin_inff();
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      float t = s[r] * a.scale;
      if (key0 + (r & 3) + 8 * (r >> 2) >= a.Tk) t = -__builtin_inff();
      s[r] = t;
      bm = fmaxf(bm, t);
    }
    bm = fmaxf(bm, __shfl_xor(bm, 32, 64));
    const float mn = fmaxf(m, bm);
    const float mu = mn == -__builtin_inff() ? 0.0f : mn;
    const float al = expf(m - mu);
    m = mn;
    float t = 0.0f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      s[r] = expf(s[r] - mu);
      t = r ? t + s[r] : s[r];
    }
    l = l * al + t;
#pragma unroll
    for (int cb = 0; cb < CB; ++cb) {
      // four independent chains of 8 keys (keys 8 g .. 8 g + 7: 4 MFMAs each), every one from +0, added as a tree: one chain over
      // the block's 32 keys - let alone over all keys - drifts when the summands are alike (32 equal p v: 4 ulp; 257: 31 ulp)
      f32x16 t4[4];
#pragma unroll
      for (int g = 0; g < 4; ++g) {
#pragma unroll
        for (int r = 0; r < 16; ++r) t4[g][r] = 0.0f;
      }
#pragma unroll
      for (int rr = 0; rr < 4; ++rr) {
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const int r = 4 * g + rr, krow = (r & 3) + 8 * (r >> 2) + 4 * half;
          t4[g] = __builtin_amdgcn_mfma_f32_32x32x2f32(lds_v[krow * VS + cb * 32 + col], s[r], t4[g], 0, 0, 0);
        }
      }
#pragma unroll
      for (int r = 0; r < 16; ++r) o[cb][r] = o[cb][r] * al + ((t4[0][r] + t4[1][r]) + (t4[2][r] + t4[3][r]));
      __builtin_amdgcn_sched_barrier(0);      // (one channel block's four accumulators at a time: 64 registers, not 128)
    }
  }
  if (!active) return;
  l = l + __shfl_xor(l, 32, 64);
  if (qi >= a.Tq) return;
  const int64_t at = b * a.os[0] + h * a.os[1] + (int64_t)qi * a.os[2];
  const EpiQuant eq(ep);
#pragma unroll
  for (int cb = 0; cb < CB; ++cb) {
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const f32x4 v = f32x4{o[cb][4 * g] / l, o[cb][4 * g + 1] / l, o[cb][4 * g + 2] / l, o[cb][4 * g + 3] / l};
      const int64_t e = at + cb * 32 + 8 * g + 4 * half;
      if (a.out) *reinterpret_cast<f32x4*>(a.out + e) = v;
      if (ep.codes) *reinterpret_cast<uint32_t*>(ep.codes + e) = eq.code4(v);
    }
  }
}

}  // namespace dlmcq

using namespace dlmcq;

// The checks: geometry (sizes, D, strides, scale), emit_set_quantiser (csrc/conv_gap.h; plain codes only: the reader is a Linear
// layer), an empty problem, emit_check_pointers, the 2^31 limits.
extern "C" int dlmcq_attention_f32(const float* q, const float* k, const float* v, float* out, void* codes, int64_t B, int64_t H, int64_t Tq,
                                   int64_t Tk, int64_t D, int64_t q_sb, int64_t q_sh, int64_t q_st, int64_t k_sb, int64_t k_sh, int64_t k_st,
                                   int64_t v_sb, int64_t v_sh, int64_t v_st, int64_t o_sb, int64_t o_sh, int64_t o_st, float scale,
                                   const float* q_scale, const float* q_zero_point, int32_t q_lo, int32_t q_hi, int32_t q_form, float q_ste_g,
                                   dlmcq_stream_t stream) {
  if (B < 0 || H < 0 || Tq < 0 || Tk < 1 || (D != 32 && D != 64) || !(scale == scale) || !(scale > -3.402823466e+38f && scale < 3.402823466e+38f))
    return DLMCQ_EINVAL;
  const int64_t strides[12] = {q_sb, q_sh, q_st, k_sb, k_sh, k_st, v_sb, v_sh, v_st, o_sb, o_sh, o_st};
  for (int i = 0; i < 12; ++i)
    if (strides[i] < 0 || strides[i] % 4 != 0) return DLMCQ_EINVAL;
  if (q_st < D || k_st < D || v_st < D || o_st < D) return DLMCQ_EINVAL;      // (unit stride in D: a token's row does not overlap the next)
  ConvEpi ep{};
  int rc = emit_set_quantiser(ep, codes, q_scale, q_zero_point, q_lo, q_hi, q_form, q_ste_g, true);
  if (rc != DLMCQ_OK) return rc;
  if (B == 0 || H == 0 || Tq == 0) return DLMCQ_OK;
  rc = emit_check_pointers({q, k, v}, {}, out, codes, 4);
  if (rc != DLMCQ_OK) return rc;
  constexpr int64_t LIM = 1ll << 31;
  const int64_t tiles = (Tq + DLMCQ_AT_ROWS - 1) / DLMCQ_AT_ROWS;
  if (B >= LIM || H >= LIM || Tq >= LIM || Tk >= LIM || B * H >= LIM || B * H * tiles >= LIM) return DLMCQ_ERANGE;
  AttnArgs a{q, k, v, out, {q_sb, q_sh, q_st}, {k_sb, k_sh, k_st}, {v_sb, v_sh, v_st}, {o_sb, o_sh, o_st}, (int)H, (int)Tq, (int)Tk, (int)tiles, scale};
  const dim3 grid((uint32_t)(B * H * tiles)), block(64 * DLMCQ_AT_WAVES);
  if (D == 64) hipLaunchKernelGGL((attention_kernel<64>), grid, block, 0, reinterpret_cast<hipStream_t>(stream), a, ep);
  else hipLaunchKernelGGL((attention_kernel<32>), grid, block, 0, reinterpret_cast<hipStream_t>(stream), a, ep);
  return launch_status();
}
