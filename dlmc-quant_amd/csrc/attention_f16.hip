// Scaled dot-product attention softmax(scale q k^T) v of fp32 [B, H, T, D] views, D in {32, 64}, on the f16 matrix cores: the same
// flash forward, arguments, views, refusals and quantiser tail as dlmcq_attention_f32 (csrc/attention.hip), with q, k, v and the
// softmax weights p as f16 OPERANDS of v_mfma_f32_32x32x16_f16 - 16 k values per lane pair and issue where v_mfma_f32_32x32x2_f32 takes
// 2 - and everything else (accumulation, scores, maximum, exp2, l, the rescale, the division, the output) in fp32.  Nothing 16-bit
// touches global memory: the fp32 inputs are read in place and converted inside the kernel, each element once per workgroup that
// needs it.  No mask, no bias, no causal flag.  The arithmetic, for query row i of one (b, h), keys j in blocks of 32, u = 2^-24,
// h(x) = x rounded to f16, round to nearest even (v_cvt_f16_f32 / v_cvt_pk_f16_f32; |x| > 65504 gives +-inf, |x| < 2^-14 is subnormal):
//     c    = fl32(scale * log2 e), computed in double on the host and rounded once: the scale is FOLDED into the base-2 exponent
//     a_ij = sum_k h(q_ik) h(k_jk), fp32 accumulation by D / 16 MFMAs of 16 products each, chained through the accumulator from +0.
//            The products of two f16 values are exact in fp32; the ORDER in which one MFMA adds its 16 products and the accumulator
//            is not documented and is NOT claimed here, and its additions are NOT round-to-nearest (measured: a negative addend of
//            2^-80 in the accumulator pulls an exact product sum of 32 down to the next fp32 below) - the sum is bounded, not
//            pinned: at most D additions, each off by at most one ulp, 2 u.
//     s_ij = fl32(a_ij * c)                one IEEE multiply; keys past Tk - 1 hold s = -inf (a select, no branch)
//     m'   = max(m, max_j s_ij)            15 v_max_f32 and one exchange with lane ^ 32; v_max drops NaNs: a NaN score reaches p instead
//     m~   = m', or 0 where m' = -inf
//     al   = exp2(fl32(m - m~)),  p_ij = exp2(fl32(s_ij - m~))      v_exp_f32, the hardware exp2 (1 ulp; a result below 2^-126 may be
//            flushed, which h() would round to 0 anyway), not the library's expf
//     P_ij = h(p_ij)                       ONE rounding to f16; P_ij < 2^-25 is 0, 2^-25 .. 2^-14 is subnormal (absolute error 2^-25)
//     l_h  = fl32(fl32(l_h * al) + t_h)    per lane half h; t_h the sum of the fp32 values of the half's 16 P_ij - of the ROUNDED weights,
//            so numerator and denominator see the same weights - as the balanced tree ((x0+x1)+(x2+x3))+((x4+x5)+(x6+x7)) + (the same
//            of x8 .. x15) over the accumulator registers 0 .. 15 (keys (r & 3) + 8 (r >> 2) + 4 h of the block)
//     o_ic = fl32(o_ic * al), then two MFMAs add sum_j h(v_jc) P_ij over the block's keys 0 .. 15 and 16 .. 31 into it (fp32
//            accumulation through the accumulator; products exact; the order inside an MFMA, again, bounded and not pinned).  Sums of
//            integers below 2^24 are exact in every order: that is what the bitwise tests use.
//     at the end: l = fl32(l_0 + l_1), out_ic = fl32(o_ic / l) - a true division; code = the consumer's quantiser of out_ic.
// Range: an input above 65504 in magnitude becomes +-inf in f16.  In q_i it makes row i non-finite and no other; in k_j every row of
// the head; in v_j[c] channel c of every row of the head (inf * P, or inf * 0 = NaN) and no other channel.  NaNs and infinities of the
// fp32 inputs propagate as in attention.hip.  This is documented, not checked at run time; an overflow of c itself (|scale| above
// 2.3e38) gives infinite scores and NaN rows.
// Lane and key maps.  S^T = k q^T is what the score MFMA computes (A = k: lane = key (lane & 31), 8 consecutive d per lane half; B =
// q^T: lane = query, the same 8 d), so a lane holds ONE query and 16 of the block's 32 keys: accumulator register r is key
// (r & 3) + 8 (r >> 2) + 4 half.  Step s (= 0, 1) of O^T = v^T P^T takes as B operand 8 k values per lane half: registers 8 s .. 8 s + 7,
// converted in place by 4 packed converts - keys 16 s + 4 half + {0 .. 3} and 16 s + 8 + 4 half + {0 .. 3}.  No lane movement, no LDS
// for P.  The A operand must hold v^T of the SAME keys in the same slots, so v is staged in LDS channel-major ([channel][32 keys] f16)
// with the keys of a block in that permuted order: key j stands at position j with bits 2 and 3 exchanged, and a lane's 8 halves of
// v^T for step s are the 16 bytes at position 16 s + 8 half of its channel's row - one ds_read_b128.  The transposition happens at the
// LDS WRITE (a thread loads the same 4 channels of two keys that are neighbours in that order - 2 j', 2 j' + 1 - and stores 4 packed
// pairs), not through the transposing LDS reads: those transpose within 16-lane groups of a key-major tile and would still need the
// key permutation as lane movement, while the write-side form costs 4 ds_write_b32 per 8 elements once per workgroup and leaves the
// four waves' reads - the larger traffic, 4 : 1 - as plain conflict-free 16-byte reads.  k is staged key-major ([32 keys][D] f16).
// LDS rows: k D + 8 halves (36 / 20 dwords: 16 lanes' 16-byte reads tile the banks), v 40 halves per channel (20 dwords, likewise)
// plus 8 halves per 16 channels (the pair stores of a wave - 16 channel quads x 4 position pairs at D = 64 - then hit 64 distinct
// banks).  Two buffers of each: 19.1 KiB at D = 64, 10.1 KiB at D = 32.
// Work split.  One workgroup of 4 waves owns 128 query rows of one (b, h), a wave 32 of them (q as f16 in D / 4 registers); idle waves
// (rows past Tq) only stage, and which wave that is rotates with the head index - attention.hip's split, kept because ViT's T = 197 is
// 7 waves of 32 either way and a taller workgroup would re-read nothing less.  Key block 32: one score tile, 16 + 8 live registers of
// s / P, against 64's 32 + 16 - the budget below is what buys the fourth wave per SIMD, and a block's MFMA work (8 issues at D = 64) is
// already short against its exp2 / convert work, so a longer block would not hide more.  Double buffer, ONE barrier per block: the
// fp32 rows of block b + 1 are loaded into registers before block b's math, converted and written to the other buffer after it, and
// the barrier that ends the iteration both publishes them and retires the reads of block b.  Registers: 32 (o) + 16 (s) + 8 (P) + 16
// (q) + 16 (staged rows) + addresses; held to 128 by __launch_bounds__(256, 4): 4 waves per SIMD (attention.hip: 2).  Table: DESIGN.md 5.32.
// Error bound against real arithmetic on the same fp32 inputs (p*, o* real), e = 2^-11:
//     delta_i = ((2 e + e^2) + (2 D + 3) u) |scale| max_j sum_k |q_ik k_jk|
//     rho_i   = expm1(2 delta_i + 2 e + e + 2^-20 + kappa u),   kappa = 2 (104 + 2 + 3 nb + 68 nb) + 1,  nb = ceil(Tk / 32)
//     |out_ic - o*_ic| <= rho_i sum_j p*_ij |v_jc| + Tk 2^-24 max_j |v_jc| + 2^-25
// delta_i bounds a score's error in natural-log units: two f16 roundings per product term ((1 + e)^2 - 1), D additions inside the
// MFMAs at 2 u each, the multiply by c and the rounding of c itself.  Scores enter only through differences, so every normalised weight
// is off by a factor within exp(+-2 delta_i) - expm1, not the first-order 2 delta_i: at e = 2^-11 and peaky rows delta_i reaches
// 10^-2 and the second order counts.  The rounding of p to P is relative e on every weight, numerator and denominator alike: a factor
// within (1 +- e) / (1 -+ e), 2 e (its third order is inside 2^-20); the rounding of v is e on every term; 2^-20 also covers the cross
// terms of these.  kappa u: the fp32 terms of attention.hip's bound, unchanged in form - the subtractions telescope to u |x| with
// |x| ln 2 <= 104 for every term that is not 0 (here: below 2^-150 <<< 2^-25), v_exp_f32 1 ulp = 2 u, 3 u per later block for al and
// the multiply, per block at most 34 additions at 2 u in o (two MFMAs of 16 products and the accumulator) and 17 at u in l - 68 nb
// covers either -, twice, one division.  Absolute terms: a P in f16's subnormal range (or rounded
// to 0) is off by at most 2^-25; l >= 1 (the maximal key's P is exactly 1 and is never rescaled below 1), so over Tk keys numerator
// and denominator are each off by at most Tk 2^-25 max_j |v_jc| relative to l: Tk 2^-24 max_j |v_jc|.  An f16-subnormal v (|v| < 2^-14)
// is off by 2^-25, times weights that sum to 1.  No margin factor.  Measured ratios: DESIGN.md 5.32.
// No atomics, no scratch: a row's result depends neither on B, H, its (b, h) nor on the launch.
#include "attention_common.h"

namespace dlmcq {

template <int D>
struct AttnF16 {
  static constexpr int THREADS = 64 * DLMCQ_AT_WAVES, D4 = D / 4, CB = D / 32, QS = D / 16;
  static constexpr int KROW = D + 8;                              // halves per key row of k
  static constexpr int VSIZE = D * 40 + (D / 16) * 8;             // halves of one v buffer
  static constexpr int KIT = DLMCQ_AT_KB * D4 / THREADS;          // k quads per thread and block: 2 / 1
  static constexpr int VITEMS = (DLMCQ_AT_KB / 2) * D4;           // (position pair, channel quad) items of v per block: 256 / 128
  __device__ static constexpr int vrow(int c) { return c * 40 + (c >> 4) * 8; }

  // the fp32 rows of one key block, as loaded: k quads [KIT], v quads of the two keys of this thread's item
  struct Staged {
    f32x4 k[KIT], v0, v1;
  };

  __device__ static __forceinline__ f32x4 row4(const float* base, int64_t stride, int key, int Tk, int c4) {
    const bool in = key < Tk;      // (a row past Tk: the last valid row is read again and replaced by +0)
    const f32x4 t = *reinterpret_cast<const f32x4*>(base + (int64_t)(in ? key : Tk - 1) * stride + c4 * 4);
    return in ? t : f32x4{0.0f, 0.0f, 0.0f, 0.0f};
  }

  __device__ static __forceinline__ void load(Staged& st, const AttnArgs& a, const float* kb_, const float* vb_, int kb, int tid) {
#pragma unroll
    for (int it = 0; it < KIT; ++it) {
      const int idx = tid + it * THREADS;
      st.k[it] = row4(kb_, a.ks[2], kb * DLMCQ_AT_KB + idx / D4, a.Tk, idx % D4);
    }
    if (VITEMS >= THREADS || tid < VITEMS) {      // (D = 32: waves 0 and 1)
      const int key = swap23(2 * (tid / D4));
      st.v0 = row4(vb_, a.vs[2], kb * DLMCQ_AT_KB + key, a.Tk, tid % D4);
      st.v1 = row4(vb_, a.vs[2], kb * DLMCQ_AT_KB + key + 1, a.Tk, tid % D4);
    }
  }

  __device__ static __forceinline__ void stage(const Staged& st, _Float16* lk, _Float16* lv, int tid) {
#pragma unroll
    for (int it = 0; it < KIT; ++it) {
      const int idx = tid + it * THREADS;
      const f16x2 lo = h2(st.k[it].x, st.k[it].y), hi = h2(st.k[it].z, st.k[it].w);
      *reinterpret_cast<f16x4*>(&lk[(idx / D4) * KROW + (idx % D4) * 4]) = f16x4{lo.x, lo.y, hi.x, hi.y};
    }
    if (VITEMS >= THREADS || tid < VITEMS) {
      const int c = 4 * (tid % D4);
      store_v_pairs(lv, vrow(c), vrow(c + 1), vrow(c + 2), vrow(c + 3), 2 * (tid / D4), st.v0, st.v1);
    }
  }
};

template <int D>
__global__ __launch_bounds__(64 * DLMCQ_AT_WAVES, 4) void attention_f16_kernel(AttnArgs a, ConvEpi ep) {
  using T = AttnF16<D>;
  constexpr int CB = T::CB, QS = T::QS, KROW = T::KROW;
  __shared__ __attribute__((aligned(16))) _Float16 lds_k[2][DLMCQ_AT_KB * KROW];
  __shared__ __attribute__((aligned(16))) _Float16 lds_v[2][T::VSIZE];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, col = lane & 31, half = lane >> 5;
  const int bh = (int)(blockIdx.x / (uint32_t)a.tiles), tile = (int)(blockIdx.x % (uint32_t)a.tiles);
  const int b = bh / a.H, h = bh % a.H;
  const int q0 = tile * DLMCQ_AT_ROWS + ((wave + bh) & (DLMCQ_AT_WAVES - 1)) * 32;
  const bool active = q0 < a.Tq;      // (wave-uniform)
  const int qi = q0 + col;
  const float* kb_ = a.k + b * a.ks[0] + h * a.ks[1];
  const float* vb_ = a.v + b * a.vs[0] + h * a.vs[1];

  typename T::Staged st;
  T::load(st, a, kb_, vb_, 0, tid);
  f16x8 qh[QS];      // h(q_i[16 s + 8 half .. + 7]): the B operand of score step s
  if (active) load_operand_f16<QS>(a.q + b * a.qs[0] + h * a.qs[1] + (int64_t)(qi < a.Tq ? qi : a.Tq - 1) * a.qs[2], half, qh);
  f32x16 o[CB];
#pragma unroll
  for (int cb = 0; cb < CB; ++cb)
#pragma unroll
    for (int r = 0; r < 16; ++r) o[cb][r] = 0.0f;
  float m = -__builtin_inff(), l = 0.0f;
  const int nkb = (a.Tk + DLMCQ_AT_KB - 1) / DLMCQ_AT_KB;
  T::stage(st, lds_k[0], lds_v[0], tid);
  __syncthreads();
  for (int kb = 0; kb < nkb; ++kb) {
    const bool more = kb + 1 < nkb;      // (uniform over the workgroup)
    if (more) T::load(st, a, kb_, vb_, kb + 1, tid);
    if (active) {
      const _Float16* lk = lds_k[kb & 1];
      const _Float16* lv = lds_v[kb & 1];
      f32x16 s;
#pragma unroll
      for (int r = 0; r < 16; ++r) s[r] = 0.0f;
#pragma unroll
      for (int t = 0; t < QS; ++t)
        s = __builtin_amdgcn_mfma_f32_32x32x16_f16(*reinterpret_cast<const f16x8*>(&lk[col * KROW + 16 * t + 8 * half]), qh[t], s, 0, 0, 0);
#pragma unroll
      for (int r = 0; r < 16; ++r) s[r] = s[r] * a.scale;
      mask_tail(s, kb * DLMCQ_AT_KB + 4 * half, a.Tk);
      const float bm = acc_max(-__builtin_inff(), s);
      const float mn = fmaxf(m, fmaxf(bm, other_half(bm)));
      const float mu = mn == -__builtin_inff() ? 0.0f : mn;
      const float al = __builtin_amdgcn_exp2f(m - mu);
      m = mn;
      f16x8 ph[2];
      l = l * al + p_step_f16<true>(s, mu, ph);      // (the scale holds log2 e: the scores are in base-2 units)
#pragma unroll
      for (int cb = 0; cb < CB; ++cb) {
#pragma unroll
        for (int r = 0; r < 16; ++r) o[cb][r] *= al;
#pragma unroll
        for (int t = 0; t < 2; ++t)
          o[cb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(*reinterpret_cast<const f16x8*>(&lv[T::vrow(cb * 32 + col) + 16 * t + 8 * half]),
                                                         ph[t], o[cb], 0, 0, 0);
      }
    }
    if (more) T::stage(st, lds_k[(kb + 1) & 1], lds_v[(kb + 1) & 1], tid);
    __syncthreads();      // (block kb + 1 is published; every read of block kb is done)
  }
  if (!active) return;
  l = l + other_half(l);
  if (qi >= a.Tq) return;
  store_normalised<CB>(o, l, a.out, ep, EpiQuant(ep), b * a.os[0] + h * a.os[1] + (int64_t)qi * a.os[2], half);
}

}  // namespace dlmcq

using namespace dlmcq;

// The checks and the launch: attention_args, attention_launch (csrc/attention_common.h), shared with dlmcq_attention_f32; the kernel
// takes c = fl32(scale log2 e) for the scale.
extern "C" int dlmcq_attention_f16(const float* q, const float* k, const float* v, float* out, void* codes, int64_t B, int64_t H, int64_t Tq,
                                   int64_t Tk, int64_t D, int64_t q_sb, int64_t q_sh, int64_t q_st, int64_t k_sb, int64_t k_sh, int64_t k_st,
                                   int64_t v_sb, int64_t v_sh, int64_t v_st, int64_t o_sb, int64_t o_sh, int64_t o_st, float scale,
                                   const float* q_scale, const float* q_zero_point, int32_t q_lo, int32_t q_hi, int32_t q_form, float q_ste_g,
                                   dlmcq_stream_t stream) {
  const int64_t strides[12] = {q_sb, q_sh, q_st, k_sb, k_sh, k_st, v_sb, v_sh, v_st, o_sb, o_sh, o_st};
  AttnArgs a;
  ConvEpi ep;
  int64_t blocks;
  const int rc = attention_args(a, ep, &blocks, q, k, v, out, codes, B, H, Tq, Tk, D, strides, scale, q_scale, q_zero_point, q_lo, q_hi, q_form,
                                q_ste_g);
  if (rc != DLMCQ_OK || blocks == 0) return rc;
  a.scale = (float)((double)scale * 1.4426950408889634074);
  return attention_launch(attention_f16_kernel<64>, attention_f16_kernel<32>, a, ep, blocks, 64 * DLMCQ_AT_WAVES, D, stream);
}
