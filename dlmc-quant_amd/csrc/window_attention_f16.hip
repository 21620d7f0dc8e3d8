// Window attention softmax(scale q k^T + bias + mask) v of fp32 [B, H, T, D] views, T = Tq = Tk in 1 .. 64, D in {32, 64}, on the f16
// matrix cores: the arguments, views, refusals, return codes and quantiser tail of dlmcq_window_attention_f32 (csrc/window_attention.hip)
// with q, k, v and the softmax weights p as f16 OPERANDS of v_mfma_f32_32x32x16_f16, and everything else - accumulation, scale, bias,
// mask, maximum, exp2, l, the division, the output - in fp32.  Nothing 16-bit touches global memory: the fp32 inputs are read in place
// and converted inside the kernel.  ONE wave owns one (b, h) and holds the whole T x T score tile: no key stream, no running maximum,
// no rescale, no workgroup barrier.  The arithmetic, for query row i of one (b, h), u = 2^-24, e = 2^-11, h(x) = x rounded to f16,
// round to nearest even (v_cvt_pk_f16_f32; |x| > 65504 gives +-inf, |x| < 2^-14 is subnormal):
//     a_ij = sum_k h(q_ik) h(k_jk), fp32 accumulation by D / 16 MFMAs of 16 products each, chained through the accumulator from +0.
//            The products are exact in fp32; the order in which one MFMA adds them and its rounding are bounded, not pinned
//            (csrc/attention_f16.hip says what was measured): at most D additions, each off by at most one ulp, 2 u.
//     s_ij = fl32(a_ij * scale)                      one IEEE multiply, in natural units: the scale is NOT folded into a base-2 constant,
//     s_ij = fl32(s_ij + bias[h, i, j])              if bias       so that a -100 or -inf mask entry and the bias keep their exact meaning
//     s_ij = fl32(s_ij + mask[b % nW, i, j])         if mask       (bias first, then mask: the fp32 window kernel's step)
//            keys past T - 1 hold s = -inf (a select, no branch)
//     m    = max_j s_ij                  v_max_f32 and one exchange with lane ^ 32; v_max drops NaNs: a NaN score reaches p instead
//     m~   = m, or 0 where m = -inf
//     p_ij = exp2(fl32(fl32(s_ij - m~) * L)),  L = fl32(log2 e) = 0x3fb8aa3b;  exp2 = v_exp_f32, the hardware exp2 (1 ulp; a result
//            below 2^-126 may be flushed, which h() would round to 0 anyway)
//     P_ij = h(p_ij)                     ONE rounding to f16; P_ij < 2^-25 is 0, 2^-25 .. 2^-14 is subnormal (absolute error 2^-25)
//     l_h  = per lane half h (keys with bit 2 clear / set) the sum of the fp32 values of the half's ROUNDED weights P_ij - numerator and
//            denominator see the same weights - per 32-key block the balanced tree ((x0+x1)+(x2+x3))+((x4+x5)+(x6+x7)) + (the same of
//            x8 .. x15) over the accumulator registers 0 .. 15 (keys (r & 3) + 8 (r >> 2) + 4 h of the block), for T > 32
//            fl32(block 0's + block 1's);  l = fl32(l_0 + l_1)
//     o_ic = sum_j h(v_jc) P_ij, two MFMAs per 32-key block (keys 0 .. 15, 16 .. 31) chained through the accumulator from +0, blocks
//            in ascending order (products exact; inside an MFMA, again, bounded and not pinned).  No rescale: there is no key stream.
//            Sums of integers below 2^24 are exact in every order: that is what the bitwise tests use.
//     out_ic = fl32(o_ic / l) - a true division;  code = the consumer's quantiser of out_ic (EpiQuant::code4, plain codes)
// Non-finite values and range: a -inf bias or mask entry removes its key (p = +0: it adds nothing to l or o); a row whose every key is
// -inf has l = 0 and is NaN (0 / 0), and no other row is touched (a query lives in its own two lanes).  An input above 65504 in
// magnitude is +-inf as an operand: in q_i it makes row i non-finite and no other; in k_j[c] it reaches every row of the head - row i
// is NaN where q_ic scale k_jc > 0 (s_ij = +inf) and loses key j where it is negative (s_ij = -inf: that row stays finite, as in torch's
// unfused graph on the rounded operands); in v_j[c] channel c of every row of the head (inf * P, or inf * 0 = NaN) and no other channel.
// Documented, not checked at run time.  NaNs and infinities of the fp32 inputs propagate as in window_attention.hip.
// Error bound against real arithmetic on the same fp32 inputs (s*, p*, o* real), nb = ceil(T / 32), t = how many of bias, mask are given:
//     delta_i = max over the finite keys j of ((2 e + e^2) + (2 D + 1) u) |scale| sum_k |q_ik k_jk| + t u (|scale a*_ij| + |bias_ij| + |mask_ij|)
//     rho_i   = expm1(2 delta_i + 3 e + 2^-20 + kappa u),   kappa = 2 (3 * 104 + 2 + 68 nb) + 1
//     |out_ic - o*_ic| <= rho_i sum_j p*_ij |v_jc| + T 2^-24 max_j |v_jc| + 2^-25
// delta_i bounds a score's error in natural units: two f16 roundings per product term ((1 + e)^2 - 1), D additions inside the MFMAs at
// 2 u each and the one multiply by the scale (attention_f16.hip's 2 D + 3 without the rounding of a folded constant and its multiply:
// they are per-weight terms here, below), and one rounding per additive term, each of a sum no larger than |scale a| + |bias| + |mask|
// (window_attention.hip's).  Scores enter only through differences, so every normalised weight is off by a factor within
// exp(+-2 delta_i) - expm1, not its first order.  3 e: the rounding of p to P is relative e on numerator and denominator alike, 2 e,
// and the rounding of v is e on every term; 2^-20 covers their cross terms and third order, as in attention_f16.hip.  kappa u, the
// fp32 steps per weight that is not 0, x = s - m~ with |x| <= 104 (below that p is 0 in fp32 and in real arithmetic under 2^-150 <<<
// 2^-25): the subtraction rounds x, u |x|; L is fl32(log2 e), relative error below u, and the product x L is rounded once - u |x| each
// in natural units: 3 * 104; v_exp_f32 1 ulp = 2 u; per block at most 34 additions at 2 u in o (two MFMAs of 16 products and the
// accumulator) and 17 at u in l - 68 nb covers either; twice, for numerator and denominator; one division.  There is no `al`:
// attention_f16.hip's 3 nb is gone.  Absolute terms, as there: a P in f16's subnormal range (or rounded to 0) is off by at most 2^-25
// and l >= 1 (the maximal key's P is exactly 1), so over T keys numerator and denominator are each off by at most T 2^-25 max_j |v_jc|
// relative to l; an f16-subnormal v is off by 2^-25, times weights that sum to 1.  No margin factor.  Measured ratios: DESIGN.md 5.33.
// Split.  A workgroup is 4 waves = 4 consecutive (b, h) (neighbouring heads of one window share the cache lines of the packed qkv
// rows); a wave past the pair count returns.  S^T = k q^T (A = k, B = q^T) with attention_f16.hip's lane map: a lane holds ONE query
// (lane & 31) of a 32-query tile and 16 keys of each 32-key block, accumulator register r = key (r & 3) + 8 (r >> 2) + 4 half - so the
// 4 keys of registers 4 g .. 4 g + 3 are consecutive and bias and mask are read by the fp32 kernel's add_term: 16-byte pieces of the
// lane's own query row, the same stride rule, the same last-piece handling.
// q and k do NOT go through LDS: a lane's operand for score step s is 8 consecutive d of its own row, 16 s + 8 half .. + 7 - two
// 16-byte loads and four packed converts, straight into the MFMA operand; the two lane halves read the two halves of a 64-byte
// piece.  Rows past T - 1 read the last valid row again (their scores are replaced by -inf, their outputs not stored).
// v needs the channel on the lane: each wave stages its head's v ONCE into a private slice of LDS as f16, channel-major ([channel][64
// positions]), the keys of each 32-block in the operand's order - position = key with bits 2 and 3 exchanged - so that a lane's 8
// halves of v^T for a step are one ds_read_b128 at position 32 kb + 16 t + 8 half.  The transposition is done at the LDS write (a lane
// loads 4 channels of the two keys at positions 2 p, 2 p + 1 - neighbours - and stores 4 packed pairs), +0 past T - 1.  Padding: a
// channel row is 64 + 8 halves = 36 dwords, so 16 lanes' 16-byte reads of 16 consecutive channels start at 36 i mod 64 - the 16
// multiples of 4 - and tile the 64 banks; and 8 more halves per 16 channels, so that the pair stores of one instruction - 16 channel
// quads x 4 position pairs at D = 64, 8 x 8 at D = 32 with the pairs taken in the order 0 1 2 3 8 9 10 11 - hit 64 distinct banks
// (144 c4 + 4 (c4 >> 2) + p mod 64).  9.06 KiB per wave at D = 64, 4.53 at D = 32 (fp32 kernel: 18 / 10): 36.25 / 18.1 KiB per
// workgroup, four workgroups in a CU's 160 KiB.  The reads are ordered behind the writes by the wave's own in-order LDS queue; the
// wave-scope fences keep the compiler from moving them.
// P is converted in place: registers 8 t .. 8 t + 7 of a lane half are the B operand of step t of O^T = v^T P^T.  No lane movement, no
// LDS for P.  Query tiles: two of 32 walked in turn (one when T <= 32), the tile body compiled once per block count (NKB = 1, 2; the
// choice is wave-uniform): straight-line code with no copies of the score registers around skipped blocks.  The converted k of a
// key block is LOADED AGAIN for the second query tile, not kept: k of both blocks is 16 / 32 registers (D = 32 / 64) that would live
// across the whole tile body, and keeping them was measured at 24 - 82 spilled registers under the 128 of 4 waves per SIMD; the
// second read is 2 / 4 16-byte loads per lane and block of rows the wave has just read (they hit the cache).  Live at the peak, D = 64:
// 32 (s) + 16 (k) + 16 (q) + 16 (a term's pieces), then 16 (P) + 16 (o, one channel block at a time).  __launch_bounds__(256, 4): at
// most 128 VGPRs; the compiler takes 115 / 83, no spill: 4 / 5 waves per SIMD (fp32 kernel: 2).  Table: DESIGN.md 5.33.
// No atomics, no scratch: a row's result depends neither on B, H, its (b, h) nor on the launch.
#include "attention_common.h"

namespace dlmcq {

template <int D>
struct WinF16 {
  static constexpr int D4 = D / 4, CB = D / 32, QS = D / 16;
  static constexpr int VSIZE = D * 72 + (D / 16) * 8;      // halves of one wave's v slice
  __device__ static constexpr int vrow(int c) { return c * 72 + (c >> 4) * 8; }

  // v of the head -> lv, f16, channel-major, the keys in the operand's order, +0 past T - 1.  Item y of a lane: position pair
  // lane / D4 + (64 / D4) y (D = 32: with bits 2 and 3 exchanged, the bank rule of the header), channels 4 (lane % D4) .. + 3
  __device__ static __forceinline__ void stage_v(_Float16* lv, const float* vb, int64_t stride, int T, int nkb, int lane) {
    const int c4 = lane % D4, c = 4 * c4;
    for (int y = lane / D4; y < 16 * nkb; y += 64 / D4) {
      const int pp = D == 32 ? swap23(y) : y, pos = 2 * pp, key = (pos & 32) | swap23(pos & 31);
      const bool in0 = key < T, in1 = key + 1 < T;      // (a row past T - 1: the last valid row is read again and replaced by +0)
      f32x4 v0 = *reinterpret_cast<const f32x4*>(vb + (int64_t)(in0 ? key : T - 1) * stride + c);
      f32x4 v1 = *reinterpret_cast<const f32x4*>(vb + (int64_t)(in1 ? key + 1 : T - 1) * stride + c);
      if (!in0) v0 = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
      if (!in1) v1 = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
      store_v_pairs(lv, vrow(c), vrow(c + 1), vrow(c + 2), vrow(c + 3), pos, v0, v1);
    }
  }
};

// the query tiles of one (b, h), NKB = ceil(T / 32) = 1 or 2 key blocks and query tiles: straight-line code per tile
template <int D, int NKB>
__device__ __forceinline__ void window_f16_tiles(const WinAttnArgs& a, const ConvEpi& ep, const _Float16* lv, int b, int h, int lane) {
  using W = WinF16<D>;
  constexpr int CB = W::CB, QS = W::QS;
  const int col = lane & 31, half = lane >> 5, T = a.T;
  const float* qb = a.q + b * a.qs[0] + h * a.qs[1];
  const float* kb_ = a.k + b * a.ks[0] + h * a.ks[1];
  const float* bias = a.bias ? a.bias + h * a.bias_sh : nullptr;
  const float* mask = a.mask ? a.mask + (b % a.nW) * a.mask_sw : nullptr;
  const EpiQuant eq(ep);
#pragma unroll 1
  for (int qt = 0; qt < NKB; ++qt) {
    const int qi = qt * 32 + col, qrow = qi < T ? qi : T - 1;
    f16x8 qh[QS];      // h(q_i[16 s + 8 half .. + 7]): the B operand of score step s
    load_operand_f16<QS>(qb + (int64_t)qrow * a.qs[2], half, qh);
    f32x16 s[NKB];
#pragma unroll
    for (int kb = 0; kb < NKB; ++kb) {
      const int key = kb * 32 + col, key0 = kb * 32 + 4 * half;
      f16x8 kh[QS];      // h(k_j[16 s + 8 half .. + 7]), j = 32 kb + col: the A operand of score step s
      load_operand_f16<QS>(kb_ + (int64_t)(key < T ? key : T - 1) * a.ks[2], half, kh);
#pragma unroll
      for (int r = 0; r < 16; ++r) s[kb][r] = 0.0f;
#pragma unroll
      for (int st = 0; st < QS; ++st) s[kb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(kh[st], qh[st], s[kb], 0, 0, 0);
#pragma unroll
      for (int r = 0; r < 16; ++r) s[kb][r] = s[kb][r] * a.scale;
      if (bias) add_term(s[kb], bias + (int64_t)qrow * a.bias_st, key0, T);
      if (mask) add_term(s[kb], mask + (int64_t)qrow * a.mask_st, key0, T);
      mask_tail(s[kb], key0, T);
      __builtin_amdgcn_sched_barrier(0);      // (one block's operands and term pieces at a time)
    }
    float m = -__builtin_inff();
#pragma unroll
    for (int kb = 0; kb < NKB; ++kb) m = acc_max(m, s[kb]);
    m = fmaxf(m, other_half(m));
    const float mu = m == -__builtin_inff() ? 0.0f : m;
    f16x8 ph[NKB][2];      // P^T: registers 8 t .. 8 t + 7 of block kb, the B operand of step t of O^T = v^T P^T
    float l = 0.0f;
#pragma unroll
    for (int kb = 0; kb < NKB; ++kb) {
      const float t = p_step_f16<false>(s[kb], mu, ph[kb]);      // (natural units: the exponent's argument is (s - m~) * fl32(log2 e))
      l = kb ? l + t : t;
    }
    l = l + other_half(l);
    const int64_t at = b * a.os[0] + h * a.os[1] + (int64_t)qi * a.os[2];
#pragma unroll
    for (int cb = 0; cb < CB; ++cb) {
      f32x16 o;
#pragma unroll
      for (int r = 0; r < 16; ++r) o[r] = 0.0f;
#pragma unroll
      for (int kb = 0; kb < NKB; ++kb)
#pragma unroll
        for (int t = 0; t < 2; ++t)
          o = __builtin_amdgcn_mfma_f32_32x32x16_f16(*reinterpret_cast<const f16x8*>(&lv[W::vrow(cb * 32 + col) + 32 * kb + 16 * t + 8 * half]),
                                                     ph[kb][t], o, 0, 0, 0);
      if (qi < T) store_normalised<1>(&o, l, a.out, ep, eq, at + cb * 32, half);
      __builtin_amdgcn_sched_barrier(0);      // (one channel block's accumulators at a time)
    }
  }
}

template <int D>
__global__ __launch_bounds__(64 * DLMCQ_WA_WAVES, 4) void window_attention_f16_kernel(WinAttnArgs a, ConvEpi ep) {
  using W = WinF16<D>;
  __shared__ __attribute__((aligned(16))) _Float16 lds_all[DLMCQ_WA_WAVES * W::VSIZE];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int pair = (int)blockIdx.x * DLMCQ_WA_WAVES + wave;
  if (pair >= a.pairs) return;      // (wave-uniform, and the kernel has no workgroup barrier)
  const int b = pair / a.H, h = pair % a.H;
  const int nkb = (a.T + 31) >> 5;      // 32-key blocks = 32-query tiles: 1 or 2
  _Float16* lv = lds_all + wave * W::VSIZE;
  W::stage_v(lv, a.v + b * a.vs[0] + h * a.vs[1], a.vs[2], a.T, nkb, lane);
  // (the wave's LDS instructions complete in order; the fences keep the compiler from moving the reads above the writes)
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  if (nkb == 2) window_f16_tiles<D, 2>(a, ep, lv, b, h, lane);      // (wave-uniform)
  else window_f16_tiles<D, 1>(a, ep, lv, b, h, lane);
}

}  // namespace dlmcq

using namespace dlmcq;

// The checks and the launch: window_attention_args, attention_launch (csrc/attention_common.h), shared with dlmcq_window_attention_f32.
extern "C" int dlmcq_window_attention_f16(const float* q, const float* k, const float* v, const float* bias, const float* mask, float* out,
                                          void* codes, int64_t B, int64_t H, int64_t T, int64_t D, int64_t nW, int64_t q_sb, int64_t q_sh,
                                          int64_t q_st, int64_t k_sb, int64_t k_sh, int64_t k_st, int64_t v_sb, int64_t v_sh, int64_t v_st,
                                          int64_t o_sb, int64_t o_sh, int64_t o_st, int64_t bias_sh, int64_t bias_st, int64_t mask_sw,
                                          int64_t mask_st, float scale, const float* q_scale, const float* q_zero_point, int32_t q_lo,
                                          int32_t q_hi, int32_t q_form, float q_ste_g, dlmcq_stream_t stream) {
  const int64_t strides[12] = {q_sb, q_sh, q_st, k_sb, k_sh, k_st, v_sb, v_sh, v_st, o_sb, o_sh, o_st};
  WinAttnArgs a;
  ConvEpi ep;
  int64_t blocks;
  const int rc = window_attention_args(a, ep, &blocks, q, k, v, bias, mask, out, codes, B, H, T, D, nW, strides, bias_sh, bias_st, mask_sw,
                                       mask_st, scale, q_scale, q_zero_point, q_lo, q_hi, q_form, q_ste_g);
  if (rc != DLMCQ_OK || blocks == 0) return rc;
  return attention_launch(window_attention_f16_kernel<64>, window_attention_f16_kernel<32>, a, ep, blocks, 64 * DLMCQ_WA_WAVES, D, stream);
}
