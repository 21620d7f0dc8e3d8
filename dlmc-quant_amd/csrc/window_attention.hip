// Window attention softmax(scale q k^T + bias + mask) v of fp32 [B, H, T, D] views, T = Tq = Tk in 1 .. 64, D in {32, 64}, to fp32 and / or
// the activation codes of the projection that reads the merged heads: the attention of a windowed transformer (Swin, LeViT, BEiT), whose
// every block adds a relative-position bias [H, T, T] and whose every second block a shift mask [nW, T, T] (row b % nW for batch element
// b: B = images * nW, the window index fastest).  ONE wave owns one (b, h) and holds the whole T x T score tile in registers: no key
// stream, no running maximum, no rescale, no workgroup barrier.  The arithmetic, once, for query row i of one (b, h), u = 2^-24:
//     a_ij = fmaf(q_i[D-1], k_j[D-1], ... fmaf(q_i[1], k_j[1], fmaf(q_i[0], k_j[0], +0)))   the k-ordered chain of v_mfma_f32_32x32x2_f32
//     s_ij = fl32(a_ij * scale)                                                              one IEEE multiply
//     s_ij = fl32(s_ij + bias[h, i, j])              if bias
//     s_ij = fl32(s_ij + mask[b % nW, i, j])         if mask       (bias first, then mask: Swin's order)
//     m    = max_j s_ij over j < T       v_max_f32, which drops NaNs: a NaN score never becomes the maximum (it reaches p, below)
//     m~   = m, or 0 where m = -inf      (a row whose every key is masked with -inf: no inf - inf here)
//     p_ij = expf(fl32(s_ij - m~))       the device library's accurate expf (1 ulp), not v_exp_f32
//     t_h  = per half h of every 32-key block (keys with bit 2 clear / set: the two lane halves) the half's p_ij - 16 per block, the
//            blocks in ascending order - added one by one from p of the lowest key, in ascending key order;  l = fl32(t_0 + t_1)
//     w_g  = the fmaf chain fmaf(v_j[c], p_ij, w_g) from +0 over the 8 keys 8 g .. 8 g + 7 of a block (g = 0 .. 3) in the order
//            0 4 1 5 2 6 3 7  (+ 8 g + 32 b: the accumulator rows of the 32x32 MFMA tile as its k steps) - csrc/attention.hip's order
//     o_ic = fl32(fl32(w_0 + w_1) + fl32(w_2 + w_3)) of block 0, and for T > 32 fl32(that + the same of block 1)
//     out_ic = fl32(o_ic / l) - a true division, correctly rounded;  code = the consumer's quantiser of out_ic (EpiQuant::code4, plain codes)
// - each step rounded to fp32 by itself under the library's flags.  Keys past T - 1 hold s = -inf (p = +0 exactly) and v = +0.
// Non-finite values: a -inf bias or mask entry removes its key (p = +0: the key adds nothing to l or o); a row whose every key is -inf
// has l = 0 and is NaN (0 / 0), as torch's softmax makes it, and no other row is touched (a query lives in its own two lanes); a NaN
// in q_i makes row i NaN, a NaN in any k_j every row of the head, a NaN in v_j[c] column c of every row of the head, a +inf score its
// row (expf(inf - inf)): the NaNs of torch's unfused graph, as csrc/attention.hip has them.
// Error bound against real arithmetic on the same fp32 inputs (s*, p*, o* real), nb = ceil(T / 32), t = how many of bias, mask are given:
//     delta_i = max over the finite keys j of  (D + 1) u |scale| sum_k |q_ik k_jk|  +  t u (|scale a*_ij| + |bias_ij| + |mask_ij|)
//     |out_ic - o*_ic| <= (2 delta_i + kappa u) sum_j p*_ij |v_jc| + 2^-126 max_j |v_jc|,   kappa = 2 (104 + 2 + 32 nb) + 1.
// delta_i bounds a score's error: D roundings of the chain and one of the multiply, as in csrc/attention.hip, and one rounding per
// additive term, each of a sum no larger than |scale a| + |bias| + |mask|; scores enter only through differences, hence 2 delta_i.
// Per term of the numerator and of l: the one subtraction s - m~ rounds its result, at most u (m - s_ij), and a term with m - s_ij >
// 104 is 0 in fp32 and below 2^-149 in real arithmetic (the last summand) - 104; expf 1 ulp = 2 u; the sum of l at most one rounding
// per key, 32 nb (the chains, the tree and the block add of o: fewer); twice, for numerator and denominator; one division.  There is
// no `al` - csrc/attention.hip's 3 nb is gone.  Measured ratios: DESIGN.md 5.31.
// The wave computes S^T = k q^T (A = k, B = q^T), csrc/attention.hip's lane map: a lane holds ONE query (lane & 31) of a 32-query tile
// and 16 keys of each 32-key block in its accumulator registers (keys (r & 3) + 8 (r >> 2) + 4 (lane >> 5)); q and k are each lane's own
// 16-byte row loads, straight to the MFMA operands; the row maximum is 31 v_max and one exchange with lane ^ 32, and P^T register r is,
// as it stands, the B operand of k step r of O^T = v^T P^T.  bias and mask: the 4 keys of registers 4 g .. 4 g + 3 are consecutive, so
// a lane reads its query's row in 16-byte pieces that land in the registers that want them - no transpose, no LDS; the two halves of
// the wave read adjacent pieces, and the pieces of a row are consumed back to back (one cache line serves them).  That is why a row's
// stride is a multiple of 4 floats: the piece that holds key T - 1 is read whole (its floats past T - 1 are dropped under a select; a
// piece wholly past T - 1 is not read: piece 0 is read again).  v needs the channel on the lane: each wave stages its head's v through
// a private slice of LDS (coalesced 16-byte row loads; rows padded by 8 floats), ordered by the wave's own in-order LDS queue.  Rows
// past T - 1 are never read: the last valid row is read again and replaced (k, v) or not stored (q), under selects, not branches.
// A workgroup is 4 waves = 4 consecutive (b, h): neighbouring heads of one window, which share the cache lines of the packed qkv rows.
// LDS 40 KiB (D = 32) / 72 KiB (D = 64) per workgroup: two workgroups fit a CU at D = 64.  No atomics, no scratch: a row's result
// depends neither on B, H, its (b, h) nor on the launch.
#include "attention_common.h"

namespace dlmcq {

template <int D>
__global__ __launch_bounds__(64 * DLMCQ_WA_WAVES) void window_attention_kernel(WinAttnArgs a, ConvEpi ep) {
  constexpr int VS = D + 8, D4 = D / 4, CB = D / 32;
  __shared__ __attribute__((aligned(16))) float lds_all[DLMCQ_WA_WAVES * DLMCQ_WA_TMAX * VS];
  const int lane = threadIdx.x & 63, col = lane & 31, half = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int pair = (int)blockIdx.x * DLMCQ_WA_WAVES + wave;
  if (pair >= a.pairs) return;      // (wave-uniform, and the kernel has no workgroup barrier)
  const int b = pair / a.H, h = pair % a.H, T = a.T;
  const int nkb = (T + 31) >> 5;      // 32-key blocks = 32-query tiles: 1 or 2
  float* lds_v = lds_all + wave * (DLMCQ_WA_TMAX * VS);
  const float* qb = a.q + b * a.qs[0] + h * a.qs[1];
  const float* kb_ = a.k + b * a.ks[0] + h * a.ks[1];
  const float* vb = a.v + b * a.vs[0] + h * a.vs[1];
  const float* bias = a.bias ? a.bias + h * a.bias_sh : nullptr;
  const float* mask = a.mask ? a.mask + (b % a.nW) * a.mask_sw : nullptr;

  // v of the head -> this wave's LDS rows, +0 past T - 1
  for (int idx = lane; idx < nkb * 32 * D4; idx += 64) {
    const int row = idx / D4, c4 = idx % D4;
    f32x4 vv = *reinterpret_cast<const f32x4*>(vb + (int64_t)(row < T ? row : T - 1) * a.vs[2] + c4 * 4);
    if (row >= T) vv = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    *reinterpret_cast<f32x4*>(&lds_v[row * VS + c4 * 4]) = vv;
  }
  // (the wave's LDS instructions complete in order; the fences keep the compiler from moving the reads above the writes)
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");

  const EpiQuant eq(ep);
  for (int qt = 0; qt < nkb; ++qt) {
    const int qi = qt * 32 + col, qrow = qi < T ? qi : T - 1;
    float qr[D / 2];
    load_operand_row<D>(qb, a.qs[2], qrow, half, qr);
    f32x16 s[2];
#pragma unroll
    for (int kb = 0; kb < 2; ++kb) {
#pragma unroll
      for (int r = 0; r < 16; ++r) s[kb][r] = kb < nkb ? 0.0f : -__builtin_inff();
      if (kb >= nkb) continue;      // (wave-uniform)
      const int key = kb * 32 + col;
      float kr[D / 2];
      load_operand_row<D>(kb_, a.ks[2], key < T ? key : T - 1, half, kr);
#pragma unroll
      for (int st = 0; st < D / 2; ++st) s[kb] = __builtin_amdgcn_mfma_f32_32x32x2f32(kr[st], qr[st], s[kb], 0, 0, 0);
      const int key0 = kb * 32 + 4 * half;
#pragma unroll
      for (int r = 0; r < 16; ++r) s[kb][r] = s[kb][r] * a.scale;
      if (bias) add_term(s[kb], bias + (int64_t)qrow * a.bias_st, key0, T);
      if (mask) add_term(s[kb], mask + (int64_t)qrow * a.mask_st, key0, T);
      mask_tail(s[kb], key0, T);
    }
    float m = acc_max(acc_max(-__builtin_inff(), s[0]), s[1]);
    m = fmaxf(m, other_half(m));
    const float mu = m == -__builtin_inff() ? 0.0f : m;
    float l = 0.0f;
#pragma unroll
    for (int kb = 0; kb < 2; ++kb) {
      if (kb >= nkb) continue;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        s[kb][r] = expf(s[kb][r] - mu);
        l = (kb | r) ? l + s[kb][r] : s[kb][r];
      }
    }
    l = l + other_half(l);
    const int64_t at = b * a.os[0] + h * a.os[1] + (int64_t)qi * a.os[2];
#pragma unroll
    for (int cb = 0; cb < CB; ++cb) {
      f32x16 o;
#pragma unroll
      for (int kb = 0; kb < 2; ++kb) {
        if (kb >= nkb) continue;
        // four independent chains of 8 keys, every one from +0, added as a tree: csrc/attention.hip's order and its reason
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
            const int r = 4 * g + rr;
            t4[g] = __builtin_amdgcn_mfma_f32_32x32x2f32(lds_v[(kb * 32 + acc_key(r, half)) * VS + cb * 32 + col], s[kb][r], t4[g], 0, 0, 0);
          }
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const float w = (t4[0][r] + t4[1][r]) + (t4[2][r] + t4[3][r]);
          o[r] = kb ? o[r] + w : w;
        }
      }
      if (qi < T) store_normalised<1>(&o, l, a.out, ep, eq, at + cb * 32, half);
      __builtin_amdgcn_sched_barrier(0);      // (one channel block's accumulators at a time)
    }
  }
}

}  // namespace dlmcq

using namespace dlmcq;

// The checks and the launch: window_attention_args, attention_launch (csrc/attention_common.h), shared with dlmcq_window_attention_f16.
extern "C" int dlmcq_window_attention_f32(const float* q, const float* k, const float* v, const float* bias, const float* mask, float* out,
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
  return attention_launch(window_attention_kernel<64>, window_attention_kernel<32>, a, ep, blocks, 64 * DLMCQ_WA_WAVES, D, stream);
}
