// Window attention softmax(scale q k^T + bias + mask) v of fp32 [B, H, T, D] views past one wave's score tile: T = Tq = Tk in 1 .. 256,
// D in {32, 64}, the arguments, terms, refusals and quantiser tail of dlmcq_window_attention_f32 (csrc/window_attention.hip) - the 12 x 12
// and 16 x 16 windows of Swin at 384^2 (T = 144, 256) and biased whole-image attention (BEiT, LeViT: T = 196, 197).  ONE WORKGROUP owns
// one (b, h) whole: ceil(T / 32) waves, each a 32-query tile for the whole kernel, k and v of the head staged in LDS once behind one
// barrier, and then every wave streams over the key blocks by itself - no further barrier.  The scores are made as
// csrc/window_attention.hip makes them and folded as csrc/attention.hip folds them.  For query row i of one (b, h), keys in blocks of
// 32, u = 2^-24:
//     a_ij = fmaf(q_i[D-1], k_j[D-1], ... fmaf(q_i[1], k_j[1], fmaf(q_i[0], k_j[0], +0)))   the k-ordered chain of v_mfma_f32_32x32x2_f32
//     s_ij = fl32(a_ij * scale)                                                              one IEEE multiply
//     s_ij = fl32(s_ij + bias[h, i, j])              if bias
//     s_ij = fl32(s_ij + mask[b % nW, i, j])         if mask       (bias first, then mask: Swin's order)            [window_attention.hip]
//     keys past T - 1 hold s = -inf under a select (p = +0 exactly), and their k and v rows are +0                 [window_attention.hip]
//     per key block, with m the running maximum (-inf before the first block):                                     [attention.hip, to the end]
//     m'   = max(m, max_j s_ij)            v_max_f32, which drops NaNs: a NaN score never becomes the maximum (it reaches p, below)
//     m~   = m', or 0 where m' = -inf      (a row that has met only -inf scores so far: no inf - inf)
//     al   = expf(fl32(m - m~))            the device library's accurate expf (1 ulp), not v_exp_f32; 0 while m = -inf
//     p_ij = expf(fl32(s_ij - m~))
//     l_h  = fl32(fl32(l_h * al) + t_h)    per half h of the block's keys (keys with bit 2 clear / set: the two lane halves), t_h the
//                                          half's 16 p_ij added one by one from p of the lowest key, in ascending key order
//     w_g  = the fmaf chain fmaf(v_j[c], p_ij, w_g) from +0 over the 8 keys 8 g .. 8 g + 7 of the block (g = 0 .. 3) in the order
//            0 4 1 5 2 6 3 7  (+ 8 g + 32 b: the accumulator rows of the 32x32 MFMA tile as its k steps)
//     o_ic = fl32(fl32(o_ic * al) + fl32(fl32(w_0 + w_1) + fl32(w_2 + w_3)))
//     after the last block: l = fl32(l_0 + l_1), out_ic = fl32(o_ic / l) - a true division, correctly rounded
//     code = the consumer's quantiser of out_ic (EpiQuant::code4, plain codes)                                     [store_normalised]
// - each step rounded to fp32 by itself under the library's flags.
// Non-finite values, the rules of both kernels: a -inf bias or mask entry removes its key (p = +0: the key adds nothing to l or o); a
// row whose every key is -inf has l = 0 and is NaN (0 / 0), as torch's softmax makes it, and no other row is touched (a query lives in
// its own two lanes of its own wave).  A key block that is all -inf for a row leaves l and o of that row as they were: before the row's
// first finite key m = -inf, m~ = 0, al = expf(-inf) = +0 and l, o are zeros that stay zeros; after it m' = m, al = expf(0) = 1, every
// p = +0, and x * 1 + 0 = x.  A NaN in q_i makes row i NaN, a NaN in any k_j every row of the head, a NaN in v_j[c] column c of every
// row of the head, a +inf score its row (expf(inf - inf)): the NaNs of torch's unfused graph.
// Error bound against real arithmetic on the same fp32 inputs (s*, p*, o* real), nb = ceil(T / 32), t = how many of bias, mask are given:
//     delta_i = max over the finite keys j of  (D + 1) u |scale| sum_k |q_ik k_jk|  +  t u (|scale a*_ij| + |bias_ij| + |mask_ij|)
//     |out_ic - o*_ic| <= (2 delta_i + kappa u) sum_j p*_ij |v_jc| + 2^-126 max_j |v_jc|,   kappa = 2 (104 + 2 + 3 nb + 32 nb) + 1.
// delta_i is window_attention.hip's: D roundings of the chain and one of the multiply, and one rounding per additive term, each of a
// sum no larger than |scale a| + |bias| + |mask|; scores enter only through differences, hence 2 delta_i.  kappa is attention.hip's:
// per term of the numerator and of l, the subtractions s - m~ and m - m~ round their results, in total (telescoped over the blocks: m
// only rises) at most u (m_final - s_ij), and a term with m_final - s_ij > 104 is 0 in fp32 and below 2^-149 in real arithmetic (the
// last summand) - 104; expf 1 ulp = 2 u; per later block one ulp of al and one multiply, 3 u - 3 nb; the sum of l at most one rounding
// per key, 32 nb (the chains, the tree and the block adds of o: fewer); twice, for numerator and denominator; one division.  No margin
// factor.  Measured ratios: DESIGN.md 5.36.
// The work split.  Grid = B H workgroups in (b, h) order: neighbours are the heads of one window and share the cache lines of the packed
// qkv rows.  A workgroup is W = ceil(T / 32) waves (3 .. 8 where the Python layer routes here; 1 or 2 are accepted), wave w the queries
// 32 w .. 32 w + 31, lane map as in the siblings (S^T = k q^T: a lane holds ONE query, lane & 31, and 16 keys of a block in its
// accumulator registers): q is each lane's own 16-byte row loads straight into the MFMA B operand (load_operand_row).  No wave is idle
// but for the rows of the last tile past T - 1, which read row T - 1 again and store nothing.
// The data movement.  k AND v of the head are staged in LDS (dynamic, sized to the window: 32 W rows, not 256), cooperatively, by
// coalesced 16-byte row loads - D / 8 per thread whatever T is -, k rows padded by 2 floats and v rows by 8 as attention.hip pads them,
// rows past T - 1 holding +0; one __syncthreads(); then no barrier: nothing in LDS is recycled, which is what owning the window buys
// (attention.hip pays two barriers per key block).  k from LDS and not from global: every one of the W waves needs every k row as its
// A operand, and from global that is W times the head's k through L1 as 16-byte loads at a row stride of 3 H D floats - one cache line
// per lane and instruction - where LDS serves it as a conflict-free 4-byte read; the budget allows it: (2 D + 10) * 4 bytes per row,
//     T <= 96: 27.8 / 51.8 KiB (D = 32 / 64)   T = 144: 46.3 / 86.3 KiB   T = 196, 197: 64.8 / 120.8 KiB   T = 256: 74 / 138 KiB
// of a CU's 160 KiB, so by LDS 3 / 1 workgroups (15 / 5 waves) per CU at T = 144 and 2 / 1 (16 / 8 waves) at T = 256.  Registers:
// 127 VGPRs at D = 32, 178 at D = 64 (__launch_bounds__(512): at most 256), no AGPRs, no spill, no scratch: 4 / 2 waves per SIMD, 16 / 8
// per CU - so the three workgroups of T = 144, D = 32 and the two of T = 256, D = 32 are resident together, and at D = 64 one is,
// by LDS and by registers alike.  Built WITHOUT packed fp32 instructions, the family's per-file flag in csrc/Makefile, because the
// register count asks for it: with them D = 32 takes 137 VGPRs - 3 waves per SIMD, two workgroups of T = 144 instead of three -
// and D = 64 the same 178.
// bias and mask are never staged: a lane reads its query's row of each term for the current key block in four 16-byte pieces that land
// in registers 4 g .. 4 g + 3 (add_term; row strides multiples of 4 floats, the piece that holds key T - 1 read whole); a [H, 144, 144]
// bias is 83 KB per head, shared by every window: it lives in L2.  No atomics, no scratch: a row's result depends neither on B, H, its
// (b, h) nor on the launch.
#include "attention_common.h"
#include "conv_i8_common.h"      // (launch_dyn_lds)

namespace dlmcq {

template <int D>
__global__ __launch_bounds__(512) void window_attention_stream_kernel(WinAttnArgs a, ConvEpi ep) {
  constexpr int KS = D + 2, VS = D + 8, D4 = D / 4, CB = D / 32;
  extern __shared__ __attribute__((aligned(16))) float ws_lds[];      // v rows [32 W][VS], then k rows [32 W][KS]
  const int tid = threadIdx.x, lane = tid & 63, col = lane & 31, half = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int T = a.T, nkb = (T + 31) >> 5, threads = 64 * nkb;      // (W = nkb waves were launched)
  const int b = (int)blockIdx.x / a.H, h = (int)blockIdx.x % a.H;
  float* lds_v = ws_lds;
  float* lds_k = ws_lds + nkb * 32 * VS;
  const float* kb_ = a.k + b * a.ks[0] + h * a.ks[1];
  const float* vb_ = a.v + b * a.vs[0] + h * a.vs[1];
  const float* bias = a.bias ? a.bias + h * a.bias_sh : nullptr;
  const float* mask = a.mask ? a.mask + (b % a.nW) * a.mask_sw : nullptr;

  // k and v of the head -> LDS, +0 past T - 1: 32 W rows of D4 pieces over 64 W threads, D4 / 2 pieces a thread
#pragma unroll
  for (int it = 0; it < D4 / 2; ++it) {
    const int idx = tid + it * threads, row = idx / D4, c4 = idx % D4;
    const bool in = row < T;
    const int64_t kr = in ? row : T - 1;
    f32x4 kk = *reinterpret_cast<const f32x4*>(kb_ + kr * a.ks[2] + c4 * 4);
    f32x4 vv = *reinterpret_cast<const f32x4*>(vb_ + kr * a.vs[2] + c4 * 4);
    if (!in) kk = f32x4{0.0f, 0.0f, 0.0f, 0.0f}, vv = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    *reinterpret_cast<f32x2*>(&lds_k[row * KS + c4 * 4]) = f32x2{kk.x, kk.y};
    *reinterpret_cast<f32x2*>(&lds_k[row * KS + c4 * 4 + 2]) = f32x2{kk.z, kk.w};
    *reinterpret_cast<f32x4*>(&lds_v[row * VS + c4 * 4]) = vv;
  }
  const int qi = wave * 32 + col, qrow = qi < T ? qi : T - 1;
  float qr[D / 2];      // q_i[2 s + half]: the B operand of k step s
  load_operand_row<D>(a.q + b * a.qs[0] + h * a.qs[1], a.qs[2], qrow, half, qr);
  if (bias) bias += (int64_t)qrow * a.bias_st;
  if (mask) mask += (int64_t)qrow * a.mask_st;
  __syncthreads();      // (the only one: from here a wave runs alone)

  f32x16 o[CB];
#pragma unroll
  for (int cb = 0; cb < CB; ++cb)
#pragma unroll
    for (int r = 0; r < 16; ++r) o[cb][r] = 0.0f;
  float m = -__builtin_inff(), l = 0.0f;
  for (int kb = 0; kb < nkb; ++kb) {
    const float* lk = lds_k + (kb * 32 + col) * KS + half;
    const float* lv = lds_v + (kb * 32 + 4 * half) * VS + col;
    f32x16 s;
#pragma unroll
    for (int r = 0; r < 16; ++r) s[r] = 0.0f;
#pragma unroll
    for (int st = 0; st < D / 2; ++st) s = __builtin_amdgcn_mfma_f32_32x32x2f32(lk[2 * st], qr[st], s, 0, 0, 0);
    const int key0 = kb * 32 + 4 * half;
#pragma unroll
    for (int r = 0; r < 16; ++r) s[r] = s[r] * a.scale;
    if (bias) add_term(s, bias, key0, T);
    if (mask) add_term(s, mask, key0, T);
    mask_tail(s, key0, T);
    const float bm = acc_max(-__builtin_inff(), s);
    const float mn = fmaxf(m, fmaxf(bm, other_half(bm)));
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
          t4[g] = __builtin_amdgcn_mfma_f32_32x32x2f32(lv[acc_key(r, 0) * VS + cb * 32], s[r], t4[g], 0, 0, 0);
        }
      }
#pragma unroll
      for (int r = 0; r < 16; ++r) o[cb][r] = o[cb][r] * al + ((t4[0][r] + t4[1][r]) + (t4[2][r] + t4[3][r]));
      __builtin_amdgcn_sched_barrier(0);      // (one channel block's four accumulators at a time: 64 registers, not 128)
    }
  }
  l = l + other_half(l);
  if (qi >= T) return;
  store_normalised<CB>(o, l, a.out, ep, EpiQuant(ep), b * a.os[0] + h * a.os[1] + (int64_t)qi * a.os[2], half);
}

template <int D>
static int window_attention_stream_launch(const WinAttnArgs& a, const ConvEpi& ep, dlmcq_stream_t stream) {
  const int waves = (a.T + 31) / 32;
  const size_t lds = (size_t)waves * 32 * (2 * D + 10) * sizeof(float);
  return launch_dyn_lds<window_attention_stream_kernel<D>>(dim3((uint32_t)a.pairs), dim3(64 * waves), lds, reinterpret_cast<hipStream_t>(stream),
                                                           a, ep);
}

}  // namespace dlmcq

using namespace dlmcq;

// The checks: window_attention_args (csrc/attention_common.h) with the token limit DLMCQ_WS_TMAX, shared with dlmcq_window_attention_f32
// and _f16; the launch: B H workgroups of ceil(T / 32) waves with the window's own LDS size.
extern "C" int dlmcq_window_attention_stream_f32(const float* q, const float* k, const float* v, const float* bias, const float* mask,
                                                 float* out, void* codes, int64_t B, int64_t H, int64_t T, int64_t D, int64_t nW, int64_t q_sb,
                                                 int64_t q_sh, int64_t q_st, int64_t k_sb, int64_t k_sh, int64_t k_st, int64_t v_sb,
                                                 int64_t v_sh, int64_t v_st, int64_t o_sb, int64_t o_sh, int64_t o_st, int64_t bias_sh,
                                                 int64_t bias_st, int64_t mask_sw, int64_t mask_st, float scale, const float* q_scale,
                                                 const float* q_zero_point, int32_t q_lo, int32_t q_hi, int32_t q_form, float q_ste_g,
                                                 dlmcq_stream_t stream) {
  const int64_t strides[12] = {q_sb, q_sh, q_st, k_sb, k_sh, k_st, v_sb, v_sh, v_st, o_sb, o_sh, o_st};
  WinAttnArgs a;
  ConvEpi ep;
  int64_t blocks;
  const int rc = window_attention_args(a, ep, &blocks, q, k, v, bias, mask, out, codes, B, H, T, D, nW, strides, bias_sh, bias_st, mask_sw,
                                       mask_st, scale, q_scale, q_zero_point, q_lo, q_hi, q_form, q_ste_g, DLMCQ_WS_TMAX);
  if (rc != DLMCQ_OK || blocks == 0) return rc;
  return D == 64 ? window_attention_stream_launch<64>(a, ep, stream) : window_attention_stream_launch<32>(a, ep, stream);
}
