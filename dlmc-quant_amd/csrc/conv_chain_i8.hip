// A residual block's LAST 1x1 convolution (+ shortcut + ReLU + the consumer's quantiser) and the NEXT block's FIRST 1x1
// convolution (+ ReLU + its consumer's quantiser) as ONE kernel.  (FSPTQuant/base.py:95-159 twice, with the `out += identity;
// relu` of the model between them; same arithmetic, same order as conv_i8.hip's kernel run twice: bit-identical.)
//
// Why: the block-end layer is an HBM stream (4 B shortcut in + 4 B fp32 out per element for a 64..256-deep reduction, MFMA
// 3-5 % busy) and the activation codes it writes are read back exactly once, by the 1x1 reduction that follows, whose own
// time is all operand traffic.  Here a workgroup owns <= 64 pixels for ALL K_d output channels of the block end, walks
// them in chunks of 64 channels, and feeds each finished chunk of codes - still in LDS - to the second reduction as one K
// step.  The wide code tensor is never read (and, inside a stage, never written); the second layer's MFMA work runs in
// the shadow of the first layer's shortcut stream.
//
// Structure (256 threads = 2 x 2 waves: wave (wr, wc) owns rows wr*32.. and the column half wc):
//   * A (the block-end input, <= 64 rows x C1 <= 256 B) is loaded ONCE into registers as MFMA fragments;
//   * per chunk n: W1[n] (64 x C1), W3[:, n] (KB x 64) and the chunk's per-channel constants arrive by LDS-DMA into a
//     double buffer, the chunk's shortcut tile by asm buffer loads into registers - all requested one chunk ahead; one
//     counted s_waitcnt + one barrier, GEMM 1 (C1/32 MFMAs), epilogue 1 in registers (dequantise, 4x4 DPP transpose
//     from the accumulator layout to rows of 4 consecutive channels, + shortcut, ReLU, 16-byte buffer stores, quantise),
//     codes -> LDS, barrier, GEMM 2 step (KB/32 MFMAs into the resident second accumulator);
//   * buffer instructions with the row guard folded into the offset (out-of-range lanes are dropped by the hardware), so
//     every wave issues the same number of vector-memory instructions and the vmcnt arithmetic is exact.
#include "conv_i8_common.h"

namespace dlmcq {

struct ChainArgs {
  // GEMM 1: block end.  x codes [M][C1], w [KD][C1] int8, per-channel scale / code sum / bias [KD]
  ChainOp o1;
  int shift1;
  const float* residual;   // fp32 [M][KD] (required unless the shortcut is a convolution: C2 > 0)
  // the shortcut as a second 1x1 convolution into the same tile (C2 > 0; the block's downsample): x codes [N][H2][W2][C2]
  // sampled at (p * stride2, q * stride2), w [KD][C2]
  ChainOp o2;
  int shift2, P, Q, H2, W2, stride2;
  FastDiv qdiv, pdiv;
  // the shortcut RECOMPUTED (CA > 0; the second block of a stage): it is the output relu?(conv1x1(xa, wa) + conv1x1(xb sampled, wb)) of the
  // stage's first, convolution-shortcut block, whose operands are handed over instead of its fp32 tensor.  The sampled operand (xb, wb, ...)
  // travels in o2 above, the unit-stride one here: x codes [M][CA], w [KD][CA]
  ChainOp oa;
  int shifta, relu_sc;
  float* out;              // fp32 [M][KD] or null
  uint8_t* codes;          // [M][KD] or null
  // GEMM 2: the next 1x1 reduction.  w3 [KB][KD] int8; its input quantiser is ep1's (scale, zero point)
  const int8_t* w3;
  const float* s_w3;
  const int32_t* wsum3;
  const float* bias3;
  uint8_t* codes2;         // [M][KB]
  int w3_row, w3_chunk;    // byte strides of w3: from output channel to output channel, from 64-column chunk to chunk (KRSC: KD, 64; chunk-major: 64, KB * 64)
  int M, KD, rows_per_tile;
  // layout of the two fp32 tensors - f_: the shortcut read, o_: the block output written - as fp32 elements from row to row / bytes
  // from 64-channel chunk to chunk.  Row-major [M][KD]: KD, 256.  Chunk-major [KD / 64][M][64] (DLMCQ_FP32_*_CHUNK_MAJOR): 64, M * 256
  int f_rowq, f_cstep, o_rowq, o_cstep;
  int lab;                     // lab builds: 1 = no shortcut loads (timing only)
  unsigned long long* trace;   // lab builds: 64 clock-stamp slots per workgroup (null: none)
};
// (the kernel's scalar argument loads stay where they were when the three operands were spelt field by field)
static_assert(sizeof(ChainOp) == 56 && offsetof(ChainArgs, residual) == 64 && offsetof(ChainArgs, P) == 132 && offsetof(ChainArgs, relu_sc) == 236 &&
              offsetof(ChainArgs, out) == 240 && offsetof(ChainArgs, w3) == 256 && offsetof(ChainArgs, M) == 304 &&
              offsetof(ChainArgs, f_rowq) == 316 && sizeof(ChainArgs) == 344, "ChainArgs: a field moved");

template <int CTRL>
__device__ __forceinline__ float quad_dpp(float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, v), CTRL, 0xf, 0xf, true));   // (every lane reads a live lane: no `old` value to initialise)
}
// 4 x 4 transpose across the four lanes of a quad: afterwards x_j of lane b is what x_b of lane j was
__device__ __forceinline__ void quad_transpose(float& x0, float& x1, float& x2, float& x3, bool b0, bool b1) {
  const float x0s = quad_dpp<0xB1>(x0), x1s = quad_dpp<0xB1>(x1), x2s = quad_dpp<0xB1>(x2), x3s = quad_dpp<0xB1>(x3);
  const float n0 = b0 ? x1s : x0, n1 = b0 ? x1 : x0s, n2 = b0 ? x3s : x2, n3 = b0 ? x3 : x2s;
  const float n0s = quad_dpp<0x4E>(n0), n1s = quad_dpp<0x4E>(n1), n2s = quad_dpp<0x4E>(n2), n3s = quad_dpp<0x4E>(n3);
  x0 = b1 ? n2s : n0;
  x2 = b1 ? n2 : n0s;
  x1 = b1 ? n3s : n1;
  x3 = b1 ? n3 : n1s;
}

// workgroups per CU the kernel is compiled for (registers), by instantiation
constexpr int CHAIN_WGS(int c1, int kb) { return c1 + kb <= 256 ? 3 : 2; }
constexpr int CH_BIG = 0x7fff0000;   // a byte offset beyond every buffer this kernel accepts (< 2^31 - 64 KiB)

// FL (round 4): what the first epilogue does, known at compile time - bit 0: ReLU, bit 1: the fp32 output is stored; -1: both read
// from the arguments at run time (the general form; the plan's launches are all ReLU ones).  A run-time flag is a uniform branch per
// group of 4 values - five per group with the quantiser's, each a bubble in a wave's issue and a basic-block boundary the scheduler
// cannot move work across.
// CA, CB (round 6): the shortcut is neither loaded nor a convolution of this block but the PREVIOUS block's output, recomputed per chunk from
// that block's two code operands (CA, CB channels; C2 = 0) with the convolution-shortcut form's own instructions in its own order - the
// same fp32 values bit for bit, for 2 x 64 B of codes per pixel instead of 1 KB of fp32 (LABNOTES 17)
template <int C1, int KB, int C2 = 0, int FL = -1, int CA = 0, int CB = 0>
__global__ __launch_bounds__(256, CHAIN_WGS(C1 + C2 + CA + CB, KB)) void conv_chain_i8_kernel(ChainArgs a, ConvEpi ep1, ConvEpi ep2) {
  constexpr bool DUALH = C2 > 0;         // the shortcut is a second convolution (no fp32 shortcut tensor)
  constexpr bool RC = CA > 0;            // the shortcut is recomputed from the previous block's operands (no fp32 shortcut tensor)
  static_assert(!RC || (C2 == 0 && CB > 0 && FL >= 0), "the recomputing form: two operands, no convolution shortcut of its own, flags known");
  constexpr int SA = CA / 64, SB = CB / 64;   // K steps of the two recomputed reductions
  constexpr int W3U = C1 / 64 + C2 / 64 + SA + SB;   // the 4 KB unit of a chunk's weights at which W3's piece starts
  const bool relu1 = FL < 0 ? ep1.relu != 0 : (FL & 1) != 0;
  const bool out1 = FL < 0 ? a.out != nullptr : (FL & 2) != 0;
  constexpr int S1 = C1 / 64;            // K steps of GEMM 1
  constexpr int S2 = C2 / 64;            // K steps of the shortcut convolution
  constexpr int U3 = KB / 64;            // 64-row units of a W3 chunk = accumulator slabs of GEMM 2 per wave (KB/2 columns)
  constexpr int WCH = (W3U + U3) * 4096;  // bytes of one chunk's weights: W1 | W2 | Wa | Wb | W3
  constexpr int NPD = DUALH ? 2 : RC ? 3 : 1;     // constant-table DMAs per wave per chunk
  constexpr int PAR = NPD * 4 * 256;     // per-channel constants of one chunk ((scale, code sum, bias) per pair) x 64 columns
  // How the accumulator layout (lane = channel, register = row) becomes rows of 4 consecutive channels per lane (TF):
  //   0  two DPP exchange rounds inside each quad (8 v_mov_dpp + 8 v_cndmask per 4 values).  The quad structure then dictates which
  //      lane owns which row: 4 adjacent lanes = 4 rows, so a 16-lane group of a shortcut load / output store touches 4 rows x 64 B;
  //   1  a wave-private 1 KB LDS stage per group of 8 rows (4 ds_write_b32 + 1 ds_read_b128; LDS operations of one wave execute in
  //      order, so neither a barrier nor a wait separates the writes from the read), same lane -> row mapping as 0: a quarter fewer
  //      vector instructions and NO gain (round 3: every chain within +-1 %) - the kernel is not bound by their count;
  //   2  the same stage read back with 8 adjacent lanes = one row's 128 bytes: a 16-lane group of a load / store now touches 2 WHOLE
  //      128-byte lines.  That is what the fp32 streams respond to (round 2's timing build with 256-byte rows said so): same box, in
  //      the plan, 56^2 chains -3 .. -7 %, 28^2 -3 .. -5 %, 14^2 -2 %; the 28^2 convolution-shortcut chain (no shortcut loads, LDS
  //      nearly full) +3 %, so it keeps form 0.  Bit-identical in all forms.
#ifndef DLMCQ_CHAIN_LDS_T
#define DLMCQ_CHAIN_LDS_T ((C1 == 128 && C2 == 256) ? 0 : 2)
#endif
  constexpr int TF = DLMCQ_CHAIN_LDS_T;
  constexpr bool LDST = TF != 0;
#ifdef DLMCQ_LAB
  // lab builds of the shapes with LDS to spare carry a 16 KB landing area for the timing-only variant `lab & 0x800` (round 5: the
  // shortcut tile by LDS-DMA instead of loads into registers - does the stream itself move differently?  56^2 mid-stage -1.7 %, 56^2
  // stage end +3.5 %: no.  LABNOTES 14)
  constexpr int LABDMA = (C2 == 0 && C1 == 64) ? 16384 : 0;
#else
  constexpr int LABDMA = 0;
#endif
  __shared__ __attribute__((aligned(1024))) int8_t lds[2 * WCH + 2 * PAR + 4096 + 3 * KB * 4 + (LDST ? 4096 : 0) + LABDMA];
  int8_t* const par0 = lds + 2 * WCH;
  int8_t* const ctile = lds + 2 * WCH + 2 * PAR;
  int8_t* const par3 = ctile + 4096;     // GEMM 2's per-channel constants, ready-made: s_in * s_w[k] | (128 - zp) * SUM qw[k] | bias[k]
  float* const tstage = reinterpret_cast<float*>(par3 + 3 * KB * 4) + (threadIdx.x >> 6) * 256;   // this wave's 8 rows x 32 channels

  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, l31 = lane & 31, hsel = lane >> 5;
  const int wr = wave >> 1, wc = wave & 1;
  // the lane's place in the row-major (transposed) form of a group of 8 rows x 32 channels: row `rsel`, channels 4 q4 .. 4 q4 + 3
  constexpr bool LDST2 = TF == 2;
  const int q4 = LDST2 ? (lane & 7) : (l31 >> 2), b4 = l31 & 3;
  const int rsel = LDST2 ? (lane >> 3) : (4 * hsel + b4);
  const bool b0 = (lane & 1) != 0, b1 = (lane & 2) != 0;
  const int64_t row0 = (int64_t)blockIdx.x * a.rows_per_tile;
  const int rows_here = (int)((a.M - row0) < a.rows_per_tile ? (a.M - row0) : a.rows_per_tile);
  const int NC = a.KD >> 6;
#ifndef DLMCQ_CHAIN_ROT
#define DLMCQ_CHAIN_ROT 0
#endif
  // -DDLMCQ_CHAIN_ROT=1 (A/B builds; round 5): workgroup b walks its chunks starting at chunk b mod NC - are all workgroups on the same
  // quarter of the channels at once?  GEMM 2's integer sum does not care about the order: bit-identical, and +-0 (LABNOTES 16)
  const int rot = DLMCQ_CHAIN_ROT ? (int)(blockIdx.x % (unsigned)NC) : 0;
  auto cn = [&](int n) { const int m = n + rot; return m >= NC ? m - NC : m; };
#ifdef DLMCQ_LAB
  unsigned long long* const tr = (a.trace && tid == 0) ? a.trace + 64 * (size_t)blockIdx.x : nullptr;
  int trn = 0;
#define CHAIN_STAMP() do { if (tr && trn < 56) tr[trn++] = __builtin_readcyclecounter(); } while (0)
#define CHAIN_FINE(k) do { if (tr && nseq == 1) tr[56 + (k)] = __builtin_readcyclecounter(); } while (0)   // chunk 1 in detail (tools/chain_trace.py)
#else
#define CHAIN_STAMP() do { } while (0)
#define CHAIN_FINE(k) do { } while (0)
#endif
  CHAIN_STAMP();   // 0: start
#ifdef DLMCQ_LAB
  // timing only (round 5): are the chip's workgroups in lockstep?  Workgroups of the FIRST round start late - 0x200: the second
  // workgroup of a CU (blockIdx 256 .. 511) by `lab >> 16` units of 64 clocks; 0x400: every workgroup by a hashed 0 .. 15 sixteenths
  // of that (later rounds inherit the offsets: a slot's next tile starts when its last one ends).  Measured: -1 .. -4 % at best (LABNOTES 14)
  if ((a.lab & 0x600) && blockIdx.x < 512) {
    const int unit = a.lab >> 16;
    const int d = (a.lab & 0x200) ? ((blockIdx.x >> 8) & 1) * unit : (int)(((blockIdx.x * 2654435761u) >> 28) * (uint32_t)unit) >> 4;
    for (int i = 0; i < d; ++i) __builtin_amdgcn_s_sleep(1);
  }
#endif

  // ---- The tile's input rows (rows beyond the tile read its last row: never stored) go to LDS by LDS-DMA, 16 rows x 64 B per
  // wave-instruction, into buffer 1 of the weight double buffer - in W1's (W2's) own unit layout and swizzle, so the fragment
  // reads below are GEMM 1's weight-fragment reads with another base.  (Round 3: the fragments used to be loaded straight into
  // registers, 16 bytes per lane from 32 different rows per instruction - the costliest shape a vector-memory instruction
  // can have here - and twice over, once per column wave; in the short chains that was a quarter of a tile's requests.) ----
  {
    const int lrw = tid >> 2;                                 // = wave * 16 + (lane >> 2): the row of a 64-row unit this lane fetches
    const int sgw = ((tid & 3) ^ ((lrw >> 2) & 3)) * 16;
    const int8_t* xp = a.o1.x + (row0 + (lrw < rows_here ? lrw : rows_here - 1)) * C1 + sgw;
#pragma unroll
    for (int s = 0; s < S1; ++s)
      __builtin_amdgcn_global_load_lds((gptr_t)(xp + s * 64), (lptr_t)(lds + WCH + s * 4096 + (tid >> 6) * 1024), 16, 0, 0);
    if constexpr (DUALH) {
      const uint32_t m = (uint32_t)(row0 + (lrw < rows_here ? lrw : rows_here - 1));
      const uint32_t t = fdiv(m, a.qdiv), nn = fdiv(t, a.pdiv);
      const int q = (int)(m - t * (uint32_t)a.Q), pp = (int)(t - nn * (uint32_t)a.P);
      const int8_t* xp2 = a.o2.x + (((int64_t)nn * a.H2 + pp * a.stride2) * a.W2 + q * a.stride2) * C2 + sgw;
#pragma unroll
      for (int s = 0; s < S2; ++s)
        __builtin_amdgcn_global_load_lds((gptr_t)(xp2 + s * 64), (lptr_t)(lds + WCH + (S1 + s) * 4096 + (tid >> 6) * 1024), 16, 0, 0);
    }
    if constexpr (RC) {      // the previous block's operands: xa row for row like x, xb sampled like the convolution shortcut's x2
      const int8_t* xpa = a.oa.x + (row0 + (lrw < rows_here ? lrw : rows_here - 1)) * CA + sgw;
#pragma unroll
      for (int s = 0; s < SA; ++s)
        __builtin_amdgcn_global_load_lds((gptr_t)(xpa + s * 64), (lptr_t)(lds + WCH + (S1 + s) * 4096 + (tid >> 6) * 1024), 16, 0, 0);
      const uint32_t m = (uint32_t)(row0 + (lrw < rows_here ? lrw : rows_here - 1));
      const uint32_t t = fdiv(m, a.qdiv), nn = fdiv(t, a.pdiv);
      const int q = (int)(m - t * (uint32_t)a.Q), pp = (int)(t - nn * (uint32_t)a.P);
      const int8_t* xpb = a.o2.x + (((int64_t)nn * a.H2 + pp * a.stride2) * a.W2 + q * a.stride2) * CB + sgw;
#pragma unroll
      for (int s = 0; s < SB; ++s)
        __builtin_amdgcn_global_load_lds((gptr_t)(xpb + s * 64), (lptr_t)(lds + WCH + (S1 + SA + s) * 4096 + (tid >> 6) * 1024), 16, 0, 0);
    }
  }
  // GEMM 2's epilogue constants, once per workgroup (its accumulator is kept with the operands swapped - weights as A, the
  // code tile as B - so a lane owns 16 consecutive channels of one pixel and reads their constants as broadcast ds_read_b128)
  const float sin2 = ep1.q_scale[0];                       // GEMM 2's input scale IS the quantiser the codes were made with
  const float zpf2 = ep1.q_zp ? ep1.q_zp[0] : 0.0f;
  const int dz2 = 128 - (int)__builtin_rintf(zpf2);
  if (tid < KB) {
    reinterpret_cast<float*>(par3)[tid] = sin2 * a.s_w3[tid];
    reinterpret_cast<int*>(par3)[KB + tid] = dz2 * a.wsum3[tid];
    reinterpret_cast<float*>(par3)[2 * KB + tid] = a.bias3 ? a.bias3[tid] : 0.0f;
  }
  // the input tile has landed, and no compiler-known load is outstanding from here on (the counted waits below assume it)
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_barrier" ::: "memory");
  i32x4 af[S1][2];
  i32x4 af2[DUALH ? S2 : 1][2];
  i32x4 afa[RC ? SA : 1][2], afb[RC ? SB : 1][2];   // the recomputed reductions' A fragments: once per tile, like af2
  {
    const int r = wr * 32 + l31;
    const int8_t* ab = lds + WCH + r * 64;
    const uint32_t xw = a.shift1 ? 0x80808080u : 0u;
#pragma unroll
    for (int s = 0; s < S1; ++s)
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        const i32x4 t = *reinterpret_cast<const i32x4*>(ab + s * 4096 + (((ks * 2 + hsel) ^ ((r >> 2) & 3)) << 4));
        af[s][ks] = i32x4{(int)(t.x ^ xw), (int)(t.y ^ xw), (int)(t.z ^ xw), (int)(t.w ^ xw)};
      }
    if constexpr (DUALH) {
      const uint32_t xw2 = a.shift2 ? 0x80808080u : 0u;
#pragma unroll
      for (int s = 0; s < S2; ++s)
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
          const i32x4 t = *reinterpret_cast<const i32x4*>(ab + (S1 + s) * 4096 + (((ks * 2 + hsel) ^ ((r >> 2) & 3)) << 4));
          af2[s][ks] = i32x4{(int)(t.x ^ xw2), (int)(t.y ^ xw2), (int)(t.z ^ xw2), (int)(t.w ^ xw2)};
        }
    }
    if constexpr (RC) {
      const uint32_t xwa = a.shifta ? 0x80808080u : 0u, xwb = a.shift2 ? 0x80808080u : 0u;
#pragma unroll
      for (int s = 0; s < SA; ++s)
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
          const i32x4 t = *reinterpret_cast<const i32x4*>(ab + (S1 + s) * 4096 + (((ks * 2 + hsel) ^ ((r >> 2) & 3)) << 4));
          afa[s][ks] = i32x4{(int)(t.x ^ xwa), (int)(t.y ^ xwa), (int)(t.z ^ xwa), (int)(t.w ^ xwa)};
        }
#pragma unroll
      for (int s = 0; s < SB; ++s)
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
          const i32x4 t = *reinterpret_cast<const i32x4*>(ab + (S1 + SA + s) * 4096 + (((ks * 2 + hsel) ^ ((r >> 2) & 3)) << 4));
          afb[s][ks] = i32x4{(int)(t.x ^ xwb), (int)(t.y ^ xwb), (int)(t.z ^ xwb), (int)(t.w ^ xwb)};
        }
    }
  }
  // (the fragments are in registers before this wave reaches chunk 0's barrier, behind which buffer 1 is requested for chunk 1)
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  CHAIN_STAMP();   // 1: A fragments in registers

  // ---- addressing of the fp32 tile in the transposed (row-major) layout: group g -> row wr*32 + 8g + 4 hsel + b4 ----
  const uint32_t fbytes = (uint32_t)((int64_t)a.M * a.KD * 4);
  const v4i r_res = make_rsrc(a.residual, fbytes);
  const v4i r_out = make_rsrc(a.out ? (const void*)a.out : (const void*)a.residual, a.out ? fbytes : 0u);
  const v4i r_cod = make_rsrc(a.codes ? (const void*)a.codes : (const void*)a.residual, a.codes ? fbytes / 4 : 0u);
  int fo[4];     // byte offset of this lane's 16 bytes in chunk 0, per group (CH_BIG: row not in the tile)
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    const int lr = wr * 32 + 8 * g + rsel;
    fo[g] = lr < rows_here ? (int)(((row0 + lr) * a.f_rowq + wc * 32 + q4 * 4) * 4) : CH_BIG;
#ifdef DLMCQ_LAB
    if (a.lab & 4) {   // timing only: the access pattern a 16 x 16 x 64 accumulator layout would have - 16 rows x 64 bytes per instruction
      const int lr2 = wr * 32 + 16 * (g >> 1) + 2 * (4 * hsel + b4) + (q4 >> 2);
      fo[g] = lr2 < rows_here ? (int)(((row0 + lr2) * a.KD + wc * 32 + 16 * (g & 1) + (q4 & 3) * 4) * 4) : CH_BIG;
    }
    if (a.lab & 8) {   // timing only: 4 rows x 256 bytes per instruction (a wave owning 16 rows x 64 channels)
      const int lr3 = wr * 32 + wc * 16 + 4 * g + (lane >> 4);
      fo[g] = lr3 < rows_here ? (int)(((row0 + lr3) * a.KD + (lane & 15) * 4) * 4) : CH_BIG;
    }
#endif
  }
  int cstep = a.f_cstep; // byte distance between a row's consecutive 64-channel chunks
#ifdef DLMCQ_LAB
  if (a.lab & 64) {      // timing only: the fp32 tensors in 64 x 64 blocks (every chunk of a tile one contiguous 16 KB)
    cstep = 64 * 256;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int lr = wr * 32 + 8 * g + rsel;
      fo[g] = lr < rows_here ? (int)(row0 * a.KD * 4 + lr * 256 + (wc * 32 + q4 * 4) * 4) : CH_BIG;
    }
  }
#endif
  // the output's offsets: the shortcut's, unless the two tensors differ in layout (one row-major, one chunk-major: a chain between a
  // kernel that does not know the chunk-major form and one that does).  The instantiation that sits at its register limit has no room
  // for a second set: chain_launch refuses mixed layouts for it.
  constexpr bool MIXED_OK = !DUALH && !RC && !(C1 == 128 && KB == 128);
  int fo2[MIXED_OK ? 4 : 1];
  const int cstep2 = a.o_cstep;
  if constexpr (MIXED_OK) {
    const bool same = a.o_rowq == a.f_rowq;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int lr = wr * 32 + 8 * g + rsel;
      fo2[g] = same ? fo[g] : (lr < rows_here ? (int)(((row0 + lr) * a.o_rowq + wc * 32 + q4 * 4) * 4) : CH_BIG);
    }
  }
  auto out_off = [&](int g, int n) {
    if constexpr (MIXED_OK) return fo2[g] + n * cstep2;
    else return fo[g] + n * cstep;
  };
  // transposition stage: row 4 hsel + j of a group holds this lane's register 4 g + j at column l31; a lane reads back row
  // 4 hsel + b4, columns 4 q4 .. + 3; 4-column slot c of row r sits at slot c ^ (r & 7)
  int tw[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) tw[j] = (4 * hsel + j) * 32 + (LDST2 ? l31 : ((l31 & 3) | ((l31 & ~3) ^ ((4 * hsel + j) * 4))));
  const int trd = LDST2 ? rsel * 32 + 4 * q4 : (4 * hsel + b4) * 32 + ((4 * q4) ^ ((4 * hsel + b4) * 4));   // (form 2: 8 lanes read one row = all 32 banks: no swizzle needed)
  const int nst = (out1 ? 4 : 0) + (a.codes ? 1 : 0);   // stores per wave per chunk

  // ---- DMA sources.  A wave-instruction lands 16 rows x 64 B; row r of a unit keeps its 16-byte segments XOR-swizzled ----
  const int lrow = lane >> 2, pslot = lane & 3;
  const int drow = wave * 16 + lrow;                       // row of a 64-row unit this lane fetches
  const int dseg = (pslot ^ ((drow >> 2) & 3)) * 16;
  const int8_t* w1p = a.o1.w + (int64_t)drow * C1 + dseg;    // + chunk * 64 * C1 + s * 64
  // W3's rows are dealt to the LDS rows so that accumulator register i of GEMM 2 (weights as the A operand) is channel
  // 16 hsel + i of its 32-channel block: LDS row d of a block holds channel 16 ((d >> 2) & 1) + 4 (d >> 3) + (d & 3)
  const int d3 = drow & 31;
  const int prow3 = (drow & 32) + 16 * ((d3 >> 2) & 1) + 4 * (d3 >> 3) + (d3 & 3);
  const int8_t* w3p = a.w3 + (int64_t)prow3 * a.w3_row + dseg;  // + unit * 64 * w3_row + chunk * w3_chunk
  const int cvo = drow < rows_here ? (int)((row0 + drow) * a.KD + dseg) : CH_BIG;   // this lane's 16 bytes of the code tile, chunk 0
  const void* const pars[4] = {a.o1.s_w, a.o1.wsum, a.o1.bias ? (const void*)a.o1.bias : (const void*)a.o1.s_w, a.o1.s_w};
  const int32_t* parp = static_cast<const int32_t*>(wave == 0 ? pars[0] : wave == 1 ? pars[1] : wave == 2 ? pars[2] : pars[3]) + lane;
  const int8_t* w2p = DUALH ? a.o2.w + (int64_t)drow * C2 + dseg : nullptr;
  const void* const pars2[4] = {a.o2.s_w, a.o2.wsum, a.o2.bias ? (const void*)a.o2.bias : (const void*)a.o2.s_w, a.o2.s_w};
  const int32_t* parp2 = static_cast<const int32_t*>(wave == 0 ? pars2[0] : wave == 1 ? pars2[1] : wave == 2 ? pars2[2] : pars2[3]) + lane;
  // the recomputed shortcut's weights and tables: Wa in units S1.., Wb behind it; tables 1 (a) and 2 (b) of the chunk's NPD = 3
  const int8_t* wap = RC ? a.oa.w + (int64_t)drow * CA + dseg : nullptr;
  const int8_t* wbp = RC ? a.o2.w + (int64_t)drow * CB + dseg : nullptr;
  const void* const parsa[4] = {a.oa.s_w, a.oa.wsum, a.oa.bias ? (const void*)a.oa.bias : (const void*)a.oa.s_w, a.oa.s_w};
  const int32_t* parpa = static_cast<const int32_t*>(wave == 0 ? parsa[0] : wave == 1 ? parsa[1] : wave == 2 ? parsa[2] : parsa[3]) + lane;

  f32x4 res[2][4];
#ifdef DLMCQ_LAB
  if (a.lab & 0x801)
    for (auto& r2 : res)
      for (auto& r : r2) r = f32x4{1.0f, 2.0f, 3.0f, 4.0f};
#endif
  auto request = [&](int nseq, auto par_c) {    // everything the nseq-th chunk of this workgroup's walk needs from memory
    constexpr int P = decltype(par_c)::value;
    const int n = cn(nseq);
    int8_t* wb = lds + P * WCH;
    bool wdma = true;
#ifdef DLMCQ_LAB
    // timing only: no weight DMA on odd chunks (16: what a tile of twice the pixels would request per output) / at all (32)
    wdma = !(((a.lab & 16) && (n & 1)) || (a.lab & 32));
#endif
#pragma unroll
    for (int s = 0; s < S1; ++s)
      if (wdma) __builtin_amdgcn_global_load_lds((gptr_t)(w1p + (int64_t)n * 64 * C1 + s * 64), (lptr_t)(wb + s * 4096 + wave * 1024), 16, 0, 0);
#pragma unroll
    for (int u = 0; u < U3; ++u)
      if (wdma) {
        const int8_t* src = w3p + (int64_t)u * 64 * a.w3_row + (int64_t)n * a.w3_chunk;
        __builtin_amdgcn_global_load_lds((gptr_t)src, (lptr_t)(wb + (W3U + u) * 4096 + wave * 1024), 16, 0, 0);
      }
    __builtin_amdgcn_global_load_lds((gptr_t)(parp + n * 64), (lptr_t)(par0 + P * PAR + wave * 256), 4, 0, 0);
    if constexpr (DUALH) {
#pragma unroll
      for (int s = 0; s < S2; ++s)
        if (wdma) __builtin_amdgcn_global_load_lds((gptr_t)(w2p + (int64_t)n * 64 * C2 + s * 64), (lptr_t)(wb + (S1 + s) * 4096 + wave * 1024), 16, 0, 0);
      __builtin_amdgcn_global_load_lds((gptr_t)(parp2 + n * 64), (lptr_t)(par0 + P * PAR + 1024 + wave * 256), 4, 0, 0);
      return;      // no fp32 shortcut tile
    }
    if constexpr (RC) {
#pragma unroll
      for (int s = 0; s < SA; ++s)
        if (wdma) __builtin_amdgcn_global_load_lds((gptr_t)(wap + (int64_t)n * 64 * CA + s * 64), (lptr_t)(wb + (S1 + s) * 4096 + wave * 1024), 16, 0, 0);
#pragma unroll
      for (int s = 0; s < SB; ++s)
        if (wdma) __builtin_amdgcn_global_load_lds((gptr_t)(wbp + (int64_t)n * 64 * CB + s * 64), (lptr_t)(wb + (S1 + SA + s) * 4096 + wave * 1024), 16, 0, 0);
      __builtin_amdgcn_global_load_lds((gptr_t)(parpa + n * 64), (lptr_t)(par0 + P * PAR + 1024 + wave * 256), 4, 0, 0);
      __builtin_amdgcn_global_load_lds((gptr_t)(parp2 + n * 64), (lptr_t)(par0 + P * PAR + 2048 + wave * 256), 4, 0, 0);
      return;      // no fp32 shortcut tile
    }
#pragma unroll
    for (int g = 0; g < 4; ++g) {
#ifdef DLMCQ_LAB
      if (a.lab & 1) continue;
      if constexpr (LABDMA > 0) {
        if (a.lab & 0x800) {    // timing only: the same 16 bytes per lane, by LDS-DMA (nt) into the landing area; `res` keeps stale values
          const int lr = wr * 32 + 8 * g + rsel;
          const float* src = a.residual + (row0 + (lr < rows_here ? lr : rows_here - 1)) * a.KD + n * 64 + wc * 32 + q4 * 4;
          __builtin_amdgcn_global_load_lds((gptr_t)src, (lptr_t)(lds + sizeof(lds) - LABDMA + wave * 4096 + g * 1024), 16, 0, 2);
          continue;
        }
      }
#endif
      int lo = fo[g] + n * cstep;
#ifdef DLMCQ_LAB
      if (a.lab & 0x2000) lo &= 0xffff;
#endif
      bload16(res[P][g], lo, r_res);
    }
  };

  const float sin1 = a.o1.s_in[0];
  const float zpf1 = a.o1.zp_in ? a.o1.zp_in[0] : 0.0f;
  const int dz1 = a.shift1 - (int)__builtin_rintf(zpf1);
  const float sin1b = (DUALH || RC) ? a.o2.s_in[0] : 0.0f;
  const int dz1b = (DUALH || RC) ? a.shift2 - (int)__builtin_rintf(a.o2.zp_in ? a.o2.zp_in[0] : 0.0f) : 0;
  const float sin1a = RC ? a.oa.s_in[0] : 0.0f;
  const int dz1a = RC ? a.shifta - (int)__builtin_rintf(a.oa.zp_in ? a.oa.zp_in[0] : 0.0f) : 0;
  ConvEpi e1 = ep1;
  e1.codes = reinterpret_cast<uint8_t*>(uintptr_t(1));   // the quantiser is always needed (GEMM 2 reads its codes)
  // FL >= 0 also says: both quantisers are the plain unsigned-byte one (epi_plain_q; the launcher checks) - code4n_plain, whose
  // saturating pack is the ReLU as far as the codes are concerned
  const EpiQuant eq1(e1, FL >= 0);
  __builtin_assume(!eq1.sgn);                            // (the range is [0, 255]: chain_launch refuses anything else)

  i32x16 acc2[U3];
#pragma unroll
  for (int j = 0; j < U3; ++j)
#pragma unroll
    for (int i = 0; i < 16; ++i) acc2[j][i] = 0;

  request(0, std::integral_constant<int, 0>{});

  auto chunk = [&](int nseq, auto par_c) {
    constexpr int P = decltype(par_c)::value;
    const int n = cn(nseq);
    // chunk n's requests have landed; the stores of chunk n-1 (younger) stay in flight.  Then the barrier: everyone's DMA pieces are
    // visible; everyone left GEMM 2 of chunk n-1.  Wait and barrier are ONE asm statement with a memory clobber, so no LDS access can
    // be scheduled between them or moved across the barrier (a bare __builtin_amdgcn_s_barrier() does not touch memory for the compiler)
    if (nseq == 0 || nst == 0) asm volatile("s_waitcnt vmcnt(0)\n\ts_barrier" ::: "memory");
    else if (nst == 4) asm volatile("s_waitcnt vmcnt(4)\n\ts_barrier" ::: "memory");
    else if (nst == 5) asm volatile("s_waitcnt vmcnt(5)\n\ts_barrier" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(1)\n\ts_barrier" ::: "memory");
    CHAIN_STAMP();   // 2 + 3n: chunk n's operands are there
    if constexpr (!DUALH && !RC) asm volatile("" : "+v"(res[P][0]), "+v"(res[P][1]), "+v"(res[P][2]), "+v"(res[P][3]));
    if (nseq + 1 < NC) request(nseq + 1, std::integral_constant<int, 1 - P>{});

    const int8_t* wb = lds + P * WCH;
    const int8_t* pp = par0 + P * PAR + (wc * 32 + l31) * 4;
    i32x16 acc;
    // (round 5: the accumulators start from ZERO - the matrix instruction's inline constant, no register moves - and the column's constant
    //  (shift - zp) * SUM qw joins in fp32: |sum| <= 256 * 128 * 127 and |constant| <= 128 * 256 * 127, so both conversions and their sum are
    //  exact (< 2^24) and fma(float(sum) + float(constant), m, b) is fma(float(sum + constant), m, b) bit for bit; the chain runs on register
    //  PAIRS - v_pk_add_f32 / v_pk_fma_f32 -: 2 instructions per element where the integer form had 3)
    f32x2 extra2[DUALH ? 8 : 1];
    if constexpr (DUALH) {   // the shortcut convolution first: dequantised, it waits in registers for the block's own sum
      const float corr2f = (float)(dz1b * *reinterpret_cast<const int*>(pp + 1024 + 256));
#pragma unroll
      for (int i = 0; i < 16; ++i) acc[i] = 0;
      const int r = wc * 32 + l31;
#pragma unroll
      for (int s = 0; s < S2; ++s)
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
          const i32x4 bf = *reinterpret_cast<const i32x4*>(wb + (S1 + s) * 4096 + r * 64 + (((ks * 2 + hsel) ^ ((r >> 2) & 3)) << 4));
          acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(af2[s][ks], bf, acc, 0, 0, 0);
        }
      const float mult2 = sin1b * *reinterpret_cast<const float*>(pp + 1024);
      const float bv2 = a.o2.bias ? *reinterpret_cast<const float*>(pp + 1024 + 512) : 0.0f;
      const f32x2 c2{corr2f, corr2f}, m2{mult2, mult2}, b2{bv2, bv2};
#pragma unroll
      for (int i = 0; i < 8; ++i) extra2[i] = pk_fma(f32x2{(float)acc[2 * i], (float)acc[2 * i + 1]} + c2, m2, b2);
    }
    // the recomputed shortcut: the previous block's `deq(Wa . xa) + deq(Wb . xb)`, ReLU - the convolution-shortcut form's statements above
    // and in epilogue 1 below (sampled operand first, the same pk_fma, the same sum, relu4_nan), on the same accumulator layout: the value that
    // block stored.  It waits in registers, accumulator layout, where the fp32 form's `res` waits in the transposed one
    f32x2 sc2[RC ? 8 : 1];
    if constexpr (RC) {
      f32x2 eb[8];
      const int r = wc * 32 + l31;
      {
        const float corrbf = (float)(dz1b * *reinterpret_cast<const int*>(pp + 2048 + 256));
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[i] = 0;
#pragma unroll
        for (int s = 0; s < SB; ++s)
#pragma unroll
          for (int ks = 0; ks < 2; ++ks) {
            const i32x4 bf = *reinterpret_cast<const i32x4*>(wb + (S1 + SA + s) * 4096 + r * 64 + (((ks * 2 + hsel) ^ ((r >> 2) & 3)) << 4));
            acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(afb[s][ks], bf, acc, 0, 0, 0);
          }
        const float multb = sin1b * *reinterpret_cast<const float*>(pp + 2048);
        const float bvb = a.o2.bias ? *reinterpret_cast<const float*>(pp + 2048 + 512) : 0.0f;
        const f32x2 c2{corrbf, corrbf}, m2{multb, multb}, b2{bvb, bvb};
#pragma unroll
        for (int i = 0; i < 8; ++i) eb[i] = pk_fma(f32x2{(float)acc[2 * i], (float)acc[2 * i + 1]} + c2, m2, b2);
      }
      {
        const float corraf = (float)(dz1a * *reinterpret_cast<const int*>(pp + 1024 + 256));
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[i] = 0;
#pragma unroll
        for (int s = 0; s < SA; ++s)
#pragma unroll
          for (int ks = 0; ks < 2; ++ks) {
            const i32x4 bf = *reinterpret_cast<const i32x4*>(wb + (S1 + s) * 4096 + r * 64 + (((ks * 2 + hsel) ^ ((r >> 2) & 3)) << 4));
            acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(afa[s][ks], bf, acc, 0, 0, 0);
          }
        const float multa = sin1a * *reinterpret_cast<const float*>(pp + 1024);
        const float bva = a.oa.bias ? *reinterpret_cast<const float*>(pp + 1024 + 512) : 0.0f;
        const f32x2 c2{corraf, corraf}, m2{multa, multa}, b2{bva, bva};
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          f32x2 f = pk_fma(f32x2{(float)acc[2 * i], (float)acc[2 * i + 1]} + c2, m2, b2);
          sc2[i] = f + eb[i];
        }
      }
      if (a.relu_sc) {
#pragma unroll
        for (int i = 0; i < 8; i += 2) {
          const f32x4 t = relu4_nan(f32x4{sc2[i].x, sc2[i].y, sc2[i + 1].x, sc2[i + 1].y});
          sc2[i] = f32x2{t.x, t.y};
          sc2[i + 1] = f32x2{t.z, t.w};
        }
      }
    }
    // ---- GEMM 1: rows wr*32.., columns n*64 + wc*32.. ----
    const float corrf = (float)(dz1 * *reinterpret_cast<const int*>(pp + 256));
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0;
    {
      const int r = wc * 32 + l31;
#pragma unroll
      for (int s = 0; s < S1; ++s)
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
          const i32x4 bf = *reinterpret_cast<const i32x4*>(wb + s * 4096 + r * 64 + (((ks * 2 + hsel) ^ ((r >> 2) & 3)) << 4));
          acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(af[s][ks], bf, acc, 0, 0, 0);
        }
    }
#ifdef DLMCQ_LAB
    if (tr && nseq == 1) asm volatile("s_nop 0" ::"v"(acc[0]), "v"(acc[15]));   // (GEMM 1 retired)
#endif
    CHAIN_FINE(0);
    // ---- epilogue 1 ----
    const float mult = sin1 * *reinterpret_cast<const float*>(pp);
    const float bv = a.o1.bias ? *reinterpret_cast<const float*>(pp + 512) : 0.0f;
    float v[16];
    {
      const f32x2 c2{corrf, corrf}, m2{mult, mult}, b2{bv, bv};
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        f32x2 f = pk_fma(f32x2{(float)acc[2 * i], (float)acc[2 * i + 1]} + c2, m2, b2);
        if constexpr (DUALH) f = f + extra2[DUALH ? i : 0];     // `out += identity`, the identity being a convolution
        if constexpr (RC) f = f + sc2[RC ? i : 0];              // ... the identity being the previous block's output (what the fp32 form adds as `res`)
        v[2 * i] = f.x;
        v[2 * i + 1] = f.y;
      }
    }
    // GP groups of 8 rows share ONE tie branch of the quantiser (code4n): with the flags above known at compile time that branch is the
    // only basic-block boundary left in the epilogue, and the scheduler can run a group's LDS round trip under its neighbour's arithmetic
#ifndef DLMCQ_CHAIN_GP
#define DLMCQ_CHAIN_GP 4
#endif
    // (the two instantiations that sit at the 168 registers of three workgroups per CU keep the branch per group: more spills otherwise)
    constexpr bool TIGHT = C2 == 0 && ((C1 == 64 && KB == 128) || (C1 == 128 && KB == 128));
    constexpr int GP = (FL < 0 || TIGHT) ? 1 : DLMCQ_CHAIN_GP;
#pragma unroll
    for (int g0 = 0; g0 < 4; g0 += GP) {
      f32x4 y[GP];
#pragma unroll
      for (int k = 0; k < GP; ++k) {
        const int g = g0 + k;
        if constexpr (LDST) {
#pragma unroll
          for (int j = 0; j < 4; ++j) tstage[tw[j]] = v[4 * g + j];
          // (the read takes what OTHER lanes of this wave wrote: LDS operations of a wave execute in order, and the compiler must
          //  keep them in this order - a memory clobber between the writes and the read, and after the read, costs no instruction)
          asm volatile("" ::: "memory");
          y[k] = *reinterpret_cast<const f32x4*>(tstage + trd);
          asm volatile("" ::: "memory");
        } else {
          quad_transpose(v[4 * g], v[4 * g + 1], v[4 * g + 2], v[4 * g + 3], b0, b1);
          y[k] = f32x4{v[4 * g], v[4 * g + 1], v[4 * g + 2], v[4 * g + 3]};
        }
        if constexpr (!DUALH && !RC) y[k] = y[k] + res[P][g];
        if (relu1 && (FL < 0 || out1)) y[k] = relu4_nan(y[k]);      // (plain quantiser: only the fp32 output needs the rectified value)
#ifdef DLMCQ_LAB
        // timing only (round 5): 0x1000 - the fp32 stores land in a 64 KB window of the output (they stay in L2: what do the STORE INSTRUCTIONS cost
        // without their HBM traffic?); 0x2000 - the same for the shortcut loads (below)
        if (out1) bstore16(y[k], (a.lab & 0x1000) ? (out_off(g, n) & 0xffff) : out_off(g, n), r_out);
#else
        if (out1) bstore16(y[k], out_off(g, n), r_out);
#endif
      }
      uint32_t c[GP];
      if constexpr (FL >= 0) {
        eq1.code4n_plain(y, c);
      } else if constexpr (GP == 1) {
        c[0] = eq1.code4(y[0]);
      } else {
        bool un[GP];
        eq1.code4n(y, c, un);
      }
#pragma unroll
      for (int k = 0; k < GP; ++k) {
        const int R = wr * 32 + 8 * (g0 + k) + rsel;
        *reinterpret_cast<uint32_t*>(ctile + R * 64 + (((wc * 2 + (q4 >> 2)) ^ ((R >> 2) & 3)) << 4) + (q4 & 3) * 4) = c[k];
        CHAIN_FINE(1 + g0 + k);
      }
    }
    CHAIN_STAMP();   // 3 + 3n: GEMM 1 + epilogue 1 issued
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");     // the 64 x 64 code tile is complete
    CHAIN_STAMP();   // 4 + 3n: past the mid-chunk barrier
    if (a.codes)     // stage ends: the tile goes out 64 contiguous bytes per pixel (slot s of row r holds segment s ^ (r >> 2 & 3))
      bstore16i(*reinterpret_cast<const i32x4*>(ctile + drow * 64 + pslot * 16), cvo == CH_BIG ? CH_BIG : cvo + n * 64, r_cod);
    // ---- GEMM 2: one K step (this chunk's 64 channels) into the resident accumulator ----
    {
      const int R = wr * 32 + l31;
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        const i32x4 t = *reinterpret_cast<const i32x4*>(ctile + R * 64 + (((ks * 2 + hsel) ^ ((R >> 2) & 3)) << 4));
        const i32x4 a2 = i32x4{(int)(t.x ^ 0x80808080u), (int)(t.y ^ 0x80808080u), (int)(t.z ^ 0x80808080u), (int)(t.w ^ 0x80808080u)};
#pragma unroll
        for (int j = 0; j < U3; ++j) {
          const int kb = wc * (KB / 2) + j * 32 + l31;
          const i32x4 bf = *reinterpret_cast<const i32x4*>(wb + W3U * 4096 + kb * 64 + (((ks * 2 + hsel) ^ ((kb >> 2) & 3)) << 4));
          acc2[j] = __builtin_amdgcn_mfma_i32_32x32x32_i8(bf, a2, acc2[j], 0, 0, 0);
        }
      }
    }
  };
  for (int n = 0; n < NC; n += 2) {
    chunk(n, std::integral_constant<int, 0>{});
    if (n + 1 < NC) chunk(n + 1, std::integral_constant<int, 1>{});
  }

  CHAIN_STAMP();   // chunks done
  // ---- epilogue 2: the reduction layer's own dequantise, ReLU, its consumer's quantiser; codes only.  Lane (p = l31, hsel) holds
  // channels wc * KB/2 + 32 j + 16 hsel + 0..15 of pixel wr * 32 + p: no transposition, the ReLU folded into the quantiser's clamp
  // (code(relu(v)) = max(code(v), code(0))), 16 finished bytes per lane and block ----
  const EpiQuant eq2(ep2, ep2.relu != 0);
  const int lr2 = wr * 32 + l31;
#pragma unroll
  for (int j = 0; j < U3; ++j) {
    const int cb = wc * (KB / 2) + j * 32 + hsel * 16;
    f32x4 y[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const f32x4 mu = *reinterpret_cast<const f32x4*>(par3 + (cb + 4 * q) * 4);
      const i32x4 co = *reinterpret_cast<const i32x4*>(par3 + (KB + cb + 4 * q) * 4);
      const f32x4 bs = *reinterpret_cast<const f32x4*>(par3 + (2 * KB + cb + 4 * q) * 4);
      y[q] = f32x4{dequant1(acc2[j][4 * q] + co.x, mu.x, bs.x), dequant1(acc2[j][4 * q + 1] + co.y, mu.y, bs.y),
                   dequant1(acc2[j][4 * q + 2] + co.z, mu.z, bs.z), dequant1(acc2[j][4 * q + 3] + co.w, mu.w, bs.w)};
    }
    uint32_t wq[4];
    if constexpr (FL >= 0) {
      eq2.code4n_plain(y, wq);
    } else {
      bool uq[4];
      eq2.code4n(y, wq, uq);
    }
    if (lr2 < rows_here)
      *reinterpret_cast<i32x4*>(ep2.codes + (row0 + lr2) * KB + cb) = i32x4{(int)wq[0], (int)wq[1], (int)wq[2], (int)wq[3]};
  }
#ifdef DLMCQ_LAB
  if (tr) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    CHAIN_STAMP();   // end
    tr[63] = __builtin_amdgcn_s_getreg(4 | (31 << 11));   // HW_ID
  }
#endif
}

}  // namespace dlmcq

using namespace dlmcq;

#ifdef DLMCQ_LAB
static unsigned long long* g_chain_trace = nullptr;   // set by dlmcq_x_chain_trace (tools/chain_trace.py)
extern "C" void dlmcq_x_chain_trace(void* buf) { g_chain_trace = static_cast<unsigned long long*>(buf); }
static int g_chain_lab = 0;
extern "C" void dlmcq_x_chain_lab(int flags) { g_chain_lab = flags; }
#endif

// value -> kernel: one launcher per instantiation, and THE table of the instantiations there are - 7 rows x 3 forms of the first
// epilogue (FL = 3: ReLU + fp32 output, 1: ReLU, -1: read at run time), 21 + 2 kernels.  A null entry: no such kernel.
typedef void (*ChainGo)(dim3 grid, size_t dyn, hipStream_t st, const ChainArgs& a, const ConvEpi& ep1, const ConvEpi& ep2);
template <int C1, int KB, int C2, int FL, int CA, int CB>
static void chain_go(dim3 grid, size_t dyn, hipStream_t st, const ChainArgs& a, const ConvEpi& ep1, const ConvEpi& ep2) {
  hipLaunchKernelGGL((conv_chain_i8_kernel<C1, KB, C2, FL, CA, CB>), grid, dim3(256), dyn, st, a, ep1, ep2);
}
struct ChainVariant {
  int C1, KB, C2, CA, CB;
  ChainGo go[3];      // FL = 3, 1, -1
};
#define DLMCQ_CHAIN_ROW(C1, KB, C2) {C1, KB, C2, 0, 0, {chain_go<C1, KB, C2, 3, 0, 0>, chain_go<C1, KB, C2, 1, 0, 0>, chain_go<C1, KB, C2, -1, 0, 0>}}
static const ChainVariant CHAIN_TABLE[] = {
    // the recomputing form is built for the plan's launch alone: stage 1's second block, ReLU, plain quantisers (no run-time-flag form)
    {64, 64, 0, 64, 64, {chain_go<64, 64, 0, 3, 64, 64>, chain_go<64, 64, 0, 1, 64, 64>, nullptr}},
    DLMCQ_CHAIN_ROW(64, 64, 0), DLMCQ_CHAIN_ROW(64, 128, 0), DLMCQ_CHAIN_ROW(128, 128, 0), DLMCQ_CHAIN_ROW(128, 256, 0),
    DLMCQ_CHAIN_ROW(256, 256, 0),
    DLMCQ_CHAIN_ROW(64, 64, 64), DLMCQ_CHAIN_ROW(128, 128, 256),       // the convolution shortcut: ResNet-50's stages 1 and 2
};
#undef DLMCQ_CHAIN_ROW

// The table, for tests (absent from include/dlmcq.h): per row six integers - C1, KB, C2, CA, CB and a mask of the FL slots that exist
// (bit 0: FL = 3, bit 1: FL = 1, bit 2: FL = -1) -, in the table's order, up to `cap_rows` rows; returns how many rows there are
extern "C" int dlmcq_x_chain_variant_table(int32_t* rows, int cap_rows) {
  int n = 0;
  for (const ChainVariant& v : CHAIN_TABLE) {
    if (rows && n < cap_rows) {
      int32_t* r = rows + 6 * n;
      r[0] = v.C1; r[1] = v.KB; r[2] = v.C2; r[3] = v.CA; r[4] = v.CB;
      r[5] = (v.go[0] ? 1 : 0) | (v.go[1] ? 2 : 0) | (v.go[2] ? 4 : 0);
    }
    ++n;
  }
  return n;
}

// What chain_launch decides for a validated call, ONCE: the launch and the route query (DLMCQ_ROUTE_ONLY | DLMCQ_ROUTE_CHAIN_VARIANT) read
// this one record.
struct ChainPick {
  int row, slot;           // CHAIN_TABLE[row].go[slot]; slot 0 / 1 / 2: FL = 3 / 1 / -1
  int rows_per_tile;       // as passed, or the automatic rule's
  bool icm, ocm2;          // the resolved layouts of the fp32 shortcut read / block output written (chunk-major)
};
// ... as the route query's answer (include/dlmcq.h: tag | row << 16 | slot << 12 | rows per tile << 4 | ocm << 1 | icm)
static int chain_variant_answer(const ChainPick& k) {
  return DLMCQ_ROUTE_CHAIN_VARIANT_TAG | (k.row << 16) | (k.slot << 12) | (k.rows_per_tile << 4) | (k.ocm2 ? 2 : 0) | (k.icm ? 1 : 0);
}

static bool op_given(const ChainOp& p) { return p.x && p.w && p.wsum && p.s_in && p.s_w; }

// Validates the record - every refusal of every chain entry point, in one order - and launches.
static int chain_launch(const ChainCall& c) {
  const ChainOperand &o = c.own, &s = c.sampled, &u = c.unit;
  const bool res = (c.uses & CHAIN_RESIDUAL) != 0, smp = (c.uses & CHAIN_SAMPLED) != 0, unt = (c.uses & CHAIN_UNIT) != 0;
  const int64_t C = o.C, K = c.K, K2 = c.K2, C2 = (smp && !unt) ? s.C : 0, CA = unt ? u.C : 0, CB = unt ? s.C : 0;
  if (o.N < 0 || o.H < 1 || o.W < 1 || C < 1 || K < 1 || K2 < 1 || K % 64 != 0) return DLMCQ_EINVAL;
  if (unt && u.C < 1) return DLMCQ_EINVAL;
  if (smp && (s.H < 1 || s.W < 1 || s.C < 1 || s.stride < 1)) return DLMCQ_EINVAL;
  if (smp && ((s.H - 1) / s.stride + 1 != o.H || (s.W - 1) / s.stride + 1 != o.W)) return DLMCQ_EINVAL;   // every operand gives [N, H, W, K]
  if (unt && c.relu_shortcut == DLMCQ_ACT_RELU6) return DLMCQ_EINVAL;
  const int64_t M = o.N * o.H * o.W;
  if (M == 0) return DLMCQ_OK;
  const ConvEpi &ep1 = c.ep1, &ep2 = c.ep2;
  if (!op_given(o.p) || (smp && !op_given(s.p)) || (unt && !op_given(u.p)) || (res && !c.residual) || !c.second.w || !c.second.wsum ||
      !c.second.s_w || !ep2.codes || !ep1.q_scale || !ep2.q_scale)
    return DLMCQ_EINVAL;
  if (!aligned16(o.p.x) || !aligned16(o.p.w) || (smp && (!aligned16(s.p.x) || !aligned16(s.p.w))) ||
      (unt && (!aligned16(u.p.x) || !aligned16(u.p.w))) || !aligned16(c.second.w) || (res && !aligned16(c.residual)) ||
      (c.out && !aligned16(c.out)) || (ep1.codes && !aligned16(ep1.codes)) || !aligned16(ep2.codes))
    return DLMCQ_EALIGN;
  if (smp && (M >= (1ll << 31) || o.N * s.H * s.W * s.C >= (1ll << 40))) return DLMCQ_ERANGE;
  if (ep1.relu == DLMCQ_ACT_RELU6 || ep2.relu == DLMCQ_ACT_RELU6) return DLMCQ_EINVAL;     // (ReLU only)
  if (c.q_lo != 0 || c.q_hi != 255) return DLMCQ_EINVAL;   // GEMM 2 reads the codes as uint8 (shift 128)
  if (ep2.ctl & (DLMCQ_FORCE_TILED | DLMCQ_PIPELINED | DLMCQ_ROUTE_HALO_VARIANT | DLMCQ_ROUTE_HALO_ROWS | DLMCQ_ROUTE_PW_VARIANT)) return DLMCQ_EINVAL;   // (no other kernel here)
  if (((ep2.ctl & DLMCQ_ROUTE_ONLY) != 0) != c.which) return DLMCQ_EINVAL;   // (one route query: both bits, DLMCQ_ROUTE_CHAIN_VARIANT's; either alone is none)
  const bool w3cm = (c.layout & DLMCQ_W2_CHUNK_MAJOR) != 0, ocm = (c.layout & DLMCQ_FP32_OUT_CHUNK_MAJOR) != 0;
  // (a call without a shortcut tensor or without an output has ONE fp32 tensor: its layout is the call's)
  const bool icm = res ? (c.layout & DLMCQ_FP32_IN_CHUNK_MAJOR) != 0 : ocm;
  const bool ocm2 = c.out ? ocm : icm;
  if (icm != ocm2 && C == 128 && K2 == 128) return DLMCQ_EINVAL;   // (no registers for two offset sets there: conv_chain_i8_kernel)
  if (c.q2_lo > c.q2_hi || c.q2_lo < -128 || c.q2_hi > 255 || c.q2_hi - c.q2_lo > 255 || c.q_form < DLMCQ_FORM_EMULATE ||
      c.q_form > DLMCQ_FORM_SYMMETRIC || ep2.q_form < 0)
    return DLMCQ_EINVAL;
  if (M * K * 4 > (int64_t)CH_BIG) return DLMCQ_ERANGE;   // 32-bit buffer offsets
  // Tile height: 64 rows.  A chunk costs a workgroup the same time at 32 .. 64 rows (round 5, tools/chain_ab.py --rows: a 14^2 launch takes
  // 238 / 218 / 241 / 249 / 258 / 323 us at 64 / 56 / 49 / 48 / 40 / 32 rows, every other shape is fastest at 64), so shorter tiles only pay
  // where they keep a nearly empty last round from costing a whole tile's life: ResNet-50's 14^2 chains at batch 512 - 1 568 tiles on the
  // 512 slots of the two-workgroup instantiations, 3.06 rounds - run 3.5 rounds of 56-row tiles 8 % faster.  The rule: few rounds, the last
  // one less than an eighth full.
  ChainPick pick{};
  pick.icm = icm; pick.ocm2 = ocm2;
  int& rows_per_tile = pick.rows_per_tile;
  rows_per_tile = c.rows_per_tile;
  if (rows_per_tile <= 0) {
    const int64_t t64 = (M + 63) / 64, slots = 256 * CHAIN_WGS((int)(C + C2 + CA + CB), (int)K2);
    const int64_t full = t64 / slots, left = t64 % slots;
    rows_per_tile = (full >= 2 && full <= 4 && left > 0 && left * 8 < slots) ? 56 : 64;
  }
  if (rows_per_tile > 64) return DLMCQ_EINVAL;
  const int64_t tiles = (M + rows_per_tile - 1) / rows_per_tile;
  if (tiles >= (1ll << 31)) return DLMCQ_ERANGE;
  // the plan's launches end their first layer with a ReLU: those get the instantiation that knows its flags at compile time
  const int fl = (ep1.relu && epi_plain_q(ep1) && epi_plain_q(ep2)) ? (c.out ? 3 : 1) : -1;
  ChainGo go = nullptr;
  pick.slot = fl == 3 ? 0 : fl == 1 ? 1 : 2;
  for (const ChainVariant& v : CHAIN_TABLE)
    if (v.C1 == C && v.KB == K2 && v.C2 == C2 && v.CA == CA && v.CB == CB) {
      pick.row = (int)(&v - CHAIN_TABLE);
      go = v.go[pick.slot];
    }
  if (!go) return DLMCQ_EINVAL;
  if (c.which) return chain_variant_answer(pick);     // (the route query: everything validated, nothing launched)

  ChainArgs a{};
  a.o1 = o.p; a.shift1 = o.shift;
  a.residual = res ? c.residual : nullptr;
  if (smp) {
    a.o2 = s.p; a.shift2 = s.shift;
    a.P = (int)o.H; a.Q = (int)o.W; a.H2 = (int)s.H; a.W2 = (int)s.W; a.stride2 = s.stride;
    a.qdiv = make_fastdiv((uint32_t)o.W);
    a.pdiv = make_fastdiv((uint32_t)o.H);
  }
  if (unt) { a.oa = u.p; a.shifta = u.shift; a.relu_sc = c.relu_shortcut != 0; }
  a.out = c.out; a.codes = ep1.codes;
  a.w3 = c.second.w; a.s_w3 = c.second.s_w; a.wsum3 = c.second.wsum; a.bias3 = c.second.bias; a.codes2 = ep2.codes;
  a.w3_row = w3cm ? 64 : (int)K;
  a.w3_chunk = w3cm ? (int)K2 * 64 : 64;
  a.M = (int)M; a.KD = (int)K; a.rows_per_tile = rows_per_tile;
  a.f_rowq = pick.icm ? 64 : (int)K;
  a.f_cstep = pick.icm ? (int)M * 256 : 256;
  a.o_rowq = pick.ocm2 ? 64 : (int)K;
  a.o_cstep = pick.ocm2 ? (int)M * 256 : 256;
  size_t dyn = 0;
#ifdef DLMCQ_LAB
  a.trace = g_chain_trace;
  a.lab = g_chain_lab;
  dyn = (g_chain_lab & 128 ? 40960 : 0) + (g_chain_lab & 256 ? 81920 : 0);   // timing only: unused dynamic LDS = fewer workgroups per CU
#endif
  go(dim3((uint32_t)tiles), dyn, c.st, a, ep1, ep2);
  return launch_status();
}

// what every chain entry point ends with: the block's width and outputs, the first quantiser, the second layer and its quantiser
static void chain_tail(ChainCall& c, int64_t K, float* out, int32_t relu, void* codes, const float* q_scale, const float* q_zero_point,
                       int32_t q_lo, int32_t q_hi, int32_t q_form, float q_ste_g, const int8_t* w2, const float* bias2, const int32_t* wsum2,
                       const float* w_scale2, int64_t K2, int32_t relu2, void* codes2, const float* q2_scale, const float* q2_zero_point,
                       int32_t q2_lo, int32_t q2_hi, int32_t q2_form, float q2_ste_g, int32_t rows_per_tile, dlmcq_stream_t stream) {
  constexpr int32_t LAYOUT = DLMCQ_W2_CHUNK_MAJOR | DLMCQ_FP32_IN_CHUNK_MAJOR | DLMCQ_FP32_OUT_CHUNK_MAJOR;
  c.K = K; c.K2 = K2; c.out = out;
  c.second = ChainOp{nullptr, w2, w_scale2, wsum2, bias2, nullptr, nullptr};
  c.ep1 = make_epi(nullptr, relu, codes, q_scale, q_zero_point, q_lo, q_hi, q_form, q_ste_g);
  c.ep2 = make_epi(nullptr, relu2, codes2, q2_scale, q2_zero_point, q2_lo, q2_hi, q2_form & ~(LAYOUT | DLMCQ_ROUTE_CHAIN_VARIANT), q2_ste_g);
  c.which = (q2_form & DLMCQ_ROUTE_CHAIN_VARIANT) != 0;      // (this entry point's own bit: epi_set_form, everyone's, does not know it)
  c.q_lo = q_lo; c.q_hi = q_hi; c.q_form = q_form; c.q2_lo = q2_lo; c.q2_hi = q2_hi;
  c.layout = (uint32_t)(q2_form & LAYOUT);
  c.rows_per_tile = rows_per_tile;
  c.st = reinterpret_cast<hipStream_t>(stream);
}
// (the second layer is `2` in the ABI's argument names, `3` where the block has two operands of its own)
#define DLMCQ_CHAIN_TAIL(n)                                                                                                       \
  K, out, relu, codes, q_scale, q_zero_point, q_lo, q_hi, q_form, q_ste_g, w##n, bias##n, wsum##n, w_scale##n, K##n, relu##n, codes##n, \
      q##n##_scale, q##n##_zero_point, q##n##_lo, q##n##_hi, q##n##_form, q##n##_ste_g, rows_per_tile, stream

extern "C" int dlmcq_conv2d_i8_nhwc_chain(const void* x, const int8_t* w, float* out, const float* bias, const int32_t* wsum,
                                          const float* in_scale, const float* in_zero_point, const float* w_scale, int64_t M,
                                          int64_t C, int64_t K, int32_t x_is_unsigned, const float* residual, int32_t relu,
                                          void* codes, const float* q_scale, const float* q_zero_point, int32_t q_lo,
                                          int32_t q_hi, int32_t q_form, float q_ste_g, const int8_t* w2, const float* bias2,
                                          const int32_t* wsum2, const float* w_scale2, int64_t K2, int32_t relu2, void* codes2,
                                          const float* q2_scale, const float* q2_zero_point, int32_t q2_lo, int32_t q2_hi,
                                          int32_t q2_form, float q2_ste_g, int32_t rows_per_tile, dlmcq_stream_t stream) {
  ChainCall c{};
  c.uses = CHAIN_RESIDUAL;
  c.own = chain_operand(x, w, bias, wsum, in_scale, in_zero_point, w_scale, M, 1, 1, C, 1, x_is_unsigned);
  c.residual = residual;
  chain_tail(c, DLMCQ_CHAIN_TAIL(2));
  return chain_launch(c);
}

extern "C" int dlmcq_conv2d_i8_nhwc_dual_chain(const void* x, const int8_t* w, float* out, const float* bias, const int32_t* wsum,
                                               const float* in_scale, const float* in_zero_point, const float* w_scale, int64_t N,
                                               int64_t H, int64_t W, int64_t C, int64_t K, int32_t x_is_unsigned, const void* x2,
                                               const int8_t* w2, const float* bias2, const int32_t* wsum2, const float* in_scale2,
                                               const float* in_zero_point2, const float* w_scale2, int64_t H2, int64_t W2,
                                               int64_t C2, int32_t stride2, int32_t x2_is_unsigned, int32_t relu, void* codes,
                                               const float* q_scale, const float* q_zero_point, int32_t q_lo, int32_t q_hi,
                                               int32_t q_form, float q_ste_g, const int8_t* w3, const float* bias3,
                                               const int32_t* wsum3, const float* w_scale3, int64_t K3, int32_t relu3, void* codes3,
                                               const float* q3_scale, const float* q3_zero_point, int32_t q3_lo, int32_t q3_hi,
                                               int32_t q3_form, float q3_ste_g, int32_t rows_per_tile, dlmcq_stream_t stream) {
  ChainCall c{};
  c.uses = CHAIN_SAMPLED;
  c.own = chain_operand(x, w, bias, wsum, in_scale, in_zero_point, w_scale, N, H, W, C, 1, x_is_unsigned);
  c.sampled = chain_operand(x2, w2, bias2, wsum2, in_scale2, in_zero_point2, w_scale2, N, H2, W2, C2, stride2, x2_is_unsigned);
  chain_tail(c, DLMCQ_CHAIN_TAIL(3));
  return chain_launch(c);
}

extern "C" int dlmcq_conv2d_i8_nhwc_recompute_chain(
    const void* x, const int8_t* w, float* out, const float* bias, const int32_t* wsum, const float* in_scale, const float* in_zero_point,
    const float* w_scale, int64_t N, int64_t H, int64_t W, int64_t C, int64_t K, int32_t x_is_unsigned, const void* xa, const int8_t* wa,
    const float* biasa, const int32_t* wsuma, const float* in_scalea, const float* in_zero_pointa, const float* w_scalea, int64_t Ca,
    int32_t xa_is_unsigned, const void* xb, const int8_t* wb, const float* biasb, const int32_t* wsumb, const float* in_scaleb,
    const float* in_zero_pointb, const float* w_scaleb, int64_t Hb, int64_t Wb, int64_t Cb, int32_t strideb, int32_t xb_is_unsigned,
    int32_t relu_shortcut, int32_t relu, void* codes, const float* q_scale, const float* q_zero_point, int32_t q_lo, int32_t q_hi,
    int32_t q_form, float q_ste_g, const int8_t* w2, const float* bias2, const int32_t* wsum2, const float* w_scale2, int64_t K2,
    int32_t relu2, void* codes2, const float* q2_scale, const float* q2_zero_point, int32_t q2_lo, int32_t q2_hi, int32_t q2_form,
    float q2_ste_g, int32_t rows_per_tile, dlmcq_stream_t stream) {
  ChainCall c{};
  c.uses = CHAIN_UNIT | CHAIN_SAMPLED;
  c.own = chain_operand(x, w, bias, wsum, in_scale, in_zero_point, w_scale, N, H, W, C, 1, x_is_unsigned);
  c.unit = chain_operand(xa, wa, biasa, wsuma, in_scalea, in_zero_pointa, w_scalea, N, H, W, Ca, 1, xa_is_unsigned);
  c.sampled = chain_operand(xb, wb, biasb, wsumb, in_scaleb, in_zero_pointb, w_scaleb, N, Hb, Wb, Cb, strideb, xb_is_unsigned);
  c.relu_shortcut = relu_shortcut;
  chain_tail(c, DLMCQ_CHAIN_TAIL(2));
  return chain_launch(c);
}
