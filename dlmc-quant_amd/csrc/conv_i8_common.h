// Definitions shared by the int8 convolution translation units: the tiled kernel's device records and helpers, and the host-side call
// records: ConvCall, which conv_launch (conv_i8.hip) and the kernel families it routes to pass around, ChainCall (conv_chain_i8.hip),
// StemCall (conv_stem_i8.hip, conv_stem_pool7_i8.hip) and DwCall (conv_dw_i8.hip, conv_dwm_i8.hip).
// Not part of the ABI.
#pragma once

#include <type_traits>

#include "dlmcq_internal.h"
#include "conv_epilogue.h"

namespace dlmcq {

constexpr int CV_BM = 128;
constexpr int CV_BK = 64;
constexpr int CV_LD = CV_BK + 16;  // LDS row stride in bytes

struct ConvGeom {
  int N, H, W, C, K, R, S, stride, pad, dil, P, Q;
  int64_t M;          // N*P*Q (< 2^31)
  int nblk_m, nblk_n;
  FastDiv qdiv, pdiv; // row index -> (n, p, q) without 64-bit divisions
};

// output row m -> image n and the top-left input coordinate of its receptive field
__device__ __forceinline__ void row_origin(const ConvGeom& g, uint32_t m, int& n, int& h0, int& w0) {
  const uint32_t t = fdiv(m, g.qdiv);
  const int q = (int)(m - t * (uint32_t)g.Q);
  const uint32_t nn = fdiv(t, g.pdiv);
  const int p = (int)(t - nn * (uint32_t)g.P);
  n = (int)nn;
  h0 = p * g.stride - g.pad;
  w0 = q * g.stride - g.pad;
}

// output row m -> image n and output pixel (p, q): what a shortcut read at a pixel stride needs (the PADRES epilogue of conv_i8.hip)
__device__ __forceinline__ void row_npq(const ConvGeom& g, uint32_t m, int& n, int& p, int& q) {
  const uint32_t t = fdiv(m, g.qdiv);
  q = (int)(m - t * (uint32_t)g.Q);
  const uint32_t nn = fdiv(t, g.pdiv);
  p = (int)(t - nn * (uint32_t)g.P);
  n = (int)nn;
}

struct PadTable {   // 64 bytes of every byte value: a padded tap reads its K chunks at offsets 0 / 32 of one line
  int8_t b[256 * 64];
  constexpr PadTable() : b() {
    for (int v = 0; v < 256; ++v)
      for (int j = 0; j < 64; ++j) b[v * 64 + j] = (int8_t)v;
  }
};
static __device__ const PadTable g_pad_table = PadTable();

typedef const __attribute__((address_space(1))) void* gptr_t;
typedef __attribute__((address_space(3))) void* lptr_t;


struct ConvSeg2 {
  const int8_t* x;
  const int8_t* w;
  const float* bias;
  const int32_t* wsum;
  const float* s_in;
  const float* zp_in;
  const float* s_w;
  ConvGeom g;
  int shift;
};

// A 16-byte global load the compiler does not know about (no s_waitcnt is generated for it: the caller counts vmcnt)
template <int OFF>
__device__ __forceinline__ void gload16(i32x4& dst, const int8_t* p) {
  asm volatile("global_load_dwordx4 %0, %1, off offset:%2" : "=v"(dst) : "v"(p), "n"(OFF) : "memory");
}

// Buffer-addressed 16-byte accesses the compiler does not know about (no s_waitcnt is generated for them: the caller counts vmcnt).
// A byte offset beyond the resource's size makes a load return zeros and a store vanish, so a lane outside its tile still ISSUES the
// instruction: every wave issues the same number of vector-memory operations, which counted waits rely on.
typedef int v4i __attribute__((ext_vector_type(4)));

__device__ __forceinline__ v4i make_rsrc(const void* p, uint32_t bytes) {
  const uint64_t a = (uint64_t)p;
  return v4i{(int)(uint32_t)a, (int)(uint32_t)((a >> 32) & 0xffffu), (int)bytes, 0x00020000};
}
// The fp32 streams (shortcut in, block output out) carry the non-temporal hint: measured twice (LABNOTES 13, 14) against temporal
// accesses - whole batches and cache-sized sub-batches walked through a stage.  -DDLMCQ_FP32_TEMPORAL builds the A/B library without it.
#ifdef DLMCQ_FP32_TEMPORAL
#define DLMCQ_NT ""
#else
#define DLMCQ_NT " nt"
#endif
__device__ __forceinline__ void bload16(f32x4& dst, int voff, const v4i& rsrc) {
  asm volatile("buffer_load_dwordx4 %0, %1, %2, 0 offen" DLMCQ_NT : "=v"(dst) : "v"(voff), "s"(rsrc) : "memory");
}
template <int OFF>
__device__ __forceinline__ void bload16i(i32x4& dst, int voff, const v4i& rsrc) {
  asm volatile("buffer_load_dwordx4 %0, %1, %2, 0 offen offset:%3" : "=v"(dst) : "v"(voff), "s"(rsrc), "n"(OFF) : "memory");
}
// (a store of more than 8 bytes reads its data registers late: gfx940+ needs TWO wait states before a VALU instruction may
//  overwrite them, and the hazard recogniser does not see inside inline asm - with one, the last quad of every 16 lanes
//  can store the NEXT value of a dword)
__device__ __forceinline__ void bstore16(const f32x4& v, int voff, const v4i& rsrc) {
  asm volatile("buffer_store_dwordx4 %0, %1, %2, 0 offen" DLMCQ_NT "\n\ts_nop 1" ::"v"(v), "v"(voff), "s"(rsrc) : "memory");
}
__device__ __forceinline__ void bstore16i(const i32x4& v, int voff, const v4i& rsrc) {
  asm volatile("buffer_store_dwordx4 %0, %1, %2, 0 offen\n\ts_nop 1" ::"v"(v), "v"(voff), "s"(rsrc) : "memory");
}
__device__ __forceinline__ void bstore16i_nt(const i32x4& v, int voff, const v4i& rsrc) {
  asm volatile("buffer_store_dwordx4 %0, %1, %2, 0 offen nt\n\ts_nop 1" ::"v"(v), "v"(voff), "s"(rsrc) : "memory");
}
constexpr int BUF_BIG = 0x7fff0000;   // a byte offset beyond every buffer these kernels accept (< 2^31 - 64 KiB)

// A pad shortcut (the PADRES instantiations of conv_i8_mfma_kernel; dlmcq_conv2d_i8_nhwc_padres): ep.residual is the dense fp32 NHWC source
// [N][h][w][c] of pad(x[:, ::stride, ::stride, :]) with `clo` zero channels in front
struct PadRes {
  int h, w, c, stride, clo;
};

// One int8 convolution as the host dispatch sees it: what an entry point of conv_i8.hip received, once, by name.  conv_launch and
// every kernel family it routes to (conv_pw_*, conv_pwr_*, conv3x3_halo_*, conv3x3_pipe_*) take this record and fill their own device
// records (ConvGeom, PwArgs, PwrArgs, HaloGeom, PipeGeom) from it.
struct ConvCall {
  const int8_t* x;
  const int8_t* w;
  float* out;
  const float* bias;
  const int32_t* wsum;
  const float* s_in;
  const float* zp_in;
  const float* s_w;
  int64_t N, H, W, C, K, R, S;
  int32_t stride, pad, dil;
  int shift;                 // 128 when the activation codes are unsigned bytes, else 0
  hipStream_t st;
  ConvEpi ep;
  const ConvSeg2* seg2;      // the dual form's second operand pair, or null
  const PadRes* padres;      // a pad shortcut's source geometry, or null
  int64_t P, Q, M;           // derived by conv_call: the output's height and width, N * P * Q
};

// THE output-size formula.  (A stride below 1 is refused by whoever validates the call; until then it must not divide by zero:
// dlmcq_conv2d_i8_nhwc_fused_observed sizes its partial planes before conv_launch has looked at the arguments.)
inline int64_t conv_out_size(int64_t in, int64_t taps, int32_t stride, int32_t pad, int32_t dil) {
  return (in + 2 * pad - dil * (taps - 1) - 1) / (stride > 0 ? stride : 1) + 1;
}

// the record of an entry point's ABI arguments; the fields particular to an entry point (ep, seg2, padres) are the caller's to set
inline ConvCall conv_call(const void* x, const int8_t* w, float* out, const float* bias, const int32_t* wsum, const float* in_scale,
                          const float* in_zero_point, const float* w_scale, int64_t N, int64_t H, int64_t W, int64_t C, int64_t K,
                          int64_t R, int64_t S, int32_t stride, int32_t pad, int32_t dilation, int32_t x_is_unsigned,
                          dlmcq_stream_t stream) {
  ConvCall c{};
  c.x = static_cast<const int8_t*>(x); c.w = w; c.out = out; c.bias = bias; c.wsum = wsum; c.s_in = in_scale; c.zp_in = in_zero_point;
  c.s_w = w_scale;
  c.N = N; c.H = H; c.W = W; c.C = C; c.K = K; c.R = R; c.S = S; c.stride = stride; c.pad = pad; c.dil = dilation;
  c.shift = x_is_unsigned ? 128 : 0;
  c.st = reinterpret_cast<hipStream_t>(stream);
  c.P = conv_out_size(H, R, stride, pad, dilation);
  c.Q = conv_out_size(W, S, stride, pad, dilation);
  c.M = N * c.P * c.Q;
  return c;
}

// the tiled kernels' geometry of a validated call (every field < 2^31); the tile counts are conv_geom_tiles'
inline ConvGeom conv_geom(const ConvCall& c) {
  ConvGeom g{};
  g.N = (int)c.N; g.H = (int)c.H; g.W = (int)c.W; g.C = (int)c.C; g.K = (int)c.K; g.R = (int)c.R; g.S = (int)c.S;
  g.stride = c.stride; g.pad = c.pad; g.dil = c.dil; g.P = (int)c.P; g.Q = (int)c.Q; g.M = c.M;
  g.qdiv = make_fastdiv((uint32_t)c.Q);
  g.pdiv = make_fastdiv((uint32_t)c.P);
  return g;
}
inline void conv_geom_tiles(ConvGeom& g, int bn) {     // CV_BM pixels x bn channels per workgroup
  g.nblk_m = (int)((g.M + CV_BM - 1) / CV_BM);
  g.nblk_n = (g.K + bn - 1) / bn;
}

// The seven pointers of one 1x1 operand of the chain kernels (conv_chain_i8.hip), as its device record ChainArgs holds them three times
struct ChainOp {
  const int8_t* x;
  const int8_t* w;
  const float* s_w;
  const int32_t* wsum;
  const float* bias;
  const float* s_in;
  const float* zp_in;
};

// ... and with its geometry, as an entry point received it: x codes [N][H][W][C], read at (p * stride, q * stride)
struct ChainOperand {
  ChainOp p;
  int64_t N, H, W, C;
  int32_t stride;
  int shift;                 // 128 when the activation codes are unsigned bytes, else 0
};

inline ChainOperand chain_operand(const void* x, const int8_t* w, const float* bias, const int32_t* wsum, const float* in_scale,
                                  const float* in_zero_point, const float* w_scale, int64_t N, int64_t H, int64_t W, int64_t C,
                                  int32_t stride, int32_t x_is_unsigned) {
  return ChainOperand{{static_cast<const int8_t*>(x), w, w_scale, wsum, bias, in_scale, in_zero_point}, N, H, W, C, stride,
                      x_is_unsigned ? 128 : 0};
}

// One chain launch as the host sees it: what an entry point of conv_chain_i8.hip received, once, by name.  `uses` says which of the
// shortcut's three sources the entry point has - chain_launch requires exactly those and ignores the others.
enum : unsigned { CHAIN_RESIDUAL = 1, CHAIN_SAMPLED = 2, CHAIN_UNIT = 4 };
struct ChainCall {
  unsigned uses;
  ChainOperand own;          // the block end: [N][H][W][C] -> K channels (the plain form passes its M rows as N x 1 x 1)
  ChainOperand sampled;      // CHAIN_SAMPLED: the 1x1 / stride-s convolution on the shortcut (its own block's, or the recomputed block's)
  ChainOperand unit;         // CHAIN_UNIT: the recomputed block's unit-stride operand
  const float* residual;     // CHAIN_RESIDUAL: fp32 [M][K]
  int32_t relu_shortcut;     // CHAIN_UNIT: the recomputed block's own activation
  float* out;                // fp32 [M][K] or null
  int64_t K, K2;
  ChainOp second;            // the next 1x1 reduction K -> K2: w, s_w, wsum, bias (its input is ep1's codes)
  ConvEpi ep1, ep2;          // ep1.codes [M][K] or null, ep2.codes [M][K2]
  int32_t q_lo, q_hi, q_form, q2_lo, q2_hi;   // the ranges and ep1's form as passed (make_epi folds them; chain_launch validates these)
  uint32_t layout;           // DLMCQ_W2_CHUNK_MAJOR | DLMCQ_FP32_IN_CHUNK_MAJOR | DLMCQ_FP32_OUT_CHUNK_MAJOR of the second `q_form`
  bool which;                // DLMCQ_ROUTE_CHAIN_VARIANT of the second `q_form` (DLMCQ_ROUTE_ONLY itself travels in ep2.ctl)
  int32_t rows_per_tile;
  hipStream_t st;
};

// compute units of the current device (cached: one device per process, dlmc/_native.py)
inline int device_cus() {
  static int cus = 0;
  if (!cus) {
    int dev = 0;
    hipDeviceProp_t prop;
    cus = (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess && prop.multiProcessorCount > 0)
              ? prop.multiProcessorCount : 256;
  }
  return cus;
}

// The weight-resident 1 x 1 kernels (conv_pw_i8.hip, conv_pwr_i8.hip): workgroups per column slice - `wgs` resident workgroups shared
// among the `nslice` slices, in whole eights (the workgroups of a group sit on one XCD and share their pixels), eight at least, and no
// more than give every one of a workgroup's `nw` waves a 32-pixel block
inline int resident_groups(int wgs, int nslice, int nblk, int nw) {
  int ngroups = (wgs / nslice) & ~7;
  if (ngroups < 8) ngroups = 8;
  const int maxg = ((nblk + nw - 1) / nw + 7) & ~7;
  return ngroups > maxg ? maxg : ngroups;
}

// Dynamic LDS beyond the default limit has to be allowed per kernel: one record per kernel instantiation (KERN) of the largest size
// allowed so far, and the attribute is set when a launch first needs more.  (A workgroup's LDS is at most 160 KB: the size fits an int.)
template <auto KERN>
inline hipError_t allow_dyn_lds(size_t lds) {
  static size_t allowed = 0;
  if (lds > allowed) {
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(KERN), hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(lds));
    if (e != hipSuccess) return e;
    allowed = lds;
  }
  return hipSuccess;
}
// Launch KERN with `lds` bytes of dynamic LDS, allowed first
template <auto KERN, typename... Args>
inline int launch_dyn_lds(dim3 grid, dim3 block, size_t lds, hipStream_t st, const Args&... args) {
  const hipError_t e = allow_dyn_lds<KERN>(lds);
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(KERN, grid, block, lds, st, args...);
  return launch_status();
}

// The kernel families conv_launch routes to.  `applies` answers for the whole record - the problem, the epilogue, the fp32 output and
// the second pair - and `launch` may be called only where it said yes.
// conv3x3_i8.hip: the halo-tile kernel for 3x3 / stride 1 or 2 / pad 1 layers that emit only their consumer's codes
bool conv3x3_halo_applies(const ConvCall& c);
int conv3x3_halo_launch(const ConvCall& c, int lab = 0, void* lab_trace = nullptr);
int conv3x3_halo_answer(const ConvCall& c);                    // DLMCQ_ROUTE_HALO_VARIANT: which instantiation the launch picks (include/dlmcq.h)
int conv3x3_halo_table(int32_t* answers, int cap);             // every instantiation the launcher holds, as such answers; returns how many
int conv3x3_halo_dense_table(int32_t* answers, int cap);       // ... and those of them that also exist with the dense row mapping (flag 8 set)

// conv3x3_pipe_i8.hip: the halo-tile kernel persistent and software-pipelined across tiles (stride 1, 128 / 256 / 512 input channels,
// plain quantiser); asked only about calls the halo kernel takes
bool conv3x3_pipe_applies(const ConvCall& c, int cus);
int conv3x3_pipe_launch(const ConvCall& c, int cus);
int conv3x3_pipe_answer(const ConvCall& c);
int conv3x3_pipe_table(int32_t* answers, int cap);

// conv_pw_i8.hip: pointwise codes-to-codes layers with the weights resident in LDS (MobileOne's 1x1 layers)
bool conv_pw_applies(const ConvCall& c);
int conv_pw_launch(const ConvCall& c, int lab = 0, void* lab_trace = nullptr);
int conv_pw_answer(const ConvCall& c);
int conv_pw_table(int32_t* answers, int cap);

// conv_pwr_i8.hip: 1 x 1 block ends with an fp32 shortcut (+ fp32 output) + ReLU + codes, the weights resident in LDS
bool conv_pwr_applies(const ConvCall& c);
int conv_pwr_launch(const ConvCall& c);
int conv_pwr_answer(const ConvCall& c);
int conv_pwr_table(int32_t* answers, int cap);

// One first-layer convolution as the host sees it: what an entry point of conv_stem_i8.hip received, once, by name.  `x` is the padded
// NHWC4 code buffer [N][Hp][Wp][4]; ep.w_off / ep.x_off / ep.x_tap (and C, xpad with them) are the entry point's to set.
struct StemCall {
  const uint8_t* x;
  const int8_t* w;
  float* out;
  const float* bias;
  const int32_t* wsum;
  const float* s_in;
  const float* zp_in;
  const float* s_w;
  int64_t C, N, Hp, Wp, K, R, S;   // C: real input channels (asymmetric weights: which operand bytes count), else 4
  int32_t stride, xpad;            // xpad: the padding the buffer carries (float activation offset only)
  int shift;                       // 128 when the activation codes are unsigned bytes, else 0
  hipStream_t st;
  ConvEpi ep;
  int32_t q_lo, q_hi, q_form;      // the quantiser's range and form as passed (stem_check validates these)
  int64_t P, Q, M;                 // derived by stem_call: the output's height and width, N * P * Q
  bool which;                      // DLMCQ_ROUTE_ONLY | DLMCQ_ROUTE_PW_VARIANT in `q_form`: validate, launch nothing, answer the instantiation
  bool lone;                       // DLMCQ_ROUTE_PW_VARIANT without DLMCQ_ROUTE_ONLY: refused whatever else the call holds
};

// One depthwise convolution as the host sees it (conv_dw_i8.hip's entry points; conv_dwm_i8.hip takes the same record)
struct DwCall {
  const void* x;
  const int8_t* w;
  float* out;
  const float* bias;
  const float* s_in;
  const float* zp_in;
  const float* s_w;
  const float* w_off;
  int64_t N, H, W, C, R, S;
  int32_t stride, pad;
  int x_signed;
  hipStream_t st;
  ConvEpi ep;                      // ep.q_form: `q_form` without the control bits; ep.x_off / ep.x_tap: the _xoff entry point's
  uint32_t ctl;                    // DLMCQ_FORCE_TILED | DLMCQ_ROUTE_ONLY | DLMCQ_ROUTE_DW_VARIANT as passed in `q_form`
  int32_t q_lo, q_hi, q_form;      // as passed (dw_launch validates these)
  int64_t P, Q;                    // derived by dw_call
};

// conv_dwm_i8.hip: depthwise 3 x 3 / stride 1 / padding 1 codes-to-codes layers on the matrix cores (diagonal weight fragments)
bool conv_dwm_applies(const DwCall& c);
int conv_dwm_launch(const DwCall& c);
int conv_dwm_answer(const DwCall& c);                          // DLMCQ_ROUTE_DW_VARIANT: which instantiation the launch picks (include/dlmcq.h)
int conv_dwm_table(int32_t* answers, int cap);                 // every instantiation the launcher holds, as such answers; returns how many

// conv_stem_pool7_i8.hip: the ResNet first layer (7x7 / 2 + ReLU + 3x3 / 2 max-pool + quantiser) with the pooling in registers
bool stem_pool7_applies(const StemCall& c);
int stem_pool7_launch(const StemCall& c);
bool stem_pool7_xs(const StemCall& c);     // which of its two instantiations (XS): read by the launch and by the route query

// uint8 -> int8 on a 16-byte MFMA fragment (xorw = 0x80808080 where the codes are unsigned bytes, else 0)
__host__ __device__ __forceinline__ i32x4 flip128(const i32x4& v, uint32_t xorw) {
  return i32x4{(int)(v.x ^ xorw), (int)(v.y ^ xorw), (int)(v.z ^ xorw), (int)(v.w ^ xorw)};
}

// A lane's 16 accumulators start from (shift - zp) * SUM qw of their 16 consecutive channels out of an LDS table (`tab`: the first of
// them): four LDS reads instead of sixteen additions per block
__device__ __forceinline__ void acc_from_lds(i32x16& acc, const void* tab) {
  const i32x4* cop = reinterpret_cast<const i32x4*>(tab);
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const i32x4 c4 = cop[q];
    acc[4 * q] = c4.x;
    acc[4 * q + 1] = c4.y;
    acc[4 * q + 2] = c4.z;
    acc[4 * q + 3] = c4.w;
  }
}

template <int N, typename F>
__device__ __forceinline__ void static_for(F&& f) {
  if constexpr (N > 0) {
    static_for<N - 1>(f);
    f(std::integral_constant<int, N - 1>{});
  }
}

}  // namespace dlmcq
