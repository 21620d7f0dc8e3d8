// Depthwise 5 x 5 convolution, padding 2, stride 1 or 2, on NHWC activation codes: the 5 x 5 layers of the MBConv family (9 of
// EfficientNet-B0's 16 depthwise layers, MobileNetV3, MnasNet), which conv_dw_i8.hip runs on its any-filter kernel - one dword per thread and
// tap, every byte of every tap converted to fp32: ~150 vector instructions per output element at 25 taps.  This kernel keeps the arithmetic
// contract of the 3 x 3 vector kernels of conv_dw_i8.hip and stays in integers:
//   * a thread owns 16 consecutive channels of ONE output pixel; neighbouring threads own the neighbouring channel groups, so a tap is one
//     coalesced row of C bytes (one 16-byte load per lane) and the overlapping taps of neighbouring pixels are served by the vector cache;
//   * the taps are requested BY FILTER ROW (5 loads, 20 registers; all 25 at once would be 100) in a loop that is NOT unrolled (unrolled,
//     the compiler hoists every row's loads and table reads: 234-256 registers, or scratch under a cap): taps 0-3 of the row are
//     byte-transposed (transpose4x4: 8 v_perm_b32 per 4 channels) so that a dword holds FOUR TAPS OF ONE CHANNEL, which v_dot4_i32_i8
//     multiplies with the channel's four weights; tap 4 is multiplied where it lies, by a weight dword that is 0 but for the channel's byte;
//   * unsigned codes are re-centred by xor 0x80 with the constant (128 - zp) * SUM w added back (the start value of the sum);
//   * a tap outside the image contributes nothing to either sum: it is replaced by the zero point (a clamped address and a select) - or,
//     where the zero point is 0 and the tensor is smaller than DW_BIG, read as an out-of-range buffer load, which returns the zero bytes;
//   * S1 = SUM (q - zp) * qw and S0 = SUM (q - zp) are exact integers (|S1| <= 25 * 255 * 255 < 2^24: exact in int32 and in fp32); after
//     them the fp32 chain of conv_dw_i8_kernel in its order, every step rounded on its own: S1 * (s_in * s_w), + S0 * (s_in * o_w) for
//     asymmetric weights, + bias, ReLU, cap6_nan4 for ReLU6, the fp32 store, EpiQuant's codes.  Bit-identical to conv_dw_i8_kernel for every
//     INTEGER zero point in the byte range (zpi = (int)zp, as in the 3 x 3 kernels; the generic kernel alone takes a fractional one).
// Weights and per-channel constants are packed once per workgroup into an LDS table (below), 57 bytes per channel: C <= 2048.
#include "conv_dw_common.h"

namespace dlmcq {

// The table: one run of 57 16-byte records per channel group (= per lane), so that a thread reads its records at constant offsets from
// one base address and neighbouring lanes start an odd number of records apart (ds_read_b128 without bank conflicts).  A record holds
// one quantity of FOUR consecutive channels (d = 0..3: channels 4d .. 4d + 3 of the group, channel 4d + j in element j):
//   [4 r + d], r = 0..4        weights of filter row r, taps 0-3 (signed bytes, tap s in byte s)
//   [20 + 4 r + d]             weight of tap 4 of row r IN BYTE j of element j, the other bytes 0: multiplied with the tap's own dword
//                              (bytes = channels 4d .. 4d + 3) by v_dot4_i32_i8, it picks channel j's byte - no transposition
//   [40 + d]                   (shift - zp) * SUM w                            (int32; shift = 128 for unsigned codes)
//   [44 + d] [48 + d] [52 + d] s_in * s_w,  s_in * o_w (0 for symmetric weights),  bias (0 without one)      (fp32)
constexpr int DW5_TAP4 = 20, DW5_DZW = 40, DW5_M = 44, DW5_RUN = 57;
constexpr int DW5_MAX_C = 2048;
constexpr int DW5_GRID = 2048;        // workgroups at most: each packs the table first, then walks pixels in a grid-stride loop

// FAST: 1 / 2 = codes-only layer with the plain quantiser, asymmetric / symmetric weights known at compile time (the fp32 chain on
// vectors of constants the compiler pairs, all four quantiser quads behind one branch: EpiQuant::code4n_plain); 0 = everything else.
// R6: ReLU6's upper bound.  The stride is a run-time argument.
template <int FAST, bool R6>
__global__ __launch_bounds__(DLMCQ_BLOCK) void conv_dw5_i8_kernel(const u32x4* __restrict__ x, const int8_t* __restrict__ w,
                                                                 float* __restrict__ out, const float* __restrict__ bias,
                                                                 const float* __restrict__ s_in, const float* __restrict__ zp_in,
                                                                 const float* __restrict__ s_w, const float* __restrict__ o_w,
                                                                 DwGeom g, int x_signed, ConvEpi ep) {
  extern __shared__ __attribute__((aligned(16))) uint8_t dw5_lds[];
  u32x4* tab = reinterpret_cast<u32x4*>(dw5_lds);
  const int C = g.C4 * 4, C16 = g.C4 >> 2;
  const float sin = s_in[0], zp = zp_in ? zp_in[0] : 0.0f;
  const int zpi = (int)zp;
  const int dz = (x_signed ? 0 : 128) - zpi;
  const bool asym = FAST ? FAST == 1 : o_w != nullptr;
  for (int c = threadIdx.x; c < C; c += blockDim.x) {
    uint32_t pk[5] = {0u, 0u, 0u, 0u, 0u}, p4[5];
    int sum = 0;
    const int e = c & 15;
#pragma unroll
    for (int r = 0; r < 5; ++r)
#pragma unroll
      for (int s = 0; s < 5; ++s) {
        const int wv = w[(r * 5 + s) * C + c];
        sum += wv;
        const uint32_t b = (uint32_t)(wv & 0xff);
        if (s < 4) pk[r] |= b << (8 * s);
        else p4[r] = b << (8 * (e & 3));
      }
    uint32_t* run = reinterpret_cast<uint32_t*>(tab + (c >> 4) * DW5_RUN);     // dword [4 record + e] of a group of four records = element e % 4 of record + e / 4
#pragma unroll
    for (int r = 0; r < 5; ++r) {
      run[16 * r + e] = pk[r];
      run[4 * DW5_TAP4 + 16 * r + e] = p4[r];
    }
    run[4 * DW5_DZW + e] = (uint32_t)(dz * sum);
    float* runf = reinterpret_cast<float*>(run);
    runf[4 * DW5_M + e] = sin * s_w[c];
    runf[4 * DW5_M + 16 + e] = asym ? sin * o_w[c] : 0.0f;
    runf[4 * DW5_M + 32 + e] = bias ? bias[c] : 0.0f;
  }
  __syncthreads();
  const int64_t total = (int64_t)g.N * g.P * g.Q * C16;
  const int64_t xbytes = (int64_t)g.N * g.H * g.W * C;
  const bool bufpath = zpi == 0 && xbytes < (int64_t)DW_BIG;
  // the buffer descriptor's parts, pinned to scalar registers: left to itself the compiler keeps the descriptor in vector registers
  // and wraps every buffer load in a readfirstlane loop (8 more vector instructions per 16-byte load)
  const uint64_t xa = reinterpret_cast<uint64_t>(x);
  // (readfirstlane returns int: each half goes through uint32_t, or a low half with bit 31 set sign-extends over the high one)
  const uint32_t xlo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)xa), xhi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(xa >> 32));
  u32x4* xu = reinterpret_cast<u32x4*>(((uint64_t)xhi << 32) | (uint64_t)xlo);
  const int xn = __builtin_amdgcn_readfirstlane(bufpath ? (int)xbytes : 0);
  const int dz25 = 25 * dz;
  const uint32_t zpw = (uint32_t)(zpi & 0xff) * 0x01010101u;
  const uint32_t xw = x_signed ? 0u : 0x80808080u;
  // codes-only layers: the ReLU is folded into the quantiser's clamp (code(relu(v)) = max(code(v), code(0)): conv_epilogue.h)
  const bool fold = ep.relu && !out && ep.codes;
  const EpiQuant eq(ep, fold);
  constexpr bool S0 = FAST != 2;          // the second sum: FAST 0 computes it whether or not the weights turn out asymmetric
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const uint32_t pix = fdiv((uint32_t)i, g.cdiv);                 // (cdiv divides by C / 16 here)
    const int c16 = (int)((uint32_t)i - pix * (uint32_t)C16);
    const uint32_t t = fdiv(pix, g.qdiv);
    const int q = (int)(pix - t * (uint32_t)g.Q);
    const uint32_t n = fdiv(t, g.pdiv);
    const int p = (int)(t - n * (uint32_t)g.P);
    const int h0 = p * g.stride - 2, w0 = q * g.stride - 2;
    const u32x4* run = tab + c16 * DW5_RUN;
    const u32x4* img = x + (int64_t)n * g.H * g.W * C16 + c16;
    const bool inside = h0 >= 0 && w0 >= 0 && h0 + 4 < g.H && w0 + 4 < g.W;
    const bool clear = !bufpath && __builtin_amdgcn_ballot_w64(!inside) == 0;      // the whole wave is away from the image border: no checks
    const int base0 = (int)(((uint32_t)n * (uint32_t)g.H + (uint32_t)h0) * (uint32_t)g.W + (uint32_t)w0) * C + c16 * 16;   // (wraps at the border: used only where valid)
    bool cok[5];
    int wc[5];
#pragma unroll
    for (int s = 0; s < 5; ++s) {
      cok[s] = (uint32_t)(w0 + s) < (uint32_t)g.W;
      wc[s] = w0 + s < 0 ? 0 : (w0 + s >= g.W ? g.W - 1 : w0 + s);
    }
    int s1[16], s0[16];
#pragma unroll
    for (int d = 0; d < 4; ++d) {
      const u32x4 z = run[DW5_DZW + d];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        s1[4 * d + j] = (int)z[j];
        s0[4 * d + j] = dz25;
      }
    }
#pragma unroll 1
    for (int r = 0; r < 5; ++r) {                                   // a real loop: one filter row's taps in registers at a time
      u32x4 a[5];
      const int h = h0 + r;
      const bool rok = (uint32_t)h < (uint32_t)g.H;
      if (bufpath) {                                                // a tap outside the image reads beyond the tensor's end = zeros = the zero point
        const __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc(xu, 0, xn, 0x00020000);
#pragma unroll
        for (int s = 0; s < 5; ++s)
          a[s] = __builtin_amdgcn_raw_buffer_load_b128(rx, (rok && cok[s]) ? base0 + (r * g.W + s) * C : DW_BIG, 0, 0) ^ xw;
      } else if (clear) {
        const u32x4* p0 = img + ((int64_t)h * g.W + w0) * C16;
#pragma unroll
        for (int s = 0; s < 5; ++s) a[s] = p0[s * C16] ^ xw;
      } else {
        const int hc = h < 0 ? 0 : (h >= g.H ? g.H - 1 : h);
#pragma unroll
        for (int s = 0; s < 5; ++s) {
          const u32x4 v = img[((int64_t)hc * g.W + wc[s]) * C16];
          a[s] = ((rok && cok[s]) ? v : u32x4{zpw, zpw, zpw, zpw}) ^ xw;      // q' = q - shift as a signed byte
        }
      }
#pragma unroll
      for (int d = 0; d < 4; ++d) {                                  // 4 channels at a time
        uint32_t T[4];
        transpose4x4(a[0][d], a[1][d], a[2][d], a[3][d], T);         // taps 0-3 of this row: T[j] = the four taps of channel 4d + j
        const u32x4 wr = run[4 * r + d], w4 = run[DW5_TAP4 + 4 * r + d];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          // tap 4 needs no transposition: channel j's byte of the tap's dword is selected by a weight dword that is 0 in its other bytes
          s1[4 * d + j] = __builtin_amdgcn_sdot4((int)T[j], (int)wr[j], s1[4 * d + j], false);
          s1[4 * d + j] = __builtin_amdgcn_sdot4((int)a[4][d], (int)w4[j], s1[4 * d + j], false);
          if constexpr (S0) {
            s0[4 * d + j] = __builtin_amdgcn_sdot4((int)T[j], 0x01010101, s0[4 * d + j], false);
            s0[4 * d + j] = __builtin_amdgcn_sdot4((int)a[4][d], 1 << (8 * j), s0[4 * d + j], false);
          }
        }
      }
    }
    const int c = c16 * 16;
    uint32_t codes[4];
    f32x4 vq[4];
#pragma unroll
    for (int d = 0; d < 4; ++d) {
      const f32x4 m = __builtin_bit_cast(f32x4, run[DW5_M + d]);
      f32x4 v = f32x4{(float)s1[4 * d], (float)s1[4 * d + 1], (float)s1[4 * d + 2], (float)s1[4 * d + 3]} * m;      // S1 = SUM (q - zp) * qw, exact
      if constexpr (S0) {
        if (asym) {
          const f32x4 mo = __builtin_bit_cast(f32x4, run[DW5_M + 4 + d]);
          v = v + f32x4{(float)s0[4 * d], (float)s0[4 * d + 1], (float)s0[4 * d + 2], (float)s0[4 * d + 3]} * mo;     // S0 = SUM (q - zp)
        }
      }
      if (FAST != 0 || bias) v = v + __builtin_bit_cast(f32x4, run[DW5_M + 8 + d]);      // (FAST, no bias: + 0, which only turns a -0 into +0 - the same code)
      if constexpr (FAST != 0) {
        vq[d] = R6 ? cap6_nan4(v) : v;
        continue;
      }
      if (ep.relu && !fold) v = f32x4{relu_nan(v.x), relu_nan(v.y), relu_nan(v.z), relu_nan(v.w)};
      if constexpr (R6) v = cap6_nan4(v);
      const int64_t at = (int64_t)pix * C + c + d * 4;
      if (out) __builtin_nontemporal_store(v, reinterpret_cast<f32x4*>(out + at));
      if (ep.codes) codes[d] = eq.code4(v);
    }
    if constexpr (FAST != 0) eq.code4n_plain(vq, codes);
    if (ep.codes) __builtin_nontemporal_store(u32x4{codes[0], codes[1], codes[2], codes[3]}, reinterpret_cast<u32x4*>(ep.codes + (int64_t)pix * C + c));
  }
}

}  // namespace dlmcq

using namespace dlmcq;

// THE table of this file's instantiations: FAST 0 / 1 / 2 x R6.  One macro line gives a row's key and the launcher of the kernel it names.
typedef void (*Dw5Go)(dim3 grid, size_t lds, const DwCall& c, const DwGeom& g);
template <int FAST, bool R6>
static void dw5_go(dim3 grid, size_t lds, const DwCall& c, const DwGeom& g) {
  hipLaunchKernelGGL((conv_dw5_i8_kernel<FAST, R6>), grid, dim3(DLMCQ_BLOCK), lds, c.st, static_cast<const u32x4*>(c.x), c.w, c.out, c.bias, c.s_in,
                     c.zp_in, c.s_w, c.w_off, g, c.x_signed, c.ep);
}
template <int FAST, bool R6>
static hipError_t dw5_big_lds() {      // tables above 64 KB (C >= 1152): the kernel's dynamic LDS limit, raised once
  return allow_dyn_lds<conv_dw5_i8_kernel<FAST, R6>>(DW5_MAX_C / 16 * DW5_RUN * 16);
}
struct Dw5Variant {
  int fast;
  bool r6;
  Dw5Go go;
  hipError_t (*big_lds)();
};
#define DLMCQ_DW5_V(FAST, R6) {FAST, R6, dw5_go<FAST, R6>, dw5_big_lds<FAST, R6>},
static const Dw5Variant DW5_TABLE[] = {DLMCQ_DW5_V(0, false) DLMCQ_DW5_V(1, false) DLMCQ_DW5_V(2, false)
                                       DLMCQ_DW5_V(0, true) DLMCQ_DW5_V(1, true) DLMCQ_DW5_V(2, true)};
#undef DLMCQ_DW5_V
constexpr int DW5_VARIANTS = sizeof(DW5_TABLE) / sizeof(DW5_TABLE[0]);
static_assert(DW5_VARIANTS == 6, "the instantiations");

// The record of a validated call (null: none - the table is complete, so never); computed ONCE per call: the launch and the route query
// read this one record.  FAST as in conv_dw_i8.hip: a codes-only layer with the plain quantiser, 1 asymmetric / 2 symmetric weights.
static const Dw5Variant* dw5_variant(const DwCall& c) {
  const int fast = (!c.out && epi_plain(c.ep)) ? (c.w_off ? 1 : 2) : 0;
  const bool r6 = c.ep.relu == DLMCQ_ACT_RELU6;
  for (const Dw5Variant& t : DW5_TABLE)
    if (t.fast == fast && t.r6 == r6) return &t;
  return nullptr;
}
// ... as the route query's answer (include/dlmcq.h: DLMCQ_ROUTE_DW5_VARIANT_TAG | FAST << 4 | 1 R6)
static int dw5_variant_answer(const Dw5Variant& v) { return DLMCQ_ROUTE_DW5_VARIANT_TAG | (v.fast << 4) | (v.r6 ? 1 : 0); }

// The table, for tests (absent from include/dlmcq.h): fills up to `cap` route answers in the table's order and returns how many there are
extern "C" int dlmcq_x_dw5_variant_table(int32_t* answers, int cap) {
  int n = 0;
  for (const Dw5Variant& t : DW5_TABLE) {
    if (answers && n < cap) answers[n] = dw5_variant_answer(t);
    ++n;
  }
  return n;
}

extern "C" int dlmcq_conv2d_dw5_i8_nhwc(const void* x, const int8_t* w, float* out, const float* bias, const float* in_scale,
                                        const float* in_zero_point, const float* w_scale, const float* w_offset, int64_t N, int64_t H,
                                        int64_t W, int64_t C, int32_t stride, int32_t pad, int32_t x_is_unsigned, int32_t relu, void* codes,
                                        const float* q_scale, const float* q_zero_point, int32_t q_lo, int32_t q_hi, int32_t q_form,
                                        float q_ste_g, dlmcq_stream_t stream) {
  const DwCall c = dw_call(x, w, out, bias, in_scale, in_zero_point, w_scale, w_offset, N, H, W, C, 5, 5, stride, pad, x_is_unsigned, relu, codes,
                           q_scale, q_zero_point, q_lo, q_hi, q_form, q_ste_g, stream);
  // the control bits: none but the route query (DLMCQ_ROUTE_ONLY | DLMCQ_ROUTE_DW_VARIANT, both); then this kernel's own geometry
  if (c.ctl != 0 && c.ctl != (uint32_t)(DLMCQ_ROUTE_ONLY | DLMCQ_ROUTE_DW_VARIANT)) return DLMCQ_EINVAL;
  if ((stride != 1 && stride != 2) || pad != 2 || C % 16 != 0 || C > DW5_MAX_C) return DLMCQ_EINVAL;
  int status;
  if (!dw_checks(c, true, status)) return status;      // (conv_dw_common.h: dlmcq_conv2d_dw_i8_nhwc's checks in their order, x and codes at 16 bytes)
  const Dw5Variant* v = dw5_variant(c);
  if (!v) return DLMCQ_EINVAL;
  if (c.ctl) return dw5_variant_answer(*v);
  DwGeom g;
  g.N = (int)c.N; g.H = (int)c.H; g.W = (int)c.W; g.C4 = (int)(c.C / 4); g.R = 5; g.S = 5; g.stride = c.stride; g.pad = c.pad;
  g.P = (int)c.P; g.Q = (int)c.Q;
  g.cdiv = make_fastdiv((uint32_t)(c.C / 16));
  g.qdiv = make_fastdiv((uint32_t)c.Q);
  g.pdiv = make_fastdiv((uint32_t)c.P);
  const size_t lds = (size_t)(c.C / 16) * DW5_RUN * 16;
  if (lds > 64 * 1024) {
    const hipError_t e = v->big_lds();
    if (e != hipSuccess) return (int)e;
  }
  const int64_t blocks = (c.N * c.P * c.Q * (c.C / 16) + DLMCQ_BLOCK - 1) / DLMCQ_BLOCK;
  v->go(dim3((uint32_t)(blocks < DW5_GRID ? blocks : DW5_GRID)), lds, c, g);
  return launch_status();
}
