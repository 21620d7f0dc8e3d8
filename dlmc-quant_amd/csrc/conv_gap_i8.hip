// The network's head in one launch: a 1 x 1 / stride 1 / unpadded convolution on activation codes (+ fp32 shortcut) (+ ReLU / ReLU6),
// pooled over the image's H W <= 64 pixels into fp32 [N, K] and / or the classifier's activation codes [N, K].  The full [N, H, W, K]
// fp32 map - the last one the plan used to write (205 MB for ResNet-50 at batch 512) - never exists.
//
//   * a workgroup (4 waves) owns a slice of BN = 64 or 128 output channels: its weights (BN x C bytes) and per-channel constants are
//     loaded into LDS ONCE, then it walks images  group, group + ngroups, ...;
//   * per image: wave w multiplies pixel rows 32 (w & 1) .. + 31 by the channel blocks of its half of the slice on
//     v_mfma_i32_32x32x32_i8, weights as the A operand from LDS, activation fragments straight from global memory to registers (the
//     same 16 bytes feed both channel blocks of a 128-wide slice); lanes of rows >= H W load pixel 0's bytes and their sums are dropped;
//   * the epilogue is the tiled kernel's chain unchanged (conv_i8.hip: dequant1 of the exact integer sum, + shortcut, relu_nan,
//     cap6_nan), written as fp32 into an LDS stage [64 pixels][BN]; rows >= H W never enter it;
//   * after a barrier one thread per 4 channels walks the rows ascending (gap.hip's sum, gap_finish4's division and quantiser).
// So pooled / codes equal dlmcq_conv2d_i8_nhwc_fused (fp32 output) followed by dlmcq_gap_nhwc_f32 bit for bit (tests/test_gpu_gap.py).
#include "conv_i8_common.h"
#include "conv_gap.h"

namespace dlmcq {

struct GapArgs {
  const int8_t* x;         // [N][HW][C] codes
  const int8_t* w;         // [K][C] int8
  const float* s_w;        // [K]
  const int32_t* wsum;     // [K]
  const float* bias;       // [K] or null
  const float* s_in;
  const float* zp_in;      // null: 0
  float* pooled;           // [N][K] or null
  int N, HW, C, K, shift, ngroups;
};

constexpr int GAP_ROWS = 64;                                  // pixel rows of the stage = the largest image
constexpr int gap_stage_ld(int bn) { return bn + 4; }         // floats per staged row (+ 4: rows 16 bytes apart in the banks)
constexpr int gap_w_ld(int c) { return c + 16; }              // bytes per weight row in LDS
static inline size_t gap_lds_bytes(int c, int bn) { return (size_t)bn * gap_w_ld(c) + 3 * bn * 4 + (size_t)GAP_ROWS * gap_stage_ld(bn) * 4; }

// NT: 32-channel blocks per wave (slice BN = 64 NT)
template <int NT>
__global__ __launch_bounds__(256) void conv_gap_i8_kernel(GapArgs a, ConvEpi ep) {
  constexpr int BN = 64 * NT;
  constexpr int SLD = gap_stage_ld(BN);
  extern __shared__ __attribute__((aligned(16))) int8_t gap_lds[];
  const int C = a.C, WLD = gap_w_ld(C);
  int8_t* const wl = gap_lds;                                          // [BN][WLD]
  float* const par = reinterpret_cast<float*>(gap_lds + BN * WLD);     // s_in s_w | (shift - zp) SUM qw | bias
  float* const stg = par + 3 * BN;                                     // [GAP_ROWS][SLD]

  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, l31 = lane & 31, hsel = lane >> 5;
  const int nslice = a.K / BN;
  const int slice = (int)(blockIdx.x % (uint32_t)nslice), group = (int)(blockIdx.x / (uint32_t)nslice);
  const int n0 = slice * BN;

  // ---- once per workgroup: the slice's weights and constants ----
  {
    const int segs = C >> 4;
    for (int i = tid; i < BN * segs; i += 256) {
      const int row = i / segs, seg = i - row * segs;
      *reinterpret_cast<i32x4*>(wl + row * WLD + seg * 16) = *reinterpret_cast<const i32x4*>(a.w + (int64_t)(n0 + row) * C + seg * 16);
    }
    const float zpf = a.zp_in ? a.zp_in[0] : 0.0f;
    const int zpi = (int)__builtin_rintf(zpf);
    const float sin = a.s_in[0];
    for (int c = tid; c < BN; c += 256) {
      par[c] = sin * a.s_w[n0 + c];
      reinterpret_cast<int*>(par)[BN + c] = (a.shift - zpi) * a.wsum[n0 + c];
      par[2 * BN + c] = a.bias ? a.bias[n0 + c] : 0.0f;
    }
  }
  __syncthreads();

  const uint32_t xorw = a.shift ? 0x80808080u : 0u;
  const int rb = wave & 1, cw = wave >> 1;          // this wave's pixel rows 32 rb .. + 31, channel blocks cw NT .. cw NT + NT - 1
  const int pix = rb * 32 + l31;
  const bool row_ok = pix < a.HW;
  const EpiQuant eq(ep);
  const int8_t* const wrow = wl + (cw * NT * 32 + l31) * WLD + hsel * 16;

  for (int n = group; n < a.N; n += a.ngroups) {
    i32x16 acc[NT];
#pragma unroll
    for (int j = 0; j < NT; ++j)
#pragma unroll
      for (int i = 0; i < 16; ++i) acc[j][i] = 0;
    const int8_t* const xrow = a.x + ((int64_t)n * a.HW + (row_ok ? pix : 0)) * C + hsel * 16;
    for (int s = 0; s < C; s += 64) {        // (C % 64 == 0: two fragments in flight per step)
      i32x4 bf[2] = {*reinterpret_cast<const i32x4*>(xrow + s), *reinterpret_cast<const i32x4*>(xrow + s + 32)};
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        bf[h] = flip128(bf[h], xorw);
#pragma unroll
        for (int j = 0; j < NT; ++j) {
          const i32x4 af = *reinterpret_cast<const i32x4*>(wrow + j * 32 * WLD + s + h * 32);
          acc[j] = __builtin_amdgcn_mfma_i32_32x32x32_i8(af, bf[h], acc[j], 0, 0, 0);
        }
      }
    }
    // ---- epilogue: register i of block j = channel 32 (cw NT + j) + 8 (i >> 2) + 4 hsel + (i & 3) of pixel `pix` ----
    if (row_ok) {
      const int64_t rrow = ((int64_t)n * a.HW + pix) * a.K + n0;
#pragma unroll
      for (int j = 0; j < NT; ++j) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int c = (cw * NT + j) * 32 + 8 * q + 4 * hsel;
          const f32x4 mu = *reinterpret_cast<const f32x4*>(par + c);
          const i32x4 co = *reinterpret_cast<const i32x4*>(par + BN + c);
          const f32x4 bs = *reinterpret_cast<const f32x4*>(par + 2 * BN + c);
          f32x4 v = f32x4{dequant1(acc[j][4 * q] + co.x, mu.x, bs.x), dequant1(acc[j][4 * q + 1] + co.y, mu.y, bs.y),
                          dequant1(acc[j][4 * q + 2] + co.z, mu.z, bs.z), dequant1(acc[j][4 * q + 3] + co.w, mu.w, bs.w)};
          if (ep.residual) {
            const f32x4 r = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(ep.residual + rrow + c));
            v = f32x4{v.x + r.x, v.y + r.y, v.z + r.z, v.w + r.w};
          }
          if (ep.relu) v = f32x4{relu_nan(v.x), relu_nan(v.y), relu_nan(v.z), relu_nan(v.w)};
          if (ep.relu == DLMCQ_ACT_RELU6) v = cap6_nan4(v);
          *reinterpret_cast<f32x4*>(stg + pix * SLD + c) = v;
        }
      }
    }
    __syncthreads();
    // ---- pool: one thread per 4 channels, rows ascending ----
    if (tid < BN / 4) {
      const float* col = stg + tid * 4;
      f32x4 sum = *reinterpret_cast<const f32x4*>(col);
      for (int p = 1; p < a.HW; ++p) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(col + p * SLD);
        sum = f32x4{sum.x + v.x, sum.y + v.y, sum.z + v.z, sum.w + v.w};
      }
      gap_finish4(sum, a.HW, eq, a.pooled, ep.codes, (int64_t)n * a.K + n0 + tid * 4);
    }
    __syncthreads();       // the stage is free for the next image
  }
}

// What the launcher decides for a problem of N images, C -> K channels on `cus` compute units, once: the launch reads this record, and
// dlmcq_x_gap_launch_record (tests) answers it
struct GapLaunch {
  int nt;          // 32-channel blocks per wave: slices of 64 nt channels
  int nslice;      // K / (64 nt)
  int ngroups;     // workgroups per slice; workgroup `group` owns images group, group + ngroups, ...
  size_t lds;      // dynamic LDS bytes of a workgroup
};

static inline GapLaunch gap_launch_record(int64_t N, int C, int K, int cus) {
  GapLaunch r;
  // 128-wide slices (one activation fragment feeds two channel blocks) where two workgroups' weights still fit a CU's LDS
  r.nt = (K % 128 == 0 && gap_lds_bytes(C, 128) <= 78 * 1024) ? 2 : 1;
  r.nslice = K / (64 * r.nt);
  int64_t ngroups = (2 * cus + r.nslice - 1) / r.nslice;               // ~2 workgroups per CU; each keeps its weights for N / ngroups images
  if (ngroups > N) ngroups = N;
  if (ngroups < 1) ngroups = 1;
  r.ngroups = (int)ngroups;
  r.lds = gap_lds_bytes(C, 64 * r.nt);
  return r;
}

template <int NT>
static int gap_go(const GapArgs& a, const ConvEpi& ep, size_t lds, int nwg, hipStream_t st) {
  return launch_dyn_lds<conv_gap_i8_kernel<NT>>(dim3((uint32_t)nwg), dim3(256), lds, st, a, ep);
}

}  // namespace dlmcq

using namespace dlmcq;

extern "C" int dlmcq_conv2d_i8_nhwc_gap(const void* x, const int8_t* w, float* pooled, const float* bias, const int32_t* wsum,
                                        const float* in_scale, const float* in_zero_point, const float* w_scale, int64_t N, int64_t H,
                                        int64_t W, int64_t C, int64_t K, int32_t x_is_unsigned, const float* residual, int32_t act,
                                        void* codes, const float* q_scale, const float* q_zero_point, int32_t q_lo, int32_t q_hi,
                                        int32_t q_form, float q_ste_g, dlmcq_stream_t stream) {
  if (N < 0 || H < 1 || W < 1 || C < 1 || K < 1) return DLMCQ_EINVAL;
  if (H * W > GAP_ROWS || H > GAP_ROWS || W > GAP_ROWS || C % 64 != 0 || C > DLMCQ_GAP_MAX_C || K % 64 != 0 || K >= (1 << 24)) return DLMCQ_EINVAL;
  if (act != DLMCQ_ACT_NONE && act != DLMCQ_ACT_RELU && act != DLMCQ_ACT_RELU6) return DLMCQ_EINVAL;
  ConvEpi ep{};
  const int rc = gap_set_quantiser(ep, codes, q_scale, q_zero_point, q_lo, q_hi, q_form, q_ste_g);
  if (rc != DLMCQ_OK) return rc;
  if (ep.ctl & ~(uint32_t)DLMCQ_ROUTE_ONLY) return DLMCQ_EINVAL;       // (refused, not stripped: this entry point has one kernel and one layout)
  ep.residual = residual;
  ep.relu = act;
  if (N == 0) return DLMCQ_OK;
  if (!x || !w || !(pooled || codes) || !wsum || !in_scale || !w_scale) return DLMCQ_EINVAL;
  if (!aligned16(x) || !aligned16(w) || (pooled && !aligned16(pooled)) || (residual && !aligned16(residual)) || (codes && !aligned4(codes)))
    return DLMCQ_EALIGN;
  if (N * H * W >= (1ll << 31)) return DLMCQ_ERANGE;
  if (ep.ctl & DLMCQ_ROUTE_ONLY) return DLMCQ_ROUTE_GAP;
  GapArgs a{};
  a.x = static_cast<const int8_t*>(x); a.w = w; a.s_w = w_scale; a.wsum = wsum; a.bias = bias; a.s_in = in_scale; a.zp_in = in_zero_point;
  a.pooled = pooled;
  a.N = (int)N; a.HW = (int)(H * W); a.C = (int)C; a.K = (int)K; a.shift = x_is_unsigned ? 128 : 0;
  const GapLaunch r = gap_launch_record(N, (int)C, (int)K, device_cus());
  a.ngroups = r.ngroups;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  return r.nt == 2 ? gap_go<2>(a, ep, r.lds, r.ngroups * r.nslice, st) : gap_go<1>(a, ep, r.lds, r.ngroups * r.nslice, st);
}

// Tests only (not in include/dlmcq.h): the launch record of dlmcq_conv2d_i8_nhwc_gap for N images and C -> K channels on the CU count the
// launcher uses - answer = {slice width, nslice, ngroups, dynamic LDS bytes}.  DLMCQ_EINVAL where the entry point refuses the shape.
extern "C" int dlmcq_x_gap_launch_record(int64_t N, int64_t C, int64_t K, int64_t* answer4) {
  if (!answer4 || N < 1 || C < 1 || K < 1 || C % 64 != 0 || C > DLMCQ_GAP_MAX_C || K % 64 != 0 || K >= (1 << 24)) return DLMCQ_EINVAL;
  const GapLaunch r = gap_launch_record(N, (int)C, (int)K, device_cus());
  answer4[0] = 64 * r.nt; answer4[1] = r.nslice; answer4[2] = r.ngroups; answer4[3] = (int64_t)r.lds;
  return DLMCQ_OK;
}
