// Fake-quant of MANY small tensors in one launch, forward and backward, for gfx950 (MI355X).
//
// A model's weight tensors are 4 KB - 9 MB each: launched one by one they run at a few percent of HBM (the launch, not the
// stream, is what is paid for).  Inside a training step the weights do not change between layers, so all their quantisers
// can run as ONE launch before the first layer and all their backward passes as ONE launch (+ one finalize) after the last.
//
// A device-resident table of segments (include/dlmcq.h: dlmcq_fq_segment) drives three kernels.  A workgroup finds its
// segment from blockIdx.x by binary search over the table's workgroup prefix; the index is wave-uniform and the table is
// const __restrict__, so those reads go through the scalar cache.  It then runs the per-workgroup body of the one-tensor
// kernels (fq_bodies.h) - the geometry of fake_quant.hip (one-wave workgroups, one float4 per lane, one 256-element chunk,
// non-temporal loads and stores) in the forward, the 256-thread workgroups and summation orders of fq_backward.hip in the
// backward - so every segment's y, gx and gscale are the bits of a launch on that tensor alone, by construction.
#include "fq_bodies.h"

namespace dlmcq {

constexpr uint32_t FWD_CHUNK = FQ_BLOCK * 4;               // elements per forward workgroup
constexpr int64_t BWD_CHUNK = (int64_t)DLMCQ_BLOCK * BWD_U * 4;  // elements per per-tensor backward workgroup
constexpr int64_t MULTI_MAX_N = BWD_CHUNK * BWD_TENSOR_BLOCKS;   // 8 388 608: beyond it the one-tensor backward grid-strides

static inline int64_t fwd_chunks(int64_t n) {
  const int64_t c = ((n >> 2) + FQ_BLOCK - 1) / FQ_BLOCK;
  return n == 0 ? 0 : (c < 1 ? 1 : c);
}

// workgroups (= partial sums) of one segment's backward: fq_backward.hip's bwd_plan for outer == 1
__host__ __device__ static inline int64_t bwd_workgroups_of(int64_t n, int64_t channels) {
  if (n == 0) return 0;
  if (channels > 1) return channels;
  const int64_t c = ((n >> 2) + DLMCQ_BLOCK * BWD_U - 1) / (DLMCQ_BLOCK * BWD_U);
  return c < 1 ? 1 : c;
}

__host__ __device__ static inline bool in_backward(const dlmcq_fq_segment& s) {
  return s.n > 0 && s.gy != nullptr && (s.gx != nullptr || s.gscale != nullptr);
}

// The last segment whose workgroup prefix is <= b.  Segments without workgroups share their successor's start, so the last
// of equals is the one that owns b; trailing ones start at the grid size and are never found.  FIELD: byte offset of the prefix.
template <size_t FIELD>
__device__ __forceinline__ int find_segment(const dlmcq_fq_segment* __restrict__ tab, int nseg, uint32_t b) {
  int lo = 0, hi = nseg;   // tab[lo].prefix <= b < tab[hi].prefix (tab[nseg].prefix = the grid size)
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    const int64_t p = *reinterpret_cast<const int64_t*>(reinterpret_cast<const char*>(tab + mid) + FIELD);
    if (p <= (int64_t)b) lo = mid; else hi = mid;
  }
  return lo;
}

// floor(e / d) for e, d < 2^24: both are exact in fp32 and the correctly rounded quotient is off by at most one
__device__ __forceinline__ uint32_t udiv24(uint32_t e, uint32_t d) {
  uint32_t q = (uint32_t)((float)e / (float)d);
  if (q * d > e) --q;
  else if ((q + 1) * d <= e) ++q;
  return q;
}

// ------------------------------------------------------------------------------------ forward
// One 256-element chunk `cx` of one segment; v is this lane's float4 (loaded by the caller when i < n4).
template <int FORM>
__device__ __forceinline__ void fq_multi_body(const dlmcq_fq_segment& sg, const f32x4& v, uint32_t cx, float2* tbl) {
  const float* x = sg.x;
  float* y = sg.y;
  const float* __restrict__ scale = sg.scale;
  const float* __restrict__ offset = sg.offset;
  const uint32_t n = (uint32_t)sg.n, n4 = n >> 2;
  const float lo = (float)(int32_t)sg.lo, hi = (float)(int32_t)sg.hi, g = (float)sg.ste_g;
  const uint32_t i = cx * FQ_BLOCK + threadIdx.x;   // this lane's float4
  const uint32_t r = n & 3;                         // tail elements, finished by the first lanes of the first chunk
  if (sg.channels == 1) {
    const ChanConst<FORM> c(scale[0], offset ? offset[0] : 0.0f, g, lo, hi);
    if (i < n4) {
      f32x4 q, o;
      fq4<FORM>(v, c, lo, hi, q, o);
      __builtin_nontemporal_store(o, reinterpret_cast<f32x4*>(y) + i);
    }
    if (cx == 0 && threadIdx.x < r) {
      float q, o;
      fq_one<FORM>(x[(n4 << 2) + threadIdx.x], c, lo, hi, q, o);
      y[(n4 << 2) + threadIdx.x] = o;
    }
    return;
  }
  const uint32_t inner = (uint32_t)sg.inner;
  if (cx == 0 && threadIdx.x < r) {   // the tail may span rows (inner < 3): each lane takes its own channel's pair
    const uint32_t e = (n4 << 2) + threadIdx.x;
    const uint32_t ch = udiv24(e, inner);
    const ChanConst<FORM> c(scale[ch], offset ? offset[ch] : 0.0f, g, lo, hi);
    float q, o;
    fq_one<FORM>(x[e], c, lo, hi, q, o);
    y[e] = o;
  }
  const uint32_t e0 = cx * FWD_CHUNK;
  const uint32_t e_end = (e0 + FWD_CHUNK < (n4 << 2)) ? e0 + FWD_CHUNK : (n4 << 2);
  if (e_end <= e0) return;            // a segment of fewer than 4 elements: the tail was all of it
  const uint32_t ch0 = udiv24(e0, inner), ch1 = udiv24(e_end - 1, inner);
  if (ch0 == ch1) {
    // the whole chunk lies in one row: (scale, offset) come through the scalar cache and broadcast for free
    const ChanConst<FORM> c(scale[ch0], offset ? offset[ch0] : 0.0f, g, lo, hi);
    if (i < n4) {
      f32x4 q, o;
      fq4<FORM>(v, c, lo, hi, q, o);
      __builtin_nontemporal_store(o, reinterpret_cast<f32x4*>(y) + i);
    }
    return;
  }
  // mixed chunk: stage the (at most 256) rows it touches, then each lane reads its row's pair back
  const uint32_t nrows = ch1 - ch0 + 1;
  for (uint32_t t = threadIdx.x; t < nrows; t += FQ_BLOCK) tbl[t] = make_float2(scale[ch0 + t], offset ? offset[ch0 + t] : 0.0f);
  __syncthreads();
  if (i < n4) {
    const uint32_t e = i << 2;
    uint32_t row = udiv24(e, inner);
    uint32_t rem = e - row * inner;
    f32x4 q, o;
    if (rem + 3 < inner) {            // the float4 lies in one row (always when inner % 4 == 0)
      const float2 so = tbl[row - ch0];
      const ChanConst<FORM> c(so.x, so.y, g, lo, hi);
      fq4<FORM>(v, c, lo, hi, q, o);
    } else {                          // it straddles rows (inner % 4 != 0, e.g. depthwise 3x3): element by element
      const float xv[4] = {v.x, v.y, v.z, v.w};
      float qv[4], ov[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float2 so = tbl[row - ch0];
        const ChanConst<FORM> c(so.x, so.y, g, lo, hi);
        fq_one<FORM>(xv[j], c, lo, hi, qv[j], ov[j]);
        if (++rem == inner) {
          rem = 0;
          ++row;
        }
      }
      o = f32x4{ov[0], ov[1], ov[2], ov[3]};
    }
    __builtin_nontemporal_store(o, reinterpret_cast<f32x4*>(y) + i);
  }
}

__global__ __launch_bounds__(FQ_BLOCK) void fq_multi_kernel(const dlmcq_fq_segment* __restrict__ tab, int nseg) {
  __shared__ float2 tbl[FWD_CHUNK];   // {scale, offset} of the rows a mixed per-channel chunk touches
  const int s = find_segment<offsetof(dlmcq_fq_segment, fwd_chunk0)>(tab, nseg, blockIdx.x);
  const dlmcq_fq_segment sg = tab[s];
  const uint32_t cx = blockIdx.x - (uint32_t)sg.fwd_chunk0;
  // issue the streaming load first; the scale fetch and the row arithmetic overlap its latency
  const uint32_t i = cx * FQ_BLOCK + threadIdx.x;
  f32x4 v = {0.0f, 0.0f, 0.0f, 0.0f};
  if (i < ((uint32_t)sg.n >> 2)) v = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(sg.x) + i);
  __builtin_amdgcn_sched_barrier(0);
  switch ((int)sg.form) {             // uniform per workgroup
    case DLMCQ_FORM_QBASE: fq_multi_body<DLMCQ_FORM_QBASE>(sg, v, cx, tbl); break;
    case DLMCQ_FORM_ZEROPOINT: fq_multi_body<DLMCQ_FORM_ZEROPOINT>(sg, v, cx, tbl); break;
    default: fq_multi_body<DLMCQ_FORM_SYMMETRIC>(sg, v, cx, tbl); break;
  }
}

// ----------------------------------------------------------------------------------- backward
__device__ __forceinline__ float bwd_g(const dlmcq_fq_segment& sg) {
  return sg.form == DLMCQ_FORM_QBASE ? (float)sg.ste_g : 1.0f;   // g scales the QBASE scale gradient only
}

__global__ __launch_bounds__(DLMCQ_BLOCK) void fq_multi_bwd_kernel(const dlmcq_fq_segment* __restrict__ tab, int nseg,
                                                                  float* __restrict__ partials) {
  const int s = find_segment<offsetof(dlmcq_fq_segment, bwd_wg0)>(tab, nseg, blockIdx.x);
  const dlmcq_fq_segment sg = tab[s];
  const int64_t w = (int64_t)blockIdx.x - sg.bwd_wg0;   // per tensor: the chunk;  per channel: the row
  const float lo = (float)(int32_t)sg.lo, hi = (float)(int32_t)sg.hi;
  const float* __restrict__ scale = sg.scale;
  const float* __restrict__ offset = sg.offset;
  float acc = 0.0f;
  if (sg.channels == 1) {
    const BwdConst c(scale[0], offset ? offset[0] : 0.0f, bwd_g(sg), (int)sg.form, lo, hi);
    bwd_tensor_chunk<BWD_U>(sg.x, sg.gy, sg.gx, w, sg.n >> 2, c, lo, hi, acc);
    if (w == 0) bwd_tensor_tail(sg.x, sg.gy, sg.gx, sg.n, c, lo, hi, acc);
  } else {
    const BwdConst k(scale[w], offset ? offset[w] : 0.0f, bwd_g(sg), (int)sg.form, lo, hi);
    if ((sg.inner & 3) == 0)
      bwd_row_walk<true>(sg.x, sg.gy, sg.gx, w * sg.inner, sg.inner, k, lo, hi, acc);
    else
      bwd_row_walk<false>(sg.x, sg.gy, sg.gx, w * sg.inner, sg.inner, k, lo, hi, acc);
  }
  const float sum = block_sum(acc);
  if (threadIdx.x == 0 && sg.gscale) partials[sg.part0 + w] = sum;
}

// One workgroup per segment.  Per tensor: fq_bwd_finalize_tensor_kernel's fold.  Per channel: fq_bwd_finalize_kernel's, one
// partial per channel.  An empty segment's gscale is zero-filled (the one-tensor call's memset).
__global__ __launch_bounds__(DLMCQ_BLOCK) void fq_multi_bwd_finalize_kernel(const dlmcq_fq_segment* __restrict__ tab,
                                                                           const float* __restrict__ partials) {
  const dlmcq_fq_segment sg = tab[blockIdx.x];
  float* gscale = sg.gscale;
  if (!gscale) return;
  if (sg.n == 0) {
    for (int64_t c = threadIdx.x; c < sg.channels; c += DLMCQ_BLOCK) gscale[c] = 0.0f;
    return;
  }
  if (!in_backward(sg)) return;
  const float g = bwd_g(sg);
  if (sg.channels == 1) {
    const float v = fold_tensor(partials + sg.part0, bwd_workgroups_of(sg.n, 1), g);
    if (threadIdx.x == 0) gscale[0] = v;
    return;
  }
  for (int64_t c = threadIdx.x; c < sg.channels; c += DLMCQ_BLOCK)
    gscale[c] = fold_channel(partials + sg.part0, 1, sg.channels, c, g);
}

}  // namespace dlmcq

using namespace dlmcq;

static_assert(sizeof(dlmcq_fq_segment) == 17 * 8, "dlmcq_fq_segment is 17 fields of 8 bytes (include/dlmcq.h)");

extern "C" size_t dlmcq_fq_segment_bytes(void) { return sizeof(dlmcq_fq_segment); }

extern "C" int dlmcq_fq_multi_prepare(dlmcq_fq_segment* segs, int64_t nseg, int64_t* fwd_workgroups, int64_t* bwd_workgroups,
                                      int64_t* finalize_workgroups, size_t* scratch_bytes) {
  if (nseg < 0 || (nseg > 0 && !segs) || !fwd_workgroups || !bwd_workgroups || !finalize_workgroups || !scratch_bytes)
    return DLMCQ_EINVAL;
  if (nseg >= (1ll << 31)) return DLMCQ_ERANGE;
  int64_t fwd = 0, bwd = 0;
  bool any_gscale = false;
  for (int64_t i = 0; i < nseg; ++i) {
    dlmcq_fq_segment& s = segs[i];
    if (s.n < 0 || s.channels < 1 || s.lo > s.hi) return DLMCQ_EINVAL;
    if (s.form != DLMCQ_FORM_QBASE && s.form != DLMCQ_FORM_ZEROPOINT && s.form != DLMCQ_FORM_SYMMETRIC) return DLMCQ_EINVAL;
    if (s.channels > 1 && (s.inner < 0 || s.n != s.channels * s.inner)) return DLMCQ_EINVAL;
    if (s.lo < INT32_MIN || s.hi > INT32_MAX) return DLMCQ_ERANGE;
    if (s.n > MULTI_MAX_N || s.channels > MULTI_MAX_N) return DLMCQ_ERANGE;
    if (s.n > 0 && (!s.x || !s.scale)) return DLMCQ_EINVAL;
    if (!aligned16(s.x) || !aligned16(s.y) || !aligned16(s.gy) || !aligned16(s.gx)) return DLMCQ_EALIGN;
    s.fwd_chunk0 = fwd;
    s.bwd_wg0 = bwd;
    s.part0 = bwd;
    if (s.y) fwd += fwd_chunks(s.n);
    if (in_backward(s)) bwd += bwd_workgroups_of(s.n, s.channels);
    if (s.gscale) any_gscale = true;
  }
  if (fwd >= (1ll << 31) || bwd >= (1ll << 31)) return DLMCQ_ERANGE;
  *fwd_workgroups = fwd;
  *bwd_workgroups = bwd;
  *finalize_workgroups = any_gscale ? nseg : 0;
  *scratch_bytes = any_gscale ? (size_t)bwd * sizeof(float) : 0;
  return DLMCQ_OK;
}

extern "C" int dlmcq_fake_quant_multi_f32(const dlmcq_fq_segment* table, int64_t nseg, int64_t fwd_workgroups,
                                          dlmcq_stream_t stream) {
  if (nseg < 0 || fwd_workgroups < 0) return DLMCQ_EINVAL;
  if (nseg >= (1ll << 31) || fwd_workgroups >= (1ll << 31)) return DLMCQ_ERANGE;
  if (fwd_workgroups == 0) return DLMCQ_OK;
  if (!table || nseg == 0) return DLMCQ_EINVAL;
  if ((((uintptr_t)table) & 7u) != 0) return DLMCQ_EALIGN;
  hipLaunchKernelGGL(fq_multi_kernel, dim3((uint32_t)fwd_workgroups), dim3(FQ_BLOCK), 0, reinterpret_cast<hipStream_t>(stream),
                     table, (int)nseg);
  return launch_status();
}

extern "C" int dlmcq_fake_quant_multi_bwd_f32(const dlmcq_fq_segment* table, int64_t nseg, int64_t bwd_workgroups,
                                              int64_t finalize_workgroups, void* scratch, size_t scratch_bytes,
                                              dlmcq_stream_t stream) {
  if (nseg < 0 || bwd_workgroups < 0 || (finalize_workgroups != 0 && finalize_workgroups != nseg)) return DLMCQ_EINVAL;
  if (nseg >= (1ll << 31) || bwd_workgroups >= (1ll << 31)) return DLMCQ_ERANGE;
  if (bwd_workgroups == 0 && finalize_workgroups == 0) return DLMCQ_OK;
  if (!table) return DLMCQ_EINVAL;
  if ((((uintptr_t)table) & 7u) != 0) return DLMCQ_EALIGN;
  const size_t need = finalize_workgroups ? (size_t)bwd_workgroups * sizeof(float) : 0;
  if (need && (!scratch || scratch_bytes < need || !aligned4(scratch))) return DLMCQ_ESCRATCH;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  float* part = reinterpret_cast<float*>(scratch);
  if (bwd_workgroups > 0) {
    hipLaunchKernelGGL(fq_multi_bwd_kernel, dim3((uint32_t)bwd_workgroups), dim3(DLMCQ_BLOCK), 0, st, table, (int)nseg, part);
    const int rc = launch_status();
    if (rc != DLMCQ_OK) return rc;
  }
  if (finalize_workgroups > 0) {
    hipLaunchKernelGGL(fq_multi_bwd_finalize_kernel, dim3((uint32_t)finalize_workgroups), dim3(DLMCQ_BLOCK), 0, st, table,
                       part);
    return launch_status();
  }
  return DLMCQ_OK;
}
