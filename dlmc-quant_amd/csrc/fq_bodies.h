// Per-workgroup bodies of the fake-quant forward and backward kernels, shared by the one-tensor launches
// (fake_quant.hip, fq_backward.hip) and the segment-table launches (fake_quant_multi.hip).  Both families call
// exactly these functions, so a tensor gives the same bits whichever launch carries it.  Not part of the ABI.
#pragma once

#include "dlmcq_internal.h"

namespace dlmcq {

// ------------------------------------------------------------------------------------ forward
// Four elements sharing one channel.
template <int FORM>
__device__ __forceinline__ void fq4(const f32x4& v, const ChanConst<FORM>& c, float lo, float hi, f32x4& q, f32x4& y) {
  float q0, q1, q2, q3, y0, y1, y2, y3;
  fq_one<FORM>(v.x, c, lo, hi, q0, y0);
  fq_one<FORM>(v.y, c, lo, hi, q1, y1);
  fq_one<FORM>(v.z, c, lo, hi, q2, y2);
  fq_one<FORM>(v.w, c, lo, hi, q3, y3);
  q = f32x4{q0, q1, q2, q3};
  y = f32x4{y0, y1, y2, y3};
}

// ----------------------------------------------------------------------------------- backward
struct BwdConst {
  float sh;  // the divisor: s^ (QBASE) or s
  float of;  // QBASE: the offset subtracted before the division;  ZEROPOINT: the zero point added after the rounding;
             // ROOTQ_ACT: the upper clip s*(hi - lo)
  float span;  // ROOTQ_ACT: hi - lo
  int form;
  __device__ __forceinline__ BwdConst(float s, float o, float g, int f, float lo, float hi)
      : sh(f == DLMCQ_FORM_QBASE ? ste_scale(s, g) : s),
        of(f == DLMCQ_FORM_SYMMETRIC ? 0.0f : (f == DLMCQ_FORM_ROOTQ_ACT ? s * (hi - lo) : o)), span(hi - lo), form(f) {}
};

// QBASE:      v = (x - o)/s^,  inside = [lo <= v <= hi],              q = R(clamp(v)),  gs += gy*(q - inside*v)
// ZEROPOINT:  u = x/s, a = R(u) + zp, inside = [lo <= a <= hi], t = clamp(a) - zp,       gs += gy*(t - inside*u)
// SYMMETRIC:  ZEROPOINT with zp = 0     (FSPTQuant/base.py:108-109, 149-152 as autograd runs them: the rounding is a
//             straight-through identity, torch.clamp passes the gradient on the closed interval, x/s gives gx = g/s)
// gx = inside ? (gy*s)/s : +0 in all three - the two roundings autograd performs.
__device__ __forceinline__ void bwd_one(float x, float gy, const BwdConst& c, float lo, float hi, float& gx,
                                        float& contrib) {
  float v, q;
  bool inside;
  if (c.form == DLMCQ_FORM_ROOTQ_ACT) {
    // RootQ/base.py:106-111 + function.py:15-20 as autograd runs them: t1 = x + relu(0 - x), t = t1 - relu(t1 - up),
    // u = t/s, y = R(u)*s.  A clipped element passes no gradient to x (gt - gt = +0); the scale collects gy*R(u) from the
    // product, -gy*u from the division and, through up = s*(hi - lo), gy*(hi - lo) from every element clipped above.
    const float t1 = x + relu_nan(0.0f - x);
    const bool below = (0.0f - x) > 0.0f, above = (t1 - c.of) > 0.0f;
    const float t = t1 - relu_nan(t1 - c.of);
    v = t / c.sh;
    q = ste_round(v);
    const float gv = (below || above) ? 0.0f : gy * c.sh;
    gx = gv / c.sh;
    contrib = gy * (q - v) + (above ? gy * c.span : 0.0f);
    return;
  }
  if (c.form == DLMCQ_FORM_QBASE) {
    v = (x - c.of) / c.sh;
    q = ste_round(clamp_nan(v, lo, hi));
    inside = (v >= lo) && (v <= hi);
  } else {
    v = x / c.sh;
    const float a = ste_round(v) + c.of;
    inside = (a >= lo) && (a <= hi);
    q = clamp_nan(a, lo, hi) - c.of;
  }
  const float gv = inside ? gy * c.sh : 0.0f;
  gx = gv / c.sh;                               // bit-exact with autograd's mul-then-div
  // autograd accumulates gy*q and -gv*(v/s) separately; gv*(v/s) == gy*v up to rounding and the scale
  // gradient is an order-dependent sum anyway, so the third division is not spent: gy*(q - [inside]*v)
  contrib = gy * (q - (inside ? v : 0.0f));
}

__device__ __forceinline__ float wave_sum(float s) {
#pragma unroll
  for (int off = DLMCQ_WAVE / 2; off > 0; off >>= 1) s += __shfl_xor(s, off, DLMCQ_WAVE);
  return s;
}

__device__ __forceinline__ float block_sum(float s) {
  __shared__ float part[DLMCQ_BLOCK / DLMCQ_WAVE];
  s = wave_sum(s);
  if ((threadIdx.x & (DLMCQ_WAVE - 1)) == 0) part[threadIdx.x / DLMCQ_WAVE] = s;
  __syncthreads();
  return part[0] + part[1] + part[2] + part[3];
}

// One float4 of x and of gy (already loaded): gx stored at float4 index i, the four contributions added as
// (e0 + e1) + (e2 + e3) - the per-lane order both kernel families share.
__device__ __forceinline__ void bwd_four(const f32x4& xv, const f32x4& gv, float* gx, int64_t i, const BwdConst& c, float lo,
                                         float hi, float& acc) {
  float o0, o1, o2, o3, e0, e1, e2, e3;
  bwd_one(xv.x, gv.x, c, lo, hi, o0, e0);
  bwd_one(xv.y, gv.y, c, lo, hi, o1, e1);
  bwd_one(xv.z, gv.z, c, lo, hi, o2, e2);
  bwd_one(xv.w, gv.w, c, lo, hi, o3, e3);
  const f32x4 o = {o0, o1, o2, o3};
  acc += (e0 + e1) + (e2 + e3);
  if (gx) __builtin_nontemporal_store(o, reinterpret_cast<f32x4*>(gx) + i);
}

// Per tensor, 16-byte aligned pointers: chunk `chunk` of DLMCQ_BLOCK*U float4 (n4 = numel / 4).
template <int U>
__device__ __forceinline__ void bwd_tensor_chunk(const float* x, const float* gy, float* gx, int64_t chunk, int64_t n4,
                                                 const BwdConst& c, float lo, float hi, float& acc) {
  const f32x4* x4 = reinterpret_cast<const f32x4*>(x);
  const f32x4* g4 = reinterpret_cast<const f32x4*>(gy);
  const int64_t i0 = chunk * (DLMCQ_BLOCK * U) + threadIdx.x;
  f32x4 xv[U], gv[U];
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const int64_t i = i0 + u * DLMCQ_BLOCK;
    if (i < n4) {
      xv[u] = __builtin_nontemporal_load(x4 + i);
      gv[u] = __builtin_nontemporal_load(g4 + i);
    }
  }
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const int64_t i = i0 + u * DLMCQ_BLOCK;
    if (i < n4) bwd_four(xv[u], gv[u], gx, i, c, lo, hi, acc);
  }
}

// ... and its 0-3 tail elements, one per lane of the workgroup that owns the first chunk.
__device__ __forceinline__ void bwd_tensor_tail(const float* x, const float* gy, float* gx, int64_t n, const BwdConst& c,
                                                float lo, float hi, float& acc) {
  if (threadIdx.x < (n & 3)) {
    const int64_t i = ((n >> 2) << 2) + threadIdx.x;
    float o, e;
    bwd_one(x[i], gy[i], c, lo, hi, o, e);
    acc += e;
    if (gx) gx[i] = o;
  }
}

// Per channel: one row of `inner` elements at `base`, walked with the workgroup's thread stride.  VEC: aligned pointers and
// inner % 4 == 0.
template <bool VEC>
__device__ __forceinline__ void bwd_row_walk(const float* x, const float* gy, float* gx, int64_t base, int64_t inner,
                                             const BwdConst& k, float lo, float hi, float& acc) {
  if (VEC) {
    const int64_t i4 = inner >> 2;
    for (int64_t i = threadIdx.x; i < i4; i += DLMCQ_BLOCK) {
      const f32x4 xv = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(x + base) + i);
      const f32x4 gv = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(gy + base) + i);
      bwd_four(xv, gv, gx ? gx + base : nullptr, i, k, lo, hi, acc);
    }
  } else {
    for (int64_t i = threadIdx.x; i < inner; i += DLMCQ_BLOCK) {
      float o, e;
      bwd_one(x[base + i], gy[base + i], k, lo, hi, o, e);
      acc += e;
      if (gx) gx[base + i] = o;
    }
  }
}

// Per channel: gscale[c] = g * sum_s partials[s][c], folded in fp64 in a fixed order.
__device__ __forceinline__ float fold_channel(const float* __restrict__ partials, int64_t nseg, int64_t channels, int64_t c,
                                              float g) {
  double s = 0.0;
  for (int64_t k = 0; k < nseg; ++k) s += (double)partials[k * channels + c];
  return (float)s * g;
}

// Per tensor: the whole workgroup folds `n` partials (strided fp64 sums, then a tree through LDS); thread 0 receives the value.
__device__ __forceinline__ float fold_tensor(const float* __restrict__ partials, int64_t n, float g) {
  __shared__ double red[DLMCQ_BLOCK];
  double s = 0.0;
  for (int64_t i = threadIdx.x; i < n; i += DLMCQ_BLOCK) s += (double)partials[i];
  red[threadIdx.x] = s;
  __syncthreads();
  for (int off = DLMCQ_BLOCK / 2; off > 0; off >>= 1) {
    if (threadIdx.x < off) red[threadIdx.x] += red[threadIdx.x + off];
    __syncthreads();
  }
  return (float)red[0] * g;
}

constexpr int FQ_BLOCK = DLMCQ_WAVE;          // forward: one-wave workgroups (see the header comment of fake_quant.hip)
constexpr int BWD_U = 1;                      // one float4 of x and of gy per lane, one chunk per workgroup
constexpr int BWD_TENSOR_BLOCKS = 8192;       // persistent grid: one partial sum per workgroup for the finalize to fold

}  // namespace dlmcq
