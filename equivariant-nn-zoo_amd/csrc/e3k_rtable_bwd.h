// The transposed knot-table interpolation, pass 1: one text for rtable_bwd_partial_kernel (e3k_rtable.hip) and for the launch that
// runs it beside the weight-gradient GEMM (e3k_wgrad_rider.hip).
#pragma once
#include "e3k_common.h"

namespace e3k {

typedef float f32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ void nt_store4(float4* p, const float4& v) {
  f32x4 t = {v.x, v.y, v.z, v.w};
  __builtin_nontemporal_store(t, reinterpret_cast<f32x4*>(p));
}
__device__ __forceinline__ float4 nt_load4(const float4* p) {
#ifdef E3K_NO_NT      // (experiment builds: tools/micro/nt_policy.sh)
  return *p;
#else
  const f32x4 t = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(p));
  return make_float4(t.x, t.y, t.z, t.w);
#endif
}

constexpr int RT_SEG = 64;          // edges of one knot summed by one wave of the transpose

// backward, pass 1: one wave per (segment of <= RT_SEG edges of ONE knot b, 256-column chunk) reads the g_w rows of its edges
// ONCE (ascending edge id) and forms their four weighted sums -- the segment's contributions to the table rows b-1 .. b+2:
// P[segment][0..3][cols].  scale [E] (optional): every edge's weights are multiplied by scale[e] (force training: the slope
// table's gradient is the transpose applied with the radius' cotangent as per-edge factor).
// `block`: the workgroup's index among the transpose's workgroups.  ROWS: g_w rows in flight per wave (a multiple of 8); whatever it
// is, every accumulator sums its edges in ascending edge order -- the same bits.
template <int ROWS>
__device__ __forceinline__ void rtable_bwd_partial_body(const float* __restrict__ gw, const float* __restrict__ coef,
                                                        const float* __restrict__ scale, const int32_t* __restrict__ ptr,
                                                        const int32_t* __restrict__ seg, const int32_t* __restrict__ perm, int32_t K,
                                                        int32_t W, int32_t n_chunks, int64_t n_seg_cap, float* __restrict__ P,
                                                        int64_t block) {
  const int64_t item = block * 4 + (threadIdx.x >> 6);
  if (item >= n_seg_cap * n_chunks) return;
  const int s = uniform((int)(item / n_chunks)), chunk = uniform((int)(item - (int64_t)s * n_chunks));
  if (s >= uniform(seg[K + 1])) return;
  int lo = 0, hi = K + 1;                     // the knot whose segment range holds s: seg[b] <= s < seg[b + 1]
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (uniform(seg[mid]) <= s) lo = mid; else hi = mid;
  }
  const int b = lo;
  const int lane = threadIdx.x & 63;
  const int col = chunk * 256 + lane * 4;
  const bool live = col < W;                  // (lanes past the last column stay: they hold edges' ids and weights for the others)
  const int beg = uniform(ptr[b]) + (s - uniform(seg[b])) * RT_SEG;
  const int end_b = uniform(ptr[b + 1]);
  const int end = beg + RT_SEG < end_b ? beg + RT_SEG : end_b;
  float4 a0 = make_float4(0.f, 0.f, 0.f, 0.f), a1 = a0, a2 = a0, a3 = a0;
  // Lane l fetches edge l's id and weights ONCE (a segment has at most 64 edges); the loop then reads them across lanes and has no
  // load that depends on another: ROWS (eight in the stand-alone kernel) independent g_w rows are in flight per wave.  (Round 4's loop fetched id -> weights -> row
  // per edge, four edges at a time: a chain of three latencies per batch, 4.0 TB/s.)  Sums in ascending edge order, as before.
  const int n = end - beg;
  int e_l = 0;
  float4 c_l = make_float4(0.f, 0.f, 0.f, 0.f);
  if (lane < n) {
    e_l = perm[beg + lane];
    c_l = *reinterpret_cast<const float4*>(coef + 4 * (int64_t)e_l);
    if (scale) {
      const float sc = scale[e_l];
      c_l.x *= sc; c_l.y *= sc; c_l.z *= sc; c_l.w *= sc;
    }
  }
  auto row_of = [&](int k) {
    const int e = __builtin_amdgcn_readlane(e_l, k);
    return live ? nt_load4(reinterpret_cast<const float4*>(gw + (int64_t)e * W + col)) : make_float4(0.f, 0.f, 0.f, 0.f);      // read once
  };
  auto acc = [&](int k, const float4& g) {
    const float c0 = __uint_as_float(__builtin_amdgcn_readlane((int)__float_as_uint(c_l.x), k));
    const float c1 = __uint_as_float(__builtin_amdgcn_readlane((int)__float_as_uint(c_l.y), k));
    const float c2 = __uint_as_float(__builtin_amdgcn_readlane((int)__float_as_uint(c_l.z), k));
    const float c3 = __uint_as_float(__builtin_amdgcn_readlane((int)__float_as_uint(c_l.w), k));
    a0.x = fmaf(c0, g.x, a0.x); a0.y = fmaf(c0, g.y, a0.y); a0.z = fmaf(c0, g.z, a0.z); a0.w = fmaf(c0, g.w, a0.w);
    a1.x = fmaf(c1, g.x, a1.x); a1.y = fmaf(c1, g.y, a1.y); a1.z = fmaf(c1, g.z, a1.z); a1.w = fmaf(c1, g.w, a1.w);
    a2.x = fmaf(c2, g.x, a2.x); a2.y = fmaf(c2, g.y, a2.y); a2.z = fmaf(c2, g.z, a2.z); a2.w = fmaf(c2, g.w, a2.w);
    a3.x = fmaf(c3, g.x, a3.x); a3.y = fmaf(c3, g.y, a3.y); a3.z = fmaf(c3, g.z, a3.z); a3.w = fmaf(c3, g.w, a3.w);
  };
  int k = 0;
  for (; k + ROWS <= n; k += ROWS) {
    float4 g[ROWS];
#pragma unroll
    for (int u = 0; u < ROWS; ++u) g[u] = row_of(k + u);
#pragma unroll
    for (int u = 0; u < ROWS; ++u) acc(k + u, g[u]);
  }
  if constexpr (ROWS > 8) {
    if (k + 8 <= n) {
      float4 g[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) g[u] = row_of(k + u);
#pragma unroll
      for (int u = 0; u < 8; ++u) acc(k + u, g[u]);
      k += 8;
    }
  }
  if (k + 4 <= n) {
    float4 g[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) g[u] = row_of(k + u);
#pragma unroll
    for (int u = 0; u < 4; ++u) acc(k + u, g[u]);
    k += 4;
  }
  for (; k < n; ++k) {
    const float4 g = row_of(k);
    acc(k, g);
  }
  if (!live) return;
  float* row = P + (int64_t)s * 4 * W + col;
  *reinterpret_cast<float4*>(row) = a0;
  *reinterpret_cast<float4*>(row + W) = a1;
  *reinterpret_cast<float4*>(row + 2 * W) = a2;
  *reinterpret_cast<float4*>(row + 3 * W) = a3;
}

// host side (e3k_rtable.hip)
inline int64_t rtable_seg_cap(int64_t E, int32_t K) { return E / RT_SEG + (int64_t)K + 2; }
// pass 2 (rtable_bwd_combine_kernel) on `stream`
void rtable_bwd_combine(const float* P, const int32_t* bin_seg, int32_t K, int32_t W, int32_t accumulate, float* g_T, hipStream_t stream);

}  // namespace e3k
