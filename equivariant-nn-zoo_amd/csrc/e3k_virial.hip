// The strain derivative of the energy for gfx950: per graph, the sum over the graph's edges of (edge vector) x (energy gradient with
// respect to that vector), from the operands of the force backward (e3k_edge_vector_bwd) -- include/e3k.h, "Virial".
//
// An O(E) stream of 28 B per edge; one workgroup per graph, no atomics: the same bits every run.
#include "e3k_common.h"

namespace e3k {

// One workgroup of 256 per graph g.  Nodes are sorted by graph, so the graph's edges are the slots [src_ptr[node_ptr[g]],
// src_ptr[node_ptr[g + 1]]) of the by-source CSR: lane k takes the slots t0 + k, t0 + k + 256, ...  Per edge
// g_e = fmaf(len > 0 ? g_len / len : 0, vec, g_vec) in fp32 -- edge_vector_bwd_kernel's expression, so that forces and virial come
// from the same numbers -- and the nine products vec[a] g_e[b] are formed and summed in double (a product of two floats is exact
// there).  The lanes' sums are added in a fixed shape: six shuffle levels inside a wavefront, then the four wave partials in order.
// out[g, 3 a + b] = -sum as fp32 (the virial; written, never accumulated: a graph without edges gets nine zeros).  The graph's bounds
// are uniform over the workgroup; every index read from memory is clamped to its table, so a bad table reads nothing outside it.
__global__ __launch_bounds__(256) void virial_edges_kernel(const float* __restrict__ g_vec, const float* __restrict__ g_len,
                                                           const float* __restrict__ vec, const float* __restrict__ len,
                                                           const int32_t* __restrict__ src_ptr, const int32_t* __restrict__ src_perm,
                                                           const int32_t* __restrict__ graph_ptr, int64_t N, int64_t E,
                                                           float* __restrict__ out) {
  __shared__ double part[4][9];
  int64_t n0 = graph_ptr[blockIdx.x], n1 = graph_ptr[blockIdx.x + 1];
  n1 = n1 < 0 ? 0 : n1 > N ? N : n1;
  n0 = n0 < 0 ? 0 : n0 > n1 ? n1 : n0;
  int64_t t0 = src_ptr[n0], t1 = src_ptr[n1];
  t1 = t1 < 0 ? 0 : t1 > E ? E : t1;
  t0 = t0 < 0 ? 0 : t0 > t1 ? t1 : t0;
  double acc[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) acc[k] = 0.0;
  // (a round is two dependent loads, slot -> edge -> operands, about 1 us: a long graph is bound by that latency.  Four slots per
  // trip in the same lane order measured no faster, 31.9 us against 28.9 on 28 rounds; slices over several workgroups would be.)
  for (int64_t t = t0 + threadIdx.x; t < t1; t += 256) {
    int64_t e = src_perm[t];
    e = e < 0 ? 0 : e >= E ? E - 1 : e;
    const float v[3] = {vec[3 * e + 0], vec[3 * e + 1], vec[3 * e + 2]};
    float g[3] = {g_vec ? g_vec[3 * e + 0] : 0.f, g_vec ? g_vec[3 * e + 1] : 0.f, g_vec ? g_vec[3 * e + 2] : 0.f};
    if (g_len) {
      const float l = len[e];
      const float f = l > 0.f ? g_len[e] / l : 0.f;
      g[0] = fmaf(f, v[0], g[0]);
      g[1] = fmaf(f, v[1], g[1]);
      g[2] = fmaf(f, v[2], g[2]);
    }
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
      for (int b = 0; b < 3; ++b) acc[3 * a + b] += (double)v[a] * (double)g[b];
  }
#pragma unroll
  for (int k = 0; k < 9; ++k) {
    double s = acc[k];
    for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6][k] = s;
  }
  __syncthreads();
  if (threadIdx.x < 9) {
    double total = 0.0;
    for (int w = 0; w < 4; ++w) total += part[w][threadIdx.x];
    out[9 * (int64_t)blockIdx.x + threadIdx.x] = (float)(-total);
  }
}

}  // namespace e3k

extern "C" int e3k_virial_edges(const float* g_vec, const float* g_len, const float* edge_vec, const float* edge_len,
                                const int32_t* src_ptr, const int32_t* src_perm, const int32_t* graph_ptr, int64_t N, int64_t E,
                                int32_t G, float* out, void* stream) {
  if (N < 0 || E < 0 || G < 0 || N >= (int64_t)1 << 31 || E >= (int64_t)1 << 31) return E3K_ERR_INVALID;
  if (G == 0) return E3K_OK;
  if (!out || !graph_ptr || !src_ptr) return E3K_ERR_INVALID;
  if (E > 0) {
    if (!edge_vec || !src_perm || (!g_vec && !g_len)) return E3K_ERR_INVALID;
    if (g_len && !edge_len) return E3K_ERR_INVALID;
  }
  // (E == 0: every graph's slot range is empty and the one launch writes the zeros)
  hipLaunchKernelGGL(e3k::virial_edges_kernel, dim3((unsigned)G), dim3(256), 0, (hipStream_t)stream, g_vec, g_len, edge_vec, edge_len,
                     src_ptr, src_perm, graph_ptr, N, E, out);
  E3K_CHECK_LAUNCH();
  return E3K_OK;
}
