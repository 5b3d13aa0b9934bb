// Periodic cells (minimum image) for the capped neighbour list and the edge vectors.
//
// The capped builder of e3k_nlist_body.h (kernel and launchers: the ones the plain cutoff and the criterion form use, with the scan
// of e3k_nlist.hip between the passes) instantiated with PeriodicRule, the rule of e3k_pbc.h.  It gains one output: the three image
// numbers of every edge's destination (edge_cell_shift [e_cap, 3] int32, zero on ghost edges).  The ghost graph is not searched.
//
// Every cell's perpendicular width along a periodic axis must exceed 2 r_max (1 + 1e-3) (the host checks it once, where the cell
// enters): an ordered pair then has at most one image inside the cutoff, the rounded one, and the list keeps one slot per ordered pair.
// Narrower cells (crystal unit cells, several images per pair) are served by the all-images rule of e3k_images.h / e3k_images.hip,
// on request; THIS rule misses pairs on them.  The search stays O(n^2) per graph: no cell list.
//
// The edge-vector kernel recomputes v from the stored integers with the same fmaf chain: its vectors are the builder's bit for bit,
// and its length is the number the builder compared with r_max.
#include "e3k_nlist_body.h"
#include "e3k_pbc.h"

namespace e3k {

// The minimum-image rule of e3k_pbc.h for the builder of e3k_nlist_body.h.  cell, inv_cell [G + 1, 3, 3]; pbc [G + 1, 3].
struct PeriodicRule {
  static constexpr bool SHIFT = true;
  static constexpr bool IMAGES = false;
  const float* cell;
  const float* inv_cell;
  const int32_t* pbc;
  // one wave, one source node, one graph: the graph id is wave-uniform (0 <= g < G < 2^31), and so are the 21 words of its cell
  __device__ __forceinline__ int64_t graph_id(int64_t g) const { return uniform((int)g); }
  template <bool FILL>
  __device__ __forceinline__ PbcCell source(int64_t, int64_t g) const {
    return pbc_load_cell(cell, inv_cell, pbc, g);
  }
  __device__ __forceinline__ bool keep(const PbcCell& c, float px, float py, float pz, const float* __restrict__ pos, int64_t, int64_t j,
                                       float r_max, float n[3]) const {
    const float dx = pos[3 * j] - px, dy = pos[3 * j + 1] - py, dz = pos[3 * j + 2] - pz;
    float v[3];
    pbc_image(c, dx, dy, dz, n);
    pbc_vector(c, dx, dy, dz, n, v);
    return pbc_length(v) < r_max;
  }
  int64_t* scan_rng() const { return nullptr; }
};

// One lane per edge: v = pos[dst] - pos[src] + shift . cell of the source's graph, by the fmaf chain of e3k_pbc.h; len = |v| as the
// builder measured it.  Node ids are clamped to [0, N - 1] and the graph id to [0, n_cells - 1] before they address anything.
__global__ __launch_bounds__(256) void pbc_edge_vector_fwd_kernel(const float* __restrict__ pos, const int32_t* __restrict__ src,
                                                                  const int32_t* __restrict__ dst, const int32_t* __restrict__ shift,
                                                                  const int64_t* __restrict__ node_seg, const float* __restrict__ cell,
                                                                  int32_t n_cells, int64_t N, int64_t E, float* __restrict__ vec,
                                                                  float* __restrict__ len) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= E) return;
  const int64_t s = clampi(src[e], 0, N - 1), d = clampi(dst[e], 0, N - 1);
  const int64_t g = clampi(node_seg[s], 0, n_cells - 1);
  PbcCell c;
#pragma unroll
  for (int k = 0; k < 9; ++k) c.a[k] = cell[9 * g + k];
  const float n[3] = {(float)shift[3 * e], (float)shift[3 * e + 1], (float)shift[3 * e + 2]};
  float v[3];
  pbc_vector(c, pos[3 * d] - pos[3 * s], pos[3 * d + 1] - pos[3 * s + 1], pos[3 * d + 2] - pos[3 * s + 2], n, v);
  vec[3 * e + 0] = v[0];
  vec[3 * e + 1] = v[1];
  vec[3 * e + 2] = v[2];
  if (len) len[e] = pbc_length(v);
}

}  // namespace e3k

extern "C" int e3k_pbc_nlist_count(const float* pos, const int64_t* node_seg, const int64_t* node_ptr, int64_t N, int32_t G, float r_max,
                                   const float* cell, const float* inv_cell, const int32_t* pbc, int32_t* counts, void* stream) {
  if (!cell || !inv_cell || !pbc) return E3K_ERR_INVALID;
  return e3k::nlist_count(pos, node_seg, node_ptr, N, G, r_max, e3k::PeriodicRule{cell, inv_cell, pbc}, counts, stream);
}

extern "C" int e3k_pbc_nlist_fill(const float* pos, const int64_t* node_seg, const int64_t* node_ptr, int64_t N, int32_t G, float r_max,
                                  const float* cell, const float* inv_cell, const int32_t* pbc, const int32_t* counts, int64_t e_cap,
                                  int64_t* offsets, int64_t* edge_index, int32_t* edge_cell_shift, int64_t* n_edges,
                                  int64_t* edge_segment, int64_t* state, int32_t* flag, void* stream) {
  if (!cell || !inv_cell || !pbc) return E3K_ERR_INVALID;
  return e3k::nlist_fill(pos, node_seg, node_ptr, N, G, r_max, e3k::PeriodicRule{cell, inv_cell, pbc}, counts, e_cap, offsets, edge_index,
                         edge_cell_shift, n_edges, edge_segment, state, flag, stream);
}

extern "C" int e3k_pbc_edge_vector_fwd(const float* pos, const int32_t* src, const int32_t* dst, const int32_t* edge_cell_shift,
                                       const int64_t* node_seg, const float* cell, int32_t n_cells, int64_t N, int64_t E,
                                       float* edge_vec, float* edge_len, void* stream) {
  if (E < 0 || N < 0 || n_cells < 0) return E3K_ERR_INVALID;
  if (E == 0) return E3K_OK;
  if (!pos || !src || !dst || !edge_cell_shift || !node_seg || !cell || !edge_vec || N < 1 || n_cells < 1) return E3K_ERR_INVALID;
  hipLaunchKernelGGL(e3k::pbc_edge_vector_fwd_kernel, dim3((unsigned)((E + 255) / 256)), dim3(256), 0, (hipStream_t)stream, pos, src,
                     dst, edge_cell_shift, node_seg, cell, n_cells, N, E, edge_vec, edge_len);
  E3K_CHECK_LAUNCH();
  return E3K_OK;
}
