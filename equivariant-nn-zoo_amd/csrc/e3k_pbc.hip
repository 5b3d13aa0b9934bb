// Periodic cells (minimum image) for the capped neighbour list and the edge vectors.
//
// The capped builder of e3k_nlist.hip with the rule of e3k_pbc.h: same layout (one wave per source node, lanes over the graph's nodes
// 64 at a time, ballot compaction in ascending j), same scan (e3k_nlist.hip's kernel, launched through e3k::nlist_scan_launch), same
// state cells, flag bit, ghost tail and guards -- every store is guarded by its slot index < e_cap, every node id read from the
// batch's bookkeeping is clamped to [0, N] before it is used as an address.  It gains one output: the three image numbers of every
// edge's destination (edge_cell_shift [e_cap, 3] int32, zero on ghost edges).  The ghost graph is not searched.
//
// Every cell's perpendicular width along a periodic axis must exceed 2 r_max (1 + 1e-3) (the host checks it once, where the cell
// enters): an ordered pair then has at most one image inside the cutoff, the rounded one, and the list keeps one slot per ordered pair.
// Narrower cells (crystal unit cells, several images per pair) are not served: the caller replicates to a supercell.  The search
// stays O(n^2) per graph: no cell list.
//
// The edge-vector kernel recomputes v from the stored integers with the same fmaf chain: its vectors are the builder's bit for bit,
// and its length is the number the builder compared with r_max.
#include "e3k_pbc.h"

namespace e3k {

// e3k_nlist.hip: launches nlist_scan_kernel (offsets, per-graph counts, E_real, the overflow report) without criterion cells
int nlist_scan_launch(const int32_t* counts, const int64_t* node_ptr, int64_t N, int32_t G, int64_t e_cap, int64_t* offsets,
                      int64_t* n_edges, int64_t* state, int32_t* flag, hipStream_t stream);

// node_seg [N]: graph of every node; node_ptr [G + 2]: first node of every graph (the ghost graph is graph G); cell, inv_cell
// [G + 1, 3, 3]; pbc [G + 1, 3].
template <bool FILL>
__global__ __launch_bounds__(256) void pbc_nlist_kernel(const float* __restrict__ pos, const int64_t* __restrict__ node_seg,
                                                        const int64_t* __restrict__ node_ptr, int64_t N, int32_t G, float r_max,
                                                        const float* __restrict__ cell, const float* __restrict__ inv_cell,
                                                        const int32_t* __restrict__ pbc, int32_t* __restrict__ counts,
                                                        const int64_t* __restrict__ offsets, int64_t e_cap, int32_t node_blocks,
                                                        int64_t* __restrict__ edge_index, int64_t* __restrict__ edge_seg,
                                                        int32_t* __restrict__ edge_shift) {
  if constexpr (FILL) {
    if ((int)blockIdx.x >= node_blocks) {
      // the ghost tail, as nlist_kernel's: slot k >= E_real holds ghost edge k - E_real; its shift is zero
      const int64_t e_real = offsets[N] < e_cap ? offsets[N] : e_cap;
      const int64_t gs = clampi(node_ptr[G], 0, N);
      const int64_t m = N - gs - 1;      // n_ghost - 1
      const int64_t stride = (int64_t)(gridDim.x - node_blocks) * 256;
      for (int64_t k = e_real + (int64_t)(blockIdx.x - node_blocks) * 256 + threadIdx.x; k < e_cap; k += stride) {
        int64_t s, d;
        if (m >= 1) {
          const int64_t kk = k - e_real, a = kk % m;
          const bool flip = ((kk / m) & 1) != 0;
          s = gs + (flip ? a + 1 : a);
          d = gs + (flip ? a : a + 1);
        } else {      // fewer than two ghost nodes (reported as overflow by the scan): a self loop on the last node, in range
          s = d = N - 1;
        }
        edge_index[k] = s;
        edge_index[e_cap + k] = d;
        if (edge_seg) edge_seg[k] = G;
        edge_shift[3 * k] = 0;
        edge_shift[3 * k + 1] = 0;
        edge_shift[3 * k + 2] = 0;
      }
      return;
    }
  }
  const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= N) return;
  const int lane = threadIdx.x & 63;
  const int64_t g_lane = node_seg[i];
  if (g_lane < 0 || g_lane >= G) {      // the ghost graph (or a bad segment id): not searched
    if constexpr (!FILL) {
      if (lane == 0) counts[i] = 0;
    }
    return;
  }
  // one wave, one source node, one graph: the graph id is wave-uniform (0 <= g < G < 2^31), and so are the 21 words of its cell
  const int64_t g = uniform((int)g_lane);
  const PbcCell c = pbc_load_cell(cell, inv_cell, pbc, g);
  const int64_t beg = clampi(node_ptr[g], 0, N), end = clampi(node_ptr[g + 1], 0, N);
  const float px = pos[3 * i], py = pos[3 * i + 1], pz = pos[3 * i + 2];
  const int64_t off = FILL ? offsets[i] : 0;
  int cnt = 0;
  for (int64_t j0 = beg; j0 < end; j0 += 64) {
    const int64_t j = j0 + lane;
    bool keep = false;
    float n[3] = {0.0f, 0.0f, 0.0f};
    if (j < end && j != i) {
      const float dx = pos[3 * j] - px, dy = pos[3 * j + 1] - py, dz = pos[3 * j + 2] - pz;
      float v[3];
      pbc_image(c, dx, dy, dz, n);
      pbc_vector(c, dx, dy, dz, n, v);
      keep = pbc_length(v) < r_max;
    }
    const unsigned long long mask = __ballot(keep);
    if constexpr (FILL) {
      const int64_t at = off + cnt + __popcll(mask & ((1ull << lane) - 1ull));
      if (keep && at < e_cap) {      // (overflow: the list is cut at e_cap)
        edge_index[at] = i;
        edge_index[e_cap + at] = j;
        if (edge_seg) edge_seg[at] = g;
        edge_shift[3 * at] = (int32_t)n[0];
        edge_shift[3 * at + 1] = (int32_t)n[1];
        edge_shift[3 * at + 2] = (int32_t)n[2];
      }
    }
    cnt += __popcll(mask);
  }
  if constexpr (!FILL) {
    if (lane == 0) counts[i] = cnt;
  }
}

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

static bool pbc_nlist_args_ok(const float* pos, const int64_t* node_seg, const int64_t* node_ptr, int64_t N, int32_t G, const float* cell,
                              const float* inv_cell, const int32_t* pbc) {
  return pos && node_seg && node_ptr && cell && inv_cell && pbc && N >= 1 && N < (int64_t)1 << 31 && G >= 0;
}

extern "C" int e3k_pbc_nlist_count(const float* pos, const int64_t* node_seg, const int64_t* node_ptr, int64_t N, int32_t G, float r_max,
                                   const float* cell, const float* inv_cell, const int32_t* pbc, int32_t* counts, void* stream) {
  if (!pbc_nlist_args_ok(pos, node_seg, node_ptr, N, G, cell, inv_cell, pbc) || !counts) return E3K_ERR_INVALID;
  hipLaunchKernelGGL((e3k::pbc_nlist_kernel<false>), dim3((unsigned)((N + 3) / 4)), dim3(256), 0, (hipStream_t)stream, pos, node_seg,
                     node_ptr, N, G, r_max, cell, inv_cell, pbc, counts, (const int64_t*)nullptr, (int64_t)0, 0, (int64_t*)nullptr,
                     (int64_t*)nullptr, (int32_t*)nullptr);
  E3K_CHECK_LAUNCH();
  return E3K_OK;
}

extern "C" int e3k_pbc_nlist_fill(const float* pos, const int64_t* node_seg, const int64_t* node_ptr, int64_t N, int32_t G, float r_max,
                                  const float* cell, const float* inv_cell, const int32_t* pbc, const int32_t* counts, int64_t e_cap,
                                  int64_t* offsets, int64_t* edge_index, int32_t* edge_cell_shift, int64_t* n_edges,
                                  int64_t* edge_segment, int64_t* state, int32_t* flag, void* stream) {
  if (!pbc_nlist_args_ok(pos, node_seg, node_ptr, N, G, cell, inv_cell, pbc) || !counts || !offsets || !edge_index || !edge_cell_shift ||
      !n_edges || !state || !flag || e_cap < 0 || e_cap >= (int64_t)1 << 31)
    return E3K_ERR_INVALID;
  const int rc = e3k::nlist_scan_launch(counts, node_ptr, N, G, e_cap, offsets, n_edges, state, flag, (hipStream_t)stream);
  if (rc != E3K_OK) return rc;
  const int node_blocks = (int)((N + 3) / 4);
  int64_t tail_blocks = (e_cap + 255) / 256;      // the tail is at most the whole buffer (an empty list)
  if (tail_blocks > 256) tail_blocks = 256;
  if (tail_blocks < 1) tail_blocks = 1;
  hipLaunchKernelGGL((e3k::pbc_nlist_kernel<true>), dim3((unsigned)(node_blocks + tail_blocks)), dim3(256), 0, (hipStream_t)stream, pos,
                     node_seg, node_ptr, N, G, r_max, cell, inv_cell, pbc, (int32_t*)nullptr, (const int64_t*)offsets, e_cap,
                     node_blocks, edge_index, edge_segment, edge_cell_shift);
  E3K_CHECK_LAUNCH();
  return E3K_OK;
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
