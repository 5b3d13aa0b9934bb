// Padded collation on the device for gfx950 (data/device_store.py, run/graph_step.CollatedStep): a batch of G graphs gathered
// from a store that lives in HBM and padded with one ghost graph to the bucket's (n_cap, e_cap) -- bit for bit what
// run/graph_step.pad_batch(store.index_select(ids), n_cap, e_cap) builds on the host with Batch.from_data_list (the reference's
// collate, e3_layers/data/dataloader.py:30-45).  Two launches with shapes fixed by the bucket, so both can sit in a HIP graph:
//   plan     one workgroup: the chosen graphs' node / edge counts -> exclusive scans (where each graph lands in the batch), the
//            per-graph counts and weights of the batch, the capacity / id checks
//   gather   one wave per (graph slot, field): a graph's rows are contiguous in the store and in the batch, so every unit is one
//            byte range (16-byte accesses where source and destination share their alignment), edge_index re-based and widened,
//            the segment ids and node weights generated, the ghost graph's rows written as pad_batch's ghost_sample makes them.
#include "e3k_common.h"

namespace e3k {

constexpr int32_t COLLATE_BAD = 16;      // bit of the persistent flag (bits 1, 4, 8: edge endpoints, one-hot types, table keys)

// work (int64) layout for G slots
__host__ __device__ __forceinline__ int64_t cw_node_off(int32_t) { return 0; }                        // [G + 1]
__host__ __device__ __forceinline__ int64_t cw_edge_off(int32_t G) { return (int64_t)G + 1; }         // [G + 1]
__host__ __device__ __forceinline__ int64_t cw_src_node(int32_t G) { return 2 * (int64_t)G + 2; }     // [G]
__host__ __device__ __forceinline__ int64_t cw_src_edge(int32_t G) { return 3 * (int64_t)G + 2; }     // [G]
__host__ __device__ __forceinline__ int64_t cw_src_graph(int32_t G) { return 4 * (int64_t)G + 2; }    // [G] (-1: none)
__host__ __device__ __forceinline__ int64_t cw_first(int32_t G) { return 5 * (int64_t)G + 2; }        // [2] ghost's source rows

__device__ __forceinline__ int64_t shfl_up64(int64_t v, int off) {
  const int lo = __shfl_up((int)(uint32_t)(uint64_t)v, off, 64);
  const int hi = __shfl_up((int)(uint32_t)((uint64_t)v >> 32), off, 64);
  return (int64_t)(((uint64_t)(uint32_t)hi << 32) | (uint32_t)lo);
}

// inclusive block scan of one int64 per thread (1024 threads); *total = the sum over the block
__device__ int64_t block_scan64(int64_t v, int64_t* wave_tot, int64_t* total) {
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  int64_t x = v;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const int64_t y = shfl_up64(x, off);
    if (lane >= off) x += y;
  }
  if (lane == 63) wave_tot[w] = x;
  __syncthreads();
  int64_t before = 0;
  for (int k = 0; k < w; ++k) before += wave_tot[k];
  if (t == 1023) *total = before + x;
  __syncthreads();
  return before + x;
}

__global__ __launch_bounds__(1024) void collate_plan_kernel(const int32_t* __restrict__ ids, int32_t G,
                                                            const int64_t* __restrict__ node_off, const int64_t* __restrict__ edge_off,
                                                            int64_t S, int64_t n_cap, int64_t e_cap, int64_t* __restrict__ work,
                                                            int64_t* __restrict__ n_nodes, int64_t* __restrict__ n_edges,
                                                            float* __restrict__ graph_weight, int32_t* __restrict__ flag) {
  __shared__ int64_t wave_tot[2][16];
  __shared__ int64_t tot[2];
  const int t = threadIdx.x;
  int64_t nc = 0, ec = 0, sn = 0, se = 0, sg = -1;
  int bad_id = 0;
  if (t < G) {
    const int64_t id = ids[t];
    if (id >= 0 && id < S) {      // (nothing is read through an id outside the store)
      sn = node_off[id];
      nc = node_off[id + 1] - sn;
      se = edge_off[id];
      ec = edge_off[id + 1] - se;
      sg = id;
    } else {
      bad_id = 1;
    }
  }
  const int64_t incl_n = block_scan64(nc, wave_tot[0], &tot[0]);
  const int64_t incl_e = block_scan64(ec, wave_tot[1], &tot[1]);
  const int64_t n = tot[0], e = tot[1];
  const bool bad = __syncthreads_or(bad_id) || n + 2 > n_cap || e > e_cap;
  int64_t ex_n = incl_n - nc, ex_e = incl_e - ec, n_real = n, e_real = e;
  if (bad) {                      // G empty graphs + a ghost that fills the bucket: in bounds whatever the ids were
    nc = ec = sn = se = ex_n = ex_e = n_real = e_real = 0;
    sg = -1;
    if (t == 0) atomicOr(flag, COLLATE_BAD);
  }
  if (t < G) {
    work[cw_node_off(G) + t] = ex_n;
    work[cw_edge_off(G) + t] = ex_e;
    work[cw_src_node(G) + t] = sn;
    work[cw_src_edge(G) + t] = se;
    work[cw_src_graph(G) + t] = sg;
    n_nodes[t] = nc;
    n_edges[t] = ec;
    graph_weight[t] = (float)(1.0 / (double)G);
  }
  if (t == 0) {                   // ghost_sample's `like` is the first real graph: its first node / edge row (-1: it has none)
    work[cw_node_off(G) + G] = n_real;
    work[cw_edge_off(G) + G] = e_real;
    work[cw_first(G)] = nc > 0 ? sn : -1;
    work[cw_first(G) + 1] = ec > 0 ? se : -1;
    n_nodes[G] = n_cap - n_real;
    n_edges[G] = e_cap - e_real;
    graph_weight[G] = 0.0f;
  }
}

struct CollateArgs {
  e3k_collate_field f[E3K_COLLATE_MAX_FIELDS];
  const int64_t* work;
  int64_t n_cap, e_cap;
  int32_t n_fields, G;
};

// wave copy of nbytes (a multiple of 4; both pointers 4-byte aligned)
__device__ __forceinline__ void wave_copy(char* __restrict__ dst, const char* __restrict__ src, int64_t nbytes, int lane) {
  if (nbytes <= 0) return;
  if (((reinterpret_cast<uintptr_t>(dst) ^ reinterpret_cast<uintptr_t>(src)) & 15) == 0) {
    int64_t head = (16 - (reinterpret_cast<uintptr_t>(dst) & 15)) & 15;
    if (head > nbytes) head = nbytes;
    if (4 * lane < head) reinterpret_cast<uint32_t*>(dst)[lane] = reinterpret_cast<const uint32_t*>(src)[lane];
    const int64_t n16 = (nbytes - head) >> 4;
    const uint4* __restrict__ s4 = reinterpret_cast<const uint4*>(src + head);
    uint4* __restrict__ d4 = reinterpret_cast<uint4*>(dst + head);
    for (int64_t i = lane; i < n16; i += 64) d4[i] = s4[i];
    const int64_t t0 = head + (n16 << 4);
    if (t0 + 4 * lane < nbytes) reinterpret_cast<uint32_t*>(dst + t0)[lane] = reinterpret_cast<const uint32_t*>(src + t0)[lane];
  } else {
    const int64_t nw = nbytes >> 2;
    const uint32_t* __restrict__ s = reinterpret_cast<const uint32_t*>(src);
    uint32_t* __restrict__ d = reinterpret_cast<uint32_t*>(dst);
    for (int64_t i = lane; i < nw; i += 64) d[i] = s[i];
  }
}

// rows x row_bytes of dst = the row at `row` repeated (row == nullptr: zeros)
__device__ __forceinline__ void wave_repeat(char* __restrict__ dst, const char* __restrict__ row, int64_t row_bytes, int64_t rows,
                                            int lane) {
  const int32_t rw = (int32_t)(row_bytes >> 2), nw = (int32_t)(rw * rows);      // (ghost rows: a few thousand words at most)
  const uint32_t* __restrict__ r = reinterpret_cast<const uint32_t*>(row);
  uint32_t* __restrict__ d = reinterpret_cast<uint32_t*>(dst);
  for (int32_t i = lane; i < nw; i += 64) d[i] = row ? r[i % rw] : 0u;
}

__global__ __launch_bounds__(256) void collate_gather_kernel(const CollateArgs a) {
  const int lane = threadIdx.x & 63;
  const int64_t unit = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int G = a.G, nf = a.n_fields;
  if (unit >= (int64_t)(G + 1) * nf) return;
  const int slot = uniform((int)(unit / nf)), fi = uniform((int)(unit % nf));
  const int64_t* __restrict__ work = a.work;
  const bool ghost = slot == G;
  const int64_t beg_n = work[cw_node_off(G) + slot], beg_e = work[cw_edge_off(G) + slot];
  const int64_t cnt_n = ghost ? a.n_cap - beg_n : work[cw_node_off(G) + slot + 1] - beg_n;
  const int64_t cnt_e = ghost ? a.e_cap - beg_e : work[cw_edge_off(G) + slot + 1] - beg_e;
  const e3k_collate_field& f = a.f[fi];
  switch (f.kind) {
    case E3K_COLLATE_NODE:
    case E3K_COLLATE_EDGE: {
      const bool node = f.kind == E3K_COLLATE_NODE;
      const int64_t rb = f.row_bytes, cnt = node ? cnt_n : cnt_e;
      char* dst = static_cast<char*>(f.dst) + (node ? beg_n : beg_e) * rb;
      const char* src = static_cast<const char*>(f.src);
      if (!ghost) {
        wave_copy(dst, src + work[(node ? cw_src_node(G) : cw_src_edge(G)) + slot] * rb, cnt * rb, lane);
      } else if (f.ghost == E3K_COLLATE_GHOST_TABLE) {
        wave_copy(dst, static_cast<const char*>(f.table), cnt * rb, lane);
      } else {
        const int64_t first = work[cw_first(G) + (node ? 0 : 1)];
        wave_repeat(dst, first >= 0 ? src + first * rb : nullptr, rb, cnt, lane);
      }
      break;
    }
    case E3K_COLLATE_GRAPH: {
      const int64_t rb = f.row_bytes, sg = ghost ? -1 : work[cw_src_graph(G) + slot];
      char* dst = static_cast<char*>(f.dst) + (int64_t)slot * rb;
      if (sg >= 0) wave_copy(dst, static_cast<const char*>(f.src) + sg * rb, rb, lane);
      else wave_repeat(dst, nullptr, rb, 1, lane);
      break;
    }
    case E3K_COLLATE_EDGE_INDEX: {
      int64_t* __restrict__ d0 = static_cast<int64_t*>(f.dst) + beg_e;
      int64_t* __restrict__ d1 = d0 + f.dst_ld;
      if (!ghost) {
        const int32_t* __restrict__ s0 = static_cast<const int32_t*>(f.src) + work[cw_src_edge(G) + slot];
        const int32_t* __restrict__ s1 = s0 + f.src_ld;
        // four rounds of loads in flight before the first store (a graph's edges are a few hundred: 1-5 rounds of 64)
        for (int64_t j0 = 0; j0 < cnt_e; j0 += 256) {
          int32_t v0[4], v1[4];
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            const int64_t j = j0 + u * 64 + lane;
            v0[u] = j < cnt_e ? s0[j] : 0;
            v1[u] = j < cnt_e ? s1[j] : 0;
          }
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            const int64_t j = j0 + u * 64 + lane;
            if (j < cnt_e) {
              d0[j] = (int64_t)v0[u] + beg_n;
              d1[j] = (int64_t)v1[u] + beg_n;
            }
          }
        }
      } else {      // ghost_sample: edge k joins ghost nodes a, a + 1 (a = k mod (n_ghost - 1)), direction flipping every lap
        const int32_t m = cnt_n - 1 > 1 ? (int32_t)(cnt_n - 1) : 1;
        for (int32_t k = lane; k < (int32_t)cnt_e; k += 64) {      // (e_cap < 2^31: 32-bit division)
          const int32_t a32 = k % m;
          const bool flip = ((k / m) & 1) != 0;
          d0[k] = beg_n + (flip ? a32 + 1 : a32);
          d1[k] = beg_n + (flip ? a32 : a32 + 1);
        }
      }
      break;
    }
    case E3K_COLLATE_NODE_SEGMENT: {
      int64_t* __restrict__ d = static_cast<int64_t*>(f.dst) + beg_n;
      for (int64_t j = lane; j < cnt_n; j += 64) d[j] = slot;
      break;
    }
    case E3K_COLLATE_EDGE_SEGMENT: {
      int64_t* __restrict__ d = static_cast<int64_t*>(f.dst) + beg_e;
      for (int64_t j = lane; j < cnt_e; j += 64) d[j] = slot;
      break;
    }
    case E3K_COLLATE_NODE_WEIGHT: {
      float* __restrict__ d = static_cast<float*>(f.dst) + beg_n;
      const float w = ghost ? 0.0f : (float)(1.0 / (double)work[cw_node_off(G) + G]);
      for (int64_t j = lane; j < cnt_n; j += 64) d[j] = w;
      break;
    }
    default:
      break;
  }
}

}  // namespace e3k

extern "C" int64_t e3k_collate_work_ints(int32_t G) { return 5 * (int64_t)G + 4; }

extern "C" int e3k_collate_plan(const int32_t* ids, int32_t G, const int64_t* node_off, const int64_t* edge_off, int64_t S,
                                int64_t n_cap, int64_t e_cap, int64_t* work, int64_t* n_nodes, int64_t* n_edges, float* graph_weight,
                                int32_t* flag, void* stream) {
  if (G < 1 || G > 1024 || S < 1 || n_cap < 2 || e_cap < 0 || n_cap >= (int64_t)1 << 31 || e_cap >= (int64_t)1 << 31) return E3K_ERR_INVALID;
  if (!ids || !node_off || !edge_off || !work || !n_nodes || !n_edges || !graph_weight || !flag) return E3K_ERR_INVALID;
  hipLaunchKernelGGL(e3k::collate_plan_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, ids, G, node_off, edge_off, S, n_cap,
                     e_cap, work, n_nodes, n_edges, graph_weight, flag);
  E3K_CHECK_LAUNCH();
  return E3K_OK;
}

extern "C" int e3k_collate_gather(const e3k_collate_field* fields, int32_t n_fields, int32_t G, int64_t n_cap, int64_t e_cap,
                                  const int64_t* work, void* stream) {
  if (!fields || !work || n_fields < 1 || n_fields > E3K_COLLATE_MAX_FIELDS || G < 1 || G > 1024 || n_cap < 2 || e_cap < 0 ||
      n_cap >= (int64_t)1 << 31 || e_cap >= (int64_t)1 << 31)
    return E3K_ERR_INVALID;
  e3k::CollateArgs a = {};
  for (int i = 0; i < n_fields; ++i) {
    const e3k_collate_field& f = fields[i];
    if (f.kind < E3K_COLLATE_NODE || f.kind > E3K_COLLATE_NODE_WEIGHT || !f.dst) return E3K_ERR_INVALID;
    const bool rows = f.kind <= E3K_COLLATE_GRAPH;
    if (rows && (f.row_bytes <= 0 || (f.row_bytes & 3))) return E3K_ERR_INVALID;      // (src may be NULL: an empty store field)
    if (rows && ((reinterpret_cast<uintptr_t>(f.src) | reinterpret_cast<uintptr_t>(f.dst)) & 3)) return E3K_ERR_INVALID;
    if (f.kind != E3K_COLLATE_GRAPH && rows && f.ghost == E3K_COLLATE_GHOST_TABLE &&
        (!f.table || (reinterpret_cast<uintptr_t>(f.table) & 3)))
      return E3K_ERR_INVALID;
    if (f.kind == E3K_COLLATE_EDGE_INDEX && (f.src_ld < 0 || f.dst_ld < e_cap)) return E3K_ERR_INVALID;
    a.f[i] = f;
  }
  a.work = work;
  a.n_cap = n_cap;
  a.e_cap = e_cap;
  a.n_fields = n_fields;
  a.G = G;
  const int64_t units = (int64_t)(G + 1) * n_fields;
  hipLaunchKernelGGL(e3k::collate_gather_kernel, dim3((unsigned)((units + 3) / 4)), dim3(256), 0, (hipStream_t)stream, a);
  E3K_CHECK_LAUNCH();
  return E3K_OK;
}
