// Capped neighbour list: what a force evaluation (run/md.py), a sampling step or a score step needs in front of the model when
// the atoms move.
//
// The capped list is the radius graph of e3k_edge.hip (same distance test -- within_cutoff of e3k_common.h -- and edge order) written into a FIXED [2, e_cap]
// buffer: nothing about its size goes to the host, so the build is part of a captured HIP graph.  The batch is one padded by
// run/graph_step.pad_batch -- its last graph is the ghost graph, which is not searched; the slots behind the real edges are
// filled with the ghost edges run/graph_step.ghost_sample defines, so that for positions that fit the buffer equals
// pad_batch(batch with computeEdgeIndex's edges, n_cap, e_cap)["edge_index"] bit for bit.
//
// Three launches: count (one wave per source node), scan (one workgroup: offsets, per-graph counts, E_real, the overflow
// report), fill (node waves + tail blocks).  Every store is guarded by its slot index < e_cap; every node id read from the
// batch's own bookkeeping is clamped to [0, N] before it is used as an address.
//
// The criterion form (e3k_nlist_count_crit / _fill_crit) keeps a pair that is inside the cutoff OR that the declarative pair rule of
// data/compute_edge.SequenceOrRandom keeps: same segment key and |i - j| < window, or a counter-based Bernoulli draw -- the 32-bit
// pair hash of e3k_draw.h over (seed, draw index, i, j) below a threshold.  The draw index is the number of the build: count reads rng[0], the scan (one
// workgroup, between the two passes) copies it to rng[1] and advances rng[0], fill reads rng[1] -- both passes see one draw, the
// index goes up once per build, three launches, and stream order is the only synchronisation needed.
#include "e3k_common.h"
#include "e3k_draw.h"

namespace e3k {

constexpr int32_t NLIST_OVERFLOW = 32;      // value ORed into the persistent flag, i.e. bit 5 (values 1, 4, 8, 16: edge endpoints, one-hot types, table keys, collation)

// The pair rule of the criterion form.  segment_key [N] int64 (NULL or window <= 0: no sequence term); threshold = floor(p 2^32)
// (0: no random term); keep_all: p = 1, whose threshold does not fit 32 bits; rng [2] int64 = (next draw index, draw index in use).
struct NlistCrit {
  const int64_t* segment_key;
  int64_t* rng;
  int64_t window;
  uint32_t threshold, seed_lo, seed_hi;
  int32_t keep_all;
};

// One wave per source node i walks its own graph's nodes 64 at a time; a ballot compacts the kept pairs in ascending j.
// node_seg [N]: graph of every node; node_ptr [G + 2]: first node of every graph (the ghost graph is graph G: its nodes count 0).
template <bool FILL, bool CRIT>
__global__ __launch_bounds__(256) void nlist_kernel(const float* __restrict__ pos, const int64_t* __restrict__ node_seg,
                                                    const int64_t* __restrict__ node_ptr, int64_t N, int32_t G, float r_max,
                                                    int32_t* __restrict__ counts, const int64_t* __restrict__ offsets,
                                                    int64_t e_cap, int32_t node_blocks, int64_t* __restrict__ edge_index,
                                                    int64_t* __restrict__ edge_seg, const NlistCrit crit) {
  if constexpr (FILL) {
    if ((int)blockIdx.x >= node_blocks) {
      // the ghost tail: slot k >= E_real holds ghost edge k - E_real -- (a, a + 1) with a = kk % (n_ghost - 1), flipped on odd rounds
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
      }
      return;
    }
  }
  const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= N) return;
  const int lane = threadIdx.x & 63;
  const int64_t g = node_seg[i];
  if (g < 0 || g >= G) {      // the ghost graph (or a bad segment id): not searched
    if constexpr (!FILL) {
      if (lane == 0) counts[i] = 0;
    }
    return;
  }
  const int64_t beg = clampi(node_ptr[g], 0, N), end = clampi(node_ptr[g + 1], 0, N);
  const float px = pos[3 * i], py = pos[3 * i + 1], pz = pos[3 * i + 2];
  const int64_t off = FILL ? offsets[i] : 0;
  // criterion form: what does not depend on j -- the source's segment key and the hash of (seed, draw, i)
  int64_t key_i = 0;
  uint32_t h_i = 0;
  bool seq_on = false;
  if constexpr (CRIT) {
    seq_on = crit.segment_key != nullptr && crit.window > 0;
    if (seq_on) key_i = crit.segment_key[i];
    const uint32_t draw = (uint32_t)crit.rng[FILL ? 1 : 0];
    h_i = mix32(draw_prefix(crit.seed_lo, crit.seed_hi, draw) ^ (uint32_t)i);
  }
  int cnt = 0;
  for (int64_t j0 = beg; j0 < end; j0 += 64) {
    const int64_t j = j0 + lane;
    bool keep = false;
    if (j < end && j != i) {
      keep = within_cutoff(px, py, pz, pos, j, r_max);
      if constexpr (CRIT) {
        if (!keep) {
          const int64_t gap = i > j ? i - j : j - i;
          const bool seq = seq_on && gap < crit.window && crit.segment_key[j] == key_i;
          const bool rnd = crit.keep_all != 0 || mix32(h_i ^ (uint32_t)j) < crit.threshold;
          keep = seq || rnd;
        }
      }
    }
    const unsigned long long mask = __ballot(keep);
    if constexpr (FILL) {
      const int64_t at = off + cnt + __popcll(mask & ((1ull << lane) - 1ull));
      if (keep && at < e_cap) {      // (overflow: the list is cut at e_cap)
        edge_index[at] = i;
        edge_index[e_cap + at] = j;
        if (edge_seg) edge_seg[at] = g;
      }
    }
    cnt += __popcll(mask);
  }
  if constexpr (!FILL) {
    if (lane == 0) counts[i] = cnt;
  }
}

// One workgroup: offsets [N + 1] = exclusive scan of counts (offsets[N] = E_real), n_edges [G + 1] = the graphs' shares of the
// list as written (cut at e_cap; the ghost graph takes the rest), state[0] = E_real; overflow: the flag bit and state[1] += 1.
__global__ __launch_bounds__(1024) void nlist_scan_kernel(const int32_t* __restrict__ counts, const int64_t* __restrict__ node_ptr,
                                                          int64_t N, int32_t G, int64_t e_cap, int64_t* __restrict__ offsets,
                                                          int64_t* __restrict__ n_edges, int64_t* __restrict__ state,
                                                          int32_t* __restrict__ flag, int64_t* __restrict__ rng) {
  __shared__ int64_t part[1024];
  const int t = threadIdx.x;
  const int64_t chunk = (N + 1023) / 1024;
  const int64_t b = t * chunk, e = b + chunk < N ? b + chunk : N;
  int64_t local = 0;
  for (int64_t i = b; i < e; ++i) local += counts[i];
  part[t] = local;
  __syncthreads();
  for (int d = 1; d < 1024; d <<= 1) {
    const int64_t add = t >= d ? part[t - d] : 0;
    __syncthreads();
    part[t] += add;
    __syncthreads();
  }
  int64_t run = part[t] - local;
  for (int64_t i = b; i < e; ++i) {
    offsets[i] = run;
    run += counts[i];
  }
  const int64_t total = part[1023];
  if (t == 0) offsets[N] = total;
  __threadfence_block();
  __syncthreads();
  for (int g = t; g <= G; g += 1024) {
    if (g < G) {
      int64_t lo = offsets[clampi(node_ptr[g], 0, N)], hi = offsets[clampi(node_ptr[g + 1], 0, N)];
      lo = lo < e_cap ? lo : e_cap;
      hi = hi < e_cap ? hi : e_cap;
      n_edges[g] = hi > lo ? hi - lo : 0;
    } else {
      n_edges[g] = e_cap - (total < e_cap ? total : e_cap);
    }
  }
  if (t == 0) {
    const int64_t n_ghost = N - clampi(node_ptr[G], 0, N);
    state[0] = total;
    if (rng) {      // criterion form: the fill pass draws what the count pass drew; the next build draws anew
      const int64_t draw = rng[0];
      rng[1] = draw;
      rng[0] = draw + 1;
    }
    if (total > e_cap || (total < e_cap && n_ghost < 2)) {
      state[1] += 1;
      atomicOr(flag, NLIST_OVERFLOW);
    }
  }
}

// The scan for the periodic builder of e3k_pbc.hip (declared there): the same kernel, no criterion cells.
int nlist_scan_launch(const int32_t* counts, const int64_t* node_ptr, int64_t N, int32_t G, int64_t e_cap, int64_t* offsets,
                      int64_t* n_edges, int64_t* state, int32_t* flag, hipStream_t stream) {
  hipLaunchKernelGGL(nlist_scan_kernel, dim3(1), dim3(1024), 0, stream, counts, node_ptr, N, G, e_cap, offsets, n_edges, state, flag,
                     (int64_t*)nullptr);
  E3K_CHECK_LAUNCH();
  return E3K_OK;
}

}  // namespace e3k

static bool nlist_args_ok(const float* pos, const int64_t* node_seg, const int64_t* node_ptr, int64_t N, int32_t G) {
  return pos && node_seg && node_ptr && N >= 1 && N < (int64_t)1 << 31 && G >= 0;
}

template <bool CRIT>
static int nlist_count(const float* pos, const int64_t* node_seg, const int64_t* node_ptr, int64_t N, int32_t G, float r_max,
                       const e3k::NlistCrit& crit, int32_t* counts, void* stream) {
  if (!nlist_args_ok(pos, node_seg, node_ptr, N, G) || !counts) return E3K_ERR_INVALID;
  hipLaunchKernelGGL((e3k::nlist_kernel<false, CRIT>), dim3((unsigned)((N + 3) / 4)), dim3(256), 0, (hipStream_t)stream, pos, node_seg,
                     node_ptr, N, G, r_max, counts, (const int64_t*)nullptr, (int64_t)0, 0, (int64_t*)nullptr, (int64_t*)nullptr, crit);
  E3K_CHECK_LAUNCH();
  return E3K_OK;
}

template <bool CRIT>
static int nlist_fill(const float* pos, const int64_t* node_seg, const int64_t* node_ptr, int64_t N, int32_t G, float r_max,
                      const e3k::NlistCrit& crit, const int32_t* counts, int64_t e_cap, int64_t* offsets, int64_t* edge_index,
                      int64_t* n_edges, int64_t* edge_segment, int64_t* state, int32_t* flag, void* stream) {
  if (!nlist_args_ok(pos, node_seg, node_ptr, N, G) || !counts || !offsets || !edge_index || !n_edges || !state || !flag ||
      e_cap < 0 || e_cap >= (int64_t)1 << 31)
    return E3K_ERR_INVALID;
  hipLaunchKernelGGL(e3k::nlist_scan_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, counts, node_ptr, N, G, e_cap, offsets,
                     n_edges, state, flag, CRIT ? crit.rng : (int64_t*)nullptr);
  E3K_CHECK_LAUNCH();
  const int node_blocks = (int)((N + 3) / 4);
  int64_t tail_blocks = (e_cap + 255) / 256;      // the tail is at most the whole buffer (an empty list)
  if (tail_blocks > 256) tail_blocks = 256;
  if (tail_blocks < 1) tail_blocks = 1;
  hipLaunchKernelGGL((e3k::nlist_kernel<true, CRIT>), dim3((unsigned)(node_blocks + tail_blocks)), dim3(256), 0, (hipStream_t)stream,
                     pos, node_seg, node_ptr, N, G, r_max, (int32_t*)nullptr, (const int64_t*)offsets, e_cap, node_blocks, edge_index,
                     edge_segment, crit);
  E3K_CHECK_LAUNCH();
  return E3K_OK;
}

extern "C" int e3k_nlist_count(const float* pos, const int64_t* node_seg, const int64_t* node_ptr, int64_t N, int32_t G, float r_max,
                               int32_t* counts, void* stream) {
  return nlist_count<false>(pos, node_seg, node_ptr, N, G, r_max, e3k::NlistCrit{}, counts, stream);
}

extern "C" int e3k_nlist_fill(const float* pos, const int64_t* node_seg, const int64_t* node_ptr, int64_t N, int32_t G, float r_max,
                              const int32_t* counts, int64_t e_cap, int64_t* offsets, int64_t* edge_index, int64_t* n_edges,
                              int64_t* edge_segment, int64_t* state, int32_t* flag, void* stream) {
  return nlist_fill<false>(pos, node_seg, node_ptr, N, G, r_max, e3k::NlistCrit{}, counts, e_cap, offsets, edge_index, n_edges,
                           edge_segment, state, flag, stream);
}

static bool nlist_crit_ok(const int64_t* rng, int64_t window) { return rng != nullptr && window >= 0; }

extern "C" int e3k_nlist_count_crit(const float* pos, const int64_t* node_seg, const int64_t* node_ptr, int64_t N, int32_t G, float r_max,
                                    const int64_t* segment_key, int64_t window, uint32_t threshold, int32_t keep_all, uint32_t seed_lo,
                                    uint32_t seed_hi, int64_t* rng, int32_t* counts, void* stream) {
  if (!nlist_crit_ok(rng, window)) return E3K_ERR_INVALID;
  const e3k::NlistCrit crit{segment_key, rng, window, threshold, seed_lo, seed_hi, keep_all};
  return nlist_count<true>(pos, node_seg, node_ptr, N, G, r_max, crit, counts, stream);
}

extern "C" int e3k_nlist_fill_crit(const float* pos, const int64_t* node_seg, const int64_t* node_ptr, int64_t N, int32_t G, float r_max,
                                   const int64_t* segment_key, int64_t window, uint32_t threshold, int32_t keep_all, uint32_t seed_lo,
                                   uint32_t seed_hi, int64_t* rng, const int32_t* counts, int64_t e_cap, int64_t* offsets,
                                   int64_t* edge_index, int64_t* n_edges, int64_t* edge_segment, int64_t* state, int32_t* flag,
                                   void* stream) {
  if (!nlist_crit_ok(rng, window)) return E3K_ERR_INVALID;
  const e3k::NlistCrit crit{segment_key, rng, window, threshold, seed_lo, seed_hi, keep_all};
  return nlist_fill<true>(pos, node_seg, node_ptr, N, G, r_max, crit, counts, e_cap, offsets, edge_index, n_edges, edge_segment,
                          state, flag, stream);
}
