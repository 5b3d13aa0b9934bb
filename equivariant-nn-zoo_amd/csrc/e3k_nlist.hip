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
// batch's own bookkeeping is clamped to [0, N] before it is used as an address.  The kernel of the count and fill passes and their
// launchers are e3k_nlist_body.h's (shared with the periodic builder of e3k_pbc.hip); this file holds the scan, the plain cutoff's
// and the criterion form's pair rules, and their entry points.
//
// The criterion form (e3k_nlist_count_crit / _fill_crit) keeps a pair that is inside the cutoff OR that the declarative pair rule of
// data/compute_edge.SequenceOrRandom keeps: same segment key and |i - j| < window, or a counter-based Bernoulli draw -- the 32-bit
// pair hash of e3k_draw.h over (seed, draw index, i, j) below a threshold.  The draw index is the number of the build: count reads rng[0], the scan (one
// workgroup, between the two passes) copies it to rng[1] and advances rng[0], fill reads rng[1] -- both passes see one draw, the
// index goes up once per build, three launches, and stream order is the only synchronisation needed.
#include "e3k_common.h"
#include "e3k_draw.h"
#include "e3k_nlist_body.h"

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

// The plain cutoff: within_cutoff of e3k_common.h and nothing else.
struct CutoffRule {
  static constexpr bool SHIFT = false;
  static constexpr bool IMAGES = false;
  struct Source {};
  __device__ __forceinline__ int64_t graph_id(int64_t g) const { return g; }
  template <bool FILL>
  __device__ __forceinline__ Source source(int64_t, int64_t) const {
    return {};
  }
  __device__ __forceinline__ bool keep(const Source&, float px, float py, float pz, const float* __restrict__ pos, int64_t, int64_t j,
                                       float r_max, float*) const {
    return within_cutoff(px, py, pz, pos, j, r_max);
  }
  int64_t* scan_rng() const { return nullptr; }
};

// The criterion form: inside the cutoff OR kept by the pair rule.  The count pass draws with rng[0], the fill pass with rng[1].
struct CriterionRule {
  static constexpr bool SHIFT = false;
  static constexpr bool IMAGES = false;
  NlistCrit crit;
  struct Source {      // the source's segment key and the hash of (seed, draw, i)
    int64_t key_i;
    uint32_t h_i;
    bool seq_on;
  };
  __device__ __forceinline__ int64_t graph_id(int64_t g) const { return g; }
  template <bool FILL>
  __device__ __forceinline__ Source source(int64_t i, int64_t) const {
    Source s{0, 0, crit.segment_key != nullptr && crit.window > 0};
    if (s.seq_on) s.key_i = crit.segment_key[i];
    const uint32_t draw = (uint32_t)crit.rng[FILL ? 1 : 0];
    s.h_i = mix32(draw_prefix(crit.seed_lo, crit.seed_hi, draw) ^ (uint32_t)i);
    return s;
  }
  __device__ __forceinline__ bool keep(const Source& s, float px, float py, float pz, const float* __restrict__ pos, int64_t i,
                                       int64_t j, float r_max, float*) const {
    if (within_cutoff(px, py, pz, pos, j, r_max)) return true;
    const int64_t gap = i > j ? i - j : j - i;
    const bool seq = s.seq_on && gap < crit.window && crit.segment_key[j] == s.key_i;
    const bool rnd = crit.keep_all != 0 || mix32(s.h_i ^ (uint32_t)j) < crit.threshold;
    return seq || rnd;
  }
  int64_t* scan_rng() const { return crit.rng; }
};

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

// The one launch site of the scan (declared in e3k_nlist_body.h); rng: the criterion form's draw-index cells, else nullptr.
int nlist_scan_launch(const int32_t* counts, const int64_t* node_ptr, int64_t N, int32_t G, int64_t e_cap, int64_t* offsets,
                      int64_t* n_edges, int64_t* state, int32_t* flag, int64_t* rng, hipStream_t stream) {
  hipLaunchKernelGGL(nlist_scan_kernel, dim3(1), dim3(1024), 0, stream, counts, node_ptr, N, G, e_cap, offsets, n_edges, state, flag, rng);
  E3K_CHECK_LAUNCH();
  return E3K_OK;
}

}  // namespace e3k

extern "C" int e3k_nlist_count(const float* pos, const int64_t* node_seg, const int64_t* node_ptr, int64_t N, int32_t G, float r_max,
                               int32_t* counts, void* stream) {
  return e3k::nlist_count(pos, node_seg, node_ptr, N, G, r_max, e3k::CutoffRule{}, counts, stream);
}

extern "C" int e3k_nlist_fill(const float* pos, const int64_t* node_seg, const int64_t* node_ptr, int64_t N, int32_t G, float r_max,
                              const int32_t* counts, int64_t e_cap, int64_t* offsets, int64_t* edge_index, int64_t* n_edges,
                              int64_t* edge_segment, int64_t* state, int32_t* flag, void* stream) {
  return e3k::nlist_fill(pos, node_seg, node_ptr, N, G, r_max, e3k::CutoffRule{}, counts, e_cap, offsets, edge_index, nullptr, n_edges,
                         edge_segment, state, flag, stream);
}

static bool nlist_crit_ok(const int64_t* rng, int64_t window) { return rng != nullptr && window >= 0; }

extern "C" int e3k_nlist_count_crit(const float* pos, const int64_t* node_seg, const int64_t* node_ptr, int64_t N, int32_t G, float r_max,
                                    const int64_t* segment_key, int64_t window, uint32_t threshold, int32_t keep_all, uint32_t seed_lo,
                                    uint32_t seed_hi, int64_t* rng, int32_t* counts, void* stream) {
  if (!nlist_crit_ok(rng, window)) return E3K_ERR_INVALID;
  const e3k::CriterionRule rule{{segment_key, rng, window, threshold, seed_lo, seed_hi, keep_all}};
  return e3k::nlist_count(pos, node_seg, node_ptr, N, G, r_max, rule, counts, stream);
}

extern "C" int e3k_nlist_fill_crit(const float* pos, const int64_t* node_seg, const int64_t* node_ptr, int64_t N, int32_t G, float r_max,
                                   const int64_t* segment_key, int64_t window, uint32_t threshold, int32_t keep_all, uint32_t seed_lo,
                                   uint32_t seed_hi, int64_t* rng, const int32_t* counts, int64_t e_cap, int64_t* offsets,
                                   int64_t* edge_index, int64_t* n_edges, int64_t* edge_segment, int64_t* state, int32_t* flag,
                                   void* stream) {
  if (!nlist_crit_ok(rng, window)) return E3K_ERR_INVALID;
  const e3k::CriterionRule rule{{segment_key, rng, window, threshold, seed_lo, seed_hi, keep_all}};
  return e3k::nlist_fill(pos, node_seg, node_ptr, N, G, r_max, rule, counts, e_cap, offsets, edge_index, nullptr, n_edges, edge_segment,
                         state, flag, stream);
}
