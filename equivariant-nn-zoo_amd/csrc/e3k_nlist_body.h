// The capped neighbour-list builder, stated once: the kernel of the count and fill passes and their two host launchers.  The pair
// rules that instantiate it: CutoffRule and CriterionRule (e3k_nlist.hip), PeriodicRule (e3k_pbc.hip), ImagesRule (e3k_images.hip).
//
// Everything a capture depends on lives here and nowhere else: the ghost tail, the ghost-graph exit, the clamp of every node id
// read from the batch's own bookkeeping to [0, N] before it is used as an address, the 64-lane walk, the ballot compaction in
// ascending j, the slot index < e_cap guard on every store, the counts store.
//
// A rule is a plain struct, passed to the kernel by value, that says which ordered pairs (i, j) of one graph are kept:
//   static constexpr bool SHIFT     the list carries the three image numbers of every edge's destination (edge_shift [e_cap, 3]
//                                   int32): written per kept slot, zero on the ghost tail, and touched only where SHIFT holds
//   graph_id(g)                     the graph id the walk uses, 0 <= g < G: g itself, or g on the scalar path where the rule's
//                                   per-graph operands are to be loaded there
//   source<FILL>(i, g)              what does not depend on j (FILL: the pass, for a rule that reads per-pass cells)
//   keep(src, px, py, pz, pos, i, j, r_max, n)      the test of one pair, j != i; a SHIFT rule leaves the image numbers in n
//   static constexpr bool IMAGES    false: the walk above, one candidate per destination j != i.  true (ImagesRule, e3k_images.hip):
//                                   a destination, j == i included, has candidates(src) candidates (wave-uniform) and the rule gives
//   keep_image(src, px, py, pz, pos, i, j, mi, r_max, n)      the test of candidate mi of destination j, in place of keep()
//   scan_rng()                      host: the draw-index cells the scan advances between the two passes (nullptr: none)
#pragma once
#include "e3k_common.h"

namespace e3k {

// e3k_nlist.hip: the one launch site of nlist_scan_kernel (offsets, per-graph counts, E_real, the overflow report; rng: see there)
int nlist_scan_launch(const int32_t* counts, const int64_t* node_ptr, int64_t N, int32_t G, int64_t e_cap, int64_t* offsets,
                      int64_t* n_edges, int64_t* state, int32_t* flag, int64_t* rng, hipStream_t stream);

// One wave per source node i walks its own graph's nodes 64 at a time; a ballot compacts the kept pairs in ascending j.
// node_seg [N]: graph of every node; node_ptr [G + 2]: first node of every graph (the ghost graph is graph G: its nodes count 0).
template <bool FILL, class Rule>
__global__ __launch_bounds__(256) void nlist_kernel(const float* __restrict__ pos, const int64_t* __restrict__ node_seg,
                                                    const int64_t* __restrict__ node_ptr, int64_t N, int32_t G, float r_max,
                                                    int32_t* __restrict__ counts, const int64_t* __restrict__ offsets,
                                                    int64_t e_cap, int32_t node_blocks, int64_t* __restrict__ edge_index,
                                                    int64_t* __restrict__ edge_seg, int32_t* __restrict__ edge_shift,
                                                    const Rule rule) {
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
        if constexpr (Rule::SHIFT) {
          edge_shift[3 * k] = 0;
          edge_shift[3 * k + 1] = 0;
          edge_shift[3 * k + 2] = 0;
        }
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
  const int64_t g = rule.graph_id(g_lane);
  const auto src = rule.template source<FILL>(i, g);
  const int64_t beg = clampi(node_ptr[g], 0, N), end = clampi(node_ptr[g + 1], 0, N);
  const float px = pos[3 * i], py = pos[3 * i + 1], pz = pos[3 * i + 2];
  const int64_t off = FILL ? offsets[i] : 0;
  int cnt = 0;
  // one round of 64 lanes: the ballot compacts the kept candidates in lane order behind the source's earlier rounds
  const auto emit = [&](bool keep, int64_t j, const float (&n)[3]) {
    const unsigned long long mask = __ballot(keep);
    if constexpr (FILL) {
      const int64_t at = off + cnt + __popcll(mask & ((1ull << lane) - 1ull));
      if (keep && at < e_cap) {      // (overflow: the list is cut at e_cap)
        edge_index[at] = i;
        edge_index[e_cap + at] = j;
        if (edge_seg) edge_seg[at] = g;
        if constexpr (Rule::SHIFT) {
          edge_shift[3 * at] = (int32_t)n[0];
          edge_shift[3 * at + 1] = (int32_t)n[1];
          edge_shift[3 * at + 2] = (int32_t)n[2];
        }
      }
    }
    cnt += __popcll(mask);
  };
  if constexpr (Rule::IMAGES) {
    // the candidates q = (j - beg) M + mi of the graph in ascending q, M per destination (wave-uniform, 1 <= M <= 15^3), j == i
    // included: (j, mi) advance by (64 / M, 64 % M) with one carry per round, so nothing is divided by M inside the loop
    const uint32_t M = (uint32_t)rule.candidates(src);
    const uint32_t step_j = 64u / M, step_m = 64u - step_j * M;
    const int64_t q_end = (end - beg) * (int64_t)M;
    int64_t j = beg + (uint32_t)lane / M;
    uint32_t mi = (uint32_t)lane % M;
    for (int64_t q = lane; q - lane < q_end; q += 64) {
      bool keep = false;
      float n[3] = {0.0f, 0.0f, 0.0f};
      if (q < q_end) keep = rule.keep_image(src, px, py, pz, pos, i, j, mi, r_max, n);
      emit(keep, j, n);
      j += step_j;
      mi += step_m;
      if (mi >= M) {
        mi -= M;
        ++j;
      }
    }
  } else {
    for (int64_t j0 = beg; j0 < end; j0 += 64) {
      const int64_t j = j0 + lane;
      bool keep = false;
      float n[3] = {0.0f, 0.0f, 0.0f};
      if (j < end && j != i) keep = rule.keep(src, px, py, pz, pos, i, j, r_max, n);
      emit(keep, j, n);
    }
  }
  if constexpr (!FILL) {
    if (lane == 0) counts[i] = cnt;
  }
}

inline bool nlist_args_ok(const float* pos, const int64_t* node_seg, const int64_t* node_ptr, int64_t N, int32_t G) {
  return pos && node_seg && node_ptr && N >= 1 && N < (int64_t)1 << 31 && G >= 0;
}

// The count pass: counts [N] = kept pairs per source node (ghost nodes: 0).  The rule's own operands are the entry point's to check.
template <class Rule>
static int nlist_count(const float* pos, const int64_t* node_seg, const int64_t* node_ptr, int64_t N, int32_t G, float r_max,
                       const Rule& rule, int32_t* counts, void* stream) {
  if (!nlist_args_ok(pos, node_seg, node_ptr, N, G) || !counts) return E3K_ERR_INVALID;
  hipLaunchKernelGGL((nlist_kernel<false, Rule>), dim3((unsigned)((N + 3) / 4)), dim3(256), 0, (hipStream_t)stream, pos, node_seg,
                     node_ptr, N, G, r_max, counts, (const int64_t*)nullptr, (int64_t)0, 0, (int64_t*)nullptr, (int64_t*)nullptr,
                     (int32_t*)nullptr, rule);
  E3K_CHECK_LAUNCH();
  return E3K_OK;
}

// The scan and the fill pass: node waves as in the count pass, and behind them at most 256 workgroups that write the ghost tail.
template <class Rule>
static int nlist_fill(const float* pos, const int64_t* node_seg, const int64_t* node_ptr, int64_t N, int32_t G, float r_max,
                      const Rule& rule, const int32_t* counts, int64_t e_cap, int64_t* offsets, int64_t* edge_index,
                      int32_t* edge_shift, int64_t* n_edges, int64_t* edge_segment, int64_t* state, int32_t* flag, void* stream) {
  if (!nlist_args_ok(pos, node_seg, node_ptr, N, G) || !counts || !offsets || !edge_index || (Rule::SHIFT && !edge_shift) ||
      !n_edges || !state || !flag || e_cap < 0 || e_cap >= (int64_t)1 << 31)
    return E3K_ERR_INVALID;
  const int rc = nlist_scan_launch(counts, node_ptr, N, G, e_cap, offsets, n_edges, state, flag, rule.scan_rng(), (hipStream_t)stream);
  if (rc != E3K_OK) return rc;
  const int node_blocks = (int)((N + 3) / 4);
  int64_t tail_blocks = (e_cap + 255) / 256;      // the tail is at most the whole buffer (an empty list)
  if (tail_blocks > 256) tail_blocks = 256;
  if (tail_blocks < 1) tail_blocks = 1;
  hipLaunchKernelGGL((nlist_kernel<true, Rule>), dim3((unsigned)(node_blocks + tail_blocks)), dim3(256), 0, (hipStream_t)stream, pos,
                     node_seg, node_ptr, N, G, r_max, (int32_t*)nullptr, (const int64_t*)offsets, e_cap, node_blocks, edge_index,
                     edge_segment, edge_shift, rule);
  E3K_CHECK_LAUNCH();
  return E3K_OK;
}

}  // namespace e3k
