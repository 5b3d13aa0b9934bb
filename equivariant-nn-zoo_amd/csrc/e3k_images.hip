// Periodic cells, every image inside the cutoff (crystal unit cells) for the capped neighbour list.
//
// The capped builder of e3k_nlist_body.h -- the kernel and the launchers the cutoff, criterion and minimum-image forms use, with the
// scan of e3k_nlist.hip between the passes -- instantiated with ImagesRule, the rule of e3k_images.h.  Rule::IMAGES switches the walk
// from the destinations of the source's graph to the candidates (destination, image offset) of it: M = prod (2 R_k + 1) per
// destination, 64 per round, so that a unit cell of a handful of atoms still fills the lanes.  Outputs are e3k_pbc_nlist_*'s:
// edge_index, edge_cell_shift (the image numbers of every edge's destination), counts, offsets, the ghost tail, the overflow report.
// A pair may hold several slots, and an atom is joined to its own images (src == dst, shift != 0).
//
// Nothing downstream changes: the edge-vector kernel of e3k_pbc.hip recomputes v from the stored integers with the same fmaf chain,
// the virial sums over edges, the CSR build takes duplicate pairs and self loops.  The search stays O(n^2 M) per graph: no cell list.
#include "e3k_images.h"
#include "e3k_nlist_body.h"

namespace e3k {

// cell, inv_cell [G + 1, 3, 3]; pbc, image_range [G + 1, 3] (zero for the ghost graph).
struct ImagesRule {
  static constexpr bool SHIFT = true;
  static constexpr bool IMAGES = true;
  const float* cell;
  const float* inv_cell;
  const int32_t* pbc;
  const int32_t* image_range;
  // one wave, one source node, one graph: the graph id is wave-uniform (0 <= g < G < 2^31), and so are the 24 words of its cell
  __device__ __forceinline__ int64_t graph_id(int64_t g) const { return uniform((int)g); }
  template <bool FILL>
  __device__ __forceinline__ ImagesCell source(int64_t, int64_t g) const {
    return images_load_cell(cell, inv_cell, pbc, image_range, g);
  }
  __device__ __forceinline__ int32_t candidates(const ImagesCell& s) const { return s.M; }
  // candidate mi of destination j (j == i included)
  __device__ __forceinline__ bool keep_image(const ImagesCell& s, float px, float py, float pz, const float* __restrict__ pos, int64_t i,
                                             int64_t j, uint32_t mi, float r_max, float n[3]) const {
    const float dx = pos[3 * j] - px, dy = pos[3 * j + 1] - py, dz = pos[3 * j + 2] - pz;
    return images_keep(s, dx, dy, dz, j == i, mi, r_max, n);
  }
  int64_t* scan_rng() const { return nullptr; }
};

}  // namespace e3k

extern "C" int e3k_images_count(const float* pos, const int64_t* node_seg, const int64_t* node_ptr, int64_t N, int32_t G, float r_max,
                                const float* cell, const float* inv_cell, const int32_t* pbc, const int32_t* image_range,
                                int32_t* counts, void* stream) {
  if (!cell || !inv_cell || !pbc || !image_range) return E3K_ERR_INVALID;
  return e3k::nlist_count(pos, node_seg, node_ptr, N, G, r_max, e3k::ImagesRule{cell, inv_cell, pbc, image_range}, counts, stream);
}

extern "C" int e3k_images_fill(const float* pos, const int64_t* node_seg, const int64_t* node_ptr, int64_t N, int32_t G, float r_max,
                               const float* cell, const float* inv_cell, const int32_t* pbc, const int32_t* image_range,
                               const int32_t* counts, int64_t e_cap, int64_t* offsets, int64_t* edge_index, int32_t* edge_cell_shift,
                               int64_t* n_edges, int64_t* edge_segment, int64_t* state, int32_t* flag, void* stream) {
  if (!cell || !inv_cell || !pbc || !image_range) return E3K_ERR_INVALID;
  return e3k::nlist_fill(pos, node_seg, node_ptr, N, G, r_max, e3k::ImagesRule{cell, inv_cell, pbc, image_range}, counts, e_cap, offsets,
                         edge_index, edge_cell_shift, n_edges, edge_segment, state, flag, stream);
}
