// The all-images rule of the periodic neighbour list, stated once, next to the minimum-image rule of e3k_pbc.h: every image of every
// ordered pair inside the cutoff, an atom's own images included.  For cells narrower than e3k_pbc.h's premise allows (crystal unit
// cells).  The builder is the one of e3k_nlist_body.h (its candidate walk, Rule::IMAGES); the rule struct and the two C entries are
// in e3k_images.hip; the torch restatement is data/compute_edge._images_rule.
//
// Per graph the HOST computes an image range R_k per axis (data/compute_edge.image_ranges, float64):
//   R_k = ceil(r_max (1 + 1e-3) / w_k + 0.5) - 1      on a periodic axis, w_k = the perpendicular width 1 / |column k of cell^-1|
//   R_k = 0                                           on a non-periodic axis
// A cell that passes check_cell (w_k > 2 r_max (1 + 1e-3)) has R = 0 on every axis.  The host refuses R_k > E3K_IMAGES_MAX_RANGE.
//
// Premise.  After the rounding step of pbc_image (base_k = -rint(s_k)) the base image's fractional components s'_k = s_k + base_k lie
// in [-1/2, 1/2], up to the fp32 rounding that the 1e-3 margin covers.  The image base + m has the vector v = sum_k (s'_k + m_k) a_k,
// and the component of v along the unit normal of the planes spanned by the other two lattice vectors is (s'_k + m_k) w_k, so
// |s'_k + m_k| w_k <= |v|.  With |v| < r_max: |m_k| < r_max / w_k + 1/2, and an integer below x is at most ceil(x) - 1: |m_k| <= R_k.
//
// The rule.  For source i, destination j of the same graph (j == i INCLUDED) and every offset m in prod_k [-R_k, R_k]:
//   d    = pos[j] - pos[i]
//   base = pbc_image(d)                               e3k_pbc.h: n_k = pbc_k ? -rintf(s_k) : 0
//   n    = base + m                                   exact: small integers held as floats
//   v    = pbc_vector(d, n)                           e3k_pbc.h's fmaf chain
//   kept iff pbc_length(v) < r_max  and not (j == i and n == 0)
// Distinct m give distinct images: nothing is emitted twice; the premise makes the list complete.
//
// Order: source ascending, then destination ascending, then m ascending with m_0 slowest and m_2 fastest, each from -R_k: candidate
//   q = (j - beg) M + ((m_0 + R_0) (2 R_1 + 1) + (m_1 + R_1)) (2 R_2 + 1) + (m_2 + R_2),      M = prod_k (2 R_k + 1)
// in ascending q.  With R = 0 this is the minimum-image list of e3k_pbc.h in its order, with the same bits.
//
// The kernel clamps every R_k it reads to [0, E3K_IMAGES_MAX_RANGE] and takes it as 0 where pbc_k == 0: a malformed table cannot
// widen the walk beyond M = 15^3 candidates per destination.
#pragma once
#include "e3k_pbc.h"      // (E3K_IMAGES_MAX_RANGE: include/e3k.h)

namespace e3k {

// What a source's wave holds of its graph: the 21 words of e3k_pbc.h and the clamped ranges -- wave-uniform, on the scalar path.
struct ImagesCell {
  PbcCell c;
  int32_t w1, w2;      // 2 R_1 + 1, 2 R_2 + 1
  int32_t r[3];        // R_k, clamped
  int32_t M;           // candidates per destination
};

__device__ __forceinline__ ImagesCell images_load_cell(const float* __restrict__ cell, const float* __restrict__ inv_cell,
                                                       const int32_t* __restrict__ pbc, const int32_t* __restrict__ image_range,
                                                       int64_t g) {
  ImagesCell s;
  s.c = pbc_load_cell(cell, inv_cell, pbc, g);
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const int32_t r = image_range[3 * g + k];
    s.r[k] = s.c.pbc[k] != 0 ? (r < 0 ? 0 : (r > E3K_IMAGES_MAX_RANGE ? E3K_IMAGES_MAX_RANGE : r)) : 0;
  }
  s.w1 = 2 * s.r[1] + 1;
  s.w2 = 2 * s.r[2] + 1;
  s.M = (2 * s.r[0] + 1) * s.w1 * s.w2;
  return s;
}

// candidate mi in [0, M) of a destination -> the image numbers n = base + m (floats) and the vector; true iff the edge is kept
__device__ __forceinline__ bool images_keep(const ImagesCell& s, float dx, float dy, float dz, bool self, uint32_t mi, float r_max,
                                            float n[3]) {
  const uint32_t w1 = (uint32_t)s.w1, w2 = (uint32_t)s.w2;
  const uint32_t hi = mi / w2;
  const int32_t m2 = (int32_t)(mi - hi * w2) - s.r[2];
  const uint32_t m0u = hi / w1;
  const int32_t m1 = (int32_t)(hi - m0u * w1) - s.r[1];
  const int32_t m0 = (int32_t)m0u - s.r[0];
  float v[3];
  pbc_image(s.c, dx, dy, dz, n);
  n[0] += (float)m0;
  n[1] += (float)m1;
  n[2] += (float)m2;
  pbc_vector(s.c, dx, dy, dz, n, v);
  if (self && n[0] == 0.0f && n[1] == 0.0f && n[2] == 0.0f) return false;
  return pbc_length(v) < r_max;
}

}  // namespace e3k
