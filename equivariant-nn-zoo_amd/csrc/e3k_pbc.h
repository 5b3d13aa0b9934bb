// The minimum-image rule of the periodic neighbour list, stated once: the capped builder and the edge-vector kernel of e3k_pbc.hip
// both include it, so a pair is kept iff the length the model later sees is < r_max, and the vectors of the two are the same bits.
//
// For source i and destination j of a graph with lattice rows a, b, c (cell [3, 3], row major), inv = cell^-1 (formed on the host in
// float64, rounded to fp32) and pbc [3]:
//   d   = pos[j] - pos[i]
//   s_k = fmaf(d_z, inv[2][k], fmaf(d_y, inv[1][k], d_x * inv[0][k]))          (builder only)
//   n_k = pbc_k ? -rintf(s_k) : 0
//   v_c = fmaf(n_2, c_c, fmaf(n_1, b_c, fmaf(n_0, a_c, d_c)))
//   keep: sqrtf((rp(v_x, v_x) + rp(v_y, v_y)) + rp(v_z, v_z)) < r_max           (rp = rounded_product: within_cutoff's test)
// Premise (checked on the host, data/compute_edge.check_cell): every periodic perpendicular width > 2 r_max (1 + 1e-3), so a pair has
// at most one image inside the cutoff and it is the rounded one.  With pbc = 0 on every axis v = d exactly.
#pragma once
#include "e3k_common.h"

namespace e3k {

// The 21 words of a graph: wave-uniform where the graph id is, so they are loaded on the scalar path.
struct PbcCell {
  float a[9];        // cell, rows a, b, c
  float inv[9];      // cell^-1
  int32_t pbc[3];
};

__device__ __forceinline__ PbcCell pbc_load_cell(const float* __restrict__ cell, const float* __restrict__ inv_cell,
                                                 const int32_t* __restrict__ pbc, int64_t g) {
  PbcCell c;
#pragma unroll
  for (int k = 0; k < 9; ++k) {
    c.a[k] = cell[9 * g + k];
    c.inv[k] = inv_cell ? inv_cell[9 * g + k] : 0.0f;
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) c.pbc[k] = pbc[3 * g + k];
  return c;
}

// the image numbers of the destination: n_k = pbc_k ? -rint(s_k) : 0, as floats (small integers)
__device__ __forceinline__ void pbc_image(const PbcCell& c, float dx, float dy, float dz, float n[3]) {
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const float s = fmaf(dz, c.inv[6 + k], fmaf(dy, c.inv[3 + k], dx * c.inv[k]));
    n[k] = c.pbc[k] != 0 ? -rintf(s) : 0.0f;
  }
}

// v = d + n_0 a + n_1 b + n_2 c, one fmaf chain per component
__device__ __forceinline__ void pbc_vector(const PbcCell& c, float dx, float dy, float dz, const float n[3], float v[3]) {
  const float d[3] = {dx, dy, dz};
#pragma unroll
  for (int k = 0; k < 3; ++k) v[k] = fmaf(n[2], c.a[6 + k], fmaf(n[1], c.a[3 + k], fmaf(n[0], c.a[k], d[k])));
}

// |v| as the model sees it: within_cutoff's sum, no fused multiply-add
__device__ __forceinline__ float pbc_length(const float v[3]) {
  const float d2 = (rounded_product(v[0], v[0]) + rounded_product(v[1], v[1])) + rounded_product(v[2], v[2]);
  return sqrtf(d2);
}

}  // namespace e3k
