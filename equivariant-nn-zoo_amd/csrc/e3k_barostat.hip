// The isotropic barostat of run/md.py (Barostat: stochastic cell rescaling in eps = ln V, and its deterministic limit, Berendsen's
// weak coupling) for gfx950 -- include/e3k.h, "Barostat".  One launch per MD step between the drift kernel and the force graph: it
// closes the loop pressure -> cell -> positions on the device, from the static buffers the graph and the kick kernel leave behind.
//
// One workgroup of 256 per real graph.  Every thread loads the graph's header (cell, virial, kinetic energy, pbc) through addresses
// that depend on the block alone and computes the scale factor mu redundantly in double: no LDS, no broadcast.  After a barrier
// (no wave may still read the old cell) thread 0 writes the new cell, its inverse and the records, and all threads stride over the
// graph's 3 (end - beg) position and velocity components.  Nothing is accumulated and nothing is zero-filled: the same bits every
// run, safe beside a capture.  A graph whose step cannot be taken is left as it is and COUNTED (an integer atomicAdd on the
// counter, as the constraint kernels': the one atomic, outside the arithmetic) -- valid numbers, wrong physics, reported.
#include "e3k_common.h"
#include "e3k_draw.h"

namespace e3k {

constexpr uint32_t BAROSTAT_SRC = 0xFFFFFFFEu;      // the src word of "a graph's barostat" in the stream of e3k_draw.h

// a . (b x c) of the rows, in double
__device__ __forceinline__ double det3(const double* c) {
  return c[0] * (c[4] * c[8] - c[5] * c[7]) - c[1] * (c[3] * c[8] - c[5] * c[6]) + c[2] * (c[3] * c[7] - c[4] * c[6]);
}

// the adjugate (the transposed cofactors): inverse = adj / det
__device__ __forceinline__ void adjugate3(const double* c, double* adj) {
  adj[0] = c[4] * c[8] - c[5] * c[7];
  adj[1] = c[2] * c[7] - c[1] * c[8];
  adj[2] = c[1] * c[5] - c[2] * c[4];
  adj[3] = c[5] * c[6] - c[3] * c[8];
  adj[4] = c[0] * c[8] - c[2] * c[6];
  adj[5] = c[2] * c[3] - c[0] * c[5];
  adj[6] = c[3] * c[7] - c[4] * c[6];
  adj[7] = c[1] * c[6] - c[0] * c[7];
  adj[8] = c[0] * c[4] - c[1] * c[3];
}

__device__ __forceinline__ bool finite_d(double v) { return fabs(v) <= 1.7976931348623157e308; }      // (false for NaN)

__global__ __launch_bounds__(256) void barostat_step_kernel(float* __restrict__ x, float* __restrict__ v, float* cell, float* inv_cell,
                                                            const int32_t* __restrict__ pbc, const float* __restrict__ virial,
                                                            const float* __restrict__ kinetic, const int64_t* __restrict__ node_ptr,
                                                            int64_t n, double p0, double a, double b, double min_width,
                                                            uint32_t seed_lo, uint32_t seed_hi, uint32_t draw, int32_t* counter,
                                                            double* __restrict__ volume, double* __restrict__ pressure) {
  const int64_t g = blockIdx.x;
  const int64_t beg = clampi(node_ptr[g], 0, n), end = clampi(node_ptr[g + 1], 0, n);
  float old_cell[9];
  double c[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) {
    old_cell[k] = cell[9 * g + k];
    c[k] = (double)old_cell[k];
  }
  const double vol = fabs(det3(c));
  const double trace = ((double)virial[9 * g] + (double)virial[9 * g + 4]) + (double)virial[9 * g + 8];
  const double p = (2.0 * (double)kinetic[g] + trace) / (3.0 * vol);
  double noise = 0.0;
  if (b > 0.0) {      // (uniform: Berendsen and kT = 0 draw nothing)
    const uint32_t h = mix32(draw_prefix(seed_lo, seed_hi, draw) ^ BAROSTAT_SRC);
    noise = sqrt(b / vol) * (double)normal_draw(h, (uint32_t)g);
  }
  const double d_eps = a * (p - p0) + noise;
  const double mu = exp(d_eps / 3.0);
  bool frozen = vol == 0.0 || !finite_d(p) || !finite_d(d_eps) || !finite_d(mu);
  const float mu_f = (float)mu, inv_mu_f = (float)(1.0 / mu);

  float new_cell[9], new_inv[9];
  double new_vol = vol;
  if (!frozen) {
    double nc[9], adj[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) {
      new_cell[k] = rounded_product(mu_f, old_cell[k]);
      nc[k] = (double)new_cell[k];
    }
    const double det = det3(nc);
    adjugate3(nc, adj);
    if (det == 0.0 || !finite_d(det)) {
      frozen = true;      // (a cell the rounding has made singular has no width)
    } else {
      double inv[9];
#pragma unroll
      for (int k = 0; k < 9; ++k) {
        inv[k] = adj[k] / det;
        new_inv[k] = (float)inv[k];
      }
#pragma unroll
      for (int k = 0; k < 3; ++k) {      // check_cell's rule on the NEW cell: 1 / |column k of the inverse| must exceed min_width
        const double width = 1.0 / sqrt((inv[k] * inv[k] + inv[3 + k] * inv[3 + k]) + inv[6 + k] * inv[6 + k]);
        if (pbc[3 * g + k] != 0 && !(width > min_width)) frozen = true;
      }
      new_vol = fabs(det);
    }
  }
  if (frozen) new_vol = vol;
  __syncthreads();      // every wave has read the old cell
  if (threadIdx.x == 0) {
    if (volume) volume[g] = new_vol;
    if (pressure) pressure[g] = p;
    if (frozen) {
      atomicAdd(counter, 1);
    } else {
#pragma unroll
      for (int k = 0; k < 9; ++k) {
        cell[9 * g + k] = new_cell[k];
        inv_cell[9 * g + k] = new_inv[k];
      }
    }
  }
  if (frozen) return;
  for (int64_t k = 3 * beg + threadIdx.x; k < 3 * end; k += 256) {
    x[k] = rounded_product(mu_f, x[k]);
    if (v) v[k] = rounded_product(inv_mu_f, v[k]);
  }
}

}  // namespace e3k

extern "C" int e3k_barostat_step(float* x, float* v, float* cell, float* inv_cell, const int32_t* pbc, const float* virial,
                                 const float* kinetic, const int64_t* node_ptr, int32_t G, int64_t n, double p0, double a, double b,
                                 double min_width, uint32_t seed_lo, uint32_t seed_hi, uint32_t draw, int32_t* counter,
                                 double* volume, double* pressure, void* stream) {
  if (G < 0 || n < 0 || !(a >= 0.0) || !(b >= 0.0) || !(a <= 1.7976931348623157e308) || !(b <= 1.7976931348623157e308) ||
      !(min_width >= 0.0))
    return E3K_ERR_INVALID;
  if (G == 0) return E3K_OK;
  if (!x || !cell || !inv_cell || !pbc || !virial || !kinetic || !node_ptr || !counter) return E3K_ERR_INVALID;
  hipLaunchKernelGGL(e3k::barostat_step_kernel, dim3((unsigned)G), dim3(256), 0, (hipStream_t)stream, x, v, cell, inv_cell, pbc, virial,
                     kinetic, node_ptr, n, p0, a, b, min_width, seed_lo, seed_hi, draw, counter, volume, pressure);
  E3K_CHECK_LAUNCH();
  return E3K_OK;
}
