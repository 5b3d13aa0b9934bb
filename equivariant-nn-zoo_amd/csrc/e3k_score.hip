// The protein score nets' training step around the model, for a step that is captured once and replayed (run/score_step.py):
// the VP-SDE perturbation with counter-based draws, the denoising loss with its gradient, and the step's record.
//
// Replaces (paths of the reference project):
//   t ~ U(eps, T) per graph, VPSDE.marginal's x_t = exp(lm) x_0 + std z               e3_layers/run/sde_utils.py:54-66, :143-160
//   the loss mean((score std + z)^2) of get_sde_loss_fn with score = -raw / std - x_t  e3_layers/run/sde_utils.py:161-171, :176-187
//
// Why counter-based draws: a replayed step whose capped neighbour list overflowed is vetoed on the device and redone eagerly by
// the host on exactly the same noised batch -- t and z are functions of (seed, draw index, graph / node, word) in the stream of
// e3k_draw.h (the thermostat's), and the draw index is a device cell the captured step reads (the step counter).
//
// The sampling side of the same nets -- the seeded predictor-corrector loop's step header, Langevin corrector and reverse
// Euler-Maruyama step, on the same stream of draws -- is e3k_sampler.hip: this object keeps the training step's three kernels.
#include "e3k_common.h"
#include "e3k_draw.h"

namespace e3k {

// One thread per node component (and the first G + 1 threads file t).  The time of graph g is the pair hash with src = 0xFFFFFFFF
// (no node has that index: N < 2^31) and dst = g; a node's threads recompute their graph's t (five integer rounds and two
// library calls: cheaper than a second launch).  lm = t (q t + h) with q = -(beta_1 - beta_0) / 4 and h = -beta_0 / 2 formed by the
// caller in fp32: one explicit FMA and one product, so that the value the two exponentials see is the same whatever the compiler
// contracts.  std = sqrt(-expm1(2 lm)): 1 - exp(2 lm) would lose most of its bits at small t.
__global__ __launch_bounds__(256) void vpsde_perturb_kernel(const float* __restrict__ x0, const int64_t* __restrict__ node_seg,
                                                            int64_t N, int32_t D, int32_t G, float q, float h, float eps, float span,
                                                            uint32_t seed_lo, uint32_t seed_hi, const int64_t* __restrict__ draw_cell,
                                                            uint32_t word0, float* __restrict__ t_out, float* __restrict__ x_t,
                                                            float* __restrict__ z_out, float* __restrict__ std_out) {
  const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const uint32_t draw = (uint32_t)draw_cell[0];
  const uint32_t h_draw = draw_prefix(seed_lo, seed_hi, draw);
  const uint32_t h_time = mix32(h_draw ^ 0xFFFFFFFFu);
  auto time_of = [&](uint32_t g) { return fmaf(span, uniform24(mix32(h_time ^ g)), eps); };
  if (k <= G) t_out[k] = k < G ? time_of((uint32_t)k) : 0.5f;
  if (k >= N * D) return;
  const int64_t i = k / D;
  const uint32_t c = (uint32_t)(k - i * D);
  const int64_t g = node_seg[i];
  if (g < 0 || g >= G) {      // the ghost graph: the padded geometry stays what pad_batch made it
    x_t[k] = x0[k];
    z_out[k] = 0.f;
    if (c == 0) std_out[i] = 1.f;
    return;
  }
  const float t = time_of((uint32_t)g);
  const float lm = t * fmaf(q, t, h);
  const float a = expf(lm), s = sqrtf(-expm1f(2.0f * lm));
  const float z = normal_draw(mix32(h_draw ^ (uint32_t)i), word0 + c);
  x_t[k] = fmaf(a, x0[k], s * z);
  z_out[k] = z;
  if (c == 0) std_out[i] = s;
}

// err = -raw - std_i x_t + z (= score std + z with score = -raw / std - x_t); loss = sum_i w_i (1 / D) sum_c err^2 and
// grad_raw = -2 w_i / D err in ONE launch.  One workgroup, a fixed summation order, in the manner of sq_error_kernel: thread t takes
// the components t, t + 1024, ...; six shuffle levels; sixteen partial sums added in order.
__global__ __launch_bounds__(1024) void denoise_loss_kernel(const float* __restrict__ raw, const float* __restrict__ x_t,
                                                            const float* __restrict__ z, const float* __restrict__ std,
                                                            const float* __restrict__ w, int64_t N, int32_t D,
                                                            float* __restrict__ loss, float* __restrict__ grad) {
  __shared__ float part[16];
  const float wu = 1.0f / (float)N, inv_d = 1.0f / (float)D;
  const int64_t n = N * D;
  float acc = 0.f;
  for (int64_t k = threadIdx.x; k < n; k += 1024) {
    const int64_t i = k / D;
    const float wi = (w ? w[i] : wu) * inv_d;
    const float err = (z[k] - raw[k]) - std[i] * x_t[k];
    acc = fmaf(wi * err, err, acc);
    grad[k] = -2.0f * wi * err;
  }
  for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    float s = 0.f;
    for (int k = 0; k < 16; ++k) s += part[k];
    loss[0] = s;
  }
}

// One thread: the step's loss into ring[step % W]; the first step whose capped list overflowed (the builder's counter is not
// zero) is remembered; the step counter goes up.  cells [2] int64 = (step, first_bad).
__global__ void score_step_record_kernel(const float* __restrict__ loss, const int64_t* __restrict__ overflow,
                                         int64_t* __restrict__ cells, float* __restrict__ ring, int32_t W) {
  const int64_t step = cells[0];
  ring[step >= 0 ? step % W : 0] = loss[0];
  if (overflow[0] != 0 && cells[1] < 0) cells[1] = step;
  cells[0] = step + 1;
}

}  // namespace e3k

extern "C" int e3k_vpsde_perturb(const float* x0, const int64_t* node_seg, int64_t N, int32_t D, int32_t G, float beta_0,
                                 float beta_1, float eps, float T, uint32_t seed_lo, uint32_t seed_hi, const int64_t* draw,
                                 uint32_t word0, float* t, float* x_t, float* z, float* std, void* stream) {
  if (N < 0 || N >= (int64_t)1 << 31 || D < 1 || D > 1024 || G < 0 || !(eps >= 0.f) || !(T >= eps) || !(beta_0 >= 0.f) ||
      !(beta_1 >= beta_0) || N * D >= (int64_t)1 << 38)
    return E3K_ERR_INVALID;
  if (!draw || !t || (N > 0 && (!x0 || !node_seg || !x_t || !z || !std))) return E3K_ERR_INVALID;
  const int64_t threads = N * D > (int64_t)G + 1 ? N * D : (int64_t)G + 1;
  const float q = -0.25f * (beta_1 - beta_0), h = -0.5f * beta_0;
  hipLaunchKernelGGL(e3k::vpsde_perturb_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x0,
                     node_seg, N, D, G, q, h, eps, T - eps, seed_lo, seed_hi, draw, word0, t, x_t, z, std);
  E3K_CHECK_LAUNCH();
  return E3K_OK;
}

extern "C" int e3k_denoise_loss(const float* raw, const float* x_t, const float* z, const float* std, const float* weight,
                                int64_t N, int32_t D, float* loss, float* grad, void* stream) {
  if (N <= 0 || D < 1 || !raw || !x_t || !z || !std || !loss || !grad) return E3K_ERR_INVALID;
  hipLaunchKernelGGL(e3k::denoise_loss_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, raw, x_t, z, std, weight, N, D, loss,
                     grad);
  E3K_CHECK_LAUNCH();
  return E3K_OK;
}

extern "C" int e3k_score_step_record(const float* loss, const int64_t* overflow, int64_t* cells, float* ring, int32_t W,
                                     void* stream) {
  if (!loss || !overflow || !cells || !ring || W < 1) return E3K_ERR_INVALID;
  hipLaunchKernelGGL(e3k::score_step_record_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, loss, overflow, cells, ring, W);
  E3K_CHECK_LAUNCH();
  return E3K_OK;
}
