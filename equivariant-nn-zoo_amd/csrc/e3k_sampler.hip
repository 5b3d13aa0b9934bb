// The seeded predictor-corrector sampler's arithmetic around the model (run/sde_sampling.get_pc_sampler(seed=...)): the step's time
// and number from device cells, the Langevin corrector and the Euler-Maruyama step of the reverse VP-SDE, one launch each per
// diffusion key.  (A file of its own beside e3k_score.hip, whose object keeps the training step's three kernels.)
//
// Replaces (paths of the reference project):
//   score = -raw / std - x with std = sqrt(1 - exp(2 lm)) per node                  e3_layers/run/sde_utils.py:176-187
//   LangevinCorrector.update_fn: randn, two row norms and their means, alphas[k],   e3_layers/run/sde_sampling.py:117-143
//     x + step score + sqrt(2 step) z
//   RSDE.sde / VPSDE.sde: the Euler-Maruyama step with dt = -1 / N                  e3_layers/run/sde_utils.py:68-81, :104-119
//   the loop's "t = timesteps[i]" per step                                          e3_layers/run/sde_sampling.py:229-242
//
// Why counter-based draws: the noise of reverse step i is a function of (seed, i, node, word) in the stream of e3k_draw.h, so the
// corrector forms both of its batch-wide norms over the REAL rows of a padded batch, recomputes the same draw for the update (no
// noise buffer), and a replayed run and an eager run at one seed see the same bits.  The words: component c of a key whose earlier
// keys hold word0 components draws word0 + c for the corrector and D_total + word0 + c for the predictor (the caller passes that sum);
// the prior x_T is draw index sde.N, words word0 + c, through e3k_vpsde_perturb's z.
//
// Conditional sampling (get_pc_sampler(fixed=...), the replacement method of Song et al. 2021, section I.2): the FIXED forms of the two
// update kernels overwrite the rows whose mask byte is not zero with the known clean value perturbed to the step's own noise level,
// fmaf(m(t), x0, s(t) z) with m = expf(lm), in the launch that made the update -- no launch joins the replayed step.  z is the same
// draw index's word 2 D_total + word0 + c after the corrector and 3 D_total + word0 + c after the predictor (word_fixed: the caller
// passes the sum).  The unconditioned entry points are the FIXED = false instances of the same bodies.
//
// The probability-flow ODE sampler (run/sde_sampling.get_ode_sampler) shares the step header and vp_std: its two kernels, the Euler
// step / Heun's stage A and Heun's stage B, stand below the predictor-corrector ones.
#include "e3k_common.h"
#include "e3k_draw.h"

namespace e3k {

// std of the perturbation kernel at time t: lm = t (q t + h), one explicit FMA and one product; sqrt(-expm1(2 lm)).
__device__ __forceinline__ float vp_std(float t, float q, float h) {
  const float lm = t * fmaf(q, t, h);
  return sqrtf(-expm1f(2.0f * lm));
}

// its mean coefficient exp(lm), the same lm (e3k_vpsde_perturb's a)
__device__ __forceinline__ float vp_mean(float t, float q, float h) {
  const float lm = t * fmaf(q, t, h);
  return expf(lm);
}

// One workgroup.  cells [2] = (next step, step in use).  Every thread reads k = cells[0] BEFORE the barrier, thread 0 writes the
// cells after it.  k outside the table: nothing is written (a run that replays past its schedule stands still).
__global__ __launch_bounds__(256) void sampler_begin_step_kernel(const float* __restrict__ times, int64_t n_times,
                                                                 int64_t* __restrict__ cells, float* __restrict__ t, int32_t G1) {
  const int64_t k = cells[0];
  if (k < 0 || k >= n_times) return;      // (uniform: the whole workgroup leaves)
  const float tk = times[k];
  for (int32_t g = threadIdx.x; g < G1; g += 256) t[g] = tk;
  __syncthreads();
  if (threadIdx.x == 0) {
    cells[1] = k;
    cells[0] = k + 1;
  }
}

// One workgroup, fixed summation order (denoise_loss_kernel's): thread j takes the rows j, j + 1024, ...; six shuffle levels;
// sixteen partial sums added in order.  Phase 1: the mean row norms of score and z over the real rows.  Phase 2: the update, with
// score and z recomputed.  x_out may alias x: a row is read and written by one thread, phase 1 writes nothing.
// FIXED: a real row whose mask byte is set takes the replacement in phase 2 instead of the update; phase 1 is the same code, so both
// norms run over all real rows, the fixed ones included (the corrector ran on the whole state).  known never aliases x_out.
template <bool FIXED>
__global__ __launch_bounds__(1024) void sampler_langevin_kernel(float* x_out, const float* x, const float* __restrict__ raw,
                                                                const float* __restrict__ known, const uint8_t* __restrict__ fixed,
                                                                const int64_t* __restrict__ node_seg, const float* __restrict__ t,
                                                                const float* __restrict__ alphas, int64_t N, int32_t D, int32_t G,
                                                                int32_t n_alpha, float q, float h, float T, float snr,
                                                                uint32_t seed_lo, uint32_t seed_hi, const int64_t* __restrict__ cells,
                                                                uint32_t word0, uint32_t word_fixed, float* __restrict__ norms) {
  __shared__ float part_g[16], part_z[16];
  __shared__ int part_n[16];
  __shared__ float mean[2];
  const uint32_t h_draw = draw_prefix(seed_lo, seed_hi, (uint32_t)cells[1]);
  float acc_g = 0.f, acc_z = 0.f;
  int acc_n = 0;
  for (int64_t i = threadIdx.x; i < N; i += 1024) {
    const int64_t g = node_seg[i];
    if (g < 0 || g >= G) continue;
    const float s = vp_std(t[g], q, h);
    const uint32_t h_node = mix32(h_draw ^ (uint32_t)i);
    float gg = 0.f, zz = 0.f;
    for (int32_t c = 0; c < D; ++c) {
      const float score = -(raw[i * D + c] / s) - x[i * D + c];
      const float z = normal_draw(h_node, word0 + (uint32_t)c);
      gg = fmaf(score, score, gg);
      zz = fmaf(z, z, zz);
    }
    acc_g += sqrtf(gg);
    acc_z += sqrtf(zz);
    acc_n += 1;
  }
  for (int off = 32; off > 0; off >>= 1) {
    acc_g += __shfl_down(acc_g, off, 64);
    acc_z += __shfl_down(acc_z, off, 64);
    acc_n += __shfl_down(acc_n, off, 64);
  }
  if ((threadIdx.x & 63) == 0) {
    part_g[threadIdx.x >> 6] = acc_g;
    part_z[threadIdx.x >> 6] = acc_z;
    part_n[threadIdx.x >> 6] = acc_n;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    float sg = 0.f, sz = 0.f;
    int n_real = 0;
    for (int k = 0; k < 16; ++k) {
      sg += part_g[k];
      sz += part_z[k];
      n_real += part_n[k];
    }
    mean[0] = norms[0] = sg / (float)n_real;
    mean[1] = norms[1] = sz / (float)n_real;
  }
  __syncthreads();
  const float ratio = (snr * mean[1]) / mean[0];
  const float base = ratio * ratio * 2.0f;
  for (int64_t i = threadIdx.x; i < N; i += 1024) {
    const int64_t g = node_seg[i];
    if (g < 0 || g >= G) {      // the ghost graph: bit for bit
      for (int32_t c = 0; c < D; ++c) x_out[i * D + c] = x[i * D + c];
      continue;
    }
    const float tg = t[g];
    const float s = vp_std(tg, q, h);
    if constexpr (FIXED) {
      if (fixed[i] != 0) {
        const float m = vp_mean(tg, q, h);
        const uint32_t h_fixed = mix32(h_draw ^ (uint32_t)i);
        for (int32_t c = 0; c < D; ++c) x_out[i * D + c] = fmaf(m, known[i * D + c], s * normal_draw(h_fixed, word_fixed + (uint32_t)c));
        continue;
      }
    }
    int64_t k = (int64_t)((tg * (float)(n_alpha - 1)) / T);
    k = k < 0 ? 0 : k > n_alpha - 1 ? n_alpha - 1 : k;
    const float step = base * alphas[k];
    const float amp = sqrtf(step * 2.0f);
    const uint32_t h_node = mix32(h_draw ^ (uint32_t)i);
    for (int32_t c = 0; c < D; ++c) {
      const float xc = x[i * D + c];
      const float score = -(raw[i * D + c] / s) - xc;
      const float z = normal_draw(h_node, word0 + (uint32_t)c);
      x_out[i * D + c] = xc + step * score + amp * z;
    }
  }
}

// One thread per component: x' = x + (-0.5 beta x) dt + sqrt(beta) sqrt(|dt|) z - dt beta score, reverse_step's arithmetic in its
// order; beta = fma(t, beta_1 - beta_0, beta_0).  x_out may alias x (an element is read and written by one thread).
// FIXED: the component of a real row whose mask byte is set is the replacement at the same t[g] instead.
template <bool FIXED>
__global__ __launch_bounds__(256) void sampler_reverse_em_kernel(float* x_out, const float* x, const float* __restrict__ raw,
                                                                 const float* __restrict__ known, const uint8_t* __restrict__ fixed,
                                                                 const int64_t* __restrict__ node_seg, const float* __restrict__ t,
                                                                 int64_t N, int32_t D, int32_t G, float q, float h, float beta_0,
                                                                 float dbeta, float dt, uint32_t seed_lo, uint32_t seed_hi,
                                                                 const int64_t* __restrict__ cells, uint32_t word0, uint32_t word_fixed) {
  const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (k >= N * D) return;
  const int64_t i = k / D;
  const uint32_t c = (uint32_t)(k - i * D);
  const int64_t g = node_seg[i];
  const float xc = x[k];
  if (g < 0 || g >= G) {
    x_out[k] = xc;
    return;
  }
  const float tg = t[g];
  const float s = vp_std(tg, q, h);
  if constexpr (FIXED) {
    if (fixed[i] != 0) {
      const uint32_t h_fixed = mix32(draw_prefix(seed_lo, seed_hi, (uint32_t)cells[1]) ^ (uint32_t)i);
      x_out[k] = fmaf(vp_mean(tg, q, h), known[k], s * normal_draw(h_fixed, word_fixed + c));
      return;
    }
  }
  const float score = -(raw[k] / s) - xc;
  const float beta = fmaf(tg, dbeta, beta_0);
  const uint32_t h_draw = draw_prefix(seed_lo, seed_hi, (uint32_t)cells[1]);
  const float z = normal_draw(mix32(h_draw ^ (uint32_t)i), word0 + c);
  const float mean = xc + (-0.5f * beta * xc) * dt;
  const float noised = mean + (sqrtf(beta) * sqrtf(fabsf(dt))) * z;
  x_out[k] = noised - (dt * beta) * score;
}

// The probability-flow ODE of the VP-SDE, dx/dt = -0.5 beta (x + score): with score = -raw / s - x the x terms cancel and the drift
// is d(raw, t) = (0.5 beta(t)) (raw / s(t)) -- the collapsed form, which never forms x + (-raw / s - x).
// Both kernels read the step k = cells[1] and the times t_k = times[k], t_{k+1} = times[k + 1] from the table, never the batch's t:
// hs = t_{k+1} - t_k (negative) is one subtraction of the two table entries.  k < 0 or k + 1 >= n_times: nothing moves.
//
// Euler step / Heun stage A, one thread per component: d1 = d(raw, t_k), x_out = fmaf(hs, d1, x).  x_out may alias x.  d_out (nullable)
// takes d1, zero on ghost rows and outside the table.  t_out (nullable): block 0 writes t_{k+1} into t_out[0 .. G1) -- the time the
// model's next call sees; no thread of this kernel reads it.
__global__ __launch_bounds__(256) void sampler_ode_euler_kernel(float* x_out, float* __restrict__ d_out, const float* x,
                                                                const float* __restrict__ raw, const int64_t* __restrict__ node_seg,
                                                                const float* __restrict__ times, int64_t n_times,
                                                                const int64_t* __restrict__ cells, float* __restrict__ t_out, int32_t G1,
                                                                int64_t N, int32_t D, int32_t G, float q, float h, float beta_0,
                                                                float dbeta) {
  const int64_t step = cells[1];
  const bool inside = step >= 0 && step + 1 < n_times;      // (uniform)
  float tk = 0.f, tn = 0.f;
  if (inside) {
    tk = times[step];
    tn = times[step + 1];
    if (t_out != nullptr && blockIdx.x == 0)
      for (int32_t g = threadIdx.x; g < G1; g += 256) t_out[g] = tn;
  }
  const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (k >= N * D) return;
  const int64_t i = k / D;
  const int64_t g = node_seg[i];
  const float xc = x[k];
  if (!inside || g < 0 || g >= G) {
    x_out[k] = xc;
    if (d_out != nullptr) d_out[k] = 0.f;
    return;
  }
  const float s = vp_std(tk, q, h);
  const float beta = fmaf(tk, dbeta, beta_0);
  const float d1 = (0.5f * beta) * (raw[k] / s);
  x_out[k] = fmaf(tn - tk, d1, xc);
  if (d_out != nullptr) d_out[k] = d1;
}

// Heun stage B at t_{k+1}, one thread per component: d2 = d(raw2, t_{k+1}), x_out = fmaf(0.5 hs, d1 + d2, x0).  x_out may alias x0
// (never d1: another launch's operand, refused by the entry point).  Ghost rows and steps outside the table: x_out = x0.
__global__ __launch_bounds__(256) void sampler_ode_heun_kernel(float* x_out, const float* x0, const float* __restrict__ d1,
                                                               const float* __restrict__ raw2, const int64_t* __restrict__ node_seg,
                                                               const float* __restrict__ times, int64_t n_times,
                                                               const int64_t* __restrict__ cells, int64_t N, int32_t D, int32_t G,
                                                               float q, float h, float beta_0, float dbeta) {
  const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (k >= N * D) return;
  const int64_t step = cells[1];
  const int64_t i = k / D;
  const int64_t g = node_seg[i];
  const float xc = x0[k];
  if (step < 0 || step + 1 >= n_times || g < 0 || g >= G) {
    x_out[k] = xc;
    return;
  }
  const float tk = times[step], tn = times[step + 1];
  const float s = vp_std(tn, q, h);
  const float beta = fmaf(tn, dbeta, beta_0);
  const float d2 = (0.5f * beta) * (raw2[k] / s);
  x_out[k] = fmaf(0.5f * (tn - tk), d1[k] + d2, xc);
}

// The log-likelihood through the same flow (run/likelihood.get_likelihood_fn): on an ASCENDING table, per real graph,
//   log p(x(eps)) = log N(x(T); 0, I) + integral of div f dt,   div f = c(t) tr(d raw / d x),   c(t) = (0.5 beta(t)) / s(t),
// the trace by Hutchinson's estimate probe . vjp (vjp = the model's backward of probe . raw with respect to x).  Three kernels: the
// probe, the quadrature term of one model call, the prior's log-density.  The two sums are in double: a run adds thousands of
// terms of both signs into one number per graph, and the prior term is orders of magnitude above the integral.
//
// The probe of one key, one thread per component: draw index `draw` (sde.N + 1 + p for probe p), word word0 + c (e3k_draw.h).
// kind 0: Rademacher, +1 when bit 31 of mix32(h_node ^ (2 word)) is clear, else -1; kind 1: normal_draw.  Ghost rows: 0.
__global__ __launch_bounds__(256) void sampler_probe_kernel(float* __restrict__ out, const int64_t* __restrict__ node_seg, int64_t N,
                                                            int32_t D, int32_t G, uint32_t seed_lo, uint32_t seed_hi, uint32_t draw,
                                                            uint32_t word0, int32_t kind) {
  const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (k >= N * D) return;
  const int64_t i = k / D;
  const uint32_t word = word0 + (uint32_t)(k - i * D);
  const int64_t g = node_seg[i];
  if (g < 0 || g >= G) {
    out[k] = 0.f;
    return;
  }
  const uint32_t h_node = mix32(draw_prefix(seed_lo, seed_hi, draw) ^ (uint32_t)i);
  out[k] = kind == 0 ? ((mix32(h_node ^ (2u * word)) >> 31) == 0u ? 1.0f : -1.0f) : normal_draw(h_node, word);
}

// The sum of a 256-thread workgroup's doubles in a fixed order: six shuffle levels inside a wavefront, the four wave partials added
// in order by thread 0, which alone holds the result.
__device__ __forceinline__ double block_sum_256(double v, double* part) {
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
  __syncthreads();
  double total = 0.0;
  if (threadIdx.x == 0)
    for (int k = 0; k < 4; ++k) total += part[k];
  return total;
}

// (the rows [beg, end) of graph g from the int32 row pointers, clamped to the tensor's N rows: a bad pointer table reads nothing
// outside it)
__device__ __forceinline__ void graph_rows(const int32_t* __restrict__ row_ptr, int64_t N, int64_t* beg, int64_t* end) {
  int64_t b = row_ptr[blockIdx.x], e = row_ptr[blockIdx.x + 1];
  e = e < 0 ? 0 : e > N ? N : e;
  b = b < 0 ? 0 : b > e ? e : b;
  *beg = b, *end = e;
}

// One workgroup per real graph g: acc[g] = fma(coef, S, acc[g]) with S = sum over the graph's rows and components of probe * vjp
// (thread j takes the elements j, j + 256, ... of the graph's contiguous range; products and sums in double) and
// coef = (w c(t)) scale.  stage 0 (Euler): w = h, t = t_k; 1 (Heun A): w = h / 2, t = t_k; 2 (Heun B): w = h / 2, t = t_{k+1};
// h = t_{k+1} - t_k and c(t) in double from the fp32 table entries; qd, hd, beta_0, dbeta: the doubles of the fp32 parameters.
// k = cells[1] outside the table: nothing is written.  One writer per acc[g], no atomics; a graph of no rows adds 0.
__global__ __launch_bounds__(256) void sampler_ode_div_kernel(double* __restrict__ acc, const float* __restrict__ probe,
                                                              const float* __restrict__ vjp, const int32_t* __restrict__ row_ptr,
                                                              const float* __restrict__ times, int64_t n_times,
                                                              const int64_t* __restrict__ cells, int64_t N, int32_t D, int32_t stage,
                                                              double scale, double qd, double hd, double beta_0, double dbeta) {
  __shared__ double part[4];
  const int64_t step = cells[1];
  if (step < 0 || step + 1 >= n_times) return;      // (uniform)
  int64_t beg, end;
  graph_rows(row_ptr, N, &beg, &end);
  double sum = 0.0;
  for (int64_t k = beg * D + threadIdx.x; k < end * D; k += 256) sum += (double)probe[k] * (double)vjp[k];
  sum = block_sum_256(sum, part);
  if (threadIdx.x != 0) return;
  const double tk = (double)times[step], tn = (double)times[step + 1];
  const double w = stage == 0 ? tn - tk : 0.5 * (tn - tk);
  const double t = stage == 2 ? tn : tk;
  const double lm = t * (qd * t + hd);
  const double c = (0.5 * (t * dbeta + beta_0)) / sqrt(-expm1(2.0 * lm));
  acc[blockIdx.x] = fma((w * c) * scale, sum, acc[blockIdx.x]);
}

// One workgroup per real graph g, the same order of summation: out[g] += -0.5 sum x^2 - (0.5 n_g D) ln(2 pi), the log-density of
// the graph's rows of one key under N(0, I).
__global__ __launch_bounds__(256) void sampler_prior_logp_kernel(double* __restrict__ out, const float* __restrict__ x,
                                                                 const int32_t* __restrict__ row_ptr, int64_t N, int32_t D) {
  __shared__ double part[4];
  int64_t beg, end;
  graph_rows(row_ptr, N, &beg, &end);
  double sum = 0.0;
  for (int64_t k = beg * D + threadIdx.x; k < end * D; k += 256) {
    const double v = (double)x[k];
    sum += v * v;
  }
  sum = block_sum_256(sum, part);
  if (threadIdx.x != 0) return;
  const double norm = (0.5 * (double)((end - beg) * D)) * 1.8378770664093454835606594728112;      // ln(2 pi)
  out[blockIdx.x] = out[blockIdx.x] + (-0.5 * sum - norm);
}

}  // namespace e3k

extern "C" int e3k_sampler_begin_step(const float* times, int64_t n_times, int64_t* cells, float* t, int32_t G1, void* stream) {
  if (!times || !cells || !t || n_times < 1 || G1 < 1) return E3K_ERR_INVALID;
  hipLaunchKernelGGL(e3k::sampler_begin_step_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, times, n_times, cells, t, G1);
  E3K_CHECK_LAUNCH();
  return E3K_OK;
}

// The two forms of each update share their checks and their launch: FIXED adds the known values and the mask.
template <bool FIXED>
static int launch_langevin(float* x_out, const float* x, const float* raw, const float* known, const uint8_t* fixed,
                           const int64_t* node_seg, const float* t, const float* alphas, int64_t N, int32_t D, int32_t G, int32_t n_alpha,
                           float beta_0, float beta_1, float T, float snr, uint32_t seed_lo, uint32_t seed_hi, const int64_t* cells,
                           uint32_t word0, uint32_t word_fixed, float* norms, void* stream) {
  if (N < 1 || N >= (int64_t)1 << 31 || D < 1 || D > 1024 || G < 1 || n_alpha < 1 || !(T > 0.f) || !(snr > 0.f) || !(beta_0 >= 0.f) ||
      !(beta_1 >= beta_0))
    return E3K_ERR_INVALID;
  if (!x_out || !x || !raw || !node_seg || !t || !alphas || !cells || !norms) return E3K_ERR_INVALID;
  if (FIXED && (!known || !fixed || known == x_out)) return E3K_ERR_INVALID;
  const float q = -0.25f * (beta_1 - beta_0), h = -0.5f * beta_0;
  hipLaunchKernelGGL(e3k::sampler_langevin_kernel<FIXED>, dim3(1), dim3(1024), 0, (hipStream_t)stream, x_out, x, raw, known, fixed,
                     node_seg, t, alphas, N, D, G, n_alpha, q, h, T, snr, seed_lo, seed_hi, cells, word0, word_fixed, norms);
  E3K_CHECK_LAUNCH();
  return E3K_OK;
}

template <bool FIXED>
static int launch_reverse_em(float* x_out, const float* x, const float* raw, const float* known, const uint8_t* fixed,
                             const int64_t* node_seg, const float* t, int64_t N, int32_t D, int32_t G, float beta_0, float beta_1,
                             int32_t n_sde, uint32_t seed_lo, uint32_t seed_hi, const int64_t* cells, uint32_t word0, uint32_t word_fixed,
                             void* stream) {
  if (N < 1 || N >= (int64_t)1 << 31 || D < 1 || D > 1024 || G < 0 || n_sde < 1 || !(beta_0 >= 0.f) || !(beta_1 >= beta_0) ||
      N * D >= (int64_t)1 << 38)
    return E3K_ERR_INVALID;
  if (!x_out || !x || !raw || !node_seg || !t || !cells) return E3K_ERR_INVALID;
  if (FIXED && (!known || !fixed || known == x_out)) return E3K_ERR_INVALID;
  const float q = -0.25f * (beta_1 - beta_0), h = -0.5f * beta_0;
  hipLaunchKernelGGL(e3k::sampler_reverse_em_kernel<FIXED>, dim3((unsigned)((N * D + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     x_out, x, raw, known, fixed, node_seg, t, N, D, G, q, h, beta_0, beta_1 - beta_0, -1.0f / (float)n_sde, seed_lo,
                     seed_hi, cells, word0, word_fixed);
  E3K_CHECK_LAUNCH();
  return E3K_OK;
}

extern "C" int e3k_sampler_langevin(float* x_out, const float* x, const float* raw, const int64_t* node_seg, const float* t,
                                    const float* alphas, int64_t N, int32_t D, int32_t G, int32_t n_alpha, float beta_0, float beta_1,
                                    float T, float snr, uint32_t seed_lo, uint32_t seed_hi, const int64_t* cells, uint32_t word0,
                                    float* norms, void* stream) {
  return launch_langevin<false>(x_out, x, raw, nullptr, nullptr, node_seg, t, alphas, N, D, G, n_alpha, beta_0, beta_1, T, snr, seed_lo,
                                seed_hi, cells, word0, 0u, norms, stream);
}

extern "C" int e3k_sampler_langevin_fixed(float* x_out, const float* x, const float* raw, const float* known, const uint8_t* fixed,
                                          const int64_t* node_seg, const float* t, const float* alphas, int64_t N, int32_t D, int32_t G,
                                          int32_t n_alpha, float beta_0, float beta_1, float T, float snr, uint32_t seed_lo,
                                          uint32_t seed_hi, const int64_t* cells, uint32_t word0, uint32_t word_fixed, float* norms,
                                          void* stream) {
  return launch_langevin<true>(x_out, x, raw, known, fixed, node_seg, t, alphas, N, D, G, n_alpha, beta_0, beta_1, T, snr, seed_lo,
                               seed_hi, cells, word0, word_fixed, norms, stream);
}

extern "C" int e3k_sampler_reverse_em(float* x_out, const float* x, const float* raw, const int64_t* node_seg, const float* t,
                                      int64_t N, int32_t D, int32_t G, float beta_0, float beta_1, int32_t n_sde, uint32_t seed_lo,
                                      uint32_t seed_hi, const int64_t* cells, uint32_t word0, void* stream) {
  return launch_reverse_em<false>(x_out, x, raw, nullptr, nullptr, node_seg, t, N, D, G, beta_0, beta_1, n_sde, seed_lo, seed_hi, cells,
                                  word0, 0u, stream);
}

extern "C" int e3k_sampler_reverse_em_fixed(float* x_out, const float* x, const float* raw, const float* known, const uint8_t* fixed,
                                            const int64_t* node_seg, const float* t, int64_t N, int32_t D, int32_t G, float beta_0,
                                            float beta_1, int32_t n_sde, uint32_t seed_lo, uint32_t seed_hi, const int64_t* cells,
                                            uint32_t word0, uint32_t word_fixed, void* stream) {
  return launch_reverse_em<true>(x_out, x, raw, known, fixed, node_seg, t, N, D, G, beta_0, beta_1, n_sde, seed_lo, seed_hi, cells,
                                 word0, word_fixed, stream);
}

// The ODE sampler's two launches (run/sde_sampling.get_ode_sampler): checks as launch_reverse_em's, the table in place of t.
static bool ode_args_ok(int64_t N, int32_t D, int32_t G, int64_t n_times, float beta_0, float beta_1) {
  return !(N < 1 || N >= (int64_t)1 << 31 || D < 1 || D > 1024 || G < 0 || n_times < 2 || !(beta_0 >= 0.f) || !(beta_1 >= beta_0) ||
           N * D >= (int64_t)1 << 38);
}

extern "C" int e3k_sampler_ode_euler(float* x_out, float* d_out, const float* x, const float* raw, const int64_t* node_seg,
                                     const float* times, int64_t n_times, const int64_t* cells, float* t_out, int32_t G1, int64_t N,
                                     int32_t D, int32_t G, float beta_0, float beta_1, void* stream) {
  if (!ode_args_ok(N, D, G, n_times, beta_0, beta_1)) return E3K_ERR_INVALID;
  if (!x_out || !x || !raw || !node_seg || !times || !cells) return E3K_ERR_INVALID;
  if (d_out && (d_out == x_out || d_out == x || d_out == raw)) return E3K_ERR_INVALID;
  if (t_out && G1 < 1) return E3K_ERR_INVALID;
  const float q = -0.25f * (beta_1 - beta_0), h = -0.5f * beta_0;
  hipLaunchKernelGGL(e3k::sampler_ode_euler_kernel, dim3((unsigned)((N * D + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x_out,
                     d_out, x, raw, node_seg, times, n_times, cells, t_out, G1, N, D, G, q, h, beta_0, beta_1 - beta_0);
  E3K_CHECK_LAUNCH();
  return E3K_OK;
}

extern "C" int e3k_sampler_ode_heun(float* x_out, const float* x0, const float* d1, const float* raw2, const int64_t* node_seg,
                                    const float* times, int64_t n_times, const int64_t* cells, int64_t N, int32_t D, int32_t G,
                                    float beta_0, float beta_1, void* stream) {
  if (!ode_args_ok(N, D, G, n_times, beta_0, beta_1)) return E3K_ERR_INVALID;
  if (!x_out || !x0 || !d1 || !raw2 || !node_seg || !times || !cells || d1 == x_out) return E3K_ERR_INVALID;
  const float q = -0.25f * (beta_1 - beta_0), h = -0.5f * beta_0;
  hipLaunchKernelGGL(e3k::sampler_ode_heun_kernel, dim3((unsigned)((N * D + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x_out, x0,
                     d1, raw2, node_seg, times, n_times, cells, N, D, G, q, h, beta_0, beta_1 - beta_0);
  E3K_CHECK_LAUNCH();
  return E3K_OK;
}

// The likelihood's three launches (run/likelihood.get_likelihood_fn).
extern "C" int e3k_sampler_probe(float* out, const int64_t* node_seg, int64_t N, int32_t D, int32_t G, uint32_t seed_lo,
                                 uint32_t seed_hi, uint32_t draw, uint32_t word0, int32_t kind, void* stream) {
  if (!out || !node_seg || N < 1 || N >= (int64_t)1 << 31 || D < 1 || D > 1024 || G < 0 || N * D >= (int64_t)1 << 38 ||
      (kind != 0 && kind != 1))
    return E3K_ERR_INVALID;
  hipLaunchKernelGGL(e3k::sampler_probe_kernel, dim3((unsigned)((N * D + 255) / 256)), dim3(256), 0, (hipStream_t)stream, out, node_seg,
                     N, D, G, seed_lo, seed_hi, draw, word0, kind);
  E3K_CHECK_LAUNCH();
  return E3K_OK;
}

extern "C" int e3k_sampler_ode_div(double* acc, const float* probe, const float* vjp, const int32_t* row_ptr, const float* times,
                                   int64_t n_times, const int64_t* cells, int64_t N, int32_t D, int32_t G, int32_t stage, double scale,
                                   float beta_0, float beta_1, void* stream) {
  if (!acc || !probe || !vjp || !row_ptr || !times || !cells || stage < 0 || stage > 2 || !(scale > 0.0) ||
      !ode_args_ok(N, D, G, n_times, beta_0, beta_1))
    return E3K_ERR_INVALID;
  if (G == 0) return E3K_OK;
  const double b0 = (double)beta_0, db = (double)beta_1 - (double)beta_0;
  hipLaunchKernelGGL(e3k::sampler_ode_div_kernel, dim3((unsigned)G), dim3(256), 0, (hipStream_t)stream, acc, probe, vjp, row_ptr, times,
                     n_times, cells, N, D, stage, scale, -0.25 * db, -0.5 * b0, b0, db);
  E3K_CHECK_LAUNCH();
  return E3K_OK;
}

extern "C" int e3k_sampler_prior_logp(double* out, const float* x, const int32_t* row_ptr, int64_t N, int32_t D, int32_t G,
                                      void* stream) {
  if (!out || !x || !row_ptr || !ode_args_ok(N, D, G, 2, 0.f, 0.f)) return E3K_ERR_INVALID;
  if (G == 0) return E3K_OK;
  hipLaunchKernelGGL(e3k::sampler_prior_logp_kernel, dim3((unsigned)G), dim3(256), 0, (hipStream_t)stream, out, x, row_ptr, N, D);
  E3K_CHECK_LAUNCH();
  return E3K_OK;
}
