// The integrators of run/md.py: the two half steps of velocity Verlet -- plain, thermostatted (Langevin) and with bond-length
// constraints (BondConstraints: SHAKE in the first half step, RATTLE in the second) -- and the FIRE iteration.  A step is the force
// graph + two launches (FIRE: + one): the constrained kernels REPLACE e3k_md_drift and e3k_md_kick / e3k_md_kick_langevin, they do
// not follow them.
//
// Each per-atom update is written once: half_kick_drift (first half) and ou_kick (second half).  The plain kernels and the free
// atoms and stars of the constrained ones call the same two functions, so with no star at all the constrained kernels give the
// plain kernels' values, and the plain kick is the thermostat's at c = 1, s = 0.  The noise is the stream of e3k_draw.h.
//
// The constraints are disjoint STARS: a centre with 1..4 satellites, every constraint centre--satellite, no atom in two stars (the
// bonds-to-hydrogen set).  One thread owns a star, so nothing is shared: no atomics in the arithmetic, the same bits every run.
// Tables (built once by the host): star_ptr [S + 1] into star_atom / star_len [n_slots] -- per star the centre, then its satellites,
// each satellite's length beside it (the centre's slot holds 0); free_atom [F]: the atoms in no star; both sorted by graph, with
// graph_star_ptr / graph_free_ptr [G + 1].  Every index read from a table is clamped before it is used as an address.
//
// A star that does not converge within max_iter sweeps (or, in SHAKE, whose moved bond has turned against the old one) adds one to a
// device counter and is written as it stands: valid numbers, wrong physics -- reported, like the neighbour list's overflow.
#include "e3k_common.h"
#include "e3k_draw.h"

namespace e3k {

constexpr int STAR_MAX = 5;      // centre + at most four satellites (CH4, NH4+)

// velocity Verlet, first half, one component: v += dt/2 f / m, x += dt v
__device__ __forceinline__ void half_kick_drift(float& x, float& v, float f, float m, float dt) {
  const float vn = v + (0.5f * dt) * f / m;
  v = vn;
  x = x + dt * vn;
}

// the first half on the n real nodes (3n components, one per thread)
__global__ __launch_bounds__(256) void md_drift_kernel(float* __restrict__ x, float* __restrict__ v, const float* __restrict__ f,
                                                       const float* __restrict__ mass, int64_t n3, float dt) {
  const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (c >= n3) return;
  half_kick_drift(x[c], v[c], f[c], mass[c / 3], dt);
}

// The second half step of one atom: v <- c v + (s / sqrt(m)) xi, then v += dt/2 f / m (kick false: skipped).  c v and the noise
// term are rounded products that meet in a plain add, whatever the compiler contracts: with c = 1 the first is v itself.  s == 0 (a
// uniform branch: NVE, friction alone, project()) draws nothing -- adding the exact zero 0 xi would change the sign of a -0 at
// most; a lane of the constrained kernel owns up to five atoms, and fifteen logarithms and cosines for nothing would be a fifth of
// its time.
struct AtomIn {
  float v[3], f[3];
};

__device__ __forceinline__ AtomIn load_atom(const float* __restrict__ v, const float* __restrict__ f, int64_t i) {
  AtomIn a;
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    a.v[d] = v[3 * i + d];
    a.f[d] = f ? f[3 * i + d] : 0.f;
  }
  return a;
}

__device__ __forceinline__ void ou_kick(const AtomIn& in, bool kick, int64_t i, float m, float dt, float c, float s, uint32_t h_wave,
                                        uint32_t word0, float& vx, float& vy, float& vz) {
  if (s != 0.f) {
    const float a = s / sqrtf(m);
    const uint32_t h_i = mix32(h_wave ^ (uint32_t)i);
    vx = rounded_product(c, in.v[0]) + rounded_product(a, normal_draw(h_i, word0));
    vy = rounded_product(c, in.v[1]) + rounded_product(a, normal_draw(h_i, word0 + 1u));
    vz = rounded_product(c, in.v[2]) + rounded_product(a, normal_draw(h_i, word0 + 2u));
  } else {
    vx = rounded_product(c, in.v[0]);
    vy = rounded_product(c, in.v[1]);
    vz = rounded_product(c, in.v[2]);
  }
  if (kick) {
    const float h = 0.5f * dt / m;
    vx = vx + h * in.f[0];
    vy = vy + h * in.f[1];
    vz = vz + h * in.f[2];
  }
}

// The second half on every atom (ou_kick; e3k_md_kick launches it with c = 1, s = 0) and the graphs' kinetic energies.  One wave per
// graph; lane l sums the nodes l, l + 64, ... of the graph in ascending order, the 64 partial sums meet in a fixed butterfly: the
// same bits every run (no atomics).  The step's record is complete in the same launch: potential[g] = energy[g] (the force graph's
// static output, overwritten by the next replay).
__global__ __launch_bounds__(256) void md_kick_kernel(float* __restrict__ v, const float* __restrict__ f, const float* __restrict__ mass,
                                                      const int64_t* __restrict__ node_ptr, int32_t G, int64_t n, float dt, float c,
                                                      float s, uint32_t seed_lo, uint32_t seed_hi, uint32_t draw, uint32_t word0,
                                                      float* __restrict__ kinetic, const float* __restrict__ energy,
                                                      float* __restrict__ potential) {
  const int g = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (g >= G) return;
  const int lane = threadIdx.x & 63;
  const int64_t beg = clampi(node_ptr[g], 0, n), end = clampi(node_ptr[g + 1], 0, n);
  const uint32_t h_wave = draw_prefix(seed_lo, seed_hi, draw);      // what does not depend on the node
  float ke = 0.f;
  for (int64_t i = beg + lane; i < end; i += 64) {
    const float m = mass[i];
    float vx, vy, vz;
    ou_kick(load_atom(v, f, i), f != nullptr, i, m, dt, c, s, h_wave, word0, vx, vy, vz);
    v[3 * i] = vx;
    v[3 * i + 1] = vy;
    v[3 * i + 2] = vz;
    // 0.5 m ((vx^2 + vy^2) + vz^2) with its contractions written out: under -ffp-contract=fast the compiler may fuse either
    // product of vx vx + vy vy into the add, and the two choices differ in the last bit
    ke = fmaf(0.5f * m, fmaf(vz, vz, fmaf(vx, vx, vy * vy)), ke);
  }
  ke = wave_sum(ke);
  if (lane == 0) {
    if (kinetic) kinetic[g] = ke;
    if (potential) potential[g] = energy[g];
  }
}

// FIRE (Bitzek et al. 2006, the step rule of ASE's optimiser) with the adaptive state PER GRAPH: one wave per graph, three
// walks over its atoms -- the reductions, the velocity update with |dr|^2, the move.  state [G, 4] = (dt, alpha, n_pos, fmax).
struct FireParams {
  float ftol, dt_max, maxstep, n_min, f_inc, f_dec, alpha_start, f_alpha;
};

__global__ __launch_bounds__(256) void fire_step_kernel(float* __restrict__ x, float* __restrict__ v, const float* __restrict__ f,
                                                        const int64_t* __restrict__ node_ptr, int32_t G, int64_t n,
                                                        float* __restrict__ state, const FireParams p,
                                                        const float* __restrict__ energy, float* __restrict__ energy_record,
                                                        float* __restrict__ fmax_record) {
  const int g = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (g >= G) return;
  const int lane = threadIdx.x & 63;
  const int64_t beg = clampi(node_ptr[g], 0, n), end = clampi(node_ptr[g + 1], 0, n);
  float dt = state[4 * g], alpha = state[4 * g + 1], n_pos = state[4 * g + 2];
  float fv = 0.f, ff = 0.f, vv = 0.f, f2max = 0.f;
  for (int64_t i = beg + lane; i < end; i += 64) {
    const float fx = f[3 * i], fy = f[3 * i + 1], fz = f[3 * i + 2];
    const float vx = v[3 * i], vy = v[3 * i + 1], vz = v[3 * i + 2];
    const float f2 = (fx * fx + fy * fy) + fz * fz;
    fv += (fx * vx + fy * vy) + fz * vz;
    ff += f2;
    vv += (vx * vx + vy * vy) + vz * vz;
    f2max = fmaxf(f2max, f2);
  }
  fv = wave_sum(fv);
  ff = wave_sum(ff);
  vv = wave_sum(vv);
  const float fmax = sqrtf(wave_max_f(f2max));
  // (wave-uniform, like every branch below: the reductions leave all lanes the same values.)  An empty graph is frozen whatever
  // ftol is: with ftol = 0 its fmax = 0 is not below the tolerance, and its dt, alpha and n_pos would go on adapting to nothing.
  const bool frozen = end <= beg || fmax < p.ftol;
  if (frozen) {
    for (int64_t i = beg + lane; i < end; i += 64) v[3 * i] = v[3 * i + 1] = v[3 * i + 2] = 0.f;
  } else {
    float keep = 0.f, mix = 0.f;      // v <- keep v + mix f
    if (fv < 0.f) {
      dt = dt * p.f_dec;
      alpha = p.alpha_start;
      n_pos = 0.f;
    } else {
      keep = 1.0f - alpha;
      mix = ff > 0.f ? alpha * (sqrtf(vv) / sqrtf(ff)) : 0.f;
      if (n_pos > p.n_min) {
        dt = fminf(dt * p.f_inc, p.dt_max);
        alpha = alpha * p.f_alpha;
      }
      n_pos = n_pos + 1.0f;
    }
    float v2 = 0.f;
    for (int64_t i = beg + lane; i < end; i += 64) {
      const float fx = f[3 * i], fy = f[3 * i + 1], fz = f[3 * i + 2];
      const float vx = (keep * v[3 * i] + mix * fx) + dt * fx;
      const float vy = (keep * v[3 * i + 1] + mix * fy) + dt * fy;
      const float vz = (keep * v[3 * i + 2] + mix * fz) + dt * fz;
      v[3 * i] = vx;
      v[3 * i + 1] = vy;
      v[3 * i + 2] = vz;
      v2 += (vx * vx + vy * vy) + vz * vz;
    }
    const float norm_dr = dt * sqrtf(wave_sum(v2));
    const float move = norm_dr > p.maxstep ? dt * (p.maxstep / norm_dr) : dt;      // dr = move v
    for (int64_t i = beg + lane; i < end; i += 64) {
      x[3 * i] = x[3 * i] + move * v[3 * i];
      x[3 * i + 1] = x[3 * i + 1] + move * v[3 * i + 1];
      x[3 * i + 2] = x[3 * i + 2] + move * v[3 * i + 2];
    }
  }
  if (lane == 0) {
    state[4 * g] = dt;
    state[4 * g + 1] = alpha;
    state[4 * g + 2] = n_pos;
    state[4 * g + 3] = fmax;
    if (energy_record) energy_record[g] = energy[g];
    if (fmax_record) fmax_record[g] = fmax;
  }
}

// The rows of star t: its atoms (clamped to [0, n - 1]), inverse masses and the satellites' lengths.  Slots behind the star's own are
// filled with the centre, unit mass and zeros: the unrolled loops below guard on k < ns, the fill only keeps every register defined.
struct StarRows {
  int64_t id[STAR_MAX];
  float inv_m[STAR_MAX], m[STAR_MAX], d0[STAR_MAX - 1];
  int ns;      // satellites; -1: an empty row (never built by the host)
};

__device__ __forceinline__ StarRows load_star(const int64_t* __restrict__ star_ptr, const int64_t* __restrict__ star_atom,
                                              const float* __restrict__ star_len, const float* __restrict__ mass, int64_t t,
                                              int64_t n_slots, int64_t n) {
  StarRows r;
  const int64_t beg = clampi(star_ptr[t], 0, n_slots), end = clampi(star_ptr[t + 1], beg, n_slots);
  const int cnt = (int)(end - beg < STAR_MAX ? end - beg : STAR_MAX);
  r.ns = cnt - 1;
#pragma unroll
  for (int a = 0; a < STAR_MAX; ++a) {
    const bool on = a < cnt;
    r.id[a] = on ? clampi(star_atom[beg + a], 0, n - 1) : (a > 0 ? r.id[0] : 0);
    r.m[a] = on ? mass[r.id[a]] : 1.0f;
    r.inv_m[a] = on ? 1.0f / r.m[a] : 0.f;
    if (a > 0) r.d0[a - 1] = on ? star_len[beg + a] : 0.f;
  }
  return r;
}

// First half step with SHAKE.  Threads [0, S): one star each; threads [S, S + F): one free atom each (half_kick_drift, as md_drift_kernel).
// A star works in coordinates RELATIVE TO ITS CENTRE'S OLD POSITION, so the rounding of a 10 A coordinate does not enter a 1 A
// bond: p = (old - centre_old) + dt v_half, sweeps over the constraints in stored order along the OLD bond vectors, the correction
// split by inverse mass, until every |d^2 - d0^2| <= 2 tol d0^2; then x = centre_old + p and v = v_half + (p - p_unconstrained) / dt.
// f NULL: positions only -- no kick, no move, v untouched (the driver's project(): the direction is the present bond).
__global__ __launch_bounds__(256) void md_drift_shake_kernel(float* __restrict__ x, float* __restrict__ v, const float* __restrict__ f,
                                                             const float* __restrict__ mass, int64_t n, float dt,
                                                             const int64_t* __restrict__ star_ptr,
                                                             const int64_t* __restrict__ star_atom,
                                                             const float* __restrict__ star_len, int64_t S, int64_t n_slots,
                                                             const int64_t* __restrict__ free_atom, int64_t F, float tol, int max_iter,
                                                             int32_t* __restrict__ counter) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= S + F) return;
  if (t >= S) {
    if (!f) return;
    const int64_t i = clampi(free_atom[t - S], 0, n - 1);
    const float m = mass[i];
#pragma unroll
    for (int c = 0; c < 3; ++c) half_kick_drift(x[3 * i + c], v[3 * i + c], f[3 * i + c], m, dt);
    return;
  }
  const StarRows st = load_star(star_ptr, star_atom, star_len, mass, t, n_slots, n);
  if (st.ns < 0) return;
  float xc[3], ro[STAR_MAX - 1][3], vh[STAR_MAX][3], p[STAR_MAX][3], q[STAR_MAX][3];
#pragma unroll
  for (int c = 0; c < 3; ++c) xc[c] = x[3 * st.id[0] + c];
#pragma unroll
  for (int a = 0; a < STAR_MAX; ++a) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const int64_t j = 3 * st.id[a] + c;
      const float rel = a == 0 ? 0.f : x[j] - xc[c];
      if (a > 0) ro[a - 1][c] = rel;
      vh[a][c] = f ? v[j] + (0.5f * dt) * f[j] / st.m[a] : v[j];
      p[a][c] = f ? rel + rounded_product(dt, vh[a][c]) : rel;
      q[a][c] = p[a][c];
    }
  }
  // A pass visits the constraints in stored order and corrects those outside the tolerance; the star is done after a pass that
  // found none.  Pass number max_iter only looks: what it still finds is a failure.
  const float two_tol = 2.0f * tol;
  bool fail = false;
  for (int it = 0; it <= max_iter; ++it) {
    bool moved = false;
#pragma unroll
    for (int k = 0; k < STAR_MAX - 1; ++k) {
      if (k < st.ns) {
        const float rx = p[k + 1][0] - p[0][0], ry = p[k + 1][1] - p[0][1], rz = p[k + 1][2] - p[0][2];
        const float d02 = st.d0[k] * st.d0[k];
        const float diff = d02 - ((rx * rx + ry * ry) + rz * rz);
        if (!(fabsf(diff) <= two_tol * d02)) {
          moved = true;
          const float rr = (rx * ro[k][0] + ry * ro[k][1]) + rz * ro[k][2];
          if (it < max_iter && rr > 0.f) {
            const float g = diff / (2.0f * rr * (st.inv_m[0] + st.inv_m[k + 1]));
            const float gs = g * st.inv_m[k + 1], gc = g * st.inv_m[0];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
              p[k + 1][c] = p[k + 1][c] + gs * ro[k][c];
              p[0][c] = p[0][c] - gc * ro[k][c];
            }
          } else {
            fail = true;
          }
        }
      }
    }
    if (!moved) break;
  }
  const float inv_dt = 1.0f / dt;
#pragma unroll
  for (int a = 0; a < STAR_MAX; ++a) {
    if (a <= st.ns) {
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const int64_t j = 3 * st.id[a] + c;
        x[j] = xc[c] + p[a][c];
        if (f) v[j] = vh[a][c] + (p[a][c] - q[a][c]) * inv_dt;
      }
    }
  }
  if (fail) atomicAdd(counter, 1);
}

// Second half step with RATTLE.  One wave per graph: lane l takes the graph's stars l, l + 64, ... and then its free atoms
// l, l + 64, ...  Every atom gets ou_kick, md_kick_kernel's update (c = 1, s = 0: the plain kick; f NULL: no kick); a star's
// velocities are then projected by sweeps along its PRESENT bond vectors r_k = x_sat - x_centre,
//   g = r_k . (v_sat - v_centre) / (|r_k|^2 (1/m_c + 1/m_s));   v_sat -= g / m_s r_k;   v_centre += g / m_c r_k,
// until every |r_k . v_rel| <= tol d0_k (|v_centre| + |v_sat|).  The kinetic energy is that of the PROJECTED velocities: a lane adds
// its stars' atoms (centre, then satellites) and then its free atoms, in that fixed order; the 64 sums meet in wave_sum's butterfly.
__global__ __launch_bounds__(256) void md_kick_rattle_kernel(float* __restrict__ v, const float* __restrict__ f,
                                                             const float* __restrict__ mass, const float* __restrict__ x, int32_t G,
                                                             int64_t n, float dt, float c, float s, uint32_t seed_lo, uint32_t seed_hi,
                                                             uint32_t draw, uint32_t word0, float* __restrict__ kinetic,
                                                             const float* __restrict__ energy, float* __restrict__ potential,
                                                             const int64_t* __restrict__ star_ptr,
                                                             const int64_t* __restrict__ star_atom,
                                                             const float* __restrict__ star_len, int64_t S, int64_t n_slots,
                                                             const int64_t* __restrict__ free_atom, int64_t F,
                                                             const int64_t* __restrict__ graph_star_ptr,
                                                             const int64_t* __restrict__ graph_free_ptr, float tol, int max_iter,
                                                             int32_t* __restrict__ counter) {
  const int g = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (g >= G) return;
  const int lane = threadIdx.x & 63;
  const uint32_t h_wave = draw_prefix(seed_lo, seed_hi, draw);
  float ke = 0.f;
  const int64_t s_beg = clampi(graph_star_ptr[g], 0, S), s_end = clampi(graph_star_ptr[g + 1], s_beg, S);
  // The lane's first free atom is read HERE, before its stars: the stars' chain of dependent loads (graph row -> star row -> atoms
  // -> their data) and the free atoms' (graph row -> atom -> its data) then run side by side instead of one after the other -- the
  // kernel is a handful of memory round trips and little else.  (No star owns a free atom, so the stars' stores do not touch it.)
  const int64_t f_beg = clampi(graph_free_ptr[g], 0, F), f_end = clampi(graph_free_ptr[g + 1], f_beg, F);
  const bool first_free = f_beg + lane < f_end;
  const int64_t i_first = first_free ? clampi(free_atom[f_beg + lane], 0, n - 1) : 0;
  const float m_first = first_free ? mass[i_first] : 1.0f;
  const AtomIn in_first = first_free ? load_atom(v, f, i_first) : AtomIn{};
  for (int64_t t = s_beg + lane; t < s_end; t += 64) {
    const StarRows st = load_star(star_ptr, star_atom, star_len, mass, t, n_slots, n);
    if (st.ns < 0) continue;
    float r[STAR_MAX - 1][3], r2[STAR_MAX - 1], u[STAR_MAX][3];
#pragma unroll
    for (int a = 0; a < STAR_MAX; ++a) {
      if (a <= st.ns) {
        ou_kick(load_atom(v, f, st.id[a]), f != nullptr, st.id[a], st.m[a], dt, c, s, h_wave, word0, u[a][0], u[a][1], u[a][2]);
      } else {
        u[a][0] = u[a][1] = u[a][2] = 0.f;
      }
      if (a > 0) {
#pragma unroll
        for (int d = 0; d < 3; ++d) r[a - 1][d] = a <= st.ns ? x[3 * st.id[a] + d] - x[3 * st.id[0] + d] : 0.f;
        r2[a - 1] = (r[a - 1][0] * r[a - 1][0] + r[a - 1][1] * r[a - 1][1]) + r[a - 1][2] * r[a - 1][2];
      }
    }
    bool fail = false;
    for (int it = 0; it <= max_iter; ++it) {      // passes as in md_drift_shake_kernel
      bool moved = false;
#pragma unroll
      for (int k = 0; k < STAR_MAX - 1; ++k) {
        if (k < st.ns) {
          const float wx = u[k + 1][0] - u[0][0], wy = u[k + 1][1] - u[0][1], wz = u[k + 1][2] - u[0][2];
          const float rv = (r[k][0] * wx + r[k][1] * wy) + r[k][2] * wz;
          const float nc = sqrtf((u[0][0] * u[0][0] + u[0][1] * u[0][1]) + u[0][2] * u[0][2]);
          const float nsat = sqrtf((u[k + 1][0] * u[k + 1][0] + u[k + 1][1] * u[k + 1][1]) + u[k + 1][2] * u[k + 1][2]);
          if (!(fabsf(rv) <= tol * st.d0[k] * (nc + nsat))) {
            moved = true;
            if (it < max_iter && r2[k] > 0.f) {
              const float gk = rv / (r2[k] * (st.inv_m[0] + st.inv_m[k + 1]));
              const float gs = gk * st.inv_m[k + 1], gc = gk * st.inv_m[0];
#pragma unroll
              for (int d = 0; d < 3; ++d) {
                u[k + 1][d] = u[k + 1][d] - gs * r[k][d];
                u[0][d] = u[0][d] + gc * r[k][d];
              }
            } else {
              fail = true;
            }
          }
        }
      }
      if (!moved) break;
    }
#pragma unroll
    for (int a = 0; a < STAR_MAX; ++a) {
      if (a <= st.ns) {
        const int64_t i = st.id[a];
        v[3 * i] = u[a][0];
        v[3 * i + 1] = u[a][1];
        v[3 * i + 2] = u[a][2];
        ke += 0.5f * st.m[a] * ((u[a][0] * u[a][0] + u[a][1] * u[a][1]) + u[a][2] * u[a][2]);
      }
    }
    if (fail) atomicAdd(counter, 1);
  }
  for (int64_t j = f_beg + lane; j < f_end; j += 64) {
    const bool first = j == f_beg + lane;
    const int64_t i = first ? i_first : clampi(free_atom[j], 0, n - 1);
    const float m = first ? m_first : mass[i];
    float vx, vy, vz;
    ou_kick(first ? in_first : load_atom(v, f, i), f != nullptr, i, m, dt, c, s, h_wave, word0, vx, vy, vz);
    v[3 * i] = vx;
    v[3 * i + 1] = vy;
    v[3 * i + 2] = vz;
    ke += 0.5f * m * ((vx * vx + vy * vy) + vz * vz);
  }
  ke = wave_sum(ke);
  if (lane == 0) {
    if (kinetic) kinetic[g] = ke;
    if (potential) potential[g] = energy[g];
  }
}

}  // namespace e3k

extern "C" int e3k_md_drift(float* x, float* v, const float* f, const float* mass, int64_t n, float dt, void* stream) {
  if (n < 0) return E3K_ERR_INVALID;
  if (n == 0) return E3K_OK;
  if (!x || !v || !f || !mass) return E3K_ERR_INVALID;
  hipLaunchKernelGGL(e3k::md_drift_kernel, dim3((unsigned)((3 * n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, v, f, mass,
                     3 * n, dt);
  E3K_CHECK_LAUNCH();
  return E3K_OK;
}

static int md_kick_launch(float* v, const float* f, const float* mass, const int64_t* node_ptr, int32_t G, int64_t n, float dt, float c,
                          float s, uint32_t seed_lo, uint32_t seed_hi, uint32_t draw, uint32_t word0, float* kinetic,
                          const float* energy, float* potential, void* stream) {
  hipLaunchKernelGGL(e3k::md_kick_kernel, dim3((unsigned)((G + 3) / 4)), dim3(256), 0, (hipStream_t)stream, v, f, mass, node_ptr, G, n,
                     dt, c, s, seed_lo, seed_hi, draw, word0, kinetic, energy, potential);
  E3K_CHECK_LAUNCH();
  return E3K_OK;
}

extern "C" int e3k_md_kick(float* v, const float* f, const float* mass, const int64_t* node_ptr, int32_t G, int64_t n, float dt,
                           float* kinetic, const float* energy, float* potential, void* stream) {
  if (n < 0 || G < 0) return E3K_ERR_INVALID;
  if (n == 0 || G == 0) return E3K_OK;
  if (!v || !f || !mass || !node_ptr || (potential && !energy)) return E3K_ERR_INVALID;
  return md_kick_launch(v, f, mass, node_ptr, G, n, dt, 1.0f, 0.f, 0u, 0u, 0u, 0u, kinetic, energy, potential, stream);
}

extern "C" int e3k_md_kick_langevin(float* v, const float* f, const float* mass, const int64_t* node_ptr, int32_t G, int64_t n, float dt,
                                    float c, float s, uint32_t seed_lo, uint32_t seed_hi, uint32_t draw, uint32_t word0,
                                    float* kinetic, const float* energy, float* potential, void* stream) {
  if (n < 0 || G < 0 || !(c >= 0.f && c <= 1.f) || !(s >= 0.f)) return E3K_ERR_INVALID;
  if (n == 0 || G == 0) return E3K_OK;
  if (!v || !mass || !node_ptr || (potential && !energy)) return E3K_ERR_INVALID;
  return md_kick_launch(v, f, mass, node_ptr, G, n, dt, c, s, seed_lo, seed_hi, draw, word0, kinetic, energy, potential, stream);
}

extern "C" int e3k_fire_step(float* x, float* v, const float* f, const int64_t* node_ptr, int32_t G, int64_t n, float* state,
                             float ftol, float dt_max, float maxstep, int32_t n_min, float f_inc, float f_dec, float alpha_start,
                             float f_alpha, const float* energy, float* energy_record, float* fmax_record, void* stream) {
  if (n < 0 || G < 0 || !(ftol >= 0.f) || !(dt_max > 0.f) || !(maxstep > 0.f) || n_min < 0) return E3K_ERR_INVALID;
  if (G == 0) return E3K_OK;
  if (!node_ptr || !state || (n > 0 && (!x || !v || !f)) || (energy_record && !energy)) return E3K_ERR_INVALID;
  const e3k::FireParams p{ftol, dt_max, maxstep, (float)n_min, f_inc, f_dec, alpha_start, f_alpha};
  hipLaunchKernelGGL(e3k::fire_step_kernel, dim3((unsigned)((G + 3) / 4)), dim3(256), 0, (hipStream_t)stream, x, v, f, node_ptr, G, n,
                     state, p, energy, energy_record, fmax_record);
  E3K_CHECK_LAUNCH();
  return E3K_OK;
}

static bool constraint_tables_ok(const int64_t* star_ptr, const int64_t* star_atom, const float* star_len, int64_t n_stars,
                                 int64_t n_slots, const int64_t* free_atom, int64_t n_free, int64_t n, float tol, int32_t max_iter,
                                 const int32_t* counter) {
  if (n < 0 || n_stars < 0 || n_slots < 0 || n_free < 0 || !(tol > 0.f) || max_iter < 1 || !counter) return false;
  if (n_stars > 0 && (!star_ptr || !star_atom || !star_len)) return false;
  if (n_free > 0 && !free_atom) return false;
  if (n_stars + n_free > 0 && n == 0) return false;
  return n_stars + n_free < (int64_t)1 << 31;
}

extern "C" int e3k_md_drift_shake(float* x, float* v, const float* f, const float* mass, int64_t n, float dt, const int64_t* star_ptr,
                                  const int64_t* star_atom, const float* star_len, int64_t n_stars, int64_t n_slots,
                                  const int64_t* free_atom, int64_t n_free, float tol, int32_t max_iter, int32_t* counter,
                                  void* stream) {
  if (!constraint_tables_ok(star_ptr, star_atom, star_len, n_stars, n_slots, free_atom, n_free, n, tol, max_iter, counter))
    return E3K_ERR_INVALID;
  if (f && !(dt != 0.f)) return E3K_ERR_INVALID;      // the velocity correction divides by dt
  if (n_stars + n_free == 0) return E3K_OK;
  if (!x || !v || !mass) return E3K_ERR_INVALID;
  hipLaunchKernelGGL(e3k::md_drift_shake_kernel, dim3((unsigned)((n_stars + n_free + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x,
                     v, f, mass, n, dt, star_ptr, star_atom, star_len, n_stars, n_slots, free_atom, n_free, tol, (int)max_iter,
                     counter);
  E3K_CHECK_LAUNCH();
  return E3K_OK;
}

extern "C" int e3k_md_kick_rattle(float* v, const float* f, const float* mass, const int64_t* node_ptr, int32_t G, int64_t n, float dt,
                                  float c, float s, uint32_t seed_lo, uint32_t seed_hi, uint32_t draw, uint32_t word0, float* kinetic,
                                  const float* energy, float* potential, const float* x, const int64_t* star_ptr,
                                  const int64_t* star_atom, const float* star_len, int64_t n_stars, int64_t n_slots,
                                  const int64_t* free_atom, int64_t n_free, const int64_t* graph_star_ptr,
                                  const int64_t* graph_free_ptr, float tol, int32_t max_iter, int32_t* counter, void* stream) {
  if (G < 0 || !(c >= 0.f && c <= 1.f) || !(s >= 0.f)) return E3K_ERR_INVALID;
  if (!constraint_tables_ok(star_ptr, star_atom, star_len, n_stars, n_slots, free_atom, n_free, n, tol, max_iter, counter))
    return E3K_ERR_INVALID;
  if (n == 0 || G == 0) return E3K_OK;
  if (!v || !mass || !node_ptr || !graph_star_ptr || !graph_free_ptr || (n_stars > 0 && !x) || (potential && !energy))
    return E3K_ERR_INVALID;
  hipLaunchKernelGGL(e3k::md_kick_rattle_kernel, dim3((unsigned)((G + 3) / 4)), dim3(256), 0, (hipStream_t)stream, v, f, mass, x, G, n,
                     dt, c, s, seed_lo, seed_hi, draw, word0, kinetic, energy, potential, star_ptr, star_atom, star_len, n_stars,
                     n_slots, free_atom, n_free, graph_star_ptr, graph_free_ptr, tol, (int)max_iter, counter);
  E3K_CHECK_LAUNCH();
  return E3K_OK;
}
