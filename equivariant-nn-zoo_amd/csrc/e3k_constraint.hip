// Bond-length constraints for the velocity-Verlet updates of e3k_nlist.hip (run/md.py: BondConstraints): SHAKE in the first half
// step, RATTLE in the second.  A constrained step stays the force graph + two launches: these kernels REPLACE e3k_md_drift and
// e3k_md_kick / e3k_md_kick_langevin, they do not follow them.
//
// The constraints are disjoint STARS: a centre with 1..4 satellites, every constraint centre--satellite, no atom in two stars (the
// bonds-to-hydrogen set).  One thread owns a star, so nothing is shared: no atomics in the arithmetic, the same bits every run.
// Tables (built once by the host): star_ptr [S + 1] into star_atom / star_len [n_slots] -- per star the centre, then its satellites,
// each satellite's length beside it (the centre's slot holds 0); free_atom [F]: the atoms in no star; both sorted by graph, with
// graph_star_ptr / graph_free_ptr [G + 1].  Every index read from a table is clamped before it is used as an address.
//
// The free atoms take the expressions of md_drift_kernel / md_kick_langevin_kernel unchanged (and, within a graph, that kernel's
// order of the kinetic sum): with no star at all the two kernels here give those kernels' values (at s = 0 the
// draw is skipped where that kernel adds an exact zero).
//
// A star that does not converge within max_iter sweeps (or, in SHAKE, whose moved bond has turned against the old one) adds one to a
// device counter and is written as it stands: valid numbers, wrong physics -- reported, like the neighbour list's overflow.
#include "e3k_common.h"

namespace e3k {

constexpr int STAR_MAX = 5;      // centre + at most four satellites (CH4, NH4+)

// (restated from e3k_nlist.hip, which restates e3k_edge.hip: the file is built with -ffp-contract=fast; the empty asm makes the
//  rounded product a value the optimiser has to materialise)
__device__ __forceinline__ float con_rounded_product(float a, float b) {
  float p = a * b;
  asm volatile("" : "+v"(p));
  return p;
}

__device__ __forceinline__ int64_t con_clampi(int64_t v, int64_t lo, int64_t hi) { return v < lo ? lo : (v > hi ? hi : v); }

__device__ __forceinline__ uint32_t con_mix32(uint32_t h) {
  h ^= h >> 16;
  h *= 0x7feb352du;
  h ^= h >> 15;
  h *= 0x846ca68bu;
  h ^= h >> 16;
  return h;
}

// e3k_nlist.hip's normal_draw: the standard normal of (seed, draw, node, word), the same bits as the unconstrained thermostat's
__device__ __forceinline__ float con_normal_draw(uint32_t h_node, uint32_t word) {
  const uint32_t h1 = con_mix32(h_node ^ (2u * word)), h2 = con_mix32(h_node ^ (2u * word + 1u));
  const float u1 = (float)((h1 >> 8) + 1u) * 0x1p-24f, u2 = (float)(h2 >> 8) * 0x1p-24f;
  return sqrtf(-2.0f * logf(u1)) * cospif(2.0f * u2);
}

// md_kick_langevin_kernel's update of one atom: v <- c v + (s / sqrt(m)) xi, then v += dt/2 f / m (kick false: skipped).  s == 0 (a
// uniform branch: NVE, project()) draws nothing -- that kernel adds an exact zero there, so the values are the same; a lane here
// owns up to five atoms, and fifteen logarithms and cosines for nothing would be a fifth of the kernel's time.
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
    const uint32_t h_i = con_mix32(h_wave ^ (uint32_t)i);
    vx = con_rounded_product(c, in.v[0]) + con_rounded_product(a, con_normal_draw(h_i, word0));
    vy = con_rounded_product(c, in.v[1]) + con_rounded_product(a, con_normal_draw(h_i, word0 + 1u));
    vz = con_rounded_product(c, in.v[2]) + con_rounded_product(a, con_normal_draw(h_i, word0 + 2u));
  } else {
    vx = con_rounded_product(c, in.v[0]);
    vy = con_rounded_product(c, in.v[1]);
    vz = con_rounded_product(c, in.v[2]);
  }
  if (kick) {
    const float h = 0.5f * dt / m;
    vx = vx + h * in.f[0];
    vy = vy + h * in.f[1];
    vz = vz + h * in.f[2];
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
  const int64_t beg = con_clampi(star_ptr[t], 0, n_slots), end = con_clampi(star_ptr[t + 1], beg, n_slots);
  const int cnt = (int)(end - beg < STAR_MAX ? end - beg : STAR_MAX);
  r.ns = cnt - 1;
#pragma unroll
  for (int a = 0; a < STAR_MAX; ++a) {
    const bool on = a < cnt;
    r.id[a] = on ? con_clampi(star_atom[beg + a], 0, n - 1) : (a > 0 ? r.id[0] : 0);
    r.m[a] = on ? mass[r.id[a]] : 1.0f;
    r.inv_m[a] = on ? 1.0f / r.m[a] : 0.f;
    if (a > 0) r.d0[a - 1] = on ? star_len[beg + a] : 0.f;
  }
  return r;
}

// First half step with SHAKE.  Threads [0, S): one star each; threads [S, S + F): one free atom each (md_drift_kernel's expressions).
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
    const int64_t i = con_clampi(free_atom[t - S], 0, n - 1);
    const float m = mass[i];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float vn = v[3 * i + c] + (0.5f * dt) * f[3 * i + c] / m;
      v[3 * i + c] = vn;
      x[3 * i + c] = x[3 * i + c] + dt * vn;
    }
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
      p[a][c] = f ? rel + con_rounded_product(dt, vh[a][c]) : rel;
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
// l, l + 64, ...  Every atom gets md_kick_langevin_kernel's update (c = 1, s = 0: the plain kick; f NULL: no kick); a star's
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
  const uint32_t h_wave = con_mix32(con_mix32(con_mix32(0x9E3779B9u ^ seed_lo) ^ seed_hi) ^ draw);
  float ke = 0.f;
  const int64_t s_beg = con_clampi(graph_star_ptr[g], 0, S), s_end = con_clampi(graph_star_ptr[g + 1], s_beg, S);
  // The lane's first free atom is read HERE, before its stars: the stars' chain of dependent loads (graph row -> star row -> atoms
  // -> their data) and the free atoms' (graph row -> atom -> its data) then run side by side instead of one after the other -- the
  // kernel is a handful of memory round trips and little else.  (No star owns a free atom, so the stars' stores do not touch it.)
  const int64_t f_beg = con_clampi(graph_free_ptr[g], 0, F), f_end = con_clampi(graph_free_ptr[g + 1], f_beg, F);
  const bool first_free = f_beg + lane < f_end;
  const int64_t i_first = first_free ? con_clampi(free_atom[f_beg + lane], 0, n - 1) : 0;
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
    const int64_t i = first ? i_first : con_clampi(free_atom[j], 0, n - 1);
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
