// The counter-based draw: the one definition of the stream that the capped list's pair criterion (e3k_nlist.hip), the thermostat
// and thermalize() (e3k_md.hip), the score step's perturbation (e3k_score.hip) and the seeded sampler (e3k_sampler.hip) read.  Nothing about a draw lives in a
// generator's state: a value is a function of five 32-bit words, so a step that is done again sees the same bits.
//
// The stream layout.  h = mix32(h ^ word) over the words, in this order, from 0x9E3779B9:
//     seed low, seed high, draw index, src, dst
//   * draw_prefix() is the chain over the first three: what does not depend on the node.
//   * src is a node index (N < 2^31), or 0xFFFFFFFF for a graph's time (then dst is the graph).
//   * src = 0xFFFFFFFE is a graph's barostat (e3k_barostat.hip): a standard normal for (that src, word = the graph), the draw index
//     being the absolute MD step, with the integrator's seed.
//   * a pair's Bernoulli draw: src = i, dst = j, the 32-bit hash against a threshold.
//   * a standard normal for (node, word): src = the node, dst = 2 word and 2 word + 1 give the two uniforms of normal_draw().
//   * the seeded sampler (e3k_sampler.hip; run/sde_utils.py restates it): D_total = the sum of the dimensions of the diffusion keys
//     (sde.irreps, in order), a key's word0 = the sum of the dimensions before it, src = the node, and for component c of a key
//         reverse step i (from 0), corrector noise:  draw index i,      word word0 + c
//         reverse step i, predictor noise:           draw index i,      word D_total + word0 + c
//         the prior x_T:                             draw index sde.N,  word word0 + c        (no step uses index sde.N)
//       and, for the rows that conditional sampling keeps on known values (get_pc_sampler(fixed=...)), the replacement's noise:
//         reverse step i, after the corrector:       draw index i,      word 2 D_total + word0 + c
//         reverse step i, after the predictor:       draw index i,      word 3 D_total + word0 + c
//       (the prior's fixed rows use the prior's own draw: m(T) x0 + s(T) z).  Blocks 0 and 1 and the prior are where they were, so an
//       unconditioned seeded run keeps its bits.
//       and, for the likelihood (run/likelihood.py; e3k_sampler_probe), the Hutchinson probes, fixed for a whole run:
//         probe p (from 0) of component c:           draw index sde.N + 1 + p,  word word0 + c
//       (no step and not the prior uses an index above sde.N).  A Rademacher probe is +1 when bit 31 of mix32(h_node ^ (2 word)) is
//       clear and -1 when it is set -- the hash normal_draw() makes its first uniform of; a Gaussian probe is normal_draw() itself.
//     The sampler's seed is an argument of its own and should differ from the pair criterion's: with one seed a node's noise and the
//     Bernoulli draws of its pairs at the same draw index come from one chain.
// data/compute_edge.py (_mix32, pair_hash, normal_draw) is the host restatement, in int64 masked to 32 bits.
#pragma once
#include <stdint.h>

#include <hip/hip_runtime.h>

namespace e3k {

// One round of the "lowbias32" integer finaliser (uint32 arithmetic).
__device__ __forceinline__ uint32_t mix32(uint32_t h) {
  h ^= h >> 16;
  h *= 0x7feb352du;
  h ^= h >> 15;
  h *= 0x846ca68bu;
  h ^= h >> 16;
  return h;
}

__device__ __forceinline__ uint32_t draw_prefix(uint32_t seed_lo, uint32_t seed_hi, uint32_t draw) {
  return mix32(mix32(mix32(0x9E3779B9u ^ seed_lo) ^ seed_hi) ^ draw);
}

// The 24-bit uniform in [0, 1) of a hash: exact in fp32.
__device__ __forceinline__ float uniform24(uint32_t h) { return (float)(h >> 8) * 0x1p-24f; }

// A standard normal for (seed, draw, node, word); h_node: the chain up to and including the node word.  u1 in (0, 1] and u2 in
// [0, 1), Box-Muller's cosine branch.  logf, sqrtf, cospif are the precise library functions; 2 u2 is exact, so the cosine sees no
// argument rounding.
__device__ __forceinline__ float normal_draw(uint32_t h_node, uint32_t word) {
  const uint32_t h1 = mix32(h_node ^ (2u * word)), h2 = mix32(h_node ^ (2u * word + 1u));
  const float u1 = (float)((h1 >> 8) + 1u) * 0x1p-24f, u2 = uniform24(h2);
  return sqrtf(-2.0f * logf(u1)) * cospif(2.0f * u2);
}

}  // namespace e3k
