// The batch descriptor of the grouped GEMM kernels and the pipelined weight-gradient body: shared by e3k_gemm.hip and the
// launch that runs the knot-table transpose beside the weight gradients (e3k_wgrad_rider.hip).  One text each.
#pragma once
#include "e3k_common.h"

namespace e3k {

typedef float f32x16 __attribute__((ext_vector_type(16)));

// 20 x 168 B of descriptors + tables = 3.85 KB of the 4 KB kernel-argument segment (round 6: 16 -> 20 -- the three weight gradients of a
// layer are 7 + 7 + 6 problems: with 16 per launch linear_1's last four went out as a second, 23 us launch of their own)
constexpr int GEMM_MAXP = 20;
struct GemmBatch {
  int n;
  int reps[GEMM_MAXP];              // > 1: the problem stands for `reps` key groups (its tile range is reps equal sub-ranges);
  long long key_stride[GEMM_MAXP];  //      key t uses B + t*key_stride and the device pair group_dev + 2*t
  int tile_start[GEMM_MAXP + 1];
  int flags[GEMM_MAXP];  // bit0: A float4-loadable, bits1-2: B mode (0 scalar, 1 n-contiguous vec, 2 k-contiguous vec), bit3: G float4-loadable (wgrad)
  int aux[GEMM_MAXP];    // wgrad: row splits (compact keyed grid: rows per split)
  e3k_gemm_problem p[GEMM_MAXP];
};
static_assert(sizeof(GemmBatch) % 4 == 0 && sizeof(e3k_gemm_problem) % 4 == 0, "word-copyable descriptors");
static_assert(sizeof(GemmBatch) + 16 <= 4096, "the batch travels by value in the kernel-argument segment");

struct BlockProblem {
  e3k_gemm_problem P;
  int flags, aux, local;
  int pi, key;      // index of the problem in the batch; key group of a keyed problem (0 otherwise): what a K-chain's followers reuse
};

// COMPACT keyed grids (round 6; flags bit 6, gemm_kernel and gemm_wgrad2_kernel): a keyed problem used to get `reps` x the tiles of its
// row bound M1 -- every key a full-size grid, the workgroups past a key's last row exit after reading their descriptor: 8 377
// workgroups for ~1 300 tiles of work in a layer's linear_1 + self-connection launch, nine rounds of empty workgroups through the
// CUs.  The key groups PARTITION the rows, so sum_k ceil(count_k M2 / bm) <= ceil(M1 M2 / bm) + reps row tiles suffice: a workgroup
// finds its key by walking the (<= 32) device-side counts.  `bm`: rows per tile; `cols(P, aux)`: workgroups per row tile.
template <class Cols>
__device__ __forceinline__ BlockProblem fetch_problem(const GemmBatch& gb, int bm, Cols cols);
struct NoCols {
  __device__ int operator()(const e3k_gemm_problem&, int) const { return 1; }
};
__device__ __forceinline__ BlockProblem fetch_problem(const GemmBatch& gb) { return fetch_problem(gb, 0, NoCols{}); }

template <class Cols>
__device__ __forceinline__ BlockProblem fetch_problem(const GemmBatch& gb, int bm, Cols cols) {
  // The batch lives in the kernel-argument segment: everything here is wave-uniform, so the compiler reads it with
  // scalar loads (s_load_dwordxN at a uniform dynamic offset) straight into SGPRs — no LDS copy, no barrier.
  const int n = gb.n;
  int pi = 0;
#pragma unroll
  for (int i = 1; i < GEMM_MAXP; ++i)
    if (i < n && (int)blockIdx.x >= gb.tile_start[i]) pi = i;
  pi = uniform(pi);
  BlockProblem out;
  out.local = blockIdx.x - gb.tile_start[pi];
  out.flags = gb.flags[pi];
  out.aux = gb.aux[pi];
  out.P = gb.p[pi];
  out.pi = pi;
  out.key = 0;
  const int reps = gb.reps[pi];
  if (reps > 1 && bm != 0 && (out.flags & 64)) {      // compact keyed grid
    if (bm < 0) bm = out.aux;                           // (the weight gradient's row tile = the rows of one split: in aux)
    const int c = cols(out.P, out.aux);
    const int rt = out.local / c, col = out.local - rt * c;
    int key = -1, rt_local = 0, base = 0;
    for (int k = 0; k < reps; ++k) {
      int cnt = uniform(out.P.group_dev[2 * k + 1]);
      cnt = cnt < out.P.M1 ? cnt : out.P.M1;
      const int t = (cnt * out.P.M2 + bm - 1) / bm;
      if (key < 0 && rt < base + t) {
        key = k;
        rt_local = rt - base;
      }
      base += t;
    }
    if (key < 0) {      // surplus workgroup (the grid is sized by the bound)
      out.local = -1;
      return out;
    }
    out.local = rt_local * c + col;
    out.P.B += (int64_t)key * gb.key_stride[pi];
    out.P.group_dev += 2 * key;
    out.key = key;
  } else if (reps > 1) {  // keyed problem: which key group this workgroup belongs to
    const int per_key = (gb.tile_start[pi + 1] - gb.tile_start[pi]) / reps;
    const int key = out.local / per_key;
    out.local -= key * per_key;
    out.P.B += (int64_t)key * gb.key_stride[pi];
    out.P.group_dev += 2 * key;
    out.key = key;
  }
  if (out.P.row_index && out.P.group_dev) {  // device-side {start, count} of this key group
    const int start = uniform(out.P.group_dev[0]), count = uniform(out.P.group_dev[1]);
    out.P.row_index += start;
    out.P.M1 = count < out.P.M1 ? count : out.P.M1;
  }
  return out;
}

// ---------------------------------------------------------------------------------------
// wgrad, software-pipelined form (round 4).  What the round's measurements say about the form above on the node-side
// problems (4 608 nodes, K = 384, N = 64, rows 3 or 5 per node): its time is a fixed 8-19 us per 64-row chunk and
// workgroup whatever the number of co-resident workgroups -- the loop is one load latency long per chunk (loads issued
// one chunk ahead, behind a barrier, waited for in front of the next) -- and it pays 16 KB of float atomics per 256 rows
// (the chip adds 1.3 TB/s of atomic bytes, MI355X_MICROARCH.md "Global float atomics").  Here: (i) two LDS stages, the
// loads of chunk c + 2 in flight while chunk c is in the matrix pipe: one barrier per chunk and two chunk times for a
// load to land; (ii) tile 128 k x 64 n (WKW = 4 waves along k, two accumulators each: the G fragment pair is reused by
// every wave, A is still read once) or 64 k x 64 n (WKW = 2) for K <= 64; (iii) the launch is sized to ONE round of
// workgroups -- three per CU, what LDS admits -- with EQUAL row ranges per workgroup (splits proportional to a problem's
// rows), so a workgroup adds its tile once per ~1/768 of the launch's work (measured: 256 / 512 / 768 / 1 024 workgroups
// 70 / 73 / 59 / 72 us on the trailing Linear: a second, partial round costs what it saves); (iv) row pointers advanced by
// constant 64-bit deltas instead of two 64-bit multiplies per load and chunk; gathered rows (IDX) through node indices
// fetched one chunk ahead.
// ---------------------------------------------------------------------------------------
constexpr int W2R = 32;   // rows per chunk
template <int WKW, bool IDX>
__device__ __forceinline__ void gemm_wgrad2_body(const BlockProblem& bp_, float* As_, float* Gs_) {
  constexpr int TK = 32 * WKW;            // k per tile
  constexpr int WNW = 4 / WKW;            // waves along n
  constexpr int NT = 2 / WNW;             // accumulators per wave (tile is 64 n wide)
  constexpr int LDA2 = TK + 4, LDG2 = 64 + 4;
  constexpr int APASS = (W2R * TK / 4) / 256;     // float4 loads of A per thread and chunk (4 or 2)
  constexpr int AROWS = 256 / (TK / 4);           // rows covered by one pass (8 or 16)
  float (*As)[W2R * LDA2] = reinterpret_cast<float (*)[W2R * LDA2]>(As_);
  float (*Gs)[W2R * LDG2] = reinterpret_cast<float (*)[W2R * LDG2]>(Gs_);
  const e3k_gemm_problem& P = bp_.P;
  const int local = bp_.local;
  const int M = P.M1 * P.M2, M2 = P.M2;
  const int tiles_k = (P.K + TK - 1) / TK, tiles_n = (P.N + 63) / 64;
  const int splits = bp_.aux;
  const int tile = local % (tiles_k * tiles_n), split = local / (tiles_k * tiles_n);
  const int k0 = (tile / tiles_n) * TK, n0 = (tile % tiles_n) * 64;
  // (compact keyed grid, flags bit 6: aux IS the rows per split -- the same for every key: fetch_problem)
  const int chunk_rows = (bp_.flags & 64) ? splits : ((M + splits - 1) / splits + W2R - 1) / W2R * W2R;
  const int rbeg = split * chunk_rows;
  const int rend = (rbeg + chunk_rows < M) ? rbeg + chunk_rows : M;
  if (rbeg >= M) return;
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const int wk = wv % WKW, wn = wv / WKW;
  const int qR = W2R / M2, remR = W2R - qR * M2;

  f32x16 acc[NT];
#pragma unroll
  for (int j = 0; j < NT; ++j)
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[j][i] = 0.f;

  // this thread's rows of a chunk: A pass p -> row (t / (TK/4)) + AROWS*p, G pass p -> row (t >> 4) + 16*p.  Plain problems:
  // row pointers advance by constant 64-bit deltas (one chunk down, and the wrap of the component index r2).  Gathered
  // rows (IDX: the keyed self-connection, rows = the nodes of one key through row_index): the node index of a row is
  // fetched one chunk ahead, behind the chunk's float4 loads, so that it has landed with them
  int aR[APASS], ar1[APASS], ar2[APASS], gR[2], gr1[2], gr2[2];
  int ia[APASS], ig[2];
  const float* pa[APASS];
  const float* pg[2];
  const int64_t dA = (int64_t)qR * P.a_r1 + (int64_t)remR * P.a_r2, wA = P.a_r1 - (int64_t)M2 * P.a_r2;
  const int64_t dG = (int64_t)qR * P.c_r1 + (int64_t)remR * P.c_r2, wG = P.c_r1 - (int64_t)M2 * P.c_r2;
  const int acol = (t % (TK / 4)) * 4, gcol = (t & 15) * 4;
  const bool a_in = k0 + acol < P.K, g_in = n0 + gcol < P.N;
#pragma unroll
  for (int p = 0; p < APASS; ++p) {
    aR[p] = rbeg + t / (TK / 4) + AROWS * p;
    ar1[p] = aR[p] / M2;
    ar2[p] = aR[p] - ar1[p] * M2;
    pa[p] = P.A + (int64_t)ar1[p] * P.a_r1 + (int64_t)ar2[p] * P.a_r2 + k0 + acol;
    ia[p] = (IDX && aR[p] < rend) ? P.row_index[ar1[p]] : 0;
  }
#pragma unroll
  for (int p = 0; p < 2; ++p) {
    gR[p] = rbeg + (t >> 4) + 16 * p;
    gr1[p] = gR[p] / M2;
    gr2[p] = gR[p] - gr1[p] * M2;
    pg[p] = P.C + (int64_t)gr1[p] * P.c_r1 + (int64_t)gr2[p] * P.c_r2 + n0 + gcol;
    ig[p] = (IDX && gR[p] < rend) ? P.row_index[gr1[p]] : 0;
  }
  float4 ra[APASS], rg[2];
  auto gload = [&]() {
#pragma unroll
    for (int p = 0; p < APASS; ++p) {
      ra[p] = make_float4(0.f, 0.f, 0.f, 0.f);
      if constexpr (IDX) {
        if (aR[p] < rend && a_in)
          ra[p] = *reinterpret_cast<const float4*>(P.A + (int64_t)ia[p] * P.a_r1 + (int64_t)ar2[p] * P.a_r2 + k0 + acol);
        aR[p] += W2R; ar1[p] += qR; ar2[p] += remR;
        if (ar2[p] >= M2) { ar2[p] -= M2; ++ar1[p]; }
      } else {
        if (aR[p] < rend && a_in) ra[p] = *reinterpret_cast<const float4*>(pa[p]);
        aR[p] += W2R; ar2[p] += remR; pa[p] += dA;
        if (ar2[p] >= M2) { ar2[p] -= M2; pa[p] += wA; }
      }
    }
#pragma unroll
    for (int p = 0; p < 2; ++p) {
      rg[p] = make_float4(0.f, 0.f, 0.f, 0.f);
      if constexpr (IDX) {
        if (gR[p] < rend && g_in)
          rg[p] = *reinterpret_cast<const float4*>(P.C + (int64_t)ig[p] * P.c_r1 + (int64_t)gr2[p] * P.c_r2 + n0 + gcol);
        gR[p] += W2R; gr1[p] += qR; gr2[p] += remR;
        if (gr2[p] >= M2) { gr2[p] -= M2; ++gr1[p]; }
      } else {
        if (gR[p] < rend && g_in) rg[p] = *reinterpret_cast<const float4*>(pg[p]);
        gR[p] += W2R; gr2[p] += remR; pg[p] += dG;
        if (gr2[p] >= M2) { gr2[p] -= M2; pg[p] += wG; }
      }
    }
    if constexpr (IDX) {      // node indices of the NEXT chunk's rows
#pragma unroll
      for (int p = 0; p < APASS; ++p) ia[p] = aR[p] < rend ? P.row_index[ar1[p]] : 0;
#pragma unroll
      for (int p = 0; p < 2; ++p) ig[p] = gR[p] < rend ? P.row_index[gr1[p]] : 0;
    }
  };
  auto lstore = [&](int st) {
#pragma unroll
    for (int p = 0; p < APASS; ++p)
      *reinterpret_cast<float4*>(&As[st][(t / (TK / 4) + AROWS * p) * LDA2 + acol]) = ra[p];
#pragma unroll
    for (int p = 0; p < 2; ++p) *reinterpret_cast<float4*>(&Gs[st][((t >> 4) + 16 * p) * LDG2 + gcol]) = rg[p];
  };
  const int n_chunks = (rend - rbeg + W2R - 1) / W2R;
  gload();
  lstore(0);
  if (n_chunks > 1) gload();
  __syncthreads();
  const int aoff = (lane >> 5) * LDA2 + wk * 32 + (lane & 31);
  const int goff = (lane >> 5) * LDG2 + wn * (32 * NT) + (lane & 31);
  for (int c = 0; c < n_chunks; ++c) {
    const int st = c & 1;
    if (c + 1 < n_chunks) lstore(st ^ 1);
    if (c + 2 < n_chunks) gload();
    const float* ap = &As[st][aoff];
    const float* gp = &Gs[st][goff];
#pragma unroll
    for (int rr = 0; rr < W2R; rr += 2) {
      const float a = ap[rr * LDA2];
#pragma unroll
      for (int j = 0; j < NT; ++j) acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, gp[rr * LDG2 + 32 * j], acc[j], 0, 0, 0);
    }
    __syncthreads();
  }
#pragma unroll
  for (int j = 0; j < NT; ++j) {
    const int n = n0 + wn * (32 * NT) + 32 * j + (lane & 31);
    if (n < P.N) {
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int k = k0 + wk * 32 + (i & 3) + 8 * (i >> 2) + 4 * (lane >> 5);
        if (k < P.K) atomicAdd(const_cast<float*>(P.B) + (int64_t)k * P.b_k + (int64_t)n * P.b_n, P.alpha * acc[j][i]);
      }
    }
  }
}

// one kernel for both tile shapes (a call's K > 64 and K <= 64 problems share a launch); registers and LDS are the wide form's
constexpr int W2_AS_FLOATS = 2 * W2R * (128 + 4), W2_GS_FLOATS = 2 * W2R * (64 + 4);
__device__ __forceinline__ void gemm_wgrad2_block(const GemmBatch& gb, float* As, float* Gs) {
  const BlockProblem bp_ = fetch_problem(gb, -1, [](const e3k_gemm_problem& Q, int) {
    return ((Q.K + (Q.K > 64 ? 127 : 63)) / (Q.K > 64 ? 128 : 64)) * ((Q.N + 63) / 64);
  });
  if (bp_.local < 0) return;      // (block-uniform: surplus workgroup of a compact keyed grid)
  if (bp_.P.row_index) {
    if (bp_.P.K > 64) gemm_wgrad2_body<4, true>(bp_, As, Gs);
    else gemm_wgrad2_body<2, true>(bp_, As, Gs);
  } else {
    if (bp_.P.K > 64) gemm_wgrad2_body<4, false>(bp_, As, Gs);
    else gemm_wgrad2_body<2, false>(bp_, As, Gs);
  }
}

// Host side.  A weight-gradient call (e3k_gemm_multi with wgrad = 1) whose FIRST pipelined batch goes out through `launch`
// instead of as gemm_wgrad2_kernel: that batch is sized to `wg_per_cu` workgroups per CU (e3k_gemm.hip, gemm_wgrad_impl; the
// stand-alone launch, and any further batch of the call, takes three).  Everything else of the call -- validation before the first launch, the one-column and the
// outer-product problems, further batches -- is the plain call's.  `used` reports whether a batch went that way.
struct WgradHook {
  void (*launch)(const GemmBatch& gb, int blocks, hipStream_t st, void* ctx);
  void* ctx;
  double wg_per_cu;
  bool used;
};
int gemm_multi_wgrad_hooked(const e3k_gemm_segment* segments, int32_t n_segments, void* stream, WgradHook* hook);
// empties the calling thread's launch record (e3k_gemm_last_routes): for an entry that may refuse before it reaches a GEMM call
void gemm_routes_clear();

}  // namespace e3k
