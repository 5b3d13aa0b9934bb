// Grouped strided GEMM on the gfx950 f32 matrix pipe (v_mfma_f32_32x32x2_f32: exact fp32 FMA
// chain, 64 FLOP/clk/SIMD — cdna_hip_programming.md §3 "FP32-input MFMA").
//
// Replaces on the node / edge side of a convolution layer (paths relative to /root/reference):
//   o3.Linear                          e3_layers/nn/message_passing.py:58,102; nn/pointwise.py:18,87,142
//   FullyConnectedNet layers           e3_layers/nn/message_passing.py:74,93      (radial MLP)
//   FullyConnectedTensorProduct (sc)   e3_layers/nn/message_passing.py:83,100     (outer mode)
//
// One problem:  C[(r1,r2), n] = alpha * sum_k Aeff[(r1,r2), k] B[k, n]  (+ C) (+ bias[n]),  rows are
// (r1 < M1 nodes/edges, r2 < M2 = 2l+1 components) with independent strides, so the same kernels
// serve the e3nn layout ([mul][2l+1]) and the channel-fastest layout ([2l+1][mul]).
//
// Kernels (256 threads = 4 waves, 32x32x2 f32 MFMA accumulators):
//   gemm_kernel<WM>     forward / dgrad.  Tile (32*WM) x 64 x 32; the library ships WM=2 only: 64x64 (wave = 32 x 32;
//                       the 128-row form WM=4 lost to it at every size measured and was removed).  A tile in LDS at an odd row stride (33): the MFMA A
//                       fragment (lane -> row l&31, k l>>5) is bank-conflict free; B tile [k][n].  Global
//                       loads are 16 B/lane into registers one K-step ahead of the MFMAs (issue early,
//                       write LDS late).  dgrad (dA = dC . B^T) = same kernel, b_k / b_n swapped.
//   gemm_outer_kernel   self-connection: Aeff[(r1,r2), u*V+v] = X[(r1,r2),u] * attrs[r1,v]; X and attrs
//                       tiles sit in LDS for the whole K loop, the product is formed when the fragment is
//                       read, so x (x) node_attrs (N x 1280 x (2l+1)) is never materialised.
//   gemm_wgrad_kernel   B[k,n] += alpha * sum_rows Aeff[row,k] G[row,n]: tile 64 k x (64 or 128) n, rows
//                       split over blocks, 64-row chunks staged in natural row-major order (both MFMA
//                       operands conflict-free), fp32 atomics on the small output.
//
// Descriptors: up to 20 problems per launch, passed by value (3.85 KB of kernel arguments); keyed and plain problems mix; every
// workgroup finds its problem and pulls it into scalar registers with s_load (the batch is wave-uniform).
#include <algorithm>
#include <cstdio>
#include <cstring>

#include "e3k_common.h"
#include "e3k_gemm_batch.h"

namespace e3k {

// (GemmBatch, BlockProblem, fetch_problem: e3k_gemm_batch.h)

constexpr int BN = 64, BK = 32;
constexpr int LDA = BK + 1;
constexpr int LDB = BN;
constexpr int XU = 64;          // outer mode: channels of X kept per super-step
constexpr int LDX = XU + 1;
constexpr int VMAX = 32;        // outer mode: max attrs width
constexpr int LDV = VMAX + 1;


// K-chain (round 6): problem pi + j, j = 1 .. P.chain of the head, continues the head's K loop into the SAME accumulators -- another A
// block times another B block summed into the same C tile (the input gradient of an irrep that feeds two outputs of a Linear:
// `64x0e` and the gates' `256x0e` both read `0e`; until now the second one was an accumulating second launch, 21 us of a
// layer's backward for 0.4 GFLOP).  A follower has its head's rows, columns, C and key groups; it brings A, B, K, their strides
// and alpha.  Zero tiles of its own: no workgroup ever finds it through tile_start.
__device__ __forceinline__ void fetch_follower(const GemmBatch& gb, int idx, const BlockProblem& head, BlockProblem& out) {
  out.P = gb.p[idx];
  out.flags = gb.flags[idx];
  if (gb.reps[idx] > 1) {
    out.P.B += (int64_t)head.key * gb.key_stride[idx];
    out.P.group_dev += 2 * head.key;
  }
  if (out.P.row_index && out.P.group_dev) {
    const int start = uniform(out.P.group_dev[0]), count = uniform(out.P.group_dev[1]);
    out.P.row_index += start;
    out.P.M1 = count < out.P.M1 ? count : out.P.M1;
  }
}

__device__ __forceinline__ float epilogue_act(const e3k_gemm_problem& P, float v) {
  if (P.act == 1) v = P.act_cst * (fmaxf(v, 0.f) + log1pf(expf(-fabsf(v))) - 0.6931471805599453f);  // shifted softplus
  return v;
}

struct BRegs {
  float4 v[2];
};

// B tile (BK x BN) global -> registers (vector modes only; issued early, written to LDS late).  ONE load statement per
// register whatever the mode: with a load in each arm of `if (bmode == 1) ... else ...` the two arms write the same
// registers, the structurised control flow keeps an edge from one arm into the other, and the compiler protects the second
// arm's zero-initialisation with s_waitcnt vmcnt(0) -- which, on the forward path, waited for the A loads issued just
// before, i.e. the K-step prefetch never overlapped the MFMAs (found in round 4 with timing-only ablations: the phases of
// these kernels added up).
__device__ __forceinline__ void load_b_regs(const e3k_gemm_problem& P, int bmode, int k0, int n0, BRegs& r) {
  const int t = threadIdx.x;
  const bool m1 = bmode == 1;
#pragma unroll
  for (int pass = 0; pass < 2; ++pass) {
    // mode 1: row k = (t >> 4) + 16 pass, columns nq..nq+3;  mode 2 (B^T view, contiguous along k): column n = t & 63, k = kq + 4 pass
    const int k = m1 ? (t >> 4) + 16 * pass : (t >> 6) * 8 + 4 * pass;
    const int n = m1 ? (t & 15) * 4 : (t & 63);
    const int64_t off = m1 ? (int64_t)(k0 + k) * P.b_k + (n0 + n) : (int64_t)(n0 + n) * P.b_n + (k0 + k);
    r.v[pass] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (k0 + k < P.K && n0 + n < P.N) r.v[pass] = *reinterpret_cast<const float4*>(P.B + off);
  }
}

__device__ __forceinline__ void store_b_regs(int bmode, const BRegs& r, float* Bs) {
  const int t = threadIdx.x;
  if (bmode == 1) {
#pragma unroll
    for (int pass = 0; pass < 2; ++pass) {
      const int k = (t >> 4) + 16 * pass, nq = (t & 15) * 4;
      *reinterpret_cast<float4*>(Bs + k * LDB + nq) = r.v[pass];
    }
  } else {
    const int n = t & 63, kq = (t >> 6) * 8;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int k = kq + 4 * h;
      Bs[(k + 0) * LDB + n] = r.v[h].x;
      Bs[(k + 1) * LDB + n] = r.v[h].y;
      Bs[(k + 2) * LDB + n] = r.v[h].z;
      Bs[(k + 3) * LDB + n] = r.v[h].w;
    }
  }
}

// generic (scalar) B staging straight to LDS
__device__ __forceinline__ void stage_b_scalar(const e3k_gemm_problem& P, int k0, int n0, float* Bs) {
  const int t = threadIdx.x;
  const int n = t & 63, kb = t >> 6;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int k = kb + 4 * j;
    float v = 0.f;
    if (n0 + n < P.N && k0 + k < P.K) v = P.B[(int64_t)(k0 + k) * P.b_k + (int64_t)(n0 + n) * P.b_n];
    Bs[k * LDB + n] = v;
  }
}

// row tables of a tile: element offsets of its A and C rows (-1 = out of range); one integer
// division per row per block instead of one per staged / stored element
template <int ROWS>
__device__ __forceinline__ void fill_row_tables(const e3k_gemm_problem& P, int row0, int M, long long* rowA,
                                                long long* rowC) {
  const int t = threadIdx.x;
  if (t < ROWS) {
    const int R = row0 + t;
    long long oa = -1, oc = -1;
    if (R < M) {
      int r1 = R / P.M2;
      const int r2 = R - r1 * P.M2;
      if (P.row_index) r1 = P.row_index[r1];
      oa = (long long)r1 * P.a_r1 + (long long)r2 * P.a_r2;
      oc = (long long)r1 * P.c_r1 + (long long)r2 * P.c_r2;
    }
    rowA[t] = oa;
    rowC[t] = oc;
  }
}

// stores NT 32x32 accumulators of one wave: rows wrow0.., columns ncol0 + 32*j.  Accumulating problems (C += ...) read ALL
// their old values first and store afterwards: written as load-add-store per element the compiler must assume that a store
// aliases the next element's load and waits for every load on its own -- 32 dependent memory round trips per wave (the
// input gradient of linear_1 on top of the self-connection's: 137 us for 0.7 GFLOP, found in round 4's launch census).
template <int NT>
__device__ __forceinline__ void store_acc(const e3k_gemm_problem& P, const f32x16 (&acc)[NT], const long long* rowC,
                                          int wrow0, int ncol0) {
  const int lane = threadIdx.x & 63;
  int n[NT];
  bool ok[NT];
  float bias[NT];
  long long cn[NT];
#pragma unroll
  for (int j = 0; j < NT; ++j) {
    n[j] = ncol0 + 32 * j + (lane & 31);
    ok[j] = n[j] < P.N;
    bias[j] = (P.bias && ok[j]) ? P.bias[n[j]] : 0.f;
    cn[j] = (long long)n[j] * P.c_n;
  }
  long long off[16];
  bool inside = true;
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    off[i] = rowC[wrow0 + (i & 3) + 8 * (i >> 2) + 4 * (lane >> 5)];
    inside = inside && off[i] >= 0;
  }
#pragma unroll
  for (int j = 0; j < NT; ++j) inside = inside && ok[j];
  if (__all(inside)) {
    // interior tile (almost all of them): straight-line code -- every old value requested, then every result stored; with a
    // predicate around each element the compiler waits (vmcnt(0), which also covers the stores issued so far) per element
    float v[NT][16];
    if (P.accumulate) {
#pragma unroll
      for (int i = 0; i < 16; ++i)
#pragma unroll
        for (int j = 0; j < NT; ++j) v[j][i] = P.C[off[i] + cn[j]];
#pragma unroll
      for (int i = 0; i < 16; ++i)
#pragma unroll
        for (int j = 0; j < NT; ++j) v[j][i] += fmaf(P.alpha, acc[j][i], bias[j]);
    } else {
#pragma unroll
      for (int i = 0; i < 16; ++i)
#pragma unroll
        for (int j = 0; j < NT; ++j) v[j][i] = fmaf(P.alpha, acc[j][i], bias[j]);
    }
    if (P.act == 1) {
#pragma unroll
      for (int i = 0; i < 16; ++i)
#pragma unroll
        for (int j = 0; j < NT; ++j) v[j][i] = epilogue_act(P, v[j][i]);
    }
#pragma unroll
    for (int i = 0; i < 16; ++i)
#pragma unroll
      for (int j = 0; j < NT; ++j) P.C[off[i] + cn[j]] = v[j][i];
    return;
  }
  // edge tile: per-element predicates
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    if (off[i] < 0) continue;
    float* c = P.C + off[i];
#pragma unroll
    for (int j = 0; j < NT; ++j) {
      if (ok[j]) {
        float v = fmaf(P.alpha, acc[j][i], bias[j]);
        if (P.accumulate) v += c[cn[j]];
        c[cn[j]] = epilogue_act(P, v);
      }
    }
  }
}

// ---------------------------------------------------------------------------------------
// plain forward / dgrad, tile (32*WM) x 64 x 32
// ---------------------------------------------------------------------------------------
// CHAIN: the launch holds K-chains (e3k.h: e3k_gemm_problem.chain).  A second instantiation: the loop over a chain's links around the
// body costs the compiler 56 more registers (100 -> 156: three waves per SIMD instead of five); launches without chains -- all but a
// layer's input gradients -- keep the lean form.
template <int WM, bool CHAIN>
__global__ __launch_bounds__(256) void gemm_kernel(const GemmBatch gb) {
  constexpr int BM_ = 32 * WM;          // rows per tile
  constexpr int WN = 4 / WM;            // waves along n
  constexpr int NT = (BN / WN) / 32;    // accumulators per wave
  constexpr int PASSES = BM_ / 32;      // float4 passes of the A staging
  constexpr int TPR = 256 / BM_;        // threads per row in the scalar path
  constexpr int KSEG = BK / TPR;
  __shared__ float As[BM_ * LDA];
  __shared__ __attribute__((aligned(16))) float Bs[BK * LDB];
  __shared__ long long rowA[BM_];
  __shared__ long long rowC[BM_];
  const BlockProblem head_ = fetch_problem(gb, BM_, [](const e3k_gemm_problem& Q, int) { return (Q.N + BN - 1) / BN; });
  if (head_.local < 0) return;      // (block-uniform: surplus workgroup of a compact keyed grid)
  BlockProblem bp_ = head_;
  const e3k_gemm_problem& P = bp_.P;
  const int local = bp_.local;
  const int M = P.M1 * P.M2;
  const int tiles_n = (P.N + BN - 1) / BN;
  const int row0 = (local / tiles_n) * BM_, n0 = (local % tiles_n) * BN;
  if (row0 >= M) return;  // block-uniform: surplus workgroup of a device-sized group
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const int wm = w % WM, wn = w / WM;
  const int chain = CHAIN ? head_.P.chain : 0;

  f32x16 acc[NT];
#pragma unroll
  for (int j = 0; j < NT; ++j)
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[j][i] = 0.f;

  for (int link = 0;; ++link) {      // (one trip unless the problem heads a K-chain)
  fill_row_tables<BM_>(P, row0, M, rowA, rowC);
  __syncthreads();

  const int flags = bp_.flags;
  const bool avec = flags & 1;
  const int bmode = (flags >> 1) & 3;
  const float* ap = As + (wm * 32 + (lane & 31)) * LDA + (lane >> 5);
  const float* bp = Bs + (lane >> 5) * LDB + wn * (BN / WN) + (lane & 31);
  auto mfma_tile = [&]() {
#pragma unroll
    for (int kk = 0; kk < BK; kk += 2) {
      const float a = ap[kk];
#pragma unroll
      for (int j = 0; j < NT; ++j) acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, bp[kk * LDB + 32 * j], acc[j], 0, 0, 0);
    }
  };

  if (avec && bmode != 0) {
    const float* arow[PASSES];
#pragma unroll
    for (int pass = 0; pass < PASSES; ++pass) {
      const long long off = rowA[(t >> 3) + 32 * pass];
      arow[pass] = off >= 0 ? P.A + off : nullptr;
    }
    const int kq = (t & 7) * 4;
    float4 ra[PASSES];
    BRegs rb;
    auto gload = [&](int k0) {
#pragma unroll
      for (int pass = 0; pass < PASSES; ++pass) {
        ra[pass] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (arow[pass] && k0 + kq < P.K) ra[pass] = *reinterpret_cast<const float4*>(arow[pass] + k0 + kq);
      }
      load_b_regs(P, bmode, k0, n0, rb);
    };
    gload(0);
    for (int k0 = 0; k0 < P.K; k0 += BK) {
#pragma unroll
      for (int pass = 0; pass < PASSES; ++pass) {
        float* d = As + ((t >> 3) + 32 * pass) * LDA + kq;
        d[0] = ra[pass].x; d[1] = ra[pass].y; d[2] = ra[pass].z; d[3] = ra[pass].w;
      }
      store_b_regs(bmode, rb, Bs);
      __syncthreads();
      if (k0 + BK < P.K) gload(k0 + BK);
      mfma_tile();
      __syncthreads();
    }
  } else {
    const long long off = rowA[t / TPR];
    const float* arow = off >= 0 ? P.A + off : nullptr;
    const int kb = (t % TPR) * KSEG;
    for (int k0 = 0; k0 < P.K; k0 += BK) {
      float* d = As + (t / TPR) * LDA + kb;
#pragma unroll
      for (int j = 0; j < KSEG; ++j) {
        float v = 0.f;
        if (arow && k0 + kb + j < P.K) v = arow[(int64_t)(k0 + kb + j) * P.a_k];
        d[j] = v;
      }
      if (bmode != 0) {
        BRegs rb;
        load_b_regs(P, bmode, k0, n0, rb);
        store_b_regs(bmode, rb, Bs);
      } else {
        stage_b_scalar(P, k0, n0, Bs);
      }
      __syncthreads();
      mfma_tile();
      __syncthreads();
    }
  }
  if (!CHAIN || link == chain) break;
  {      // the next link: acc holds sum / alpha of what is behind; alpha is applied once, in the epilogue, with the LAST link's value
    const float behind = P.alpha;
    fetch_follower(gb, head_.pi + link + 1, head_, bp_);
    const float ratio = behind / P.alpha;
    if (ratio != 1.0f) {
#pragma unroll
      for (int j = 0; j < NT; ++j)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[j][i] *= ratio;
    }
  }
  }
  store_acc<NT>(P, acc, rowC, wm * 32, n0 + wn * (BN / WN));
}

// ---------------------------------------------------------------------------------------
// few rows, long K (the radial MLP's dgrad on the knot table: 4097 x 64 outputs, K ~ 2000): a 64-row tile grid would
// occupy a quarter of the chip with one serial K loop each.  Here a workgroup owns 32 x 32 outputs and its four waves
// split K; operands go global -> registers (both k-contiguous, no LDS), the four partial tiles are summed through
// LDS in wave order (deterministic).
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void gemm_splitk_kernel(const GemmBatch gb) {
  constexpr int SKC = 64;                       // k per super-chunk: 8 per lane half and MFMA group, 4 groups in flight
  __shared__ float red[4][32 * 33];
  __shared__ long long rowA[32];
  __shared__ long long rowC[32];
  const BlockProblem bp_ = fetch_problem(gb);
  const e3k_gemm_problem& P = bp_.P;
  const int M = P.M1 * P.M2, K = P.K;
  const int tiles_n = (P.N + 31) / 32;
  const int row0 = (bp_.local / tiles_n) * 32, n0 = (bp_.local % tiles_n) * 32;
  if (row0 >= M) return;
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  fill_row_tables<32>(P, row0, M, rowA, rowC);
  __syncthreads();
  const int r = lane & 31, hh = lane >> 5;
  // rows / columns beyond the problem read a valid row instead (their outputs are never stored): no guards in the loop
  const long long offa = rowA[r] >= 0 ? rowA[r] : rowA[0];
  const float* arow = P.A + offa;
  const float* brow = P.B + (int64_t)(n0 + r < P.N ? n0 + r : n0) * P.b_n;
  const int chunks = K / SKC, per = (chunks + 3) / 4;          // K % 64 == 0 (dispatch condition)
  const int c_beg = uniform(w * per), c_end = uniform((c_beg + per < chunks) ? c_beg + per : chunks);   // (scalar loop control)
  f32x16 acc;
#pragma unroll
  for (int i = 0; i < 16; ++i) acc[i] = 0.f;
  float4 a0[8], b0[8], a1[8], b1[8];
#define SPLITK_LOAD(c, xa, xb)                                                        \
  _Pragma("unroll") for (int g = 0; g < 4; ++g) _Pragma("unroll") for (int q = 0; q < 2; ++q) { \
    const int k = (c) * SKC + 16 * g + 8 * hh + 4 * q;                                \
    xa[2 * g + q] = *reinterpret_cast<const float4*>(arow + k);                       \
    xb[2 * g + q] = *reinterpret_cast<const float4*>(brow + k);                       \
  }
#define SPLITK_MFMA(xa, xb)                                                           \
  _Pragma("unroll") for (int j = 0; j < 8; ++j) {                                     \
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(xa[j].x, xb[j].x, acc, 0, 0, 0);       \
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(xa[j].y, xb[j].y, acc, 0, 0, 0);       \
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(xa[j].z, xb[j].z, acc, 0, 0, 0);       \
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(xa[j].w, xb[j].w, acc, 0, 0, 0);       \
  }
  // two chunks per trip, every load and MFMA of the trip unconditional (a conditional load makes the compiler wait for
  // ALL outstanding loads before the MFMAs of the other buffer); loads past the wave's range re-read its last chunk
  const int n_chunks = c_end - c_beg;
  if (n_chunks > 0) {
    const int last = c_end - 1;
    SPLITK_LOAD(c_beg, a0, b0)
    for (int i = 0; i + 1 < n_chunks; i += 2) {
      const int c1 = c_beg + i + 1, c2 = (c_beg + i + 2 < last) ? c_beg + i + 2 : last;
      // (the fences keep the scheduler from sinking the loads to their uses: the point is a full chunk in flight)
      SPLITK_LOAD(c1, a1, b1)
      __builtin_amdgcn_sched_barrier(0);
      SPLITK_MFMA(a0, b0)
      __builtin_amdgcn_sched_barrier(0);
      SPLITK_LOAD(c2, a0, b0)
      __builtin_amdgcn_sched_barrier(0);
      SPLITK_MFMA(a1, b1)
      __builtin_amdgcn_sched_barrier(0);
    }
    if (n_chunks & 1) { SPLITK_MFMA(a0, b0) }
  }
#undef SPLITK_LOAD
#undef SPLITK_MFMA
#pragma unroll
  for (int i = 0; i < 16; ++i) red[w][((i & 3) + 8 * (i >> 2) + 4 * hh) * 33 + r] = acc[i];
  __syncthreads();
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int o = t + 256 * j, row = o >> 5, col = o & 31;
    const long long offc = rowC[row];
    const int n = n0 + col;
    if (offc < 0 || n >= P.N) continue;
    float v = ((red[0][row * 33 + col] + red[1][row * 33 + col]) + red[2][row * 33 + col]) + red[3][row * 33 + col];
    v = fmaf(P.alpha, v, P.bias ? P.bias[n] : 0.f);
    float* c = P.C + offc + (long long)n * P.c_n;
    if (P.accumulate) v += *c;
    *c = epilogue_act(P, v);
  }
}

// (An fp32 GEMM on the bf16 matrix pipe -- every operand split into three bf16 planes, six 32x32x16 bf16 MFMAs per k-block
// instead of eight 32x32x2 f32 ones -- was built and measured in round 1: 2.7x cheaper on the matrix pipe and as accurate,
// but +12 % at best (K = N = 1024) and -12 % on the radial shapes: the split costs VALU per staged element and these GEMMs
// are not matrix-pipe-bound.  Removed in round 2)

// ---------------------------------------------------------------------------------------
// outer-mode forward:  Aeff[(r1,r2), u*V+v] = X[(r1,r2),u] * attrs[r1,v]
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void gemm_outer_kernel(const GemmBatch gb) {
  constexpr int BM_ = 128;
  __shared__ float Xs[BM_ * LDX];
  __shared__ float Vs[BM_ * LDV];
  __shared__ __attribute__((aligned(16))) float Bs[BK * LDB];
  __shared__ long long rowA[BM_];
  __shared__ long long rowC[BM_];
  const BlockProblem bp_ = fetch_problem(gb);
  const e3k_gemm_problem& P = bp_.P;
  const int flags = bp_.flags, local = bp_.local;
  const int bmode = (flags >> 1) & 3;
  const int M = P.M1 * P.M2, V = P.V, U = P.K / P.V;
  const int tiles_n = (P.N + BN - 1) / BN;
  const int row0 = (local / tiles_n) * BM_, n0 = (local % tiles_n) * BN;
  const int t = threadIdx.x, lane = t & 63, wr = t >> 6;

  f32x16 acc[2];
#pragma unroll
  for (int j = 0; j < 2; ++j)
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[j][i] = 0.f;

  fill_row_tables<BM_>(P, row0, M, rowA, rowC);
  // attrs tile: row r -> attrs[r1(r), 0..V)
  {
    const int r = t >> 1, R = row0 + r;
    const int vb = (t & 1) * 16;
    if (R < M) {
      int r1 = R / P.M2;
      if (P.row_index) r1 = P.row_index[r1];
      const float* src = P.A2 + (int64_t)r1 * P.a2_r1;
#pragma unroll
      for (int j = 0; j < 16; ++j) Vs[r * LDV + vb + j] = (vb + j < V) ? src[vb + j] : 0.f;
    } else {
#pragma unroll
      for (int j = 0; j < 16; ++j) Vs[r * LDV + vb + j] = 0.f;
    }
  }
  __syncthreads();
  const long long xoff = rowA[t >> 1];
  const float* xrow = xoff >= 0 ? P.A + xoff : nullptr;
  const float* xp = Xs + (wr * 32 + (lane & 31)) * LDX;
  const float* vp = Vs + (wr * 32 + (lane & 31)) * LDV;
  const float* bp = Bs + (lane >> 5) * LDB + (lane & 31);

  for (int u0 = 0; u0 < U; u0 += XU) {
    {
      // (the trailing barrier of the previous super-step guarantees nobody still reads Xs)
      const int ub = (t & 1) * 32;
      float* d = Xs + (t >> 1) * LDX + ub;
      if (xrow && P.a_k == 1 && u0 + ub + 32 <= U && ((reinterpret_cast<uintptr_t>(xrow + u0 + ub) & 15) == 0)) {
#pragma unroll
        for (int j = 0; j < 32; j += 4) {
          const float4 v = *reinterpret_cast<const float4*>(xrow + u0 + ub + j);
          d[j] = v.x; d[j + 1] = v.y; d[j + 2] = v.z; d[j + 3] = v.w;
        }
      } else {
#pragma unroll 8
        for (int j = 0; j < 32; ++j) {
          float v = 0.f;
          if (xrow && u0 + ub + j < U) v = xrow[(int64_t)(u0 + ub + j) * P.a_k];
          d[j] = v;
        }
      }
    }
    const int uend = (u0 + XU < U) ? u0 + XU : U;
    const int kbeg = u0 * V, kend = uend * V;
    BRegs rb;
    if (bmode != 0) load_b_regs(P, bmode, kbeg, n0, rb);
    for (int k0 = kbeg; k0 < kend; k0 += BK) {
      // rows of B beyond kend belong to the next super-step: their A operand is forced to zero below
      if (bmode != 0) store_b_regs(bmode, rb, Bs);
      else stage_b_scalar(P, k0, n0, Bs);
      __syncthreads();
      if (bmode != 0 && k0 + BK < kend) load_b_regs(P, bmode, k0 + BK, n0, rb);
      int kg = k0 + (lane >> 5);
      int u = kg / V, v = kg - u * V;
      u -= u0;
#pragma unroll 4
      for (int kk = 0; kk < BK; kk += 2) {
        float a = 0.f;
        if (kg < kend) a = xp[u] * vp[v];
        const float b0 = bp[kk * LDB], b1 = bp[kk * LDB + 32];
        acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b0, acc[0], 0, 0, 0);
        acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b1, acc[1], 0, 0, 0);
        kg += 2;
        v += 2;
        while (v >= V) {
          v -= V;
          ++u;
        }
      }
      __syncthreads();
    }
  }
  store_acc<2>(P, acc, rowC, wr * 32, n0);
}

// ---------------------------------------------------------------------------------------
// wgrad:  B[k, n] += alpha * sum_rows Aeff[row, k] * G[row, n]      (G passed in P.C)
// ---------------------------------------------------------------------------------------
constexpr int WK = 64, WR = 64;  // output tile 64 k x (64*TN) n, 64-row chunks
constexpr int LDWA = WK + 4;

// a row cursor that advances by WR rows per iteration without integer division
struct RowCursor {
  int R, r1, r2;
  __device__ __forceinline__ void init(int row, int M2) {
    R = row;
    r1 = row / M2;
    r2 = row - r1 * M2;
  }
  __device__ __forceinline__ void advance(int q, int rem, int M2) {
    R += WR;
    r1 += q;
    r2 += rem;
    if (r2 >= M2) {
      r2 -= M2;
      ++r1;
    }
  }
};

template <bool OUTER, int TN>
__device__ __forceinline__ void gemm_wgrad_body(const BlockProblem& bp_, float* As, float* Gs, float* Vs) {
  constexpr int WN = 64 * TN;
  constexpr int LDWG = WN + 4;
  const e3k_gemm_problem& P = bp_.P;
  const int flags = bp_.flags, local = bp_.local;
  const int M = P.M1 * P.M2, M2 = P.M2;
  const int tiles_k = (P.K + WK - 1) / WK, tiles_n = (P.N + WN - 1) / WN;
  const int splits = bp_.aux;
  const int tile = local % (tiles_k * tiles_n), split = local / (tiles_k * tiles_n);
  const int k0 = (tile / tiles_n) * WK, n0 = (tile % tiles_n) * WN;
  const int chunk_rows = ((M + splits - 1) / splits + WR - 1) / WR * WR;
  const int rbeg = split * chunk_rows;
  const int rend = (rbeg + chunk_rows < M) ? rbeg + chunk_rows : M;
  if (rbeg >= M) return;  // block-uniform: this split has no rows
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const int wk = wv >> 1, wn = wv & 1;  // wave = 32 k x (32*TN) n
  const int q64 = WR / M2, rem64 = WR - q64 * M2;

  f32x16 acc[TN];
#pragma unroll
  for (int j = 0; j < TN; ++j)
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[j][i] = 0.f;

  const bool gvec = flags & 8;
  const float* gp = Gs + (lane >> 5) * LDWG + wn * (32 * TN) + (lane & 31);

  if constexpr (!OUTER) {
    // (scalar staging only: a problem whose A and G are both 16-byte-loadable goes to gemm_wgrad2_kernel -- gemm_wgrad_impl)
    RowCursor cur;
    cur.init(rbeg + (t >> 2), M2);
    const int cb = (t & 3) * 16;
    const float* ap = As + (lane >> 5) * LDWA + wk * 32 + (lane & 31);
    for (int r0 = rbeg; r0 < rend; r0 += WR) {
      const bool ok = cur.R < rend;
      const int n1 = (ok && P.row_index) ? P.row_index[cur.r1] : cur.r1;
      const float* sa = P.A + (int64_t)n1 * P.a_r1 + (int64_t)cur.r2 * P.a_r2;
      const float* sg = P.C + (int64_t)n1 * P.c_r1 + (int64_t)cur.r2 * P.c_r2;
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        float va = 0.f;
        if (ok && k0 + cb + j < P.K) va = sa[(int64_t)(k0 + cb + j) * P.a_k];
        As[(t >> 2) * LDWA + cb + j] = va;
      }
#pragma unroll
      for (int j = 0; j < 16 * TN; ++j) {
        float vg = 0.f;
        const int c = (t & 3) * 16 * TN + j;
        if (ok && n0 + c < P.N) vg = sg[(int64_t)(n0 + c) * P.c_n];
        Gs[(t >> 2) * LDWG + c] = vg;
      }
      cur.advance(q64, rem64, M2);
      __syncthreads();
#pragma unroll 8
      for (int rr = 0; rr < WR; rr += 2) {
        const float a = ap[rr * LDWA];
#pragma unroll
        for (int j = 0; j < TN; ++j) acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, gp[rr * LDWG + 32 * j], acc[j], 0, 0, 0);
      }
      __syncthreads();
    }
  } else {
    // outer mode: this lane's k index -> (u, v), fixed for the whole loop
    const int V = P.V;
    const int ulo = k0 / V;
    const int klast = (k0 + WK - 1 < P.K - 1) ? k0 + WK - 1 : P.K - 1;
    const int uw = klast / V - ulo + 1;  // <= WK/2 + 1 < LDWA
    const int ki = k0 + wk * 32 + (lane & 31);
    const bool kvalid = ki < P.K;
    const int lu = kvalid ? ki / V - ulo : 0;
    const int lv = kvalid ? ki % V : 0;
    RowCursor cur;
    cur.init(rbeg + (t >> 2), M2);
    const float* ap = As + (lane >> 5) * LDWA + lu;
    const float* vp = Vs + (lane >> 5) * LDV + lv;
    for (int r0 = rbeg; r0 < rend; r0 += WR) {
      const bool ok = cur.R < rend;
      const int n1 = (ok && P.row_index) ? P.row_index[cur.r1] : cur.r1;
      const float* sx = P.A + (int64_t)n1 * P.a_r1 + (int64_t)cur.r2 * P.a_r2;
      const float* sv = P.A2 + (int64_t)n1 * P.a2_r1;
      const float* sg = P.C + (int64_t)n1 * P.c_r1 + (int64_t)cur.r2 * P.c_r2;
      for (int j = (t & 3); j < uw; j += 4) As[(t >> 2) * LDWA + j] = ok ? sx[(int64_t)(ulo + j) * P.a_k] : 0.f;
      for (int j = (t & 3); j < V; j += 4) Vs[(t >> 2) * LDV + j] = ok ? sv[j] : 0.f;
      const int cb = (t & 3) * 16 * TN;
      if (gvec) {
#pragma unroll
        for (int j = 0; j < 16 * TN; j += 4) {
          float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
          if (ok && n0 + cb + j < P.N) v = *reinterpret_cast<const float4*>(sg + n0 + cb + j);
          *reinterpret_cast<float4*>(Gs + (t >> 2) * LDWG + cb + j) = v;
        }
      } else {
#pragma unroll
        for (int j = 0; j < 16 * TN; ++j) {
          float vg = 0.f;
          if (ok && n0 + cb + j < P.N) vg = sg[(int64_t)(n0 + cb + j) * P.c_n];
          Gs[(t >> 2) * LDWG + cb + j] = vg;
        }
      }
      cur.advance(q64, rem64, M2);
      __syncthreads();
#pragma unroll 8
      for (int rr = 0; rr < WR; rr += 2) {
        const float a = kvalid ? ap[rr * LDWA] * vp[rr * LDV] : 0.f;
#pragma unroll
        for (int j = 0; j < TN; ++j) acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, gp[rr * LDWG + 32 * j], acc[j], 0, 0, 0);
      }
      __syncthreads();
    }
  }
  // ---- atomic accumulate into B
#pragma unroll
  for (int j = 0; j < TN; ++j) {
    const int n = n0 + wn * (32 * TN) + 32 * j + (lane & 31);
    if (n < P.N) {
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int k = k0 + wk * 32 + (i & 3) + 8 * (i >> 2) + 4 * (lane >> 5);
        if (k < P.K) atomicAdd(const_cast<float*>(P.B) + (int64_t)k * P.b_k + (int64_t)n * P.b_n, P.alpha * acc[j][i]);
      }
    }
  }
}

// (one kernel serving both tile widths by a per-problem flag was built and measured: 164 VGPRs and 51 KB of LDS for every
//  problem -- three workgroups per CU -- made the 64-wide problems 55 % slower; a call issues one launch per width)
template <bool OUTER, int TN>
__global__ __launch_bounds__(256) void gemm_wgrad_kernel(const GemmBatch gb) {
  __shared__ __attribute__((aligned(16))) float As[WR * LDWA];
  __shared__ __attribute__((aligned(16))) float Gs[WR * (64 * TN + 4)];
  __shared__ float Vs[OUTER ? WR * LDV : 1];
  const BlockProblem bp_ = fetch_problem(gb);
  gemm_wgrad_body<OUTER, TN>(bp_, As, Gs, Vs);
}

// (wgrad, software-pipelined form -- gemm_wgrad2_body: e3k_gemm_batch.h)
__global__ __launch_bounds__(256, 2) void gemm_wgrad2_kernel(const GemmBatch gb) {
  __shared__ __attribute__((aligned(16))) float As[W2_AS_FLOATS];
  __shared__ __attribute__((aligned(16))) float Gs[W2_GS_FLOATS];
  gemm_wgrad2_block(gb, As, Gs);
}

// ---------------------------------------------------------------------------------------
// small helpers: column sums and the self-connection backward reduction
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void colsum_kernel(const float* __restrict__ G, int64_t rows, int cols, int64_t ld,
                                                      float* __restrict__ out) {
  // block = 256 threads: 64 columns x 4 row phases; grid.x tiles columns, grid.y splits rows
  __shared__ float part[4][64];
  const int c = blockIdx.x * 64 + (threadIdx.x & 63), ph = threadIdx.x >> 6;
  float s = 0.f;
  if (c < cols)
    for (int64_t r = (int64_t)blockIdx.y * 4 + ph; r < rows; r += (int64_t)gridDim.y * 4) s += G[r * ld + c];
  part[ph][threadIdx.x & 63] = s;
  __syncthreads();
  if (ph == 0 && c < cols) atomicAdd(out + c, part[0][threadIdx.x] + part[1][threadIdx.x] + part[2][threadIdx.x] + part[3][threadIdx.x]);
}

// Forward of a Linear with ONE output column (the energy head): C[row] = alpha <A[row, :], B> (+ bias) (+ C): a wave per row, the
// lanes walk K, one butterfly.  (On the 64 x 64 tile kernel: 74 workgroups, 10.7 us for 1.2 MB.)
__global__ __launch_bounds__(256) void gemm_n1_kernel(const float* __restrict__ A, const float* __restrict__ B, int64_t M1, int M2, int K,
                                                       int64_t a_r1, int64_t a_r2, int64_t a_k, int64_t b_k, int64_t c_r1, int64_t c_r2,
                                                       float alpha, const float* __restrict__ bias, int accumulate, int act, float act_cst,
                                                       float* __restrict__ C) {
  const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= M1 * M2) return;
  const int lane = threadIdx.x & 63;
  const int64_t r1 = r / M2, r2 = r - r1 * M2;
  const float* __restrict__ a = A + r1 * a_r1 + r2 * a_r2;
  float s = 0.f;
  for (int k = lane; k < K; k += 64) s = fmaf(a[k * a_k], B[k * b_k], s);
  s = wave_sum(s);
  if (lane == 0) {
    float* c = C + r1 * c_r1 + r2 * c_r2;
    float v = fmaf(alpha, s, bias ? bias[0] : 0.f);
    if (accumulate) v += *c;
    if (act == 1) v = act_cst * (fmaxf(v, 0.f) + log1pf(expf(-fabsf(v))) - 0.6931471805599453f);
    *c = v;
  }
}

// Weight gradient of a Linear with ONE output column (the energy head's `64x0e -> 1x0e`, e3_layers/nn/pointwise.py:18): B[k] += alpha
// sum_rows A[row, k] g[row] is a weighted column sum, not a GEMM -- on the MFMA tile kernels its 4 704 x 64 rows made 74 workgroups
// wait 22 us for 1.2 MB.  Same shape as colsum_kernel: 64 columns x 4 row phases per block, grid.y splits the rows.
__global__ __launch_bounds__(256) void wgrad_n1_kernel(const float* __restrict__ A, const float* __restrict__ g, int64_t M1, int M2,
                                                        int K, int64_t a_r1, int64_t a_r2, int64_t a_k, int64_t c_r1, int64_t c_r2,
                                                        int64_t b_k, float alpha, float* __restrict__ B) {
  __shared__ float part[4][64];
  const int k = blockIdx.x * 64 + (threadIdx.x & 63), ph = threadIdx.x >> 6;
  const int64_t rows = M1 * M2;
  float s = 0.f;
  if (k < K)
    for (int64_t r = (int64_t)blockIdx.y * 4 + ph; r < rows; r += (int64_t)gridDim.y * 4) {
      const int64_t r1 = r / M2, r2 = r - r1 * M2;
      s = fmaf(A[r1 * a_r1 + r2 * a_r2 + k * a_k], g[r1 * c_r1 + r2 * c_r2], s);
    }
  part[ph][threadIdx.x & 63] = s;
  __syncthreads();
  if (ph == 0 && k < K)
    atomicAdd(B + k * b_k, alpha * (part[0][threadIdx.x] + part[1][threadIdx.x] + part[2][threadIdx.x] + part[3][threadIdx.x]));
}

// Coalesced variant for V in {4, 8, 16, 32} (V/4 lanes share one u, a lane owns four consecutive v for the whole row):
// one wave per (r1, r2) row streams the row's U*V floats as 16-byte loads, 1 KB per wave-instruction.  (The generic
// kernel below lets every lane walk its own 4*V-byte segment: 64 cache lines in flight per instruction, 0.75 TB/s.)
template <int V>
__global__ __launch_bounds__(256) void fctp_reduce_vec_kernel(const float* __restrict__ H, const float* __restrict__ X,
                                                               const float* __restrict__ A2, int M1, int M2, int U,
                                                               int64_t x_r1, int64_t x_r2, int64_t a2_r1,
                                                               float* __restrict__ dX, int dx_acc, float* __restrict__ dA2) {
  constexpr int LPU = V / 4;          // lanes per u
  constexpr int UPI = 64 / LPU;       // u values per wave-iteration
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= (int64_t)M1 * M2) return;
  const int lane = threadIdx.x & 63;
  const int r1 = (int)(row / M2), r2 = (int)(row - (int64_t)r1 * M2);
  const float4* h4 = reinterpret_cast<const float4*>(H + row * (int64_t)U * V);
  const float* x = X + (int64_t)r1 * x_r1 + (int64_t)r2 * x_r2;
  float* dx = dX + (int64_t)r1 * x_r1 + (int64_t)r2 * x_r2;
  const int v0 = (lane % LPU) * 4, usub = lane / LPU;
  const float4 av = *reinterpret_cast<const float4*>(A2 + (int64_t)r1 * a2_r1 + v0);
  float4 da = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int ub = 0; ub < U; ub += UPI) {
    const int u = ub + usub;
    const bool ok = u < U;
    const float4 hv = ok ? h4[(int64_t)(ub / UPI) * 64 + lane] : make_float4(0.f, 0.f, 0.f, 0.f);
    const float xv = ok ? x[u] : 0.f;
    float s = fmaf(av.x, hv.x, fmaf(av.y, hv.y, fmaf(av.z, hv.z, av.w * hv.w)));
#pragma unroll
    for (int off = 1; off < LPU; off <<= 1) s += __shfl_xor(s, off, 64);
    da.x = fmaf(xv, hv.x, da.x);
    da.y = fmaf(xv, hv.y, da.y);
    da.z = fmaf(xv, hv.z, da.z);
    da.w = fmaf(xv, hv.w, da.w);
    if (ok && (lane % LPU) == 0) dx[u] = dx_acc ? dx[u] + s : s;
  }
#pragma unroll
  for (int off = LPU; off < 64; off <<= 1) {
    da.x += __shfl_xor(da.x, off, 64);
    da.y += __shfl_xor(da.y, off, 64);
    da.z += __shfl_xor(da.z, off, 64);
    da.w += __shfl_xor(da.w, off, 64);
  }
  if (lane < LPU) {
    float* o = dA2 + (int64_t)r1 * a2_r1 + v0;
    atomicAdd(o + 0, da.x);
    atomicAdd(o + 1, da.y);
    atomicAdd(o + 2, da.z);
    atomicAdd(o + 3, da.w);
  }
}

// one wave per (r1, r2) row: lanes over u; H row = [U*V] (u-major, v-minor)
__global__ __launch_bounds__(256) void fctp_reduce_kernel(const float* __restrict__ H, const float* __restrict__ X,
                                                           const float* __restrict__ A2, int M1, int M2, int U, int V,
                                                           int64_t x_r1, int64_t x_r2, int64_t a2_r1,
                                                           float* __restrict__ dX, int dx_acc, float* __restrict__ dA2) {
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= (int64_t)M1 * M2) return;
  const int lane = threadIdx.x & 63;
  const int r1 = (int)(row / M2), r2 = (int)(row - (int64_t)r1 * M2);
  const float* h = H + row * (int64_t)U * V;
  const float* a = A2 + (int64_t)r1 * a2_r1;
  const float* x = X + (int64_t)r1 * x_r1 + (int64_t)r2 * x_r2;
  float* dx = dX + (int64_t)r1 * x_r1 + (int64_t)r2 * x_r2;
  float da[VMAX];
#pragma unroll
  for (int v = 0; v < VMAX; ++v) da[v] = 0.f;
  for (int u = lane; u < U; u += 64) {
    const float xv = x[u];
    float s = 0.f;
#pragma unroll
    for (int v = 0; v < VMAX; ++v) {
      if (v < V) {
        const float hv = h[(int64_t)u * V + v];
        s = fmaf(a[v], hv, s);
        da[v] = fmaf(xv, hv, da[v]);
      }
    }
    dx[u] = dx_acc ? dx[u] + s : s;
  }
#pragma unroll
  for (int v = 0; v < VMAX; ++v) {
    if (v < V) {
      const float tot = wave_sum(da[v]);
      if (lane == 0) atomicAdd(dA2 + (int64_t)r1 * a2_r1 + v, tot);
    }
  }
}

}  // namespace e3k

// ---------------------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------------------
namespace {
bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

int cu_count() {      // compute units of the current device (launches sized to the chip)
  static int n = 0;
  if (!n) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) n = 256;
  }
  return n;
}

// The launches of the calling thread's most recent GEMM-family call (e3k_gemm_last_routes): each launch site records the kernel
// as it spells it, "(e3k::gemm_kernel<2, false>)", and the batched kernels their number of problems.  Every entry point clears the
// record on entry and again when it fails.
thread_local char gemm_routes[4096];
thread_local int gemm_routes_len = 0;
void routes_clear() {
  gemm_routes_len = 0;
  gemm_routes[0] = 0;
}
void routes_add(const char* spelled, int n_problems) {
  const char* s = spelled + (sizeof("(e3k::") - 1);
  const int len = (int)strlen(s) - 1;      // (without the closing parenthesis)
  const int room = (int)sizeof(gemm_routes) - gemm_routes_len;
  const int w = n_problems > 0 ? snprintf(gemm_routes + gemm_routes_len, room, "%s%.*s[%d]", gemm_routes_len ? ";" : "", len, s, n_problems)
                               : snprintf(gemm_routes + gemm_routes_len, room, "%s%.*s", gemm_routes_len ? ";" : "", len, s);
  gemm_routes_len = w < room ? gemm_routes_len + w : (int)sizeof(gemm_routes) - 1;
}
int routes_kept(int rc) {      // an entry point's return: a call that fails leaves no record
  if (rc != E3K_OK) routes_clear();
  return rc;
}
}  // namespace
// K: the kernel in parentheses (template arguments hold commas); n: problems of a batched launch, 0 for the single-problem kernels
#define E3K_GEMM_GO(K, n, ...)          \
  do {                                  \
    routes_add(#K, n);                  \
    hipLaunchKernelGGL(K, __VA_ARGS__); \
  } while (0)
#define E3K_GEMM_BATCH(K, b, st) E3K_GEMM_GO(K, (b).gb.n, dim3((b).blocks), dim3(256), 0, st, (b).gb)
namespace {

int validate(const e3k_gemm_problem& P, bool wgrad) {
  if (P.M1 < 0 || P.M2 <= 0 || P.N <= 0 || P.K <= 0) return E3K_ERR_INVALID;
  if ((int64_t)P.M1 * P.M2 > E3K_GEMM_MAX_ROWS) return E3K_ERR_UNSUPPORTED;      // (the kernels' row arithmetic is int)
  if (P.M1 == 0) return E3K_OK;   // empty problem (a batch without edges): skipped, its pointers may be NULL
  if (!P.A || !P.B || !P.C) return E3K_ERR_INVALID;
  if (P.V < 0 || P.V > e3k::VMAX) return E3K_ERR_UNSUPPORTED;
  if (P.V > 0 && (!P.A2 || P.K % P.V != 0)) return E3K_ERR_INVALID;
  if (wgrad && (P.bias || P.act || P.chain)) return E3K_ERR_INVALID;
  if (P.act < 0 || P.act > 1) return E3K_ERR_INVALID;
  if (P.chain < 0 || P.chain >= e3k::GEMM_MAXP) return E3K_ERR_INVALID;
  return E3K_OK;
}

// followers of a K-chain (e3k.h): the head's rows, columns, output and key groups
bool follows(const e3k_gemm_problem& H, const e3k_gemm_problem& F) {
  return F.chain == 0 && F.V == 0 && H.V == 0 && !F.bias && F.M1 == H.M1 && F.M2 == H.M2 && F.N == H.N && F.C == H.C && F.c_r1 == H.c_r1 &&
         F.c_r2 == H.c_r2 && F.c_n == H.c_n && F.row_index == H.row_index && F.group_dev == H.group_dev && F.alpha != 0.f;
}

bool a_vec(const e3k_gemm_problem& P) {
  return P.V == 0 && P.a_k == 1 && P.K % 4 == 0 && P.a_r1 % 4 == 0 && (P.M2 == 1 || P.a_r2 % 4 == 0) && aligned16(P.A);
}
int b_mode(const e3k_gemm_problem& P) {
  if (P.b_n == 1 && P.N % 4 == 0 && P.b_k % 4 == 0 && aligned16(P.B)) return 1;
  if (P.b_k == 1 && P.K % 4 == 0 && P.b_n % 4 == 0 && aligned16(P.B)) return 2;
  return 0;
}

// The batched kinds launch in this order; the one-column problems (gemm_n1_kernel) before them, a K-chain's followers with their head
enum FwdKind { FWD_PLAIN = 0, FWD_OUTER, FWD_SPLITK, FWD_KINDS, FWD_N1, FWD_FOLLOWER };

struct Batcher {
  e3k::GemmBatch gb{};
  int blocks = 0;
  bool chained = false;      // the batch holds a K-chain
  void reset() {
    gb = e3k::GemmBatch{};
    blocks = 0;
    chained = false;
  }
};
constexpr int MAX_CALL = 64;   // problems per C-ABI call

// Plain problems run on 64-row tiles (gemm_kernel<2>).  Round 3 switched to 128-row tiles from three per CU; re-measured in
// round 4 (tools/ab_bench.py, 2-3 interleaved rounds): the 64-row form wins at every size met -- trailing Linear forward 56 vs
// 62 us (twice the tiles: the unequal-K problems of a launch spread more evenly over the CUs), 256 molecules 4.65 vs 4.69 ms,
// l_max 3 7.03 vs 7.16, the protein net 8.99 vs 9.09.  The 128-row form (gemm_kernel<4>) was kept for launches of more than
// 2^20 such tiles, which no layer issues, and has been removed.

// a forward call, planned: every problem's kind and the order in which the batches take them
struct FwdPlan {
  const e3k_gemm_problem* problems;
  const int* reps;
  const long long* key_stride;
  int n;
  int kind[MAX_CALL];
  int order[MAX_CALL];
};

// The batches of kind k, filled in plan order: launched, or with launch == false only sized (the plan's dry run).  Both runs go
// through this one loop, so the dry run meets every check the launching run would.
int fwd_batches(const FwdPlan& pl, int k, bool launch, hipStream_t st) {
  Batcher b;
  auto flush = [&]() {
    if (launch && b.blocks) {
      b.gb.tile_start[b.gb.n] = b.blocks;
      switch (k) {
        case FWD_PLAIN:
          if (b.chained) E3K_GEMM_BATCH((e3k::gemm_kernel<2, true>), b, st);
          else E3K_GEMM_BATCH((e3k::gemm_kernel<2, false>), b, st);
          break;
        case FWD_SPLITK: E3K_GEMM_BATCH((e3k::gemm_splitk_kernel), b, st); break;
        default: E3K_GEMM_BATCH((e3k::gemm_outer_kernel), b, st); break;
      }
    }
    b.reset();
  };
  for (int oi = 0; oi < pl.n; ++oi) {
    const int i = pl.order[oi];
    if (pl.kind[i] != k) continue;
    const e3k_gemm_problem& P = pl.problems[i];
    const int64_t M = (int64_t)P.M1 * P.M2;
    if (M == 0) continue;
    if (P.chain > 0 && b.gb.n + 1 + P.chain > e3k::GEMM_MAXP) flush();      // a chain does not straddle two launches
    const int rp = pl.reps && pl.reps[i] > 1 ? pl.reps[i] : 1;
    const int tiles_n = (P.N + e3k::BN - 1) / e3k::BN;
    int64_t blocks;
    if (k == FWD_SPLITK) blocks = ((M + 31) / 32) * ((P.N + 31) / 32);
    else if (k == FWD_PLAIN) blocks = ((M + 63) / 64) * tiles_n;
    else blocks = ((M + 127) / 128) * tiles_n;
    const bool compact = rp > 1 && P.group_dev && P.row_index && k == FWD_PLAIN;
    if (compact) {
      // (blocks = row tiles x workgroups per row tile: the key groups partition the rows, see fetch_problem)
      const int64_t row_tiles = (M + 63) / 64, per_row = blocks / row_tiles;
      blocks = (row_tiles + rp) * per_row;
    } else {
      blocks *= rp;
    }
    if (b.blocks + blocks > 0x7fffffffLL) return E3K_ERR_INVALID;
    e3k::GemmBatch& gb = b.gb;
    gb.p[gb.n] = P;
    gb.reps[gb.n] = rp;
    gb.key_stride[gb.n] = rp > 1 ? pl.key_stride[i] : 0;
    gb.flags[gb.n] = (a_vec(P) ? 1 : 0) | (b_mode(P) << 1) | (compact ? 64 : 0);
    gb.aux[gb.n] = 0;
    gb.tile_start[gb.n] = b.blocks;
    b.blocks += (int)blocks;
    ++gb.n;
    if (P.chain > 0) b.chained = true;
    for (int j = 1; j <= P.chain; ++j) {      // the followers: right behind their head, no tiles of their own
      const e3k_gemm_problem& F = pl.problems[i + j];
      gb.p[gb.n] = F;
      gb.p[gb.n].accumulate = P.accumulate;      // (the last link's descriptor runs the epilogue)
      gb.p[gb.n].bias = P.bias;
      gb.p[gb.n].act = P.act;
      gb.p[gb.n].act_cst = P.act_cst;
      gb.reps[gb.n] = rp;
      gb.key_stride[gb.n] = rp > 1 ? pl.key_stride[i + j] : 0;
      gb.flags[gb.n] = (a_vec(F) ? 1 : 0) | (b_mode(F) << 1);
      gb.aux[gb.n] = 0;
      gb.tile_start[gb.n] = b.blocks;
      ++gb.n;
    }
    if (gb.n == e3k::GEMM_MAXP) flush();
  }
  flush();
  return E3K_OK;
}
}  // namespace

// reps[i] > 1: problem i is a keyed template (row_index = the key-sorted permutation, group_dev = the pair of key 0,
// B of key t at B + t * key_stride[i]); reps == nullptr: all plain.
// Plan, then launch: every problem is validated and classified and every batch sized before the first launch, so a call that
// fails has written nothing (a retry with `accumulate` set would otherwise apply the problems that went out twice).
static int gemm_fwd_impl(const e3k_gemm_problem* problems, int n_problems, const int* reps, const long long* key_stride,
                         void* stream) {
  if (n_problems < 0 || n_problems > MAX_CALL || (n_problems && !problems)) return E3K_ERR_INVALID;
  hipStream_t st = (hipStream_t)stream;
  FwdPlan pl;
  pl.problems = problems;
  pl.reps = reps;
  pl.key_stride = key_stride;
  pl.n = n_problems;
  int* const kind = pl.kind;
  int follower_of[MAX_CALL];
  for (int i = 0; i < n_problems; ++i) follower_of[i] = -1;
  for (int i = 0; i < n_problems; ++i) {
    const e3k_gemm_problem& P = problems[i];
    const int rc = validate(P, false);
    if (rc != E3K_OK) return rc;
    if (P.chain > 0) {      // a K-chain: head and followers on the plain kernel, in one batch
      if (follower_of[i] >= 0 || i + P.chain >= n_problems) return E3K_ERR_INVALID;
      for (int j = 1; j <= P.chain; ++j) {
        if (!follows(P, problems[i + j]) || (reps && (reps[i + j] > 1) != (reps[i] > 1)) || (reps && reps[i + j] != reps[i])) return E3K_ERR_INVALID;
        const int rcf = validate(problems[i + j], false);
        if (rcf != E3K_OK) return rcf;
        follower_of[i + j] = i;
      }
    }
  }
  // (The resident-A small-K kernel of rounds 2-5 was switched off in round 6 and later removed: with the plain kernel back at five
  // waves per SIMD and the keyed grids compact, every workload measured ran faster with its K <= 64 problems on gemm_kernel<2> --
  // 256 molecules 3.88 -> 3.82 ms, l_max 3 6.39 -> 6.28, 32 molecules 1.52 -> 1.47, force training 5.40 -> 5.33, config_diffusion
  // 3.34 -> 3.29, config_diffusion_CA 8.03 -> 7.76.  Its 51 KB of LDS and 152 registers left three workgroups per CU where a launch
  // has two rounds of them.)
  for (int i = 0; i < n_problems; ++i) {
    const e3k_gemm_problem& P = problems[i];
    const int64_t M = (int64_t)P.M1 * P.M2;
    if (follower_of[i] >= 0) {
      kind[i] = FWD_FOLLOWER;
      continue;
    }
    if (P.N == 1 && P.V == 0 && P.chain == 0 && !P.row_index && !(reps && reps[i] > 1)) {      // one output column: gemm_n1_kernel
      kind[i] = FWD_N1;
      continue;
    }
    if (P.chain > 0) {
      kind[i] = FWD_PLAIN;
      continue;
    }
    if (P.V > 0) kind[i] = FWD_OUTER;
    else if (a_vec(P) && b_mode(P) == 2 && P.K >= 256 && P.K % 64 == 0 && ((M + 63) / 64) * ((P.N + e3k::BN - 1) / e3k::BN) < 128)
      kind[i] = FWD_SPLITK;
    else
      kind[i] = FWD_PLAIN;
  }
  // A split-K problem next to plain ones costs the call a launch of its own (the accumulating second round of a layer's input
  // gradients: the gate scalars' K = 256 block of the self-connection goes split-K, its sibling of the trailing Linear plain:
  // 13 + 14 us as two dependent launches in the replayed step).  When the call has plain problems anyway and the split-K one is
  // small (K <= 512), it rides in their launch as a plain problem: its 64-row tiles finish under the siblings' tiles.
  {
    bool any_plain = false;
    for (int i = 0; i < n_problems; ++i) any_plain = any_plain || kind[i] == FWD_PLAIN;
    if (any_plain)
      for (int i = 0; i < n_problems; ++i)
        if (kind[i] == FWD_SPLITK && problems[i].K <= 512) kind[i] = FWD_PLAIN;
  }
  // ... and the other way round: a PLAIN problem of a few tiles with a long-ish K loop (the radial stack's last-layer input gradient of
  // layer 0: 9 tiles, K = 192, beside its siblings' K = 960 .. 1 920 which go split-K) waits 10 us in a launch of its own for nine
  // serial K loops.  When the call has split-K problems anyway, it joins them.
  {
    bool any_splitk = false;
    for (int i = 0; i < n_problems; ++i) any_splitk = any_splitk || kind[i] == FWD_SPLITK;
    if (any_splitk)
      for (int i = 0; i < n_problems; ++i) {
        const e3k_gemm_problem& P = problems[i];
        const int64_t M = (int64_t)P.M1 * P.M2;
        if (kind[i] == FWD_PLAIN && P.chain == 0 && !(reps && reps[i] > 1) && a_vec(P) && b_mode(P) == 2 && P.K >= 128 && P.K % 64 == 0 &&
            ((M + 63) / 64) * ((P.N + e3k::BN - 1) / e3k::BN) < 32)
          kind[i] = FWD_SPLITK;
      }
  }
  // longest-processing-time-first: workgroups are dispatched in blockIdx order, so the problems with the longest
  // K loops go first and the short ones fill the tail of the launch
  for (int i = 0; i < n_problems; ++i) pl.order[i] = i;
  auto k_total = [&](int a) {
    int kt = problems[a].K;
    for (int j = 1; j <= problems[a].chain; ++j) kt += problems[a + j].K;
    return kt;
  };
  std::stable_sort(pl.order, pl.order + n_problems, [&](int a, int b) { return k_total(a) > k_total(b); });
  for (int k = 0; k < FWD_KINDS; ++k) {      // the dry run: every batch sized as it will launch
    const int rc = fwd_batches(pl, k, false, st);
    if (rc != E3K_OK) return rc;
  }

  // launch: the one-column problems in problem order, then the batches kind by kind
  for (int i = 0; i < n_problems; ++i) {
    const e3k_gemm_problem& P = problems[i];
    const int64_t M = (int64_t)P.M1 * P.M2;
    if (kind[i] == FWD_N1 && M > 0)
      E3K_GEMM_GO((e3k::gemm_n1_kernel), 0, dim3((unsigned)((M + 3) / 4)), dim3(256), 0, st, P.A, P.B, (int64_t)P.M1, P.M2, P.K, P.a_r1, P.a_r2,
                         P.a_k, P.b_k, P.c_r1, P.c_r2, P.alpha, P.bias, P.accumulate, P.act, P.act_cst, P.C);
  }
  for (int k = 0; k < FWD_KINDS; ++k) (void)fwd_batches(pl, k, true, st);      // (passed the dry run: cannot fail)
  E3K_CHECK_LAUNCH();
  return E3K_OK;
}

extern "C" int e3k_gemm(const e3k_gemm_problem* problems, int n_problems, void* stream) {
  routes_clear();
  return routes_kept(gemm_fwd_impl(problems, n_problems, nullptr, nullptr, stream));
}

static int gemm_wgrad_impl(const e3k_gemm_problem* problems, int n_problems, const int* reps, const long long* key_stride,
                           void* stream, e3k::WgradHook* hook = nullptr) {
  if (n_problems < 0 || n_problems > MAX_CALL || (n_problems && !problems)) return E3K_ERR_INVALID;
  hipStream_t st = (hipStream_t)stream;
  for (int i = 0; i < n_problems; ++i) {
    const int rc = validate(problems[i], true);
    if (rc != E3K_OK) return rc;
  }
  bool taken[MAX_CALL] = {};
  // one output column, plain rows: a weighted column sum (wgrad_n1_kernel)
  for (int i = 0; i < n_problems; ++i) {
    const e3k_gemm_problem& P = problems[i];
    if (P.N != 1 || P.V != 0 || P.row_index || (reps && reps[i] > 1) || (int64_t)P.M1 * P.M2 <= 0) continue;
    const int64_t rows = (int64_t)P.M1 * P.M2;
    int gy = (int)((rows + 31) / 32);
    if (gy > 1024) gy = 1024;
    E3K_GEMM_GO((e3k::wgrad_n1_kernel), 0, dim3((P.K + 63) / 64, gy), dim3(256), 0, st, P.A, P.C, (int64_t)P.M1, P.M2, P.K, P.a_r1,
                       P.a_r2, P.a_k, P.c_r1, P.c_r2, P.b_k, P.alpha, const_cast<float*>(P.B));
    taken[i] = true;
  }
  auto g_vec = [](const e3k_gemm_problem& P) {
    return P.c_n == 1 && P.N % 4 == 0 && P.c_r1 % 4 == 0 && (P.M2 == 1 || P.c_r2 % 4 == 0) && aligned16(P.C);
  };
  auto tiles_of = [](const e3k_gemm_problem& P) { return ((P.K + (P.K > 64 ? 127 : 63)) / (P.K > 64 ? 128 : 64)) * ((P.N + 63) / 64); };
  const int n_cu = cu_count();
  // Problems with 16-byte-loadable operands (plain and keyed; not the outer-product form): the pipelined kernel, ONE launch
  // sized to one round of workgroups (three per CU), every workgroup the same number of rows -- splits proportional to a
  // problem's rows, at least kMinChunks chunks of W2R rows each.  A keyed problem's key groups partition its M1 rows: it counts
  // once, every key gets the splits of the whole, and the workgroups past a key's last row exit.
  {
    constexpr int kMinChunks = 2;
    const double target = 3.0 * n_cu;
    const double target_hooked = hook ? hook->wg_per_cu * n_cu : target;      // the FIRST batch's, when it goes out through the hook
    int n_sized = 0;
    auto eligible = [&](int i) {
      const e3k_gemm_problem& P = problems[i];
      return P.V == 0 && (int64_t)P.M1 * P.M2 > 0 && a_vec(P) && g_vec(P);
    };
    double total = 0;      // rows x tiles over the problems of this launch
    for (int i = 0; i < n_problems; ++i)
      if (eligible(i)) total += (double)problems[i].M1 * problems[i].M2 * tiles_of(problems[i]);
    Batcher b;
    auto flush = [&]() {
      if (b.blocks) {
        b.gb.tile_start[b.gb.n] = b.blocks;
        if (hook && !hook->used) {      // (e3k_wgrad_rider.hip: this batch and the knot-table transpose in one launch)
          routes_add("(e3k::gemm_wgrad2_with_table_bwd_kernel)", b.gb.n);
          hook->launch(b.gb, b.blocks, st, hook->ctx);
          hook->used = true;
        } else {
          E3K_GEMM_BATCH((e3k::gemm_wgrad2_kernel), b, st);
        }
      }
      b.reset();
    };
    for (int i = 0; i < n_problems && total > 0; ++i) {
      if (!eligible(i)) continue;
      const e3k_gemm_problem& P = problems[i];
      const int64_t M = (int64_t)P.M1 * P.M2;
      const int rp = reps && reps[i] > 1 ? reps[i] : 1;
      taken[i] = true;
      const double tgt = n_sized++ < e3k::GEMM_MAXP ? target_hooked : target;
      int64_t splits = (int64_t)(tgt * (double)M / total);      // rounded down: the launch stays within one round
      const int64_t max_splits = (M + kMinChunks * e3k::W2R - 1) / (kMinChunks * e3k::W2R);
      if (splits > max_splits) splits = max_splits;
      if (splits < 1) splits = 1;
      e3k::GemmBatch& gb = b.gb;
      gb.p[gb.n] = P;
      gb.reps[gb.n] = rp;
      gb.key_stride[gb.n] = rp > 1 ? key_stride[i] : 0;
      gb.flags[gb.n] = 9;
      gb.aux[gb.n] = (int)splits;
      gb.tile_start[gb.n] = b.blocks;
      if (rp > 1 && P.group_dev && P.row_index) {
        // the key groups partition the M rows: `splits` splits of the whole (+ one per key for the remainders) instead of `splits` per key
        const int64_t rows = ((M + splits - 1) / splits + e3k::W2R - 1) / e3k::W2R * e3k::W2R;
        gb.flags[gb.n] |= 64;
        gb.aux[gb.n] = (int)rows;
        b.blocks += tiles_of(P) * (int)((M + rows - 1) / rows + rp);
      } else {
        b.blocks += tiles_of(P) * (int)splits * rp;
      }
      if (++gb.n == e3k::GEMM_MAXP) flush();
    }
    flush();
  }
  // the rest (outer-product form, operands that are not 16-byte-loadable) on gemm_wgrad_kernel: about kTarget workgroups per problem,
  // kChunks chunks of WR rows per workgroup
  constexpr int64_t kTarget = 1024;
  constexpr int kChunks = 4;
  for (int mode = 0; mode < 4; ++mode) {  // (outer: x (x) attrs formed on the fly?, 128-wide output tile?)
    const bool outer = mode & 1;
    const int tn = (mode & 2) ? 2 : 1;
    Batcher b;
    auto flush = [&]() {
      if (b.blocks) {
        b.gb.tile_start[b.gb.n] = b.blocks;
        if (!outer && tn == 2) E3K_GEMM_BATCH((e3k::gemm_wgrad_kernel<false, 2>), b, st);
        else if (!outer) E3K_GEMM_BATCH((e3k::gemm_wgrad_kernel<false, 1>), b, st);
        else if (tn == 2) E3K_GEMM_BATCH((e3k::gemm_wgrad_kernel<true, 2>), b, st);
        else E3K_GEMM_BATCH((e3k::gemm_wgrad_kernel<true, 1>), b, st);
      }
      b.reset();
    };
    for (int i = 0; i < n_problems; ++i) {
      const e3k_gemm_problem& P = problems[i];
      if (taken[i]) continue;
      if ((P.V > 0) != outer) continue;
      if ((P.N >= 128 ? 2 : 1) != tn) continue;
      const int64_t M = (int64_t)P.M1 * P.M2;
      if (M == 0) continue;
      const int rp = reps && reps[i] > 1 ? reps[i] : 1;
      const int f = g_vec(P) ? 8 : 0;      // (A by scalar loads here: a problem with both operands 16-byte-loadable took gemm_wgrad2_kernel)
      const int wn = 64 * tn;
      const int tiles = ((P.K + e3k::WK - 1) / e3k::WK) * ((P.N + wn - 1) / wn);
      int64_t splits = (kTarget + tiles - 1) / tiles;
      // rows per workgroup: kChunks chunks of WR rows -- unless that leaves most of the chip idle (round 6: the one-hot embeddings'
      // and the energy head's weight gradients are ONE tile over 4 600 rows: 18 workgroups walking four chunks each took 17-22 us
      // apiece in the replayed step; a chunk per workgroup, 73 workgroups, is one load latency long)
      int chunks = kChunks;
      while (chunks > 1 && tiles * ((M + (int64_t)chunks * e3k::WR - 1) / ((int64_t)chunks * e3k::WR)) < n_cu) chunks >>= 1;
      const int64_t max_splits = (M + chunks * e3k::WR - 1) / (chunks * e3k::WR);
      if (splits > max_splits) splits = max_splits;
      if (splits < 1) splits = 1;
      e3k::GemmBatch& gb = b.gb;
      gb.p[gb.n] = P;
      gb.reps[gb.n] = rp;
      gb.key_stride[gb.n] = rp > 1 ? key_stride[i] : 0;
      gb.flags[gb.n] = f;
      gb.aux[gb.n] = (int)splits;
      gb.tile_start[gb.n] = b.blocks;
      b.blocks += tiles * (int)splits * rp;
      if (++gb.n == e3k::GEMM_MAXP) flush();
    }
    flush();
  }
  E3K_CHECK_LAUNCH();
  return E3K_OK;
}

extern "C" int e3k_gemm_wgrad(const e3k_gemm_problem* problems, int n_problems, void* stream) {
  routes_clear();
  return routes_kept(gemm_wgrad_impl(problems, n_problems, nullptr, nullptr, stream));
}

namespace {
// resolves one segment's templates into `out` (pointer fields of a template hold byte offsets; A2 / bias offset + 1)
int resolve_segment(const e3k_gemm_segment& sg, e3k_gemm_problem* out, int* reps, long long* key_stride, int cap) {
  if (sg.n_templates < 0 || sg.n_templates > cap || (sg.n_templates && !sg.templates)) return -1;
  if (sg.M1 > 0x7fffffffLL) return -1;
  const bool keyed = sg.n_keys > 0;
  if (keyed && (!sg.perm || !sg.groups_dev)) return -1;
  const auto off = [](const void* q) { return reinterpret_cast<uintptr_t>(q); };
  for (int i = 0; i < sg.n_templates; ++i) {
    e3k_gemm_problem p = sg.templates[i];
    p.A = reinterpret_cast<const float*>(off(sg.a_base) + off(p.A));
    p.B = reinterpret_cast<const float*>(off(sg.b_base) + off(p.B));
    p.C = reinterpret_cast<float*>(off(sg.c_base) + off(p.C));
    if (sg.M1 >= 0) {   // rebased templates (M1 < 0: the templates carry addresses and their own row counts)
      if (p.A2) {
        if (!sg.a2_base) return -1;
        p.A2 = reinterpret_cast<const float*>(off(sg.a2_base) + off(p.A2) - 1);
      }
      if (p.bias) {
        if (!sg.bias_base) return -1;
        p.bias = reinterpret_cast<const float*>(off(sg.bias_base) + off(p.bias) - 1);
      }
      p.M1 = (int32_t)sg.M1;
    }
    if (keyed) {
      p.row_index = sg.perm;
      p.group_dev = sg.groups_dev;
    }
    out[i] = p;
    reps[i] = keyed ? sg.n_keys : 1;
    key_stride[i] = keyed ? sg.b_key_stride : 0;
  }
  return sg.n_templates;
}
}  // namespace

static int gemm_multi_impl(const e3k_gemm_segment* segments, int32_t n_segments, int32_t wgrad, void* stream,
                           e3k::WgradHook* hook = nullptr) {
  if (n_segments < 0 || (n_segments && !segments)) return E3K_ERR_INVALID;
  e3k_gemm_problem buf[MAX_CALL];
  int reps[MAX_CALL];
  long long ks[MAX_CALL];
  int n = 0;
  for (int s = 0; s < n_segments; ++s) {
    const int got = resolve_segment(segments[s], buf + n, reps + n, ks + n, MAX_CALL - n);
    if (got < 0) return E3K_ERR_INVALID;
    n += got;
  }
  return wgrad ? gemm_wgrad_impl(buf, n, reps, ks, stream, hook) : gemm_fwd_impl(buf, n, reps, ks, stream);
}

extern "C" int e3k_gemm_multi(const e3k_gemm_segment* segments, int32_t n_segments, int32_t wgrad, void* stream) {
  routes_clear();
  return routes_kept(gemm_multi_impl(segments, n_segments, wgrad, stream));
}

void e3k::gemm_routes_clear() { routes_clear(); }

int e3k::gemm_multi_wgrad_hooked(const e3k_gemm_segment* segments, int32_t n_segments, void* stream, WgradHook* hook) {
  routes_clear();
  return routes_kept(gemm_multi_impl(segments, n_segments, 1, stream, hook));
}

extern "C" int e3k_gemm_rebased(const e3k_gemm_problem* templates, int n_templates, const void* a_base,
                                const void* a2_base, const void* b_base, void* c_base, const void* bias_base,
                                int64_t M1, int32_t wgrad, void* stream) {
  routes_clear();
  if (M1 < 0) return E3K_ERR_INVALID;
  e3k_gemm_segment sg{};
  sg.templates = templates; sg.n_templates = n_templates;
  sg.a_base = a_base; sg.a2_base = a2_base; sg.b_base = b_base; sg.c_base = c_base; sg.bias_base = bias_base;
  sg.M1 = M1;
  return e3k_gemm_multi(&sg, 1, wgrad, stream);
}

extern "C" int e3k_gemm_grouped(const e3k_gemm_problem* templates, int n_templates, const int32_t* perm,
                                const int32_t* groups_dev, int32_t n_keys, int64_t b_key_stride, int32_t wgrad,
                                void* stream) {
  routes_clear();
  if (n_keys <= 0) return E3K_ERR_INVALID;
  e3k_gemm_segment sg{};
  sg.templates = templates; sg.n_templates = n_templates;
  sg.M1 = -1;
  sg.perm = perm; sg.groups_dev = groups_dev; sg.n_keys = n_keys; sg.b_key_stride = b_key_stride;
  return e3k_gemm_multi(&sg, 1, wgrad, stream);
}

extern "C" int e3k_gemm_grouped_rebased(const e3k_gemm_problem* templates, int n_templates, const void* a_base,
                                        const void* b_base, void* c_base, int64_t M1, const int32_t* perm,
                                        const int32_t* groups_dev, int32_t n_keys, int64_t b_key_stride, int32_t wgrad,
                                        void* stream) {
  routes_clear();
  if (M1 < 0 || n_keys <= 0) return E3K_ERR_INVALID;
  e3k_gemm_segment sg{};
  sg.templates = templates; sg.n_templates = n_templates;
  sg.a_base = a_base; sg.b_base = b_base; sg.c_base = c_base;
  sg.M1 = M1;
  sg.perm = perm; sg.groups_dev = groups_dev; sg.n_keys = n_keys; sg.b_key_stride = b_key_stride;
  return e3k_gemm_multi(&sg, 1, wgrad, stream);
}

extern "C" int e3k_colsum(const float* G, int64_t rows, int32_t cols, int64_t ld, float* out, void* stream) {
  routes_clear();
  if (rows < 0 || cols <= 0 || !out) return E3K_ERR_INVALID;
  if (rows == 0) return E3K_OK;
  if (!G) return E3K_ERR_INVALID;
  // (a thread's walk down its rows is a chain of load latencies: 64 rows per thread took 15 us for a 1 MB matrix -- 8 rows, 3 us)
  int gy = (int)((rows + 31) / 32);
  if (gy > 1024) gy = 1024;
  E3K_GEMM_GO((e3k::colsum_kernel), 0, dim3((cols + 63) / 64, gy), dim3(256), 0, (hipStream_t)stream, G, rows, cols, ld, out);
  return routes_kept(hipGetLastError() == hipSuccess ? E3K_OK : E3K_ERR_LAUNCH);
}

extern "C" int e3k_fctp_reduce_bwd(const float* H, const float* X, const float* A2, int32_t M1, int32_t M2, int32_t U,
                                   int32_t V, int64_t x_r1, int64_t x_r2, int64_t a2_r1, float* dX,
                                   int32_t dx_accumulate, float* dA2, void* stream) {
  routes_clear();
  if (M1 < 0 || M2 <= 0 || U <= 0 || V <= 0 || V > e3k::VMAX) return E3K_ERR_INVALID;
  if (M1 == 0) return E3K_OK;
  if (!H || !X || !A2 || !dX || !dA2) return E3K_ERR_INVALID;
  const int64_t rows = (int64_t)M1 * M2;
  const dim3 grid((unsigned)((rows + 3) / 4));
  hipStream_t st = (hipStream_t)stream;
  // 16-byte streams need: H rows (U*V floats) and the A2 rows 16-byte aligned
  const bool vec = aligned16(H) && aligned16(A2) && a2_r1 % 4 == 0 && ((int64_t)U * V) % 4 == 0 && 64 % (V / 4 > 0 ? V / 4 : 1) == 0;
#define E3K_FCTP_VEC(VV)                                                                                                   \
  E3K_GEMM_GO((e3k::fctp_reduce_vec_kernel<VV>), 0, grid, dim3(256), 0, st, H, X, A2, M1, M2, U, x_r1, x_r2, a2_r1, dX, \
              dx_accumulate, dA2)
  if (vec && V == 32) E3K_FCTP_VEC(32);
  else if (vec && V == 16) E3K_FCTP_VEC(16);
  else if (vec && V == 8) E3K_FCTP_VEC(8);
  else if (vec && V == 4) E3K_FCTP_VEC(4);
  else
    E3K_GEMM_GO((e3k::fctp_reduce_kernel), 0, grid, dim3(256), 0, st, H, X, A2, M1, M2, U, V, x_r1, x_r2, a2_r1, dX, dx_accumulate, dA2);
#undef E3K_FCTP_VEC
  return routes_kept(hipGetLastError() == hipSuccess ? E3K_OK : E3K_ERR_LAUNCH);
}

extern "C" const char* e3k_gemm_last_routes(void) { return gemm_routes; }
