// Pieces of the tensor-product kernels (e3k_tp.hip, e3k_tp_scalar.hip): compile-time loops over the (l2, l3) slots of an input
// degree, the spherical-harmonics registers, buffer addressing, the packed table's records, the work-order prologue, the plan object.
#pragma once
#include <type_traits>

#include "e3k_common.h"
#include "e3k_cg_gen.h"

static_assert(E3K_MAXQ == E3K_TP_MAXQ, "e3k.h and e3k_cg_gen.h disagree on the slot count");
static_assert(E3K_L2MAX == 2, "YRegs below is written for sh degrees 0..2");

// the per-edge weights are read once per pass and the weight gradients written once: streamed past the caches
// (the cache lines stay for the gathered node rows)
#ifdef E3K_NO_NT
#define E3K_STREAM_LOAD(p) (*(p))
#define E3K_STREAM_STORE(v, p) (*(p) = (v))
#define E3K_STREAM_AUX 0
#else
#define E3K_STREAM_AUX 2   // buffer-load cache policy bit 1 = nt
#define E3K_STREAM_LOAD(p) __builtin_nontemporal_load(p)
#define E3K_STREAM_STORE(v, p) __builtin_nontemporal_store((v), (p))
#endif

namespace e3k {

template <int I, int N, class F>
__device__ __forceinline__ void static_for(F&& f) {
  if constexpr (I < N) {
    f(std::integral_constant<int, I>{});
    static_for<I + 1, N>(f);
  }
}

struct YRegs {
  float y0[1];
  float y1[3];
  float y2[5];
};
template <int L2>
__device__ __forceinline__ auto& yref(YRegs& y) {
  if constexpr (L2 == 0) return y.y0;
  else if constexpr (L2 == 1) return y.y1;
  else return y.y2;
}

struct TpArgs {
  const float* x;      // [N, d_in]  cf
  const float* sh;     // [E, d_sh]
  const float* w;      // [E, W]
  const float* g_out;  // [N, d_mid] cf (backward)
  float* out;          // [N, d_mid] cf (forward)
  float* g_w;          // [E, W]
  float* g_w2;         // [E, W], optional second weight-gradient output (tp_bwd_x MODE 7: the plain one beside the dual one)
  float* g_sh;         // [E, d_sh]
  float* g_x;          // [N, d_in]
  const int32_t* nbr;  // src[e] (fwd, bwd_w) or dst[e] (bwd_x)
  const int32_t* ptr;  // CSR row pointers [N+1]
  const int32_t* perm; // CSR edge ids [E]
  const int32_t* bin;  // TABLE kernels: knot i of every edge [E] (stencil rows i-1 .. i+2); w is then the knot table [K + 1, W]
  const float* coef;   // TABLE kernels: the four interpolation weights of every edge [E, 4] (e3k_rtable_bins)
  // force training on the table: the slope table D [K + 1, W] (d T / d r on the knots, interpolated with the SAME weights:
  // dw/dr[e] = sum_k coef[e, k] D[bin[e] - 1 + k]) and the second operand set of the JVP / DUAL forms (the double backward:
  // the product rule over (x, sh, r))
  const float* w2;     // D
  const float* x2;     // [N, d_in] cf
  const float* sh2;    // [E, d_sh]
  const float* s2;     // [E]: the radius' partner (a cotangent): the third term's weights are s2[e] * dw/dr[e]
  float* g_r;          // [E]: gradient w.r.t. the radius (tp_bwd_e), accumulated with one atomic per wave and edge
  const int32_t* erec; // FULL kernels, optional: the walk's edge records [E, 16] (e3k_edge_records) -- perm, nbr, bin, coef, sh are then unused
  int32_t d_in, d_sh, W, d_mid;
  int32_t x_shared;    // bwd_x: some input block is read by more than one group => accumulate g_x with atomics
  int32_t _pad;        // (holds order and e_store at their offsets: next to x_shared, order is fetched with it in one load and the
                       //  compiler schedules the tensor-product kernels differently)
  int32_t order;       // work order of the launch (E3K_TP_PROLOGUE): 0 node-major, 1 group-major inside an XCD's node slice
  int32_t e_store;     // edge gradients (g_sh, g_r): 0 = float atomics into [E, .]; 1 = every work item STORES its share into its own
                       // slice of [n_gc, E, .] (g_sh / g_r point at the slices' base, e_edges = E): summed in a fixed order afterwards
  int64_t e_edges;
  int64_t n_items;
};

struct GroupRegs {
  int x_off, mul;
  unsigned mask;
  int y_off[3];
};

__device__ __forceinline__ void load_y(YRegs& y, const float* __restrict__ yr, const e3k_tp_group& g) {
  // wave-uniform addresses: these become scalar loads
  if (g.y_off[0] >= 0) y.y0[0] = yr[g.y_off[0]];
  if (g.y_off[1] >= 0) {
#pragma unroll
    for (int j = 0; j < 3; ++j) y.y1[j] = yr[g.y_off[1] + j];
  }
  if (g.y_off[2] >= 0) {
#pragma unroll
    for (int j = 0; j < 5; ++j) y.y2[j] = yr[g.y_off[2] + j];
  }
}

// ------------------------------------------------------------------------------------------
// forward
// ------------------------------------------------------------------------------------------
// visits the path slots whose output degree the plan can contain: slots with l3 > L3MAX are compiled out, so an
// l_max = 2 model carries no accumulators for l3 = 3 outputs (14 of the 36 registers of an l1 = 2 group)
// PART splits a group's slots between two waves (0: slots below the split point, 1: the rest, 2: all of them): at
// l_max = 3 a group carries 27-36 accumulators; halving them takes the kernels from 3-4 to 6-7 waves per SIMD at the
// price of gathering x[src] twice (an L2 hit).  Split points: l1 = 1 -> slot 4, l1 = 2 -> slot 4, l1 = 3 -> slot 3.
template <int L1> struct SplitAt { static constexpr int Q = L1 == 3 ? 3 : 4; };
template <class S, int L1, int L3MAX, int PART, class F>
__device__ __forceinline__ void slot_for_part(F&& f) {
  static_for<0, S::NQ>([&](auto qc) {
    constexpr int Q = decltype(qc)::value;
    constexpr bool in_part = PART == 2 || (PART == 0 ? Q < SplitAt<L1>::Q : Q >= SplitAt<L1>::Q);
    if constexpr (S::L3[Q] <= L3MAX && in_part) f(qc);
  });
}

// ---- shared by the packed-table walks of e3k_tp.hip and e3k_tp_scalar.hip ------------------------------------------------------
__device__ __forceinline__ __amdgpu_buffer_rsrc_t row_rsrc(const float* base, int bytes) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(base), 0, bytes, 0x00020000);
}
__device__ __forceinline__ float buf_ld(__amdgpu_buffer_rsrc_t r, int voff, int soff) {
  return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r, voff, soff, 0));
}
__device__ __forceinline__ float buf_ld_stream(__amdgpu_buffer_rsrc_t r, int voff, int soff) {
  return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r, voff, soff, E3K_STREAM_AUX));
}
__device__ __forceinline__ void buf_st_stream(float v, __amdgpu_buffer_rsrc_t r, int voff, int soff) {
  __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v), r, voff, soff, E3K_STREAM_AUX);
}

// The packed table (round 5): the same cubic from 12 bytes per (knot, weight) in ONE table row -- {d0, d1: f32; d2 * 2^10,
// d3 * 2^16: f16}, the Taylor coefficients about the middle of the knot interval (e3k_rtable_pack; a row = its W (d0, d1) pairs, then
// its W f16 pairs) -- one dwordx2 + one dword load per slot instead of four dword loads out of four rows: 23 instead of 31 KB of
// table per edge through L1, half the table's VMEM instructions.  a.w is then the packed table [K + 1, 3 W] (dwords).
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
struct PackedRec {
  float d0, d1;
  unsigned int pk;
};
struct KnotPacked {
  __amdgpu_buffer_rsrc_t r;
  float s, s2, s3;
};
// the t-th edge of the walk as one aligned 64-byte record (e3k_edge_records): a single s_load_dwordx16 whose address follows from
// the loop counter -- the packed-table kernels fetch edge t + 1's record while edge t is computed
struct EdgeRec {
  int nbr, bin;
  float c0, c1, c2, c3;
  float y[9];
  int e;
};
// The record is read through a constant-address-space pointer: a kernel that stores through other members of its TpArgs (g_x, g_w:
// every backward walk) otherwise gets the record by vector loads of one lane-uniform address, a v_readfirstlane per dword and a wait
// for the "prefetched" record in front of the edge's row loads, because nothing tells the compiler that its stores leave the records
// alone.  This rests on ONE condition: the record buffer is written by EARLIER launches only (e3k_edge_records, in the preparation
// that precedes the walks on the same stream or graph), never by the kernel that reads it -- the scalar cache is not coherent with
// a kernel's own vector stores.  The forward walk's record loads, scalar by themselves, have always rested on the same condition.
typedef const __attribute__((address_space(4))) int32_t* const_words;
__device__ __forceinline__ const_words as_constant(const int32_t* p) { return (const_words)p; }
// the row range [ptr[node], ptr[node + 1]) of a backward walk, the same way and on the same condition (e3k_csr_build precedes the walks)
__device__ __forceinline__ int2 row_range(const int32_t* ptr, int node) {
  const const_words p = as_constant(ptr + node);
  return make_int2(p[0], p[1]);
}
__device__ __forceinline__ EdgeRec load_rec(const int32_t* __restrict__ erec, int t) {
  const const_words p = as_constant(static_cast<const int32_t*>(__builtin_assume_aligned(erec + 16 * (int64_t)t, 64)));
  EdgeRec r;
  r.nbr = uniform(p[0]);
  r.bin = uniform(p[1]);
  r.c0 = __int_as_float(uniform(p[2])); r.c1 = __int_as_float(uniform(p[3]));
  r.c2 = __int_as_float(uniform(p[4])); r.c3 = __int_as_float(uniform(p[5]));
#pragma unroll
  for (int j = 0; j < 9; ++j) r.y[j] = __int_as_float(uniform(p[6 + j]));
  r.e = uniform(p[15]);
  return r;
}
__device__ __forceinline__ void rec_y(YRegs& y, const EdgeRec& r) {
  y.y0[0] = r.y[0];
#pragma unroll
  for (int j = 0; j < 3; ++j) y.y1[j] = r.y[1 + j];
#pragma unroll
  for (int j = 0; j < 5; ++j) y.y2[j] = r.y[4 + j];
}
__device__ __forceinline__ KnotPacked knot_packed_rec(const TpArgs& a, const EdgeRec& r, int row_p) {
  KnotPacked k;
  k.r = row_rsrc(a.w + 3 * (int64_t)r.bin * a.W, row_p);
  k.s = fmaf(2.f, r.c3, r.c2 - r.c0) - 0.5f;      // t = sum_k x_k L_k(t), x = (-1, 0, 1, 2); s = t - 1/2
  k.s2 = k.s * (1.f / 1024.f);
  k.s3 = k.s * (1.f / 64.f);
  return k;
}
// slot at weight offset woff4 (bytes of a 4-byte column) of the row, lane channel u4 = 4 u; pk_base = 8 W (bytes)
__device__ __forceinline__ PackedRec buf_ld_rec(__amdgpu_buffer_rsrc_t r, int u4, int woff4, int pk_base) {
  const auto v = __builtin_amdgcn_raw_buffer_load_b64(r, u4 * 2, woff4 * 2, 0);
  PackedRec p;
  p.d0 = __uint_as_float(v[0]);
  p.d1 = __uint_as_float(v[1]);
  p.pk = __builtin_amdgcn_raw_buffer_load_b32(r, u4, pk_base + woff4, 0);
  return p;
}
__device__ __forceinline__ float packed_mix(const KnotPacked& k, const PackedRec& v) {      // the order of e3k::packed_eval (e3k_rtable.hip)
  const f16x2 h = __builtin_bit_cast(f16x2, v.pk);
  return fmaf(k.s, fmaf(k.s2, fmaf(k.s3, (float)h.y, (float)h.x), v.d1), v.d0);
}

}  // namespace e3k

// Work order.  0: node-major -- XCD x owns a contiguous slice of the (node, group-chunk) list, a workgroup = four consecutive items
// (mostly the groups of ONE node).  1 (table forms): group-major inside the XCD's node slice -- XCD x owns nodes [x N / 8, (x + 1) N / 8)
// and walks them group-chunk by group-chunk, a workgroup = four consecutive NODES of one group-chunk: at any time an XCD's L2 then
// holds the table columns of ONE group (2.4 of the packed table's 11.8 MB) beside that group's feature columns of its own nodes.
#define E3K_TP_PROLOGUE                                                        \
  int node_, gci_;                                                             \
  if (a.order == 0) {                                                          \
    const int b = xcd_remap(blockIdx.x, gridDim.x);                            \
    const int64_t item = (int64_t)b * 4 + (threadIdx.x >> 6);                  \
    if (item >= a.n_items) return;                                             \
    node_ = (int)(item / n_gc);                                                \
    gci_ = (int)(item % n_gc);                                                 \
  } else {                                                                     \
    const int64_t n_nodes = a.n_items / n_gc;                                  \
    const int xcd = blockIdx.x & 7;                                            \
    const int64_t n0 = xcd * n_nodes / 8, nx = (xcd + 1) * n_nodes / 8 - n0;   \
    const int64_t j = (int64_t)(blockIdx.x >> 3) * 4 + (threadIdx.x >> 6);     \
    if (j >= nx * n_gc) return;                                                \
    gci_ = (int)(j / nx);                                                      \
    node_ = (int)(n0 + j % nx);                                                \
  }                                                                            \
  const int node = uniform(node_);                                             \
  const int gci = uniform(gci_);                                               \
  const int2 gcv = gc[gci];                                                    \
  const e3k_tp_group& g = groups[uniform(gcv.x)];                              \
  const int part = uniform(gcv.y) >> 16;                                        \
  const int u = (uniform(gcv.y) & 0xffff) * 64 + (threadIdx.x & 63);

struct e3k_tp_plan {
  int32_t n_groups, d_in, d_sh, w_numel, d_mid;
  e3k_tp_group* d_groups;
  int2* d_gc;     // (group, 64-channel chunk) work list, all degrees
  int32_t n_gc;
  int32_t max_l1; // largest input degree among the groups (selects the kernel instantiation)
  int32_t max_l3; // largest output degree any group's mask enables
  int32_t split;  // 1: groups with l1 >= 1 are walked by two waves (slot parts 0 / 1)
  int32_t x_cols; // input columns owned by some group: sum over groups of (2 l1 + 1) * mul
  int32_t full64;   // 1: every group has a multiple of 64 channels (the kernels drop their idle-lane handling)
  int32_t x_shared; // 1: two groups read overlapping input columns (an sh degree that repeats opens a second group)
  e3k_tp_group* h_groups;   // the groups as e3k_tp_plan_create received them (host)
};

namespace e3k {
// the calling thread's route record (e3k_tp_last_route) for a launch made outside e3k_tp.hip: `family` is a string literal
void tp_record_route(const char* family);
}  // namespace e3k
