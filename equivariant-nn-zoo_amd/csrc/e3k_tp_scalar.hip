// The input-gradient walk of a tensor product whose every path ends in a SCALAR: plans in which each group enables exactly the slot
// (l2 = l1, l3 = 0) -- what is left of a layer's 'uvu' product when only the 0e block of its output carries a gradient (the last
// convolution of a network whose head is an o3.Linear to 1x0e: e3_layers/nn/message_passing.py:104-109 under autograd, with the
// head of e3_layers/configs/layer_configs.py's addEnergyOutput behind it).
//
// Same execution shape as tp_bwd_x_kernel<.., kBwdXwPacked> (csrc/e3k_tp.hip): one wave per (source node, group, 64-channel chunk),
// lane = channel, the node's own rows x[s] in registers (2 l1 + 1), g_x accumulated in registers (2 l1 + 1), no LDS, no atomics.
// Per edge: the 64-byte edge record (scalar load, the next one prefetched), ONE 256-byte row of g_out[dst] (the group's 0e block),
// one packed table record per lane (dwordx2 + dword), one 256-byte streamed store of the weight gradient.  The dense kernel gathers
// 22-31 gradient rows and 6-8 records per edge and group and stores 6-8 rows.
//
//   g_x[s, x_off + i mul + u]        = sum_{e: src(e) = s} coeff w[e, u] C_ii0 sh[e, i] g_out[dst(e), out_off + u]
//   g_w[e, w_off + u]                = coeff g_out[dst(e), out_off + u] sum_i C_ii0 x[s, x_off + i mul + u] sh[e, i]
//
// with w[e, u] interpolated from the packed table exactly as the dense kernel does (knot_packed_rec / buf_ld_rec / packed_mix) and
// the sums formed by the same CG<l1, l1, 0>::yt (e3k_cg_gen.h) and the same FMA chain: both outputs carry the bits the dense kernel
// gives for these slots when the other slots' gradient rows are zero.
//
// The plan numbers its weight columns COMPACTLY (w_off, w_numel: the row of g_w); the packed table may be wider -- a dense layer's
// table [K + 1, 3 table_w], the group's column there in table_off[group].  The second kernel spreads a compact [rows, w] array over
// the dense columns (the knot-table gradient the radial stack's backward expects), zero elsewhere.
#include "e3k_tp_body.h"

namespace e3k {

constexpr int kScalarMaxGroups = 8;
struct ScalarCols {
  int32_t w_live;                           // columns of g_w (the plan's compact weight row); TpArgs.W is the packed table's
  int32_t table_off[kScalarMaxGroups];      // column of the group's slot in the packed table's rows
};
// the slot (l2 = l1, l3 = 0) of an input degree
template <int L1> struct ScalarSlot { static constexpr int Q = L1 == 0 ? 0 : (L1 == 1 ? 1 : 4); };
static_assert(Slots<0>::L2[ScalarSlot<0>::Q] == 0 && Slots<0>::L3[ScalarSlot<0>::Q] == 0, "slot table changed");
static_assert(Slots<1>::L2[ScalarSlot<1>::Q] == 1 && Slots<1>::L3[ScalarSlot<1>::Q] == 0, "slot table changed");
static_assert(Slots<2>::L2[ScalarSlot<2>::Q] == 2 && Slots<2>::L3[ScalarSlot<2>::Q] == 0, "slot table changed");

template <int L1>
__device__ __forceinline__ void tp_bwd_xw_scalar_body(const TpArgs& a, const e3k_tp_group& g, const int w_live, const int table_off,
                                                      const int node, const int u) {
  constexpr int D1 = 2 * L1 + 1, Q = ScalarSlot<L1>::Q;
  const int mul = g.mul;
  const int u4 = u * 4;
  const int goff4 = uniform(g.out_off[Q] * 4), woff4 = uniform(g.w_off[Q] * 4), toff4 = uniform(table_off * 4);
  const float cf = g.coeff[Q];
  const int row_g = a.d_mid * 4, row_t = a.W * 4, row_w = w_live * 4;
  float gx[D1], xs[D1];
  const float* __restrict__ xr = a.x + (int64_t)node * a.d_in + g.x_off;      // wave-uniform
#pragma unroll
  for (int i = 0; i < D1; ++i) {
    gx[i] = 0.0f;
    xs[i] = (xr + i * mul)[u];
  }
  const int2 rr = row_range(a.ptr, node);
  const int beg = rr.x, end = rr.y;
  EdgeRec cur{};
  if (beg < end) cur = load_rec(a.erec, beg);
  for (int t = beg; t < end; ++t) {
    const EdgeRec nxt = load_rec(a.erec, t + 1 < end ? t + 1 : t);      // (records in the order of the source-CSR walk)
    YRegs yc;
    rec_y(yc, cur);
    const __amdgpu_buffer_rsrc_t rg = row_rsrc(a.g_out + (int64_t)cur.nbr * a.d_mid, row_g);
    const __amdgpu_buffer_rsrc_t rgw = row_rsrc(a.g_w + (int64_t)cur.e * w_live, row_w);
    const KnotPacked kp = knot_packed_rec(a, cur, row_t * 3);
    float gk[1];
    gk[0] = buf_ld(rg, u4, goff4);
    const PackedRec rec = buf_ld_rec(kp.r, u4, toff4, row_t * 2);
    const float sw = packed_mix(kp, rec) * cf;
    float tq[D1];
    CG<L1, L1, 0>::yt(yref<L1>(yc), gk, tq);
    float dot = 0.0f;
#pragma unroll
    for (int i = 0; i < D1; ++i) {
      gx[i] = fmaf(sw, tq[i], gx[i]);
      dot = fmaf(xs[i], tq[i], dot);
    }
    buf_st_stream(dot * cf, rgw, u4, woff4);
    cur = nxt;
  }
  float* __restrict__ gxr = a.g_x + (int64_t)node * a.d_in + g.x_off;
#pragma unroll
  for (int i = 0; i < D1; ++i) (gxr + i * mul)[u] = gx[i];
}

__global__ __launch_bounds__(256) void tp_bwd_xw_scalar_kernel(TpArgs a, ScalarCols cols, const e3k_tp_group* __restrict__ groups,
                                                               const int2* __restrict__ gc, int n_gc) {
  E3K_TP_PROLOGUE
  (void)part;
  const int toff = cols.table_off[uniform(gcv.x)];
  const int l1 = g.l1;
  if (l1 == 0) tp_bwd_xw_scalar_body<0>(a, g, cols.w_live, toff, node, u);
  else if (l1 == 1) tp_bwd_xw_scalar_body<1>(a, g, cols.w_live, toff, node, u);
  else tp_bwd_xw_scalar_body<2>(a, g, cols.w_live, toff, node, u);
}

constexpr int kExpandMaxRanges = E3K_NARROW_MAX_SLOTS;      // (a range per live slot of a narrow layer; callers merge neighbours)
struct ExpandRanges {
  int32_t n;
  int32_t src[kExpandMaxRanges], dst[kExpandMaxRanges], len[kExpandMaxRanges];      // columns; all multiples of 4
};
// dst [rows, w_dst] = 0 except dst[r, ranges.dst[k] + c] = src[r, ranges.src[k] + c]; one thread per four columns of dst
__global__ __launch_bounds__(256) void expand_columns_kernel(const float* __restrict__ src, int64_t rows, int w_src, int w_dst,
                                                             ExpandRanges rg, float* __restrict__ dst) {
  const int q_dst = w_dst / 4;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= rows * q_dst) return;
  const int64_t r = i / q_dst;
  const int c = (int)(i - r * q_dst) * 4;
  float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int k = 0; k < rg.n; ++k)
    if (c >= rg.dst[k] && c < rg.dst[k] + rg.len[k]) v = *reinterpret_cast<const float4*>(src + r * w_src + rg.src[k] + (c - rg.dst[k]));
  *reinterpret_cast<float4*>(dst + r * w_dst + c) = v;
}

}  // namespace e3k

extern "C" int e3k_tp_scalar_supported(const e3k_tp_plan* p) {
  if (!p || !p->h_groups || p->n_groups > e3k::kScalarMaxGroups || p->split || p->x_shared || p->d_sh != 9) return 0;
  int64_t w = 0;
  for (int i = 0; i < p->n_groups; ++i) {
    const e3k_tp_group& g = p->h_groups[i];
    if (g.l1 < 0 || g.l1 > 2 || g.mul <= 0 || g.mul % 64) return 0;
    const int q = g.l1 == 0 ? e3k::ScalarSlot<0>::Q : (g.l1 == 1 ? e3k::ScalarSlot<1>::Q : e3k::ScalarSlot<2>::Q);
    if (g.mask != (1u << q)) return 0;
    // the edge records carry sh degrees 0, 1, 2 at columns 0, 1, 4
    if (g.y_off[g.l1] != (g.l1 == 0 ? 0 : (g.l1 == 1 ? 1 : 4))) return 0;
    if (g.x_off < 0 || g.x_off + (2 * g.l1 + 1) * g.mul > p->d_in) return 0;
    if (g.out_off[q] < 0 || g.out_off[q] + g.mul > p->d_mid || g.w_off[q] < 0 || g.w_off[q] + g.mul > p->w_numel) return 0;
    w += g.mul;
  }
  return w <= p->w_numel ? 1 : 0;
}

extern "C" int e3k_tp_bwd_xw_scalar_ptable(const e3k_tp_plan* plan, const float* x, const void* P, int32_t table_w,
                                           const int32_t* table_off, const int32_t* erec_src, const float* g_out,
                                           const int32_t* src_ptr, int64_t N, int64_t E, float* g_x, float* g_w, void* stream) {
  if (!plan || N < 0 || E < 0) return E3K_ERR_INVALID;
  if (!e3k_tp_scalar_supported(plan)) return E3K_ERR_UNSUPPORTED;
  if (N == 0) return E3K_OK;
  if (!x || !g_out || !g_x || !src_ptr || (E > 0 && (!P || !erec_src || !g_w))) return E3K_ERR_INVALID;
  if (reinterpret_cast<uintptr_t>(erec_src) & 63) return E3K_ERR_UNSUPPORTED;
  if (table_off ? table_w <= 0 : table_w != 0) return E3K_ERR_INVALID;
  const int tw = table_off ? table_w : plan->w_numel;
  if ((int64_t)tw * 12 > 0x7fffffffLL) return E3K_ERR_UNSUPPORTED;
  e3k::ScalarCols cols{};
  cols.w_live = plan->w_numel;
  for (int i = 0; i < plan->n_groups; ++i) {
    const e3k_tp_group& g = plan->h_groups[i];
    const int q = g.l1 == 0 ? e3k::ScalarSlot<0>::Q : (g.l1 == 1 ? e3k::ScalarSlot<1>::Q : e3k::ScalarSlot<2>::Q);
    cols.table_off[i] = table_off ? table_off[i] : g.w_off[q];
    if (cols.table_off[i] < 0 || cols.table_off[i] + g.mul > tw) return E3K_ERR_INVALID;
  }
  const int n_gc = plan->n_gc;
  e3k::TpArgs a{};
  a.d_in = plan->d_in; a.d_sh = plan->d_sh; a.d_mid = plan->d_mid;
  a.W = tw;                    // the packed table's columns (a.w); g_w's are cols.w_live
  a.ptr = src_ptr;
  a.x = x; a.w = static_cast<const float*>(P); a.erec = erec_src; a.g_out = g_out; a.g_x = g_x; a.g_w = g_w;
  a.n_items = N * n_gc;
  // the work order of the dense packed kinds (launch_all, e3k_tp.hip): one sub-grid per XCD from 64 nodes on
  a.order = N >= 64 ? 1 : 0;
  int64_t blocks = (a.n_items + 3) / 4;
  if (a.order) blocks = 8 * ((((N + 7) / 8) * n_gc + 3) / 4);
  if (blocks > 0x7fffffffLL) return E3K_ERR_INVALID;
  if (blocks == 0) return E3K_OK;
  e3k::tp_record_route("tp_bwd_xw_scalar_kernel");
  hipLaunchKernelGGL(e3k::tp_bwd_xw_scalar_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, a, cols, plan->d_groups,
                     plan->d_gc, n_gc);
  E3K_CHECK_LAUNCH();
  return E3K_OK;
}

extern "C" int e3k_expand_columns(const float* src, int64_t rows, int32_t w_src, int32_t w_dst, const int32_t* src_col,
                                  const int32_t* dst_col, const int32_t* len, int32_t n_ranges, float* dst, void* stream) {
  if (rows < 0 || w_src <= 0 || w_dst <= 0 || n_ranges < 0 || (n_ranges && (!src_col || !dst_col || !len))) return E3K_ERR_INVALID;
  if (n_ranges > e3k::kExpandMaxRanges || (w_src % 4) || (w_dst % 4)) return E3K_ERR_UNSUPPORTED;
  if (rows == 0) return E3K_OK;
  if (!dst || (n_ranges && !src)) return E3K_ERR_INVALID;
  if ((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst)) & 15) return E3K_ERR_UNSUPPORTED;
  e3k::ExpandRanges rg{};
  rg.n = n_ranges;
  for (int k = 0; k < n_ranges; ++k) {
    if (src_col[k] < 0 || dst_col[k] < 0 || len[k] <= 0 || src_col[k] + len[k] > w_src || dst_col[k] + len[k] > w_dst) return E3K_ERR_INVALID;
    if ((src_col[k] | dst_col[k] | len[k]) & 3) return E3K_ERR_UNSUPPORTED;
    for (int j = 0; j < k; ++j)
      if (dst_col[k] < dst_col[j] + len[j] && dst_col[j] < dst_col[k] + len[k]) return E3K_ERR_INVALID;      // ranges of dst overlap
    rg.src[k] = src_col[k]; rg.dst[k] = dst_col[k]; rg.len[k] = len[k];
  }
  const int64_t blocks = (rows * (w_dst / 4) + 255) / 256;
  if (blocks > 0x7fffffffLL) return E3K_ERR_INVALID;
  hipLaunchKernelGGL(e3k::expand_columns_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, src, rows, w_src, w_dst, rg, dst);
  E3K_CHECK_LAUNCH();
  return E3K_OK;
}
