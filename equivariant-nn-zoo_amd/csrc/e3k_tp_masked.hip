// The fused packed-table input-gradient walk (tp_bwd_x_kernel<.., kBwdXwPacked>, csrc/e3k_tp.hip) for a plan that keeps only SOME
// slots of its groups: what is left of a layer's 'uvu' product when the gradient of its output is zero outside some column blocks
// and the dead paths are not all but one per group (that case is e3k_tp_scalar.hip's).  The layer below the last convolution of a
// network with a scalar head: half of its slots at l_max 2 (backend/conv_native.py, NativeLayer.narrow).
//
// Same execution shape as the dense kernel: one wave per (source node, group, 64-channel chunk), lane = channel, x[s] and g_x in
// registers, the 64-byte edge record prefetched one edge ahead, no LDS.  Per slot a wave-uniform test of the group's mask skips the
// rows of g_out, the table record, the CG contraction and the store of the weight gradient.  The branch around a dead slot's row
// loads sets the row registers to zero instead: with those left undefined the compiler needs 80 bytes of scratch per lane at eight
// waves per SIMD, with them defined 63 VGPRs and none (the dense kernel: 61).  Live slots are visited in the dense
// kernel's order with its products (knot_packed_rec / buf_ld_rec / packed_mix, CG<l1, l2, l3>::yt, the same FMA chain); the dense
// kernel adds fmaf(sw, 0, gx) for a slot whose rows of g_out are zero, so g_x and the live columns of g_w carry the dense kernel's
// bits where g_x is stored (no input block shared between groups).
//
// Two column offsets per slot: the plan numbers its weight columns COMPACTLY (w_off, w_numel: the row of g_w); the packed table is
// the dense layer's, [K + 1, 3 table_w], the slot's column there in MaskedCols::table_off[group][slot].
#include "e3k_tp_body.h"

namespace e3k {

constexpr int kMaskedMaxGroups = 8;
constexpr int kMaskedL3Max = 2;      // output degrees the kernel carries accumulators for (un-split plans: l_max <= 2 models)
struct MaskedCols {
  int32_t w_live;                                      // columns of g_w (the plan's compact weight row); TpArgs.W is the packed table's
  int32_t table_off[kMaskedMaxGroups][E3K_MAXQ];       // column of (group, slot) in the packed table's rows
};

template <int L1>
__device__ __forceinline__ void tp_bwd_xw_masked_body(const TpArgs& a, const e3k_tp_group& g, const MaskedCols& cols, const int gi,
                                                      const int node, const int u) {
  using S = Slots<L1>;
  constexpr int D1 = 2 * L1 + 1, L3MAX = kMaskedL3Max;
  const int mul = g.mul;
  const int u4 = u * 4;
  const unsigned mask = uniform(g.mask);
  const int row_g = a.d_mid * 4, row_t = a.W * 4, row_w = cols.w_live * 4;
  int goff4[S::NQ], gstr4[S::NQ], woff4[S::NQ], toff4[S::NQ];
  float cf[S::NQ];
  slot_for_part<S, L1, L3MAX, 2>([&](auto qc) {
    constexpr int Q = decltype(qc)::value;
    goff4[Q] = uniform(g.out_off[Q] * 4);
    gstr4[Q] = uniform(g.out_stride[Q] * 4);
    woff4[Q] = uniform(g.w_off[Q] * 4);
    toff4[Q] = uniform(cols.table_off[gi][Q] * 4);
    cf[Q] = g.coeff[Q];
  });
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
    const __amdgpu_buffer_rsrc_t rgw = row_rsrc(a.g_w + (int64_t)cur.e * cols.w_live, row_w);
    const KnotPacked kp = knot_packed_rec(a, cur, row_t * 3);
    float gn[S::TOTAL];
    PackedRec rec[S::NQ];
    slot_for_part<S, L1, L3MAX, 2>([&](auto qc) {
      constexpr int Q = decltype(qc)::value;
      constexpr int L3 = S::L3[Q], OFF = S::OFF[Q];
      if (mask & (1u << Q)) {
#pragma unroll
        for (int k = 0; k < 2 * L3 + 1; ++k)
          gn[OFF + k] = buf_ld(rg, u4, goff4[Q] + k * gstr4[Q]);
        rec[Q] = buf_ld_rec(kp.r, u4, toff4[Q], row_t * 2);
      } else {      // (defined values: with the rows left undefined here the kernel needs scratch, see the top of the file)
#pragma unroll
        for (int k = 0; k < 2 * L3 + 1; ++k) gn[OFF + k] = 0.0f;
      }
    });
    __builtin_amdgcn_sched_barrier(0);
    float wn[S::NQ];
    slot_for_part<S, L1, L3MAX, 2>([&](auto qc) {
      constexpr int Q = decltype(qc)::value;
      wn[Q] = packed_mix(kp, rec[Q]);
    });
    slot_for_part<S, L1, L3MAX, 2>([&](auto qc) {
      constexpr int Q = decltype(qc)::value;
      constexpr int L2 = S::L2[Q], L3 = S::L3[Q], OFF = S::OFF[Q];
      if (mask & (1u << Q)) {
        float gk[2 * L3 + 1];
#pragma unroll
        for (int k = 0; k < 2 * L3 + 1; ++k) gk[k] = gn[OFF + k];
        float tq[D1];
        CG<L1, L2, L3>::yt(yref<L2>(yc), gk, tq);
        const float sw = wn[Q] * cf[Q];
        float dot = 0.0f;
#pragma unroll
        for (int i = 0; i < D1; ++i) {
          gx[i] = fmaf(sw, tq[i], gx[i]);
          dot = fmaf(xs[i], tq[i], dot);
        }
        buf_st_stream(dot * cf[Q], rgw, u4, woff4[Q]);
      }
    });
    cur = nxt;
  }
  float* __restrict__ gxr = a.g_x + (int64_t)node * a.d_in + g.x_off;
#pragma unroll
  for (int i = 0; i < D1; ++i) {
    if (!a.x_shared) (gxr + i * mul)[u] = gx[i];
    else atomicAdd(gxr + i * mul + u, gx[i]);
  }
}

// (eight waves per SIMD as the dense kernel is built: E3K_TP_BWDX_WAVES, e3k_tp.hip)
__global__ __launch_bounds__(256, 8) void tp_bwd_xw_masked_kernel(TpArgs a, MaskedCols cols, const e3k_tp_group* __restrict__ groups,
                                                                  const int2* __restrict__ gc, int n_gc) {
  E3K_TP_PROLOGUE
  (void)part;
  const int gi = uniform(gcv.x);
  const int l1 = g.l1;
  if (l1 == 0) tp_bwd_xw_masked_body<0>(a, g, cols, gi, node, u);
  else if (l1 == 1) tp_bwd_xw_masked_body<1>(a, g, cols, gi, node, u);
  else tp_bwd_xw_masked_body<2>(a, g, cols, gi, node, u);
}

namespace {
// output degree of slot q of input degree l1 (l1 <= 2), -1 past the last slot
int masked_slot_l3(int l1, int q) {
  if (q < 0) return -1;
  if (l1 == 0) return q < Slots<0>::NQ ? Slots<0>::L3[q] : -1;
  if (l1 == 1) return q < Slots<1>::NQ ? Slots<1>::L3[q] : -1;
  return q < Slots<2>::NQ ? Slots<2>::L3[q] : -1;
}
}  // namespace

}  // namespace e3k

extern "C" int e3k_tp_masked_supported(const e3k_tp_plan* p) {
  if (!p || !p->h_groups || p->n_groups > e3k::kMaskedMaxGroups || p->split || p->d_sh != 9) return 0;
  for (int i = 0; i < p->n_groups; ++i) {
    const e3k_tp_group& g = p->h_groups[i];
    if (g.l1 < 0 || g.l1 > 2 || g.mul <= 0 || g.mul % 64 || !g.mask) return 0;
    // the edge records carry sh degrees 0, 1, 2 at columns 0, 1, 4
    if (g.y_off[0] != 0 || g.y_off[1] != 1 || g.y_off[2] != 4) return 0;
    if (g.x_off < 0 || g.x_off + (2 * g.l1 + 1) * g.mul > p->d_in) return 0;
    for (int q = 0; q < E3K_MAXQ; ++q) {
      if (!((g.mask >> q) & 1u)) continue;
      const int l3 = e3k::masked_slot_l3(g.l1, q);
      if (l3 < 0 || l3 > e3k::kMaskedL3Max) return 0;
      if (g.out_off[q] < 0 || g.out_stride[q] < 0 || (int64_t)g.out_off[q] + 2 * l3 * (int64_t)g.out_stride[q] + g.mul > p->d_mid) return 0;
      if (g.w_off[q] < 0 || g.w_off[q] + g.mul > p->w_numel) return 0;
    }
  }
  return 1;
}

extern "C" int e3k_tp_bwd_xw_masked_ptable(const e3k_tp_plan* plan, const float* x, const void* P, int32_t table_w,
                                           const int32_t* live_col, const int32_t* erec_src, const float* g_out,
                                           const int32_t* src_ptr, int64_t N, int64_t E, float* g_x, float* g_w, void* stream) {
  if (!plan || N < 0 || E < 0) return E3K_ERR_INVALID;
  if (!e3k_tp_masked_supported(plan)) return E3K_ERR_UNSUPPORTED;
  if (N == 0) return E3K_OK;
  if (!x || !g_out || !g_x || !src_ptr || (E > 0 && (!P || !erec_src || !g_w))) return E3K_ERR_INVALID;
  if (reinterpret_cast<uintptr_t>(erec_src) & 63) return E3K_ERR_UNSUPPORTED;
  if (live_col ? table_w <= 0 : table_w != 0) return E3K_ERR_INVALID;
  const int tw = live_col ? table_w : plan->w_numel;
  if ((int64_t)tw * 12 > 0x7fffffffLL) return E3K_ERR_UNSUPPORTED;
  e3k::MaskedCols cols{};
  cols.w_live = plan->w_numel;
  for (int i = 0, k = 0; i < plan->n_groups; ++i) {
    const e3k_tp_group& g = plan->h_groups[i];
    for (int q = 0; q < E3K_MAXQ; ++q) {
      if (!((g.mask >> q) & 1u)) continue;
      const int col = live_col ? live_col[k] : g.w_off[q];
      ++k;
      if (col < 0 || col + g.mul > tw) return E3K_ERR_INVALID;
      cols.table_off[i][q] = col;
    }
  }
  const int n_gc = plan->n_gc;
  e3k::TpArgs a{};
  a.d_in = plan->d_in; a.d_sh = plan->d_sh; a.d_mid = plan->d_mid;
  a.W = tw;                    // the packed table's columns (a.w); g_w's are cols.w_live
  a.ptr = src_ptr;
  a.x = x; a.w = static_cast<const float*>(P); a.erec = erec_src; a.g_out = g_out; a.g_x = g_x; a.g_w = g_w;
  a.x_shared = plan->x_shared;
  a.n_items = N * n_gc;
  // the work order of the dense packed kinds (launch_all, e3k_tp.hip): one sub-grid per XCD from 64 nodes on
  a.order = N >= 64 ? 1 : 0;
  int64_t blocks = (a.n_items + 3) / 4;
  if (a.order) blocks = 8 * ((((N + 7) / 8) * n_gc + 3) / 4);
  if (blocks > 0x7fffffffLL) return E3K_ERR_INVALID;
  if (blocks == 0) return E3K_OK;
  e3k::tp_record_route("tp_bwd_xw_masked_kernel");
  hipLaunchKernelGGL(e3k::tp_bwd_xw_masked_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, a, cols, plan->d_groups,
                     plan->d_gc, n_gc);
  E3K_CHECK_LAUNCH();
  return E3K_OK;
}
