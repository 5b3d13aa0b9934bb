// The knot-table transpose beside the weight-gradient GEMM, in ONE launch (gfx950).
//
// In the replayed training step every kernel runs alone on the chip.  Two neighbours of a layer's backward are both off the
// critical path and use different parts of it: rtable_bwd_partial_kernel (e3k_rtable.hip) is an HBM read stream without LDS or
// MFMA, gemm_wgrad2_kernel (e3k_gemm.hip) is bound by MFMA and LDS.  Here the first `first` workgroups of one launch run the
// GEMM's body on the batch and the workgroups behind them ("riders") run the transpose's body; both bodies are the stand-alone
// kernels' texts (e3k_gemm_batch.h, e3k_rtable_bwd.h), so the results are theirs.
//
// LDS is a property of the LAUNCH, not of a workgroup: a rider is allotted the GEMM's 51 200 B although it touches none of it,
// and a CU holds three workgroups of this kernel whatever their kind (160 KB / 51 200 B).  Riders therefore run BESIDE the GEMM
// only where the GEMM leaves a workgroup slot free: the batch is sized to RIDER_WG_PER_CU = 1.5 workgroups per CU instead of the
// stand-alone launch's three (fewer, longer row ranges per workgroup), which leaves every CU one or two slots for riders from
// the first cycle on; workgroups are placed in index order, so the GEMM's go first.  With at most three waves per SIMD a rider
// keeps RIDER_ROWS = 16 rows of g_w in flight instead of eight (the registers are the GEMM's 105 anyway).  Measured, DESIGN.md
// sections 4 and 5: 1.5 / 2 / 3 workgroups per CU -0.16 / -0.11 / -0.06 ms per step against the two launches.
#include "e3k_common.h"
#include "e3k_gemm_batch.h"
#include "e3k_rtable_bwd.h"

namespace e3k {

constexpr double RIDER_WG_PER_CU = 1.5;      // GEMM workgroups per CU of the fused launch
constexpr int RIDER_ROWS = 16;                // g_w rows in flight per rider wave

struct TableBwd {
  const float* gw;
  const float* coef;
  const float* scale;
  const int32_t* ptr;
  const int32_t* seg;
  const int32_t* perm;
  float* P;
  int64_t n_seg_cap;
  int32_t K, W, n_chunks;
  int32_t first;      // workgroups in front of the riders: the GEMM batch's
};
static_assert(sizeof(GemmBatch) + sizeof(TableBwd) <= 4096, "both descriptors travel by value in the kernel-argument segment");

__global__ __launch_bounds__(256, 2) void gemm_wgrad2_with_table_bwd_kernel(const GemmBatch gb, const TableBwd tb) {
  __shared__ __attribute__((aligned(16))) float As[W2_AS_FLOATS];
  __shared__ __attribute__((aligned(16))) float Gs[W2_GS_FLOATS];
  if ((int)blockIdx.x < tb.first) {      // (block-uniform)
    gemm_wgrad2_block(gb, As, Gs);
    return;
  }
  rtable_bwd_partial_body<RIDER_ROWS>(tb.gw, tb.coef, tb.scale, tb.ptr, tb.seg, tb.perm, tb.K, tb.W, tb.n_chunks, tb.n_seg_cap, tb.P,
                                          (int64_t)blockIdx.x - tb.first);
}

namespace {
struct RiderCtx {
  TableBwd tb;
  int64_t rider_blocks;
};
void launch_fused(const GemmBatch& gb, int blocks, hipStream_t st, void* ctx) {
  RiderCtx& c = *static_cast<RiderCtx*>(ctx);
  c.tb.first = blocks;
  hipLaunchKernelGGL(gemm_wgrad2_with_table_bwd_kernel, dim3((unsigned)(blocks + c.rider_blocks)), dim3(256), 0, st, gb, c.tb);
}
}  // namespace

}  // namespace e3k

extern "C" int e3k_wgrad_with_table_bwd(const e3k_gemm_segment* segments, int32_t n_segments, const float* g_w, const float* coef,
                                        const float* scale, const int32_t* bin_ptr, const int32_t* bin_seg, const int32_t* bin_perm,
                                        int64_t E, int32_t K, int32_t W, float* workspace, float* g_T, int32_t accumulate,
                                        void* stream) {
  // the table side's refusals (e3k_rtable_interp_bwd) first; the GEMM side's run inside its call, before its first launch
  e3k::gemm_routes_clear();      // (a call that is refused leaves no launch record)
  if (E < 0 || K < 4 || W <= 0) return E3K_ERR_INVALID;
  if (W % 4 || E >= 0x7fffffffLL) return E3K_ERR_UNSUPPORTED;
  if (!g_T || !bin_ptr || !bin_seg || !workspace || (E > 0 && (!g_w || !coef || !bin_perm))) return E3K_ERR_INVALID;
  e3k::RiderCtx c{};
  const int n_chunks = (W + 255) / 256;
  const int64_t cap = e3k::rtable_seg_cap(E, K);
  c.tb = e3k::TableBwd{g_w, coef, scale, bin_ptr, bin_seg, bin_perm, workspace, cap, K, W, n_chunks, 0};
  c.rider_blocks = (cap * n_chunks + 3) / 4;
  e3k::WgradHook hook{e3k::launch_fused, &c, e3k::RIDER_WG_PER_CU, false};
  // (a grid of 2^31 workgroups or more: the two launches)
  const bool fuse = E > 0 && c.rider_blocks < 0x40000000LL;
  const int rc = fuse ? e3k::gemm_multi_wgrad_hooked(segments, n_segments, stream, &hook) : e3k_gemm_multi(segments, n_segments, 1, stream);
  if (rc != E3K_OK) return rc;
  if (!hook.used)      // no problem for the pipelined kernel, or no edges
    return e3k_rtable_interp_bwd(g_w, coef, scale, bin_ptr, bin_seg, bin_perm, E, K, W, workspace, g_T, accumulate, stream);
  e3k::rtable_bwd_combine(workspace, bin_seg, K, W, accumulate, g_T, (hipStream_t)stream);
  E3K_CHECK_LAUNCH();
  return E3K_OK;
}
