/*
 * e3k.h — C ABI of libe3k.so, the MI355X (gfx950) kernels behind the e3_layers tensor-product
 * message-passing path.
 *
 * The reference (20171130/Equivariant-NN-Zoo) has no native plugin interface: its hot path is
 * Python that calls e3nn / torch_runstats operators.  Each entry point below
 * therefore cites the *operator call site* it replaces (paths relative to /root/reference).
 *
 * Conventions
 *  - every pointer is a DEVICE pointer owned by the caller (PyTorch on the Python side); the
 *    library allocates nothing except the opaque plans created by e3k_tp_plan_create;
 *  - `stream` is a hipStream_t passed as void*; all work is enqueued on it, nothing synchronises;
 *  - return value: 0 = ok, <0 = error (see e3k_strerror); no exceptions cross the boundary;
 *  - floating tensors are fp32, node/edge ids are int32 inside the library (the int64
 *    `edge_index` of the reference's Batch is narrowed once per batch by the host shim);
 *  - feature layouts: "e3nn" = each `mul x l` block stored [mul][2l+1] (reference layout,
 *    README.md:108-110); "cf" = channel-fastest, block stored [2l+1][mul] (internal layout of
 *    the fused convolution: 64 channels = 64 lanes read 256 contiguous bytes).
 *
 * THIS HEADER IS PARSED: the Python binding (e3_layers_amd/backend/abi.py -> lib.py) derives every ctypes struct, signature
 * and constant from it at import, so it is the only place the interface is written down -- and it must stay inside the C
 * subset that parser knows (anything else makes the import raise, naming the text):
 *  - `#define E3K_NAME <integer literal>`, optionally parenthesised (expression bodies are allowed and ignored); no other
 *    preprocessor line between the include guard and its #endif but the two `extern "C"` blocks;
 *  - `typedef struct { ... } e3k_x;` and opaque `typedef struct e3k_x e3k_x;` -- no unions, enums, bit-fields, nested
 *    struct bodies or function pointers;
 *  - fields and parameters of the types int, int32_t, uint32_t, int64_t, uint8_t, float, double, structs defined above
 *    (by value or by pointer), pointers (to pointers) to any of these, to void and to opaque types, `const` anywhere;
 *    several declarators per line (`void *a, *b;`); field arrays sized by a literal or an integer #define;
 *  - prototypes returning int, int64_t, void or const char*.
 */
#ifndef E3K_H
#define E3K_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define E3K_OK 0
#define E3K_ERR_INVALID (-1)     /* bad argument / unsupported shape */
#define E3K_ERR_LAUNCH (-2)      /* hip launch or runtime error */
#define E3K_ERR_UNSUPPORTED (-3) /* degree beyond the generated CG tables */

#define E3K_TP_MAXQ 8 /* max (l2,l3) slots per input degree — must equal E3K_MAXQ of e3k_cg_gen.h */
#define E3K_NARROW_MAX_SLOTS 48 /* live path slots a narrow layer can name (e3k_layer_desc.live_col; e3k_expand_columns' ranges) */

const char* e3k_strerror(int code);
int e3k_version(void);
/* compile-time limits of the generated Clebsch-Gordan tables: l1max, l2max, l3max */
void e3k_tp_limits(int* l1max, int* l2max, int* l3max);

/* ------------------------------------------------------------------------------------------
 * Grouped strided GEMM on the f32 MFMA pipe (v_mfma_f32_32x32x2_f32).
 * Replaces: o3.Linear (nn/message_passing.py:58,102; nn/pointwise.py:18,87,142),
 *           e3nn.nn.FullyConnectedNet layers (nn/message_passing.py:74,93),
 *           o3.FullyConnectedTensorProduct with scalar second operand (nn/message_passing.py:83,100).
 *
 * One problem computes, for rows (r1, r2), r1 < M1, r2 < M2:
 *     C[r1, r2, n] = alpha * sum_k Aeff[r1, r2, k] * B[k, n]  (+ C if accumulate) (+ bias[n])
 * with   A addr = A + r1*a_r1 + r2*a_r2 + k*a_k,  B addr = B + k*b_k + n*b_n,
 *        C addr = C + r1*c_r1 + r2*c_r2 + n*c_n   (all strides in elements).
 * Outer mode (V > 0): K = U*V and Aeff[r1,r2,u*V+v] = A[r1,r2,u] * A2[r1*a2_r1 + v]
 * (the x (x) node_attrs operand of the self-connection, never materialised).
 * ------------------------------------------------------------------------------------------ */
typedef struct {
  const float* A;
  const float* A2;
  const float* B;
  float* C;
  const float* bias;
  const int32_t* row_index; /* optional: r1 := row_index[r1] for the A, A2 and C rows (grouped GEMM over a
                               gathered subset of nodes); M1 = length of the list */
  const int32_t* group_dev; /* optional, with row_index: DEVICE pair {start, count}; the list is
                               row_index[start .. start+count) and M1 is only an upper bound of count
                               (grids are sized from M1, surplus workgroups exit) -- no host sync needed */
  int32_t M1, M2, N, K;
  int32_t V;
  int32_t accumulate;
  int64_t a_r1, a_r2, a_k;
  int64_t a2_r1;
  int64_t b_k, b_n;
  int64_t c_r1, c_r2, c_n;
  float alpha;
  int32_t act;   /* 0 none; 1: C = act_cst * ssp(alpha*A.B + bias) fused into the epilogue (radial MLP layers) */
  float act_cst; /* second-moment normalisation constant of the activation */
  int32_t chain; /* K-chain (e3k_gemm, e3k_gemm_multi; forward / input-gradient problems only): the `chain` problems that FOLLOW
                    this one in the array continue its K loop into the same accumulators,
                        C = alpha_0 A_0.B_0 + alpha_1 A_1.B_1 + ...  (+ C if the head accumulates) (+ the head's bias, activation),
                    in ONE pass over C instead of one accumulating launch per term -- e3nn's o3.Linear input gradient of an irrep
                    that feeds several outputs (e3_layers/nn/pointwise.py:87-92: `0e` feeds the scalars and the gates).  A follower
                    repeats the head's M1, M2, N, C, c_* strides, row_index / group_dev (keyed: the same groups) and has chain = 0,
                    V = 0, no bias; it brings A, B, K, their strides and alpha.  Every link runs on the plain kernel. */
} e3k_gemm_problem;

/* Rows of one problem: M1 * M2 <= E3K_GEMM_MAX_ROWS, else the call fails with E3K_ERR_UNSUPPORTED (the kernels index rows in
 * 32-bit ints; the margin below 2^31 covers a row tile and a chunk of rows past the last one). */
#define E3K_GEMM_MAX_ROWS ((1LL << 31) - (1LL << 16))

int e3k_gemm(const e3k_gemm_problem* problems, int n_problems, void* stream);

/* Weight gradient ("TN"):  B[k, n] += alpha * sum_{r1,r2} Aeff[r1,r2,k] * C[r1,r2,n]
 * (C is read as the incoming gradient, B is accumulated with fp32 atomics; the caller zeroes B). */
int e3k_gemm_wgrad(const e3k_gemm_problem* problems, int n_problems, void* stream);

/* Cached-descriptor launch: `templates` is an array the host built once per (layer, pass); its pointer fields hold
 * BYTE OFFSETS instead of addresses -- A, B, C relative to a_base, b_base, c_base; A2 and bias hold offset + 1
 * (0 = absent) relative to a2_base, bias_base -- and M1 is overwritten by the argument.  wgrad != 0 runs
 * e3k_gemm_wgrad semantics.  Same kernels, same results as e3k_gemm / e3k_gemm_wgrad on the resolved problems. */
int e3k_gemm_rebased(const e3k_gemm_problem* templates, int n_templates, const void* a_base, const void* a2_base,
                     const void* b_base, void* c_base, const void* bias_base, int64_t M1, int32_t wgrad,
                     void* stream);

/* Several descriptor arrays in ONE call (as few launches as the kernel kinds allow; up to 20 problems per launch, keyed
 * and plain problems mixed): what a convolution layer issues together -- linear_1 with the keyed self-connection
 * (e3_layers/nn/message_passing.py:100,102: both read the node features), the input gradients of the trailing Linear
 * and of the self-connection (both read the gradient of the convolution output), the three weight gradients.
 * A segment is a template array as for e3k_gemm_rebased (byte offsets in the pointer fields, M1 >= 0 overwrites the
 * templates' row count; M1 < 0: the templates carry addresses and row counts) and, with n_keys > 0, the key expansion
 * of e3k_gemm_grouped (row_index = perm, group_dev = groups_dev + 2 t, B += t * b_key_stride for key t).
 * At most 64 problems per call. */
typedef struct {
  const e3k_gemm_problem* templates;
  int32_t n_templates;
  int32_t n_keys;            /* 0: plain problems */
  const void* a_base;
  const void* a2_base;
  const void* b_base;
  void* c_base;
  const void* bias_base;
  int64_t M1;
  const int32_t* perm;
  const int32_t* groups_dev;
  int64_t b_key_stride;
} e3k_gemm_segment;
int e3k_gemm_multi(const e3k_gemm_segment* segments, int32_t n_segments, int32_t wgrad, void* stream);

/* Grouped launch over key groups: every template problem is expanded into n_keys problems, one per
 * key t, with  B += t * b_key_stride,  row_index = perm,  group_dev = groups_dev + 2*t  and M1 kept as the
 * (host-known) upper bound of the group size.  wgrad != 0 runs e3k_gemm_wgrad semantics (B accumulated).
 * Used by the keyed self-connection: rows = nodes sorted by the key of their attribute row.
 * The key groups must PARTITION the problem's M1 rows (counts summing to at most M1, as a stable sort by key gives):
 * the grid is sized for M1 rows plus one partial tile per key, not n_keys times M1 (compact keyed grids), and
 * with groups that overlap or over-count, the rows past that budget are not computed.  Nothing checks this at run time. */
int e3k_gemm_grouped(const e3k_gemm_problem* templates, int n_templates, const int32_t* perm,
                     const int32_t* groups_dev, int32_t n_keys, int64_t b_key_stride, int32_t wgrad, void* stream);

/* e3k_gemm_grouped over cached descriptors: A, B, C of the templates hold byte offsets relative to the bases (as in
 * e3k_gemm_rebased; no A2 / bias in keyed problems), M1 is overwritten. */
int e3k_gemm_grouped_rebased(const e3k_gemm_problem* templates, int n_templates, const void* a_base,
                             const void* b_base, void* c_base, int64_t M1, const int32_t* perm,
                             const int32_t* groups_dev, int32_t n_keys, int64_t b_key_stride, int32_t wgrad,
                             void* stream);

/* Column sums: out[n] += sum_r G[r*ld + n]   (bias gradients) */
int e3k_colsum(const float* G, int64_t rows, int32_t cols, int64_t ld, float* out, void* stream);

/* Self-connection backward helper: H[(r1,r2),(u,v)] = dC . W^T was produced by e3k_gemm; this
 * reduces it to  dX[r1,r2,u] (+)= sum_v A2[r1,v] H[..,(u,v)]  and  dA2[r1,v] += sum_{r2,u} X[r1,r2,u] H[..].
 * X/dX addressed as x + r1*x_r1 + r2*x_r2 + u (cf layout). */
int e3k_fctp_reduce_bwd(const float* H, const float* X, const float* A2, int32_t M1, int32_t M2, int32_t U,
                        int32_t V, int64_t x_r1, int64_t x_r2, int64_t a2_r1, float* dX, int32_t dx_accumulate,
                        float* dA2, void* stream);

/* The launches of the calling thread's most recent call of e3k_gemm, e3k_gemm_wgrad, e3k_gemm_multi, e3k_gemm_rebased,
 * e3k_gemm_grouped, e3k_gemm_grouped_rebased, e3k_colsum or e3k_fctp_reduce_bwd, in launch order and separated by ';': the kernel
 * as e3k_gemm.hip spells it, with the number of problems of a batched launch in brackets, e.g.
 * "gemm_n1_kernel;gemm_kernel<2, false>[20];gemm_kernel<2, false>[3];gemm_splitk_kernel[2]".  Empty when the call launched nothing
 * or failed (every call clears it on entry).  For tests: which kernels a call reached.  Valid until the thread's next such call. */
const char* e3k_gemm_last_routes(void);

/* ------------------------------------------------------------------------------------------
 * Edge geometry.  Replaces computeEdgeVector (data/compute_edge.py:13-36),
 * o3.SphericalHarmonics via SphericalEncoding (nn/embedding.py:163-178) and
 * BesselBasis x cutoff via RadialBasisEncoding (nn/embedding.py:114-127,31-40,210-219).
 * ------------------------------------------------------------------------------------------ */
int e3k_edge_vector_fwd(const float* pos, const int32_t* src, const int32_t* dst, int64_t E, float* edge_vec,
                        float* edge_len, void* stream);
/* g_pos[n] = sum_{e: dst=n} gv[e] - sum_{e: src=n} gv[e], gv = g_vec + g_len * vec/len; CSR by dst and by src */
int e3k_edge_vector_bwd(const float* g_vec, const float* g_len, const float* edge_vec, const float* edge_len,
                        const int32_t* dst_ptr, const int32_t* dst_perm, const int32_t* src_ptr,
                        const int32_t* src_perm, int64_t N, float* g_pos, void* stream);

/* ls: a HOST list of n_ls <= 8 degrees, each 0 .. 3, in any order and with repeats; the output holds one block of 2l + 1 components
 * per entry, in the order of the list (dim = sum of 2l + 1).  normalization: 0 component, 1 integral, 2 norm.
 * normalize != 0 evaluates at u = vec / max(|vec|, 1e-12) (torch.nn.functional.normalize): the zero vector gives u = 0 (every block
 * of l >= 1 is zero), a vector shorter than 1e-12 is scaled by 1e12 and NOT brought to unit length; in both cases the backward passes
 * treat the divisor as the constant 1e-12 (no projection onto the tangent plane). */
int e3k_sph_harm_fwd(const float* vec, int64_t E, const int32_t* ls, int32_t n_ls, int32_t normalize,
                     int32_t normalization, float* sh, void* stream);
int e3k_sph_harm_bwd(const float* vec, const float* g_sh, int64_t E, const int32_t* ls, int32_t n_ls,
                     int32_t normalize, int32_t normalization, float* g_vec, void* stream);
/* double backward: g_hat [E,3] is the cotangent of e3k_sph_harm_bwd's g_vec.
 * g_gsh [E,dim] = J(vec) g_hat;  g_vec [E,3] = d/dvec <g_hat, sph_harm_bwd(vec, g_sh)>  (either may be NULL). */
int e3k_sph_harm_bwd2(const float* vec, const float* g_sh, const float* g_hat, int64_t E, const int32_t* ls,
                      int32_t n_ls, int32_t normalize, int32_t normalization, float* g_gsh, float* g_vec,
                      void* stream);

/* cutoff_kind: 0 polynomial (p), 1 symmetric (x^2-1)^2 */
int e3k_radial_basis_fwd(const float* r, int64_t E, const float* bessel_w, int32_t n_basis, float r_max, float r_min,
                         float p, int32_t one_over_r, int32_t cutoff_kind, float* out, void* stream);
/* g_r [E] is written; g_w [n_basis] is ACCUMULATED with atomics (the caller zeroes it).  Either may be NULL, not both. */
int e3k_radial_basis_bwd(const float* r, const float* g_out, int64_t E, const float* bessel_w, int32_t n_basis,
                         float r_max, float r_min, float p, int32_t one_over_r, int32_t cutoff_kind, float* g_r,
                         float* g_w, void* stream);
/* The compile-time bound of e3k_radial_basis_bwd's basis loop for n_basis: 8, 16, 32 or 64 (the smallest that holds n_basis), or -1
 * for a count the launcher refuses (n_basis <= 0 or > 64).  Host only: nothing is launched. */
int e3k_radial_basis_bwd_unroll(int32_t n_basis);
/* double backward: hat_r [E] / hat_w [n_basis] are the cotangents of e3k_radial_basis_bwd's g_r / g_w (either
 * may be NULL = zero).  g_gout [E,n_basis] = d out along (hat_r, hat_w); g_r [E] written, g_w [n_basis]
 * ACCUMULATED (caller zeroes): the second derivatives contracted with g_out.  Outputs may be NULL. */
int e3k_radial_basis_bwd2(const float* r, const float* g_out, const float* hat_r, const float* hat_w, int64_t E,
                          const float* bessel_w, int32_t n_basis, float r_max, float r_min, float p,
                          int32_t one_over_r, int32_t cutoff_kind, float* g_gout, float* g_r, float* g_w,
                          void* stream);

/* ------------------------------------------------------------------------------------------
 * Fused 'uvu' tensor product + destination reduce.
 * Replaces TensorProductExpansion.tp (nn/pointwise.py:78-85,94-99) applied to x[edge_src]
 * (nn/message_passing.py:104-106) followed by scatter over edge_dst (:109).  The trailing
 * per-edge o3.Linear of the reference (nn/pointwise.py:87-92,99) commutes with the sum and is
 * applied on nodes by e3k_gemm.
 *
 * A group = one input irrep block (degree l1, `mul` channels at x_off in the cf row) and up
 * to E3K_TP_MAXQ paths, at most one per (l2, l3) slot; slot q is the q-th valid (l2,l3) pair
 * for l1 in the order of e3k_cg_gen.h (l2 ascending, then l3 ascending).
 *   out[n, out_off[q] + k*out_stride[q] + u] =
 *       sum_{e: dst(e)=n} coeff[q] * w[e, w_off[q]+u] * sum_ij C_ijk x[src(e), x_off + i*mul + u] sh[e, y_off[l2]+j]
 * ------------------------------------------------------------------------------------------ */
typedef struct {
  int32_t l1, x_off, mul;
  uint32_t mask; /* bit q set => slot q present */
  int32_t y_off[4];
  int32_t w_off[E3K_TP_MAXQ];
  int32_t out_off[E3K_TP_MAXQ];
  int32_t out_stride[E3K_TP_MAXQ];
  float coeff[E3K_TP_MAXQ];
} e3k_tp_group;

typedef struct e3k_tp_plan e3k_tp_plan;

int e3k_tp_plan_create(const e3k_tp_group* groups, int32_t n_groups, int32_t d_in, int32_t d_sh, int32_t w_numel,
                       int32_t d_mid, e3k_tp_plan** plan);
void e3k_tp_plan_destroy(e3k_tp_plan* plan);

/* x [N,d_in] cf, sh [E,d_sh], w [E,w_numel]; src [E]; CSR by destination (dst_ptr [N+1],
 * dst_perm [E] = edge ids grouped by destination, ascending inside a group); out [N,d_mid].
 * E = 0, for every tensor-product entry point of this section: the per-edge arrays may be NULL; the calls with a per-node output
 * (out, g_x) run and give every node the result of a node without edges -- out and a stored g_x are written as zeros, an
 * accumulated g_x keeps the caller's zero-fill -- while the calls whose outputs are all per edge (e3k_tp_bwd_w, e3k_tp_bwd_w_ordered,
 * e3k_tp_bwd_e_table, e3k_tp_bwd_w_dual) launch nothing, write nothing and return E3K_OK before they look at the plan: also for a
 * plan they would otherwise refuse with E3K_ERR_UNSUPPORTED.  N = 0 returns E3K_OK likewise. */
int e3k_tp_fwd(const e3k_tp_plan* plan, const float* x, const float* sh, const float* w, const int32_t* src,
               const int32_t* dst_ptr, const int32_t* dst_perm, int64_t N, int64_t E, float* out, void* stream);
/* g_w [E,w_numel] written (may be NULL when only g_sh is wanted); g_sh [E,d_sh] accumulated with atomics when
 * non-null (needs w). */
int e3k_tp_bwd_w(const e3k_tp_plan* plan, const float* x, const float* sh, const float* w, const float* g_out,
                 const int32_t* src, const int32_t* dst_ptr, const int32_t* dst_perm, int64_t N, int64_t E,
                 float* g_w, float* g_sh, void* stream);
/* e3k_tp_bwd_w with g_sh (required; needs w) summed in a FIXED order, bit-reproducible run to run: every (node, group) work item
 * stores its share of an edge's g_sh into its own slice of e_partials [n_gc, E, d_sh], which the CALLER ZERO-FILLS
 * (e3k_tp_edge_partials_floats(plan, E) floats: a group writes only the degrees it reads), and the slices are added in item order
 * into g_sh [E,d_sh], which is overwritten.  g_w as above (may be NULL).  The likelihood's vector-Jacobian products use it
 * (ops.ordered_edge_gradients()). */
int e3k_tp_bwd_w_ordered(const e3k_tp_plan* plan, const float* x, const float* sh, const float* w, const float* g_out,
                         const int32_t* src, const int32_t* dst_ptr, const int32_t* dst_perm, int64_t N, int64_t E,
                         float* g_w, float* g_sh, float* e_partials, void* stream);
/* g_x [N,d_in]: the CALLER ZERO-FILLS it; plans whose groups are walked by two waves (l_max = 3: more than 24
 * accumulators per group) add their two partial sums with atomics (order independent), the others store.
 * CSR by source (src_ptr, src_perm), dst [E]. */
/* 1 when e3k_tp_bwd_x stores every element of g_x (no zero-fill needed): single-wave groups that tile [0, d_in). */
int e3k_tp_bwd_x_overwrites(const e3k_tp_plan* plan);
/* The kernel instantiation of the calling thread's most recent tensor-product launch, e.g. "tp_bwd_x_kernel<2, 3, true, true, 5>"
 * (template arguments as in e3k_tp.hip), or NULL before the first.  For tests: which form a plan and a call kind reached.  The
 * string stays valid until the thread's next call of this function. */
const char* e3k_tp_last_route(void);

/* The forward and the node-feature backward with the per-edge path weights interpolated INSIDE the kernel from the radial
 * knot table (the weights `self.fc(edge_radial)` of nn/message_passing.py:93, never materialised as [E, W]):
 * T [K + 1, W] = the radial MLP on the knots, bin [E] = each edge's knot i (stencil rows i - 1 .. i + 2), coef [E, 4] = its
 * four interpolation weights (e3k_rtable_bins).
 * Same results as e3k_rtable_interp_fwd followed by e3k_tp_fwd / e3k_tp_bwd_x (same interpolation arithmetic).
 * e3k_tp_table_supported: 1 when the plan has this form (channel-complete plans: every group a multiple of 64 channels with
 * all its degree slots present -- the inner layers of every shipped model), else the two entry points return
 * E3K_ERR_UNSUPPORTED. */
int e3k_tp_table_supported(const e3k_tp_plan* plan);
int e3k_tp_fwd_table(const e3k_tp_plan* plan, const float* x, const float* sh, const float* T, const int32_t* bin,
                     const float* coef, const int32_t* src, const int32_t* dst_ptr, const int32_t* dst_perm, int64_t N, int64_t E,
                     float* out, void* stream);
int e3k_tp_bwd_x_table(const e3k_tp_plan* plan, const float* sh, const float* T, const int32_t* bin, const float* coef,
                       const float* g_out, const int32_t* dst, const int32_t* src_ptr, const int32_t* src_perm, int64_t N,
                       int64_t E, float* g_x, void* stream);
/* ... and from the PACKED table P [K + 1, 3 W] (e3k_rtable_pack) -- same plans, same results up to the fp16 rounding stated there --
 * walking EDGE RECORDS (e3k_edge_records): erec_dst over the destination CSR (dst_perm, src), erec_src over the source CSR
 * (src_perm, dst); each [E, 16] int32, 64-byte aligned. */
int e3k_tp_fwd_ptable(const e3k_tp_plan* plan, const float* x, const void* P, const int32_t* erec_dst, const int32_t* dst_ptr,
                      int64_t N, int64_t E, float* out, void* stream);
int e3k_tp_bwd_x_ptable(const e3k_tp_plan* plan, const void* P, const int32_t* erec_src, const float* g_out, const int32_t* src_ptr,
                        int64_t N, int64_t E, float* g_x, void* stream);
/* ... the input gradient AND every edge's weight gradient in the one walk (replaces e3k_tp_bwd_x_ptable + e3k_tp_bwd_w of a layer's
 * backward, nn/message_passing.py:93,104-109 under autograd): x [N, d_in] channel-fastest = the layer's tensor-product input rows,
 * g_w [E, W] row e = d F / d w[e] (written once each: no zero-fill).  g_x carries the bits of e3k_tp_bwd_x_ptable. */
int e3k_tp_bwd_xw_ptable(const e3k_tp_plan* plan, const float* x, const void* P, const int32_t* erec_src, const float* g_out,
                         const int32_t* src_ptr, int64_t N, int64_t E, float* g_x, float* g_w, void* stream);
/* ... and for plans whose every group enables exactly the slot (l2 = l1, l3 = 0), l1 <= 2, groups of a multiple of 64 channels on
 * distinct input blocks, d_sh = 9 (e3k_tp_scalar_supported; else E3K_ERR_UNSUPPORTED, nothing written) -- what is left of a layer's
 * product when only the 0e block of its output carries a gradient (the last convolution in front of an o3.Linear to 1x0e,
 * nn/message_passing.py:104-109 under autograd) -- csrc/e3k_tp_scalar.hip:
 *   g_x[s, x_off + i mul + u] = sum_{e: src(e) = s} coeff w[e, u] C_ii0 sh[e, i] g_out[dst(e), out_off + u]     (the groups' blocks only:
 *                                                                         the caller zero-fills what no group owns)
 *   g_w[e, w_off + u]         = coeff g_out[dst(e), out_off + u] sum_i C_ii0 x[s, x_off + i mul + u] sh[e, i]   (g_w [E, plan w_numel])
 * The plan numbers its weight columns compactly (w_off, w_numel); the packed table may be a wider layer's: P [K + 1, 3 table_w] with
 * group i's column at table_off[i] (HOST array, n_groups entries).  table_off = NULL, table_w = 0: the table has the plan's own
 * columns.  Of g_out only the columns out_off .. out_off + mul of the groups are read.  Same bits as e3k_tp_bwd_xw_ptable gives for
 * these slots on a dense plan when the rest of g_out is zero. */
int e3k_tp_scalar_supported(const e3k_tp_plan* plan);
int e3k_tp_bwd_xw_scalar_ptable(const e3k_tp_plan* plan, const float* x, const void* P, int32_t table_w, const int32_t* table_off,
                                const int32_t* erec_src, const float* g_out, const int32_t* src_ptr, int64_t N, int64_t E, float* g_x,
                                float* g_w, void* stream);
/* ... and for plans that keep SOME slots of their groups (e3k_tp_masked_supported: at most 8 groups of a multiple of 64 channels,
 * l1 <= 2, enabled slots with l3 <= 2, not split, d_sh = 9; else E3K_ERR_UNSUPPORTED, nothing written) -- what is left of a layer's
 * product when the gradient of its output is zero outside some blocks -- csrc/e3k_tp_masked.hip.  The sums of e3k_tp_bwd_xw_ptable
 * over the enabled slots only, in its order: g_x (the groups' blocks only: the caller zero-fills what no group owns, and all of it
 * when two groups share an input block) and the enabled slots' columns of g_w [E, plan w_numel] carry the bits it gives on the
 * dense plan when the other slots' rows of g_out are zero.  The plan numbers its weight columns compactly; the packed table may be
 * a wider layer's: P [K + 1, 3 table_w] with the column of the k-th enabled slot, counted in (group, slot) order, at live_col[k]
 * (HOST array).  live_col = NULL, table_w = 0: the table has the plan's own columns.  Of g_out only the enabled slots' rows are
 * read. */
int e3k_tp_masked_supported(const e3k_tp_plan* plan);
int e3k_tp_bwd_xw_masked_ptable(const e3k_tp_plan* plan, const float* x, const void* P, int32_t table_w, const int32_t* live_col,
                                const int32_t* erec_src, const float* g_out, const int32_t* src_ptr, int64_t N, int64_t E, float* g_x,
                                float* g_w, void* stream);
/* dst [rows, w_dst] = 0, except dst[r, dst_col[k] + c] = src[r, src_col[k] + c] for c < len[k], k < n_ranges <= 48 (HOST arrays;
 * columns, widths and lengths multiples of 4, src and dst 16-byte aligned, the ranges of dst disjoint): a compact knot-table
 * gradient spread over the dense table's columns.  One launch, every element of dst written. */
int e3k_expand_columns(const float* src, int64_t rows, int32_t w_src, int32_t w_dst, const int32_t* src_col, const int32_t* dst_col,
                       const int32_t* len, int32_t n_ranges, float* dst, void* stream);
/* ... the same pair of gradients with the weights streamed from w [E, W] (every plan): replaces e3k_tp_bwd_x + e3k_tp_bwd_w where
 * both are wanted (layers whose radial MLP runs per edge; force training's materialised rows). */
int e3k_tp_bwd_xw(const e3k_tp_plan* plan, const float* x, const float* sh, const float* w, const float* g_out, const int32_t* dst,
                  const int32_t* src_ptr, const int32_t* src_perm, int64_t N, int64_t E, float* g_x, float* g_w, void* stream);
/* Force training on the table (GradientOutput: nn/output.py:31-53 with create_graph = self.training; the per-edge weights
 * then depend on pos through the radius, nn/message_passing.py:93).  With F = <g, TP(x[src], sh, w(T, coef))>, linear in each
 * of (g, x, sh, T, coef), every first and second derivative is one of the walks below (plans with e3k_tp_table2_supported:
 * channel-complete, one wave per group -- the l_max <= 2 models):
 * D [K + 1, W] is the SLOPE table dT/dr on the knots (e3k_radial_slope_fwd), interpolated with the same weights:
 * dw/dr[e] = sum_k coef[e,k] D[bin[e] - 1 + k]  (differentiating the weights instead would amplify the table's fp32 rounding by
 * 1 / knot spacing: measured 7e-6 .. 4e-5 relative slope error at any knot count, against 5e-8 this way).
 *   e3k_tp_bwd_e_table      g_sh [E, d_sh] = dF/dsh, g_r [E] = <dF/dw, dw/dr> (either may be NULL), g_w [E, W] = dF/dw written when
 *                           non-null -- the first backward of a force evaluation.  A work item (node, group) holds only its group's
 *                           share of an edge's sum: with e_partials (e3k_tp_edge_partials_floats(plan, E) floats of scratch) every
 *                           item STORES its share into its own slice and a second launch adds the slices in item order into g_sh /
 *                           g_r (overwritten: no zero fill, bit-reproducible -- round 6); with e_partials = NULL the shares are
 *                           float atomics onto g_sh / g_r, which the caller zero-fills (not reproducible run to run)
 *   e3k_tp_fwd_jvp_table    out = TP(x2, sh, w) + TP(x, sh2, w) + TP(x, sh, s2 * dw/dr)          (s2 [E]: the radius' partner)
 *   e3k_tp_bwd_x_dual_table g_x = dF/dx at (sh2, w) + dF/dx at (sh, s2 * dw/dr)
 *   e3k_tp_bwd_w_dual       g_w = dF/dw at (x2, sh) + dF/dw at (x, sh2)           (w is the open slot: no table involved)
 * With bin = coef = NULL the first three take w and dw/dr MATERIALISED: T = w [E, W], D = dw/dr [E, W] (e3k_rtable_interp_fwd of
 * either table): five or six kernels per layer read them, and one 7.7 KB row per edge is a quarter of four table rows. */
int e3k_tp_table2_supported(const e3k_tp_plan* plan);
/* ... and with the weights and their slope passed MATERIALISED (bin = coef = NULL): every channel-complete plan, the l_max 3 ones
 * (two waves per group) included */
int e3k_tp_second_order_streamed_supported(const e3k_tp_plan* plan);
int e3k_tp_bwd_e_table(const e3k_tp_plan* plan, const float* x, const float* sh, const float* T, const float* D,
                       const int32_t* bin, const float* coef, const float* g_out, const int32_t* src, const int32_t* dst_ptr,
                       const int32_t* dst_perm, int64_t N, int64_t E, float* g_sh, float* g_r, float* g_w, float* e_partials,
                       void* stream);
int64_t e3k_tp_edge_partials_floats(const e3k_tp_plan* plan, int64_t E);
int e3k_tp_fwd_jvp_table(const e3k_tp_plan* plan, const float* x, const float* x2, const float* sh, const float* sh2,
                         const float* T, const float* D, const int32_t* bin, const float* coef, const float* s2,
                         const int32_t* src, const int32_t* dst_ptr, const int32_t* dst_perm, int64_t N, int64_t E, float* out,
                         void* stream);
int e3k_tp_bwd_x_dual_table(const e3k_tp_plan* plan, const float* sh, const float* sh2, const float* T, const float* D,
                            const int32_t* bin, const float* coef, const float* s2, const float* g_out, const int32_t* dst,
                            const int32_t* src_ptr, const int32_t* src_perm, int64_t N, int64_t E, float* g_x, void* stream);
/* The first backward of a force evaluation w.r.t. everything an edge touches, in ONE walk of the source CSR (streamed rows w,
 * dw [E, W]): g_x (e3k_tp_bwd_x), g_sh [E, d_sh] and g_r [E] (as e3k_tp_bwd_e_table, e_partials included; either may be NULL, not
 * both) and, when g_w != NULL, the per-edge weight gradient (e3k_tp_bwd_w).  Channel-complete plans. */
int e3k_tp_bwd_xe(const e3k_tp_plan* plan, const float* x, const float* sh, const float* w, const float* dw, const float* g_out,
                  const int32_t* dst, const int32_t* src_ptr, const int32_t* src_perm, int64_t N, int64_t E, float* g_x, float* g_sh,
                  float* g_r, float* g_w, float* e_partials, void* stream);
/* e3k_tp_bwd_x_dual_table on streamed rows (w, dw [E, W]; bin = coef = NULL there) that ALSO writes the weight gradients sharing its
 * per-edge sums: g_w = e3k_tp_bwd_w_dual's, g_w_plain (may be NULL) = e3k_tp_bwd_w's -- one walk instead of three (the u-sweep of
 * force training: the adjoint of nn/output.py:42-50's first backward) */
int e3k_tp_bwd_xw_dual(const e3k_tp_plan* plan, const float* x, const float* x2, const float* sh, const float* sh2, const float* w,
                       const float* dw, const float* s2, const float* g_out, const int32_t* dst, const int32_t* src_ptr,
                       const int32_t* src_perm, int64_t N, int64_t E, float* g_x, float* g_w, float* g_w_plain, void* stream);
int e3k_tp_bwd_w_dual(const e3k_tp_plan* plan, const float* x, const float* x2, const float* sh, const float* sh2,
                      const float* g_out, const int32_t* src, const int32_t* dst_ptr, const int32_t* dst_perm, int64_t N, int64_t E,
                      float* g_w, void* stream);
int e3k_tp_bwd_x(const e3k_tp_plan* plan, const float* sh, const float* w, const float* g_out, const int32_t* dst,
                 const int32_t* src_ptr, const int32_t* src_perm, int64_t N, int64_t E, float* g_x, void* stream);

/* ------------------------------------------------------------------------------------------
 * Per-batch graph topology (csrc/e3k_graph.hip).
 * Replaces what the reference leaves to scatter(ef, edge_dst) (nn/message_passing.py:109) and Batch's segment
 * bookkeeping (data/batch.py:164-178): from edge_index int64 [2,E] (row 0 sources, row 1 destinations) builds
 *   src, dst [E] int32; dst_ptr/src_ptr [N+1] row pointers; dst_perm/src_perm [E] edge ids grouped by endpoint,
 *   ASCENDING inside a row (= a stable sort by endpoint, the reference's CPU summation order);
 * workspace: e3k_csr_workspace_ints(N, E) int32.  bad_flag [1]: set to 1 when an endpoint is outside [0, N)
 * (such edges are attached to node 0 and counted there, so the lists stay complete: every edge id appears exactly once in
 * each perm and every element of every output is written -- the result is that of the edge list with each such edge replaced
 * by (0, 0); the caller reads the flag when it chooses to).  N = 0 with E > 0 (no node 0 to attach to): E3K_ERR_INVALID.
 * ------------------------------------------------------------------------------------------ */
int64_t e3k_csr_workspace_ints(int64_t N, int64_t E);
int e3k_csr_build(const int64_t* edge_index, int64_t N, int64_t E, int32_t* src, int32_t* dst, int32_t* dst_ptr,
                  int32_t* dst_perm, int32_t* src_ptr, int32_t* src_perm, int32_t* workspace, int32_t* bad_flag,
                  void* stream);

/* Edge records: what a tensor-product kernel needs about the t-th edge of a CSR walk (perm [E]: the walk's edge ids, nbr [E]: the
 * neighbour node of an edge -- src for the destination CSR, dst for the source CSR) as ONE 64-byte block per edge, in walk order:
 *   rec[t] = { nbr[e], bin[e], coef[e, 0..3], sh[e, 0..8], e },  e = perm[t]        (bin / coef NULL: zeros; d_sh < 9: zero padded)
 * replacing the chain perm[t] -> e -> {nbr, bin, coef, sh}[e] of dependent scalar loads in front of every edge's row loads
 * (reference: what `x[edge_src]`, `edge_spherical[e]`, `weight[e]` index, nn/message_passing.py:96-109).  rec: 64-byte aligned.
 * E < 2^31 - 1 (perm holds int32 edge ids): E3K_ERR_UNSUPPORTED beyond. */
int e3k_edge_records(const int32_t* perm, const int32_t* nbr, const int32_t* bin, const float* coef, const float* sh, int32_t d_sh,
                     int64_t E, int32_t* rec, void* stream);

/* Rows grouped by a small categorical key (the keyed self-connection groups nodes by species: node_attrs =
 * Linear(one_hot(species)), layer_configs.py:104-118 feeding nn/message_passing.py:81-87,100): perm [R] int32 = row ids
 * sorted by key, stable; bounds [K,2] int32 = {start, count} per key; reps [K] int64 = first row of each key (0 for an
 * absent key).  K <= 256.  bad_flag [1]: set when a key is outside [0, K); such rows are left out of bounds and reps, perm holds
 * the remaining rows in its first sum(count) elements and the rest of perm is not written (read perm through bounds only). */
int e3k_group_rows(const int64_t* key, int64_t R, int32_t K, int32_t* perm, int32_t* bounds, int64_t* reps,
                   int32_t* bad_flag, void* stream);

/* ------------------------------------------------------------------------------------------
 * Padded collation on the device (csrc/e3k_collate.hip; data/device_store.py).
 * Replaces, per batch, the reference's collate (Batch.from_data_list over Data objects, e3_layers/data/dataloader.py:30-45)
 * followed by run/graph_step.pad_batch: G graphs chosen by `ids` are gathered from a device-resident store (graph s owns node
 * rows [node_off[s], node_off[s+1]) and edge rows [edge_off[s], edge_off[s+1]), edge_index sample-local int32 [2, E_store])
 * and padded with ONE ghost graph to exactly n_cap nodes and e_cap edges -- bit for bit what pad_batch(store.index_select(ids),
 * n_cap, e_cap) builds on the host.  Two launches, fixed shapes per (G, n_cap, e_cap), no host read-back, no memset:
 *   e3k_collate_plan    one workgroup (G <= 1024): exclusive scans of the chosen graphs' counts into `work`
 *                       (e3k_collate_work_ints(G) int64), n_nodes / n_edges [G+1] (the ghost's last), graph_weight [G+1]
 *                       (1/G, ghost 0).  An id outside [0, S), n + 2 > n_cap or e > e_cap ORs bit 4 (16) into *flag (a
 *                       persistent flag: never cleared here) and collates the batch as G EMPTY graphs plus a ghost that fills
 *                       the capacities -- nothing is read through a bad id, nothing is written past a capacity.
 *   e3k_collate_gather  one wave per (graph slot, field): the fields below, ghost rows included.
 * ------------------------------------------------------------------------------------------ */
#define E3K_COLLATE_NODE 0         /* row copy: node rows (ghost: see `ghost`) */
#define E3K_COLLATE_EDGE 1         /* row copy: edge rows (ghost: see `ghost`) */
#define E3K_COLLATE_GRAPH 2        /* row copy: one row per graph (ghost: zeros) */
#define E3K_COLLATE_EDGE_INDEX 3   /* src int32 [2, src_ld] sample-local -> dst int64 [2, dst_ld] + the graph's first node */
#define E3K_COLLATE_NODE_SEGMENT 4 /* dst int64 [n_cap]: graph slot of every node */
#define E3K_COLLATE_EDGE_SEGMENT 5 /* dst int64 [e_cap]: graph slot of every edge */
#define E3K_COLLATE_NODE_WEIGHT 6  /* dst float [n_cap]: (float)(1.0 / n) on the real nodes, 0 on the ghost's */
#define E3K_COLLATE_GHOST_FIRST 0  /* ghost rows = the first real graph's first row (zeros when it has none) */
#define E3K_COLLATE_GHOST_TABLE 1  /* ghost row k = row k of `table` (>= n_cap rows; ghost positions) */
#define E3K_COLLATE_MAX_FIELDS 16
typedef struct {
  int32_t kind;       /* E3K_COLLATE_* */
  int32_t ghost;      /* node / edge rows: E3K_COLLATE_GHOST_* */
  int64_t row_bytes;  /* row copies: bytes per row, a multiple of 4 */
  const void* src;    /* the store's tensor (row copies, edge_index) */
  void* dst;          /* the batch's tensor */
  const void* table;  /* E3K_COLLATE_GHOST_TABLE */
  int64_t src_ld;     /* edge_index: elements between the store's two rows (E_store) */
  int64_t dst_ld;     /* edge_index: elements between the batch's two rows (e_cap) */
} e3k_collate_field;
int64_t e3k_collate_work_ints(int32_t G);
int e3k_collate_plan(const int32_t* ids, int32_t G, const int64_t* node_off, const int64_t* edge_off, int64_t S, int64_t n_cap,
                     int64_t e_cap, int64_t* work, int64_t* n_nodes, int64_t* n_edges, float* graph_weight, int32_t* flag,
                     void* stream);
int e3k_collate_gather(const e3k_collate_field* fields, int32_t n_fields, int32_t G, int64_t n_cap, int64_t e_cap,
                       const int64_t* work, void* stream);

/* ------------------------------------------------------------------------------------------
 * Radial weights through a knot table (csrc/e3k_rtable.hip).
 * Replaces weight = fc(edge_radial) (nn/message_passing.py:74-79,93) evaluated per edge when edge_radial is
 * RadialBasisEncoding(edge_length) (nn/embedding.py:210-219): the MLP is evaluated on the K + 1 knots j * r_max / K
 * (T [K+1, W], by the caller, with the same kernels) and every edge interpolates the FOUR knots around it (cubic Lagrange
 * weights: error 3/128 h^4 max|d4f|; ~1e-7 relative at K = 512 for the shipped models, the fp32 rounding of the table).
 *   e3k_rtable_bins       r [E], h_inv = 1 / knot spacing (a power of two makes r / h and the offsets exact; the knots are then
 *                         exactly representable too) -> bin [E] (knot i = floor(r / h) clamped to [1, K - 2]; stencil rows
 *                         i - 1 .. i + 2),
 *                         coef [E, 4] (the four weights), and the edges grouped
 *                         by knot with a STABLE counting sort: bin_ptr [K + 2], bin_perm [E] (ascending edge id inside a knot),
 *                         bin_seg [K + 2] (first segment of <= 64 edges of every knot: the transpose's work list).
 *                         workspace: e3k_rtable_bins_workspace_ints(E, K) int32.  Three launches, no atomics, no sort.
 *   e3k_rtable_interp_fwd w[e,:] = sum_k coef[e,k] T[bin[e] - 1 + k,:]     (edges visited in knot order, bin_perm, so that
 *                         neighbouring waves share table rows)
 *   e3k_rtable_interp_bwd g_T[j,:] (+)= sum over the edges whose stencil holds row j of their weight for it (times scale[e] when
 *                         scale is given) times g_w[e,:]; every row written; no atomics: per-segment partial sums in the
 *                         workspace, then a fixed-order combination (bit-identical run to run).
 * W must be a multiple of 4 (else E3K_ERR_UNSUPPORTED).  E < 2^31 - 1 everywhere (bin_perm holds int32 edge ids), at most 4 001
 * table rows for e3k_rtable_bins / _keyed: E3K_ERR_UNSUPPORTED beyond.
 * ------------------------------------------------------------------------------------------ */
int64_t e3k_rtable_bins_workspace_ints(int64_t E, int32_t K);
int e3k_rtable_bins(const float* r, int64_t E, float h_inv, int32_t K, int32_t* bin, float* coef,
                    int32_t* bin_ptr, int32_t* bin_seg, int32_t* bin_perm, int32_t* workspace, void* stream);
/* KEYED tables: the edge embedding is a function of the radius and of a small categorical key per edge (config_diffusion.py:73-82:
 * the Bessel basis concatenated with a 4-way bond-type one-hot) -- n_keys tables of K + 1 rows stacked into one of n_keys (K + 1)
 * rows, bin[e] = key[e] (K + 1) + i.  bin_ptr / bin_seg [n_keys (K + 1) + 1]; workspace e3k_rtable_bins_workspace_ints(E,
 * n_keys (K + 1) - 1).  Every consumer takes the stacked table with K := n_keys (K + 1) - 1.
 * bad_flag (may be NULL): bit 3 is ORed in when a key lies outside [0, n_keys) (such an edge interpolates in block 0); the flag is
 * never cleared here, so it may be a persistent one shared with other checks (e3k_flag_fetch_clear hands it to the host). */
int e3k_rtable_bins_keyed(const float* r, const int64_t* key, int32_t n_keys, int64_t E, float h_inv, int32_t K, int32_t* bin,
                          float* coef, int32_t* bin_ptr, int32_t* bin_seg, int32_t* bin_perm, int32_t* workspace, int32_t* bad_flag,
                          void* stream);
int e3k_rtable_interp_fwd(const float* T, const int32_t* bin_perm, const int32_t* bin, const float* coef, int64_t E, int32_t K,
                          int32_t W, float* w, void* stream);
/* two tables of one shape through the same weights in one pass (force training: w from T and dw/dr from the slope table) */
int e3k_rtable_interp_fwd2(const float* T, const float* T2, const int32_t* bin_perm, const int32_t* bin, const float* coef, int64_t E,
                           int32_t K, int32_t W, float* w, float* w2, void* stream);
/* workspace: e3k_rtable_bwd_workspace_floats(E, K, W) floats (per-segment partial sums, combined in a fixed order) */
int64_t e3k_rtable_bwd_workspace_floats(int64_t E, int32_t K, int32_t W);
int e3k_rtable_interp_bwd(const float* g_w, const float* coef, const float* scale, const int32_t* bin_ptr,
                          const int32_t* bin_seg, const int32_t* bin_perm, int64_t E, int32_t K, int32_t W, float* workspace,
                          float* g_T, int32_t accumulate, void* stream);
/* e3k_gemm_multi(segments, n_segments, wgrad = 1, stream) and e3k_rtable_interp_bwd(g_w .. accumulate, stream) as ONE call: the
 * weight-gradient problems of the pipelined kernel (16-byte-loadable operands, not the outer-product form) and the transpose's first
 * pass go out as one launch, gemm_wgrad2_with_table_bwd_kernel -- the GEMM's workgroups first, the transpose's behind them --, then
 * the transpose's second pass.  Same results: g_T bit for bit, the weight gradients up to the order of their fp32 atomics.  Every
 * argument error of either call is refused before anything is launched.  Without such a problem, or with E = 0, the two calls are
 * made one after the other.  e3k_gemm_last_routes() reports the GEMM side's launches. */
int e3k_wgrad_with_table_bwd(const e3k_gemm_segment* segments, int32_t n_segments, const float* g_w, const float* coef,
                             const float* scale, const int32_t* bin_ptr, const int32_t* bin_seg, const int32_t* bin_perm, int64_t E,
                             int32_t K, int32_t W, float* workspace, float* g_T, int32_t accumulate, void* stream);

/* The table packed for the tensor-product kernels: 12 bytes per (knot, weight) in ONE row -- the cubic through rows i-1 .. i+2 as
 * its Taylor polynomial about the middle of knot interval i, {d0: f32, d1: f32, d2 * 2^10: f16, d3 * 2^16: f16} -- instead of four
 * 4-byte values in four rows 4 W bytes apart: e3k_tp_fwd_ptable / e3k_tp_bwd_x_ptable read one dwordx2 and one dword per path slot
 * and edge (23 instead of 31 KB of table per edge through L1).  P [K + 1, 3 W] dwords: a row = its W (d0, d1) pairs, then its W
 * f16 pairs.  Same function as the four-row form up to the fp16
 * rounding of the two small coefficients (economised into the fp32 pair: <= 2^-11 (|d2| / 8 + |d3| / 32), ~6e-8 of the values on
 * 512 knots).
 * e3k_rtable_interp_packed materialises w[e, :] from P with the kernels' own arithmetic (bit-identical; tests). */
int e3k_rtable_pack(const float* T, int32_t K, int32_t W, void* P, void* stream);
/* ... n <= 16 tables of one row count (the layers of a radial stack) in ONE launch; the same bits as n e3k_rtable_pack calls */
int e3k_rtable_pack_multi(const float* const* T, int32_t K, const int32_t* W, void* const* P, int32_t n, void* stream);
int e3k_rtable_interp_packed(const void* P, const int32_t* bin_perm, const int32_t* bin, const float* coef, int64_t E, int32_t K,
                             int32_t W, float* w, void* stream);

/* A-posteriori bound of the table's interpolation error, evaluated ON THE DEVICE (the reference evaluates fc(edge_radial)
 * exactly on every edge, nn/message_passing.py:74-79,93: the table must know when it stops being a stand-in).  With
 * err_c = 3/128 max_i |4th difference of T[:, c] at i| (cubic Lagrange on the table's knots; packed != 0: plus the fp16 rounding of
 * the packed table's two small coefficients, 2^-11 (|2nd difference| / 16 + |3rd difference| / 192)):
 *     table-wide ratio  est_g = max_c err_c / max |T|
 *     per-column ratio  est_c = max_c err_c / max(max_i |T[i, c]|, floor_rel * max |T|)
 *     reported          est   = max(est_g, col_weight * est_c)        (col_weight = table-wide tolerance / per-column tolerance)
 * for up to 16 tables of `rows` rows in ONE launch (the layers of a radial stack).  states[t] float [4]: [0] running maximum of
 * est since the caller last zeroed it (atomic max: survives HIP-graph replays, which never re-enter the host code that would
 * read a per-launch value), [1] est of this launch, [2] unused (never read or written), [3] est_c of this launch.
 * scratch[t] float [16 * widths[t]].  A non-finite table entry gives +inf in [0], [1] and [3].  rows < 5: nothing to do, nothing
 * written. */
int e3k_rtable_guard(const float* const* tables, float* const* states, float* const* scratch, const int32_t* widths, int32_t n,
                     int32_t rows, float floor_rel, float col_weight, int32_t packed, void* stream);

/* ------------------------------------------------------------------------------------------
 * Node-side elementwise kernels.
 * ------------------------------------------------------------------------------------------ */
/* activation ids: 0 identity, 1 ssp, 2 silu, 3 tanhlu, 4 tanh, 5 abs */
int e3k_act_fwd(const float* x, int64_t n, int32_t act, float cst, float* y, void* stream);
int e3k_act_bwd(const float* x, const float* g_y, int64_t n, int32_t act, float cst, float* g_x, void* stream);
/* same derivative from the OUTPUT y = cst*act(x) (act = 1 ssp only: cst*sigmoid(x) = cst*(1 - 0.5*exp(-y/cst))),
 * so a fused linear+activation layer keeps only its output */
int e3k_act_bwd_from_output(const float* y, const float* g_y, int64_t n, int32_t act, float cst, float* g_x,
                            void* stream);
/* double backward (GradientOutput with create_graph=True, e3_layers/nn/output.py:42-50 — force training):
 * e3k_act_bwd computed g_x = g_y*cst*act'(x); given the cotangent g_hat of that g_x,
 *   g_gy = g_hat*cst*act'(x)   and   g_x = g_hat*g_y*cst*act''(x)   (either output may be NULL). */
int e3k_act_bwd2(const float* x, const float* g_y, const float* g_hat, int64_t n, int32_t act, float cst,
                 float* g_gy, float* g_x, void* stream);

/* layout change of a feature row: blocks (off, mul, dim=2l+1); to_cf=1: [mul][dim] -> [dim][mul]. */
typedef struct {
  int32_t off, mul, dim, _pad;
} e3k_block;
int e3k_relayout(const float* x, int64_t rows, int32_t row_dim, const e3k_block* blocks, int32_t n_blocks,
                 int32_t to_cf, float* y, void* stream);

/* Gate (e3nn.nn.Gate, nn/message_passing.py:195-205,249): input row in cf layout
 * [scalars | gates | gated blocks], output row in e3nn layout [act(scalars) | gated*act(gate)]. */
typedef struct {
  int32_t kind;    /* 0: scalar block with activation, 1: gated block */
  int32_t in_off;  /* offset of the block in the input row */
  int32_t gate_off;/* kind 1: offset of its gate scalars in the input row */
  int32_t out_off; /* offset in the output row */
  int32_t mul, dim;
  int32_t act;     /* activation of the scalars (kind 0) or of the gates (kind 1) */
  float cst;       /* its second-moment normalisation constant */
} e3k_gate_seg;
/* out_cf: layout of the OUTPUT row (y, g_y, g_y2, g_gy): 0 = e3nn blocks [mul][2l+1], 1 = channel-fastest [2l+1][mul]
 * (consecutive MessagePassing layers hand their features over in cf: no relayout between them).  The input row x is
 * always channel-fastest.  g_y2 (may be NULL): a second addend of the incoming gradient, summed inside the kernel. */
int e3k_gate_fwd(const float* x, int64_t rows, int32_t in_dim, int32_t out_dim, const e3k_gate_seg* segs,
                 int32_t n_segs, int32_t out_cf, float* y, void* stream);
int e3k_gate_bwd(const float* x, const float* g_y, const float* g_y2, int64_t rows, int32_t in_dim, int32_t out_dim,
                 const e3k_gate_seg* segs, int32_t n_segs, int32_t out_cf, float* g_x, void* stream);
/* Which kernel e3k_gate_fwd (backward = 0) / e3k_gate_bwd (backward = 1) picks for these segments when every base pointer is
 * 16-byte aligned: 1 = the 16-byte form (one segment per workgroup, four channels per lane), 0 = the scalar form.  The 16-byte
 * form needs offsets and channel counts that are multiples of four, gated blocks of dim 1, 3, 5 or 7, and segments that tile
 * the written row exactly.  Host only: nothing is launched. */
int e3k_gate_path(int32_t in_dim, int32_t out_dim, const e3k_gate_seg* segs, int32_t n_segs, int32_t backward);
/* double backward of the gate: g_hat [rows,in_dim] is the cotangent of e3k_gate_bwd's g_x;
 * g_gy [rows,out_dim] = (dy/dx) g_hat,  g_x [rows,in_dim] = d/dx <g_hat, gate_bwd(x, g_y)>  (either may be NULL). */
int e3k_gate_bwd2(const float* x, const float* g_y, const float* g_hat, int64_t rows, int32_t in_dim, int32_t out_dim,
                  const e3k_gate_seg* segs, int32_t n_segs, int32_t out_cf, float* g_gy, float* g_x, void* stream);

/* NormActivation (e3nn.nn.NormActivation as built at e3_layers/nn/message_passing.py:212-219; the 'norm'
 * nonlinearity_type of MessagePassing): per irrep channel n2 = max(sum_m x_m^2, epsilon^2), n = sqrt(n2),
 * y_m = x_m * act(n) / n (normalize = 1; normalize = 0: y_m = x_m * act(n); epsilon = 0: y_m = x_m * act(sum_m x_m^2), no
 * clamp).  Columns that no block covers come out ZERO in every output of the three functions (y; g_x; g_gy and g_x); input
 * channel-fastest [2l+1][mul], output e3nn layout [mul][2l+1] at the same offsets; act ids as e3k_act_fwd, raw
 * (no second-moment constant).  At most 16 blocks. */
int e3k_norm_act_fwd(const float* x, int64_t rows, int32_t row_dim, const e3k_block* blocks, int32_t n_blocks, int32_t act,
                     float epsilon, int32_t normalize, float* y, void* stream);
int e3k_norm_act_bwd(const float* x, const float* g_y, int64_t rows, int32_t row_dim, const e3k_block* blocks,
                     int32_t n_blocks, int32_t act, float epsilon, int32_t normalize, float* g_x, void* stream);
/* backward of e3k_norm_act_bwd (force training through a 'norm' nonlinearity: GradientOutput, create_graph=True): with the
 * cotangent h on g_x (layout of x), g_gy (layout of g_y) and g_x; either may be NULL. */
int e3k_norm_act_bwd2(const float* x, const float* g_y, const float* h, int64_t rows, int32_t row_dim, const e3k_block* blocks,
                      int32_t n_blocks, int32_t act, float epsilon, int32_t normalize, float* g_gy, float* g_x, void* stream);

/* per-irreps-block RMS normalisation (LayerNormalization, nn/pointwise.py:32-51), e3nn layout:
 *   inv_norm[r, k] = (sum_j x_j^2 / mul_k + 1e-6)^-1/2 over the mul_k * dim_k elements of block k,  y_j = x_j * inv_norm * std[k].
 * All three functions WRITE y / g_x / g_gy ON THE BLOCK COLUMNS ONLY: a column that no block covers is left as the caller
 * handed it over (the kernels walk blocks, one wave per row; a caller whose table has a gap zero-fills first).  At most 16
 * blocks.  e3k_layernorm_bwd: g_std [n_blocks] ACCUMULATED (caller zeroes). */
int e3k_layernorm_fwd(const float* x, int64_t rows, int32_t row_dim, const e3k_block* blocks, int32_t n_blocks,
                      const float* std, float* y, float* inv_norm, void* stream);
int e3k_layernorm_bwd(const float* x, const float* g_y, const float* inv_norm, int64_t rows, int32_t row_dim,
                      const e3k_block* blocks, int32_t n_blocks, const float* std, float* g_x, float* g_std,
                      void* stream);
/* double backward: h [rows,row_dim] is the cotangent of e3k_layernorm_bwd's g_x, h_std [n_blocks] that of its g_std (may
 * be NULL); g_gy, g_x [rows,row_dim] written on the block columns (the caller zero-fills uncovered columns), g_std
 * [n_blocks] ACCUMULATED (any of the three may be NULL). */
int e3k_layernorm_bwd2(const float* x, const float* g_y, const float* h, const float* h_std, const float* inv_norm,
                       int64_t rows, int32_t row_dim, const e3k_block* blocks, int32_t n_blocks, const float* std,
                       float* g_gy, float* g_x, float* g_std, void* stream);

/* segment sizes -> row pointers (what Pooling derives from the batch's per-graph node counts, nn/output.py:66-74):
 * ptr[0] = 0, ptr[s + 1] = counts[0] + .. + counts[s]; ptr has n_seg + 1 entries */
int e3k_counts_to_ptr(const int64_t* counts, int32_t n_seg, int32_t* ptr, void* stream);
/* one-hot rows of a type index (OneHotEncoding, nn/embedding.py:271-281: torch.nn.functional.one_hot(...).to(float)):
 * out [rows, num_types], out[r, t] = (idx[r] == t); an index outside [0, num_types) gives a zero row AND ORs bit 2 into
 * *bad_flag (may be NULL; never cleared here: the reference's one_hot raises on such an index) */
int e3k_onehot(const int64_t* idx, int64_t rows, int32_t num_types, float* out, int32_t* bad_flag, void* stream);
/* *host_out = *flag; *flag = 0 -- one launch, in stream order (host_out: pinned, device-visible host memory).  How a persistent
 * device error flag that kernels only ever OR into (captured index checks, the two above) reaches the host exactly once per
 * flagged batch. */
int e3k_flag_fetch_clear(int32_t* flag, int32_t* host_out, void* stream);
/* sorted-segment sum (Pooling, nn/output.py:66-74): out[s, :] = sum_{r in [ptr[s], ptr[s+1])} x[r, :] (* 1/count if mean) */
int e3k_segment_sum(const float* x, const int32_t* ptr, int64_t n_seg, int32_t dim, int32_t mean, float* out,
                    void* stream);

/* ------------------------------------------------------------------------------------------
 * Keyed self-connection weights (see e3k_gemm_grouped): rows of node_attrs that carry the same key share
 *     M[t, (j,u,w)] = sum_v a[t,v] * W_j[u,v,w]
 * with W_j the [U][V][Wout] weight block of instruction j of FullyConnectedTensorProduct(x, node_attrs)
 * (e3_layers/nn/message_passing.py:81-87, e3nn 'uvw' weight order) at element offset w_off of the flat weight,
 * and its U*Wout columns at m_off of M (columns packed in instruction order, row stride ld_m).
 * a [n_keys, V] (V <= 32; the keys are tiled 64 per workgroup, or 512 when the columns alone make 1024 or more workgroups).  backward: g_a [n_keys,V] ACCUMULATED (caller zeroes), g_W flat like W:
 * written (accumulate_w = 0) or added to (accumulate_w = 1); either may be NULL.  g_a needs a device `workspace` of
 * e3k_keyed_weights_bwd_workspace(...) floats (per-block partial sums, reduced by a second launch — same-address
 * atomics from every block serialise).  `instr` is a HOST array. */
typedef struct {
  int64_t w_off, m_off;
  int32_t u, w_out;
} e3k_kw_instr;
int e3k_keyed_weights_fwd(const float* a, const float* W, const e3k_kw_instr* instr, int32_t n_instr, int32_t n_keys,
                          int32_t V, int64_t ld_m, float* M, void* stream);
int64_t e3k_keyed_weights_bwd_workspace(const e3k_kw_instr* instr, int32_t n_instr, int32_t n_keys, int32_t V);
int e3k_keyed_weights_bwd(const float* a, const float* W, const float* g_M, const e3k_kw_instr* instr, int32_t n_instr,
                          int32_t n_keys, int32_t V, int64_t ld_m, float* g_a, float* g_W, int32_t accumulate_w,
                          float* workspace, void* stream);

/* The same for the self-connections of several layers that read the SAME attribute rows `a` (the convolutions of one network:
 * nn/message_passing.py:81-87 x layers), one launch per pass instead of one per layer.  e3k_kw_args: a layer's instruction
 * table in device memory, created once.  items[i].M: forward OUT [n_keys, ld_m_i]; backward IN (g_M of layer i).  g_W as in
 * e3k_keyed_weights_bwd, per item; g_a [n_keys, V] ACCUMULATED over all the layers (caller zeroes).  At most 8 layers. */
typedef struct e3k_kw_args e3k_kw_args;
int e3k_kw_args_create(const e3k_kw_instr* instr, int32_t n_instr, int32_t V, int64_t ld_m, e3k_kw_args** out);
void e3k_kw_args_destroy(e3k_kw_args* args);
typedef struct {
  const e3k_kw_args* args;
  const float* W;
  float* M;
  float* g_W;
  int32_t accumulate_w, _pad;
} e3k_kw_multi_item;
int e3k_keyed_weights_fwd_multi(const e3k_kw_multi_item* items, int32_t n, const float* a, int32_t n_keys, void* stream);
int64_t e3k_keyed_weights_bwd_multi_workspace(const e3k_kw_multi_item* items, int32_t n, int32_t n_keys);
int e3k_keyed_weights_bwd_multi(const e3k_kw_multi_item* items, int32_t n, const float* a, int32_t n_keys, float* g_a,
                                float* workspace, void* stream);

/* ------------------------------------------------------------------------------------------
 * Fused hidden chain of the radial MLP.
 * Replaces the hidden layers of e3nn.nn.FullyConnectedNet([n_radial, H, ..., H, weight_numel], act)
 * (e3_layers/nn/message_passing.py:74-79, call :93): per layer l < n_layers
 *     z_l = alphas[l] * (prev @ W_l),   h_l = cst * act(z_l),   prev = x for l = 0, else h_{l-1}
 * x [E,k0] (k0 <= 64), W_0 [k0,h], W_l [h,h] row-major, h in {32, 64}, n_layers <= 4; out = h_{n_layers-1} [E,h].
 * `weights`, `z`, `g_weights` are HOST arrays of n_layers device pointers.
 *   forward : z[l] [E,h] receive the pre-activations the backward needs (z or any z[l] may be NULL: inference).
 *   backward: g_out = gradient wrt out; g_weights[l] (same shapes as W_l) are ACCUMULATED with atomics
 *             (caller zeroes; NULL entries / NULL array are skipped); g_x [E,k0] written when not NULL. */
int e3k_mlp_hidden_fwd(const float* x, int64_t E, int32_t k0, int32_t h, int32_t n_layers, const float* const* weights,
                       const float* alphas, int32_t act, float cst, float* const* z, float* out, void* stream);
int e3k_mlp_hidden_bwd(const float* x, int64_t E, int32_t k0, int32_t h, int32_t n_layers, const float* const* weights,
                       const float* alphas, int32_t act, float cst, const float* const* z, const float* g_out,
                       float* const* g_weights, float* g_x, void* stream);
/* Rows per tile of the hidden chain for E rows and n_nets nets in one launch: 64, or 16 when the 64-row tiles of all the nets
 * would not give every compute unit a workgroup (the knot rows of the radial tables).  Host only: nothing is launched. */
int e3k_mlp_tile_rows(int64_t E, int32_t n_nets);

/* Several MLPs of ONE shape over the SAME input rows in one launch each way (the radial MLPs of all the layers of a
 * network read one edge embedding: nn/message_passing.py:74-79,93 per layer).  g_x is per net (the caller sums). */
typedef struct {
  const float* weights[4];
  float* z[4];            /* forward: pre-activations out (NULL entries: not kept); backward: in */
  float* out;             /* forward: [E, h] */
  const float* g_out;     /* backward: gradient w.r.t. out */
  float* g_weights[4];    /* backward: accumulated (NULL entries: skipped) */
  float* g_x;             /* backward: [E, k0] or NULL */
} e3k_mlp_net;
int e3k_mlp_hidden_fwd_multi(const e3k_mlp_net* nets, int32_t n_nets, const float* x, int64_t E, int32_t k0, int32_t h,
                             int32_t n_layers, const float* alphas, int32_t act, float cst, void* stream);
int e3k_mlp_hidden_bwd_multi(const e3k_mlp_net* nets, int32_t n_nets, const float* x, int64_t E, int32_t k0, int32_t h,
                             int32_t n_layers, const float* alphas, int32_t act, float cst, void* stream);

/* ------------------------------------------------------------------------------------------
 * Radius graph on the device.
 * Replaces computeEdgeIndex (e3_layers/data/compute_edge.py:38-113) for the criteria-free case: per graph all
 * ordered pairs (i, j), i != j, with fp32 sqrt(|pos_i - pos_j|^2) < r_max (strict), in the reference's order
 * (graphs concatenated, i slow, j fast); pre-existing edges (old_ptr [N+1] CSR by source with old_dst ascending
 * inside a row; NULL = none) are kept whatever their length.
 *   graph_start / graph_end [N]: first node / one-past-last node of the graph node i belongs to.
 *   pass 1 writes counts [N] (kept pairs per source); the caller scans them (exclusive, int64) into offsets [N];
 *   pass 2 writes edge_index int64 [2, E] (row 0 sources, row 1 destinations), E = total count. */
int e3k_radius_graph_count(const float* pos, const int32_t* graph_start, const int32_t* graph_end, int64_t N,
                           float r_max, const int32_t* old_ptr, const int32_t* old_dst, int32_t* counts, void* stream);
int e3k_radius_graph_fill(const float* pos, const int32_t* graph_start, const int32_t* graph_end, int64_t N,
                          float r_max, const int32_t* old_ptr, const int32_t* old_dst, const int64_t* offsets, int64_t E,
                          int64_t* edge_index, void* stream);

/* ------------------------------------------------------------------------------------------
 * Capped neighbour list (csrc/e3k_nlist.hip; the integrators further down: csrc/e3k_md.hip): the radius graph above into a
 * buffer of FIXED size, for loops that evaluate a model over and over while the atoms move inside one captured HIP graph.
 * Replaces computeEdgeIndex (e3_layers/data/compute_edge.py:38-113) where the sampling loop drops and rebuilds
 * edge_index after every update (e3_layers/run/sde_sampling.py:236-241) and where an MD driver (torchMD.ipynb) calls the
 * model on moved positions: same distance test, same edge order, no pre-existing edges, nothing read back by the host.
 * The batch is a padded one (run/graph_step.pad_batch): graphs 0 .. G-1 are real, graph G is the ghost graph and is not
 * searched.
 *   node_seg [N] int64: graph of every node; node_ptr [G + 2] int64: first node of every graph (node_ptr[G + 1] = N).
 *   e3k_nlist_count writes counts [N] (kept pairs per source node; 0 for ghost nodes).
 *   e3k_nlist_fill scans them on the device into offsets [N + 1] (workspace) and writes
 *     edge_index int64 [2, e_cap]: the E_real real edges, then in the slots [E_real, e_cap) ghost edge kk = k - E_real of
 *       run/graph_step.ghost_sample: (a, a + 1) + node_ptr[G], a = kk % (n_ghost - 1), endpoints swapped when
 *       kk / (n_ghost - 1) is odd -- for positions that fit, bit for bit pad_batch's edge_index of the rebuilt batch;
 *     n_edges [G + 1] int64 (ghost graph last), edge_segment [e_cap] int64 (NULL: not wanted), state[0] = E_real.
 *   Overflow (E_real > e_cap, or slots left over with fewer than two ghost nodes to take them): the real edges are cut
 *   at e_cap, every index written is a node of the batch, nothing is written outside the buffers; the value 32 (bit 5) is ORed into
 *   *flag (the device's persistent flag) and state[1] is incremented. */
int e3k_nlist_count(const float* pos, const int64_t* node_seg, const int64_t* node_ptr, int64_t N, int32_t G, float r_max,
                    int32_t* counts, void* stream);
int e3k_nlist_fill(const float* pos, const int64_t* node_seg, const int64_t* node_ptr, int64_t N, int32_t G, float r_max,
                   const int32_t* counts, int64_t e_cap, int64_t* offsets, int64_t* edge_index, int64_t* n_edges,
                   int64_t* edge_segment, int64_t* state, int32_t* flag, void* stream);

/* The same with a declarative pair criterion evaluated in the kernels (data/compute_edge.SequenceOrRandom).
 * Replaces the criteria callback of computeEdgeIndex (e3_layers/data/compute_edge.py:72-75) as the protein score nets use it
 * (e3_layers/configs/config_diffusion_CA.py:58-64: same chain and |i - j| < 5, or a 2 % random subset), which forces the
 * all-pairs candidate list and a host synchronisation per model call.  A pair (i, j), j != i, of one real graph is kept when
 *   |pos_i - pos_j| < r_max,  or  segment_key[i] == segment_key[j] and |i - j| < window,  or  hash(seed, draw, i, j) < threshold
 * with i, j the batch's global node indices; same edge order, buffers and overflow contract as above.
 *   segment_key [N] int64 (NULL or window 0: no sequence term); threshold = floor(p 2^32) (0: no random term); keep_all != 0:
 *   p = 1, every candidate pair is kept.  hash: the lowbias32 finaliser mix(h) = (h ^= h >> 16, h *= 0x7feb352d, h ^= h >> 15,
 *   h *= 0x846ca68b, h ^= h >> 16) chained as h = mix(h ^ word) over seed_lo, seed_hi, draw (low 32 bits), i, j from 0x9E3779B9.
 *   rng [2] int64 = (next draw index, draw index in use): e3k_nlist_count_crit draws with rng[0]; e3k_nlist_fill_crit's scan
 *   copies rng[0] to rng[1] and adds one to rng[0], its fill pass draws with rng[1] -- one draw per build, the index goes up once
 *   per build, nothing read by the host. */
int e3k_nlist_count_crit(const float* pos, const int64_t* node_seg, const int64_t* node_ptr, int64_t N, int32_t G, float r_max,
                         const int64_t* segment_key, int64_t window, uint32_t threshold, int32_t keep_all, uint32_t seed_lo,
                         uint32_t seed_hi, int64_t* rng, int32_t* counts, void* stream);
int e3k_nlist_fill_crit(const float* pos, const int64_t* node_seg, const int64_t* node_ptr, int64_t N, int32_t G, float r_max,
                        const int64_t* segment_key, int64_t window, uint32_t threshold, int32_t keep_all, uint32_t seed_lo,
                        uint32_t seed_hi, int64_t* rng, const int32_t* counts, int64_t e_cap, int64_t* offsets, int64_t* edge_index,
                        int64_t* n_edges, int64_t* edge_segment, int64_t* state, int32_t* flag, void* stream);

/* Velocity Verlet around a force evaluation (the integrator of torchMD.ipynb's driver) on the n real nodes of a padded
 * batch -- the ghost nodes behind them never move.  x, v, f [n, 3], mass [n].
 *   e3k_md_drift: v += dt/2 f / m;  x += dt v.
 *   e3k_md_kick : v += dt/2 f / m;  kinetic [G] = per-graph sum of m v^2 / 2 through node_ptr [G + 1] int64 (NULL: not
 *                 wanted).  One wave per graph, fixed summation order, no atomics: the same bits every run.
 *                 potential [G] (NULL: not wanted) = energy [G], the force evaluation's static output, kept for the step's
 *                 record in the same launch. */
int e3k_md_drift(float* x, float* v, const float* f, const float* mass, int64_t n, float dt, void* stream);
int e3k_md_kick(float* v, const float* f, const float* mass, const int64_t* node_ptr, int32_t G, int64_t n, float dt,
                float* kinetic, const float* energy, float* potential, void* stream);

/* The thermostatted second half step (the Langevin integrator of torchMD.ipynb's driver: Integrator(..., gamma, T)) and the
 * Maxwell-Boltzmann draw (its maxwell_boltzmann), in e3k_md_kick's walk with e3k_md_kick's records:
 *   v <- c v + (s / sqrt(m)) xi;   v <- v + dt/2 f / m  (f NULL: skipped);   kinetic, potential as e3k_md_kick files them.
 * c = exp(-gamma dt), s = sqrt((1 - c^2) kT) (the caller forms them in float64): the exact Ornstein-Uhlenbeck step, stable for any
 * gamma dt; c = 1, s = 0 is e3k_md_kick bit for bit; c = 0, s = sqrt(kT), f = NULL draws Maxwell-Boltzmann velocities.
 * xi: a counter-based standard normal, the same bits for the same (seed, draw, node i, word w), w = word0 + component:
 *   h1 = hash(seed_lo, seed_hi, draw, i, 2 w), h2 = hash(seed_lo, seed_hi, draw, i, 2 w + 1)   (the pair hash above)
 *   u1 = ((h1 >> 8) + 1) 2^-24 in (0, 1],  u2 = (h2 >> 8) 2^-24 in [0, 1)   (exact in fp32)
 *   xi = sqrtf(-2 logf(u1)) cospif(2 u2)   (precise library functions; |xi| <= sqrt(48 ln 2) = 5.77)
 * i is the node's row in v.  A step's thermostat draw uses word0 = 0 with the step number as draw; thermalize uses word0 = 4 with
 * a counter of its own (data/compute_edge.normal_draw restates xi on the host).  0 <= c <= 1 and s >= 0, or invalid. */
int e3k_md_kick_langevin(float* v, const float* f, const float* mass, const int64_t* node_ptr, int32_t G, int64_t n, float dt,
                         float c, float s, uint32_t seed_lo, uint32_t seed_hi, uint32_t draw, uint32_t word0, float* kinetic,
                         const float* energy, float* potential, void* stream);

/* One FIRE iteration (Bitzek et al., PRL 97, 170201; the step rule of ASE's optimiser, which stands in for the notebook's
 * minimize_bfgs) on forces f [n, 3] at x, every graph with its OWN adaptive state: state [G, 4] fp32 = (dt, alpha, n_pos, fmax).
 * One wave per graph, fixed-order sums, no atomics.  Per graph, with P = sum f.v and fmax = max_i |f_i|:
 *   fmax < ftol: v <- 0, x untouched (frozen; graphs share no edges, so it stays frozen while it goes on being evaluated);
 *   else P < 0:  v <- 0, dt <- dt f_dec, alpha <- alpha_start, n_pos <- 0;
 *   else:        v <- (1 - alpha) v + alpha |v| f / |f|;  if n_pos > n_min: dt <- min(dt f_inc, dt_max), alpha <- alpha f_alpha;
 *                n_pos <- n_pos + 1          (P = 0 counts as downhill -- ASE asks P > 0 -- so that the first iteration from
 *                                             v = 0 does not halve dt);
 *   then (both):  v <- v + dt f (unit masses);  dr = dt v, scaled to length maxstep if its norm over the graph exceeds it;  x += dr.
 * The state row is written back with fmax; energy_record [G] = energy [G] and fmax_record [G] = fmax where the pointers are given.
 * An empty graph is frozen with fmax = 0. */
int e3k_fire_step(float* x, float* v, const float* f, const int64_t* node_ptr, int32_t G, int64_t n, float* state, float ftol,
                  float dt_max, float maxstep, int32_t n_min, float f_inc, float f_dec, float alpha_start, float f_alpha,
                  const float* energy, float* energy_record, float* fmax_record, void* stream);

/* Bond-length constraints for the two half steps above (csrc/e3k_md.hip; SHAKE: Ryckaert, Ciccotti, Berendsen 1977; RATTLE:
 * Andersen 1983).  The constraints form disjoint STARS -- a centre with 1..4 satellites, every constraint centre--satellite, no atom
 * in two stars (the bonds-to-hydrogen set) -- so one thread owns a star: no atomics in the arithmetic, the same bits every run.
 * Tables, built once by the caller:
 *   star_ptr [n_stars + 1] int64: star t is the slots [star_ptr[t], star_ptr[t + 1]) (2..5 of them) of
 *   star_atom [n_slots] int64 and star_len [n_slots] fp32: the centre first (its length slot is not read), then the satellites,
 *             each with the length of its bond beside it;
 *   free_atom [n_free] int64: the atoms in no star;  stars and free atoms are sorted by graph (the free atoms of a graph ascending):
 *   graph_star_ptr, graph_free_ptr [G + 1] int64: each graph's range of stars and of free_atom entries.
 * Every index read from a table is clamped before it is used as an address.  tol > 0 (1e-5 is the usual fp32 setting; below
 * 16 2^-24 fp32 cannot reach it), max_iter >= 1 sweeps.  counter: one DEVICE int32 per call site; a star that does not meet its
 * stopping rule within max_iter sweeps adds 1 to it and is written as it stands (valid numbers, wrong physics): the caller reads the
 * counter where it synchronises anyway and throws the steps since the last reading away.
 *
 * e3k_md_drift_shake replaces e3k_md_drift.  Threads: one per star, behind them one per free atom (e3k_md_drift's expressions,
 *   unchanged).  A star, in coordinates relative to its centre's OLD position (a 10 A coordinate's rounding stays out of a 1 A bond):
 *   v_half = v + dt/2 f / m;  p = old + dt v_half;  passes over its constraints in stored order, with r = p_sat - p_centre and the
 *   OLD bond vector r_old as the direction: a constraint with |r.r - d0^2| > 2 tol d0^2 is corrected,
 *   g = (d0^2 - r.r) / (2 r.r_old (1/m_c + 1/m_s));  p_sat += g / m_s r_old;  p_centre -= g / m_c r_old;  the star is done after a
 *   pass that corrected nothing (at most max_iter correcting passes, then one that only looks).  Then x = centre_old + p and
 *   v = v_half + (p - p_unconstrained) / dt.  r.r_old <= 0 (the bond turned over within the step) counts as a failure.
 *   f NULL: positions only (no kick, no move, v and the free atoms untouched): the lengths are enforced at the present positions
 *   along the present bonds.  Otherwise dt != 0.
 * e3k_md_kick_rattle replaces e3k_md_kick / e3k_md_kick_langevin (their arguments, then x and the tables).  One wave per graph; its
 *   lanes take the graph's stars l, l + 64, ..., then its free atoms l, l + 64, ....  Every atom gets e3k_md_kick_langevin's update
 *   (c = 1, s = 0: the plain kick; f NULL: no kick; c = 0, s = sqrt(kT), f NULL: a Maxwell-Boltzmann draw); a star's velocities
 *   are then projected along its present bond vectors r = x_sat - x_centre:  g = r.(v_sat - v_centre) / (r.r (1/m_c + 1/m_s));
 *   v_sat -= g / m_s r;  v_centre += g / m_c r;  in passes as above, a constraint being corrected while
 *   |r.v_rel| > tol d0 (|v_centre| + |v_sat|).  kinetic [G] is the energy
 *   of the PROJECTED velocities (a lane adds its stars' atoms, then its free atoms; the lanes meet in e3k_md_kick's butterfly);
 *   potential as e3k_md_kick files it.  With no star the two calls give e3k_md_drift's and e3k_md_kick_langevin's values (s = 0
 *   draws nothing where that kernel adds an exact zero).
 *   node_ptr [G + 1] is checked and otherwise unused: the walk follows the tables. */
int e3k_md_drift_shake(float* x, float* v, const float* f, const float* mass, int64_t n, float dt, const int64_t* star_ptr,
                       const int64_t* star_atom, const float* star_len, int64_t n_stars, int64_t n_slots, const int64_t* free_atom,
                       int64_t n_free, float tol, int32_t max_iter, int32_t* counter, void* stream);
int e3k_md_kick_rattle(float* v, const float* f, const float* mass, const int64_t* node_ptr, int32_t G, int64_t n, float dt, float c,
                       float s, uint32_t seed_lo, uint32_t seed_hi, uint32_t draw, uint32_t word0, float* kinetic, const float* energy,
                       float* potential, const float* x, const int64_t* star_ptr, const int64_t* star_atom, const float* star_len,
                       int64_t n_stars, int64_t n_slots, const int64_t* free_atom, int64_t n_free, const int64_t* graph_star_ptr,
                       const int64_t* graph_free_ptr, float tol, int32_t max_iter, int32_t* counter, void* stream);

/* ------------------------------------------------------------------------------------------
 * Training-step plumbing on the flat parameter vector.
 * Replaces clip_grad_norm_ + optim.step() + ema.update() (e3_layers/run/trainer.py:374-386) and the variant that
 * skips the optimizer step on a non-finite gradient (e3_layers/run/sde_utils.py:233-248): torch.optim.Adam
 * (amsgrad off) and torch_ema.ExponentialMovingAverage semantics, one pass over HBM.
 *   param, grad, exp_avg, exp_avg_sq, ema (NULL = no EMA): flat fp32 [n], 16-byte aligned.
 *   max_grad_norm <= 0: no clipping.  skip_nonfinite: leave param / moments untouched when the gradient norm is
 *   not finite (the EMA still updates, as in the reference).
 *   state: DEVICE float[16], zero-initialised once by the caller; holds the step count, bias corrections, clip
 *   coefficient, skip flag, gradient norm ([7]) and the EMA update count — so a captured HIP graph replays
 *   correctly. */
/* A squared-error loss term and its gradient in one launch (a trainer's coefficient x MSELoss term, e3_layers/run/loss.py:186-288
 * with torch.nn.MSELoss; weight != NULL: a weighted sum instead of the mean -- padded batches give their ghost entries weight 0):
 *   loss[0] = scale * sum_i w_i (pred_i - target_i)^2,   grad[i] = 2 scale w_i (pred_i - target_i),   w_i = weight[i / w_group] (one
 * weight per w_group consecutive entries: per node for its three force components), or 1 / n when weight == NULL.
 * One workgroup, fixed summation order. */
int e3k_sq_error(const float* pred, const float* target, const float* weight, int32_t w_group, int64_t n, float scale, float* loss,
                 float* grad, void* stream);
int e3k_adam_ema_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, float* ema, int64_t n,
                      float lr, float beta1, float beta2, float eps, float weight_decay, float ema_decay,
                      int32_t ema_use_num_updates, float max_grad_norm, int32_t skip_nonfinite, float* state,
                      void* stream);
/* The same step under a device-side veto (run/score_step.py: the capped neighbour-list build of a replayed step raises the cell
 * when the list did not fit, after the optimizer launch has long been recorded).  veto: one DEVICE int64, read by the tick(s).
 * While veto[0] != 0 the step does not happen: param, the moments and the EMA shadow keep their bits, state[0] (steps taken) and
 * state[8] (EMA updates) do not advance, state[5] is reset, state[6] = 1, and the effective EMA decay of the launch (state[9]) is
 * 1.  veto[0] == 0: the step above, bit for bit.  veto NULL: invalid. */
int e3k_adam_ema_step_vetoed(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, float* ema, int64_t n,
                             float lr, float beta1, float beta2, float eps, float weight_decay, float ema_decay,
                             int32_t ema_use_num_updates, float max_grad_norm, int32_t skip_nonfinite, float* state,
                             const int64_t* veto, void* stream);

/* ------------------------------------------------------------------------------------------
 * The diffusion score nets' training step around the model (csrc/e3k_score.hip), for a step that is captured once and replayed
 * on a capped neighbour list (run/score_step.py).  Replaces t ~ U(eps, T) and VPSDE.marginal (e3_layers/run/sde_utils.py:54-66,
 * :143-160) and the loss of get_sde_loss_fn (:161-171 with the score of :176-187), whose draws come from a torch generator: here
 * every draw is a function of (seed, draw index, graph or node, word), the pair hash and the normal xi of e3k_md_kick_langevin
 * above (csrc/e3k_draw.h: one definition for both), so a step that has to be redone is redone on exactly the same noised batch.
 *
 * e3k_vpsde_perturb: one launch, one thread per node component.  x0, x_t, z [N, D], std [N], t [G + 1], node_seg [N] int64;
 *   draw: one DEVICE int64 read by every thread and not written (its low 32 bits are the draw index).  Per graph g < G:
 *     u = (hash(seed_lo, seed_hi, draw, 0xFFFFFFFF, g) >> 8) 2^-24;   t_g = fma(T - eps, u, eps);
 *     lm = t (q t + h),  q = -(beta_1 - beta_0) / 4,  h = -beta_0 / 2  (fp32, q t + h one FMA);   a = expf(lm);
 *     s = sqrtf(-expm1f(2 lm))      (1 - expf(2 lm) would lose most of its bits at small t)
 *   per node i of graph g and component c:  z = xi(seed, draw, i, word0 + c);  x_t = fma(a, x0, s z);  std_i = s.
 *   Rows with node_seg outside [0, G) (the ghost graph of a padded batch): x_t = x0, z = 0, std = 1; t[G] = 0.5.
 *   Several diffused keys: one call per key with word0 = the sum of the earlier keys' D; every call files the same t.
 *   0 <= eps <= T, 0 <= beta_0 <= beta_1, 1 <= D <= 1024, or invalid.
 * e3k_denoise_loss: err = -raw - std_i x_t + z (= score std + z with score = -raw / std - x_t);
 *   loss[0] = sum_i w_i (1 / D) sum_c err^2;   grad [N, D] = -2 w_i / D err (the gradient with respect to raw), the same launch.
 *   weight [N] (NULL: 1 / N each).  One workgroup, fixed summation order.
 * e3k_score_step_record: one thread.  cells [2] DEVICE int64 = (step, first_bad):  ring[step mod W] = loss[0];  if overflow[0] != 0
 *   and first_bad < 0: first_bad = step;  step += 1.  overflow: the capped builder's overflow counter (state[1] of e3k_nlist_fill).
 * ------------------------------------------------------------------------------------------ */
int e3k_vpsde_perturb(const float* x0, const int64_t* node_seg, int64_t N, int32_t D, int32_t G, float beta_0, float beta_1,
                      float eps, float T, uint32_t seed_lo, uint32_t seed_hi, const int64_t* draw, uint32_t word0, float* t,
                      float* x_t, float* z, float* std, void* stream);
int e3k_denoise_loss(const float* raw, const float* x_t, const float* z, const float* std, const float* weight, int64_t N,
                     int32_t D, float* loss, float* grad, void* stream);
int e3k_score_step_record(const float* loss, const int64_t* overflow, int64_t* cells, float* ring, int32_t W, void* stream);

/* ------------------------------------------------------------------------------------------
 * The seeded predictor-corrector sampler's arithmetic around the model (csrc/e3k_sampler.hip; run/sde_sampling.py
 * get_pc_sampler(seed=...)).  Replaces the per-step "t = timesteps[i]", get_score_fn's score = -raw / std - x
 * (e3_layers/run/sde_utils.py:176-187), LangevinCorrector.update_fn (e3_layers/run/sde_sampling.py:117-143) and the reverse
 * Euler-Maruyama step (e3_layers/run/sde_utils.py:68-81, :104-119), whose noise came from a torch generator: here the noise of
 * reverse step i is xi(seed, i, node, word) of csrc/e3k_draw.h.  Operands fp32; node_seg [N] int64, a row whose segment is
 * outside [0, G) is a ghost row (e3k_vpsde_perturb's convention): it is copied through bit for bit and enters no sum.
 * cells [2] DEVICE int64 = (next step, step in use).  s(t) = sqrtf(-expm1f(2 lm)), lm = t fma(q, t, h) as e3k_vpsde_perturb.
 *
 * e3k_sampler_begin_step: one workgroup.  k = cells[0]; if 0 <= k < n_times: t[g] = times[k] for every g < G1 (the ghost graph
 *   included), then cells = (k + 1, k).  k outside the table: nothing is written.
 * e3k_sampler_langevin: one workgroup, fixed summation order; x_out may alias x.  Per real row i of graph g:
 *     score_c = -(raw_c / s(t_g)) - x_c;   z_c = xi(seed, cells[1], i, word0 + c);
 *   norms[0] = mean_i sqrtf(sum_c score_c^2), norms[1] = mean_i sqrtf(sum_c z_c^2) over the real rows;
 *     k_i = (int64)((t_g (float)(n_alpha - 1)) / T) clamped to the table;   step_i = ((snr norms[1]) / norms[0])^2 * 2 * alphas[k_i];
 *     x_out_c = x_c + step_i score_c + sqrtf(step_i * 2) z_c.
 *   A zero mean score norm divides by zero, as the reference does.
 * e3k_sampler_reverse_em: one thread per component; x_out may alias x.  dt = -1 / n_sde, beta = fma(t_g, beta_1 - beta_0, beta_0),
 *     z = xi(seed, cells[1], i, word0 + c)   (the caller passes D_total + the key's first word: not the corrector's words);
 *     x_out = x + (-0.5 beta x) dt + sqrtf(beta) sqrtf(|dt|) z - dt beta score.
 * Null pointers, N < 1, D outside [1, 1024], n_times, G1, n_alpha, n_sde < 1, T <= 0, snr <= 0, beta_1 < beta_0: invalid.
 *
 * Conditional sampling (get_pc_sampler(fixed=...): the replacement method of Song et al. 2021, section I.2).
 * e3k_sampler_langevin_fixed, e3k_sampler_reverse_em_fixed: the same kernels' FIXED instances, still one launch.  known [N, D]
 *   fp32 (the known clean values x0, in the model's scaled space), fixed [N] uint8 (not zero: the row is fixed).  A real row i of
 *   graph g with fixed[i] != 0 becomes, instead of the update,
 *     x_out_c = fmaf(expf(lm(t_g)), known_c, s(t_g) * xi(seed, cells[1], i, word_fixed + c))
 *   at the t_g the update read (the caller passes word_fixed = 2 D_total + the key's first word after the corrector,
 *   3 D_total + it after the predictor).  Every other row is what the unconditioned entry point writes, bit for bit: an all-zero
 *   mask reproduces it.  The Langevin norms run over ALL real rows, the fixed ones included, as in e3k_sampler_langevin (the
 *   corrector ran on the whole state; the fixed rows are replaced afterwards).  Ghost rows are copied through whatever their mask
 *   byte holds.  x_out may alias x.  Additionally invalid: null known or fixed, known == x_out.
 * ------------------------------------------------------------------------------------------ */
int e3k_sampler_begin_step(const float* times, int64_t n_times, int64_t* cells, float* t, int32_t G1, void* stream);
int e3k_sampler_langevin(float* x_out, const float* x, const float* raw, const int64_t* node_seg, const float* t,
                         const float* alphas, int64_t N, int32_t D, int32_t G, int32_t n_alpha, float beta_0, float beta_1, float T,
                         float snr, uint32_t seed_lo, uint32_t seed_hi, const int64_t* cells, uint32_t word0, float* norms,
                         void* stream);
int e3k_sampler_reverse_em(float* x_out, const float* x, const float* raw, const int64_t* node_seg, const float* t, int64_t N,
                           int32_t D, int32_t G, float beta_0, float beta_1, int32_t n_sde, uint32_t seed_lo, uint32_t seed_hi,
                           const int64_t* cells, uint32_t word0, void* stream);
int e3k_sampler_langevin_fixed(float* x_out, const float* x, const float* raw, const float* known, const uint8_t* fixed,
                               const int64_t* node_seg, const float* t, const float* alphas, int64_t N, int32_t D, int32_t G,
                               int32_t n_alpha, float beta_0, float beta_1, float T, float snr, uint32_t seed_lo, uint32_t seed_hi,
                               const int64_t* cells, uint32_t word0, uint32_t word_fixed, float* norms, void* stream);
int e3k_sampler_reverse_em_fixed(float* x_out, const float* x, const float* raw, const float* known, const uint8_t* fixed,
                                 const int64_t* node_seg, const float* t, int64_t N, int32_t D, int32_t G, float beta_0, float beta_1,
                                 int32_t n_sde, uint32_t seed_lo, uint32_t seed_hi, const int64_t* cells, uint32_t word0,
                                 uint32_t word_fixed, void* stream);

/* ------------------------------------------------------------------------------------------
 * The probability-flow ODE sampler's arithmetic around the model (csrc/e3k_sampler.hip; run/sde_sampling.py get_ode_sampler):
 * fixed-step Euler and Heun on dx/dt = -0.5 beta(t) [x + score(x, t)].  With the head convention score = -raw / s(t) - x the
 * x terms cancel and the drift is
 *     d(raw, t) = (0.5f * beta(t)) * (raw / s(t)),   beta(t) = fma(t, beta_1 - beta_0, beta_0),   s(t) as above
 * -- the collapsed form the kernels evaluate (no x + (-raw / s - x)).  Operands fp32, ghost rows as above.
 * times [n_times] DEVICE fp32: the run's grid, linspace(T, eps, n_steps + 1).  cells [2] DEVICE int64 (next step, step in use),
 * read and never written.  With k = cells[1]: t_k = times[k], t_n = times[k + 1], hs = t_n - t_k (one fp32 subtraction, negative);
 * the batch's own t is not read.  k < 0 or k + 1 >= n_times: nothing moves (below).
 *
 * e3k_sampler_ode_euler (the Euler step and Heun's stage A): one thread per component.  Real rows inside the table:
 *     d1 = d(raw, t_k);   x_out = fmaf(hs, d1, x);   d_out = d1 (d_out nullable).
 *   Ghost rows, and every row outside the table: x_out = x bit for bit, d_out = 0.  x_out may alias x; d_out aliases nothing.
 *   t_out nullable: inside the table t_out[g] = t_n for every g < G1 (the time of the model's next call; the ghost graph included);
 *   outside it t_out is untouched.  G1 is not read when t_out is null.
 * e3k_sampler_ode_heun (Heun's stage B, at t_n): one thread per component.  Real rows inside the table:
 *     d2 = d(raw2, t_n);   x_out = fmaf(0.5f * hs, d1 + d2, x0).
 *   Ghost rows and every row outside the table: x_out = x0 bit for bit.  x_out may alias x0.
 * Invalid: null pointers (but d_out, t_out), N < 1, N >= 2^31, D outside [1, 1024], G < 0, n_times < 2, beta_0 < 0,
 *   beta_1 < beta_0, N D >= 2^38, t_out with G1 < 1, d_out == x_out, x or raw, d1 == x_out.
 * ------------------------------------------------------------------------------------------ */
int e3k_sampler_ode_euler(float* x_out, float* d_out, const float* x, const float* raw, const int64_t* node_seg, const float* times,
                          int64_t n_times, const int64_t* cells, float* t_out, int32_t G1, int64_t N, int32_t D, int32_t G,
                          float beta_0, float beta_1, void* stream);
int e3k_sampler_ode_heun(float* x_out, const float* x0, const float* d1, const float* raw2, const int64_t* node_seg,
                         const float* times, int64_t n_times, const int64_t* cells, int64_t N, int32_t D, int32_t G, float beta_0,
                         float beta_1, void* stream);

/* ------------------------------------------------------------------------------------------
 * The log-likelihood through the probability-flow ODE (csrc/e3k_sampler.hip; run/likelihood.py get_likelihood_fn; Song et al.
 * 2021, section 4.3 and appendix D.2).  The table ASCENDS (linspace(eps, T, n_steps + 1), hs > 0: data to prior); the two step
 * kernels above run it unchanged.  Per real graph g
 *     log p(x_g(eps)) = log N(x_g(T); 0, I) + integral of div f dt,   div f = c(t) tr(d raw / d x),   c(t) = (0.5 beta(t)) / s(t),
 * the trace by Hutchinson's estimate probe . vjp, vjp = d (probe . raw) / d x from the model's backward.
 * row_ptr [G + 1] DEVICE int32: the graphs' row pointers (e3k_counts_to_ptr), rows sorted by graph; clamped to [0, N].
 *
 * e3k_sampler_probe: one thread per component, out [N, D] fp32.  h_node = the chain of csrc/e3k_draw.h over (seed, draw, i),
 *   word = word0 + c.  kind 0 (Rademacher): +1 if bit 31 of mix32(h_node ^ (2 word)) is clear, else -1; kind 1: xi(seed, draw, i,
 *   word).  Ghost rows (segment outside [0, G)): 0.  draw is a value, not a cell: sde.N + 1 + p for probe p.
 * e3k_sampler_ode_div: one workgroup per real graph, fixed summation order, one writer per acc[g] (DEVICE double [G]):
 *     S = sum over the graph's rows and components of (double)probe * (double)vjp;   acc[g] = fma((w c(t)) scale, S, acc[g]).
 *   k = cells[1], t_k = times[k], t_n = times[k + 1], h = (double)t_n - (double)t_k;  stage 0 (Euler): w = h, t = t_k; 1 (Heun A):
 *   w = h / 2, t = t_k; 2 (Heun B): w = h / 2, t = t_n.  c(t) in double: lm = t (q t + hh) with q = -(beta_1 - beta_0) / 4,
 *   hh = -beta_0 / 2 from the doubles of the fp32 arguments, s = sqrt(-expm1(2 lm)), beta = t (beta_1 - beta_0) + beta_0.
 *   k < 0 or k + 1 >= n_times: acc is untouched.  A graph of no rows adds 0.  Several keys: consecutive launches into one acc.
 * e3k_sampler_prior_logp: the same shape of work: out[g] += -0.5 sum x^2 - (0.5 n_g D) ln(2 pi), double.
 * Invalid: null pointers, N < 1, N >= 2^31, D outside [1, 1024], G < 0, N D >= 2^38, kind outside {0, 1}, stage outside {0, 1, 2},
 *   scale <= 0, n_times < 2, beta_0 < 0, beta_1 < beta_0.  G = 0: nothing is launched.
 * ------------------------------------------------------------------------------------------ */
int e3k_sampler_probe(float* out, const int64_t* node_seg, int64_t N, int32_t D, int32_t G, uint32_t seed_lo, uint32_t seed_hi,
                      uint32_t draw, uint32_t word0, int32_t kind, void* stream);
int e3k_sampler_ode_div(double* acc, const float* probe, const float* vjp, const int32_t* row_ptr, const float* times,
                        int64_t n_times, const int64_t* cells, int64_t N, int32_t D, int32_t G, int32_t stage, double scale,
                        float beta_0, float beta_1, void* stream);
int e3k_sampler_prior_logp(double* out, const float* x, const int32_t* row_ptr, int64_t N, int32_t D, int32_t G, void* stream);

/* ------------------------------------------------------------------------------------------
 * A convolution layer as ONE call (csrc/e3k_layer.hip): FactorizedConvolution + Gate
 * (e3_layers/nn/message_passing.py:91-124, 249) forward and backward -- the launch sequence of
 * backend/conv_block.py issued from native code on the caller's streams, with the library's own events
 * for the cross-stream edges.  The arithmetic is the kernels above, unchanged; what this removes is
 * the host: ~15 ctypes calls, ~12 stream switches and ~20 tensor allocations per layer and pass
 * (0.22 ms forward / 0.30 ms backward of Python per layer: at <= 128 molecules the whole training
 * step was bound by it, at 256 it equalled the GPU time).
 *
 * A layer is described once (template sets as for e3k_gemm_rebased / e3k_gemm_grouped_rebased: byte
 * offsets in the pointer fields; the arrays are copied).  Every buffer is the caller's (PyTorch's
 * allocator): inputs, outputs, saved activations and scratch arrive as device pointers.
 * ------------------------------------------------------------------------------------------ */
typedef struct {
  const e3k_gemm_problem* p;   /* n problems, round-major: round r = p[round_start[r] .. round_start[r + 1]) */
  int32_t n;
  int32_t n_rounds;            /* problems of one round write distinct blocks; round r + 1 accumulates on top of round r */
  int32_t round_start[5];      /* (a Linear whose input block feeds two output blocks -- scalars and gates -- has a */
  int32_t _pad;                /*  two-round input gradient) */
} e3k_gemm_set;

typedef struct {
  const e3k_tp_plan* tp;
  e3k_gemm_set lin1_fwd, lin1_dgrad, lin1_dgrad_acc, lin1_wgrad;
  e3k_gemm_set post_fwd, post_dgrad, post_wgrad; /* post_fwd: conv (+)= scale * Linear(mid); accumulates iff a self-connection exists */
  e3k_gemm_set sc_fwd, sc_dgrad, sc_wgrad;       /* keyed (e3k_gemm_grouped) templates; sc_fwd.n == 0: no self-connection */
  e3k_gemm_set last_fwd, last_dgrad, last_wgrad; /* last layer of the radial MLP: [rows, h] -> [rows, W] */
  const e3k_gate_seg* gate;
  int32_t n_gate;
  int32_t n_in_blocks;
  const e3k_block* in_blocks;                    /* e3nn <-> cf relayout of the layer input */
  const e3k_kw_instr* kw;
  int32_t n_kw, V;
  int64_t ld_m;
  int32_t k0, h, n_hidden, act;                  /* radial MLP hidden chain (e3k_mlp_hidden_*) */
  float cst;
  float alphas[4];
  int32_t d_in, d_x1, d_mid, d_conv, d_out, W;
  int32_t post_in_covered, sc_in_covered, lin1_in_covered, sc_out_covered, post_out_covered, tp_bwd_x_overwrites;
  /* A NARROW layer (w_live > 0; backward only): the same layer for a gy that is zero outside some columns, so that only n_live path
   * slots carry a gradient.  `tp` is then a pruned plan with the weight columns numbered compactly (w_numel = w_live: live slot i's
   * live_len[i] = mul columns behind those of the live slots before it, in (group, slot) order); slot i's column in the DENSE weight
   * row (W wide: the packed table, g_T) is live_col[i].  The plan names which of the two forms the layer is:
   *   SCALAR  e3k_tp_scalar_supported(tp): every live slot is (l2 = l1, l3 = 0), one group per live slot (csrc/e3k_tp_scalar.hip);
   *   MASKED  otherwise, e3k_tp_masked_supported(tp): the live groups with their live slots' mask (csrc/e3k_tp_masked.hip).
   * The backward template sets hold only the problems that end in a live block.  g_w is then [E, w_live], g_mid is written (and
   * read) on the live slots' columns only, the table gradient is formed compactly in g_T_live [knots + 1, w_live] and spread into
   * the dense, zero-filled g_T.  e3k_layer_bwd takes such a layer on the fused packed-table route with the rows from the radial
   * stack only (E3K_ERR_UNSUPPORTED otherwise); e3k_layer_fwd refuses it. */
  int32_t w_live, n_live;
  int32_t live_col[E3K_NARROW_MAX_SLOTS], live_len[E3K_NARROW_MAX_SLOTS];
} e3k_layer_desc;

typedef struct e3k_layer e3k_layer;
int e3k_layer_create(const e3k_layer_desc* desc, e3k_layer** out);
void e3k_layer_destroy(e3k_layer* layer);

/* radial branch of a layer: hidden chain + last layer on R rows (R = E edges, or knots + 1 table rows) and, with the
 * table, the interpolation to the E edges */
typedef struct {
  int64_t R, E;
  int32_t use_table, keep, knots;
  int32_t have_rows;         /* the MLP's output rows (T with the table, else w) were computed by e3k_radial_stack_fwd:
                                the layer only interpolates (table) / uses w as it is; its backward stops at the gradient
                                of those rows (g_T resp. g_w), which e3k_radial_stack_bwd takes from there */
  int32_t in_kernel;         /* table only, plans with e3k_tp_table_supported: the tensor-product kernels interpolate the
                                path weights from T themselves (e3k_tp_fwd_table / e3k_tp_bwd_x_table): no interpolation
                                pass, w unused (may be null); the backward needs T */
  int32_t packed;            /* P already holds the packed form of T (e3k_radial_stack_fwd packs the tables of all its layers
                                in one launch when their rads carry in_kernel and P): the layer does not pack again */
  const float* radial;       /* [R, k0] */
  const int32_t* bin;        /* table: knot per edge, */
  const int32_t* bin_ptr;    /*        edges grouped by knot (backward), */
  const int32_t* bin_perm;
  const float* bin_coef;     /*        the four interpolation weights per edge [E, 4], */
  const int32_t* bin_seg;    /*        first <= 64-edge segment of every knot [knots + 2] (e3k_rtable_bins) */
  const float* w_last;
  const float* w_hidden[4];
  float* h;                  /* [R, h] out */
  float* z[4];               /* [R, h] pre-activations (keep) */
  float* T;                  /* table: [R, W] out; without the table unused */
  float* w;                  /* [E, W] out */
  const int32_t* erec_dst;   /* with P: the batch's edge records over the destination CSR (forward) and over the source CSR */
  const int32_t* erec_src;   /* (input gradient), e3k_edge_records with this table's bin / coef */
  void* P;                   /* in_kernel only: the table packed for the tensor-product kernels [R, W, 3] dwords (e3k_rtable_pack),
                              * written behind T by the forward, read by tp_fwd / tp_bwd_x; NULL: they gather four rows of T */
} e3k_layer_radial;

typedef struct {
  int64_t N, E;
  int32_t in_cf, out_cf, keep, fork, has_w, n_keys;
  int32_t have_m, _pad;              /* have_m: the per-key self-connection weights `m` were computed by e3k_kw_stack_fwd */
  void *main, *side, *side2;
  const float *x, *node_attrs, *sh;
  const int32_t *src, *dst_ptr, *dst_perm;
  const int32_t *perm, *bounds;
  const int64_t* reps;
  const float *w_lin1, *w_post, *w_sc;
  e3k_layer_radial rad;              /* this layer's radial branch (skipped when has_w: rad.w already holds the weights) */
  const e3k_layer* next;             /* look-ahead: the next layer's radial branch, issued behind this layer's tensor product */
  const e3k_layer_radial* next_rad;
  float *x_cf, *a_rep, *m, *conv, *x1, *mid, *y;
} e3k_layer_fwd_args;
int e3k_layer_fwd(const e3k_layer* layer, const e3k_layer_fwd_args* a);

typedef struct {
  int64_t N, E;
  int32_t in_cf, out_cf, fork, n_keys, need_x, need_attrs, need_radial, acc_sc;
  int32_t have_m, fuse_xw;           /* have_m: `gm` (gradient of the per-key weights) is an OUTPUT handed to e3k_kw_stack_bwd;
                                        no weight / attribute gradient of the self-connection is formed here (2: gm arrives
                                        zero-filled, 1: it is zero-filled here).
                                        fuse_xw: with rad.P, the per-edge weight gradient g_w is formed by the input-gradient
                                        walk (e3k_tp_bwd_xw_ptable) instead of a pass of its own (e3k_tp_bwd_w) */
  void *main, *side, *side2, *side3;
  /* saved by the forward */
  const float *x_cf, *sh, *x1, *mid, *conv, *a_rep, *m;
  const int32_t *src, *dst, *dst_ptr, *dst_perm, *src_ptr, *src_perm;
  const int32_t *perm, *bounds;
  const int64_t* reps;
  const float *w_lin1, *w_post, *w_sc;
  e3k_layer_radial rad;              /* as in the forward (h, z, w, radial, bins, weights) */
  const float* gy;
  /* gradient buffers (NULL = not needed); accumulated (gradient sink) or written into zero-filled temporaries */
  float *gb_lin1, *gb_post, *gb_sc, *gb_last;
  float* gb_hidden[4];
  /* outputs */
  float *g_x;        /* [N, d_in] in the layer input's layout (need_x) */
  float *g_attrs;    /* [N, V] (need_attrs): zero-filled here, the per-key rows scattered to the keys' representatives */
  float *g_radial;   /* [R, k0] (need_radial) */
  /* scratch */
  float *g_conv, *g_mid, *g_x1, *g_xcf, *g_w, *g_T, *table_ws, *g_h, *gm, *ga, *kw_ws;
  float *g_T_live;   /* narrow layers: [knots + 1, w_live] scratch */
} e3k_layer_bwd_args;
int e3k_layer_bwd(const e3k_layer* layer, const e3k_layer_bwd_args* a);

/* The radial MLPs of several layers that read the same rows (one edge embedding / one knot basis), batched: hidden
 * chains in ONE launch (e3k_mlp_hidden_fwd_multi), last layers in ONE e3k_gemm_multi call -> rads[i].T (table) or
 * rads[i].w (per edge); backward: last-layer weight gradients in one call, input gradients in one, hidden chains in
 * one.  Per layer this was 2 launches forward and 4-5 backward on 4 097 knot rows -- latency, not work: 0.6 ms of a
 * 3.4 ms step at 64 molecules.  All layers must share k0 / h / depth / activation (the shipped models do). */
typedef struct {
  e3k_layer_radial rad;      /* radial rows, weights, h, z as in the forward */
  const float* g_rows;       /* [R, W] gradient of the MLP's output rows (from e3k_layer_bwd: g_T or g_w) */
  float* gb_last;            /* weight-gradient buffers (NULL = not needed), accumulated */
  float* gb_hidden[4];
  float* g_h;                /* scratch [R, h] */
  float* g_radial;           /* [R, k0] per layer (the caller sums) or NULL */
  /* force training on the table: the gradient of the SLOPE table D = H' W_last (e3k_radial_slope_fwd) joins the table's --
   * gb_last += H'^T g_slope here by the ordinary GEMM; g_hp = g_slope W_last^T is handed to the float64 reverse sweep of the
   * tangent chain (e3k_slope_tangent_bwd), which adds the hidden weights' share into gb_hidden.  All NULL: no slope table. */
  const float* g_slope;      /* [R, W] gradient of D */
  const float* hp;           /* [R, h] H' (fp32) as e3k_radial_slope_fwd wrote it */
  float* g_hp;               /* scratch [R, h] */
} e3k_radial_stack_item;
/* what the slope tables' chain needs besides the layers' weights: the knot radii, the basis and float64 scratch */
typedef struct {
  const float* knots;        /* [R] */
  const float* bessel_w;     /* [k0] */
  float r_max, r_min, p;
  int32_t one_over_r, cutoff_kind, _pad;
  double* acc;               /* backward: e3k_slope_tangent_bwd_scratch(n, n_hidden, k0, h, R) doubles */
  float* g_bessel;           /* backward: [k0] fp32, ADDED to (NULL: the frequencies need no gradient) */
} e3k_slope_ctx;
int e3k_radial_stack_fwd(const e3k_layer* const* layers, const e3k_layer_radial* rads, int32_t n, void* stream);
/* slope: NULL unless some item carries a slope gradient */
int e3k_radial_stack_bwd(const e3k_layer* const* layers, const e3k_radial_stack_item* items, int32_t n, const e3k_slope_ctx* slope,
                         void* stream);
/* The slope tables D_l [R, W] = d/dr fc_l(basis(r)) on the R = knots + 1 knots for the n layers of a radial stack
 * (csrc/e3k_slope.hip): H'_l = forward-mode derivative of the hidden chain, per knot in float64 (fp32 out, hp[l] [R, h], kept for
 * the backward) -> D_l = H'_l W_last_l (the layers' LAST_FWD GEMM sets). */
int e3k_radial_slope_fwd(const e3k_layer* const* layers, const e3k_layer_radial* rads, int32_t n, const e3k_slope_ctx* slope,
                         float* const* hp, float* const* D, void* stream);
/* pieces (also exported for tests).  n_nets <= 16 chains of n_hidden <= 4 layers on the same R knots; w_hidden[i * 4 + l]: layer l of
 * net i, fp32 [k_l, H] with k_0 = k0, k_l = H; H in {32, 64}, 0 < k0 <= H; act in {0 identity, 1 ssp, 2 silu, 4 tanh} (the others have
 * no second derivative here: E3K_ERR_UNSUPPORTED); cutoff_kind 0 polynomial (p), 1 symmetric (x^2 - 1)^2; r_max > r_min;
 * 0 < R < 2^31 - 1 (beyond: E3K_ERR_UNSUPPORTED).  With one_over_r set every knot must be > 0: r = 0 gives 0 * inf = NaN in its row.
 *   forward : hp[i] [R, H] WRITTEN (fp32 rounding of the float64 tangent); a row with r >= r_max is exactly zero.
 *   backward: g_hidden[i * 4 + l] (fp32 [k_l, H]) and g_bessel (fp32 [k0], summed over the nets) are ADDED to -- the caller zeroes or
 *             accumulates; NULL entries of g_hidden and a NULL g_bessel are skipped (the array g_hidden itself must not be NULL).
 *             acc: e3k_slope_tangent_bwd_scratch(...) doubles, 8-byte aligned, written before they are read: it may be handed
 *             over uninitialised, and its contents afterwards are not part of the interface. */
int e3k_slope_tangent_fwd(const float* const* w_hidden, int32_t n_nets, int32_t n_hidden, const float* alphas, const float* knots,
                          int64_t R, const float* bessel_w, int32_t k0, int32_t H, float r_max, float r_min, float p,
                          int32_t one_over_r, int32_t cutoff_kind, int32_t act, float cst, float* const* hp, void* stream);
int64_t e3k_slope_tangent_bwd_scratch(int32_t n_nets, int32_t n_hidden, int32_t k0, int32_t H, int64_t R);
int e3k_slope_tangent_bwd(const float* const* w_hidden, int32_t n_nets, int32_t n_hidden, const float* alphas, const float* knots,
                          int64_t R, const float* bessel_w, int32_t k0, int32_t H, float r_max, float r_min, float p,
                          int32_t one_over_r, int32_t cutoff_kind, int32_t act, float cst, const float* const* g_hp, double* acc,
                          float* const* g_hidden, float* g_bessel, void* stream);

/* The per-key self-connection weights M_l = sum_v a[key, v] W_l[:, v, :] of several layers that read the same node attributes
 * (nn/message_passing.py:81-87, 100 x layers), batched: forward = one gather of the keys' representative rows + ONE launch for
 * all layers; backward (behind the first layer's backward, with the gm each layer's e3k_layer_bwd wrote) = ONE launch for the
 * weight gradients, one + a reduction for the attribute gradient summed over the layers, one scatter to the representatives.
 * Per layer that was 2 launches forward and 6 backward + an autograd add. */
typedef struct {
  const float* w_sc;
  float* m;                  /* forward: OUT [n_keys, ld_m]; backward: IN, the gradient gm of that block */
  float* gb_sc;              /* backward: weight-gradient buffer (NULL = not needed) */
  int32_t acc_sc, _pad;      /*           1 = accumulate into it (gradient sink), 0 = write */
} e3k_kw_stack_item;
int e3k_kw_stack_fwd(const e3k_layer* const* layers, const e3k_kw_stack_item* items, int32_t n, const float* node_attrs,
                     const int64_t* reps, int32_t n_keys, float* a_rep, void* stream);
int64_t e3k_kw_stack_bwd_workspace(const e3k_layer* const* layers, int32_t n, int32_t n_keys);
int e3k_kw_stack_bwd(const e3k_layer* const* layers, const e3k_kw_stack_item* items, int32_t n, const float* a_rep,
                     const int64_t* reps, const int32_t* bounds, int64_t N, int32_t n_keys, float* ga, float* g_attrs,
                     float* workspace, void* stream);

/* Per-kernel timing of a layer's edge kernels (bench.py's roofline block: HIP events on the stream that runs the kernel).
 * e3k_layer_profile(layer, capacity): capacity > 0 arms `capacity` event pairs per kind, 0 disarms.
 * e3k_layer_profile_read: waits for the recorded pairs of `kind` and returns their count (<= cap), filling the elapsed
 * milliseconds and the node / edge counts (table kinds: table rows / edges) of each launch. */
#define E3K_PROF_TP_FWD 0
#define E3K_PROF_TP_BWD_X 1
#define E3K_PROF_TP_BWD_W 2
#define E3K_PROF_RTABLE_FWD 3
#define E3K_PROF_RTABLE_BWD 4
#define E3K_PROF_RADIAL_LAST_FWD 5
int e3k_layer_profile(e3k_layer* layer, int32_t capacity);
/* the same, recording only the kinds whose bit is set in `kinds` (bit = E3K_PROF_* value): a timed region that wants the
 * dominant kernel's durations live without event pairs around every other launch */
int e3k_layer_profile_mask(e3k_layer* layer, int32_t capacity, uint32_t kinds);
int e3k_layer_profile_read(e3k_layer* layer, int32_t kind, float* ms, int64_t* n, int64_t* e, int32_t cap);

/* ------------------------------------------------------------------------------------------
 * Periodic cells, minimum image (csrc/e3k_pbc.hip; the rule itself: csrc/e3k_pbc.h).  Replaces the pbc branch of ASE's
 * neighbour list as the reference's data sets use it (ase.neighborlist: cell, pbc, one image shift per edge) for the capped
 * list above and the edge vectors, under ONE restriction the host checks (data/compute_edge.check_cell): the perpendicular
 * width of every cell along each periodic axis exceeds 2 r_max (1 + 1e-3).  An ordered pair then has at most one image inside
 * the cutoff, an atom never sees its own image, and that image is the one found by rounding the fractional displacement, so
 * the list keeps one slot per ordered pair.  Narrower cells are NOT served by THESE entries (nothing here detects them: pairs
 * are missed); e3k_images_count / _fill below build the list of every image for them.
 * For source i, destination j of graph g, in fp32:
 *   d   = pos[j] - pos[i]
 *   s_k = fmaf(d_z, inv[2][k], fmaf(d_y, inv[1][k], d_x * inv[0][k]))         inv = inv_cell[g]
 *   n_k = pbc[g][k] ? -rintf(s_k) : 0
 *   v_c = fmaf(n_2, c_c, fmaf(n_1, b_c, fmaf(n_0, a_c, d_c)))                  a, b, c = the rows of cell[g]
 *   kept iff sqrtf((v_x v_x + v_y v_y) + v_z v_z) < r_max                      every product rounded on its own, strict
 * With pbc = 0 on every axis v = d exactly and the kept set is e3k_nlist_fill's.  Positions are never wrapped: the image is
 * taken from differences (fp32: sound up to about a thousand cell widths from the origin).
 *   cell, inv_cell [G + 1, 3, 3] fp32 (rows = lattice vectors; inv_cell = the inverse, formed on the host in float64),
 *   pbc [G + 1, 3] int32 (non-zero: periodic); the last entry of each is the ghost graph's (zeros), which is not searched.
 *   e3k_pbc_nlist_count / e3k_pbc_nlist_fill: the contract of e3k_nlist_count / e3k_nlist_fill -- node_seg, node_ptr, counts,
 *     offsets, edge_index [2, e_cap], n_edges, edge_segment (NULL: not wanted), state, flag, the ghost tail, the cut at e_cap
 *     with the value 32 ORed into *flag and state[1] incremented, every node id clamped to [0, N], every store guarded by its
 *     slot < e_cap -- and additionally edge_cell_shift [e_cap, 3] int32 = (n_0, n_1, n_2) of every real edge written, zeros on
 *     the ghost edges.  Refused (E3K_ERR_INVALID, nothing launched): a NULL pointer other than edge_segment, N < 1 or
 *     N >= 2^31, G < 0, e_cap < 0 or e_cap >= 2^31.
 *   e3k_pbc_edge_vector_fwd: edge_vec [E, 3] = v above from the STORED shifts (the builder's vectors bit for bit), edge_len [E]
 *     (NULL: not wanted) = the length the builder compared with r_max.  src, dst [E] int32 are clamped to [0, N - 1]; the graph
 *     is node_seg[src] ([N] int64), clamped to [0, n_cells - 1]; cell [n_cells, 3, 3].  E = 0 launches nothing.  Refused: E, N
 *     or n_cells < 0; with E > 0 a NULL pointer other than edge_len, N < 1 or n_cells < 1.  The backward is
 *     e3k_edge_vector_bwd unchanged (the shift is a constant).
 * ------------------------------------------------------------------------------------------ */
int e3k_pbc_nlist_count(const float* pos, const int64_t* node_seg, const int64_t* node_ptr, int64_t N, int32_t G, float r_max,
                        const float* cell, const float* inv_cell, const int32_t* pbc, int32_t* counts, void* stream);
int e3k_pbc_nlist_fill(const float* pos, const int64_t* node_seg, const int64_t* node_ptr, int64_t N, int32_t G, float r_max,
                       const float* cell, const float* inv_cell, const int32_t* pbc, const int32_t* counts, int64_t e_cap,
                       int64_t* offsets, int64_t* edge_index, int32_t* edge_cell_shift, int64_t* n_edges, int64_t* edge_segment,
                       int64_t* state, int32_t* flag, void* stream);
int e3k_pbc_edge_vector_fwd(const float* pos, const int32_t* src, const int32_t* dst, const int32_t* edge_cell_shift,
                            const int64_t* node_seg, const float* cell, int32_t n_cells, int64_t N, int64_t E, float* edge_vec,
                            float* edge_len, void* stream);

/* ------------------------------------------------------------------------------------------
 * Periodic cells, every image inside the cutoff (csrc/e3k_images.hip; the rule itself, its premise and the order:
 * csrc/e3k_images.h).  For cells narrower than the minimum-image section above allows (crystal unit cells): the capped list of
 * the same builder kernel, with every image of every ordered pair of a graph whose vector is shorter than r_max, an atom's own
 * images included (src == dst, shift != 0).  The host gives an image range per graph and axis (data/compute_edge.image_ranges:
 * R_k = ceil(r_max (1 + 1e-3) / w_k + 0.5) - 1 on a periodic axis of perpendicular width w_k, 0 on the others; a cell the section
 * above accepts has R = 0).  For source i, destination j (j == i included) and every offset m in prod_k [-R_k, R_k], in fp32:
 *   d, s_k as above;  n_k = (pbc[g][k] ? -rintf(s_k) : 0) + m_k;  v from n by the fmaf chain above
 *   kept iff sqrtf((v_x v_x + v_y v_y) + v_z v_z) < r_max  and not (j == i and n == 0)
 * Order: source ascending, destination ascending, then m ascending with m_0 slowest and m_2 fastest, each from -R_k.  With every
 * range zero the outputs are e3k_pbc_nlist_count / _fill's bit for bit.
 *   image_range [G + 1, 3] int32 (the ghost graph's row: zeros).  Every entry is clamped to [0, E3K_IMAGES_MAX_RANGE] and taken as
 *   0 where pbc is 0, so a malformed table cannot widen the walk; every other argument, output, guard and refusal is
 *   e3k_pbc_nlist_count / _fill's, and a NULL image_range is refused (E3K_ERR_INVALID, nothing launched).  The host keeps
 *   (nodes of a graph) x prod_k (2 R_k + 1) below 2^31.
 * ------------------------------------------------------------------------------------------ */
#define E3K_IMAGES_MAX_RANGE 7
int e3k_images_count(const float* pos, const int64_t* node_seg, const int64_t* node_ptr, int64_t N, int32_t G, float r_max,
                     const float* cell, const float* inv_cell, const int32_t* pbc, const int32_t* image_range, int32_t* counts,
                     void* stream);
int e3k_images_fill(const float* pos, const int64_t* node_seg, const int64_t* node_ptr, int64_t N, int32_t G, float r_max,
                    const float* cell, const float* inv_cell, const int32_t* pbc, const int32_t* image_range, const int32_t* counts,
                    int64_t e_cap, int64_t* offsets, int64_t* edge_index, int32_t* edge_cell_shift, int64_t* n_edges,
                    int64_t* edge_segment, int64_t* state, int32_t* flag, void* stream);

/* ------------------------------------------------------------------------------------------
 * Virial (csrc/e3k_virial.hip): the strain derivative of the energy from the operands of the force backward.
 * Row-vector convention (cell's): under x -> x (I + eps), cell -> cell (I + eps),
 *   dE_g / d eps_ab = sum over the edges e of graph g of  v_e[a] g_e[b],
 *   g_e = fmaf(len > 0 ? g_len / len : 0, vec, g_vec)      (fp32: e3k_edge_vector_bwd's per-edge gradient, bit for bit)
 * with v_e = edge_vec[e], the vector the model saw (the periodic shift included).  e3k_virial_edges writes
 *   out[g, 3 a + b] = -(that sum)      the virial, fp32 [G, 9]; written, never accumulated: a graph without edges gets zeros.
 * The nine products and sums are formed in double and rounded once.  One workgroup per graph walks the graph's slots of the
 * by-source CSR -- nodes are sorted by graph, so they are [src_ptr[graph_ptr[g]], src_ptr[graph_ptr[g + 1]]) of src_perm -- and
 * adds in a fixed order: no atomics, the same bits every run, one launch and no zero fill (safe inside a capture).
 *   g_vec [E, 3] or NULL, g_len [E] or NULL (one of them at least), edge_vec [E, 3], edge_len [E] (needed with g_len),
 *   src_ptr [N + 1], src_perm [E] int32 (GraphTopo's), graph_ptr [G + 1] int32 row pointers of the graphs over the nodes.
 *   Every index read is clamped to its table.  G == 0 launches nothing; E == 0 writes the zeros.  Refused (E3K_ERR_INVALID,
 *   nothing launched): N, E or G < 0, N or E >= 2^31; with G > 0 a NULL out, graph_ptr or src_ptr; with E > 0 a NULL edge_vec or
 *   src_perm, both gradients NULL, g_len without edge_len.
 * ------------------------------------------------------------------------------------------ */
int e3k_virial_edges(const float* g_vec, const float* g_len, const float* edge_vec, const float* edge_len, const int32_t* src_ptr,
                     const int32_t* src_perm, const int32_t* graph_ptr, int64_t N, int64_t E, int32_t G, float* out, void* stream);

/* ------------------------------------------------------------------------------------------
 * Barostat (csrc/e3k_barostat.hip): one isotropic pressure-coupling step per graph, on the device, between the drift kernel
 * and the force graph of an MD step.  Stochastic cell rescaling (Bernetti & Bussi 2020) in eps = ln V, Euler-Maruyama; b = 0 is
 * its deterministic limit (Berendsen's weak coupling to first order in a).  Per real graph g, in double:
 *   V     = |det cell[g]|                                  of the fp32 cell
 *   P     = (2 kinetic[g] + virial[g][0] + virial[g][4] + virial[g][8]) / (3 V)
 *   d_eps = a (P - p0) + sqrt(b / V) xi                    a = compressibility dt / tau, b = 2 kT compressibility dt / tau
 *   mu    = exp(d_eps / 3)
 * xi is the standard normal of the draw stream (csrc/e3k_draw.h) for (seed, draw, src = 0xFFFFFFFE, word = g), fp32; b = 0
 * draws nothing.  In the eps form the drift has no kT / V term.  Then, with mu_f = (float)mu and inv_mu_f = (float)(1.0 / mu):
 *   cell[g][k] <- mu_f cell[g][k];  x[c] <- mu_f x[c];  v[c] <- inv_mu_f v[c]  (v NULL: positions and cell only)
 * over the components c of the graph's nodes [node_ptr[g], node_ptr[g + 1]) (each entry clamped to [0, n]); every product is
 * rounded to fp32 once, on its own.  inv_cell[g] <- adjugate / determinant of the NEW fp32 cell, formed in double and rounded to
 * fp32: the inverse of the cell as the periodic builder reads it (exact zeros stay zeros).  volume[g] (NULL: not wanted) = the
 * new |det|, pressure[g] (NULL: not wanted) = the P used; both double.
 * A graph is FROZEN for the call -- nothing of it is written, volume[g] = the old V, pressure[g] = the computed P -- and adds one
 * to *counter (int32, never reset here) when V is 0; when P, d_eps or mu is not finite; when the new cell's determinant is 0 or
 * not finite; or when the new cell's perpendicular width along an axis with pbc[g][k] != 0, 1 / |column k of the inverse| in
 * double, does not exceed min_width (data/compute_edge.check_cell's rule: min_width = 2 r_max (1 + 1e-3)).  Valid numbers, wrong
 * physics, reported: the builder never sees a cell that breaks its one-image premise.
 * One launch, one workgroup of 256 per graph; no atomics in the arithmetic (the counter is an integer add), written not
 * accumulated, no zero fill: the same bits every run, safe beside a capture.  G counts the REAL graphs: the ghost graph's rows
 * of cell, inv_cell and pbc (index G) are never touched.
 *   x [n, 3], v [n, 3] or NULL, cell, inv_cell [>= G, 3, 3] fp32; pbc [>= G, 3] int32; virial [G, 9], kinetic [G] fp32;
 *   node_ptr [G + 1] int64.  G == 0: E3K_OK, nothing launched.  Refused (E3K_ERR_INVALID, nothing launched): G < 0, n < 0, a or b
 *   negative or not finite, min_width < 0 (or NaN); with G > 0 a NULL x, cell, inv_cell, pbc, virial, kinetic, node_ptr or counter.
 * ------------------------------------------------------------------------------------------ */
int e3k_barostat_step(float* x, float* v, float* cell, float* inv_cell, const int32_t* pbc, const float* virial,
                      const float* kinetic, const int64_t* node_ptr, int32_t G, int64_t n, double p0, double a, double b,
                      double min_width, uint32_t seed_lo, uint32_t seed_hi, uint32_t draw, int32_t* counter, double* volume,
                      double* pressure, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* E3K_H */
