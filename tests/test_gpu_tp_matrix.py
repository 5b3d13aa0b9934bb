"""Every tensor-product kernel instantiation (csrc/e3k_tp.hip) against float64 on the CPU.

One case per plan shape.  A case builds a plan, a handmade graph and its inputs, then runs every call kind the plan supports.  It
compares each output with a float64 reference and asserts through ``e3k_tp_last_route()`` that the instantiation in its row
launched.  The kinds the plan does not support must refuse with E3K_ERR_UNSUPPORTED and leave their outputs alone.

References (all float64):
  streamed   F(x, sh, w) = to_cf(scatter(oracle TP(x[src], sh, w), dst)) and its autograd gradients;
  table      w[e] = sum_k coef[e, k] T[bin[e] - 1 + k];
  packed     w[e] = d0 + s (d1 + s (d2 + s d3)), the records of P decoded on the host, s from the edge's Lagrange weights;
  2nd order  the bilinear sums of include/e3k.h (the product rule along (x2, sh2, s2 dw/dr); g_r = <dF/dw, dw/dr>).

``CASES`` is a plain table; tests/test_tp_inventory.py holds it to the kernels the library ships (no GPU needed there).

Element by element.  Beside those normwise comparisons (kept as they were) every element of every output is held to
|got - ref| <= gamma_k M, gamma_k = k u / (1 - k u), u = 2^-24:
  ref, M   ``PlainRef``: the trilinear form written out in numpy float64 over the plan's paths, and the same sum over the absolute
           values of every factor.  tests/test_tp_inventory.py ties it to ``_Oracle`` within 1e-13 M on every case.  The three weight
           sources (``w_streamed``, ``w_table``, ``w_packed``) bring the magnitude of their own sum and their roundings.
  k        the roundings on the longest chain that reaches the element in the kernel as written, a sum of the named terms K_* below
           (each with its source line) plus the terms that depend on the row: one fmaf per in-edge of the node (per out-edge and
           path for g_x; two under the JVP / dual forms), the cross-half add under HALF, and one rounding per share where work
           items meet in atomics or in the ordered combine (g_x of split plans and of plans with a shared input block, g_sh, g_r;
           accumulated outputs are compared after subtracting the prefill, which takes part in those additions).  No constant comes
           from a measurement of the kernels.
  zeros    M == 0 leaves no room: rows of nodes without in-edges (out-edges for g_x), columns no path feeds, and the elements that
           vanish when sh degree 1 is zero (``ZERO_DEGREE``, one channel-complete and one partial case) are exactly zero.
  arena    all buffers of a call lie in one NaN-filled arena with slack round each; every word the header says the call writes is
           claimed by one comparison, every other word -- inputs, slack, and everything when a call is refused -- keeps its bits.
  graphs   the case's graph; one node with a self-loop; three nodes without an edge (what include/e3k.h says of E = 0).
Worst error / bound on an MI355X, over all cases and graphs (a record, not a threshold; profiles/tp_matrix_measured.jsonl):
  fwd 0.546, fwd_table 0.397, fwd_ptable 0.200, fwd_jvp 0.377, fwd_jvp_table 0.259;
  g_w: bwd_w / bwd_w_sh / bwd_e / bwd_e_table 0.481, bwd_xw / bwd_xw_ptable / bwd_xe / bwd_xw_dual plain 0.507, bwd_w_dual 0.434,
  bwd_xw_dual 0.421;  g_x: bwd_x / bwd_xw 0.318, bwd_x_table 0.156, bwd_x_ptable / bwd_xw_ptable 0.102, bwd_x_dual / bwd_xw_dual 0.210,
  bwd_x_dual_table 0.126, bwd_xe 0.227;  g_sh: bwd_w_sh 0.195, bwd_e / bwd_xe 0.102 (stored 0.093), bwd_e_table 0.067 (stored 0.070);
  g_r: bwd_e / bwd_xe 0.227 (stored 0.098 / 0.075), bwd_e_table 0.070 (stored 0.066).
The float32 models of tests/test_tp_inventory.py reach the same values and say why they stay below 1.
"""
import numpy as np
import pytest
import torch

from oracle import e3ref
from tests.util import from_cf, record_measured, rel_err, to_cf

TOL = 1e-5      # (test_gpu_ops.TOL / GTOL)
GTOL = 2e-5
E3K_ERR_UNSUPPORTED = -3
SH9 = "1x0e+1x1o+1x2e"

FIRST_ORDER = ("fwd", "bwd_w", "bwd_w_sh", "bwd_x", "bwd_xw")
SECOND_TABLE = ("fwd_jvp_table", "bwd_x_dual_table", "bwd_e_table")


def _b(v):
    return "true" if v else "false"


def routes(cell):
    """{call kind: kernel instantiation} for a plan in cell (MAXL, L3MAX, SPLIT, FULL): what launch_all must pick."""
    ml, l3, sp, fu = cell
    a = f"{ml}, {l3}, {_b(sp)}, {_b(fu)}"
    r = {"fwd": f"tp_fwd_kernel<{a}, 0>", "bwd_w": f"tp_bwd_w_kernel<false, {a}>", "bwd_w_sh": f"tp_bwd_w_kernel<true, {a}>",
         "bwd_x": f"tp_bwd_x_kernel<{a}, 0>", "bwd_xw": f"tp_bwd_x_kernel<{a}, 6>"}
    if not fu:
        return r
    r.update({"fwd_table": f"tp_fwd_kernel<{a}, 1>", "bwd_x_table": f"tp_bwd_x_kernel<{a}, 1>", "fwd_ptable": f"tp_fwd_kernel<{a}, 4>",
              "bwd_x_ptable": f"tp_bwd_x_kernel<{a}, 4>", "bwd_xw_ptable": f"tp_bwd_x_kernel<{a}, 5>",
              "fwd_jvp": f"tp_fwd_kernel<{a}, 3>", "bwd_x_dual": f"tp_bwd_x_kernel<{a}, 3>", "bwd_xw_dual": f"tp_bwd_x_kernel<{a}, 7>",
              "bwd_xe": f"tp_bwd_x_kernel<{a}, 8>", "bwd_e": f"tp_bwd_e_kernel<{ml}, {l3}, true, {_b(sp)}>",
              "bwd_w_dual": f"tp_bwd_w_dual_kernel<{ml}, {l3}, {_b(sp)}>"})
    if not sp:
        r.update({"fwd_jvp_table": f"tp_fwd_kernel<{a}, 2>", "bwd_x_dual_table": f"tp_bwd_x_kernel<{a}, 2>",
                  "bwd_e_table": f"tp_bwd_e_kernel<{ml}, {l3}, false, false>"})
    return r


def _case(id_, left, sh, out, n, cell, why, y_off_all=False):
    """y_off_all: the groups name the columns of all three sh degrees, used or not (the C ABI allows it; the Python plan builder
    leaves unused degrees at -1, which keeps a one-slot degree-0 plan from being channel-complete)"""
    return {"id": id_, "left": left, "sh": sh, "out": out, "n": n, "cell": cell, "why": why, "routes": routes(cell),
            "y_off_all": y_off_all}


# cell = (MAXL, L3MAX, SPLIT, FULL).  n = 37: below the packed kinds' XCD-ordering threshold (N >= 64); 203: above it, not a multiple of 8
CASES = [
    # ---- channel-complete plans (every group a multiple of 64 channels, every slot of the instantiation enabled, sh 0e+1o+2e)
    _case("full_l0_l3max0", "64x0e", SH9, "64x0e", 37, (0, 0, False, True), "one slot", y_off_all=True),
    _case("full_l0_l3max3", "128x0e", SH9, "1x0e+1x1o+1x2e", 203, (0, 3, False, True), "two 64-channel chunks"),
    _case("full_l1_l3max1", "128x1o", SH9, "1x0e+1x1o+1x1e", 203, (1, 1, False, True), "outputs stop at the input degree"),
    _case("full_l2_l3max2", "64x0e+64x0o+64x1e+64x1o+64x2e+64x2o", SH9, "1x0e+1x0o+1x1e+1x1o+1x2e+1x2o", 37, (2, 2, False, True),
          "both parities"),
    _case("full_l1_split", "64x0e+128x1o", SH9, "1x0e+1x1o+1x1e+1x2e+1x2o+1x3o", 37, (1, 3, True, True), "split, two chunks"),
    _case("full_l2_split", "64x0e+64x1o+64x2e", SH9, "1x0e+1x1o+1x1e+1x2e+1x2o+1x3o+1x3e", 203, (2, 3, True, True), "split"),
    _case("full_l3_split", "64x0e+64x1o+64x2e+64x3o", SH9, "1x0e+1x1o+1x1e+1x2e+1x2o+1x3o+1x3e", 203, (3, 3, True, True),
          "split, l1 = 3"),
    # ---- plans that are not channel-complete
    _case("part_l0_half", "24x0e", SH9, "1x0e", 37, (0, 0, False, False), "HALF: two edges per wave"),
    _case("part_l0_dsh16", "48x0e", "1x0e+1x1o+1x2e+1x3o", "1x0e+1x1o+1x2e", 203, (0, 3, False, False),
          "partial chunk; d_sh = 16 (sh degree 3 feeds no path)"),
    _case("part_l1_mask", "32x0e+80x1o", SH9, "1x0e+1x1o", 37, (1, 1, False, False), "HALF; 80 = one chunk and a partial one; slot 1e missing"),
    _case("part_l1_l3max3", "16x0e+128x1o", SH9, "1x0e+1x2e+1x3o", 203, (1, 3, False, False), "multi-chunk; masks with gaps"),
    _case("part_l1_split_empty_hi", "40x1o", "1x0e+1x1o+1x2e+1x1e", "1x0e+1x1o+1x1e+1x2e+1x2o+1x3o", 203, (1, 3, True, False),
          "two groups on one input block (x_shared), the second with an empty high part; d_sh = 12"),
    _case("part_l2_shared", "32x0e+32x1o+32x2e", "1x0e+1x1o+1x2e+1x1e", "1x0e+1x1o+1x2e", 37, (2, 2, False, False),
          "HALF; repeated sh degree (x_shared); d_sh = 12"),
    _case("part_l2_l3max3", "24x1o+80x2e", SH9, "1x0e+1x3o", 37, (2, 3, False, False), "HALF and a partial chunk"),
    _case("part_l2_split_half", "24x1o+64x2e", SH9, "1x0e+1x1o+1x1e+1x2e+1x2o+1x3o+1x3e", 203, (2, 3, True, False),
          "HALF inside a split plan"),
    _case("part_l2_split_empty_parts", "40x1o+40x2o", "1x0e+1x1o+1x2e+1x2o+1x1e+1x1o", "1x0o+1x2o+1x3e+1x3o", 37, (2, 3, True, False),
          "an l1 = 1 group with an empty low part, an l1 = 2 group with an empty high part; d_sh = 20"),
    _case("part_l3", "32x0e+48x3o", SH9, "1x0e+1x3o", 203, (3, 3, False, False), "l1 = 3 unsplit"),
    _case("part_l3_split", "40x1o+64x3o", SH9, "1x0e+1x1o+1x1e+1x2e+1x2o+1x3o", 37, (3, 3, True, False), "l1 = 3 split, slot 3e missing"),
]


def table_routes():
    return {r for c in CASES for r in c["routes"].values()}


# ---------------------------------------------------------------------------------------------------------------------------------
def _graph(n, seed):
    """edge_index [2, E]: node 0 receives 301 edges, node 1 sends 300; node n - 1 is isolated, n - 2 only sends, n - 3 only
    receives; a self-loop and a repeated (src, dst) pair; in-degrees of the rest 0..7 (odd ones leave a HALF trip half empty);
    edge ids shuffled."""
    g = torch.Generator().manual_seed(seed)
    senders = torch.tensor([i for i in range(n - 3)] + [n - 2])
    receivers = torch.arange(n - 2)
    src = [senders[torch.randint(0, len(senders), (301,), generator=g)], torch.full((300,), 1)]
    dst = [torch.zeros(301, dtype=torch.long), receivers[torch.randint(0, len(receivers), (300,), generator=g)]]
    for v in range(2, n - 3):
        k = int(torch.randint(0, 8, (1,), generator=g))
        src.append(senders[torch.randint(0, len(senders), (k,), generator=g)])
        dst.append(torch.full((k,), v))
    src.append(torch.tensor([2, 3, 3, n - 2, 5]))
    dst.append(torch.tensor([2, 4, 4, 6, n - 3]))
    ei = torch.stack([torch.cat(src), torch.cat(dst)]).long()
    return ei[:, torch.randperm(ei.shape[1], generator=g)]


class _Oracle:
    """F(x_cf, sh, w) [N, d_mid] in the kernels' layout, float64, and its gradients."""

    def __init__(self, left, sh_ir, out, simp, ei, n):
        self.tp = e3ref.TensorProductExpansion(left, (sh_ir, "edge_spherical"), (out, "edge_features"), "uvu",
                                               internal_weight=False).double().tp
        self.left, self.simp, self.src, self.dst, self.n = left, simp, ei[0], ei[1], n

    def F(self, x, sh, w):
        y = self.tp(from_cf(x, self.left)[self.src], sh, w)
        return to_cf(e3ref.scatter(y, self.dst, dim_size=self.n), self.simp)

    def G(self, x, sh, w, g):
        """(dF/dx, dF/dsh, dF/dw) contracted with g"""
        args = [t.detach().clone().requires_grad_(True) for t in (x, sh, w)]
        return torch.autograd.grad(self.F(*args), args, g)


def _interp64(table, bins):
    t64, b, c = table.cpu().double(), bins.bin.cpu().long(), bins.coef.cpu().double()
    return sum(c[:, k:k + 1] * t64[b - 1 + k] for k in range(4))


def _packed_fields(packed):
    """(d0, d1, d2, d3) [K + 1, W] float64 from P (row: W (d0, d1) f32 pairs, then W f16 pairs (d2 2^10, d3 2^16))"""
    rows, w = packed.shape[0], packed.shape[1]
    p = packed.cpu().reshape(rows, 3 * w)
    pairs = p[:, :2 * w].contiguous().view(torch.float32).double()
    h = p[:, 2 * w:].contiguous().view(torch.float16).double().reshape(rows, w, 2)
    return pairs[:, 0::2], pairs[:, 1::2], h[..., 0] / 1024.0, h[..., 1] / 65536.0


def _packed_w64(packed, bins):
    d0, d1, d2, d3 = _packed_fields(packed)
    c, b = bins.coef.cpu().double(), bins.bin.cpu().long()
    s = (2.0 * c[:, 3] + c[:, 2] - c[:, 0] - 0.5).unsqueeze(1)      # t = sum_k x_k L_k(t), x = (-1, 0, 1, 2); s = t - 1/2
    return d0[b] + s * (d1[b] + s * (d2[b] + s * d3[b]))


def _check_packing(table, packed, knots):
    """The records against the cubic of the fp32 table in float64: within the fp16 rounding bound of e3k_rtable.hip
    (2^-11 (|d2| / 8 + |d3| / 32), after economisation) plus the fp32 rounding of d0 and d1, for |s| <= 1/2."""
    d0, d1, d2, d3 = _packed_fields(packed)
    t = table.cpu().double()
    i = torch.arange(1, knots - 1)
    a, b, c, d = t[i - 1], t[i], t[i + 1], t[i + 2]
    c1, c2, c3 = -a / 3 - b / 2 + c - d / 6, a / 2 - b + c / 2, -a / 6 + b / 2 - c / 2 + d / 6
    e0, e1, e2, e3 = b + c1 / 2 + c2 / 4 + c3 / 8, c1 + c2 + 0.75 * c3, c2 + 1.5 * c3, c3
    bound = 2.0 ** -11 * (e2.abs() / 8 + e3.abs() / 32) + 2.0 ** -24 * (e0.abs() + e1.abs() / 2) + 2.0 ** -40
    for s in torch.linspace(-0.5, 0.5, 9, dtype=torch.float64):
        got = d0[i] + s * (d1[i] + s * (d2[i] + s * d3[i]))
        exact = e0 + s * (e1 + s * (e2 + s * e3))
        assert bool(((got - exact).abs() <= 1.25 * bound).all()), float(((got - exact).abs() / bound).max())
    assert bool((packed.cpu().reshape(packed.shape[0], -1)[[0, knots - 1, knots]] == 0).all())      # rows no edge uses


# ---------------------------------------------------------------------------------------------------------------------------------
# The plain float64 reference: the trilinear form written out over the plan's paths, with magnitudes
U = 2.0 ** -24


def gamma(k):
    k = np.asarray(k, np.float64)
    return k * U / (1.0 - k * U)


# Roundings of the kernels, by name (e3k_tp.hip / e3k_tp_body.h / e3k_cg_gen.h as committed with this file).  A chain is counted on
# the term that passes through the most of them; every other term of the same sum passes through fewer.
K_PROD = 1         # p = a[i] * b[j]                                      e3k_cg_gen.h: "const T p{i}_{j} = ..." (tools/gen_cg.py:42)
K_LIT = 2          # the Wigner-3j literal: nine decimals after the point of the mantissa (tools/gen_cg.py:28, relative 5e-10 = u / 119),
#                    then the compiler's fp32 rounding: (1 + u / 119)(1 + u) <= (1 + u)^2
#  + nt              c * p, then one cg_fma per further term of the output component (tools/gen_cg.py:50-54): nt = its term count
K_COEFF = 1        # coeff[q] reaches the plan as the fp32 of sqrt(2 l3 + 1) (nn/core.py: g.coeff[q] = math.sqrt(...) into a c_float)
K_SCALE = 1        # wv = w * coeff (e3k_tp.hip:231, 319, 504, 603, 787, 802, 821, 934, 943); gw = dot * coeff (:502, 600, 794, 813, 828, 941)
K_TABLE = 4        # knot_mix (e3k_tp.hip:126-128): c0 * va, then three fmaf
K_PACKED = 12      # packed_mix (e3k_tp_body.h:202-205): three fmaf on the d3 term, whose three factors s carry three roundings each --
#                    s = fmaf(2, c3, c2 - c0) - 0.5 (e3k_tp_body.h:188): the difference, the fmaf, the shift; s / 1024, s / 64, the
#                    fp16 -> fp32 conversions and the power-of-two scales of d2, d3 are exact
K_S2 = 1           # w2 = s2[e] * dw/dr (e3k_tp.hip:209, 224, 747, 766)
K_ADD = 1          # ta[k] + tb[k] (e3k_tp.hip:241), tt[k] += tb[k] (:492)
K_HALF = 1         # acc += __shfl_xor(acc, 32) (e3k_tp.hip:333, 950): the two lane halves' partial sums
K_BUTTERFLY = 6    # wave_add9 (e3k_tp.hip:356-385): six levels of adds over 64 lanes; wave_sum (e3k_common.h:84-88) likewise
# (per in-edge: one fmaf into the accumulator, e3k_tp.hip:244, 323; two under JVP, :241.  per out-edge and path: one fmaf into gx,
#  inside CG::yg (tools/gen_cg.py:56) or :791, 805, 808, 825, 938; the dots: one fmaf per component, :500, 598, 792, 809-811, 826, 939.
#  atomics, e3k_tp.hip:403, 618, 848, 858, 957, and the ordered combine :1069, 1073: one rounding per share, in any order)


def host_csr(key, n):
    """(ptr [n + 1], perm [E]) int32: the edges grouped by key, ascending edge id inside a group"""
    key = np.asarray(key, np.int64)
    return (np.concatenate([[0], np.cumsum(np.bincount(key, minlength=n))]).astype(np.int32),
            np.argsort(key, kind="stable").astype(np.int32))


class PlainRef:
    """out[n, out_off + k stride + u] = sum_{e: dst(e) = n} coeff sum_ij C_ijk x[src(e), x_off + i mul + u] sh[e, y_off + j] w[e, w_off + u]
    over the paths of ``plan.groups`` (offsets, multiplicities, masks as the plan hands them to e3k_tp_plan_create; C from
    o3/wigner.py in float64), its three gradients contracted with g, and for each the same sum over the absolute values of every
    factor (``mag=True``): the magnitude M the bounds are multiples of.  numpy float64 throughout.

    The path coefficient: the plan carries the fp32 of sqrt(2 l3 + 1), the reference uses the square root itself (K_COEFF counts
    the rounding; test_tp_inventory asserts that the plan's value is that rounding)."""

    def __init__(self, plan, ei, n, full):
        import math
        from types import SimpleNamespace

        from e3_layers_amd.nn.core import tp_slots
        from e3_layers_amd.o3.wigner import wigner_3j

        ei = np.asarray(ei, np.int64).reshape(2, -1)
        self.plan, self.n, self.full = plan, int(n), bool(full)
        self.src, self.dst, self.e = ei[0], ei[1], ei.shape[1]
        self.d_in, self.d_sh, self.W, self.d_mid = plan.d_in, plan.d_sh, plan.w_numel, plan.d_mid
        self.A_dst = np.zeros((self.n, self.e))
        self.A_dst[self.dst, np.arange(self.e)] = 1.0
        self.A_src = np.zeros((self.n, self.e))
        self.A_src[self.src, np.arange(self.e)] = 1.0
        self.deg_in, self.deg_out = np.bincount(self.dst, minlength=self.n), np.bincount(self.src, minlength=self.n)
        self.paths, self._seen = [], {}
        for gi, g in enumerate(plan.groups):
            for q, (l2, l3) in enumerate(tp_slots(g.l1)):
                if not (g.mask >> q) & 1:
                    continue
                c = np.asarray(wigner_3j(g.l1, l2, l3), np.float64)
                nz = c != 0
                cols = g.out_off[q] + np.arange(2 * l3 + 1)[:, None] * g.out_stride[q] + np.arange(g.mul)[None, :]
                self.paths.append(SimpleNamespace(
                    g=gi, q=q, l1=g.l1, l2=l2, l3=l3, x_off=g.x_off, mul=g.mul, y_off=g.y_off[l2], w_off=g.w_off[q], cols=cols,
                    coeff=math.sqrt(2 * l3 + 1), coeff32=float(g.coeff[q]), C=c, nt_xy=int(nz.sum((0, 1)).max()),
                    nt_yg=int(nz.sum((1, 2)).max()), nt_xg=int(nz.sum((0, 2)).max())))
        # the work items as e3k_tp_plan_create lists them (e3k_tp.hip:1325-1357): (group, part, paths); a 64-channel chunk each
        n_acc = [sum(2 * p.l3 + 1 for p in self.paths if p.g == gi) for gi in range(len(plan.groups))]
        self.split = any(g.l1 >= 1 and a > 24 for g, a in zip(plan.groups, n_acc))
        self.items = []
        for gi, g in enumerate(plan.groups):
            mine = [p for p in self.paths if p.g == gi]
            if self.split and g.l1 >= 1:
                at = 3 if g.l1 == 3 else 4
                for part, sel in ((0, [p for p in mine if p.q < at]), (1, [p for p in mine if p.q >= at])):
                    if sel:
                        self.items.append(SimpleNamespace(g=gi, part=part, paths=sel, chunks=(g.mul + 63) // 64))
            else:
                self.items.append(SimpleNamespace(g=gi, part=2, paths=mine, chunks=(g.mul + 63) // 64))
        self.n_gc = sum(it.chunks for it in self.items)
        blocks = [(g.x_off, g.x_off + (2 * g.l1 + 1) * g.mul) for g in plan.groups]
        self.x_shared = any(a[0] < b[1] and b[0] < a[1] for i, a in enumerate(blocks) for b in blocks[:i])

    def half(self, gi):
        """two edges per wave (e3k_tp.hip:273-277, 421-425, 873-877): plans that are not channel-complete, groups of <= 32 channels"""
        return (not self.full) and self.plan.groups[gi].mul <= 32

    # ---- the four sums (a call is remembered by its operands: the call kinds share most of them)
    def _memo(self, name, args, mag, fn):
        key = (name, mag) + tuple(id(v) for v in args)
        hit = self._seen.get(key)
        if hit is None:
            hit = self._seen[key] = (fn(np.abs if mag else (lambda v: v)), args)      # (args kept: their ids are the key)
        return hit[0]

    def _X(self, p, x, a):
        return a(x[:, p.x_off:p.x_off + (2 * p.l1 + 1) * p.mul][self.src]).reshape(self.e, 2 * p.l1 + 1, p.mul)

    def _CY(self, p, sh, a):
        """[E, 2 l1 + 1, 2 l3 + 1]: sum_j C_ijk sh[e, y_off + j]"""
        return np.einsum("ijk,ej->eik", a(p.C), a(sh[:, p.y_off:p.y_off + 2 * p.l2 + 1]))

    def _G(self, p, g, a):
        return a(g[:, p.cols.ravel()][self.dst]).reshape(self.e, 2 * p.l3 + 1, p.mul)

    def F(self, x, sh, w, mag=False):
        def run(a):
            out = np.zeros((self.n, self.d_mid))
            for p in self.paths:
                msg = p.coeff * np.matmul(self._CY(p, sh, a).transpose(0, 2, 1), self._X(p, x, a)) * a(w[:, None, p.w_off:p.w_off + p.mul])
                out[:, p.cols.ravel()] += self.A_dst @ msg.reshape(self.e, p.cols.size)
            return out
        return self._memo("F", (x, sh, w), mag, run)

    def Gw(self, x, sh, g, mag=False):
        def run(a):
            out = np.zeros((self.e, self.W))
            for p in self.paths:
                t = np.matmul(self._CY(p, sh, a).transpose(0, 2, 1), self._X(p, x, a))
                out[:, p.w_off:p.w_off + p.mul] += p.coeff * (t * self._G(p, g, a)).sum(1)
            return out
        return self._memo("Gw", (x, sh, g), mag, run)

    def Gx(self, sh, w, g, mag=False):
        def run(a):
            out = np.zeros((self.n, self.d_in))
            for p in self.paths:
                msg = p.coeff * np.matmul(self._CY(p, sh, a), self._G(p, g, a)) * a(w[:, None, p.w_off:p.w_off + p.mul])
                out[:, p.x_off:p.x_off + (2 * p.l1 + 1) * p.mul] += self.A_src @ msg.reshape(self.e, (2 * p.l1 + 1) * p.mul)
            return out
        return self._memo("Gx", (sh, w, g), mag, run)

    def Gsh(self, x, w, g, mag=False):
        def run(a):
            out = np.zeros((self.e, self.d_sh))
            for p in self.paths:
                gw = self._G(p, g, a) * a(w[:, None, p.w_off:p.w_off + p.mul])
                xg = np.matmul(self._X(p, x, a), gw.transpose(0, 2, 1))      # [E, 2 l1 + 1, 2 l3 + 1]
                out[:, p.y_off:p.y_off + 2 * p.l2 + 1] += p.coeff * np.einsum("ijk,eik->ej", a(p.C), xg)
            return out
        return self._memo("Gsh", (x, w, g), mag, run)

    # ---- the roundings on the longest chain that reaches an element: k, as arrays shaped like the outputs
    def k_fwd(self, k_w, jvp=False):
        """out [N, d_mid]: the CG sum, coeff, w * coeff, the weight source (k_w) and the walk over the node's in-edges"""
        k = np.zeros((self.n, self.d_mid))
        for p in self.paths:
            deg = self.deg_in.astype(np.float64)
            if jvp:      # fmaf(wv, ta + tb, fmaf(wv2, tt, acc)): two per edge; ta + tb; w2 = s2 * dw/dr
                walk = 2 * deg + K_ADD + K_S2
            elif self.half(p.g):      # half the edges each (the odd one to the lower half), then the cross-half add
                walk = np.ceil(deg / 2) + K_HALF
            else:
                walk = deg
            k[:, p.cols.ravel()] = (K_PROD + K_LIT + p.nt_xy + K_COEFF + K_SCALE + k_w + walk)[:, None]
        return k

    def k_gw(self, form, dual=False):
        """g_w [E, W].  form "xy": dot over the 2 l3 + 1 components of xy(x, sh) (tp_bwd_w, tp_bwd_e); "yt": dot over the 2 l1 + 1
        components of yt(sh, g) (tp_bwd_x with g_w).  dual: two such sums in one dot (xy: added before the dot)"""
        k = np.zeros((self.e, self.W))
        for p in self.paths:
            if form == "xy":
                v = K_PROD + K_LIT + p.nt_xy + (K_ADD if dual else 0) + (2 * p.l3 + 1)
            else:
                v = K_PROD + K_LIT + p.nt_yg + (2 if dual else 1) * (2 * p.l1 + 1)
            k[:, p.w_off:p.w_off + p.mul] = v + K_SCALE + K_COEFF
        return k

    def k_gx(self, k_w, dual=False):
        """g_x [N, d_in]: per work item the CG sum, w * coeff, the weight source, one fmaf per (out-edge, path of the item) -- two
        under dual, whose second weight is s2 * dw/dr -- the cross-half add; then one rounding per item that adds into the element
        where the items meet in atomics (two parts of a split group, groups that share an input block)"""
        k, m = np.zeros((self.n, self.d_in)), np.zeros(self.d_in)
        for it in self.items:
            g = self.plan.groups[it.g]
            deg = self.deg_out.astype(np.float64)
            if self.half(it.g):
                walk = np.ceil(deg / 2) * len(it.paths) + K_HALF
            else:
                walk = deg * len(it.paths) * (2 if dual else 1) + (K_S2 if dual else 0)
            v = K_PROD + K_LIT + max(p.nt_yg for p in it.paths) + K_SCALE + K_COEFF + k_w + walk
            sl = slice(g.x_off, g.x_off + (2 * g.l1 + 1) * g.mul)
            k[:, sl] = np.maximum(k[:, sl], v[:, None])
            m[sl] += 1
        atomic = np.zeros(self.d_in)
        for it in self.items:      # e3k_tp.hip:857, 956: stored only by an unsplit group on a plan without shared blocks
            g = self.plan.groups[it.g]
            if it.part != 2 or self.x_shared:
                atomic[g.x_off:g.x_off + (2 * g.l1 + 1) * g.mul] = 1
        return k + (m * atomic)[None, :]

    def k_gsh(self, k_w):
        """(k [E, d_sh] of a work item's share, m [E, d_sh]: the shares that meet in the element): per item the CG sum, w * coeff, the
        weight source, one fmaf per path of the item with that sh degree, the butterfly; then one rounding per share"""
        k, m = np.zeros((self.e, self.d_sh)), np.zeros((self.e, self.d_sh))
        for it in self.items:
            for l2 in sorted({p.l2 for p in it.paths}):
                sel = [p for p in it.paths if p.l2 == l2]
                v = K_PROD + K_LIT + max(p.nt_xg for p in sel) + K_SCALE + K_COEFF + k_w + len(sel) + K_BUTTERFLY
                sl = slice(sel[0].y_off, sel[0].y_off + 2 * l2 + 1)
                k[:, sl] = np.maximum(k[:, sl], v)
                m[:, sl] += it.chunks
        return k, m

    def k_gr(self, form, k_d):
        """(k [E], m [E]) of g_r = <g_w, dw/dr>: g_w's chain (form), dw/dr's source (k_d), one fmaf per path of the item, wave_sum"""
        kw = self.k_gw(form)
        k = max(float(kw[0, p.w_off]) if self.e else 0.0 for p in self.paths) + k_d + max(len(it.paths) for it in self.items) + K_BUTTERFLY
        return np.full(self.e, k), np.full(self.e, float(self.n_gc))


# ---- the three weight sources: (w float64, magnitude of its own sum, roundings the kernel spends on it)
def w_streamed(w):
    w = np.asarray(w, np.float64)
    return w, np.abs(w), 0


def w_table(table, bin_, coef):
    """w[e] = sum_k coef[e, k] T[bin[e] - 1 + k] (knot_mix)"""
    t, b, c = np.asarray(table, np.float64), np.asarray(bin_, np.int64), np.asarray(coef, np.float64)
    rows = [t[b - 1 + k] for k in range(4)] if len(b) else [np.zeros((0, t.shape[1]))] * 4
    return (sum(c[:, k:k + 1] * rows[k] for k in range(4)), sum(np.abs(c[:, k:k + 1] * rows[k]) for k in range(4)), K_TABLE)


def w_packed(fields, bin_, coef):
    """w[e] = d0 + s (d1 + s (d2 + s d3)), s = 2 c3 + c2 - c0 - 1/2 (packed_mix); the magnitude: the same polynomial over
    |d| and S = 2 |c3| + |c2| + |c0| + 1/2 >= |s| -- the kernel's s has an absolute error, gamma_3 S, not a relative one"""
    d0, d1, d2, d3 = (np.asarray(d, np.float64) for d in fields)
    b, c = np.asarray(bin_, np.int64), np.asarray(coef, np.float64)
    s = (2.0 * c[:, 3] + c[:, 2] - c[:, 0] - 0.5)[:, None]
    S = (2.0 * np.abs(c[:, 3]) + np.abs(c[:, 2]) + np.abs(c[:, 0]) + 0.5)[:, None]
    return (d0[b] + s * (d1[b] + s * (d2[b] + s * d3[b])),
            np.abs(d0[b]) + S * (np.abs(d1[b]) + S * (np.abs(d2[b]) + S * np.abs(d3[b]))), K_PACKED)


def reference(ref, kind, ops, src_w, src_d=None):
    """{output: (value, bound, prefill share)} of one call kind.  ops: x, x2, g, sh, sh2, s2 (float64); src_w = (w, M_w, k_w) and
    src_d = (dw/dr, M_d, k_d) from a weight source above.  bound = gamma_k M elementwise; outputs accumulated with atomics come
    with m, the number of shares that meet in the element: their bound is gamma_(k + m) M + gamma_m |prefill| (the caller adds the
    second term: the prefill takes part in the m additions)."""
    x, x2, g, sh, sh2, s2 = (ops.get(k) for k in ("x", "x2", "g", "sh", "sh2", "s2"))
    w, Mw, k_w = src_w
    if src_d is not None:
        dw, Md, k_d = src_d
        sdw, sMd = s2[:, None] * dw, np.abs(s2)[:, None] * Md
    out = {}

    def put(name, val, k, M, m=None):
        out[name] = (val, gamma(k + (0 if m is None else m)) * M, m)

    if kind in ("fwd", "fwd_table", "fwd_ptable"):
        put("out", ref.F(x, sh, w), ref.k_fwd(k_w), ref.F(x, sh, Mw, True))
    elif kind in ("bwd_w", "bwd_w_sh"):
        put("g_w", ref.Gw(x, sh, g), ref.k_gw("xy"), ref.Gw(x, sh, g, True))
        if kind == "bwd_w_sh":
            k, m = ref.k_gsh(k_w)
            put("g_sh", ref.Gsh(x, w, g), k, ref.Gsh(x, Mw, g, True), m)
    elif kind in ("bwd_x", "bwd_x_table", "bwd_x_ptable", "bwd_xw", "bwd_xw_ptable"):
        put("g_x", ref.Gx(sh, w, g), ref.k_gx(k_w), ref.Gx(sh, Mw, g, True))
        if kind in ("bwd_xw", "bwd_xw_ptable"):
            put("g_w", ref.Gw(x, sh, g), ref.k_gw("yt"), ref.Gw(x, sh, g, True))
    elif kind in ("fwd_jvp", "fwd_jvp_table"):
        put("out", ref.F(x2, sh, w) + ref.F(x, sh2, w) + ref.F(x, sh, sdw), ref.k_fwd(max(k_w, k_d), jvp=True),
            ref.F(x2, sh, Mw, True) + ref.F(x, sh2, Mw, True) + ref.F(x, sh, sMd, True))
    elif kind in ("bwd_x_dual", "bwd_x_dual_table", "bwd_xw_dual"):
        put("g_x", ref.Gx(sh2, w, g) + ref.Gx(sh, sdw, g), ref.k_gx(max(k_w, k_d), dual=True),
            ref.Gx(sh2, Mw, g, True) + ref.Gx(sh, sMd, g, True))
        if kind == "bwd_xw_dual":
            put("g_w", ref.Gw(x2, sh, g) + ref.Gw(x, sh2, g), ref.k_gw("yt", dual=True), ref.Gw(x2, sh, g, True) + ref.Gw(x, sh2, g, True))
            put("g_w_plain", ref.Gw(x, sh, g), ref.k_gw("yt"), ref.Gw(x, sh, g, True))
    elif kind == "bwd_w_dual":
        put("g_w", ref.Gw(x2, sh, g) + ref.Gw(x, sh2, g), ref.k_gw("xy", dual=True), ref.Gw(x2, sh, g, True) + ref.Gw(x, sh2, g, True))
    elif kind in ("bwd_e", "bwd_e_table", "bwd_xe"):
        form = "yt" if kind == "bwd_xe" else "xy"
        gw, Mgw = ref.Gw(x, sh, g), ref.Gw(x, sh, g, True)
        if kind == "bwd_xe":
            put("g_x", ref.Gx(sh, w, g), ref.k_gx(k_w), ref.Gx(sh, Mw, g, True))
        k, m = ref.k_gsh(k_w)
        put("g_sh", ref.Gsh(x, w, g), k, ref.Gsh(x, Mw, g, True), m)
        k, m = ref.k_gr(form, k_d)
        put("g_r", (gw * dw).sum(1), k, (Mgw * Md).sum(1), m)
        put("g_w", gw, ref.k_gw(form), Mgw)
    else:
        raise KeyError(kind)
    return out


def within(label, got, entry):
    """|got - ref| <= bound on every element of one output of ``reference`` (got: an array or tensor shaped like it); returns the
    worst error / bound.  An element whose bound is zero must be exact."""
    val, bound, _ = entry
    got = np.asarray(got.detach().cpu().numpy() if isinstance(got, torch.Tensor) else got, np.float64)
    assert got.shape == val.shape and np.isfinite(got).all(), f"{label}: shape, or an element that is not finite"
    err = np.abs(got - val)
    bad = np.argwhere(err > bound)
    assert len(bad) == 0, (f"{label}: {len(bad)} of {err.size} elements outside gamma_k M; first at {bad[:4].tolist()}: got {got[tuple(bad[0])]}, "
                           f"want {val[tuple(bad[0])]}, bound {bound[tuple(bad[0])]}")
    live = bound > 0
    return float((err[live] / bound[live]).max()) if live.any() else 0.0


# ---------------------------------------------------------------------------------------------------------------------------------
# graphs and operands of a case (tests/test_tp_inventory.py draws the same ones on the CPU)
R_MAX, KNOT_TARGET = 5.0, 128
GRAPHS = ("main", "self_loop", "no_edges")
# the operand set with one sh degree zero (sh and sh2): whole paths vanish, M says which elements must be exactly zero
ZERO_DEGREE = {"full_l2_l3max2": 1, "part_l1_mask": 1}


def case_plan(case):
    from e3_layers_amd.nn.core import UVUTensorProduct

    tpm = UVUTensorProduct(case["left"], case["sh"], case["out"])
    if case["y_off_all"]:
        for grp in tpm.plan.groups:
            grp.y_off[0], grp.y_off[1], grp.y_off[2] = 0, 1, 4
    return tpm


def case_graph(case, graph):
    """(n, edge_index): the case's graph; one node with a self-loop; three nodes without an edge"""
    if graph == "main":
        return case["n"], _graph(case["n"], 7 + case["n"])
    return (1, torch.zeros(2, 1, dtype=torch.long)) if graph == "self_loop" else (3, torch.zeros(2, 0, dtype=torch.long))


def case_inputs(case, plan, n, e, graph="main", zero_degree=None):
    """fp32 numpy operands: x, x2, g [N, .]; sh, sh2, w, dw, s2, radius, pre_sh, pre_r [E, .]; T, D, smooth [K + 1, W]"""
    from e3_layers_amd.backend.radial_table import layout

    torch.manual_seed(1000 + CASES.index(case) + 100 * GRAPHS.index(graph))
    d_in, d_sh, W, d_mid = plan.d_in, plan.d_sh, plan.w_numel, plan.d_mid

    def rnd(*shape):
        return torch.randn(*shape, dtype=torch.float64).float().numpy()

    o = dict(x=rnd(n, d_in), x2=rnd(n, d_in), g=rnd(n, d_mid), sh=rnd(e, d_sh), sh2=rnd(e, d_sh), w=rnd(e, W), dw=rnd(e, W), s2=rnd(e))
    radius = (torch.rand(e, dtype=torch.float64).float() * 5.2).numpy()
    radius[:3] = np.array([0.0, 5.0, 0.01], np.float32)[:min(e, 3)]      # r = 0, r = r_max; the rest reach beyond r_max
    knots, h = layout(R_MAX, KNOT_TARGET)
    o.update(radius=radius, T=rnd(knots + 1, W), D=rnd(knots + 1, W), pre_sh=rnd(e, d_sh), pre_r=rnd(e), knots=knots, spacing=h)
    rows, cols = np.arange(knots + 1, dtype=np.float64)[:, None] * h, np.arange(W, dtype=np.float64)[None, :]
    o["smooth"] = (np.sin(rows * (1.0 + 5.0 * cols / W)) * np.exp(-0.2 * rows)).astype(np.float32)
    if zero_degree is not None:
        for grp in plan.groups:
            off = grp.y_off[zero_degree]
            if off >= 0:
                o["sh"][:, off:off + 2 * zero_degree + 1] = 0.0
                o["sh2"][:, off:off + 2 * zero_degree + 1] = 0.0
    return o


def host_bins(radius, knots, spacing):
    """(bin int32 [E], coef fp32 [E, 4]) by the formulas of e3k_rtable_bins (tests/test_gpu_rtable_matrix.py's reference, rounded
    to fp32): what the CPU tests interpolate with.  The GPU test takes the library's."""
    from tests.test_gpu_rtable_matrix import bins_reference

    i, c, _, _ = bins_reference(np.asarray(radius, np.float32), 1.0 / spacing, knots)
    return i.astype(np.int32), c.astype(np.float32)


def host_pack(table, knots):
    """(d0, d1, d2, d3) [K + 1, W] float64 by the formulas of e3k_rtable_pack in include/e3k.h: d2, d3 through fp16 at scales 2^10,
    2^16, d0 and d1 in fp32 with the halves' rounding folded in; rows 0, K - 1 and K zero"""
    from tests.test_gpu_rtable_matrix import taylor64

    b, c1, c2, c3, e2, _ = taylor64(np.asarray(table, np.float32), knots)
    d2 = (e2 * 1024.0).astype(np.float16).astype(np.float64) / 1024.0
    d3 = (c3 * 65536.0).astype(np.float16).astype(np.float64) / 65536.0
    d0 = (b + c1 / 2 + c2 / 4 + c3 / 8 + (e2 - d2) / 8).astype(np.float32).astype(np.float64)
    d1 = (c1 + c2 + 0.75 * c3 + 3.0 * (c3 - d3) / 16).astype(np.float32).astype(np.float64)
    out = [np.zeros((knots + 1, table.shape[1])) for _ in range(4)]
    for full, rows in zip(out, (d0, d1, d2, d3)):
        full[1:knots - 1] = rows
    return out


def operands64(o):
    return {k: np.asarray(o[k], np.float64) for k in ("x", "x2", "g", "sh", "sh2", "s2")}


# C entry and its arguments after the plan, in order (0: a NULL pointer; N, E: the counts); the outputs are named below
SPEC = {
    "fwd": ("e3k_tp_fwd", "x sh w src dst_ptr dst_perm N E out"),
    "bwd_w": ("e3k_tp_bwd_w", "x sh w g src dst_ptr dst_perm N E g_w 0"),
    "bwd_w_sh": ("e3k_tp_bwd_w", "x sh w g src dst_ptr dst_perm N E g_w g_sh"),
    "bwd_x": ("e3k_tp_bwd_x", "sh w g dst src_ptr src_perm N E g_x"),
    "bwd_xw": ("e3k_tp_bwd_xw", "x sh w g dst src_ptr src_perm N E g_x g_w"),
    "fwd_table": ("e3k_tp_fwd_table", "x sh T bin coef src dst_ptr dst_perm N E out"),
    "bwd_x_table": ("e3k_tp_bwd_x_table", "sh T bin coef g dst src_ptr src_perm N E g_x"),
    "fwd_ptable": ("e3k_tp_fwd_ptable", "x P erec_dst dst_ptr N E out"),
    "bwd_x_ptable": ("e3k_tp_bwd_x_ptable", "P erec_src g src_ptr N E g_x"),
    "bwd_xw_ptable": ("e3k_tp_bwd_xw_ptable", "x P erec_src g src_ptr N E g_x g_w"),
    "fwd_jvp_table": ("e3k_tp_fwd_jvp_table", "x x2 sh sh2 T D bin coef s2 src dst_ptr dst_perm N E out"),
    "fwd_jvp": ("e3k_tp_fwd_jvp_table", "x x2 sh sh2 w dw 0 0 s2 src dst_ptr dst_perm N E out"),
    "bwd_x_dual_table": ("e3k_tp_bwd_x_dual_table", "sh sh2 T D bin coef s2 g dst src_ptr src_perm N E g_x"),
    "bwd_x_dual": ("e3k_tp_bwd_x_dual_table", "sh sh2 w dw 0 0 s2 g dst src_ptr src_perm N E g_x"),
    "bwd_xw_dual": ("e3k_tp_bwd_xw_dual", "x x2 sh sh2 w dw s2 g dst src_ptr src_perm N E g_x g_w g_w_plain"),
    "bwd_xe": ("e3k_tp_bwd_xe", "x sh w dw g dst src_ptr src_perm N E g_x g_sh g_r g_w e_partials"),
    "bwd_e_table": ("e3k_tp_bwd_e_table", "x sh T D bin coef g src dst_ptr dst_perm N E g_sh g_r g_w e_partials"),
    "bwd_e": ("e3k_tp_bwd_e_table", "x sh w dw 0 0 g src dst_ptr dst_perm N E g_sh g_r g_w e_partials"),
    "bwd_w_dual": ("e3k_tp_bwd_w_dual", "x x2 sh sh2 g src dst_ptr dst_perm N E g_w"),
}
OUTPUTS = ("out", "g_x", "g_w", "g_w_plain", "g_sh", "g_r", "e_partials")
# with E = 0 these return before any launch (include/e3k.h): every output of theirs is per edge
EDGE_ONLY = ("bwd_w", "bwd_w_sh", "bwd_e", "bwd_e_table", "bwd_w_dual")
NAN32 = np.float32(np.nan)


def _nan_arena(seed):
    """tests/test_gpu_rtable_matrix.py's arena with NaN in the slack and in every block without an initial value: a read
    outside an input poisons the output it feeds"""
    from tests.test_gpu_rtable_matrix import Arena

    class NanArena(Arena):
        def upload(self, dev):
            self.x0 = np.full(self.n + 32, NAN32).view(np.int32).copy()
            for name, init in self.inits:
                off, n = self.blocks[name]
                self.x0[off:off + n] = np.ascontiguousarray(init).ravel().view(np.int32)
            self.buf = torch.from_numpy(self.x0.copy()).to(dev)
            self.base = self.buf.data_ptr()
            assert self.base % 64 == 0
            return self

    return NanArena(seed)


def _run_graph(dev, case, tpm, graph, zero_degree, measured):
    from e3_layers_amd.backend import lib as L
    from e3_layers_amd.backend import radial_table
    from e3_layers_amd.backend.graph import build_topology
    from tests.test_gpu_rtable_matrix import Check

    lib = L.load()
    want, plan = case["routes"], tpm.plan
    h = plan.handle(dev)
    full = case["cell"][3]
    split = full and case["cell"][2]
    main = graph == "main" and zero_degree is None      # (the normwise assertions of the earlier test: on the case's own operands)
    n, ei = case_graph(case, graph)
    e, d_in, d_sh, W, d_mid = ei.shape[1], plan.d_in, plan.d_sh, plan.w_numel, plan.d_mid
    o = case_inputs(case, plan, n, e, graph, zero_degree)
    ref = PlainRef(plan, ei.numpy(), n, full)
    assert ref.split == bool(case["cell"][2]) and int(lib.e3k_tp_edge_partials_floats(h, 5)) == ref.n_gc * 5 * (d_sh + 1)
    assert bool(plan.bwd_x_overwrites(dev)) == (not ref.split and not ref.x_shared and
                                               sum((2 * g.l1 + 1) * g.mul for g in plan.groups) == d_in)
    hub_in, hub_out = [0], [1]                                           # 301 in-edges, 300 out-edges
    no_in, no_out = [n - 1, n - 2], [n - 1, n - 3]
    e_hub = torch.cat([(ei[1] == 0).nonzero().flatten(), (ei[0] == 1).nonzero().flatten()])
    node_rows = hub_in + hub_out

    # ---- the host side of every buffer a call can name
    dst_ptr, dst_perm = host_csr(ei[1].numpy(), n)
    src_ptr, src_perm = host_csr(ei[0].numpy(), n)
    host = {k: o[k] for k in ("x", "x2", "g", "sh", "sh2", "w", "dw", "s2", "T", "D")}
    host.update(src=ei[0].numpy().astype(np.int32), dst=ei[1].numpy().astype(np.int32), dst_ptr=dst_ptr, dst_perm=dst_perm,
                src_ptr=src_ptr, src_perm=src_perm)
    knots = o["knots"]
    smooth_t = torch.from_numpy(o["smooth"]).to(dev)
    packed = radial_table.pack_raw(smooth_t, knots)
    _check_packing(smooth_t, packed, knots)
    host["P"] = packed.cpu().numpy().reshape(-1)
    if e:
        topo = build_topology(ei.to(dev), n)
        for name in ("dst_ptr", "dst_perm", "src_ptr", "src_perm", "src", "dst"):
            assert np.array_equal(getattr(topo, name).cpu().numpy(), host[name]), name
        bins = radial_table.build_bins(torch.from_numpy(o["radius"]).to(dev), R_MAX, KNOT_TARGET)
        assert bins.knots == knots and bins.spacing == o["spacing"]
        host["bin"], host["coef"] = bins.bin.cpu().numpy().copy(), bins.coef.cpu().numpy().copy()
        SH = torch.from_numpy(o["sh"]).to(dev)
        for walk in ("dst", "src"):
            host["erec_" + walk] = (bins.records(topo, SH, walk).cpu().numpy()[:e].copy() if d_sh <= 9
                                    else np.zeros((e, 16), np.int32))
    else:
        host.update(bin=np.zeros(0, np.int32), coef=np.zeros((0, 4), np.float32), erec_dst=np.zeros((0, 16), np.int32),
                    erec_src=np.zeros((0, 16), np.int32))
    n_part = int(lib.e3k_tp_edge_partials_floats(h, e))
    shapes = {"out": (n, d_mid), "g_x": (n, d_in), "g_w": (e, W), "g_w_plain": (e, W), "g_sh": (e, d_sh), "g_r": (e,),
              "e_partials": (max(n_part, 1),)}
    gx0 = NAN32 if plan.bwd_x_overwrites(dev) else np.float32(0.0)      # g_x as documented: written, or zero-filled by the caller

    def route():
        r = lib.e3k_tp_last_route()
        return r.decode() if r is not None else None

    def launch(kind, init=(), null=(), refuse=False):
        """One call with every buffer it names in one NaN arena.  init: {output: initial array}; the others start as NaN (g_x: as
        the header asks).  null: outputs passed as NULL.  Returns the arena's Check."""
        fn, names = SPEC[kind]
        names = names.split()
        ar = _nan_arena(CASES.index(case) * 131 + len(kind))
        init = dict(init)
        for name in dict.fromkeys(names):
            if name in ("0", "N", "E") or name in null:
                continue
            if name in OUTPUTS:
                v = init.get(name, gx0 if name == "g_x" and not refuse else NAN32)
                v = np.full(shapes[name], v, np.float32) if np.ndim(v) == 0 else np.asarray(v, np.float32)
                assert v.shape == shapes[name], (name, v.shape)
            else:
                v = host[name]
            ar.alloc(name, v.size, init=v, align=16)
        ar.upload(dev)
        args = [None if a == "0" or a in null else n if a == "N" else e if a == "E" else ar.p(a) for a in names]
        r0 = route()
        rc = getattr(lib, fn)(h, *args, L.stream_ptr())
        ck = Check(ar, case)
        if refuse:      # E3K_ERR_UNSUPPORTED, nothing launched, every word of the arena keeps its bits
            # (E = 0: a call whose outputs are all per edge returns E3K_OK before it looks at the plan -- include/e3k.h)
            assert rc == (0 if e == 0 and kind in EDGE_ONLY else E3K_ERR_UNSUPPORTED) and route() == r0, kind
            ck.unchanged()
            return ck
        L.check(rc, kind)
        if e == 0 and kind in EDGE_ONLY:
            assert route() == r0, (kind, "launched with E = 0")
        else:
            assert route() == want[kind], (kind, route(), want[kind])
        return ck

    def elementwise(ck, kind, what, refs, pre=None, tag=""):
        """every element of output `what`: |got - ref| <= bound (accumulated outputs: after subtracting the prefill, whose share of
        the m atomic additions the bound gains); M == 0 leaves no room: such an element is exactly zero (or exactly its prefill)"""
        val, bound, m = refs[what]
        ck._claim(what)
        raw = ck.dev(what, np.float32).reshape(val.shape)
        got = raw.astype(np.float64)
        if pre is not None:
            got = got - pre.astype(np.float64)
            bound = bound + gamma(m) * np.abs(pre)
        assert np.isfinite(raw).all(), f"{kind} {what}{tag}: an element was left unwritten or is not finite"
        err = np.abs(got - val)
        bad = np.argwhere(err > bound)
        assert len(bad) == 0, (f"{graph} {kind} {what}{tag}: {len(bad)} of {err.size} elements outside gamma_k M; first at {bad[:4].tolist()}: "
                               f"got {got[tuple(bad[0])]}, want {val[tuple(bad[0])]}, bound {bound[tuple(bad[0])]}")
        live = bound > 0
        r = float((err[live] / bound[live]).max()) if live.any() else 0.0
        key = (kind, what + tag)
        measured[key] = max(measured.get(key, 0.0), r)
        return torch.from_numpy(raw.copy())

    def close(name, got, ref_, tol, rows=(), zero_rows=()):
        """the normwise comparison this test made before it had bounds: kept beside them, on the case's graph and operands"""
        if not main:
            return
        got = got.detach().double().cpu()
        err = rel_err(got, ref_)
        assert err < tol, f"{name}: rel err {err:.3e}"
        rows = torch.as_tensor(list(rows), dtype=torch.long)
        if rows.numel() and float(ref_[rows].norm()) > 0:
            err_r = rel_err(got[rows], ref_[rows])
            assert err_r < tol, f"{name}: rel err {err_r:.3e} on the high-degree rows"
        for r in zero_rows:
            assert bool((got[r] == 0).all()), f"{name}: row {r} of a node without edges is not exactly zero"

    ops = operands64(o)
    t64 = lambda a: torch.from_numpy(np.asarray(a, np.float64))
    streamed, d_streamed = w_streamed(o["w"]), w_streamed(o["dw"])
    ran = set()
    if main:
        orc = _Oracle(case["left"], case["sh"], case["out"], tpm.irreps_mid_simplified, ei, n)
        assert orc.tp.weight_numel == W
        x64, x264, g64, sh64, sh264, w64, dw64, s264 = (t64(o[k]) for k in ("x", "x2", "g", "sh", "sh2", "w", "dw", "s2"))
        ref_out = orc.F(x64, sh64, w64)
        RGx, RGsh, RGw = orc.G(x64, sh64, w64, g64)
    else:
        orc = ref_out = RGx = RGsh = RGw = None

    # ---- weights streamed from w [E, W]
    r = reference(ref, "fwd", ops, streamed)
    ck = launch("fwd")
    close("fwd", elementwise(ck, "fwd", "out", r), ref_out, TOL, node_rows, no_in)
    ck.unchanged()
    r = reference(ref, "bwd_w_sh", ops, streamed)
    ck = launch("bwd_w", null=("g_sh",))
    close("bwd_w g_w", elementwise(ck, "bwd_w", "g_w", r), RGw, GTOL, e_hub)
    ck.unchanged()
    ck = launch("bwd_w_sh", init={"g_sh": o["pre_sh"]})
    close("bwd_w_sh g_w", elementwise(ck, "bwd_w_sh", "g_w", r), RGw, GTOL, e_hub)
    gsh = elementwise(ck, "bwd_w_sh", "g_sh", r, pre=o["pre_sh"])
    close("bwd_w_sh g_sh (accumulated)", gsh.double() - t64(o["pre_sh"]), RGsh, GTOL, e_hub)
    ck.unchanged()
    r = reference(ref, "bwd_xw", ops, streamed)
    ck = launch("bwd_x")
    close("bwd_x", elementwise(ck, "bwd_x", "g_x", r), RGx, GTOL, node_rows, no_out)
    ck.unchanged()
    ck = launch("bwd_xw")
    close("bwd_xw g_x", elementwise(ck, "bwd_xw", "g_x", r), RGx, GTOL, node_rows, no_out)
    close("bwd_xw g_w", elementwise(ck, "bwd_xw", "g_w", r), RGw, GTOL, e_hub)
    ck.unchanged()
    ran.update(FIRST_ORDER)

    later = [k for k in SPEC if k not in FIRST_ORDER]
    if not full:
        for kind in later:
            launch(kind, refuse=True)
        assert ran == set(want) and len(ran) == 5
        return

    # ---- the table forms, packed and not
    tab, d_tab = w_table(o["T"], host["bin"], host["coef"]), w_table(o["D"], host["bin"], host["coef"])
    pk = w_packed([f.numpy() for f in _packed_fields(packed)], host["bin"], host["coef"])
    if main:
        bins_t = type("B", (), {"bin": torch.from_numpy(host["bin"]), "coef": torch.from_numpy(host["coef"])})
        w_tab, dw_tab, w_pk = _interp64(torch.from_numpy(o["T"]), bins_t), _interp64(torch.from_numpy(o["D"]), bins_t), _packed_w64(packed, bins_t)
        assert np.abs(w_tab.numpy() - tab[0]).max() <= 1e-14 and np.abs(w_pk.numpy() - pk[0]).max() <= 1e-14
        TGx, TGsh, _ = orc.G(x64, sh64, w_tab, g64)
        PGx, _, _ = orc.G(x64, sh64, w_pk, g64)
        F_tab, F_pk = orc.F(x64, sh64, w_tab), orc.F(x64, sh64, w_pk)
    else:
        w_tab = dw_tab = w_pk = TGx = TGsh = PGx = F_tab = F_pk = None
    for kind, src, what, old, tol, rows, zero in (
            ("fwd_table", tab, "out", F_tab, TOL, node_rows, no_in), ("bwd_x_table", tab, "g_x", TGx, GTOL, node_rows, no_out),
            ("fwd_ptable", pk, "out", F_pk, TOL, node_rows, no_in), ("bwd_x_ptable", pk, "g_x", PGx, GTOL, node_rows, no_out)):
        ck = launch(kind)
        close(kind, elementwise(ck, kind, what, reference(ref, kind, ops, src)), old, tol, rows, zero)
        ck.unchanged()
        ran.add(kind)
    r = reference(ref, "bwd_xw_ptable", ops, pk)
    ck = launch("bwd_xw_ptable")
    close("bwd_xw_ptable g_x", elementwise(ck, "bwd_xw_ptable", "g_x", r), PGx, GTOL, node_rows, no_out)
    close("bwd_xw_ptable g_w", elementwise(ck, "bwd_xw_ptable", "g_w", r), RGw, GTOL, e_hub)      # (dF/dw does not depend on w)
    ck.unchanged()
    ran.add("bwd_xw_ptable")

    # ---- second order: the product rule along (x2, sh2, s2 dw/dr), and the edge gradients
    def second(suffix, src_w, src_d, w_o, dw_o, Gsh_o):
        """the kinds named `kind + suffix` ("": streamed rows; "_table": both tables), their float64 sums from the oracle beside"""
        if main:
            s2c = s264.unsqueeze(1)
            Gx_sh2, _, _ = orc.G(x64, sh264, w_o, g64)
            Gx_dw, _, _ = orc.G(x64, sh64, s2c * dw_o, g64)
            old_jvp = orc.F(x264, sh64, w_o) + orc.F(x64, sh264, w_o) + orc.F(x64, sh64, s2c * dw_o)
            old_gx, old_gr = Gx_sh2 + Gx_dw, (RGw * dw_o).sum(1)
        else:
            old_jvp = old_gx = old_gr = None
        kind = "fwd_jvp" + suffix
        ck = launch(kind)
        close(kind, elementwise(ck, kind, "out", reference(ref, kind, ops, src_w, src_d)), old_jvp, TOL, node_rows, no_in)
        ck.unchanged()
        kind = "bwd_x_dual" + suffix
        ck = launch(kind)
        close(kind, elementwise(ck, kind, "g_x", reference(ref, kind, ops, src_w, src_d)), old_gx, GTOL, node_rows, no_out)
        ck.unchanged()
        # edge gradients: stored through the per-item partials (NaN in every buffer: all written), and accumulated without them
        kind = "bwd_e" + suffix
        r = reference(ref, kind, ops, src_w, src_d)
        ck = launch(kind)
        close(kind + " g_sh", elementwise(ck, kind, "g_sh", r, tag=" (stored)"), Gsh_o, GTOL, e_hub)
        close(kind + " g_r", elementwise(ck, kind, "g_r", r, tag=" (stored)"), old_gr, GTOL, e_hub)
        close(kind + " g_w", elementwise(ck, kind, "g_w", r), RGw, GTOL, e_hub)
        ck.free("e_partials", n_part)      # (scratch: its contents are not part of the ABI)
        ck.unchanged()
        ck = launch(kind, init={"g_sh": o["pre_sh"], "g_r": o["pre_r"]}, null=("g_w", "e_partials"))
        gsh = elementwise(ck, kind, "g_sh", r, pre=o["pre_sh"])
        gr = elementwise(ck, kind, "g_r", r, pre=o["pre_r"])
        close(kind + " g_sh (accumulated)", gsh.double() - t64(o["pre_sh"]), Gsh_o, GTOL, e_hub)
        close(kind + " g_r (accumulated)", gr.double() - t64(o["pre_r"]), old_gr, GTOL, e_hub)
        ck.unchanged()
        ran.update({"fwd_jvp" + suffix, "bwd_x_dual" + suffix, "bwd_e" + suffix})
        return old_gx, old_gr

    old_gx, old_gr = second("", streamed, d_streamed, w64 if main else None, dw64 if main else None, RGsh)
    old_gw_dual = orc.G(x264, sh64, w64, g64)[2] + orc.G(x64, sh264, w64, g64)[2] if main else None
    r = reference(ref, "bwd_xw_dual", ops, streamed, d_streamed)
    ck = launch("bwd_xw_dual")
    close("bwd_xw_dual g_x", elementwise(ck, "bwd_xw_dual", "g_x", r), old_gx, GTOL, node_rows, no_out)
    close("bwd_xw_dual g_w", elementwise(ck, "bwd_xw_dual", "g_w", r), old_gw_dual, GTOL, e_hub)
    close("bwd_xw_dual g_w_plain", elementwise(ck, "bwd_xw_dual", "g_w_plain", r), RGw, GTOL, e_hub)
    ck.unchanged()
    ck = launch("bwd_w_dual")
    close("bwd_w_dual", elementwise(ck, "bwd_w_dual", "g_w", reference(ref, "bwd_w_dual", ops, streamed)), old_gw_dual, GTOL, e_hub)
    ck.unchanged()
    r = reference(ref, "bwd_xe", ops, streamed, d_streamed)
    ck = launch("bwd_xe")
    close("bwd_xe g_x", elementwise(ck, "bwd_xe", "g_x", r), RGx, GTOL, node_rows, no_out)
    close("bwd_xe g_sh", elementwise(ck, "bwd_xe", "g_sh", r, tag=" (stored)"), RGsh, GTOL, e_hub)
    close("bwd_xe g_r", elementwise(ck, "bwd_xe", "g_r", r, tag=" (stored)"), old_gr, GTOL, e_hub)
    close("bwd_xe g_w", elementwise(ck, "bwd_xe", "g_w", r), RGw, GTOL, e_hub)
    ck.free("e_partials", n_part)
    ck.unchanged()
    ck = launch("bwd_xe", init={"g_sh": o["pre_sh"], "g_r": o["pre_r"]}, null=("g_w", "e_partials"))
    close("bwd_xe g_x (no partials)", elementwise(ck, "bwd_xe", "g_x", r), RGx, GTOL, node_rows, no_out)
    gsh = elementwise(ck, "bwd_xe", "g_sh", r, pre=o["pre_sh"])
    gr = elementwise(ck, "bwd_xe", "g_r", r, pre=o["pre_r"])
    close("bwd_xe g_sh (accumulated)", gsh.double() - t64(o["pre_sh"]), RGsh, GTOL, e_hub)
    close("bwd_xe g_r (accumulated)", gr.double() - t64(o["pre_r"]), old_gr, GTOL, e_hub)
    ck.unchanged()
    ran.update({"bwd_xw_dual", "bwd_w_dual", "bwd_xe"})

    if split:
        for kind in SECOND_TABLE:      # the table second-order forms are not built split
            launch(kind, refuse=True)
    else:
        second("_table", tab, d_tab, w_tab, dw_tab, TGsh)
    assert ran == set(want), sorted(set(want) - ran)


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=[c["id"] for c in CASES])
def test_tp_kernel_matrix_against_float64(dev, case):
    """Every call kind of the case's plan on the case's graph, on a single node with a self-loop, on three nodes without an edge,
    and (two cases) with one sh degree zero: each output element by element inside gamma_k M, every other word of the call's arena
    unchanged, the route, and the normwise comparisons this test made before."""
    from e3_layers_amd.backend import lib as L

    lib = L.load()
    tpm = case_plan(case)
    h = tpm.plan.handle(dev)
    full = case["cell"][3]
    split = full and case["cell"][2]
    assert lib.e3k_tp_table_supported(h) == int(full)
    assert lib.e3k_tp_second_order_streamed_supported(h) == int(full)
    assert lib.e3k_tp_table2_supported(h) == int(full and not split)
    runs = [(g, None) for g in GRAPHS] + ([("main", ZERO_DEGREE[case["id"]])] if case["id"] in ZERO_DEGREE else [])
    for graph, zero_degree in runs:
        measured = {}
        _run_graph(dev, case, tpm, graph, zero_degree, measured)
        tag = graph + ("" if zero_degree is None else f"_sh{zero_degree}_zero")
        for (kind, what), r in sorted(measured.items()):
            print(f"{case['id']} {tag} {kind} {what}: worst error / bound {r:.3f}")
            record_measured("test_gpu_tp_matrix", case=case["id"], graph=tag, kind=kind, output=what, error_over_bound=r)
