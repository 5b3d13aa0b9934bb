"""Every edge-geometry kernel of csrc/e3k_edge.hip (13 instantiations) against float64 on the CPU, element by element.

One case per C-ABI call.  A case lays every operand out in ONE arena of 4-byte words with slack round every block (the arena of
tests/test_gpu_rtable_matrix.py).  Outputs a call overwrites start as NaN (int outputs: a sentinel), the accumulated g_w as random
values.  After the call the WHOLE arena is compared: elements the call writes against the float64 reference under the bounds below,
everything else bit for bit (all of the arena when a call is refused).  No element is masked; where a bound is zero the output must be
exactly zero (or exactly the reference).

References.  float64 on the CPU: oracle/e3ref.py's spherical_harmonics (its F.normalize defines the zero vector and the vector under
the 1e-12 clamp; see normalize64), a torch restatement of BesselBasis x cutoff (x = r / r_max instead of r * (1 / r_max): the comparison x < 1 must
not depend on a float64 rounding; tests/test_edge_inventory.py holds it to e3ref's BesselBasis, poly_cutoff, symmetric_cutoff), and
float64 torch.autograd on them for the first-order results and the Jacobian- / Hessian-vector products of the bwd2 kernels.
edge_vector_bwd: the sum of include/e3k.h restated with np.add.at, its CSR built with a stable argsort.  Radius graph: a numpy
float32 model of the stated arithmetic (unfused products and sums, correctly rounded sqrt, strict <): exact comparison.

Bounds (u = 2^-24; gamma(n) = n u / (1 - n u); every count is an upper estimate of the roundings on the longest path of the kernel
as written, -ffp-contract=fast only removes roundings; sqrtf and / are correctly rounded: the Makefile sets no fast-math flag).

edge_vector_fwd.  vec is one fp32 subtraction: bit-equal to numpy's.  len: three products, two sums (3 u of a positive sum), halved by
  the square root, plus its rounding: 3 u len.  A self-loop: exactly 0.
edge_vector_bwd.  A term is g_vec + (g_len / len) vec: one division, one FMA: 2 u (|g_vec| + |g_len / len| |vec|); a node's n = in +
  out terms are one serial FMA chain (the hub: thousands): gamma(n + 2) sum (|g_vec| + |g_len / len| |vec|).  No term: exactly 0.
spherical harmonics.  MAJORANT: the same polynomial with every coefficient and input replaced by its absolute value and every minus
  by plus (sh_blocks(..., sgn=+1)); float64 autograd of it gives the majorants of the derivatives.  A monomial of degree-l block passes
  at most R_l = 2, 4, 7, 10 roundings (l = 0 .. 3: rounded constants, products, sums, two for the normalization factor: 'component'
  takes them off again, its factor is 1.0f; 'norm' adds rsqrtf: 2 ULP_RSQRT); the forward counts per component (SH_R_M).  Sharper
  still for the three components s15 (a b) of a degree-2 block without normalize under 'component': the representation error of the
  constant (0.474 u) plus u for each of the two products that is inexact in fp32 (_sharpen_s15_products) -- without that no bound
  could tell sqrt(15) from 3.873, a change of 72 u.
  fwd: gamma(R_l + 5 l [normalize]) maj: with normalize u_k = v_k / max(|v|, 1e-12) carries 4.5 u (|v|^2: 3 u, sqrt: 1.5 u + u, the
    reciprocal, the product) and a degree-l monomial l times that.
  bwd: the duals add l + 1 roundings, the FMA chain over the dim outputs dim: raw gradient G within gamma(R + l + 1 + dim + 5 l) M, M =
    majorant gradient with |g_sh|.  normalize: (G - u (u . G)) / |v|: majorant (M_k + |u_k| sum_j M_j |u_j|) / |v|, 15 more roundings
    (the dot product 3 + its inputs 5, the product and the difference 2, 1 / |v| 4, the last product 1).  Under the clamp the divisor is
    the constant 1e-12: no projection (majorant M_k 1e12).
  bwd2, g_gsh = J t: the tangent of u is du = t / |v| - v (v . t) / |v|^3, majorant T_k = (|t_k| + |u_k| sum_j |u_j| |t_j|) / |v|, 20
    roundings (the dual square root and division); gamma(R_l + l + 1 + 5 l + 20) J_abs T.  Without normalize T = |t|.
  bwd2, g_vec: raw H t within gamma(R + 2 l + 2 + dim) HT (HT = majorant Hessian applied to T, with |g_sh|); normalize: the dual of the
    projection: [HT_k + T_k D + |u_k| (sum_j HT_j |u_j| + sum_j M_j T_j)] / |v| + (M_k + |u_k| D) sum_j |u_j t_j| / |v|^2, D = sum_j M_j
    |u_j|, 5 l + 60 more roundings.
  Sub-clamp vectors are only given with normalize (without it their cubes are fp32 subnormals: no relative bound).
radial basis.  out = (2 / delta) sin(w r / delta) c(r) [/ r].  MAJORANT: sin and cos replaced by exp(arg - arg_0) (value and every
  derivative 1 >= |sin^(k)|), 1 / r by 1 / (2 r_0 - r) (derivatives k! / r_0^(k+1)), the cutoff by 1 + c0 x^p + c1 x^(p+1) + c2 x^(p+2)
  resp. (x^2 + 1)^2, all at |r|, |w|, zero beyond the cutoff (the outputs are exactly 0 there); float64 autograd of it per (edge, basis
  function) gives the majorants of every derivative.  This makes the bound ABSOLUTE where the formula cancels (the polynomial near x =
  1, its derivative, cos (w / delta) / r - sin / r^2 at small r).  Relative to the majorant an output carries gamma(C) for the roundings,
  eps_t = k u |arg| + 2 u max(ULP_SIN, ULP_COS) for sin / cos (k = 2: w r / delta in fwd and bwd, delta = r_max - r_min exact in every
  case: asserted; k = 3 in bwd2: (1 / delta) (w r)) and, polynomial cutoff, eps_p = (2 ULP_POW + p) u for powf and the rounding of x.
  C: fwd 14; g_r 17 + n_basis (FMA chain); g_w 16 and the sum; bwd2: g_gout 16, g_r 20 + n_basis, g_w 18 and the sum.
  Sums g_w: (chain length + tree levels + atomics) u (sum |terms| + |old|), any atomic order: bwd: chain ceil(E / (256 blocks)),
  blocks = min(ceil(E / 256), 256), 6 wave levels + 3 for the four waves in LDS + blocks atomics + 1; bwd2: blocks up to 512, 6 levels +
  4 blocks atomics.
  The symmetric cutoff's second derivative jumps at |r| = r_max: its bwd2 cases keep radii 4 ulp away from that point; the
  polynomial cutoff is C^2 there and is tested on the point, one ulp below and above.
radius graph.  Exact: counts and edge_index equal the model, nothing written past E.

Device math library.  sinf / cosf / sincosf / powf / rsqrtf come from the device library; test_device_math_library measures torch's
own float32 sin / cos / pow / rsqrt on the device against numpy float64 over |arg| <= 64 pi 1.2 (10^7 uniform samples, 10^5 log-uniform
small ones, and the fp32 neighbours of k pi and (k - 1/2) pi, k <= 77: the radii on the cutoff), x in (0, 1) with the exponents p, p -
1, p - 2 of the cases' p = 6, 2, 2.5, and 1, 3, 5, 7 for rsqrt.  Measured worst ulp errors on an MI355X: see MEASURED_ULP below; the
constants are the smallest integers >= twice those.

Defects these cases exposed in the kernels as they were (fixed in csrc/e3k_edge.hip):
  rg_planted: the radius graph's distance test was FUSED.  __fmul_rn / __fadd_rn are plain x * y / x + y in this toolchain, contracted
    under -ffp-contract=fast like any other, and __fsqrt_rn is the 1-ulp native square root: 26 of the case's 119 counts differed
    from the stated arithmetic.  Now: products held apart by an empty asm, sqrtf.
  sh_bwd_special_n1, sh_bwd2_special_n1: under the 1e-12 clamp u = v 1e12 is linear in v, but the backward kernels still projected
    (g - u (u . g)): 1.8e4 bounds off on (2e-13, 3e-13, -6e-13).  Now: no projection under the clamp, as F.normalize differentiates.

``CASES`` is a plain table; tests/test_edge_inventory.py holds it to the kernels the library ships, shows the bounds to hold for
float32 models of the forward and first-order kernels and to be sharp against planted mutants (no GPU needed there).
"""
import ctypes as C
import math
import zlib
from fractions import Fraction

import numpy as np
import pytest
import torch

from oracle import e3ref
from tests.test_gpu_rtable_matrix import Arena, Check as _Check
from tests.util import record_measured

pytestmark = pytest.mark.gpu

E3K_OK, E3K_ERR_INVALID, E3K_ERR_UNSUPPORTED = 0, -1, -3
U24 = 2.0 ** -24
SENT = -77777777

# worst ulp error seen on an MI355X (test_device_math_library, fixed seed) and the constants: smallest integer >= 2 x measured
MEASURED_ULP = {"sin": 1.540, "cos": 1.538, "pow": 1.332, "rsqrt": 0.208}
ULP_SIN, ULP_COS, ULP_POW, ULP_RSQRT = 4, 4, 3, 1
POW_EXPONENTS = (6.0, 2.0, 2.5, 5.0, 1.0, 1.5, 4.0, 0.5, 0.0)      # p, p - 1, p - 2 of the cases' p


def gamma(n):
    n = np.asarray(n, np.float64)
    return n * U24 / (1.0 - n * U24)


# ---------------------------------------------------------------------------------------------------------------------------------
# the table's vocabulary
def evf(id_, why, E, N=50, with_len=True):
    return dict(id=id_, kind="evf", why=why, E=E, N=N, with_len=with_len, funcs={"e3k_edge_vector_fwd"},
                kernels={"edge_vector_fwd_kernel"} if E else set())


def evb(id_, why, N, graph="random", g_vec=True, g_len=True):
    return dict(id=id_, kind="evb", why=why, N=N, graph=graph, g_vec=g_vec, g_len=g_len, funcs={"e3k_edge_vector_bwd"},
                kernels={"edge_vector_bwd_kernel"} if N and (g_vec or g_len) else set())


SH_K = {"fwd": "sph_harm_kernel<false>", "bwd": "sph_harm_kernel<true>", "bwd2": "sph_harm_bwd2_kernel"}


def sh(id_, why, op, ls, E=300, vecs="random", normalize=1, normalization=0, outs="both"):
    """op: fwd / bwd / bwd2; vecs: see sh_inputs; outs (bwd2): "gsh", "vec" or "both" """
    return dict(id=id_, kind="sh", why=why, op=op, ls=list(ls), E=E, vecs=vecs, normalize=normalize, normalization=normalization, outs=outs,
                funcs={"e3k_sph_harm_" + op}, kernels={SH_K[op]} if E else set())


def rad(id_, why, op, nb, E=257, cut=0, oor=1, p=6.0, r_min=0.0, radii="uniform", trained=False, outs=None, hats="rw", r_max=4.0):
    """op: fwd / bwd / bwd2; outs: letters of the outputs given (bwd: r, w; bwd2: o (g_gout), r, w); hats (bwd2): r, w or rw"""
    outs = outs or {"fwd": "o", "bwd": "rw", "bwd2": "orw"}[op]
    kern = {"fwd": "radial_fwd_kernel", "bwd": "radial_bwd_kernel<%d>" % (8 if nb <= 8 else 16 if nb <= 16 else 32 if nb <= 32 else 64),
            "bwd2": "radial_bwd2_kernel"}[op]
    return dict(id=id_, kind="rad", why=why, op=op, nb=nb, E=E, cut=cut, oor=oor, p=p, r_min=r_min, r_max=r_max, radii=radii, trained=trained,
                outs=outs, hats=hats, funcs={"e3k_radial_basis_" + op} | ({"e3k_radial_basis_bwd_unroll"} if op == "bwd" else set()),
                kernels={kern} if E else set())


def rg(id_, why, sizes, planted=False, old=False, box=6.0, spread=False):
    return dict(id=id_, kind="rg", why=why, sizes=list(sizes), planted=planted, old=old, box=box, spread=spread,
                funcs={"e3k_radius_graph_count", "e3k_radius_graph_fill"},
                kernels={"radius_graph_kernel<false>"} | (set() if spread else {"radius_graph_kernel<true>"}))


def refuse(id_, why, fn, rc, **over):
    return dict(id=id_, kind="refuse", why=why, fn=fn, rc=rc, over=over, kernels=set(), funcs={"e3k_" + fn})


_CUTS = [(0, 1), (0, 0), (1, 1), (1, 0)]
_SH_LS = [[0], [1], [2], [3], [0, 1, 2], [0, 1, 2, 3], [2, 1], [1, 1], [3] * 8]


def _ls_id(ls):
    return "".join(str(l) for l in ls)


CASES = [
    # ---- edge vectors
    *[evf(f"evf_E{E}", "E at the 256-lane block seams, one edge, none, many blocks; a self-loop, nodes 0 and N - 1; vec bit-equal", E)
      for E in (0, 1, 255, 256, 257, 70001)],
    evf("evf_no_len", "edge_len NULL: vec alone is written", 257, with_len=False),
    evf("evf_two_nodes", "N = 2: every edge between node 0 and node N - 1, or a self-loop", 300, N=2),
    *[evb(f"evb_N{N}", "N at the 256-lane block seams; a node without edges, one with in-edges only, one with out-edges only, a "
          "self-loop, a zero-length edge with g_len", N) for N in (0, 1, 255, 256, 257)],
    evb("evb_hub", "a hub with 3 000 in- and 2 000 out-edges: the long serial FMA chain", 300, graph="hub"),
    evb("evb_no_g_vec", "g_vec NULL: the length term alone", 257, g_vec=False),
    evb("evb_no_g_len", "g_len NULL: edge_vec and edge_len NULL too", 257, g_len=False),
    evb("evb_both_null", "g_vec and g_len NULL: refused, nothing written", 257, g_vec=False, g_len=False),
    # ---- spherical harmonics: degrees x op, flags, vectors, sizes
    *[sh(f"sh_{op}_ls{_ls_id(ls)}", "every degree list: single degrees, ascending, descending, repeated, eight entries of 3 (dim 56)", op, ls)
      for op in ("fwd", "bwd", "bwd2") for ls in _SH_LS],
    *[sh(f"sh_{op}_n{nz}_norm{nn}", "normalize crossed with normalization 0 / 1 / 2 on lengths 1e-6 .. 1e6", op, [0, 1, 2, 3], vecs="lengths",
         normalize=nz, normalization=nn) for op in ("fwd", "bwd", "bwd2") for nz in (0, 1) for nn in (0, 1, 2)],
    *[sh(f"sh_{op}_special_n{nz}", "the six axis vectors (exact zeros), coordinate-plane vectors, the zero vector" +
         (", vectors under the 1e-12 clamp" if nz else ""), op, [0, 1, 2, 3], E=64, vecs="special", normalize=nz)
      for op in ("fwd", "bwd", "bwd2") for nz in (0, 1)],
    *[sh(f"sh_{op}_E{E}", "E at the 256-lane block seams, none, one large", op, [0, 1, 2, 3], E=E)
      for op in ("fwd", "bwd", "bwd2") for E in (0, 255, 256, 257, 70001)],
    sh("sh_fwd_raw_ls2", "degree 2 alone without normalize: the shortest paths (s15 x y: three roundings)", "fwd", [2], normalize=0),
    sh("sh_bwd2_gsh_only", "g_vec NULL (g_sh NULL too): the Jacobian-vector product alone", "bwd2", [0, 1, 2, 3], outs="gsh"),
    sh("sh_bwd2_vec_only", "g_gsh NULL: the Hessian-vector product alone", "bwd2", [0, 1, 2, 3], outs="vec"),
    sh("sh_bwd2_vec_only_raw", "g_gsh NULL, no normalize", "bwd2", [2, 3], outs="vec", normalize=0),
    # ---- radial basis
    *[rad(f"rad_{op}_nb{nb}", "n_basis at and past every unroll bound of radial_bwd_kernel, not a power of two; trained weights", op, nb,
          trained=True) for op in ("fwd", "bwd", "bwd2") for nb in (1, 8, 9, 16, 17, 32, 33, 48, 64)],
    *[rad(f"rad_{op}_E{E}", "E at the 256-lane block seams, none, one", op, 8, E=E) for op in ("fwd", "bwd", "bwd2") for E in (0, 1, 255, 256)],
    *[rad(f"rad_{op}_nb{nb}_E{E}", "E at the start of the grid-stride loops: 65 536 fills radial_bwd's 256 blocks, 65 537 starts its second "
          "round; 131 073 starts radial_bwd2's", op, nb, E=E, radii="uniform") for op in ("bwd", "bwd2") for nb in (8, 64)
      for E in (65536, 65537, 131073)],
    rad("rad_fwd_nb8_E131073", "many blocks of the forward", "fwd", 8, E=131073),
    *[rad(f"rad_{op}_cut{k}_oor{o}_edge", "both cutoff kinds x one_over_r on the edge radii: r_max, one ulp under and over, beyond, r = 1e-3 "
          "with one_over_r, negative and zero r for the symmetric cutoff without it (bwd2 symmetric: 4 ulp from |r| = r_max)", op, 8,
          cut=k, oor=o, radii="edge") for op in ("fwd", "bwd", "bwd2") for k, o in _CUTS],
    *[rad(f"rad_{op}_p{p}", "p = 2 and a non-integer p, edge radii", op, 9, p=p, radii="edge") for op in ("fwd", "bwd", "bwd2")
      for p in (2.0, 2.5)],
    *[rad(f"rad_{op}_rmin", "r_min = 0.5: delta = 3.5 is not r_max; trained weights; edge radii", op, 17, r_min=0.5, trained=True,
          radii="edge", oor=o) for op, o in (("fwd", 1), ("bwd", 0), ("bwd2", 1))],
    rad("rad_bwd_no_g_r", "g_r NULL; g_w accumulated onto old values", "bwd", 16, outs="w"),
    rad("rad_bwd_no_g_w", "g_w NULL", "bwd", 33, outs="r"),
    *[rad(f"rad_bwd2_outs_{o}", "every output subset of bwd2", "bwd2", 9, outs=o, cut=1 if len(o) == 2 else 0)
      for o in ("o", "r", "w", "or", "ow", "rw")],
    rad("rad_bwd2_no_hat_r", "hat_r NULL = zero", "bwd2", 16, hats="w"),
    rad("rad_bwd2_no_hat_w", "hat_w NULL = zero", "bwd2", 16, hats="r", cut=1, oor=0),
    # ---- radius graph
    rg("rg_sizes", "graphs of 1, 63, 64, 65, 129, 150 and 3 nodes (N = 475, not a multiple of 4): one ballot round and several", (1, 63, 64, 65, 129, 150, 3)),
    rg("rg_planted", "pairs the unfused fp32 test keeps and a fused one drops, the reverse, pairs the exact distance decides the other way, "
       "a pair exactly on the cutoff", (), planted=True),
    rg("rg_old_edges", "pre-existing edges longer than the cutoff, one onto node 63 and one onto node 64 of a graph (the ballot-round seam), "
       "one that the distance test keeps anyway", (150, 65, 7), old=True),
    rg("rg_no_edges", "every node alone beyond the cutoff: counts 0, E = 0, fill writes nothing", (5, 1, 1), spread=True),
    # ---- refusals: the return code, and the arena bit-identical
    refuse("refuse_sh_9_degrees", "n_ls = 9", "sph_harm_fwd", E3K_ERR_INVALID, ls=[1] * 9),
    refuse("refuse_sh_l4", "l = 4", "sph_harm_fwd", E3K_ERR_UNSUPPORTED, ls=[0, 4]),
    refuse("refuse_sh_l_negative", "l = -1", "sph_harm_bwd", E3K_ERR_INVALID, ls=[1, -1]),
    refuse("refuse_sh_normalization_3", "normalization 3", "sph_harm_bwd", E3K_ERR_INVALID, normalization=3),
    refuse("refuse_sh_bwd2_l4", "l = 4 in bwd2", "sph_harm_bwd2", E3K_ERR_UNSUPPORTED, ls=[4]),
    refuse("refuse_sh_bwd2_no_output", "g_gsh and g_vec NULL", "sph_harm_bwd2", E3K_ERR_INVALID, g_gsh=None, g_vec=None),
    refuse("refuse_sh_bwd2_g_vec_without_g_sh", "g_vec without g_sh", "sph_harm_bwd2", E3K_ERR_INVALID, g_sh=None),
    refuse("refuse_sh_fwd_null_out", "sh NULL", "sph_harm_fwd", E3K_ERR_INVALID, sh=None),
    refuse("refuse_rad_nb0", "n_basis 0", "radial_basis_fwd", E3K_ERR_INVALID, nb=0),
    refuse("refuse_rad_nb65", "n_basis 65", "radial_basis_fwd", E3K_ERR_INVALID, nb=65),
    refuse("refuse_rad_bwd_nb65", "n_basis 65", "radial_basis_bwd", E3K_ERR_INVALID, nb=65),
    refuse("refuse_rad_bwd2_nb65", "n_basis 65", "radial_basis_bwd2", E3K_ERR_INVALID, nb=65),
    refuse("refuse_rad_rmax_eq_rmin", "r_max = r_min", "radial_basis_fwd", E3K_ERR_INVALID, r_min=4.0),
    refuse("refuse_rad_bwd_rmax_below_rmin", "r_max < r_min", "radial_basis_bwd", E3K_ERR_INVALID, r_min=5.0),
    refuse("refuse_rad_bwd2_rmax_nan", "r_max NaN", "radial_basis_bwd2", E3K_ERR_INVALID, r_max=float("nan")),
    refuse("refuse_rad_cutoff_2", "cutoff_kind 2", "radial_basis_fwd", E3K_ERR_INVALID, cut=2),
    refuse("refuse_rad_bwd_cutoff_2", "cutoff_kind 2", "radial_basis_bwd", E3K_ERR_INVALID, cut=2),
    refuse("refuse_rad_bwd2_cutoff_negative", "cutoff_kind -1", "radial_basis_bwd2", E3K_ERR_INVALID, cut=-1),
    refuse("refuse_rad_bwd_no_output", "g_r and g_w NULL", "radial_basis_bwd", E3K_ERR_INVALID, g_r=None, g_w=None),
    refuse("refuse_rad_bwd2_no_hat", "hat_r and hat_w NULL", "radial_basis_bwd2", E3K_ERR_INVALID, hat_r=None, hat_w=None),
    refuse("refuse_rad_bwd2_no_output", "g_gout, g_r and g_w NULL", "radial_basis_bwd2", E3K_ERR_INVALID, g_gout=None, g_r=None, g_w=None),
    refuse("refuse_rad_E_negative", "E < 0", "radial_basis_fwd", E3K_ERR_INVALID, E=-1),
    refuse("refuse_evf_null_vec", "edge_vec NULL", "edge_vector_fwd", E3K_ERR_INVALID, vec=None),
    refuse("refuse_evb_g_len_without_len", "g_len without edge_len", "edge_vector_bwd", E3K_ERR_INVALID, len=None),
    refuse("refuse_rg_old_ptr_without_old_dst", "old_ptr without old_dst", "radius_graph_count", E3K_ERR_INVALID, old_dst=None),
    refuse("refuse_rg_fill_old_ptr_without_old_dst", "old_ptr without old_dst", "radius_graph_fill", E3K_ERR_INVALID, old_dst=None),
    refuse("refuse_rg_N_negative", "N < 0", "radius_graph_count", E3K_ERR_INVALID, N=-1),
]


def table_kernels():
    return set().union(*(c["kernels"] for c in CASES))


def table_functions():
    return set().union(*(c["funcs"] for c in CASES))


def _rng(c):
    return np.random.default_rng(zlib.crc32(c["id"].encode()))


# ---------------------------------------------------------------------------------------------------------------------------------
# edge vectors
def evf_inputs(c):
    rng, E, N = _rng(c), c["E"], c["N"]
    pos = (2.0 * rng.standard_normal((N, 3))).astype(np.float32)
    src, dst = rng.integers(0, N, E).astype(np.int32), rng.integers(0, N, E).astype(np.int32)
    if E >= 4:
        src[0] = dst[0] = N // 2
        src[1], dst[1], src[2], dst[2] = 0, N - 1, N - 1, 0
    elif E == 1:
        src[0], dst[0] = 0, N - 1
    return dict(pos=pos, src=src, dst=dst)


def evf_reference(inp):
    """(vec fp32: exact, len float64, bound)"""
    vec = inp["pos"][inp["dst"]] - inp["pos"][inp["src"]]
    ln = np.sqrt((vec.astype(np.float64) ** 2).sum(-1))
    return vec, ln, 3 * U24 * ln


def evb_inputs(c):
    rng, N = _rng(c), c["N"]
    pos = (2.0 * rng.standard_normal((N, 3))).astype(np.float32)
    edges = []
    role = {}
    if N >= 8:
        lone, sink, source, loop, za, zb = (int(v) for v in rng.permutation(N)[:6])
        role = dict(lone=lone, sink=sink, source=source, loop=loop, za=za, zb=zb)
        pos[zb] = pos[za]
        free = np.array([n for n in range(N) if n not in (lone, sink, source)])
        m = 4 * N
        edges += list(zip(free[rng.integers(0, len(free), m)], free[rng.integers(0, len(free), m)]))
        edges += [(int(free[k]), sink) for k in range(3)] + [(source, int(free[k])) for k in range(4)] + [(loop, loop), (za, zb), (zb, za)]
        if c["graph"] == "hub":
            hub = int(free[7])
            role["hub"] = hub
            edges += [(int(free[k]), hub) for k in rng.integers(0, len(free), 3000)] + [(hub, int(free[k])) for k in rng.integers(0, len(free), 2000)]
    elif N >= 1:
        edges += [(int(a), int(b)) for a, b in zip(rng.integers(0, N, 5), rng.integers(0, N, 5))]
    e = np.array(edges, np.int64).reshape(-1, 2)
    e = e[rng.permutation(len(e))]
    src, dst = e[:, 0].astype(np.int32), e[:, 1].astype(np.int32)
    E = len(src)
    vec = pos[dst] - pos[src]
    ln = np.sqrt((vec[:, 0] * vec[:, 0] + vec[:, 1] * vec[:, 1]) + vec[:, 2] * vec[:, 2])
    csr = {}
    for name, idx in (("dst", dst), ("src", src)):
        csr[name + "_perm"] = np.argsort(idx, kind="stable").astype(np.int32)
        csr[name + "_ptr"] = np.concatenate([[0], np.cumsum(np.bincount(idx, minlength=N))]).astype(np.int32)
    return dict(N=N, src=src, dst=dst, vec=vec, len=ln.astype(np.float32), g_vec=rng.standard_normal((E, 3)).astype(np.float32),
                g_len=rng.standard_normal(E).astype(np.float32), role=role, **csr)


def evb_reference(inp, g_vec=True, g_len=True, mutant=None):
    """g_pos [N, 3] float64 and its bound.  mutants: "src_sign" (out-edges added), "no_inv_len" (g_len vec instead of g_len vec / len)"""
    N, src, dst = inp["N"], inp["src"], inp["dst"]
    E = len(src)
    gv, mag = np.zeros((E, 3)), np.zeros((E, 3))
    if g_vec:
        gv += inp["g_vec"].astype(np.float64)
        mag += np.abs(inp["g_vec"].astype(np.float64))
    if g_len:
        ln = inp["len"].astype(np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            f = np.where(ln > 0, inp["g_len"].astype(np.float64) / (1.0 if mutant == "no_inv_len" else ln), 0.0)
        gv += f[:, None] * inp["vec"].astype(np.float64)
        mag += np.abs(f[:, None] * inp["vec"].astype(np.float64))
    want, tot = np.zeros((N, 3)), np.zeros((N, 3))
    np.add.at(want, dst, gv)
    np.add.at(want, src, gv if mutant == "src_sign" else -gv)
    np.add.at(tot, dst, mag)
    np.add.at(tot, src, mag)
    n = np.bincount(dst, minlength=N) + np.bincount(src, minlength=N)
    return want, np.where(n[:, None] > 0, gamma(n + 2)[:, None] * tot, 0.0)


# ---------------------------------------------------------------------------------------------------------------------------------
# spherical harmonics
S3, S5, S15, S7 = math.sqrt(3.0), math.sqrt(5.0), math.sqrt(15.0), math.sqrt(7.0)
SH_A, SH_B = math.sqrt(42.0) / 6.0, math.sqrt(168.0) / 8.0
SH_R = (2, 4, 7, 10)                                   # the longest path of a block, the two roundings of the normalization factor included
SH_R_M = ((2,), (4, 4, 4), (5, 5, 7, 5, 6), (10,) * 7)      # ... per component
NORMALIZATIONS = ("component", "integral", "norm")


def sh_dim(ls):
    return sum(2 * l + 1 for l in ls)


def sh_blocks(ls, vec, normalization, sgn=-1.0, mutant=None):
    """sgn = -1: the real harmonics of include/e3k.h at vec [E, 3] (torch float64), [E, dim]; sgn = +1: their majorant (vec >= 0).
    mutants: "s15" (sqrt(15) truncated to 3.873), "swap_m1" (l = 3: m = -1 and m = +1 exchanged), "norm_2l1" ('norm' as 1 / (2 l + 1))"""
    x, y, z = vec[..., 0], vec[..., 1], vec[..., 2]
    s15 = 3.873 if mutant == "s15" else S15
    x2, yy, z2 = x * x, y * y, z * z
    x2z2 = x2 + z2
    q = [s15 * x * z, s15 * x * y, S5 * (yy + sgn * 0.5 * x2z2), s15 * y * z, 0.5 * s15 * (z2 + sgn * x2)]
    f = 4.0 * yy + sgn * x2z2
    blocks = []
    for l in ls:
        if l == 0:
            b = [torch.ones_like(x)]
        elif l == 1:
            b = [S3 * x, S3 * y, S3 * z]
        elif l == 2:
            b = q
        else:
            b = [SH_A * (q[0] * z + q[4] * x), S7 * q[0] * y, SH_B * f * x, 0.5 * S7 * y * (2.0 * yy + sgn * 3.0 * x2z2), SH_B * z * f,
                 S7 * q[4] * y, SH_A * (q[4] * z + sgn * q[0] * x)]
            if mutant == "swap_m1":
                b[2], b[4] = b[4], b[2]
        nf = 1.0 if normalization == 0 else 1.0 / math.sqrt(4.0 * math.pi) if normalization == 1 else \
            (1.0 / (2 * l + 1) if mutant == "norm_2l1" else 1.0 / math.sqrt(2 * l + 1))
        blocks.append(nf * torch.stack(b, -1))
    return torch.cat(blocks, -1)


def normalize64(v):
    """torch.nn.functional.normalize(v, dim=-1) = v / max(|v|, 1e-12) to float64 rounding (tests/test_edge_inventory.py), written so that the
    clamped branch differentiates as the constant it is: autograd's SECOND derivative of F.normalize is NaN at the zero vector (the
    norm's), where the function is the linear map v 1e12"""
    s = (v * v).sum(-1, keepdim=True)
    n = torch.sqrt(torch.where(s > 0, s, torch.ones_like(s)))
    return v / torch.where((s > 0) & (n > 1e-12), n, torch.full_like(n, 1e-12))


def sh_function(ls, normalize, normalization, mutant=None):
    """vec [E, 3] float64 -> sh [E, dim]: e3ref.spherical_harmonics, or the restatement carrying a mutant"""
    if mutant is None:
        return lambda v: e3ref.spherical_harmonics(ls, normalize64(v) if normalize else v, False, NORMALIZATIONS[normalization])
    if mutant == "no_projection":      # (1 / |v| held constant in every derivative)
        return lambda v: sh_blocks(ls, v / v.detach().norm(dim=-1, keepdim=True).clamp_min(1e-12) if normalize else v, normalization)
    return lambda v: sh_blocks(ls, normalize64(v) if normalize else v, normalization, mutant=mutant)


def _grad(out, inp, go=None, keep=True):
    (g,) = torch.autograd.grad(out, inp, go, create_graph=keep, allow_unused=True)
    return torch.zeros_like(inp) if g is None else g


def per_edge_derivatives(fn, v, g, t):
    """fn: [E, 3] -> [E, dim], edge by edge.  Returns Y, J^T g [E, 3], J t [E, dim], d/d eps (J(v + eps t)^T g) [E, 3] by float64
    autograd (the Jacobian-vector product through the double-backward trick)"""
    v = v.clone().requires_grad_(True)
    Y = fn(v) + 0.0 * v.sum(-1, keepdim=True)
    w = torch.ones_like(Y, requires_grad=True)
    G = _grad(Y, v, w)
    jvp = _grad((G * t).sum() + 0.0 * w.sum(), w, keep=False)
    B = _grad(Y, v, g) + 0.0 * v
    hvp = _grad((B * t).sum(), v, keep=False)
    return Y.detach(), B.detach(), jvp.detach(), hvp.detach()


def sh_inputs(c):
    rng, E = _rng(c), c["E"]
    dim = sh_dim(c["ls"]) if all(0 <= l <= 3 for l in c["ls"]) else 1
    v = 2.0 * rng.standard_normal((E, 3))
    if c["vecs"] == "lengths":
        v = v / np.linalg.norm(v, axis=1, keepdims=True) * 10.0 ** rng.uniform(-6, 6, (E, 1))
    elif c["vecs"] == "special":
        sp = [[2, 0, 0], [-2, 0, 0], [0, 2, 0], [0, -2, 0], [0, 0, 2], [0, 0, -2], [0, 0, 1], [0, -3, 0], [1e5, 0, 0], [0, 0, -1e-4],
              [1.5, -0.7, 0], [0, 0.3, 2.2], [-1.1, 0, 0.4], [1, 1, 0], [0, 1, -1], [1, 0, 1], [0, 0, 0]]
        if c["normalize"]:
            sp += [[3e-13, -4e-13, 0], [0, 0, 1e-13], [2e-13, 3e-13, -6e-13], [1e-20, 0, 0]]
        v[:len(sp)] = sp
    return dict(vec=v.astype(np.float32), g_sh=rng.standard_normal((E, dim)).astype(np.float32),
                g_hat=rng.standard_normal((E, 3)).astype(np.float32))


S15_REPR = abs(float(np.float32(S15)) - S15) / S15 / U24      # 0.474: the fp32 constant is that many u from sqrt(15)


def _sharpen_s15_products(ls, vec32, want, bound):
    """The components s15 (a b) of a degree-2 block, without normalize and under 'component' (factor 1.0f): the constant's own
    representation error, plus u for each of the two products that is INEXACT in fp32 (decided with a float32 model of that one
    product: a property of the format).  At a b a power of two the error is the constant's alone: 0.474 u.  In place."""
    off = 0
    for l in ls:
        if l == 2:
            for m, (i, j) in ((0, (0, 2)), (1, (0, 1)), (3, (1, 2))):
                a, b = vec32[:, i], vec32[:, j]
                ab = a * b
                n1 = ab.astype(np.float64) != a.astype(np.float64) * b.astype(np.float64)
                n2 = (np.float32(S15) * ab).astype(np.float64) != float(np.float32(S15)) * ab.astype(np.float64)
                bound[:, off + m] = (S15_REPR + n1 + n2) * U24 * (1.0 + 1e-9) * np.abs(want[:, off + m])      # (1e-9: this line's own float64)
        off += 2 * l + 1


def sh_reference(c, inp, mutant=None):
    """{output: (want, bound)} of the case's op, float64.  Outputs: sh | g_vec | g_gsh, g_vec2"""
    ls, nz, nn = c["ls"], c["normalize"], c["normalization"]
    v, g, t = (torch.from_numpy(inp[k].astype(np.float64)) for k in ("vec", "g_sh", "g_hat"))
    if mutant == "hessian_const_inv":
        # the first-order formula written out with 1 / |v| a constant of the differentiation (also inside u)
        assert nz
        vv = v.clone().requires_grad_(True)
        inv = 1.0 / v.norm(dim=-1, keepdim=True).clamp_min(1e-12)
        uu = vv * inv
        G = _grad(sh_blocks(ls, uu, nn) + 0.0 * uu.sum(-1, keepdim=True), uu, g) + 0.0 * uu
        B = (G - uu * (uu * G).sum(-1, keepdim=True)) * inv
        hvp = _grad((B * t).sum(), vv, keep=False).detach()
        Y, B0, jvp, _ = per_edge_derivatives(sh_function(ls, nz, nn), v, g, t)
    else:
        Y, B0, jvp, hvp = per_edge_derivatives(sh_function(ls, nz, nn, mutant), v, g, t)
    # ---- majorants at a = |u|
    nrm = v.norm(dim=-1, keepdim=True)
    clamped = (nrm <= 1e-12) if nz else torch.zeros_like(nrm, dtype=torch.bool)
    inv = 1.0 / nrm.clamp_min(1e-12) if nz else torch.ones_like(nrm)
    a = (v * inv).abs()
    ta, ga = t.abs(), g.abs()
    T = torch.where(clamped, ta * inv, (ta + a * (a * ta).sum(-1, keepdim=True)) * inv) if nz else ta
    absf = lambda vv: sh_blocks(ls, vv, nn, sgn=+1.0)
    Ya, M, JT, HT = per_edge_derivatives(absf, a, ga, T)
    D = (M * a).sum(-1, keepdim=True)
    lm, dim = max(ls), sh_dim(ls)
    rs = 2 * ULP_RSQRT if nn == 2 else -2 if nn == 0 else 0      # ('component': the factor is 1.0f, exact)
    col_l = np.concatenate([[l] * (2 * l + 1) for l in ls])
    R = np.concatenate([SH_R_M[l] for l in ls]) + rs
    out = {}
    if c["op"] == "fwd":
        bound = gamma(R + 5 * col_l * nz)[None, :] * Ya.numpy()
        if not nz and nn == 0:
            _sharpen_s15_products(ls, inp["vec"], Y.numpy(), bound)
        out["sh"] = (Y, bound)
    elif c["op"] == "bwd":
        Cb = SH_R[lm] + rs + lm + 1 + dim + nz * (5 * lm + 15)
        maj = torch.where(clamped, M * inv, (M + a * D) * inv) if nz else M
        out["g_vec"] = (B0, gamma(Cb) * maj.numpy())
    else:
        out["g_gsh"] = (jvp, gamma(R + col_l + 1 + nz * (5 * col_l + 20))[None, :] * JT.numpy())
        Ch = SH_R[lm] + rs + 2 * lm + 2 + dim + nz * (5 * lm + 60)
        if nz:
            Ie = (a * ta).sum(-1, keepdim=True) * inv * inv
            full = (HT + T * D + a * ((HT * a).sum(-1, keepdim=True) + (M * T).sum(-1, keepdim=True))) * inv + (M + a * D) * Ie
            maj = torch.where(clamped, HT * inv, full)
        else:
            maj = HT
        out["g_vec2"] = (hvp, gamma(Ch) * maj.numpy())
    res = {}
    for k, (w, b) in out.items():
        w = w.numpy()
        assert np.isfinite(w).all() and np.isfinite(b).all(), f"the reference of {k} is not finite"
        res[k] = (w, b)
    return res


# ---------------------------------------------------------------------------------------------------------------------------------
# radial basis
def rad_params(c):
    f = lambda v: float(np.float32(v))
    prm = dict(r_max=f(c["r_max"]), r_min=f(c["r_min"]), p=f(c["p"]), oor=c["oor"], cut=c["cut"])
    assert f(np.float32(prm["r_max"]) - np.float32(prm["r_min"])) == prm["r_max"] - prm["r_min"], "delta must be exact in fp32"
    return prm


def rad_formula(R, W, prm, absf=False, mutant=None):
    """out(r, w) = (2 / delta) sin(w r / delta) c(r) [/ r], elementwise in torch float64; absf: the majorant (R, W >= 0)"""
    r_max, p = prm["r_max"], prm["p"]
    delta = r_max if mutant == "delta_is_r_max" else r_max - prm["r_min"]
    arg = W * R / delta
    x = R / r_max
    if absf:
        s = torch.exp(arg - arg.detach())
        inv_r = 1.0 / (2.0 * R.detach() - R) if prm["oor"] else 1.0
        sg = 1.0
    else:
        s = torch.sin(arg)
        inv_r = 1.0 / R if prm["oor"] else 1.0
        sg = -1.0
    if prm["cut"] == 0:
        xs = torch.where(x < 1.0, x, torch.zeros_like(x))      # (beyond the cutoff the value is 0 whatever x^p is)
        t0, t1, t2 = ((p + 1.0) * (p + 2.0) / 2.0) * xs ** p, p * (p + 2.0) * xs ** (p + 1.0), (p * (p + 1.0) / 2.0) * xs ** (p + 2.0)
        cc = (1.0 + t0 + t1 + t2 if absf else 1.0 - t0 + t1 - t2) * (x < 1.0)
    else:
        cc = (x * x + sg) ** 2 * (x.abs() < 1.0)
    return (2.0 / delta) * s * inv_r * cc


def rad_derivatives(r, w, prm, absf=False, second=False, mutant=None, chunk=16384):
    """out, f_R, f_W (and f_RR, f_RW, f_WR, f_WW) per (edge, basis function), [E, nb] float64, by autograd on operands broadcast to
    [E, nb] (every element its own scalar problem)"""
    nb = len(w)
    keys = ["out", "fR", "fW"] + (["fRR", "fRW", "fWR", "fWW"] if second else [])
    parts = {k: [] for k in keys}
    for lo in range(0, max(len(r), 1), chunk):
        rr = torch.from_numpy(r[lo:lo + chunk])
        R = rr[:, None].expand(len(rr), nb).clone().requires_grad_(True)
        W = torch.from_numpy(w)[None, :].expand(len(rr), nb).clone().requires_grad_(True)
        out = rad_formula(R, W, prm, absf, mutant)
        fR, fW = torch.autograd.grad(out.sum(), (R, W), create_graph=second)
        vals = [out, fR, fW]
        if second:
            vals += list(torch.autograd.grad(fR.sum(), (R, W), retain_graph=True)) + list(torch.autograd.grad(fW.sum(), (R, W)))
        for k, v in zip(keys, vals):
            parts[k].append(v.detach().numpy())
    return {k: np.concatenate(v, 0) for k, v in parts.items()}


def rad_inputs(c):
    rng, E, nb = _rng(c), c["E"], max(min(c["nb"], 64), 1)
    r_max = np.float32(c["r_max"])
    r = rng.uniform(0.1, 1.15, E) * float(r_max)
    if c["radii"] == "edge":
        up = lambda v, k: np.float32(v) + np.float32(k) * np.spacing(np.float32(v))
        sym2 = c["cut"] == 1 and c["op"] == "bwd2"
        sp = [up(r_max, -4), up(r_max, 4)] if sym2 else [r_max, np.nextafter(r_max, np.float32(0)), np.nextafter(r_max, np.float32(9))]
        sp += [1.5 * r_max, 0.999 * r_max, 0.5 * r_max]
        if c["oor"]:
            sp += [1e-3, 2e-3]
        elif c["cut"] == 1:
            sp += [0.0, -0.3 * r_max, -1.2 * r_max, -up(r_max, -4), -up(r_max, 4), -1e-3] + ([] if sym2 else [-r_max, -np.nextafter(r_max, np.float32(0))])
        r[rng.permutation(E)[:len(sp)]] = sp[:E]
    w = np.arange(1, nb + 1) * math.pi
    if c["trained"]:
        w = w * (1.0 + 0.05 * rng.standard_normal(nb))
    return dict(r=r.astype(np.float32), w=w.astype(np.float32), g=rng.standard_normal((E, nb)).astype(np.float32),
                hat_r=rng.standard_normal(E).astype(np.float32), hat_w=rng.standard_normal(nb).astype(np.float32),
                old_w=rng.standard_normal(nb).astype(np.float32))


def rad_sum_terms(op, E):
    """roundings of the summation of one g_w entry (chain + tree + atomics)"""
    if E == 0:
        return 0
    blocks = min(-(-E // 256), 256 if op == "bwd" else 512)
    chain = -(-E // (256 * blocks))
    return chain + 6 + 3 + blocks + 1 if op == "bwd" else chain + 6 + 4 * blocks


RAD_C = dict(fwd=14, g_r=17, g_w=16, gout2=16, g_r2=20, g_w2=18)


def rad_reference(c, inp, mutant=None):
    """{output: (want, bound)} of the case's op: out | g_r, g_w | g_gout, g_r2, g_w2 (every output, whatever subset the case asks for)"""
    prm, op, nb, E = rad_params(c), c["op"], len(inp["w"]), len(inp["r"])
    r, w, g = inp["r"].astype(np.float64), inp["w"].astype(np.float64), inp["g"].astype(np.float64)
    hr = inp["hat_r"].astype(np.float64) if "r" in c["hats"] else np.zeros(E)
    hw = inp["hat_w"].astype(np.float64) if "w" in c["hats"] else np.zeros(nb)
    old = inp["old_w"].astype(np.float64)
    second = op == "bwd2"
    d = rad_derivatives(r, w, prm, second=second, mutant=mutant)
    m = rad_derivatives(np.abs(r), np.abs(w), prm, absf=True, second=second)
    arg = np.abs(r[:, None] * w[None, :]) / (prm["r_max"] - prm["r_min"])
    eps_p = (2 * ULP_POW + prm["p"]) * U24 if prm["cut"] == 0 else 0.0
    k = 3 if second else 2
    eps_t = k * U24 * arg + 2 * U24 * (ULP_SIN if op == "fwd" else max(ULP_SIN, ULP_COS))
    ga, hra, hwa = np.abs(g), np.abs(hr)[:, None], np.abs(hw)[None, :]
    ns = rad_sum_terms(op, E)
    if op == "fwd":
        return dict(out=(d["out"], (gamma(RAD_C["fwd"]) + eps_t + eps_p) * m["out"]))
    if op == "bwd":
        tr, tw = ga * m["fR"], ga * m["fW"]
        return dict(g_r=((g * d["fR"]).sum(1), ((gamma(RAD_C["g_r"] + nb) + eps_t + eps_p) * tr).sum(1)),
                    g_w=(old + (g * d["fW"]).sum(0), ((gamma(RAD_C["g_w"]) + eps_t + eps_p) * tw).sum(0) + gamma(ns) * (tw.sum(0) + np.abs(old))))
    t2r, t2w = ga * (m["fRR"] * hra + m["fRW"] * hwa), ga * (m["fWR"] * hra + m["fWW"] * hwa)
    return dict(g_gout=(d["fR"] * hr[:, None] + d["fW"] * hw[None, :], (gamma(RAD_C["gout2"]) + eps_t + eps_p) * (m["fR"] * hra + m["fW"] * hwa)),
                g_r2=((g * (d["fRR"] * hr[:, None] + d["fRW"] * hw[None, :])).sum(1), ((gamma(RAD_C["g_r2"] + nb) + eps_t + eps_p) * t2r).sum(1)),
                g_w2=(old + (g * (d["fWR"] * hr[:, None] + d["fWW"] * hw[None, :])).sum(0),
                      ((gamma(RAD_C["g_w2"]) + eps_t + eps_p) * t2w).sum(0) + gamma(ns) * (t2w.sum(0) + np.abs(old))))


def rad_bwd_explicit(inp, prm, mutant=None):
    """(g_r, g_w without the old values) from the first-order formulas of the kernel written out in numpy float64.
    mutants: "no_sin_r2" (dbasis without - pref sin / r^2), "c1_p" (c1 (p + 1) replaced by c1 p in dc)"""
    r, w, g = inp["r"].astype(np.float64)[:, None], inp["w"].astype(np.float64)[None, :], inp["g"].astype(np.float64)
    r_max, p = prm["r_max"], prm["p"]
    delta = r_max - prm["r_min"]
    pref, x = 2.0 / delta, r / r_max
    with np.errstate(invalid="ignore", divide="ignore"):
        if prm["cut"] == 1:
            q = x * x - 1.0
            cc, dc = np.where(np.abs(x) < 1, q * q, 0.0), np.where(np.abs(x) < 1, 4.0 * q * x / r_max, 0.0)
        else:
            c0, c1, c2 = (p + 1) * (p + 2) / 2, p * (p + 2), p * (p + 1) / 2
            xs = np.where(x < 1, x, 0.0)
            cc = np.where(x < 1, 1 - c0 * xs ** p + c1 * xs ** (p + 1) - c2 * xs ** (p + 2), 0.0)
            dc = np.where(x < 1, (-c0 * p * xs ** (p - 1) + c1 * (p if mutant == "c1_p" else p + 1) * xs ** p - c2 * (p + 2) * xs ** (p + 1)) / r_max, 0.0)
        inv_r = 1.0 / r if prm["oor"] else np.ones_like(r)
    sn, cs = np.sin(w * r / delta), np.cos(w * r / delta)
    dbasis = pref * cs * (w / delta) * inv_r
    if prm["oor"] and mutant != "no_sin_r2":
        dbasis = dbasis - pref * sn * inv_r * inv_r
    return (g * (dbasis * cc + pref * sn * inv_r * dc)).sum(1), (g * pref * cs * (r / delta) * inv_r * cc).sum(0)


# ---------------------------------------------------------------------------------------------------------------------------------
# radius graph
RG_RMAX = 4.0


def rg_keep_unfused(pi, pj, r_max=RG_RMAX):
    """the stated arithmetic in numpy float32: every product and sum rounded, correctly rounded sqrt, strict <"""
    d = pi.astype(np.float32) - pj.astype(np.float32)
    d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    assert d2.dtype == np.float32
    return np.sqrt(d2) < np.float32(r_max)


def rg_keep_fused(pi, pj, r_max=RG_RMAX):
    """what -ffp-contract=fast would make of dx dx + dy dy + dz dz: fma(dz, dz, fma(dy, dy, dx dx)); the exact products are formed in
    float64 (48 bits: exact), each sum rounded to fp32"""
    d = (pi.astype(np.float32) - pj.astype(np.float32)).astype(np.float64)
    a = (d[..., 0] * d[..., 0]).astype(np.float32).astype(np.float64)
    a = (d[..., 1] * d[..., 1] + a).astype(np.float32).astype(np.float64)
    a = (d[..., 2] * d[..., 2] + a).astype(np.float32)
    return np.sqrt(a) < np.float32(r_max)


def rg_keep_exact(pi, pj, r_max=RG_RMAX):
    """the exact distance of the fp32 positions against r_max, in rational arithmetic"""
    pi, pj = np.atleast_2d(pi), np.atleast_2d(pj)
    out = np.zeros(len(pi), bool)
    for k in range(len(pi)):
        d2 = sum((Fraction(float(a)) - Fraction(float(b))) ** 2 for a, b in zip(pi[k], pj[k]))
        out[k] = d2 < Fraction(float(np.float32(r_max))) ** 2
    return out


RG_CLASSES = ("unfused_keeps_fused_drops", "unfused_drops_fused_keeps", "unfused_keeps_exact_drops", "unfused_drops_exact_keeps")


def rg_planted_pairs(n_per_class=6):
    """{class: (pos_i [n, 3], pos_j [n, 3])} fp32: pairs within 3e-7 (relative) of r_max, found by search on the CPU"""
    rng = np.random.default_rng(77)
    found = {k: ([], []) for k in RG_CLASSES}
    while any(len(v[0]) < n_per_class for v in found.values()):
        pi = rng.uniform(-3, 3, (200000, 3)).astype(np.float32)
        dr = rng.standard_normal((200000, 3))
        dr /= np.linalg.norm(dr, axis=1, keepdims=True)
        pj = (pi.astype(np.float64) + dr * RG_RMAX * (1.0 + rng.uniform(-3e-7, 3e-7, (200000, 1)))).astype(np.float32)
        ku, kf = rg_keep_unfused(pi, pj), rg_keep_fused(pi, pj)
        d = pi.astype(np.float64) - pj.astype(np.float64)
        ke = (d * d).sum(-1) < RG_RMAX ** 2      # (float64 for the search; rg_keep_exact decides the planted ones)
        for name, sel in zip(RG_CLASSES, (ku & ~kf, ~ku & kf, ku & ~ke, ~ku & ke)):
            for k in np.flatnonzero(sel)[:50]:
                if len(found[name][0]) < n_per_class and ("exact" not in name or rg_keep_exact(pi[k], pj[k])[0] == ke[k]):
                    found[name][0].append(pi[k])
                    found[name][1].append(pj[k])
    return {k: (np.array(a), np.array(b)) for k, (a, b) in found.items()}


def rg_inputs(c):
    rng = _rng(c)
    graphs = []
    for n in c["sizes"]:
        graphs.append(rng.uniform(0, c["box"], (n, 3)).astype(np.float32) if not c["spread"] else
                      (100.0 * np.arange(n)[:, None] + rng.uniform(0, 1, (n, 3))).astype(np.float32))
    if c["planted"]:
        pairs = rg_planted_pairs()
        # every class in a graph of its own: 2 n nodes, pair k = nodes (k, n + k); a far translation would change the roundings, so the
        # pairs stay where they were found and the other pairs of the graph are decided by the same model
        for name in RG_CLASSES:
            graphs.append(np.concatenate(pairs[name], 0))
        graphs.append(np.array([[0, 0, 0], [RG_RMAX, 0, 0], [1, 2, 3], [1, 2 + RG_RMAX, 3], [0.5, 0.5, 0.5]], np.float32))      # on the cutoff
        graphs.append(rng.uniform(0, 6, (66, 3)).astype(np.float32))
    pos = np.concatenate(graphs, 0)
    sizes = [len(g) for g in graphs]
    start = np.repeat(np.cumsum([0] + sizes[:-1]), sizes).astype(np.int32)
    end = np.repeat(np.cumsum(sizes), sizes).astype(np.int32)
    old_ptr = old_dst = None
    if c["old"]:
        N = len(pos)
        rows = {i: set() for i in range(N)}
        far = lambda i, j: not rg_keep_unfused(pos[i], pos[j])
        # graph 0 (150 nodes): onto nodes 63 and 64 (the last lane of the first ballot round, the first of the second), 127, 128, 149, 0
        for i, j in [(5, 63), (5, 64), (5, 127), (5, 128), (5, 149), (149, 0), (64, 63), (63, 64), (0, 149), (100, 3)]:
            rows[i].add(j)
        for i in range(150):      # (one long row: every far node of node 77)
            if i != 77 and far(77, i):
                rows[77].add(i)
        near = [j for j in range(150) if j != 9 and not far(9, j)]
        rows[9].add(near[0] if near else 10)      # (kept by the distance test anyway: not counted twice)
        rows[150 + 64].add(150)      # graph 1 (65 nodes): its last node onto its first
        rows[150].add(150 + 64)
        cnt = [len(rows[i]) for i in range(N)]
        old_ptr = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int32)
        old_dst = np.array([j for i in range(N) for j in sorted(rows[i])], np.int32)
        assert sum(far(i, j) for i in rows for j in rows[i]) >= 20
    return dict(pos=pos, start=start, end=end, old_ptr=old_ptr, old_dst=old_dst)


def rg_reference(inp, keep=rg_keep_unfused):
    """counts [N] int32 and edge_index [2, E] int64 of the model"""
    pos, start, end = inp["pos"], inp["start"], inp["end"]
    N = len(pos)
    src, dst, counts = [], [], np.zeros(N, np.int32)
    for i in range(N):
        j = np.arange(start[i], end[i])
        k = keep(np.broadcast_to(pos[i], (len(j), 3)), pos[j]) & (j != i)
        if inp["old_ptr"] is not None:
            k |= np.isin(j, inp["old_dst"][inp["old_ptr"][i]:inp["old_ptr"][i + 1]])
        counts[i] = k.sum()
        src += [i] * int(k.sum())
        dst += list(j[k])
    return counts, np.array([src, dst], np.int64).reshape(2, -1)


# ---------------------------------------------------------------------------------------------------------------------------------
class Check(_Check):
    def finish(self):
        self.unchanged()
        for family, r in self.ratios.items():
            print(f"{self.case['id']}: {family} worst error / bound {r:.3f}")
            record_measured("test_gpu_edge_matrix", case=self.case["id"], family=family, error_over_bound=r)


def _arena(c):
    return Arena(zlib.crc32(c["id"].encode()) ^ 0x5A5A)


NANF = np.float32(np.nan)


def run_evf(dev, c, L):
    lib, st = L.load(), L.stream_ptr()
    inp = evf_inputs(c)
    E = c["E"]
    ar = _arena(c)
    ar.alloc("pos", inp["pos"].size, inp["pos"]).alloc("src", E, inp["src"]).alloc("dst", E, inp["dst"]).alloc("vec", 3 * E, NANF).alloc("len", E, NANF)
    ar.upload(dev)
    rc = lib.e3k_edge_vector_fwd(ar.p("pos"), ar.p("src"), ar.p("dst"), E, ar.p("vec"), ar.p("len") if c["with_len"] else None, st)
    assert rc == E3K_OK
    ck = Check(ar, c)
    vec, ln, bound = evf_reference(inp)
    if E:
        ck.exact("vec", vec)
        if c["with_len"]:
            ck.close("len", ln, bound, "edge_vector_fwd")
    ck.finish()


def run_evb(dev, c, L):
    lib, st = L.load(), L.stream_ptr()
    inp = evb_inputs(c)
    N, E = c["N"], len(inp["src"])
    ar = _arena(c)
    for k in ("g_vec", "g_len", "vec", "len", "dst_ptr", "dst_perm", "src_ptr", "src_perm"):
        ar.alloc(k, inp[k].size, inp[k])
    ar.alloc("g_pos", 3 * N, NANF).upload(dev)
    gl = c["g_len"]
    rc = lib.e3k_edge_vector_bwd(ar.p("g_vec") if c["g_vec"] else None, ar.p("g_len") if gl else None, ar.p("vec") if gl else None,
                                 ar.p("len") if gl else None, ar.p("dst_ptr"), ar.p("dst_perm"), ar.p("src_ptr"), ar.p("src_perm"), N, ar.p("g_pos"), st)
    ck = Check(ar, c)
    if not (c["g_vec"] or gl):
        assert rc == E3K_ERR_INVALID
    else:
        assert rc == E3K_OK
        if N:
            want, bound = evb_reference(inp, c["g_vec"], gl)
            if inp["role"]:
                assert (bound[inp["role"]["lone"]] == 0).all() and (want[inp["role"]["lone"]] == 0).all()
            ck.close("g_pos", want, bound, "edge_vector_bwd")
    ck.finish()


def _ls_array(ls):
    return (C.c_int32 * max(len(ls), 1))(*ls)


def run_sh(dev, c, L):
    lib, st = L.load(), L.stream_ptr()
    inp = sh_inputs(c)
    E, dim, op = c["E"], sh_dim(c["ls"]), c["op"]
    ar = _arena(c)
    ar.alloc("vec", 3 * E, inp["vec"]).alloc("g_sh", E * dim, inp["g_sh"]).alloc("g_hat", 3 * E, inp["g_hat"])
    ar.alloc("sh", E * dim, NANF).alloc("g_vec", 3 * E, NANF).alloc("g_gsh", E * dim, NANF).alloc("g_vec2", 3 * E, NANF)
    ar.upload(dev)
    ls, n, nz, nn = _ls_array(c["ls"]), len(c["ls"]), c["normalize"], c["normalization"]
    if op == "fwd":
        rc, outs = lib.e3k_sph_harm_fwd(ar.p("vec"), E, ls, n, nz, nn, ar.p("sh"), st), ["sh"]
    elif op == "bwd":
        rc, outs = lib.e3k_sph_harm_bwd(ar.p("vec"), ar.p("g_sh"), E, ls, n, nz, nn, ar.p("g_vec"), st), ["g_vec"]
    else:
        o = c["outs"]
        rc = lib.e3k_sph_harm_bwd2(ar.p("vec"), ar.p("g_sh") if o != "gsh" else None, ar.p("g_hat"), E, ls, n, nz, nn,
                                   ar.p("g_gsh") if o != "vec" else None, ar.p("g_vec2") if o != "gsh" else None, st)
        outs = [k for k, on in (("g_gsh", o != "vec"), ("g_vec2", o != "gsh")) if on]
    assert rc == E3K_OK
    ck = Check(ar, c)
    if E:
        ref = sh_reference(c, inp)
        for k in outs:
            ck.close(k, ref[k][0], ref[k][1], "sph_harm_" + op)
    ck.finish()


def run_rad(dev, c, L):
    lib, st = L.load(), L.stream_ptr()
    inp = rad_inputs(c)
    prm = rad_params(c)
    E, nb, op, o = c["E"], c["nb"], c["op"], c["outs"]
    ar = _arena(c)
    ar.alloc("r", E, inp["r"]).alloc("w", nb, inp["w"]).alloc("g", E * nb, inp["g"]).alloc("hat_r", E, inp["hat_r"]).alloc("hat_w", nb, inp["hat_w"])
    ar.alloc("out", E * nb, NANF).alloc("g_r", E, NANF).alloc("g_w", nb, inp["old_w"]).upload(dev)
    args = (nb, prm["r_max"], prm["r_min"], prm["p"], prm["oor"], prm["cut"])
    if op == "fwd":
        rc, outs = lib.e3k_radial_basis_fwd(ar.p("r"), E, ar.p("w"), *args, ar.p("out"), st), [("out", "out")]
    elif op == "bwd":
        assert lib.e3k_radial_basis_bwd_unroll(nb) == int(next(iter(rad("x", "x", "bwd", nb)["kernels"])).split("<")[1][:-1])
        rc = lib.e3k_radial_basis_bwd(ar.p("r"), ar.p("g"), E, ar.p("w"), *args, ar.p("g_r") if "r" in o else None, ar.p("g_w") if "w" in o else None, st)
        outs = [(k, k) for k in ("g_r", "g_w") if k[-1] in o]
    else:
        rc = lib.e3k_radial_basis_bwd2(ar.p("r"), ar.p("g"), ar.p("hat_r") if "r" in c["hats"] else None, ar.p("hat_w") if "w" in c["hats"] else None,
                                       E, ar.p("w"), *args, ar.p("out") if "o" in o else None, ar.p("g_r") if "r" in o else None,
                                       ar.p("g_w") if "w" in o else None, st)
        outs = [(k, ref) for k, ref, on in (("out", "g_gout", "o" in o), ("g_r", "g_r2", "r" in o), ("g_w", "g_w2", "w" in o)) if on]
    assert rc == E3K_OK
    ck = Check(ar, c)
    if E:
        ref = rad_reference(c, inp)
        for k, name in outs:
            want, bound = ref[name]
            assert np.isfinite(want).all() and np.isfinite(bound).all(), f"the reference of {name} is not finite"
            ck.close(k, want, bound, "radial_basis_" + op)
    ck.finish()


def run_rg(dev, c, L):
    lib, st = L.load(), L.stream_ptr()
    inp = rg_inputs(c)
    counts, ei = rg_reference(inp)
    N, E = len(inp["pos"]), ei.shape[1]
    assert c["id"] != "rg_sizes" or N % 4 != 0
    assert (E == 0) == c["spread"]
    offsets = (np.cumsum(counts.astype(np.int64)) - counts).astype(np.int64)
    ar = _arena(c)
    ar.alloc("pos", 3 * N, inp["pos"]).alloc("start", N, inp["start"]).alloc("end", N, inp["end"]).alloc("counts", N, np.int32(SENT))
    ar.alloc("offsets", 2 * N, offsets.view(np.int32), align=2).alloc("ei", 4 * E, np.int32(SENT), align=2)
    if c["old"]:
        ar.alloc("old_ptr", N + 1, inp["old_ptr"]).alloc("old_dst", len(inp["old_dst"]), inp["old_dst"])
    ar.upload(dev)
    op, od = (ar.p("old_ptr"), ar.p("old_dst")) if c["old"] else (None, None)
    assert lib.e3k_radius_graph_count(ar.p("pos"), ar.p("start"), ar.p("end"), N, RG_RMAX, op, od, ar.p("counts"), st) == E3K_OK
    ck = Check(ar, c)      # the counts BEFORE the fill is launched: it places its writes by them
    ck.exact("counts", counts)
    ck.unchanged()
    assert lib.e3k_radius_graph_fill(ar.p("pos"), ar.p("start"), ar.p("end"), N, RG_RMAX, op, od, ar.p("offsets"), E, ar.p("ei"), st) == E3K_OK
    ck = Check(ar, c)
    ck.exact("counts", counts)
    if E:
        ck.exact("ei", ei.view(np.int32))
    ck.ratio("radius_graph", 0.0)
    ck.finish()


def run_refuse(dev, c, L):
    """A small valid problem of every entry point, one argument replaced: the return code, and the arena bit-identical."""
    lib, st = L.load(), L.stream_ptr()
    ar = _arena(c)
    E, nb, N, dim = 10, 8, 6, 16
    a = dict(E=E, nb=nb, N=N, ls=[0, 1, 2, 3], normalization=0, r_max=4.0, r_min=0.0, cut=0)
    ar.alloc("vec", 3 * E).alloc("g_sh", E * 56).alloc("g_hat", 3 * E).alloc("sh", E * 56).alloc("g_vec", 3 * E).alloc("g_gsh", E * 56)
    ar.alloc("r", E, ar.rng.uniform(0.5, 3.5, E).astype(np.float32)).alloc("w", 65).alloc("g", E * 65).alloc("hat_r", E).alloc("hat_w", 65)
    ar.alloc("g_gout", E * 65).alloc("g_r", E).alloc("g_w", 65).alloc("pos", 3 * N).alloc("src", E, np.zeros(E, np.int32)).alloc("dst", E, np.ones(E, np.int32))
    ar.alloc("len", E).alloc("g_len", E).alloc("g_pos", 3 * N)
    ptr = np.array([0, 0, E, E, E, E, E], np.int32)
    ar.alloc("dst_ptr", N + 1, ptr).alloc("src_ptr", N + 1, np.array([0, E, E, E, E, E, E], np.int32)).alloc("perm", E, np.arange(E, dtype=np.int32))
    ar.alloc("start", N, np.zeros(N, np.int32)).alloc("end", N, np.full(N, N, np.int32)).alloc("counts", N).alloc("old_ptr", N + 1, np.zeros(N + 1, np.int32))
    ar.alloc("old_dst", 4).alloc("offsets", 2 * N, np.zeros(2 * N, np.int32), align=2).alloc("ei", 4 * 30, align=2)
    ar.upload(dev)
    a.update({k: k for k in ar.blocks})
    a.update(c["over"])
    p = lambda k: ar.p(a[k])
    ls, fn = _ls_array(a["ls"]), c["fn"]
    rargs = (a["nb"], a["r_max"], a["r_min"], 6.0, 1, a["cut"])
    if fn == "sph_harm_fwd":
        rc = lib.e3k_sph_harm_fwd(p("vec"), a["E"], ls, len(a["ls"]), 1, a["normalization"], p("sh"), st)
    elif fn == "sph_harm_bwd":
        rc = lib.e3k_sph_harm_bwd(p("vec"), p("g_sh"), a["E"], ls, len(a["ls"]), 1, a["normalization"], p("g_vec"), st)
    elif fn == "sph_harm_bwd2":
        rc = lib.e3k_sph_harm_bwd2(p("vec"), p("g_sh"), p("g_hat"), a["E"], ls, len(a["ls"]), 1, a["normalization"], p("g_gsh"), p("g_vec"), st)
    elif fn == "radial_basis_fwd":
        rc = lib.e3k_radial_basis_fwd(p("r"), a["E"], p("w"), *rargs, p("g_gout"), st)
    elif fn == "radial_basis_bwd":
        rc = lib.e3k_radial_basis_bwd(p("r"), p("g"), a["E"], p("w"), *rargs, p("g_r"), p("g_w"), st)
    elif fn == "radial_basis_bwd2":
        rc = lib.e3k_radial_basis_bwd2(p("r"), p("g"), p("hat_r"), p("hat_w"), a["E"], p("w"), *rargs, p("g_gout"), p("g_r"), p("g_w"), st)
    elif fn == "edge_vector_fwd":
        rc = lib.e3k_edge_vector_fwd(p("pos"), p("src"), p("dst"), a["E"], p("vec"), p("len"), st)
    elif fn == "edge_vector_bwd":
        rc = lib.e3k_edge_vector_bwd(p("g_vec"), p("g_len"), p("vec"), p("len"), p("dst_ptr"), p("perm"), p("src_ptr"), p("perm"), a["N"], p("g_pos"), st)
    elif fn == "radius_graph_count":
        rc = lib.e3k_radius_graph_count(p("pos"), p("start"), p("end"), a["N"], RG_RMAX, p("old_ptr"), p("old_dst"), p("counts"), st)
    else:
        assert fn == "radius_graph_fill"
        rc = lib.e3k_radius_graph_fill(p("pos"), p("start"), p("end"), a["N"], RG_RMAX, p("old_ptr"), p("old_dst"), p("offsets"), 30, p("ei"), st)
    assert rc == c["rc"], f"return code {rc}"
    Check(ar, c).finish()


RUNNERS = dict(evf=run_evf, evb=run_evb, sh=run_sh, rad=run_rad, rg=run_rg, refuse=run_refuse)


@pytest.mark.parametrize("c", CASES, ids=[c["id"] for c in CASES])
def test_edge_case_against_float64(dev, c):
    from e3_layers_amd.backend import lib as L

    RUNNERS[c["kind"]](dev, c, L)


# ---------------------------------------------------------------------------------------------------------------------------------
def _worst_ulp(got32, ref64):
    sp = np.spacing(np.abs(ref64).astype(np.float32)).astype(np.float64)
    return float((np.abs(got32.astype(np.float64) - ref64) / sp).max())


def math_library_samples():
    """the arguments the cases give sin / cos (|arg| <= 64 pi 1.2) and pow (x in (0, 1)), fp32"""
    rng = np.random.default_rng(2024)
    n = 10_000_000
    amax = 64 * math.pi * 1.2
    kpi = (np.arange(1, 78) * math.pi).astype(np.float32)
    near = np.concatenate([kpi, np.nextafter(kpi, np.float32(0)), np.nextafter(kpi, np.float32(1e9)), ((np.arange(1, 78) - 0.5) * math.pi).astype(np.float32)])
    arg = np.concatenate([rng.uniform(-amax, amax, n).astype(np.float32), (10.0 ** rng.uniform(-6, 0, 100000)).astype(np.float32), near, -near])
    x = np.concatenate([rng.uniform(0, 1, n).astype(np.float32), (10.0 ** rng.uniform(-6, 0, 100000)).astype(np.float32)])
    return arg, x[(x > 0) & (x < 1)]


def test_device_math_library(dev):
    """The device library's float32 sin / cos / pow / rsqrt (through torch, not through the kernels under test) against numpy float64:
    twice the worst ulp error must stay within ULP_SIN, ULP_COS, ULP_POW, ULP_RSQRT, the constants every radial bound uses."""
    arg, x = math_library_samples()
    t = torch.from_numpy(arg).to(dev)
    worst = dict(sin=_worst_ulp(torch.sin(t).cpu().numpy(), np.sin(arg.astype(np.float64))),
                 cos=_worst_ulp(torch.cos(t).cpu().numpy(), np.cos(arg.astype(np.float64))))
    tx = torch.from_numpy(x).to(dev)
    worst["pow"] = max(_worst_ulp(torch.pow(tx, p).cpu().numpy(), x.astype(np.float64) ** p) for p in POW_EXPONENTS)
    v = np.array([1, 3, 5, 7], np.float32)
    worst["rsqrt"] = _worst_ulp(torch.rsqrt(torch.from_numpy(v).to(dev)).cpu().numpy(), 1.0 / np.sqrt(v.astype(np.float64)))
    chosen = dict(sin=ULP_SIN, cos=ULP_COS, pow=ULP_POW, rsqrt=ULP_RSQRT)
    for k, w in worst.items():
        print(f"device math library: {k} worst {w:.3f} ulp, constant {chosen[k]}")
        record_measured("test_gpu_edge_matrix", case="device_math_library", family=k, worst_ulp=w, constant=chosen[k])
    for k, w in worst.items():
        assert 2.0 * w <= chosen[k], f"{k}: worst error {w} ulp, the bounds assume at most {chosen[k]} / 2"
    assert ULP_SIN <= 4 and ULP_COS <= 4 and ULP_POW <= 16      # (the OpenCL full-profile limits)
