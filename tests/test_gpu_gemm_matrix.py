"""Every GEMM kernel and dispatch rule of csrc/e3k_gemm.hip against float64 on the CPU.

One case per call.  A case lays its problems out in one float32 arena, with slack rows and columns around every A, A2, B, C and bias
block, runs one C-ABI call, asserts the exact launch record of ``e3k_gemm_last_routes()`` and compares the whole arena afterwards:

* every element the call writes against a float64 reference built from the formulas of include/e3k.h (strided rows, ``row_index``,
  key groups, the outer product, ``+C``, bias, the shifted-softplus epilogue, ``+=`` for weight gradients);
* every other element bit for bit: slack columns and rows, rows outside every key group, the other keys' B slices, and all of the
  arena when the call is refused.

Outputs a call overwrites start as NaN; accumulated outputs and weight gradients start as random values.

Bound, per element (u = 2^-24, the fp32 unit roundoff).  An output is a sum of n products plus at most two addends (bias, old C),
formed by fp32 FMA chains in some order (MFMA, split-K partials, atomics, one alpha scaling per K-chain link).  Its error is at most
gamma_{n + 8} |terms| <= (n + 8) u (|alpha| (|A| |B|) + |bias| + |C_old|) elementwise; (n + 8) u < 1e-4 here, so gamma's first-order
form holds with room.  With the activation y = c (softplus(x) - log 2), |dy/dx| <= c: the bound becomes c (bound_x + 16 u (|x| + 1))
(expf, log1pf and the subtraction of log 2 each a few ulps of |x| + log 2).  n is K (sum of the links' K for a chain) for outputs of
the forward, and the number of summed rows for weight gradients and the reductions.  The bound is worst case: one missing, repeated
or misplaced row, column, key or K-tail term moves an element by about one |a b| term, far above it on most elements.

``CASES`` is a plain table; tests/test_gemm_inventory.py holds its routes to the kernels the library ships (no GPU needed there).
"""
import zlib

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

E3K_OK, E3K_ERR_INVALID, E3K_ERR_UNSUPPORTED = 0, -1, -3
MAX_ROWS = 2 ** 31 - 2 ** 16      # E3K_GEMM_MAX_ROWS
U24 = 2.0 ** -24
LOG2 = float(np.log(2.0))


# ---------------------------------------------------------------------------------------------------------------------------------
# the table's vocabulary
def pr(M1, M2, K, N, *, lay="cf", lay_c=None, a="vec", bm=1, acc=0, bias=False, act=0, cst=1.7, alpha=0.71, V=0, gather=False,
       g=True, links=(), empty=False):
    """One problem.  lay: A (and C) rows "cf" ([M2][K], a_k = 1) or "e3nn" ([K][M2], a_k = M2); lay_c: C's, when it differs.
    a: "vec" (16-byte-loadable A), "mis" (base 4 bytes past a 16-byte boundary), "r1" (a_r1 not a multiple of 4), "any" (whatever
    the layout gives).  bm: B mode 1 (n-contiguous), 2 (k-contiguous), 0 (scalar: a row stride that is not a multiple of 4).
    V > 0: outer form, K = U * V.  gather: rows through row_index (non-keyed).  g: weight gradients, G (in C) 16-byte-loadable or not.
    links: the K-chain's followers, dicts of K, bm, alpha, a.  empty: M1 = 0 and NULL pointers."""
    return dict(M1=M1, M2=M2, K=K, N=N, lay=lay, lay_c=lay_c or lay, a=a, bm=bm, acc=acc, bias=bias, act=act, cst=cst, alpha=alpha,
                V=V, gather=gather, g=g, links=[dict(dict(K=K, bm=bm, alpha=alpha, a=a), **l) for l in links], empty=empty)


def seg(*probs, keys=None, rebase=False):
    """keys: dict(sizes=[count of key t], spare=rows of the permutation outside every group); group starts are shuffled.
    rebase: pointer fields hold byte offsets, M1 comes from the segment (the templates carry a wrong one)."""
    return dict(probs=list(probs), keys=keys, rebase=rebase)


def case(id_, entry, segs, route, why, rc=E3K_OK, wgrad=False):
    return dict(id=id_, entry=entry, segs=segs, route=route, why=why, rc=rc, wgrad=wgrad or entry == "wgrad")


G1 = "gemm_kernel<2, false>"
GC = "gemm_kernel<2, true>"
SK = "gemm_splitk_kernel"
OU = "gemm_outer_kernel"
W2 = "gemm_wgrad2_kernel"


def _r(*parts):
    return ";".join(parts)


def _many(n, K=64, N=64, M1=70):
    return [pr(M1 + i, 1, K, N, bm=1 + i % 2, acc=i % 2) for i in range(n)]


# fctp_reduce and colsum have their own argument lists
def fctp(M1, M2, U, V, *, acc=0, mis=False):
    return dict(M1=M1, M2=M2, U=U, V=V, acc=acc, mis=mis)


CASES = [
    # ---- the plain forward kernel: operand paths, layouts, tails, epilogues
    case("fwd_interior_bias_act", "gemm", [seg(pr(128, 1, 64, 128, bias=True, act=1))], f"{G1}[1]",
         "interior tiles only (2 x 2 tiles of 64): bias and ssp in the straight-line epilogue"),
    case("fwd_edge_acc_bias_act", "gemm", [seg(pr(65, 1, 96, 65, bm=2, acc=1, bias=True, act=1))], f"{G1}[1]",
         "rows and columns one past a tile: per-element epilogue with +C, bias and ssp"),
    case("fwd_m2_layouts", "gemm",
         [seg(*[pr(37 + m2, m2, k, 64 + 8 * i, lay=lay, a="vec" if lay == "cf" or m2 == 1 else "any", acc=i % 2)
                for i, (m2, lay, k) in enumerate([(1, "cf", 40), (3, "cf", 24), (5, "cf", 72), (7, "cf", 100), (1, "e3nn", 36),
                                                  (3, "e3nn", 20), (5, "e3nn", 33), (7, "e3nn", 64)])])],
         f"{G1}[8]", "M2 in {1, 3, 5, 7} in both stride layouts (e3nn: a_k = M2, scalar A); K tails 40, 72, 100, 33; K < 32"),
    case("fwd_operand_paths", "gemm",
         [seg(pr(90, 3, 64, 64, a="vec", bm=1), pr(91, 3, 64, 64, lay="e3nn", a="any", bm=2), pr(92, 3, 64, 68, a="mis", bm=0),
              pr(93, 3, 64, 60, a="r1", bm=2, acc=1))],
         f"{G1}[4]", "float4 A; scalar A from a_k != 1, from a misaligned base, from a_r1 % 4 != 0; B modes 1, 2, 0"),
    case("fwd_empty_between", "gemm", [seg(pr(64, 1, 32, 64), pr(0, 1, 32, 64, empty=True), pr(129, 1, 32, 64, acc=1))], f"{G1}[2]",
         "an empty problem (M1 = 0, NULL pointers) between live ones; 129 rows: one past two tiles"),
    case("fwd_one_column", "gemm",
         [seg(pr(301, 3, 96, 1, lay="e3nn", a="any", bm=0, bias=True, act=1), pr(64, 1, 64, 1, bm=2, acc=1),
              pr(77, 1, 64, 1, bm=2, gather=True, bias=True), pr(50, 1, 64, 64))],
         _r("gemm_n1_kernel", "gemm_n1_kernel", f"{G1}[2]"),
         "N = 1: a wave per row, with bias + ssp and with +C; N = 1 with row_index stays on the tile kernel"),
    # ---- split-K and the ride-along rules
    case("splitk_epilogues", "gemm",
         [seg(pr(40, 1, 1024, 96, bm=2, bias=True, act=1), pr(64, 1, 256, 64, bm=2, acc=1),
              pr(11, 3, 512, 40, bm=2, acc=1, bias=True))],
         f"{SK}[3]", "few rows, K % 64 == 0: four waves split K; 32-row tiles full and partial; bias, +C, ssp"),
    case("ride_along_splitk_into_plain", "gemm", [seg(pr(300, 1, 96, 64), pr(40, 1, 512, 64, bm=2, acc=1))], f"{G1}[2]",
         "a K <= 512 split-K problem joins its plain sibling's launch"),
    case("ride_along_plain_into_splitk", "gemm", [seg(pr(30, 1, 1024, 64, bm=2), pr(100, 1, 128, 64, bm=2, bias=True))], f"{SK}[2]",
         "a small plain problem with K >= 128 joins its split-K sibling"),
    # ---- the outer form (self-connection)
    case("outer_fwd", "gemm",
         [seg(pr(129, 3, 20 * 8, 64, V=8, a="any", bias=True, act=1), pr(128, 1, 3 * 32, 72, V=32, lay="e3nn", a="any", bm=0, acc=1),
              pr(60, 5, 7 * 5, 64, V=5, lay="e3nn", a="any", bm=2, gather=True, acc=1))],
         f"{OU}[3]", "x (x) attrs formed in LDS: 129 x 3 rows (edge tile), V = 32, V = 5 with gathered rows (A2 through row_index)"),
    # ---- K-chains
    case("chain_two_links", "gemm", [seg(pr(200, 1, 64, 96, bm=2, alpha=1e-3, links=[dict(K=256, alpha=1.0)], bias=True, act=1))],
         f"{GC}[2]", "two links whose alphas differ by 10^3: the ratio rescale between links; bias + ssp on the last link"),
    case("chain_three_links", "gemm",
         [seg(pr(95, 3, 40, 72, acc=1, alpha=0.5, links=[dict(K=64, bm=2, alpha=500.0), dict(K=24, a="vec", alpha=-0.7)]),
              pr(70, 1, 64, 64))],
         _r(f"{GC}[4]"), "three links with K tails, +C; an unchained problem shares the launch"),
    case("chain_straddles_launch", "gemm",
         [seg(*_many(18, K=96), pr(66, 1, 16, 64, alpha=2.0, links=[dict(K=24, alpha=2e3), dict(K=40, alpha=0.3)]))],
         _r(f"{G1}[18]", f"{GC}[3]"), "18 problems, then a 3-link chain (smallest total K, so last) that would straddle the 20"),
    case("chain_follower_refused", "gemm", [seg(pr(64, 1, 64, 64, links=[dict(K=32, N=68)]))],
         "", "a follower that does not repeat its head's N: refused, nothing launched", rc=E3K_ERR_INVALID),
    # ---- batching
    case("batch_21", "gemm", [seg(*_many(21))], _r(f"{G1}[20]", f"{G1}[1]"), "21 problems: 20 per launch"),
    case("batch_64", "gemm", [seg(*_many(64, M1=3))], _r(f"{G1}[20]", f"{G1}[20]", f"{G1}[20]", f"{G1}[4]"), "64: the most per call"),
    case("batch_65_refused", "gemm", [seg(*_many(65, M1=3))], "", "65 problems: refused", rc=E3K_ERR_INVALID),
    case("rebased_a2_bias", "rebased",
         [seg(pr(150, 3, 6 * 4, 64, V=4, a="any", bias=True), pr(150, 3, 48, 64, bias=True, acc=1), rebase=True)],
         _r(f"{G1}[1]", f"{OU}[1]"), "byte offsets; A2 and bias as offset + 1; M1 from the call"),
    case("multi_mixed_segments", "multi",
         [seg(pr(80, 3, 64, 64), pr(33, 1, 96, 72, bm=2, acc=1)),
          seg(pr(0, 3, 64, 64), keys=dict(sizes=[20, 0, 33, 5], spare=4), rebase=True),
          seg(pr(50, 1, 32, 64, acc=1), rebase=True)],
         f"{G1}[4]", "M1 < 0 templates, a keyed rebased segment and a plain rebased one in one launch"),
    # ---- keyed problems (e3k_gemm_grouped / _rebased)
    case("keyed_fwd_5", "grouped", [seg(pr(0, 3, 64, 64, acc=1), keys=dict(sizes=[0, 7, 64, 30, 101], spare=9))], f"{G1}[1]",
         "compact grid: groups of size 0, under a tile (21 rows), an exact tile multiple (192 rows); starts not ascending; "
         "9 rows outside every group stay untouched"),
    case("keyed_fwd_1", "grouped", [seg(pr(0, 5, 40, 72, lay="e3nn", a="any", bias=True), keys=dict(sizes=[45], spare=6))],
         f"{G1}[1]", "one key: reps = 1, the group pair read by the non-compact path"),
    case("keyed_fwd_40", "grouped_rebased",
         [seg(pr(0, 1, 64, 64), pr(0, 1, 32, 128, bm=2, acc=1), keys=dict(sizes=[(7 * t) % 23 for t in range(40)], spare=3),
              rebase=True)], f"{G1}[2]", "40 keys, compact grid, byte offsets"),
    case("keyed_splitk", "grouped", [seg(pr(0, 1, 512, 64, bm=2, acc=1), keys=dict(sizes=[5, 40, 0, 12], spare=2))], f"{SK}[1]",
         "split-K with key groups: the non-compact keyed grid (a full grid per key)"),
    case("keyed_outer", "grouped", [seg(pr(0, 3, 10 * 8, 64, V=8, a="any", bias=False), keys=dict(sizes=[30, 0, 50, 2, 9], spare=5))],
         f"{OU}[1]", "the keyed self-connection: attrs rows through the permutation, non-compact grid"),
    case("keyed_chain", "grouped",
         [seg(pr(0, 3, 64, 64, alpha=1e3, links=[dict(K=128, bm=2, alpha=1.0)]), keys=dict(sizes=[11, 70, 0, 25, 1], spare=8))],
         f"{GC}[2]", "a keyed K-chain: followers take the head's key group and B slice"),
    # ---- weight gradients
    case("wgrad2_k64_plain", "wgrad", [seg(pr(1000, 3, 64, 64))], f"{W2}[1]", "gemm_wgrad2_body<2, false>: K <= 64, plain rows"),
    case("wgrad2_k192_plain", "wgrad", [seg(pr(777, 5, 192, 128))], f"{W2}[1]", "gemm_wgrad2_body<4, false>: K > 64, plain rows"),
    case("wgrad2_k64_gathered", "wgrad", [seg(pr(1200, 3, 60, 64, gather=True))], f"{W2}[1]",
         "gemm_wgrad2_body<2, true>: K <= 64, rows through row_index, two chunks per split"),
    case("wgrad2_k448_gathered", "wgrad", [seg(pr(640, 5, 448, 72, gather=True))], f"{W2}[1]",
         "gemm_wgrad2_body<4, true>: K > 64 with a K tail, gathered rows"),
    case("wgrad_tn_switch", "wgrad",
         [seg(pr(301, 3, 72, 65, lay="e3nn", lay_c="cf", a="any"), pr(302, 3, 100, 127, lay="e3nn", lay_c="cf", a="any"),
              pr(303, 3, 36, 128, lay="e3nn", lay_c="cf", a="any"), pr(304, 1, 64, 129, a="mis", g=False),
              pr(99, 3, 20, 128, a="r1", lay_c="e3nn"))],
         _r("gemm_wgrad_kernel<false, 1>[2]", "gemm_wgrad_kernel<false, 2>[3]"),
         "scalar A: N = 65, 127 (64-wide tile), 128, 129 (128-wide); g_vec on for N = 128 (cf G), off otherwise"),
    case("wgrad_outer", "wgrad",
         [seg(pr(200, 3, 12 * 8, 64, V=8, a="any"), pr(150, 1, 5 * 32, 128, V=32, lay="e3nn", a="any", gather=True),
              pr(99, 5, 6 * 4, 72, V=4, lay="e3nn", a="any", g=False))],
         _r("gemm_wgrad_kernel<true, 1>[2]", "gemm_wgrad_kernel<true, 2>[1]"),
         "outer form: g_vec on (cf G) and off; gathered rows; the 128-wide tile"),
    case("wgrad_one_column", "wgrad", [seg(pr(4704, 1, 64, 1, bm=2), pr(333, 3, 100, 1, lay="e3nn", a="any"),
                                           pr(500, 1, 64, 1, gather=True))],
         _r("wgrad_n1_kernel", "wgrad_n1_kernel", "gemm_wgrad_kernel<false, 1>[1]"),
         "N = 1: weighted column sums; with row_index the tile kernel"),
    case("wgrad_empty_between", "wgrad", [seg(pr(100, 1, 64, 64), pr(0, 3, 64, 64, empty=True), pr(65, 3, 64, 64))], f"{W2}[2]",
         "an empty problem between live ones"),
    case("wgrad_batch_21", "wgrad", [seg(*_many(21, M1=40))], _r(f"{W2}[20]", f"{W2}[1]"), "21 problems: 20 per launch"),
    case("keyed_wgrad2", "grouped", [seg(pr(0, 3, 64, 64), pr(0, 3, 128, 64), keys=dict(sizes=[0, 7, 64, 30, 101], spare=9))],
         f"{W2}[2]", "compact keyed grid of the pipelined kernel (gathered bodies, K <= 64 and K > 64); the other keys' B slices untouched",
         wgrad=True),
    case("keyed_wgrad_scalar", "grouped_rebased",
         [seg(pr(0, 3, 40, 64, lay="e3nn", a="any"), keys=dict(sizes=[(5 * t) % 17 for t in range(40)], spare=2), rebase=True)],
         "gemm_wgrad_kernel<false, 1>[1]", "40 keys on the scalar weight-gradient kernel: non-compact keyed grid", wgrad=True),
    case("keyed_wgrad_outer", "grouped", [seg(pr(0, 3, 10 * 4, 64, V=4, a="any"), keys=dict(sizes=[33, 0, 12], spare=4))],
         "gemm_wgrad_kernel<true, 1>[1]", "keyed outer weight gradient", wgrad=True),
    case("multi_wgrad_mixed", "multi",
         [seg(pr(300, 3, 64, 64), pr(200, 3, 48, 72, lay="e3nn", a="any")),
          seg(pr(0, 1, 96, 64), keys=dict(sizes=[50, 3, 0, 64, 1], spare=5), rebase=True)],
         _r(f"{W2}[2]", "gemm_wgrad_kernel<false, 1>[1]"), "keyed and plain segments in one weight-gradient call", wgrad=True),
    # ---- the row limit
    case("row_limit_fwd", "gemm", [seg(pr(MAX_ROWS // 3 + 1, 3, 64, 64))], "",
         "M1 M2 > 2^31 - 2^16: the kernels' int row arithmetic would wrap", rc=E3K_ERR_UNSUPPORTED),
    case("row_limit_wgrad", "wgrad", [seg(pr(2 ** 16, 2 ** 15, 64, 64))], "", "the limit on the weight gradient", rc=E3K_ERR_UNSUPPORTED),
    # ---- the reductions
    case("colsum", "colsum", [dict(rows=1000, cols=70, ld=83)], "colsum_kernel", "bias gradient: column sums, +="),
    case("fctp_v4", "fctp", [fctp(300, 3, 40, 4)], "fctp_reduce_vec_kernel<4>", "16-byte H rows, 16 lanes per u"),
    case("fctp_v8", "fctp", [fctp(100, 5, 24, 8, acc=1)], "fctp_reduce_vec_kernel<8>", "dX accumulated"),
    case("fctp_v16", "fctp", [fctp(90, 1, 70, 16)], "fctp_reduce_vec_kernel<16>", "U not a multiple of the u per wave-step"),
    case("fctp_v32", "fctp", [fctp(64, 3, 33, 32, acc=1)], "fctp_reduce_vec_kernel<32>", "V = 32"),
    case("fctp_generic", "fctp", [fctp(120, 3, 70, 12)], "fctp_reduce_kernel", "V = 12: the generic kernel"),
    case("fctp_generic_misaligned", "fctp", [fctp(50, 5, 20, 8, acc=1, mis=True)], "fctp_reduce_kernel",
         "V = 8 with a misaligned H: the generic kernel"),
]


def table_routes():
    out = set()
    for c in CASES:
        for r in filter(None, c["route"].split(";")):
            out.add(r.split("[")[0])
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# layout: every block in one arena, element offsets
class Arena:
    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        self.n = 0

    def alloc(self, n, mis=0):
        self.n += 3 + int(self.rng.integers(0, 9))      # slack in front of every block
        self.n = (self.n + 3) // 4 * 4 + mis
        off = self.n
        self.n += n
        return off


def _a_vec(d):
    return d["V"] == 0 and d["a_k"] == 1 and d["K"] % 4 == 0 and d["a_r1"] % 4 == 0 and (d["M2"] == 1 or d["a_r2"] % 4 == 0) and \
        d["A"] % 4 == 0


def _b_mode(d):
    if d["b_n"] == 1 and d["N"] % 4 == 0 and d["b_k"] % 4 == 0 and d["B"] % 4 == 0:
        return 1
    if d["b_k"] == 1 and d["K"] % 4 == 0 and d["b_n"] % 4 == 0 and d["B"] % 4 == 0:
        return 2
    return 0


def _g_vec(d):
    return d["c_n"] == 1 and d["N"] % 4 == 0 and d["c_r1"] % 4 == 0 and (d["M2"] == 1 or d["c_r2"] % 4 == 0) and d["C"] % 4 == 0


def _bstrides(K, N, bm):
    """(b_k, b_n) of B mode 1, 2 or 0"""
    return (N + 4, 1) if bm == 1 else (1, K + 4) if bm == 2 else (N + 3, 1)


def _bfoot(K, N, bm):
    b_k, b_n = _bstrides(K, N, bm)
    return (K - 1) * b_k + (N - 1) * b_n + 1


def _rows_block(ar, nodes, M2, cols, lay, kind):
    """[nodes, d] row matrix with the block at column `lead`: returns (offset of row 0's block, r1, r2, col strides)."""
    if lay == "cf":
        r2s, cs = cols + 4, 1
        foot = (M2 - 1) * r2s + cols
    else:
        r2s, cs = 1, M2
        foot = cols * M2
    lead = 5 if kind == "mis" else 4
    d = (lead + foot + 3 + 3) // 4 * 4 + (2 if kind == "r1" else 0)
    return ar.alloc(nodes * d) + lead, d, r2s, cs


def materialise(c):
    """Descriptors (element offsets), host index arrays and the arena size of a case."""
    ar = Arena(zlib.crc32(c["id"].encode()))
    segs = []
    for s in c["segs"]:
        keys = None
        probs = s["probs"]
        if s["keys"]:
            sizes, spare = s["keys"]["sizes"], s["keys"]["spare"]
            M1 = sum(sizes) + spare
            nodes = M1 + 11
            perm = ar.rng.permutation(nodes)[:M1].astype(np.int32)
            order = ar.rng.permutation(len(sizes))      # the order of the groups in the permutation: starts not ascending
            starts, pos = [0] * len(sizes), spare // 2
            for t in order:
                starts[t] = pos
                pos += sizes[t]
            keys = dict(perm=perm, groups=np.array([[starts[t], sizes[t]] for t in range(len(sizes))], np.int32).reshape(-1))
        ks = 0
        if keys:      # b_key_stride is one per segment: the largest B block of its problems, and slack
            ks = max(_bfoot(l.get("K", p["K"]), l.get("N", p["N"]), l.get("bm", p["bm"])) for p in probs for l in [{}] + p["links"])
            ks = (ks + 8 + 3) // 4 * 4
        out = []
        for p in probs:
            M1 = len(keys["perm"]) if keys else p["M1"]
            nodes = (M1 + 11 if p["gather"] else M1) if not keys else len(keys["perm"]) + 11
            idx = ar.rng.permutation(nodes)[:M1].astype(np.int32) if p["gather"] else None
            links = [dict(p, K=p["K"], bm=p["bm"], alpha=p["alpha"], a=p["a"])] + [dict(p, **l) for l in p["links"]]
            N = p["N"]
            # C, bias: the head's
            small = p["M1"] * p["M2"] > 10 ** 7      # (the row-limit cases: nothing is read; a token block)
            rows_c = 1 if small else nodes
            C_off, d_c, c_r2, c_n = _rows_block(ar, rows_c, p["M2"], N, p["lay_c"], "vec" if p["g"] else "r1")
            bias = ar.alloc(N) if p["bias"] else None
            descs = []
            for j, l in enumerate(links):
                Kj, Nj = l["K"], l.get("N", N)
                Uj = Kj // p["V"] if p["V"] else Kj
                A_off, d_a, a_r2, a_k = _rows_block(ar, rows_c, p["M2"], Uj, p["lay"], l["a"])
                A2 = a2_r1 = None
                if p["V"]:
                    a2_r1 = p["V"] + 3
                    A2 = ar.alloc(nodes * a2_r1)
                b_k, b_n = _bstrides(Kj, Nj, l["bm"])
                bfoot = _bfoot(Kj, Nj, l["bm"])
                nk = len(keys["groups"]) // 2 if keys else 1
                B_off = ar.alloc(max(nk * ks, bfoot) if not small else 64)
                d = dict(M1=M1 if not p["empty"] else 0, M2=p["M2"], N=Nj, K=Kj, V=p["V"], acc=p["acc"], A=A_off, A2=A2, a2_r1=a2_r1 or 0,
                         B=B_off, C=C_off, bias=bias if j == 0 else None, a_r1=d_a, a_r2=a_r2, a_k=a_k, b_k=b_k, b_n=b_n, c_r1=d_c,
                         c_r2=c_r2, c_n=c_n, alpha=l["alpha"], act=p["act"] if j == 0 else 0, cst=p["cst"] if j == 0 else 1.0,
                         chain=len(links) - 1 if j == 0 else 0, idx=idx, ks=ks, empty=p["empty"], spec=l)
                descs.append(d)
            if not (p["empty"] or small) and c["rc"] == E3K_OK:     # the table's operand paths are what it says they are
                h = descs[0]
                if p["a"] == "vec":
                    assert _a_vec(h), (c["id"], "A not 16-byte-loadable")
                elif p["a"] in ("mis", "r1"):
                    assert not _a_vec(h)
                for l in descs:
                    if l["spec"]["bm"] and l["N"] % 4 == 0 and l["K"] % 4 == 0:
                        assert _b_mode(l) == l["spec"]["bm"], (c["id"], "B mode")
                if c["wgrad"] and p["g"] and p["lay_c"] == "cf" and p["N"] % 4 == 0:
                    assert _g_vec(h)
            out.extend(descs)
        segs.append(dict(descs=out, keys=keys, rebase=s["rebase"]))
    return ar, segs


# ---------------------------------------------------------------------------------------------------------------------------------
# float64 reference
def _groups(d, keys):
    """[(key, node of each r1)] of a problem"""
    if d["M1"] == 0:
        return []
    if keys is None:
        r1 = np.arange(d["M1"])
        return [(0, d["idx"][r1] if d["idx"] is not None else r1)]
    g = keys["groups"].reshape(-1, 2)
    return [(t, keys["perm"][s:s + min(n, d["M1"])]) for t, (s, n) in enumerate(g) if n > 0]


def _aeff(x, d, n1, r2):
    base = d["A"] + n1 * d["a_r1"] + r2 * d["a_r2"]
    if d["V"] == 0:
        return x[base[:, None] + np.arange(d["K"])[None, :] * d["a_k"]]
    U, V = d["K"] // d["V"], d["V"]
    xu = x[base[:, None] + np.arange(U)[None, :] * d["a_k"]]
    av = x[d["A2"] + n1[:, None] * d["a2_r1"] + np.arange(V)[None, :]]
    return (xu[:, :, None] * av[:, None, :]).reshape(len(n1), U * V)


def _bidx(d, key):
    k, n = np.arange(d["K"]), np.arange(d["N"])
    return d["B"] + key * d["ks"] + k[:, None] * d["b_k"] + n[None, :] * d["b_n"]


def reference(segs, x, wgrad):
    """written indices, expected values and bounds; `over`: indices the call overwrites (initialised to NaN)"""
    idx_all, want_all, bnd_all, over = [], [], [], []
    for s in segs:
        descs, keys = s["descs"], s["keys"]
        i = 0
        while i < len(descs):
            head = descs[i]
            chain = descs[i:i + 1 + head["chain"]]
            i += 1 + head["chain"]
            for key, nodes in _groups(head, keys):
                n1 = np.repeat(nodes, head["M2"])
                r2 = np.tile(np.arange(head["M2"]), len(nodes))
                n = np.arange(head["N"])
                cidx = head["C"] + n1[:, None] * head["c_r1"] + r2[:, None] * head["c_r2"] + n[None, :] * head["c_n"]
                if wgrad:
                    A = _aeff(x, head, n1, r2)
                    G = x[cidx]
                    bidx = _bidx(head, key)
                    old = x[bidx]
                    want = old + head["alpha"] * (A.T @ G)
                    bnd = (len(n1) + 8) * U24 * (abs(head["alpha"]) * (np.abs(A).T @ np.abs(G)) + np.abs(old))
                    idx_all.append(bidx.ravel()); want_all.append(want.ravel()); bnd_all.append(bnd.ravel())
                    continue
                S = np.zeros((len(n1), head["N"]))
                Sa = np.zeros_like(S)
                ktot = 0
                for d in chain:
                    A = _aeff(x, d, n1, r2)
                    B = x[_bidx(d, key)]
                    S += d["alpha"] * (A @ B)
                    Sa += abs(d["alpha"]) * (np.abs(A) @ np.abs(B))
                    ktot += d["K"]
                pre, extra = S, np.zeros_like(S)
                if head["bias"] is not None:
                    bv = x[head["bias"] + n][None, :]
                    pre = pre + bv
                    extra = extra + np.abs(bv)
                if head["acc"]:
                    old = x[cidx]
                    pre = pre + old
                    extra = extra + np.abs(old)
                else:
                    over.append(cidx.ravel())
                bnd = (ktot + 8) * U24 * (Sa + extra)
                if head["act"]:
                    want = head["cst"] * (np.logaddexp(0.0, pre) - LOG2)
                    bnd = head["cst"] * (bnd + 16 * U24 * (np.abs(pre) + 1))
                else:
                    want = pre
                idx_all.append(cidx.ravel()); want_all.append(want.ravel()); bnd_all.append(bnd.ravel())
    cat = lambda v: np.concatenate(v) if v else np.zeros(0, np.int64)
    return cat(idx_all).astype(np.int64), cat(want_all), cat(bnd_all), cat(over).astype(np.int64)


def _reduction_reference(c, a, x):
    if c["entry"] == "colsum":
        G = x[a["G"] + np.arange(a["rows"])[:, None] * a["ld"] + np.arange(a["cols"])[None, :]]
        o = a["out"] + np.arange(a["cols"])
        return o, x[o] + G.sum(0), (a["rows"] + 8) * U24 * (np.abs(G).sum(0) + np.abs(x[o])), np.zeros(0, np.int64)
    M1, M2, Uu, V = a["M1"], a["M2"], a["U"], a["V"]
    r1 = np.repeat(np.arange(M1), M2)
    r2 = np.tile(np.arange(M2), M1)
    H = x[a["H"] + np.arange(M1 * M2)[:, None] * (Uu * V) + np.arange(Uu * V)[None, :]].reshape(M1 * M2, Uu, V)
    X = x[a["X"] + (r1 * a["x_r1"] + r2 * a["x_r2"])[:, None] + np.arange(Uu)[None, :]]
    A2 = x[a["A2"] + np.arange(M1)[:, None] * a["a2_r1"] + np.arange(V)[None, :]]
    dxi = a["dX"] + (r1 * a["x_r1"] + r2 * a["x_r2"])[:, None] + np.arange(Uu)[None, :]
    s = np.einsum("rv,ruv->ru", A2[r1], H)
    sa = np.einsum("rv,ruv->ru", np.abs(A2[r1]), np.abs(H))
    old = x[dxi] if a["acc"] else 0.0
    dx_want, dx_bnd = old + s, (V + 8) * U24 * (sa + np.abs(old))
    da = np.zeros((M1, V))
    daa = np.zeros((M1, V))
    np.add.at(da, r1, np.einsum("ru,ruv->rv", X, H))
    np.add.at(daa, r1, np.einsum("ru,ruv->rv", np.abs(X), np.abs(H)))
    dai = a["dA2"] + np.arange(M1)[:, None] * a["a2_r1"] + np.arange(V)[None, :]
    da_want, da_bnd = x[dai] + da, (M2 * Uu + 8) * U24 * (daa + np.abs(x[dai]))
    over = np.zeros(0, np.int64) if a["acc"] else dxi.ravel()
    return (np.concatenate([dxi.ravel(), dai.ravel()]), np.concatenate([dx_want.ravel(), da_want.ravel()]),
            np.concatenate([dx_bnd.ravel(), da_bnd.ravel()]), over)


def _materialise_reduction(c):
    ar = Arena(zlib.crc32(c["id"].encode()))
    a = dict(c["segs"][0])
    if c["entry"] == "colsum":
        a["G"] = ar.alloc(a["rows"] * a["ld"]) + 2
        a["out"] = ar.alloc(a["cols"])
    else:
        M1, M2, Uu, V = a["M1"], a["M2"], a["U"], a["V"]
        a["H"] = ar.alloc(M1 * M2 * Uu * V + 1, mis=1 if a["mis"] else 0)
        a["x_r1"], a["x_r2"] = M2 * (Uu + 3) + 2, Uu + 3
        a["X"] = ar.alloc(M1 * a["x_r1"]) + 1
        a["dX"] = ar.alloc(M1 * a["x_r1"]) + 1
        a["a2_r1"] = V + 4
        a["A2"] = ar.alloc(M1 * a["a2_r1"])
        a["dA2"] = ar.alloc(M1 * a["a2_r1"])
    return ar, a


# ---------------------------------------------------------------------------------------------------------------------------------
def _problem(L, d, base, rebase, M1_wrong):
    p = L.GemmProblem()
    el = (lambda off: None if off is None else 4 * off) if rebase else (lambda off: None if off is None else base + 4 * off)
    opt = (lambda off: None if off is None else 4 * off + 1) if rebase else el
    if d["empty"]:
        p.A = p.A2 = p.B = p.C = p.bias = None
    else:
        p.A, p.B, p.C = el(d["A"]), el(d["B"]), el(d["C"])
        p.A2, p.bias = opt(d["A2"]), opt(d["bias"])
    p.row_index, p.group_dev = None, None
    p.M1 = 1 if (rebase and M1_wrong) else d["M1"]
    p.M2, p.N, p.K, p.V, p.accumulate = d["M2"], d["N"], d["K"], d["V"], d["acc"]
    p.a_r1, p.a_r2, p.a_k, p.a2_r1 = d["a_r1"], d["a_r2"], d["a_k"], d["a2_r1"]
    p.b_k, p.b_n, p.c_r1, p.c_r2, p.c_n = d["b_k"], d["b_n"], d["c_r1"], d["c_r2"], d["c_n"]
    p.alpha, p.act, p.act_cst, p.chain = d["alpha"], d["act"], d["cst"], d["chain"]
    return p


def _invoke(L, c, segs, base, dev, keep):
    lib = L.load()
    st = L.stream_ptr()
    wg = 1 if c["wgrad"] else 0
    e = c["entry"]
    if e in ("colsum", "fctp"):
        a = segs
        if e == "colsum":
            return lib.e3k_colsum(base + 4 * a["G"], a["rows"], a["cols"], a["ld"], base + 4 * a["out"], st)
        return lib.e3k_fctp_reduce_bwd(base + 4 * a["H"], base + 4 * a["X"], base + 4 * a["A2"], a["M1"], a["M2"], a["U"], a["V"],
                                       a["x_r1"], a["x_r2"], a["a2_r1"], base + 4 * a["dX"], a["acc"], base + 4 * a["dA2"], st)

    def dev_int(v):
        t = torch.from_numpy(v).to(dev)
        keep.append(t)
        return t.data_ptr()

    csegs = []
    for s in segs:
        probs = []
        for d in s["descs"]:
            p = _problem(L, d, base, s["rebase"], True)
            if d["idx"] is not None:
                p.row_index = dev_int(d["idx"])
            probs.append(p)
        arr = (L.GemmProblem * len(probs))(*probs)
        keep.append(arr)
        csegs.append((arr, len(probs), s))
    arr, n, s = csegs[0]
    M1 = s["descs"][0]["M1"] if s["descs"] else 0
    if e == "gemm":
        return lib.e3k_gemm(arr, n, st)
    if e == "wgrad":
        return lib.e3k_gemm_wgrad(arr, n, st)
    if e == "rebased":
        return lib.e3k_gemm_rebased(arr, n, base, base, base, base, base, M1, wg, st)
    k = s["keys"]
    if e == "grouped":
        return lib.e3k_gemm_grouped(arr, n, dev_int(k["perm"]), dev_int(k["groups"]), len(k["groups"]) // 2, s["descs"][0]["ks"], wg, st)
    if e == "grouped_rebased":
        return lib.e3k_gemm_grouped_rebased(arr, n, base, base, base, M1, dev_int(k["perm"]), dev_int(k["groups"]), len(k["groups"]) // 2,
                                            s["descs"][0]["ks"], wg, st)
    assert e == "multi"
    ms = []
    for arr, n, s in csegs:
        g = L.GemmSegment()
        g.templates, g.n_templates = arr, n
        g.a_base = g.a2_base = g.b_base = g.c_base = g.bias_base = base if s["rebase"] else None
        g.M1 = s["descs"][0]["M1"] if s["rebase"] else -1
        if s["keys"]:
            g.n_keys, g.perm, g.groups_dev = len(s["keys"]["groups"]) // 2, dev_int(s["keys"]["perm"]), dev_int(s["keys"]["groups"])
            g.b_key_stride = s["descs"][0]["ks"]
        else:
            g.n_keys, g.perm, g.groups_dev, g.b_key_stride = 0, None, None, 0
        ms.append(g)
    marr = (L.GemmSegment * len(ms))(*ms)
    keep.append(marr)
    return lib.e3k_gemm_multi(marr, len(ms), wg, st)


@pytest.mark.parametrize("c", CASES, ids=[c["id"] for c in CASES])
def test_gemm_case_against_float64(dev, c):
    from e3_layers_amd.backend import lib as L

    if c["entry"] in ("colsum", "fctp"):
        ar, segs = _materialise_reduction(c)
    else:
        ar, segs = materialise(c)
    x0 = ar.rng.standard_normal(ar.n + 16).astype(np.float32)
    x64 = x0.astype(np.float64)
    if c["rc"] != E3K_OK:
        idx = want = bnd = over = np.zeros(0)
    elif c["entry"] in ("colsum", "fctp"):
        idx, want, bnd, over = _reduction_reference(c, segs, x64)
    else:
        idx, want, bnd, over = reference(segs, x64, c["wgrad"])
    assert len(np.unique(idx)) == len(idx), "a case must write every element once"
    x0[over.astype(np.int64)] = np.nan
    buf = torch.from_numpy(x0.copy()).to(dev)
    keep = []
    rc = _invoke(L, c, segs, buf.data_ptr(), dev, keep)
    torch.cuda.synchronize()
    route = L.load().e3k_gemm_last_routes().decode()
    assert rc == c["rc"], f"return code {rc}"
    assert route == c["route"], f"launched {route!r}"
    got = buf.cpu().numpy()
    idx = idx.astype(np.int64)
    written = np.zeros(len(x0), bool)
    written[idx] = True
    untouched = got.view(np.int32)[~written] == x0.view(np.int32)[~written]
    assert untouched.all(), f"{int((~untouched).sum())} elements outside the outputs changed, e.g. at " \
                            f"{np.flatnonzero(~written)[~untouched][:5]}"
    g = got[idx].astype(np.float64)
    err = np.abs(g - want)
    ok = np.isfinite(g) & (err <= bnd)
    if not ok.all():
        bad = np.flatnonzero(~ok)
        pytest.fail(f"{len(bad)} of {len(idx)} outputs outside the bound; first at arena {idx[bad[:5]]}: got {g[bad[:5]]}, "
                    f"want {want[bad[:5]]}, bound {bnd[bad[:5]]}")
    assert len(idx) > 0 or c["rc"] != E3K_OK


def test_a_failed_call_clears_the_record(dev):
    """A call that fails leaves an empty record even right after one that launched."""
    from e3_layers_amd.backend import lib as L

    lib = L.load()
    a = torch.randn(64, 64, device=dev)
    p = L.GemmProblem()
    p.A, p.A2, p.B, p.C, p.bias, p.row_index, p.group_dev = a.data_ptr(), None, a.data_ptr(), a.data_ptr(), None, None, None
    p.M1, p.M2, p.N, p.K, p.V, p.accumulate = 64, 1, 64, 64, 0, 1
    p.a_r1, p.a_r2, p.a_k, p.b_k, p.b_n, p.c_r1, p.c_r2, p.c_n = 64, 64, 1, 64, 1, 64, 64, 1
    p.alpha, p.act, p.act_cst, p.chain = 0.0, 0, 1.0, 0
    L.check(lib.e3k_gemm((L.GemmProblem * 1)(p), 1, L.stream_ptr()), "e3k_gemm")
    assert lib.e3k_gemm_last_routes().decode() == f"{G1}[1]"
    before = a.clone()
    p.M1, p.M2 = MAX_ROWS // 2 + 1, 2      # (refused before anything is sized or launched)
    assert lib.e3k_gemm((L.GemmProblem * 1)(p), 1, L.stream_ptr()) == E3K_ERR_UNSUPPORTED
    assert lib.e3k_gemm_last_routes().decode() == ""
    p.M1, p.M2 = 64, 1
    L.check(lib.e3k_gemm_wgrad((L.GemmProblem * 1)(p), 1, L.stream_ptr()), "e3k_gemm_wgrad")
    assert lib.e3k_gemm_last_routes().decode() == f"{W2}[1]"
    assert lib.e3k_colsum(a.data_ptr(), -1, 64, 64, a.data_ptr(), L.stream_ptr()) == E3K_ERR_INVALID
    assert lib.e3k_gemm_last_routes().decode() == ""
    torch.cuda.synchronize()
    assert torch.equal(a, before)      # (alpha = 0 added nothing)
