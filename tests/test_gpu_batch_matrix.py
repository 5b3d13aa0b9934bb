"""Every kernel that builds the batch itself -- csrc/e3k_graph.hip (csr_count / scan / fill / sort, group_rows), csrc/e3k_collate.hip
(collate_plan, collate_gather), csrc/e3k_nlist.hip (the four nlist_kernel<FILL, CutoffRule | CriterionRule>, nlist_scan) and e3k_common.h's zero_words_kernel
as e3k_csr_build launches it -- against an exact host model, element by element.

These are the integer kernels every other kernel indexes memory through.  One case per C-ABI call or short chain (plan -> gather,
count -> fill), called through ctypes.  A case lays every operand out in ONE arena of 4-byte words with slack on both sides of every
block (the Arena of tests/test_gpu_rtable_matrix.py).  Integer outputs start as a sentinel, float outputs as NaN, workspaces as a
sentinel.  After the calls the WHOLE arena is compared: what a call writes against the model, EXACTLY, everything else bit for bit
(slack, inputs, output elements the contract leaves alone, workspace past the size the library asks for, all of the arena when a call is
refused).  Only the inside of e3k_csr_build's workspace is left out.  Nothing here has a tolerance.

The models are numpy restatements of include/e3k.h: stable argsort, bincount, cumsum (CSR, row groups); exclusive scans, the ghost
graph's rule -- ghost edge k joins ghost nodes a, a + 1 with a = k mod (n_ghost - 1), swapped when k / (n_ghost - 1) is odd -- and
(float)(1.0 / n) (collation); the radius graph's fp32 distance test (rg_keep_unfused of tests/test_gpu_edge_matrix.py, the shared
within_cutoff) with the pair rule and the lowbias32 chain from 0x9E3779B9 (capped list).  They do not import the project's host mirrors;
tests/test_batch_inventory.py holds them to those on the CPU, holds ``CASES`` to the kernels the library ships, and shows the table to
be sharp (wrong models disagree on the cases' own inputs).

Every case is prepared on the host alone (``PREPARE[kind](c)`` -> arena layout and inputs, ``MODEL[kind](c, inp)`` -> {block: expected
words}); only ``LAUNCH[kind]`` needs the device.

zero_words_kernel.  The adjacent block [flag | dst_ptr | src_ptr] holds 2 N + 3 >= 3 words and the kernel's head at most three, so in that
layout the head is never longer than the fill; the cases place the block at 0, 4, 8 and 12 bytes past a 16-byte boundary with three and
seven words (head alone; head, one uint4, tail).  The head clamp (fewer words than the head) is taken by the fills of the layout with the
three blocks apart: one word (the flag) and two words (the pointers of N = 1) at the same four offsets.

e3k_csr_build with an endpoint outside [0, N): the edge is attached to node 0 AND counted there, so both lists are complete (every edge
id exactly once in each perm; the cases assert that no output word is left as the sentinel).  Before that was fixed the edge was not
counted but still claimed a slot of row 0: the last k slots of both perm lists were never written for k bad edges.
"""
import ctypes as C
import zlib

import numpy as np
import pytest
import torch

from tests.test_gpu_edge_matrix import RG_CLASSES, RG_RMAX, rg_keep_unfused, rg_planted_pairs
from tests.test_gpu_rtable_matrix import Arena, Check

pytestmark = pytest.mark.gpu

E3K_OK, E3K_ERR_INVALID, E3K_ERR_UNSUPPORTED = 0, -1, -3
SENT = -77777777      # int outputs and workspaces start as this
SENT64 = int(np.array([SENT, SENT], np.int32).view(np.int64)[0])
I64_MIN = -2 ** 63
M32 = 0xFFFFFFFF

CSR_K = {"csr_count_kernel", "csr_scan_kernel", "csr_fill_kernel", "csr_sort_kernel", "zero_words_kernel"}
NL_K = {False: {"nlist_kernel<false, e3k::CutoffRule>", "nlist_kernel<true, e3k::CutoffRule>", "nlist_scan_kernel"},
        True: {"nlist_kernel<false, e3k::CriterionRule>", "nlist_kernel<true, e3k::CriterionRule>", "nlist_scan_kernel"}}
ROWS = (0, 1, 63, 64, 65, 128, 129, 200)      # row lengths: empty, one lane, around one 64-wide tile, two tiles, a partial third / fourth


# ---------------------------------------------------------------------------------------------------------------------------------
# the table's vocabulary
def csr(id_, why, N, E, edges="random", layout="adjacent", shift=0, bad=None, used=None, stream=False):
    """e3k_csr_build.  edges: see _csr_edges; layout: [flag | dst_ptr | src_ptr] "adjacent" (one fill) or "apart" (three); shift: words
    of the flag block past a 16-byte boundary (apart: of all three blocks); bad: (where, values, count) planted endpoints."""
    return dict(id=id_, kind="csr", why=why, N=N, E=E, edges=edges, layout=layout, shift=shift, bad=bad, used=used, stream=stream,
                kernels=set(CSR_K) if (E > 0 and N > 0) else {"zero_words_kernel"}, funcs={"e3k_csr_build", "e3k_csr_workspace_ints"})


def group(id_, why, R, K, keys="random", stream=False):
    return dict(id=id_, kind="group", why=why, R=R, K=K, keys=keys, stream=stream, kernels={"group_rows_kernel"}, funcs={"e3k_group_rows"})


def collate(id_, why, sizes, ids, n_cap, e_cap, fields=(), flag0=0, stream=False):
    """e3k_collate_plan, then e3k_collate_gather on that plan when `fields` are given.  sizes: (nodes, edges) of the store's graphs;
    ids: the chosen graphs; n_cap / e_cap: an int, or ("fit", k): the chosen graphs' total + k.  fields: see _collate_fields."""
    return dict(id=id_, kind="collate", why=why, sizes=list(sizes), ids=list(ids), n_cap=n_cap, e_cap=e_cap, fields=list(fields), flag0=flag0,
                stream=stream, kernels={"collate_plan_kernel"} | ({"collate_gather_kernel"} if fields else set()),
                funcs={"e3k_collate_plan", "e3k_collate_work_ints"} | ({"e3k_collate_gather"} if fields else set()))


def nlist(id_, why, sizes, ghost, box, e_cap="fit", crit=None, planted=False, seg_bad=False, ptr_bad=False, eseg=True, flag0=0, twice=False,
          stream=False):
    """count -> fill (crit: the _crit pair).  sizes: nodes of the real graphs, uniform in [0, box)^3; ghost: ghost nodes behind them;
    e_cap: "fit" (E_real), ("fit", k), "cut" (inside one source's row) or an int.  crit: dict(window, key, threshold, keep_all, seed, d).
    twice: a second build on the same rng cells into outputs of its own."""
    on = crit is not None
    return dict(id=id_, kind="nlist", why=why, sizes=list(sizes), ghost=ghost, box=box, e_cap=e_cap, crit=crit, planted=planted, seg_bad=seg_bad,
                ptr_bad=ptr_bad, eseg=eseg, flag0=flag0, twice=twice, stream=stream, kernels=set(NL_K[on]),
                funcs={"e3k_nlist_count_crit", "e3k_nlist_fill_crit"} if on else {"e3k_nlist_count", "e3k_nlist_fill"})


def refuse(id_, why, fn, rc, **over):
    return dict(id=id_, kind="refuse", why=why, fn=fn, rc=rc, over=over, stream=False, kernels=set(), funcs={"e3k_" + fn})


def crit(window=0, key=None, threshold=0, keep_all=0, seed=0x1234567089ABCDEF, d=0):
    return dict(window=window, key=key, threshold=threshold, keep_all=keep_all, seed=seed, d=d)


# the store of the collation cases: graphs of 0 .. 7 nodes in every order of size (every head / tail of wave_copy at 4-byte rows), one of
# 300 (a 16-byte body of more than 1 024 bytes: a second trip), the edge counts of the EDGE_INDEX trips
STORE = [(3, 4), (0, 0), (1, 0), (5, 1), (2, 64), (7, 255), (4, 256), (6, 257), (300, 513), (1, 2), (2, 0), (3, 7), (5, 9), (4, 3), (6, 70), (7, 5)]
STORE_IDS = [8, 0, 1, 2, 3, 4, 5, 6, 7, 9, 10, 11, 12, 13, 14, 15, 1, 3, 3, 0, 12, 2, 7, 5]
ROW_FIELDS = [("node", 4, "first", 0, 0), ("node", 4, "table", 4, 4), ("node", 4, "first", 8, 8), ("node", 4, "table", 12, 12),
              ("node", 4, "first", 0, 4), ("node", 4, "table", 8, 0), ("node", 8, "first", 0, 0), ("node", 12, "table", 4, 4),
              ("node", 20, "first", 8, 12), ("node", 1040, "first", 0, 0), ("edge", 4, "first", 0, 0), ("edge", 8, "first", 4, 8),
              ("edge", 12, "table", 0, 0), ("graph", 4), ("graph", 8), ("nw",)]
INDEX_FIELDS = [("ei", 0), ("ei", 3), ("nseg",), ("eseg",), ("nw",), ("edge", 4, "first", 0, 0), ("node", 12, "first", 0, 0)]
SMALL = [(3, 4), (2, 1), (0, 0), (4, 6)]
NL_SIZES = [1, 2, 63, 64, 65, 129, 200]

CASES = [
    # ---- e3k_csr_build: node counts across the scan's 1 024-node chunk and its carry
    csr("csr_N1", "one node: every edge a self loop on node 0, duplicates", 1, 3),
    *[csr(f"csr_N{N}", "N at the scan kernel's chunk (1 024) and past it: the carry into the second and third chunk", N, (5 * N) // 2)
      for N in (1023, 1024, 1025, 2500)],
    *[csr(f"csr_E{E}", "E at the 256-thread block of count / fill", 40, E) for E in (1, 255, 256, 257)],
    csr("csr_E0", "no edges, N > 0: the pointers all zero, nothing else touched (edge pointers NULL)", 7, 0),
    csr("csr_rows_dst", "destination rows of 0, 1, 63, 64, 65, 128, 129, 200 edges: the tiled long-row path with a partial last tile", 12,
        sum(ROWS), "rows_dst"),
    csr("csr_rows_src", "the same row lengths in the source list", 12, sum(ROWS), "rows_src"),
    csr("csr_duplicates_self_loops", "three nodes, 300 edges: every pair many times over, one edge in five a self loop", 3, 300, "dups"),
    csr("csr_sorted", "an edge list already sorted by destination", 300, 900, "sorted"),
    csr("csr_trailing_isolated", "the last 40 of 100 nodes without an edge: the row pointers stay flat to the end", 100, 250, "low", used=60),
    csr("csr_apart", "the three zero-filled blocks apart: three fills", 300, 800, layout="apart"),
    csr("csr_stream", "on a stream of its own", 1025, 2000, stream=True),
    *[csr(f"csr_adjacent_shift{s}_N0", "N = 0, E = 0: the adjacent block is three words, 4 s bytes past a 16-byte boundary: head words only",
          0, 0, shift=s) for s in (0, 1, 2, 3)],
    *[csr(f"csr_adjacent_shift{s}", "the adjacent block (2 N + 3 = 7 words) 4 s bytes past a 16-byte boundary: head, one uint4, tail", 2, 5,
          shift=s) for s in (0, 1, 2, 3)],
    *[csr(f"csr_apart_shift{s}", "three fills of 1, 2, 2 words 4 s bytes past a 16-byte boundary: fewer words than zero_words_kernel's head",
          1, 2, layout="apart", shift=s) for s in (0, 1, 2, 3)],
    # ---- bad endpoints: flagged, attached to node 0 and counted there; no output word left unwritten
    csr("csr_bad_one_src", "one edge with source -1", 50, 120, bad=("src", [-1], 1)),
    csr("csr_bad_one_dst", "one edge with destination N", 50, 120, bad=("dst", ["N"], 1)),
    csr("csr_bad_one_both", "one edge with both endpoints 2^40 (no int32 wrap)", 50, 120, bad=("both", [2 ** 40], 1)),
    csr("csr_bad_several", "-1, N, 2^40, INT64_MIN as source only, destination only and both, 24 edges", 50, 200,
        bad=("mix", [-1, "N", 2 ** 40, I64_MIN], 24)),
    csr("csr_bad_several_N1100", "the same past the scan's chunk: row 0 grows by 70 edges (a long row), every later row moves", 1100, 2600,
        bad=("mix", [-1, "N", 2 ** 40, I64_MIN], 70)),
    csr("csr_bad_every", "every edge bad: all 130 edges in row 0 of both lists", 9, 130, bad=("mix", [-1, "N", 2 ** 40, I64_MIN], "all")),
    # ---- e3k_group_rows
    *[group(f"group_R{R}", "R at a lane, a wave and the 1 024-row chunk; the running offset carried into the second and third chunk", R, 5)
      for R in (0, 1, 63, 64, 65, 1023, 1024, 1025, 2049)],
    *[group(f"group_K{K}", "K around a wave of keys and at the limit of 256: the (wave, key) table over 1 024 threads", 700, K)
      for K in (1, 2, 63, 64, 65, 255, 256)],
    group("group_one_key", "every row under key 2 of 4", 1500, 4, "one"),
    group("group_absent_keys", "keys 0, 3 and 6 of 7 absent: reps 0, bounds {start, 0}", 1300, 7, "absent"),
    group("group_key_in_last_chunk", "key 3 only in the last row of the third chunk", 2049, 5, "last"),
    group("group_bad_keys", "-1, K, 2^32, 2^32 + 1 among the keys: flagged (not wrapped), left out of bounds / reps / perm, whose rest stays",
          1500, 6, "bad"),
    group("group_stream", "on a stream of its own", 1500, 6, stream=True),
    # ---- e3k_collate_plan
    *[collate(f"plan_G{G}", "G at a wave, past it and at the full block: the int64 block scan over 16 waves", [(n % 4, (n * 3) % 5 if n % 4 else 0)
                                                                                                           for n in range(37)],
              [(7 * k + 3) % 37 for k in range(G)], ("fit", 5), ("fit", 9)) for G in (1, 63, 64, 65, 1024)],
    collate("plan_repeated_ids", "one graph chosen five times", SMALL, [3, 3, 0, 3, 3, 3], ("fit", 2), ("fit", 0)),
    collate("plan_fits_exactly", "n + 2 == n_cap and e == e_cap", SMALL, [0, 1, 2, 3], ("fit", 2), ("fit", 0), flag0=1 | 4 | 8),
    collate("plan_one_node_short", "n + 1 == n_cap: an empty batch, flag |= 16 on top of 1|4|8", SMALL, [0, 1, 2, 3], ("fit", 1), ("fit", 0),
            flag0=1 | 4 | 8),
    collate("plan_one_edge_short", "e == e_cap + 1: an empty batch", SMALL, [0, 1, 2, 3], ("fit", 2), ("fit", -1), flag0=1 | 4 | 8),
    collate("plan_first_graph_empty", "slot 0 holds a graph without nodes: first = {-1, -1}", SMALL, [2, 0, 3], ("fit", 3), ("fit", 2)),
    *[collate(f"plan_bad_id_{name}", "a bad id: nothing read through it, the batch collated as empty graphs, flag |= 16", SMALL, ids, 40, 40,
              flag0=4)
      for name, ids in (("slot0_S", [4, 1, 2]), ("last_minus1", [0, 1, -1]), ("int32_min", [0, -2 ** 31, 2]), ("last_S", [0, 1, 2, 3, 4]))],
    # ---- e3k_collate_gather, each on the plan its case just made
    collate("gather_rows", "sixteen fields: rows of 4, 8, 12, 20, 1 040 bytes, store and batch blocks 0 / 4 / 8 / 12 bytes past a 16-byte "
            "boundary, co-aligned and not; graphs of 0 .. 7 and 300 rows; GHOST_FIRST and GHOST_TABLE; graph rows; node weights", STORE,
            STORE_IDS, ("fit", 9), ("fit", 77), ROW_FIELDS),
    collate("gather_rows_stream", "the same fields on a stream of its own, another choice of graphs", STORE, STORE_IDS[::-1][:17],
            ("fit", 2), ("fit", 1), ROW_FIELDS, stream=True),
    collate("gather_index_ghost2", "EDGE_INDEX over 0, 1, 64, 255, 256, 257, 513 edges per graph; two ghost nodes (m = 1): every ghost edge "
            "flips; 150 ghost edges", STORE, STORE_IDS, ("fit", 2), ("fit", 150), INDEX_FIELDS),
    collate("gather_index_ghost3", "three ghost nodes, 70 ghost edges: the flip happens 34 times", STORE, STORE_IDS, ("fit", 3), ("fit", 70),
            INDEX_FIELDS),
    collate("gather_index_ghost_many", "40 ghost nodes, 100 ghost edges: above two laps of m = 39, the flip happens twice", STORE, STORE_IDS,
            ("fit", 40), ("fit", 100), INDEX_FIELDS),
    collate("gather_index_ghost_1_edge", "one ghost edge", STORE, STORE_IDS, ("fit", 5), ("fit", 1), INDEX_FIELDS),
    collate("gather_index_ghost_0_edges", "no ghost edge: e == e_cap", STORE, STORE_IDS, ("fit", 5), ("fit", 0), INDEX_FIELDS),
    collate("gather_one_field", "n_fields = 1: the edge index alone", SMALL, [3, 0, 1], ("fit", 4), ("fit", 5), [("ei", 0)]),
    collate("gather_first_graph_empty", "GHOST_FIRST with a first graph without rows: the ghost's rows are zeros", SMALL, [2, 0, 3], ("fit", 3),
            ("fit", 4), [("node", 12, "first", 0, 0), ("edge", 8, "first", 0, 0), ("graph", 8), ("nseg",), ("eseg",), ("nw",), ("ei", 0)]),
    collate("gather_bad_plan", "behind a bad plan: G empty graphs, the ghost fills the bucket (GHOST_FIRST: zeros; the table; ghost edges; "
            "weights 0)", SMALL, [0, 7, 1], 30, 45,
            [("node", 12, "first", 0, 0), ("node", 12, "table", 4, 8), ("edge", 8, "first", 0, 0), ("graph", 8), ("nseg",), ("eseg",), ("nw",),
             ("ei", 3)]),
    collate("gather_G1024", "1 024 slots of 0 .. 3 nodes", [(n % 4, (n * 3) % 5 if n % 4 else 0) for n in range(37)],
            [(7 * k + 3) % 37 for k in range(1024)], ("fit", 6), ("fit", 11), [("node", 12, "table", 4, 4), ("ei", 0), ("nseg",), ("nw",),
                                                                                  ("graph", 4)]),
    # ---- the capped neighbour list
    nlist("nlist_sizes", "graphs of 1, 2, 63, 64, 65, 129, 200 nodes: one, two, three and four ballot rounds per source, cnt carried between "
          "them", NL_SIZES, 4, 7.0),
    nlist("nlist_N1024", "N = 1 024: the scan's chunk is one node", [200, 200, 200, 200, 200, 22], 2, 7.0),
    nlist("nlist_N1025", "N = 1 025: chunks of two nodes, the last threads of the scan without a node", [200, 200, 200, 200, 200, 22], 3, 7.0,
          eseg=False),
    nlist("nlist_N2100", "about 2 100 nodes: chunks of three", NL_SIZES * 4, 4, 7.0, ("fit", 100)),
    nlist("nlist_G0", "no real graph: only the ghost's edges", [], 5, 7.0, 7),
    nlist("nlist_G1", "one graph", [65], 2, 5.0, ("fit", 3)),
    nlist("nlist_G1030", "1 030 graphs of one or two nodes: the scan's graph loop takes a second trip", [1 + (k * 7) % 2 for k in range(1030)], 3,
          3.0, ("fit", 10)),
    nlist("nlist_planted", "pairs within 3e-7 of the cutoff that a fused or an exact distance test decides the other way, and pairs exactly "
          "on it (strict <)", [66], 4, 6.0, ("fit", 20), planted=True),
    nlist("nlist_e_cap_0", "e_cap = 0 with real edges: nothing written to the list, overflow", [5, 9], 3, 3.0, 0, flag0=1),
    nlist("nlist_fit_plus_1", "one ghost edge", NL_SIZES, 4, 7.0, ("fit", 1)),
    nlist("nlist_tail_70000", "70 000 ghost edges over 300 ghost nodes: the tail's stride loop (256 blocks of 256) takes a second trip", [64, 30],
          300, 7.0, ("fit", 70000)),
    nlist("nlist_overflow_cut", "e_cap inside one source's row: the first e_cap edges, the ghost's share 0, state[1] 5 -> 6, flag 1|4 -> 1|4|32",
          NL_SIZES, 4, 7.0, "cut", flag0=1 | 4),
    nlist("nlist_ghost_0", "no ghost node and slots left over: self loops on N - 1, overflow", [10, 20], 0, 5.0, ("fit", 6)),
    nlist("nlist_ghost_0_fits", "no ghost node and no slot left over: no overflow", [10, 20], 0, 5.0),
    nlist("nlist_ghost_1", "one ghost node and slots left over: self loops on N - 1, overflow", [10, 20], 1, 5.0, ("fit", 6)),
    nlist("nlist_ghost_2", "two ghost nodes (m = 1): every ghost edge flips", [10, 20], 2, 5.0, ("fit", 9)),
    nlist("nlist_ghost_3", "three ghost nodes, nine ghost edges: two flips", [10, 20], 3, 5.0, ("fit", 9), eseg=False),
    nlist("nlist_bad_segments", "node_seg entries -1, G and 2^40: not searched, count 0, still found as neighbours by their graph's nodes",
          [30, 70, 20], 3, 5.0, ("fit", 4), seg_bad=True),
    nlist("nlist_bad_node_ptr", "node_ptr entries -5 and N + 1000: clamped to [0, N], every index written is a node of the batch", [30, 70, 20], 3,
          5.0, ("fit", 4), ptr_bad=True),
    nlist("nlist_stream", "on a stream of its own", [65, 129], 4, 6.0, ("fit", 30), stream=True),
    nlist("crit_no_key", "segment_key NULL with a window: no sequence term; p = 1/2", [20, 70, 5], 3, 40.0, ("fit", 5),
          crit(window=5, threshold=2 ** 31)),
    *[nlist(f"crit_window_{w}", "chains of seven nodes by GLOBAL index: a window across a key boundary and a graph boundary", [20, 70, 33], 3, 40.0,
            ("fit", 5), crit(window=w, key="chains")) for w in (0, 1, 5)],
    *[nlist(f"crit_threshold_{name}", "the random term alone at this threshold", [20, 130, 5], 3, 40.0, ("fit", 5), crit(threshold=t))
      for name, t in (("0", 0), ("1", 1), ("2_31", 2 ** 31), ("max", 0xFFFFFFFF))],
    nlist("crit_keep_all", "p = 1: every pair of a graph, 200 nodes (four rounds)", [200, 3], 3, 40.0, ("fit", 5), crit(keep_all=1)),
    nlist("crit_all_terms", "cutoff, sequence and random term together in a dense box; draw index 2^32 + 3: the low 32 bits draw, "
          "rng = [d, junk] -> [d + 1, d]", [64, 65, 129], 4, 9.0, ("fit", 17), crit(window=5, key="chains", threshold=2 ** 28, d=2 ** 32 + 3)),
    nlist("crit_twice", "a second build on the same rng cells draws anew: rng = [0, junk] -> [2, 1]", [40, 90], 3, 40.0, ("fit", 5),
          crit(threshold=2 ** 30), twice=True),
    nlist("crit_overflow_stream", "the criterion form cut at e_cap, on a stream of its own", [40, 90], 3, 40.0, "cut",
          crit(window=3, key="chains", threshold=2 ** 29), flag0=8, stream=True),
    # ---- refusals: the return code, and the whole arena bit-identical
    refuse("refuse_csr_N_negative", "N < 0", "csr_build", E3K_ERR_INVALID, N=-1),
    refuse("refuse_csr_E_negative", "E < 0", "csr_build", E3K_ERR_INVALID, E=-1),
    refuse("refuse_csr_N_2_31", "N >= 2^31 - 1", "csr_build", E3K_ERR_UNSUPPORTED, N=2 ** 31 - 1),
    refuse("refuse_csr_E_2_31", "E >= 2^31 - 1", "csr_build", E3K_ERR_UNSUPPORTED, E=2 ** 31 - 1),
    refuse("refuse_csr_N0_with_edges", "N = 0 with E > 0: no node 0 to attach an edge to", "csr_build", E3K_ERR_INVALID, N=0),
    *[refuse(f"refuse_csr_null_{k}", f"{k} NULL", "csr_build", E3K_ERR_INVALID, **{k: None})
      for k in ("ei", "src", "dst", "dst_ptr", "dst_perm", "src_ptr", "src_perm", "ws", "flag")],
    refuse("refuse_group_R_negative", "R < 0", "group_rows", E3K_ERR_INVALID, R=-1),
    refuse("refuse_group_K0", "K = 0", "group_rows", E3K_ERR_INVALID, K=0),
    refuse("refuse_group_K257", "K = 257", "group_rows", E3K_ERR_UNSUPPORTED, K=257),
    refuse("refuse_group_R_2_31", "R >= 2^31 - 1", "group_rows", E3K_ERR_UNSUPPORTED, R=2 ** 31 - 1),
    *[refuse(f"refuse_group_null_{k}", f"{k} NULL", "group_rows", E3K_ERR_INVALID, **{k: None}) for k in ("key", "perm", "bounds", "reps", "flag")],
    *[refuse(f"refuse_plan_{name}", why, "collate_plan", E3K_ERR_INVALID, **over)
      for name, why, over in (("G0", "G = 0", dict(G=0)), ("G1025", "G = 1 025", dict(G=1025)), ("S0", "S = 0", dict(S=0)),
                              ("n_cap_1", "n_cap = 1", dict(n_cap=1)), ("n_cap_2_31", "n_cap = 2^31", dict(n_cap=2 ** 31)),
                              ("e_cap_2_31", "e_cap = 2^31", dict(e_cap=2 ** 31)), ("e_cap_negative", "e_cap < 0", dict(e_cap=-1)))],
    *[refuse(f"refuse_plan_null_{k}", f"{k} NULL", "collate_plan", E3K_ERR_INVALID, **{k: None})
      for k in ("ids", "node_off", "edge_off", "work", "n_nodes", "n_edges", "gw", "flag")],
    *[refuse(f"refuse_gather_{name}", why, "collate_gather", E3K_ERR_INVALID, **over)
      for name, why, over in (("17_fields", "17 fields", dict(n_fields=17)), ("0_fields", "no field", dict(n_fields=0)),
                              ("row_bytes_6", "row_bytes = 6", dict(row_bytes=6)), ("row_bytes_0", "row_bytes = 0", dict(row_bytes=0)),
                              ("src_off_by_2", "a store pointer 2 bytes off", dict(src_shift=2)),
                              ("dst_off_by_2", "a batch pointer 2 bytes off", dict(dst_shift=2)),
                              ("table_missing", "GHOST_TABLE without a table", dict(table=None)),
                              ("dst_ld_short", "dst_ld < e_cap", dict(dst_ld=-1)), ("kind_7", "kind 7", dict(kind=7)),
                              ("kind_negative", "kind -1", dict(kind=-1)), ("dst_null", "a field without dst", dict(fdst=None)),
                              ("G0", "G = 0", dict(G=0)), ("G1025", "G = 1 025", dict(G=1025)), ("null_fields", "fields NULL", dict(fields=None)),
                              ("null_work", "work NULL", dict(work=None)))],
    *[refuse(f"refuse_{fn}_{name}", why, fn, E3K_ERR_INVALID, **over)
      for fn in ("nlist_count", "nlist_count_crit", "nlist_fill", "nlist_fill_crit")
      for name, why, over in (("N0", "N = 0", dict(N=0)), ("N_2_31", "N >= 2^31", dict(N=2 ** 31)), ("G_negative", "G < 0", dict(G=-1)),
                              ("null_pos", "pos NULL", dict(pos=None)), ("null_node_seg", "node_seg NULL", dict(seg=None)),
                              ("null_node_ptr", "node_ptr NULL", dict(ptr=None)), ("null_counts", "counts NULL", dict(counts=None)))],
    *[refuse(f"refuse_{fn}_{name}", why, fn, E3K_ERR_INVALID, **over)
      for fn in ("nlist_fill", "nlist_fill_crit")
      for name, why, over in (("e_cap_negative", "e_cap < 0", dict(e_cap=-1)), ("e_cap_2_31", "e_cap >= 2^31", dict(e_cap=2 ** 31)),
                              ("null_offsets", "offsets NULL", dict(offsets=None)), ("null_edge_index", "edge_index NULL", dict(ei=None)),
                              ("null_n_edges", "n_edges NULL", dict(n_edges=None)), ("null_state", "state NULL", dict(state=None)),
                              ("null_flag", "flag NULL", dict(flag=None)))],
    *[refuse(f"refuse_{fn}_{name}", why, fn, E3K_ERR_INVALID, **over)
      for fn in ("nlist_count_crit", "nlist_fill_crit")
      for name, why, over in (("window_negative", "window < 0", dict(window=-1)), ("null_rng", "rng NULL", dict(rng=None)))],
]


def table_kernels():
    return set().union(*(c["kernels"] for c in CASES))


def table_functions():
    return set().union(*(c["funcs"] for c in CASES))


def _arena(c):
    return Arena(zlib.crc32(c["id"].encode()) ^ 0xB47C)


def _words(a):
    return np.ascontiguousarray(a).ravel().view(np.int32)


def _i64(a):
    return np.asarray(a, dtype=np.int64)


# ---------------------------------------------------------------------------------------------------------------------------------
# e3k_csr_build
def _csr_edges(c, rng):
    N, E, kind = c["N"], c["E"], c["edges"]
    if E == 0:
        return np.zeros((2, 0), np.int64)
    if kind in ("random", "sorted"):
        ei = rng.integers(0, N, (2, E))
        if kind == "sorted":
            ei = ei[:, np.argsort(ei[1], kind="stable")]
    elif kind in ("rows_dst", "rows_src"):      # node k is the endpoint of ROWS[k] edges; the other endpoints anywhere; shuffled
        hub = np.repeat(np.arange(len(ROWS)), ROWS)
        other = rng.integers(0, N, len(hub))
        order = rng.permutation(len(hub))
        ei = np.stack([other, hub] if kind == "rows_dst" else [hub, other])[:, order]
    elif kind == "dups":
        ei = rng.integers(0, N, (2, E))
        ei[1, ::5] = ei[0, ::5]
    else:
        assert kind == "low"
        ei = rng.integers(0, c["used"], (2, E))
    ei = _i64(ei)
    assert ei.shape == (2, E)
    if c["bad"]:
        where, values, count = c["bad"]
        values = [N if v == "N" else v for v in values]
        at = np.arange(E) if count == "all" else rng.permutation(E)[:count]
        for k, e in enumerate(at):
            v = values[k % len(values)]
            w = where if where != "mix" else ("src", "dst", "both")[(k // len(values)) % 3]
            if w in ("src", "both"):
                ei[0, e] = v
            if w in ("dst", "both"):
                ei[1, e] = v
    return ei


def csr_model(ei, N, mutant=None):
    """{flag, src, dst, dst_ptr, dst_perm, src_ptr, src_perm} of include/e3k.h: a bad edge is edge (0, 0); perm = the stable argsort by
    endpoint; ptr = [0, cumsum(bincount)].  mutant "unstable": descending edge ids inside a row; "uncounted": a bad edge is not
    counted (the behaviour before the fix: the pointers of the good edges alone, the tail of both perm lists never written)."""
    E = ei.shape[1]
    bad = ((ei < 0) | (ei >= N)).any(0)
    s, d = np.where(bad, 0, ei[0]), np.where(bad, 0, ei[1])
    out = dict(flag=np.int32(bad.any()), src=s.astype(np.int32), dst=d.astype(np.int32))
    for name, col in (("dst", d), ("src", s)):
        counted = col[~bad] if mutant == "uncounted" else col
        out[name + "_ptr"] = np.concatenate([[0], np.cumsum(np.bincount(counted, minlength=N))]).astype(np.int32)
        if mutant == "no_carry" and N > 1024:
            out[name + "_ptr"][1025:] -= out[name + "_ptr"][1024]
        perm = np.argsort(col, kind="stable")
        if mutant == "unstable":
            perm = np.lexsort((-np.arange(E), col))
        if mutant == "uncounted":
            perm = np.concatenate([perm[:E - int(bad.sum())], np.full(int(bad.sum()), SENT)])
        out[name + "_perm"] = perm.astype(np.int32)
    return out


def prepare_csr(c):
    ar = _arena(c)
    N, E = c["N"], c["E"]
    ei = _csr_edges(c, ar.rng)
    ws_n = 2 * N + 2 * E + 2
    ar.alloc("ei", 4 * E, ei, align=2)
    if c["layout"] == "adjacent":
        ar.alloc("fpp", 1 + 2 * (N + 1), np.int32(SENT), align=4, shift=c["shift"])
    else:
        for name, n in (("flag", 1), ("dst_ptr", N + 1), ("src_ptr", N + 1)):
            ar.alloc(name, n, np.int32(SENT), align=4, shift=c["shift"])
    for name in ("src", "dst", "dst_perm", "src_perm"):
        ar.alloc(name, E, np.int32(SENT))
    ar.alloc("ws", ws_n, np.int32(SENT))
    return ar, dict(ei=ei, ws_n=ws_n)


def model_csr(c, inp, mutant=None):
    m = csr_model(inp["ei"], c["N"], mutant)
    if c["E"] == 0 or c["N"] == 0:
        m = {k: v for k, v in m.items() if k in ("flag", "dst_ptr", "src_ptr")}
    if c["layout"] == "adjacent":
        m["fpp"] = np.concatenate([[m.pop("flag")], m.pop("dst_ptr"), m.pop("src_ptr")]).astype(np.int32)
    if c["bad"] and mutant is None:      # the lists are complete: every edge id once in each perm, no word left as it was
        for k, v in m.items():
            assert not (np.atleast_1d(v) == SENT).any(), k
        assert m["fpp"][0] == 1 and m["fpp"][1 + c["N"]] == c["E"] == m["fpp"][-1]
        assert np.array_equal(np.sort(m["dst_perm"]), np.arange(c["E"])) and np.array_equal(np.sort(m["src_perm"]), np.arange(c["E"]))
    return m, {"ws": inp["ws_n"]}


def launch_csr(c, ar, inp, lib, st):
    N, E = c["N"], c["E"]
    assert lib.e3k_csr_workspace_ints(N, E) == inp["ws_n"]
    p = (lambda n: ar.p(n) if E > 0 else None)
    if c["layout"] == "adjacent":
        flag = ar.p("fpp")
        dst_ptr, src_ptr = flag + 4, flag + 4 * (N + 2)
    else:
        flag, dst_ptr, src_ptr = ar.p("flag"), ar.p("dst_ptr"), ar.p("src_ptr")
    assert lib.e3k_csr_build(p("ei"), N, E, p("src"), p("dst"), dst_ptr, p("dst_perm"), src_ptr, p("src_perm"), p("ws"), flag, st) == E3K_OK


# ---------------------------------------------------------------------------------------------------------------------------------
# e3k_group_rows
def _group_keys(c, rng):
    R, K, kind = c["R"], c["K"], c["keys"]
    if kind == "one":
        return np.full(R, 2, np.int64)
    if kind == "absent":
        return _i64(rng.choice([1, 2, 4, 5], R))
    if kind == "last":
        key = _i64(rng.choice([0, 1, 2, 4], R))
        key[-1] = 3
        return key
    key = _i64(rng.integers(0, K, R))
    if kind == "bad":
        key[rng.permutation(R)[:40]] = np.tile([-1, K, 2 ** 32, 2 ** 32 + 1], 10)
        key[[0, R - 1]] = [2 ** 32 + 1, -1]
    return key


def group_model(key, K, mutant=None):
    """bounds [K, 2] = {start, count} of the rows with a key inside [0, K), perm = those rows in stable key order (the rest of perm is
    not written), reps [K] = the first row of a key (0: absent), flag = a key outside [0, K)"""
    R = len(key)
    good = (key >= 0) & (key < K)
    rows, k = np.flatnonzero(good), key[good]
    cnt = np.bincount(k, minlength=K)
    start = np.cumsum(cnt) - cnt
    order = np.argsort(k, kind="stable") if mutant != "unstable" else np.lexsort((-np.arange(len(k)), k))
    perm = np.full(R, SENT, np.int32)
    perm[:len(rows)] = rows[order]
    reps = np.where(cnt > 0, perm[np.minimum(start, max(R - 1, 0))] if R else 0, 0).astype(np.int64)
    return dict(perm=perm, bounds=np.stack([start, cnt], 1).astype(np.int32), reps=reps, flag=np.int32(not good.all()))


def prepare_group(c):
    ar = _arena(c)
    R, K = c["R"], c["K"]
    key = _group_keys(c, ar.rng)
    ar.alloc("key", 2 * R, key, align=2).alloc("perm", R, np.int32(SENT)).alloc("bounds", 2 * K, np.int32(SENT))
    ar.alloc("reps", 2 * K, np.int32(SENT), align=2).alloc("flag", 1, np.int32(SENT))
    return ar, dict(key=key)


def model_group(c, inp, mutant=None):
    return group_model(inp["key"], c["K"], mutant), {}


def launch_group(c, ar, inp, lib, st):
    p = (lambda n: ar.p(n) if c["R"] > 0 else None)
    assert lib.e3k_group_rows(p("key"), c["R"], c["K"], p("perm"), ar.p("bounds"), ar.p("reps"), ar.p("flag"), st) == E3K_OK


# ---------------------------------------------------------------------------------------------------------------------------------
# collation
def ghost_edges(n_edges, n_ghost, first, mutant=None):
    """[2, n_edges] int64: ghost edge k joins ghost nodes a, a + 1, a = k mod (n_ghost - 1), swapped when k / (n_ghost - 1) is odd"""
    k = np.arange(n_edges, dtype=np.int64)
    m = max(n_ghost - 1, 1)
    a = k % m
    flip = ((k // m) % 2 == 1) & (mutant != "no_flip")
    return first + np.stack([np.where(flip, a + 1, a), np.where(flip, a, a + 1)])


def recip32(n, mutant=None):
    """(float)(1.0 / n).  mutant "recip_1ulp": rounded toward zero instead of to nearest"""
    w = np.float32(1.0 / n)
    if mutant == "recip_1ulp" and float(w) > 1.0 / n:
        w = np.nextafter(w, np.float32(0))
    return w


def plan_model(ids, node_off, edge_off, n_cap, e_cap, flag0):
    G, S = len(ids), len(node_off) - 1
    ok = (ids >= 0) & (ids < S)
    idc = np.where(ok, ids, 0).astype(np.int64)
    sn, se = np.where(ok, node_off[idc], 0), np.where(ok, edge_off[idc], 0)
    nc, ec = np.where(ok, node_off[idc + 1] - node_off[idc], 0), np.where(ok, edge_off[idc + 1] - edge_off[idc], 0)
    sg = np.where(ok, idc, -1)
    n, e = int(nc.sum()), int(ec.sum())
    bad = (not ok.all()) or n + 2 > n_cap or e > e_cap
    if bad:
        sn, se, nc, ec, sg, n, e = (np.zeros(G, np.int64),) * 4 + (np.full(G, -1, np.int64), 0, 0)
    ex_n, ex_e = np.cumsum(nc) - nc, np.cumsum(ec) - ec
    first = [sn[0] if nc[0] > 0 else -1, se[0] if ec[0] > 0 else -1]
    plan = dict(bad=bad, n=n, e=e, beg_n=_i64(np.append(ex_n, n)), beg_e=_i64(np.append(ex_e, e)), sn=_i64(sn), se=_i64(se), sg=_i64(sg),
                first=first, cnt_n=_i64(np.append(nc, n_cap - n)), cnt_e=_i64(np.append(ec, e_cap - e)))
    out = dict(work=_i64(np.concatenate([plan["beg_n"], plan["beg_e"], sn, se, sg, first])), n_nodes=plan["cnt_n"], n_edges=plan["cnt_e"],
               gw=np.append(np.full(G, np.float32(1.0 / G), np.float32), np.float32(0)), flag=np.int32(flag0 | (16 if bad else 0)))
    return plan, out


def _collate_fields(c, ar, st):
    """Allocates the store / batch / table blocks of every field: ("node" | "edge", row_bytes, "first" | "table", bytes of the store block
    past a 16-byte boundary, the same of the batch block), ("graph", row_bytes), ("ei", dst_ld - e_cap), ("nseg",), ("eseg",), ("nw",)"""
    rng = ar.rng
    fields = []
    for k, f in enumerate(c["fields"]):
        d = dict(kind=f[0], k=k)
        if f[0] in ("node", "edge"):
            rb, ghost, sa, da = f[1:]
            rw = rb // 4
            rows_s, rows_d = (st["NS"], st["n_cap"]) if f[0] == "node" else (st["ES"], st["e_cap"])
            ar.alloc(f"s{k}", rows_s * rw, align=4, shift=sa // 4).alloc(f"d{k}", rows_d * rw, np.int32(SENT), align=4, shift=da // 4)
            if ghost == "table":
                ar.alloc(f"t{k}", rows_d * rw, align=4, shift=(da // 4 + k) % 4)
            d.update(rb=rb, ghost=ghost, rows_s=rows_s, rows_d=rows_d)
        elif f[0] == "graph":
            ar.alloc(f"s{k}", st["S"] * f[1] // 4).alloc(f"d{k}", (st["G"] + 1) * f[1] // 4, np.int32(SENT))
            d.update(rb=f[1])
        elif f[0] == "ei":
            local = np.concatenate([rng.integers(0, max(n, 1), (2, e)) for n, e in c["sizes"]], 1).astype(np.int32)
            d.update(local=local, ld=st["e_cap"] + f[1])
            ar.alloc(f"s{k}", 2 * st["ES"], local).alloc(f"d{k}", 4 * d["ld"], np.int32(SENT), align=2)
        elif f[0] == "nw":
            ar.alloc(f"d{k}", st["n_cap"], np.float32(np.nan))
        else:
            assert f[0] in ("nseg", "eseg")
            ar.alloc(f"d{k}", 2 * (st["n_cap"] if f[0] == "nseg" else st["e_cap"]), np.int32(SENT), align=2)
        fields.append(d)
    return fields


def prepare_collate(c):
    ar = _arena(c)
    sizes = np.array(c["sizes"], np.int64).reshape(-1, 2)
    S = len(sizes)
    node_off, edge_off = _i64(np.concatenate([[0], np.cumsum(sizes[:, 0])])), _i64(np.concatenate([[0], np.cumsum(sizes[:, 1])]))
    ids = np.array(c["ids"], np.int32)
    G = len(ids)
    ok = (ids >= 0) & (ids < S)
    n, e = int(sizes[ids[ok], 0].sum()), int(sizes[ids[ok], 1].sum())
    n_cap = c["n_cap"] if isinstance(c["n_cap"], int) else n + c["n_cap"][1]
    e_cap = c["e_cap"] if isinstance(c["e_cap"], int) else e + c["e_cap"][1]
    st = dict(S=S, G=G, NS=int(node_off[-1]), ES=int(edge_off[-1]), n_cap=n_cap, e_cap=e_cap, node_off=node_off, edge_off=edge_off, ids=ids)
    ar.alloc("ids", G, ids).alloc("node_off", 2 * (S + 1), node_off, align=2).alloc("edge_off", 2 * (S + 1), edge_off, align=2)
    ar.alloc("work", 2 * (5 * G + 4), np.int32(SENT), align=2).alloc("n_nodes", 2 * (G + 1), np.int32(SENT), align=2)
    ar.alloc("n_edges", 2 * (G + 1), np.int32(SENT), align=2).alloc("gw", G + 1, np.float32(np.nan)).alloc("flag", 1, np.int32(c["flag0"]))
    st["fields"] = _collate_fields(c, ar, st)
    return ar, st


def copy_classes(c, ar, st):
    """the paths of wave_copy this case's real graphs and GHOST_TABLE rows take: ("co", head, tail), ("short",) (a range shorter than its
    head), ("second_trip",) (a 16-byte body above 1 024 bytes), ("apart",) (not co-aligned, more than 64 words)"""
    plan, _ = plan_model(st["ids"], st["node_off"], st["edge_off"], st["n_cap"], st["e_cap"], 0)
    seen = set()
    for f in st["fields"]:
        if f["kind"] not in ("node", "edge"):
            continue
        node = f["kind"] == "node"
        beg, cnt, srow = (plan["beg_n"], plan["cnt_n"], plan["sn"]) if node else (plan["beg_e"], plan["cnt_e"], plan["se"])
        units = [(4 * ar.blocks[f"d{f['k']}"][0] + beg[s] * f["rb"], 4 * ar.blocks[f"s{f['k']}"][0] + srow[s] * f["rb"], cnt[s] * f["rb"])
                 for s in range(st["G"])]
        if f["ghost"] == "table":
            units.append((4 * ar.blocks[f"d{f['k']}"][0] + beg[-1] * f["rb"], 4 * ar.blocks[f"t{f['k']}"][0], cnt[-1] * f["rb"]))
        for dst, src, nbytes in units:
            if nbytes <= 0:
                seen.add(("empty",))
            elif (dst ^ src) & 15:
                seen.add(("apart",) if nbytes > 256 else ("apart_short",))
            else:
                head = (16 - (dst & 15)) & 15
                if head > nbytes:
                    seen.add(("short",))
                else:
                    seen.add(("co", int(head), int((nbytes - head) & 15)))
                    if nbytes - head > 1024:
                        seen.add(("second_trip",))
    return seen


def model_collate(c, st, mutant=None):
    plan, out = plan_model(st["ids"], st["node_off"], st["edge_off"], st["n_cap"], st["e_cap"], c["flag0"])
    G, n_cap, e_cap = st["G"], st["n_cap"], st["e_cap"]
    assert (plan["cnt_n"] >= 0).all() and (plan["cnt_e"] >= 0).all() and plan["cnt_n"].sum() == n_cap and plan["cnt_e"].sum() == e_cap
    for f in st["fields"]:
        k, kind = f["k"], f["kind"]
        if kind in ("node", "edge"):
            node = kind == "node"
            rw = f["rb"] // 4
            store = st["host"](f"s{k}").reshape(-1, rw)
            beg, cnt, srow = (plan["beg_n"], plan["cnt_n"], plan["sn"]) if node else (plan["beg_e"], plan["cnt_e"], plan["se"])
            want = np.full((f["rows_d"], rw), SENT, np.int32)
            for s in range(G):
                want[beg[s]:beg[s] + cnt[s]] = store[srow[s]:srow[s] + cnt[s]]
            first = plan["first"][0 if node else 1]
            if f["ghost"] == "table":
                want[beg[G]:] = st["host"](f"t{k}").reshape(-1, rw)[:cnt[G]]
            else:
                want[beg[G]:] = store[first] if first >= 0 else 0
        elif kind == "graph":
            rw = f["rb"] // 4
            store = st["host"](f"s{k}").reshape(-1, rw)
            want = np.zeros((G + 1, rw), np.int32)
            want[:G][plan["sg"] >= 0] = store[plan["sg"][plan["sg"] >= 0]]
        elif kind == "ei":
            want = np.full((2, f["ld"]), SENT64, np.int64)
            for s in range(G):
                b, n_e = plan["beg_e"][s], plan["cnt_e"][s]
                want[:, b:b + n_e] = f["local"][:, plan["se"][s]:plan["se"][s] + n_e].astype(np.int64) + plan["beg_n"][s]
            want[:, plan["beg_e"][G]:e_cap] = ghost_edges(plan["cnt_e"][G], plan["cnt_n"][G], plan["beg_n"][G], mutant)
            assert want[:, :e_cap].min(initial=0) >= 0 and want[:, :e_cap].max(initial=0) < n_cap
        elif kind == "nw":
            want = np.zeros(n_cap, np.float32)
            if plan["n"]:
                want[:plan["n"]] = recip32(plan["n"], mutant)
        else:
            cnt = plan["cnt_n"] if kind == "nseg" else plan["cnt_e"]
            want = np.repeat(np.arange(G + 1, dtype=np.int64), cnt)
        out[f"d{k}"] = want
    return out, {}


KIND_ID = dict(node=0, edge=1, graph=2, ei=3, nseg=4, eseg=5, nw=6)


def _field_structs(L, ar, st):
    arr = (L.CollateField * max(len(st["fields"]), 1))()
    for f in st["fields"]:
        k = f["k"]
        a = arr[k]
        a.kind, a.dst = KIND_ID[f["kind"]], ar.p(f"d{k}")
        if f["kind"] in ("node", "edge", "graph"):
            a.row_bytes, a.src = f["rb"], ar.p(f"s{k}")
            if f.get("ghost") == "table":
                a.ghost, a.table = 1, ar.p(f"t{k}")
        elif f["kind"] == "ei":
            a.src, a.src_ld, a.dst_ld = ar.p(f"s{k}"), st["ES"], f["ld"]
    return arr


def launch_collate(c, ar, st, lib, stream, L=None):
    G = st["G"]
    assert lib.e3k_collate_work_ints(G) == 5 * G + 4
    assert lib.e3k_collate_plan(ar.p("ids"), G, ar.p("node_off"), ar.p("edge_off"), st["S"], st["n_cap"], st["e_cap"], ar.p("work"),
                                ar.p("n_nodes"), ar.p("n_edges"), ar.p("gw"), ar.p("flag"), stream) == E3K_OK
    if st["fields"]:
        arr = _field_structs(L, ar, st)
        assert lib.e3k_collate_gather(arr, len(st["fields"]), G, st["n_cap"], st["e_cap"], ar.p("work"), stream) == E3K_OK


# ---------------------------------------------------------------------------------------------------------------------------------
# the capped neighbour list
def mix32(h):
    """one round of lowbias32 on uint64 arrays holding values below 2^32"""
    h = h ^ (h >> np.uint64(16))
    h = (h * np.uint64(0x7feb352d)) & np.uint64(M32)
    h = h ^ (h >> np.uint64(15))
    h = (h * np.uint64(0x846ca68b)) & np.uint64(M32)
    return h ^ (h >> np.uint64(16))


def pair_hash32(seed, draw, i, j):
    """h = mix(h ^ word) over seed low, seed high, draw (low 32 bits), i, j from 0x9E3779B9"""
    h = np.full(1, 0x9E3779B9, np.uint64)
    for w in (seed & M32, (seed >> 32) & M32, draw & M32, i, j):
        h = mix32(h ^ (np.asarray(w).astype(np.uint64) & np.uint64(M32)))
    return h


def _nlist_geometry(c, rng):
    graphs = [rng.uniform(0, c["box"], (n, 3)).astype(np.float32) for n in c["sizes"]]
    if c["planted"]:
        pairs = rg_planted_pairs()
        graphs += [np.concatenate(pairs[name], 0) for name in RG_CLASSES]
        graphs.append(np.array([[0, 0, 0], [RG_RMAX, 0, 0], [1, 2, 3], [1, 2 + RG_RMAX, 3], [0.5, 0.5, 0.5]], np.float32))      # on the cutoff
    sizes = [len(g) for g in graphs]
    G = len(sizes)
    graphs.append(rng.uniform(0, 2.0, (c["ghost"], 3)).astype(np.float32))      # (ghost nodes inside the cutoff of each other: not searched)
    pos = np.concatenate(graphs, 0)
    N = len(pos)
    node_ptr = _i64(np.concatenate([[0], np.cumsum(sizes), [N]]))
    node_seg = _i64(np.repeat(np.arange(G + 1), sizes + [c["ghost"]]))
    assert len(node_ptr) == G + 2 and len(node_seg) == N
    if c["seg_bad"]:
        node_seg[[3, 31, 45, N - c["ghost"] - 1]] = [-1, G, 2 ** 40, G + 7]
    if c["ptr_bad"]:      # (node_ptr[1], the seam of graphs 0 and 1, and node_ptr[G], the ghost's first node)
        node_ptr[1], node_ptr[G] = -5, N + 1000
    return pos, node_seg, node_ptr, G


def nlist_model(pos, node_seg, node_ptr, G, r_max, e_cap, cr=None, draw=0, state1=0, flag0=0, mutant=None):
    """counts, offsets, edge_index [2, e_cap], edge_seg [e_cap], n_edges [G + 1], state, flag of include/e3k.h's capped list.
    e_cap: an int, ("fit", k) or "cut".  mutants: "self" (j != i dropped), "le" (<= at the cutoff), "no_flip", "no_carry" (the scan's
    offsets restart at node 1 024)"""
    N = len(pos)
    clamp = lambda v: int(min(max(int(v), 0), N))
    src, dst, seg, counts = [], [], [], np.zeros(N, np.int32)
    key = cr["keys"] if cr is not None and cr["keys"] is not None and cr["window"] > 0 else None
    for i in range(N):
        g = int(node_seg[i])
        if g < 0 or g >= G:
            continue
        j = np.arange(clamp(node_ptr[g]), clamp(node_ptr[g + 1]), dtype=np.int64)
        pi = np.broadcast_to(pos[i], (len(j), 3))
        keep = rg_keep_unfused(pi, pos[j], r_max)
        if mutant == "le":
            d = pi - pos[j]
            keep = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]) <= np.float32(r_max)
        if cr is not None:
            if key is not None:
                keep |= (np.abs(j - i) < cr["window"]) & (key[j] == key[i])
            keep |= (pair_hash32(cr["seed"], draw, i, j) < np.uint64(cr["threshold"])) | bool(cr["keep_all"])
        if mutant != "self":
            keep &= j != i
        counts[i] = keep.sum()
        src += [i] * int(keep.sum())
        dst += list(j[keep])
        seg += [g] * int(keep.sum())
    offsets = _i64(np.concatenate([[0], np.cumsum(counts.astype(np.int64))]))
    if mutant == "no_carry" and N > 1024:
        offsets[1024:] -= offsets[1024]
    total = int(counts.sum())
    if e_cap == "cut":      # inside the row of a source with at least four edges, about the middle of the list
        i = next(i for i in np.argsort(np.abs(offsets[:-1] - total // 2)) if counts[i] >= 4)
        e_cap = int(offsets[i] + counts[i] // 2)
        assert offsets[i] < e_cap < offsets[i + 1]
    elif not isinstance(e_cap, int):
        e_cap = total + (0 if e_cap == "fit" else e_cap[1])
    n_real = min(total, e_cap)
    gs = clamp(node_ptr[G])
    n_ghost = N - gs
    ei = np.empty((2, e_cap), np.int64)
    ei[0, :n_real], ei[1, :n_real] = src[:n_real], dst[:n_real]
    ei[:, n_real:] = ghost_edges(e_cap - n_real, n_ghost, gs, mutant) if n_ghost >= 2 else N - 1
    assert e_cap == 0 or (ei.min() >= 0 and ei.max() < N)
    eseg = _i64(seg[:n_real] + [G] * (e_cap - n_real))
    cut = lambda v: min(int(offsets[clamp(v)]), e_cap)
    n_edges = _i64([max(cut(node_ptr[g + 1]) - cut(node_ptr[g]), 0) for g in range(G)] + [e_cap - n_real])
    over = total > e_cap or (total < e_cap and n_ghost < 2)
    return dict(counts=counts, offsets=offsets, ei=ei, eseg=eseg, n_edges=n_edges, state=_i64([total, state1 + over]),
                flag=np.int32(flag0 | (32 if over else 0)), e_cap=e_cap, over=over, total=total)


def _nlist_models(c, inp, mutant=None):
    cr = dict(c["crit"], keys=inp["keys"]) if c["crit"] else None
    d = c["crit"]["d"] if c["crit"] else 0
    first = nlist_model(inp["pos"], inp["node_seg"], inp["node_ptr"], inp["G"], RG_RMAX, c["e_cap"], cr, d, 5, c["flag0"], mutant)
    models = [first]
    if c["twice"]:
        models.append(nlist_model(inp["pos"], inp["node_seg"], inp["node_ptr"], inp["G"], RG_RMAX, first["e_cap"], cr, d + 1, 5 + first["over"],
                                  int(first["flag"]), mutant))
    return models


def prepare_nlist(c):
    ar = _arena(c)
    pos, node_seg, node_ptr, G = _nlist_geometry(c, ar.rng)
    N = len(pos)
    keys = None
    if c["crit"] and c["crit"]["key"] == "chains":
        keys = _i64(np.arange(N) // 7 + 100)
    inp = dict(pos=pos, node_seg=node_seg, node_ptr=node_ptr, G=G, N=N, keys=keys)
    inp["models"] = _nlist_models(c, inp)
    e_cap = inp["e_cap"] = inp["models"][0]["e_cap"]
    ar.alloc("pos", 3 * N, pos).alloc("seg", 2 * N, node_seg, align=2).alloc("ptr", 2 * (G + 2), node_ptr, align=2)
    if keys is not None:
        ar.alloc("keys", 2 * N, keys, align=2)
    if c["crit"]:
        ar.alloc("rng", 4, _i64([c["crit"]["d"], 0x0BAD0BAD0BAD]), align=2)
    ar.alloc("state", 4, _i64([SENT64, 5]), align=2).alloc("flag", 1, np.int32(c["flag0"]))
    for sfx in ("", "_2")[:len(inp["models"])]:
        ar.alloc("counts" + sfx, N, np.int32(SENT)).alloc("offsets" + sfx, 2 * (N + 1), np.int32(SENT), align=2)
        ar.alloc("ei" + sfx, 4 * e_cap, np.int32(SENT), align=2).alloc("n_edges" + sfx, 2 * (G + 1), np.int32(SENT), align=2)
        if c["eseg"]:
            ar.alloc("eseg" + sfx, 2 * e_cap, np.int32(SENT), align=2)
    return ar, inp


def model_nlist(c, inp, mutant=None):
    models = inp["models"] if mutant is None else _nlist_models(c, inp, mutant)
    out = {}
    for sfx, m in zip(("", "_2"), models):
        out.update({k + sfx: m[k] for k in ("counts", "offsets", "ei", "n_edges") + (("eseg",) if c["eseg"] else ())})
    last = models[-1]
    out.update(state=last["state"], flag=last["flag"])
    if c["crit"]:
        d = c["crit"]["d"]
        out["rng"] = _i64([d + len(models), d + len(models) - 1])
    return out, {}


def launch_nlist(c, ar, inp, lib, st):
    N, G, e_cap = inp["N"], inp["G"], inp["e_cap"]
    head = (ar.p("pos"), ar.p("seg"), ar.p("ptr"), N, G, RG_RMAX)
    for sfx in ("", "_2")[:len(inp["models"])]:
        tail = (e_cap, ar.p("offsets" + sfx), ar.p("ei" + sfx), ar.p("n_edges" + sfx), ar.p("eseg" + sfx) if c["eseg"] else None, ar.p("state"),
                ar.p("flag"), st)
        if c["crit"]:
            cr = c["crit"]
            rule = (ar.p("keys") if inp["keys"] is not None else None, cr["window"], cr["threshold"], cr["keep_all"], cr["seed"] & M32,
                    cr["seed"] >> 32, ar.p("rng"))
            assert lib.e3k_nlist_count_crit(*head, *rule, ar.p("counts" + sfx), st) == E3K_OK
            assert lib.e3k_nlist_fill_crit(*head, *rule, ar.p("counts" + sfx), *tail) == E3K_OK
        else:
            assert lib.e3k_nlist_count(*head, ar.p("counts" + sfx), st) == E3K_OK
            assert lib.e3k_nlist_fill(*head, ar.p("counts" + sfx), *tail) == E3K_OK


# ---------------------------------------------------------------------------------------------------------------------------------
# refusals: a small valid problem of every entry point, one argument replaced
def prepare_refuse(c):
    ar = _arena(c)
    N, E, R, K, G, S, n_cap, e_cap = 6, 10, 12, 4, 3, 4, 16, 20
    ei = _i64(ar.rng.integers(0, N, (2, E)))
    ar.alloc("ei", 4 * E, ei, align=2).alloc("flag", 1, np.int32(0)).alloc("dst_ptr", N + 1).alloc("src_ptr", N + 1)
    for name in ("src", "dst", "dst_perm", "src_perm"):
        ar.alloc(name, E)
    ar.alloc("ws", 2 * N + 2 * E + 2)
    ar.alloc("key", 2 * R, _i64(ar.rng.integers(0, K, R)), align=2).alloc("perm", R).alloc("bounds", 2 * K).alloc("reps", 2 * K, align=2)
    node_off, edge_off = _i64([0, 3, 5, 5, 9]), _i64([0, 4, 5, 5, 11])
    ar.alloc("ids", G, np.array([0, 1, 3], np.int32)).alloc("node_off", 2 * (S + 1), node_off, align=2)
    ar.alloc("edge_off", 2 * (S + 1), edge_off, align=2).alloc("n_nodes", 2 * (G + 1), align=2).alloc("n_edges", 2 * (G + 1), align=2)
    ar.alloc("gw", G + 1)
    _, plan = plan_model(np.array([0, 1, 3]), node_off, edge_off, n_cap, e_cap, 0)
    ar.alloc("work", 2 * (5 * G + 4), plan["work"], align=2)
    ar.alloc("f_src", 3 * 9, align=4).alloc("f_dst", 3 * n_cap + 2, align=4).alloc("f_table", 3 * n_cap, align=4)
    ar.alloc("f_ei_src", 2 * 11, ar.rng.integers(0, 2, 22).astype(np.int32)).alloc("f_ei_dst", 4 * e_cap, align=2)
    pos = ar.rng.uniform(0, 3, (N, 3)).astype(np.float32)
    ar.alloc("pos", 3 * N, pos).alloc("seg", 2 * N, _i64([0, 0, 0, 1, 2, 2]), align=2).alloc("ptr", 8, _i64([0, 3, 4, 6]), align=2)
    ar.alloc("counts", N, np.zeros(N, np.int32)).alloc("offsets", 2 * (N + 1), align=2).alloc("nl_ei", 4 * e_cap, align=2)
    ar.alloc("nl_n_edges", 6, align=2).alloc("state", 4, align=2).alloc("rng", 4, _i64([0, 0]), align=2).alloc("keys", 2 * N, _i64([0] * N), align=2)
    return ar, dict(N=N, E=E, R=R, K=K, G=G, S=S, n_cap=n_cap, e_cap=e_cap)


def model_refuse(c, inp, mutant=None):
    return {}, {}


def launch_refuse(c, ar, inp, lib, st, L=None):
    a = dict(inp, window=2, **{k: k for k in ar.blocks})
    a.update(gw="gw", n_fields=2, row_bytes=12, src_shift=0, dst_shift=0, table="f_table", dst_ld=0, kind=0, fields=True, fdst="f_dst")
    if c["fn"].startswith("nlist"):
        a.update(G=2, ei="nl_ei", n_edges="nl_n_edges")
    a.update(c["over"])
    p = lambda k: ar.p(a[k])
    fn = c["fn"]
    if fn == "csr_build":
        rc = lib.e3k_csr_build(p("ei"), a["N"], a["E"], p("src"), p("dst"), p("dst_ptr"), p("dst_perm"), p("src_ptr"), p("src_perm"), p("ws"),
                               p("flag"), st)
    elif fn == "group_rows":
        rc = lib.e3k_group_rows(p("key"), a["R"], a["K"], p("perm"), p("bounds"), p("reps"), p("flag"), st)
    elif fn == "collate_plan":
        rc = lib.e3k_collate_plan(p("ids"), a["G"], p("node_off"), p("edge_off"), a["S"], a["n_cap"], a["e_cap"], p("work"), p("n_nodes"),
                                  p("n_edges"), p("gw"), p("flag"), st)
    elif fn == "collate_gather":
        arr = (L.CollateField * 17)()
        for f in arr:      # (seventeen valid fields: the first two are the call unless n_fields says otherwise)
            f.kind, f.ghost, f.row_bytes, f.src, f.dst, f.table = 0, 0, 12, ar.p("f_src"), ar.p("f_dst"), None
        f = arr[0]
        f.kind, f.ghost, f.row_bytes, f.table = a["kind"], 1, a["row_bytes"], p("table")
        f.src, f.dst = ar.p("f_src") + a["src_shift"], (p("fdst") + a["dst_shift"]) if a["fdst"] else None
        g = arr[1]
        g.kind, g.src, g.dst, g.src_ld, g.dst_ld = 3, ar.p("f_ei_src"), ar.p("f_ei_dst"), 11, inp["e_cap"] + a["dst_ld"]
        rc = lib.e3k_collate_gather(arr if a["fields"] else None, a["n_fields"], a["G"], inp["n_cap"], inp["e_cap"], p("work"), st)
    else:
        head = (p("pos"), p("seg"), p("ptr"), a["N"], a["G"], 2.0)
        rule = (p("keys"), a["window"], 2 ** 30, 0, 7, 9, p("rng"))
        tail = (a["e_cap"], p("offsets"), p("ei"), p("n_edges"), None, p("state"), p("flag"), st)
        if fn == "nlist_count":
            rc = lib.e3k_nlist_count(*head, p("counts"), st)
        elif fn == "nlist_count_crit":
            rc = lib.e3k_nlist_count_crit(*head, *rule, p("counts"), st)
        elif fn == "nlist_fill":
            rc = lib.e3k_nlist_fill(*head, p("counts"), *tail)
        else:
            assert fn == "nlist_fill_crit"
            rc = lib.e3k_nlist_fill_crit(*head, *rule, p("counts"), *tail)
    assert rc == c["rc"], f"return code {rc}"


PREPARE = dict(csr=prepare_csr, group=prepare_group, collate=prepare_collate, nlist=prepare_nlist, refuse=prepare_refuse)
MODEL = dict(csr=model_csr, group=model_group, collate=model_collate, nlist=model_nlist, refuse=model_refuse)
LAUNCH = dict(csr=launch_csr, group=launch_group, collate=launch_collate, nlist=launch_nlist, refuse=launch_refuse)


def prepared(c):
    """(arena with its host image, inputs) of a case: everything but the device"""
    ar, inp = PREPARE[c["kind"]](c)
    ar.x0 = ar.rng.standard_normal(ar.n + 32).astype(np.float32).view(np.int32)
    for name, init in ar.inits:
        off, n = ar.blocks[name]
        v = np.asarray(init)
        ar.x0[off:off + n] = _words(v) if v.ndim else np.full(n, v).astype(v.dtype).view(np.int32)
    if c["kind"] == "collate":
        inp["host"] = lambda name: ar.host(name, np.int32)
    return ar, inp


def expected(c, ar, inp, mutant=None):
    return MODEL[c["kind"]](c, inp, mutant)


@pytest.mark.parametrize("c", CASES, ids=[c["id"] for c in CASES])
def test_batch_case_against_the_host_model(dev, c):
    from e3_layers_amd.backend import lib as L

    lib = L.load()
    ar, inp = prepared(c)
    want, free = expected(c, ar, inp)
    ar.buf = torch.from_numpy(ar.x0.copy()).to(dev)
    ar.base = ar.buf.data_ptr()
    assert ar.base % 64 == 0
    torch.cuda.synchronize()
    extra = dict(L=L) if c["kind"] in ("collate", "refuse") else {}
    if c["stream"]:
        with torch.cuda.stream(torch.cuda.Stream()):
            st = L.stream_ptr()
            assert st not in (None, 0)
            LAUNCH[c["kind"]](c, ar, inp, lib, st, **extra)
    else:
        LAUNCH[c["kind"]](c, ar, inp, lib, L.stream_ptr(), **extra)
    ck = Check(ar, c)
    for name, n in free.items():
        ck.free(name, n)
    for name, w in want.items():
        ck.exact(name, w)
    ck.finish()
