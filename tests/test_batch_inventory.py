"""The batch-structure kernels the library ships == the kernels tests/test_gpu_batch_matrix.py's cases name (no GPU needed); the premises
its cases rest on; its numpy models held to the project's host constructions; and the table shown to be sharp: a wrong model disagrees
with the right one on a case's own inputs.

Reads the gfx950 code objects of e3k_graph.o, e3k_collate.o and e3k_nlist.o: a kernel added without an exactly checked case, or a case
naming a kernel that no longer exists, fails here; so does a function of include/e3k.h's CSR / row-group / collation / capped-list
sections that no case calls.  e3k_common.h's static zero_words_kernel is emitted into every object; it counts where the file calls
zero_fill (e3k_graph.hip alone).  edge_records_kernel of e3k_graph.hip belongs to tests/test_gpu_rtable_matrix.py's ``records`` cases.

Wrong models (planted in the numpy model, never in the library):
  unstable     a stable sort replaced by one that is descending inside a row / key
  no_carry     the scan's carry dropped past 1 024 (CSR row pointers; the capped list's offsets)
  self         j != i dropped from the capped list
  le           < replaced by <= at the cutoff
  no_flip      the ghost edges' flip dropped
  recip_1ulp   1 / n rounded toward zero.  "1 / n formed in fp32" itself is NOT a wrong model: a correctly rounded fp32 division of
               the integers 1 and n < 2^24 equals (float)(1.0 / (double)n) for every such n (test_fp32_reciprocal_is_the_same_number
               checks all of them: rounding the double quotient a second time never crosses an fp32 midpoint).  What the table can
               and does catch is a reciprocal that is off by one ulp.
  uncounted    bad edges left uncounted: e3k_csr_build before its fix
"""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from tests import test_gpu_batch_matrix as M
from tests import test_gpu_rtable_matrix as RT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "equivariant-nn-zoo_amd", "csrc")
HEADER = os.path.join(ROOT, "include", "e3k.h")
LLVM = "/opt/rocm/llvm/bin"
CASES = {c["id"]: c for c in M.CASES}
FILES = ("e3k_graph", "e3k_collate", "e3k_nlist")

_prepared = {}


def prep(cid):
    """(case, arena, inputs, expected words) -- prepared once per case and shared"""
    if cid not in _prepared:
        c = CASES[cid]
        ar, inp = M.prepared(c)
        _prepared[cid] = (c, ar, inp, M.expected(c, ar, inp)[0])
    return _prepared[cid]


def _tool(name):
    path = os.path.join(LLVM, name)
    return path if os.path.exists(path) else name


def _shipped_kernels(tmp_path, stem):
    obj = os.path.join(CSRC, stem + ".o")
    if not os.path.exists(obj):
        import __graft_entry__

        __graft_entry__.build()
    work = tmp_path / stem
    work.mkdir()
    os.symlink(obj, work / (stem + ".o"))
    subprocess.run([_tool("llvm-objdump"), "--offloading", stem + ".o"], check=True, cwd=work, capture_output=True)
    bundles = [p for p in os.listdir(work) if p.endswith("gfx950")]
    assert len(bundles) == 1, os.listdir(work)
    syms = subprocess.run([_tool("llvm-readelf"), "-sW", str(work / bundles[0])], check=True, capture_output=True, text=True).stdout
    names = [f[7] for f in (line.split() for line in syms.splitlines()) if len(f) >= 8 and f[3] == "FUNC" and f[4] == "GLOBAL"]
    demangled = subprocess.run(["c++filt"], input="\n".join(names), check=True, capture_output=True, text=True).stdout
    found = {m.group(1) for m in re.finditer(r"e3k::(\w+_kernel(?:<[^>]*>)?)\(", demangled)}
    with open(os.path.join(CSRC, stem + ".hip")) as f:
        text = f.read()
    if "zero_fill(" not in text:      # (emitted into every object, launched by this file or not)
        assert "zero_words" not in text
        found -= {"zero_words_kernel"}
    return found


def test_every_batch_kernel_has_an_exactly_checked_case(tmp_path):
    shipped = set().union(*(_shipped_kernels(tmp_path, stem) for stem in FILES))
    assert "edge_records_kernel" in shipped
    records = [c for c in RT.CASES if c["kind"] == "records"]
    assert len(records) >= 4 and all("e3k_edge_records" in c["funcs"] for c in records)      # (edge_records_kernel: checked there)
    shipped -= {"edge_records_kernel"}
    table = M.table_kernels()
    assert len(shipped) == 13, sorted(shipped)
    assert {f"nlist_kernel<{a}, e3k::{b}>" for a in ("false", "true") for b in ("CutoffRule", "CriterionRule")} <= shipped
    assert shipped - table == set(), f"kernels without a case in test_gpu_batch_matrix.CASES: {sorted(shipped - table)}"
    assert table - shipped == set(), f"the case table names kernels the library does not ship: {sorted(table - shipped)}"
    for k in shipped:      # every kernel is named by a case that calls the library (a refusal launches nothing and names none)
        assert any(k in c["kernels"] and c["kind"] != "refuse" for c in M.CASES), k


def test_every_batch_function_of_the_header_is_called_by_a_case():
    with open(HEADER) as f:
        declared = set(re.findall(r"\b(e3k_(?:csr|collate|nlist)_\w+|e3k_group_rows)\s*\(", f.read()))
    assert len(declared) == 10, sorted(declared)
    called = M.table_functions()
    assert declared - called == set(), f"declared in include/e3k.h, called by no case: {sorted(declared - called)}"
    assert called - declared == set(), f"cases call functions the header does not declare: {sorted(called - declared)}"
    for fn in declared:      # ... and refused by one, where it can refuse
        if not fn.endswith("_ints"):
            assert any(c["kind"] == "refuse" and fn in c["funcs"] for c in M.CASES), fn


def test_case_ids_are_unique():
    ids = [c["id"] for c in M.CASES]
    assert len(ids) == len(set(ids))
    assert all(c["why"] for c in M.CASES)


@pytest.mark.parametrize("cid", [c["id"] for c in M.CASES if c["kind"] != "refuse"])
def test_every_case_prepares_on_the_host(cid):
    """the arena of a case holds every block its model names, and the model's words fit their blocks"""
    c, ar, inp, want = prep(cid)
    for name, w in want.items():
        assert name in ar.blocks, name
        assert len(M._words(w)) <= ar.blocks[name][1], (name, len(M._words(w)), ar.blocks[name])
    if c["kind"] == "nlist":      # every index of the model's list is a node of the batch
        m = inp["models"][0]
        assert m["e_cap"] == 0 or (0 <= m["ei"].min() and m["ei"].max() < inp["N"])


# ---------------------------------------------------------------------------------------------------------------------------------
# premises: the boundaries the cases claim to cross
def test_csr_cases_cross_their_boundaries():
    for kind, row in (("rows_dst", 1), ("rows_src", 0)):
        c, ar, inp, want = prep("csr_" + kind)
        deg = np.bincount(inp["ei"][row], minlength=c["N"])
        assert tuple(deg[:len(M.ROWS)]) == M.ROWS
    c, ar, inp, want = prep("csr_duplicates_self_loops")
    ei = inp["ei"]
    assert (ei[0] == ei[1]).sum() >= 60 and len({tuple(p) for p in ei.T}) <= 9
    c, ar, inp, want = prep("csr_trailing_isolated")
    assert want["fpp"][1 + 60] == want["fpp"][1 + 100] == 250
    c, ar, inp, want = prep("csr_sorted")
    assert (np.diff(inp["ei"][1]) >= 0).all()
    for s in range(4):      # the adjacent block's first word sits 4 s bytes past a 16-byte boundary
        for cid in (f"csr_adjacent_shift{s}", f"csr_adjacent_shift{s}_N0"):
            assert prep(cid)[1].blocks["fpp"][0] % 4 == s
        blocks = prep(f"csr_apart_shift{s}")[1].blocks
        assert all(blocks[k][0] % 4 == s for k in ("flag", "dst_ptr", "src_ptr"))
        head = (4 - s) % 4      # zero_words_kernel's head in words; the flag's fill has one word, the pointers' two
        assert s == 0 or (head > 1 if s < 3 else head == 1)
    seen = set()
    for cid, c in CASES.items():
        if c["kind"] == "csr" and c["bad"]:
            ei, N = prep(cid)[2]["ei"], c["N"]
            bad = (ei < 0) | (ei >= N)
            seen |= {(("src", "dst")[r], int(v) if v != N else "N") for r in (0, 1) for v in np.unique(ei[r][bad[r]])}
            seen |= {"both"} if (bad[0] & bad[1]).any() else set()
            seen |= {"src_only"} if (bad[0] & ~bad[1]).any() else set()
            seen |= {"dst_only"} if (~bad[0] & bad[1]).any() else set()
    assert {(r, v) for r in ("src", "dst") for v in (-1, "N", 2 ** 40, M.I64_MIN)} | {"both", "src_only", "dst_only"} <= seen, seen


def test_group_cases_cross_their_boundaries():
    c, ar, inp, want = prep("group_key_in_last_chunk")
    assert np.flatnonzero(inp["key"] == 3).tolist() == [2048]
    c, ar, inp, want = prep("group_absent_keys")
    assert (want["bounds"].reshape(-1, 2)[[0, 3, 6], 1] == 0).all() and (want["reps"][[0, 3, 6]] == 0).all()
    assert want["bounds"].reshape(-1, 2)[3, 0] == (inp["key"] < 3).sum() > 0
    c, ar, inp, want = prep("group_bad_keys")
    assert {-1, 6, 2 ** 32, 2 ** 32 + 1} <= set(inp["key"].tolist()) and want["flag"] == 1
    n_good = int(((inp["key"] >= 0) & (inp["key"] < 6)).sum())
    assert 40 <= c["R"] - n_good <= 42 and (want["perm"][n_good:] == M.SENT).all() and (want["perm"][:n_good] != M.SENT).all()
    assert want["bounds"].reshape(-1, 2)[:, 1].sum() == n_good


def test_collate_cases_cross_their_boundaries():
    seen, trips, ghost = set(), set(), set()
    for cid, c in CASES.items():
        if c["kind"] == "collate" and c["fields"]:
            _, ar, st, want = prep(cid)
            seen |= M.copy_classes(c, ar, st)
            plan, _ = M.plan_model(st["ids"], st["node_off"], st["edge_off"], st["n_cap"], st["e_cap"], 0)
            if any(f["kind"] == "ei" for f in st["fields"]):
                trips |= set(plan["cnt_e"][:-1].tolist())
                m = max(int(plan["cnt_n"][-1]) - 1, 1)
                ghost.add((int(plan["cnt_n"][-1]), int(plan["cnt_e"][-1]), int(plan["cnt_e"][-1]) > 2 * m))
    # wave_copy: every head and every tail of the co-aligned path, a range shorter than its head, a second trip of the 16-byte loop,
    # the word loop with more than 64 words
    assert {h for k in seen if k[0] == "co" for h in k[1:2]} == {0, 4, 8, 12}, seen
    assert {k[2] for k in seen if k[0] == "co"} == {0, 4, 8, 12}, seen
    assert {("short",), ("second_trip",), ("apart",), ("empty",)} <= seen, seen
    assert {0, 1, 64, 255, 256, 257, 513} <= trips
    assert {n for n, e, laps in ghost} >= {2, 3, 40} and {e for n, e, laps in ghost} >= {0, 1, 70} and any(laps and n > 3 for n, e, laps in ghost)
    c, ar, st, want = prep("gather_first_graph_empty")
    assert want["work"][-2:].tolist() == [-1, -1] and want["flag"] == 0 and not want["d0"].ravel()[-3 * 3:].any()
    c, ar, st, want = prep("gather_bad_plan")
    assert want["flag"] == 16 and (want["n_nodes"] == [0, 0, 0, 30]).all() and not want["d0"].any() and not want["d6"].any()
    c, ar, st, want = prep("gather_rows")
    assert len(c["fields"]) == 16 and want["work"][-2] >= 0      # (GHOST_FIRST with a first graph that has rows)
    for cid, flag in (("plan_fits_exactly", 13), ("plan_one_node_short", 29), ("plan_one_edge_short", 29)):
        assert prep(cid)[3]["flag"] == flag
    for cid, c in CASES.items():
        if cid.startswith("plan_bad_id"):
            assert prep(cid)[3]["flag"] == 4 | 16 and (prep(cid)[3]["work"][-2:] == -1).all()


def test_nlist_cases_cross_their_boundaries():
    c, ar, inp, want = prep("nlist_sizes")
    m = inp["models"][0]
    # sources of the 129- and 200-node graphs keep neighbours in more than one 64-wide round
    for g in (5, 6):
        beg = int(inp["node_ptr"][g])
        sel = m["ei"][0] == beg + 70
        rounds = {(int(j) - beg) // 64 for j in m["ei"][1][sel]}
        assert len(rounds) >= 2, rounds
    assert not m["over"] and m["total"] == m["e_cap"]
    assert prep("nlist_N1024")[2]["N"] == 1024 and prep("nlist_N1025")[2]["N"] == 1025 and 2048 < prep("nlist_N2100")[2]["N"] <= 3072
    assert prep("nlist_G1030")[2]["G"] == 1030 and prep("nlist_G0")[2]["G"] == 0
    m = prep("nlist_tail_70000")[2]["models"][0]
    assert m["e_cap"] - m["total"] == 70000 > 256 * 256
    for cid in ("nlist_overflow_cut", "crit_overflow_stream"):
        c, ar, inp, want = prep(cid)
        m = inp["models"][0]
        i = int(np.searchsorted(m["offsets"], m["e_cap"], side="right")) - 1
        assert m["offsets"][i] < m["e_cap"] < m["offsets"][i + 1] and m["over"]
        assert m["n_edges"].sum() == m["e_cap"] and m["n_edges"][-1] == 0 and m["state"][1] == 6 and m["flag"] == c["flag0"] | 32
    for cid, over in (("nlist_ghost_0", True), ("nlist_ghost_0_fits", False), ("nlist_ghost_1", True), ("nlist_ghost_2", False), ("nlist_e_cap_0", True)):
        m = prep(cid)[2]["models"][0]
        assert bool(m["over"]) == over
        if over and m["e_cap"]:
            assert (m["ei"][:, m["total"]:] == prep(cid)[2]["N"] - 1).all()
    # the planted pairs: kept and dropped as the fp32 model says, the pairs exactly on the cutoff dropped
    c, ar, inp, want = prep("nlist_planted")
    m = inp["models"][0]
    edges = set(map(tuple, m["ei"][:, :m["total"]].T))
    first = int(inp["node_ptr"][1])
    for k, name in enumerate(M.RG_CLASSES):
        for q in range(6):
            i, j = first + 12 * k + q, first + 12 * k + 6 + q
            assert ((i, j) in edges) == name.startswith("unfused_keeps") == ((j, i) in edges)
    on = first + 48
    assert (on, on + 1) not in edges and (on + 2, on + 3) not in edges and (on, on + 4) in edges
    # the criterion cases: each term decides pairs of its own
    for cid in ("crit_window_1", "crit_window_5", "crit_threshold_1", "crit_threshold_2_31", "crit_threshold_max", "crit_keep_all"):
        c, ar, inp, want = prep(cid)
        plain = M.nlist_model(inp["pos"], inp["node_seg"], inp["node_ptr"], inp["G"], M.RG_RMAX, ("fit", 0))
        more = inp["models"][0]["total"] - plain["total"]
        pairs = sum(n * (n - 1) for n in c["sizes"])
        if cid == "crit_window_1" or cid == "crit_threshold_1":
            assert more == 0      # (|i - j| < 1 holds for no pair; a hash below 1 is a hash of 0)
        elif cid == "crit_keep_all":
            assert inp["models"][0]["total"] == pairs
        elif cid == "crit_threshold_max":
            assert pairs - 3 <= inp["models"][0]["total"] <= pairs
        else:
            assert more > 100
    c, ar, inp, want = prep("crit_window_5")
    m = inp["models"][0]
    far = ~M.rg_keep_unfused(inp["pos"][m["ei"][0][:m["total"]]], inp["pos"][m["ei"][1][:m["total"]]])
    gap = np.abs(m["ei"][0] - m["ei"][1])[:m["total"]][far]
    assert gap.max() == 4 and (inp["keys"][m["ei"][0][:m["total"]][far]] == inp["keys"][m["ei"][1][:m["total"]][far]]).all()
    assert inp["keys"][19] == inp["keys"][20] and inp["node_seg"][19] != inp["node_seg"][20]      # a chain across a graph boundary: cut
    a, b = prep("crit_twice")[2]["models"]
    assert not np.array_equal(a["counts"], b["counts"]) and prep("crit_twice")[3]["rng"].tolist() == [2, 1]
    assert prep("crit_all_terms")[3]["rng"].tolist() == [2 ** 32 + 4, 2 ** 32 + 3]
    c, ar, inp, want = prep("nlist_bad_segments")
    assert (want["counts"][[3, 31, 45]] == 0).all() and {3, 31, 45} <= set(want["ei"][1].tolist())
    c, ar, inp, want = prep("nlist_bad_node_ptr")
    assert (want["counts"][:30] == 0).all() and want["counts"][30:100].sum() > 0 and inp["models"][0]["over"]


# ---------------------------------------------------------------------------------------------------------------------------------
# the models against the project's host constructions
def test_csr_model_equals_build_topology_on_the_host():
    from e3_layers_amd.backend.graph import build_topology

    for cid in ("csr_N1025", "csr_rows_dst", "csr_duplicates_self_loops", "csr_trailing_isolated", "csr_E1"):
        c, ar, inp, want = prep(cid)
        topo = build_topology(torch.from_numpy(inp["ei"]), c["N"])
        m = M.csr_model(inp["ei"], c["N"])
        for name, t in (("src", topo.src), ("dst", topo.dst), ("dst_ptr", topo.dst_ptr), ("dst_perm", topo.dst_perm), ("src_ptr", topo.src_ptr),
                        ("src_perm", topo.src_perm)):
            assert np.array_equal(m[name], t.numpy().astype(np.int32)), (cid, name)
    # a bad edge IS edge (0, 0): the model of the flagged build is the model of the repaired list
    c, ar, inp, want = prep("csr_bad_several")
    ei = inp["ei"].copy()
    bad = ((ei < 0) | (ei >= c["N"])).any(0)
    assert bad.sum() == 24
    ei[:, bad] = 0
    fixed, m = M.csr_model(ei, c["N"]), M.csr_model(inp["ei"], c["N"])
    assert m["flag"] == 1 and fixed["flag"] == 0 and all(np.array_equal(fixed[k], m[k]) for k in m if k != "flag")
    with pytest.raises(ValueError):      # edges without a node: refused on the host as e3k_csr_build refuses them
        build_topology(torch.zeros(2, 3, dtype=torch.long), 0)
    assert build_topology(torch.zeros(2, 0, dtype=torch.long), 0).dst_ptr.tolist() == [0]


def test_group_model_equals_row_groups_on_the_host():
    from e3_layers_amd.nn.core import row_groups

    for cid in ("group_R2049", "group_K256", "group_absent_keys", "group_one_key"):
        c, ar, inp, want = prep(cid)
        g = row_groups(torch.from_numpy(inp["key"].copy()), c["K"])
        assert np.array_equal(want["perm"], g.perm.numpy()) and np.array_equal(want["bounds"], g.bounds.numpy()), cid
        present = want["bounds"][:, 1] > 0      # (an absent key's representative is row 0 on the device, any row on the host)
        assert np.array_equal(want["reps"][present], g.reps.numpy()[present]) and (want["reps"][~present] == 0).all()


def test_collate_model_equals_pad_batch():
    from e3_layers_amd.data.synthetic import synth_qm9
    from e3_layers_amd.run.graph_step import ghost_sample, pad_batch

    host = synth_qm9(3, 5)
    nn, ne = host["_n_nodes"].reshape(-1).numpy(), host["_n_edges"].reshape(-1).numpy()
    n, e, G = int(nn.sum()), int(ne.sum()), len(nn)
    for dn, de in ((2, 0), (2, 7), (3, 9), (11, 25)):
        n_cap, e_cap = n + dn, e + de
        padded = pad_batch(host, n_cap, e_cap)
        node_off, edge_off = np.concatenate([[0], np.cumsum(nn)]), np.concatenate([[0], np.cumsum(ne)])
        plan, out = M.plan_model(np.arange(G, dtype=np.int32), node_off, edge_off, n_cap, e_cap, 0)
        assert not plan["bad"]
        assert np.array_equal(out["n_nodes"], padded["_n_nodes"].reshape(-1).numpy()) and np.array_equal(out["n_edges"], padded["_n_edges"].reshape(-1).numpy())
        assert np.array_equal(out["gw"], padded["_graph_weight"].reshape(-1).numpy())
        w = np.zeros(n_cap, np.float32)
        w[:n] = M.recip32(n)
        assert np.array_equal(w, padded["_node_weight"].reshape(-1).numpy())
        ei = padded["edge_index"].numpy()
        assert np.array_equal(ei[:, e:], M.ghost_edges(de, dn, n))
    like = host.get(0) if hasattr(host, "get") else None
    if like is not None:
        for n_ghost, n_edges in ((2, 5), (3, 9), (40, 100), (7, 0)):
            assert np.array_equal(ghost_sample(like, n_ghost, n_edges)["edge_index"].numpy(), M.ghost_edges(n_edges, n_ghost, 0))
    # one bad id or one node too many: the empty batch
    plan, out = M.plan_model(np.array([0, G], np.int32), node_off, edge_off, n_cap, e_cap, 1)
    assert plan["bad"] and out["flag"] == 17 and out["n_nodes"].tolist() == [0, 0, n_cap] and out["work"].tolist() == [0] * 6 + [0] * 4 + [-1] * 4
    with pytest.raises(ValueError):
        pad_batch(host, n + 1, e)


def test_pair_hash_model_equals_the_host_restatement():
    from e3_layers_amd.data.compute_edge import pair_hash

    rng = np.random.default_rng(11)
    i, j = rng.integers(0, 2 ** 31, 500), rng.integers(0, 2 ** 31, 500)
    for seed, draw in ((0, 0), (0x1234567089ABCDEF, 7), (2 ** 64 - 1, 2 ** 32 + 3), (5, 2 ** 31)):
        got = M.pair_hash32(seed, draw, i, j)
        s = seed - 2 ** 64 if seed >= 2 ** 63 else seed
        want = pair_hash(s, draw, torch.from_numpy(i), torch.from_numpy(j)).numpy()
        assert np.array_equal(got.astype(np.int64), want)
        assert np.array_equal(got, M.pair_hash32(seed, draw & 0xFFFFFFFF, i, j))      # (the low 32 bits of the draw index draw)
    assert int(M.mix32(np.full(1, 1, np.uint64))[0]) == _lowbias32(1) and int(M.mix32(np.full(1, 0xDEADBEEF, np.uint64))[0]) == _lowbias32(0xDEADBEEF)


def _lowbias32(h):
    h ^= h >> 16
    h = (h * 0x7feb352d) & 0xFFFFFFFF
    h ^= h >> 15
    h = (h * 0x846ca68b) & 0xFFFFFFFF
    return h ^ (h >> 16)


def test_cutoff_model_is_the_edge_matrix_model():
    from tests import test_gpu_edge_matrix as EM

    assert M.rg_keep_unfused is EM.rg_keep_unfused and M.rg_planted_pairs is EM.rg_planted_pairs and M.RG_RMAX == EM.RG_RMAX
    # the plain capped list of real graphs is the radius graph of the edge matrix's model
    c, ar, inp, want = prep("nlist_planted")
    N, G = inp["N"], inp["G"]
    real = int(inp["node_ptr"][G])
    start = np.repeat(inp["node_ptr"][:G], np.diff(inp["node_ptr"][:G + 1])).astype(np.int32)
    end = np.repeat(inp["node_ptr"][1:G + 1], np.diff(inp["node_ptr"][:G + 1])).astype(np.int32)
    counts, ei = EM.rg_reference(dict(pos=inp["pos"][:real], start=start, end=end, old_ptr=None, old_dst=None))
    m = inp["models"][0]
    assert np.array_equal(counts, m["counts"][:real]) and np.array_equal(ei, m["ei"][:, :m["total"]])


# ---------------------------------------------------------------------------------------------------------------------------------
# the table is sharp
def _disagreeing(mutant, kinds):
    out = []
    for cid, c in CASES.items():
        if c["kind"] in kinds:
            _, ar, inp, want = prep(cid)
            mut = M.expected(c, ar, inp, mutant)[0]
            if any(not np.array_equal(M._words(want[k]), M._words(mut[k])) for k in want):
                out.append(cid)
    return out


MUTANTS = [
    # (wrong model, the kinds of case it is planted in, cases that must notice)
    ("unstable", ("csr", "group"), {"csr_N1025", "csr_rows_dst", "csr_rows_src", "csr_duplicates_self_loops", "group_R1025", "group_K256"}),
    ("no_carry", ("csr", "nlist"), {"csr_N1025", "csr_N2500", "csr_bad_several_N1100", "nlist_N1025", "nlist_N2100", "nlist_G1030"}),
    ("self", ("nlist",), {"nlist_sizes", "nlist_G1", "crit_keep_all"}),
    ("le", ("nlist",), {"nlist_planted"}),
    ("no_flip", ("collate", "nlist"), {"gather_index_ghost2", "gather_index_ghost3", "gather_index_ghost_many", "gather_bad_plan",
                                       "nlist_ghost_2", "nlist_ghost_3", "nlist_tail_70000"}),
    ("recip_1ulp", ("collate",), {"gather_first_graph_empty", "gather_rows_stream"}),      # (n = 7 and n = 349: 1 / n rounds up)
    ("uncounted", ("csr",), {cid for cid, c in CASES.items() if c["kind"] == "csr" and c["bad"]}),
]


@pytest.mark.parametrize("mutant,kinds,must", MUTANTS, ids=[m[0] for m in MUTANTS])
def test_a_wrong_model_disagrees_on_the_cases_own_inputs(mutant, kinds, must):
    noticed = set(_disagreeing(mutant, kinds))
    print(f"{mutant}: {len(noticed)} cases disagree: {sorted(noticed)}")
    assert must and must <= noticed, f"{mutant}: not noticed by {sorted(must - noticed)}"
    if mutant == "uncounted":      # ... and by nothing else: for valid input the fix changes nothing
        assert noticed == must and len(must) == 6
        for cid in must:      # what the unfixed kernel leaves unwritten: the last k slots of both lists
            c, ar, inp, want = prep(cid)
            mut = M.expected(c, ar, inp, mutant)[0]
            k = int(((inp["ei"] < 0) | (inp["ei"] >= c["N"])).any(0).sum())
            for name in ("dst_perm", "src_perm"):
                assert (mut[name][-k:] == M.SENT).all() and (mut[name][:c["E"] - k] != M.SENT).all() and (want[name] != M.SENT).all()
            assert mut["fpp"][-1] == c["E"] - k and want["fpp"][-1] == c["E"]


def test_fp32_reciprocal_is_the_same_number():
    """1.0f / (float)n == (float)(1.0 / (double)n) for every integer 1 <= n < 2^24: "1 / n formed in fp32" is no wrong model"""
    n = np.arange(1, 2 ** 24, dtype=np.int64)
    assert np.array_equal(np.float32(1) / n.astype(np.float32), (1.0 / n.astype(np.float64)).astype(np.float32))
    up = [n_ for n_ in (3, 7, 11, 100, 1000) if float(np.float32(1.0 / n_)) > 1.0 / n_]
    assert up and all(M.recip32(n_, "recip_1ulp") == np.nextafter(M.recip32(n_), np.float32(0)) for n_ in up)
