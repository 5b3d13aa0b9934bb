"""The periodic rule on the host (no GPU needed): the numpy fp32 model of tests/test_gpu_pbc_matrix.py held to a float64 brute force over
the 27 neighbouring images; ``check_cell``; the CPU path of ``computeEdgeIndex`` held to the model exactly; the model shown to be sharp
(a wrong model disagrees with it on the cases' own inputs); and the kernels of e3k_pbc.o and the ``e3k_pbc_*`` functions of the header
held to the GPU case table.

Wrong models (planted in the numpy model, never in the library):
  plus_rint    +rint for -rint
  transposed   the cell used transposed
  no_shift     the shift ignored in the vector
  le           < replaced by <= at the cutoff
  wrap_all     a non-periodic axis wrapped
"""
import os
import re

import numpy as np
import pytest
import torch

from tests import test_gpu_pbc_matrix as M
from tests.test_batch_inventory import _shipped_kernels

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "e3k.h")
CASES = {c["id"]: c for c in M.CASES}
f32, f64 = np.float32, np.float64

_prepared = {}


def prep(cid):
    """(case, arena, inputs, expected words) -- prepared once per case and shared"""
    if cid not in _prepared:
        c = CASES[cid]
        ar, inp = M.prepared(c)
        _prepared[cid] = (c, ar, inp, M.expected(c, ar, inp))
    return _prepared[cid]


# ---------------------------------------------------------------------------------------------------------------------------------
# inventory
def test_every_pbc_kernel_has_an_exactly_checked_case(tmp_path):
    shipped = _shipped_kernels(tmp_path, "e3k_pbc")
    table = M.table_kernels()
    assert len(shipped) == 3, sorted(shipped)
    builders = {k for k in shipped if "nlist" in k}      # the one builder kernel of e3k_nlist_body.h, no copy of its own
    assert len(builders) == 2 and all(k.startswith("nlist_kernel<") for k in builders) and "pbc_nlist_kernel" not in str(shipped), builders
    assert shipped - table == set(), f"kernels without a case in test_gpu_pbc_matrix.CASES: {sorted(shipped - table)}"
    assert table - shipped == set(), f"the case table names kernels the library does not ship: {sorted(table - shipped)}"
    for k in shipped:
        assert any(k in c["kernels"] and c["kind"] != "refuse" for c in M.CASES), k


def test_every_pbc_function_of_the_header_is_called_by_a_case():
    with open(HEADER) as f:
        declared = set(re.findall(r"\b(e3k_pbc_\w+)\s*\(", f.read()))
    assert len(declared) == 3, sorted(declared)
    called = M.table_functions()
    assert declared == called, (sorted(declared - called), sorted(called - declared))
    for fn in declared:      # ... and refused by one
        assert any(c["kind"] == "refuse" and fn in c["funcs"] for c in M.CASES), fn
    ids = [c["id"] for c in M.CASES]
    assert len(ids) == len(set(ids)) and all(c["why"] for c in M.CASES)


@pytest.mark.parametrize("cid", [c["id"] for c in M.CASES])
def test_every_case_prepares_on_the_host(cid):
    c, ar, inp, want = prep(cid)
    for name, w in want.items():
        assert name in ar.blocks, name
        assert len(M._words(w)) <= ar.blocks[name][1], (name, len(M._words(w)), ar.blocks[name])
    if c["kind"] == "nlist":      # every index of the model's list is a node of the batch; every periodic width is wide enough
        m = inp["model"]
        assert m["e_cap"] == 0 or (0 <= m["ei"].min() and m["ei"].max() < inp["N"])
        for g in range(inp["G"]):
            assert (M.widths(inp["cell"][g].astype(f64))[inp["pbc"][g] != 0] > M.MIN_WIDTH).all()


# ---------------------------------------------------------------------------------------------------------------------------------
# premises: the boundaries the cases claim to cross
def test_cases_cross_their_boundaries():
    c, ar, inp, want = prep("nlist_sizes")
    m = inp["model"]
    assert np.diff(inp["node_ptr"])[:-1].tolist() == M.SIZES and not m["over"] and m["total"] == m["e_cap"]
    for g in (4, 5):      # sources of the 129- and 200-node graphs keep neighbours in more than one 64-wide round
        beg = int(inp["node_ptr"][g])
        rounds = {(int(j) - beg) // 64 for j in m["ei"][1][m["ei"][0] == beg + 70]}
        assert len(rounds) >= 2, rounds
    real = m["shift"][:m["total"]]
    assert np.abs(real).max() >= 3 and (real != 0).any(1).mean() > 0.5      # atoms up to +-3 cells outside: large image numbers
    assert {tuple(p) for p in inp["pbc"][:inp["G"]]} == {(1, 1, 1), (1, 1, 0)}
    assert prep("nlist_N1025")[2]["N"] == 1025 and 2048 < prep("nlist_N2100")[2]["N"] <= 3072
    assert prep("nlist_G1")[2]["G"] == 1 and prep("nlist_G0")[2]["G"] == 0
    m0 = prep("nlist_G0")[2]["model"]
    assert m0["total"] == 0 and m0["e_cap"] == 37 and not m0["shift"].any()
    c, ar, inp, want = prep("nlist_slab")
    m = inp["model"]
    assert not m["shift"][:, 2].any() and m["shift"][:, :2].any()
    c, ar, inp, want = prep("nlist_overflow_cut")
    m = inp["model"]
    i = int(np.searchsorted(m["offsets"], m["e_cap"], side="right")) - 1
    assert m["offsets"][i] < m["e_cap"] < m["offsets"][i + 1] and m["over"]
    assert m["n_edges"].sum() == m["e_cap"] and m["n_edges"][-1] == 0 and m["state"][1] == 6 and m["flag"] == 1 | 32
    assert m["shift"].any()
    m = prep("nlist_tail_3000")[2]["model"]
    assert m["e_cap"] - m["total"] == 3000 and not m["shift"][m["total"]:].any() and m["shift"][:m["total"]].any()
    m = prep("nlist_open")[2]["model"]
    assert not m["shift"].any() and m["total"] > 100
    # the planted pairs: on the cutoff dropped, one ulp inside kept -- through a face, an edge and a corner image
    c, ar, inp, want = prep("nlist_planted")
    m = inp["model"]
    edges = {tuple(p): tuple(s) for p, s in zip(m["ei"][:, :m["total"]].T, m["shift"][:m["total"]])}
    first = int(inp["node_ptr"][1])
    for k, (name, comp) in enumerate(M.PLANTS):
        on, inside = first + 4 * k, first + 4 * k + 2
        assert (on, on + 1) not in edges and (on + 1, on) not in edges, name
        image = tuple(-1 if x > 0 else 0 for x in comp)
        assert edges.get((inside, inside + 1)) == image and edges.get((inside + 1, inside)) == tuple(-x for x in image), name
        d = (inp["pos"][on + 1] - inp["pos"][on])[None]
        _, v, length, keep = M.pbc_rule(d, inp["cell"][1][None], inp["inv"][1][None], inp["pbc"][1][None])
        assert length[0] == f32(M.R_MAX) and not keep[0] and sorted(np.abs(v[0])) == sorted(comp), name
    for E in (0, 1, 255, 256, 257):
        assert prep(f"evf_E{E}")[2]["E"] == E
    inp = prep("evf_E257")[2]
    assert inp["real"].any() and inp["shift"].any()


# ---------------------------------------------------------------------------------------------------------------------------------
# the rule against a float64 brute force over the 27 neighbouring images
def _brute_force(pos, cell, pbc, r_max):
    """every (i, j, image) with |pos_j - pos_i + n . cell| < r_max in float64, n over the 27 images of the cell NEAREST to the pair (the
    images around the rounded fractional displacement: atoms may sit many cells apart)"""
    pos, cell = pos.astype(f64), cell.astype(f64)
    inv = np.linalg.inv(cell)
    out = {}
    for i in range(len(pos)):
        for j in range(len(pos)):
            if i == j:
                continue
            d = pos[j] - pos[i]
            base = -np.floor(d @ inv + 0.5) * (pbc != 0)
            for dn in np.ndindex(3, 3, 3):
                n = base + (np.array(dn) - 1) * (pbc != 0)
                v = d + n @ cell
                if np.linalg.norm(v) < r_max:
                    out.setdefault((i, j), set()).add((tuple(int(x) for x in n), tuple(v)))
    return {k: next(iter(v)) for k, v in out.items()}, {k for k, v in out.items() if len({n for n, _ in v}) > 1}


@pytest.mark.parametrize("kind", ["ortho", "tri", "slab"])
def test_the_rounding_rule_finds_the_brute_force_images(kind):
    rng = np.random.default_rng({"ortho": 1, "tri": 2, "slab": 3}[kind])
    n_close = n_pairs = 0
    for trial in range(3):
        cell, pbc = M.make_cell(kind, rng)
        frac = rng.uniform(0, 1, (40, 3)) + rng.integers(-3, 4, (40, 3))
        pos = (frac @ cell).astype(f32)
        cell32, inv32 = cell.astype(f32), np.linalg.inv(cell).astype(f32)
        brute, several = _brute_force(pos, cell32, pbc, M.R_MAX)
        assert not several      # the width rule: one image per ordered pair at most
        i, j = (a.ravel() for a in np.meshgrid(np.arange(40), np.arange(40), indexing="ij"))
        P = len(i)
        n, v, length, keep = M.pbc_rule(pos[j] - pos[i], np.broadcast_to(cell32, (P, 3, 3)), np.broadcast_to(inv32, (P, 3, 3)),
                                        np.broadcast_to(pbc, (P, 3)))
        keep &= i != j
        for q in range(P):
            pair = (int(i[q]), int(j[q]))
            d = pos[j[q]].astype(f64) - pos[i[q]].astype(f64)
            exact = np.linalg.norm(d + n[q].astype(f64) @ cell32.astype(f64))
            if i[q] == j[q]:
                continue
            n_pairs += 1
            if abs(exact - M.R_MAX) < 1e-6 or (pair in brute and abs(np.linalg.norm(brute[pair][1]) - M.R_MAX) < 1e-6):
                n_close += 1      # within 1e-6 of the cutoff: decided by the fp32 model (the planted pairs of the GPU table)
                continue
            assert keep[q] == (pair in brute), (pair, exact)
            if keep[q]:
                assert tuple(n[q]) == brute[pair][0]
                assert np.abs(v[q].astype(f64) - np.array(brute[pair][1])).max() < 1e-5
    assert n_close <= 0.01 * n_pairs


# ---------------------------------------------------------------------------------------------------------------------------------
# check_cell
def test_check_cell_accepts_and_refuses_at_the_margin():
    from e3_layers_amd.data.compute_edge import check_cell

    r = 4.0
    for axis in range(3):
        for factor, ok in ((1.002, True), (1.0005, False)):
            lengths = [30.0, 30.0, 30.0]
            lengths[axis] = 2 * r * factor
            cell = torch.diag(torch.tensor(lengths, dtype=torch.float64))
            tri = cell.clone()
            tri[axis] += 0.3 * cell[(axis + 1) % 3]      # shearing the axis' own vector along another keeps its perpendicular width
            for c in (cell, tri):
                both = torch.stack([torch.eye(3, dtype=torch.float64) * 30.0, c]).to(torch.float32)
                if ok:
                    check_cell(both, None, r)
                else:
                    with pytest.raises(ValueError, match=rf"graph 1, axis {'abc'[axis]}.*{2 * r * factor:.5g}"):
                        check_cell(both, None, r)
                pbc = torch.ones(2, 3, dtype=torch.int64)
                pbc[1, axis] = 0
                check_cell(both, pbc, r)      # the narrow axis is not periodic: ignored
    check_cell(torch.zeros(1, 3, 3), torch.zeros(1, 3), r)      # no periodic axis: any cell, the zero cell included
    with pytest.raises(ValueError, match="singular"):
        check_cell(torch.zeros(1, 3, 3), None, r)
    with pytest.raises(ValueError, match="axis c"):      # a tilted cell: the perpendicular width, not the vector's length, counts
        check_cell(torch.tensor([[30.0, 0, 0], [0, 30.0, 0], [0, 9.0, 5.0]]).reshape(1, 3, 3), None, 2.5)


# ---------------------------------------------------------------------------------------------------------------------------------
# the CPU path of computeEdgeIndex
def _batch(inp, with_pbc=True, cell=True):
    from e3_layers_amd.data.data import Batch, Data

    attrs = {"pos": ("node", "1x1o"), "cell": ("graph", "3x1o"), "pbc": ("graph", "3x0e")}
    samples = []
    for g in range(inp["G"]):
        a, b = int(inp["node_ptr"][g]), int(inp["node_ptr"][g + 1])
        t = dict(pos=torch.from_numpy(inp["pos"][a:b].copy()))
        if cell:
            t["cell"] = torch.from_numpy(inp["cell"][g].reshape(1, 9).copy())
            if with_pbc:
                t["pbc"] = torch.from_numpy(inp["pbc"][g].reshape(1, 3).astype(np.int64))
        samples.append(Data(attrs={k: v for k, v in attrs.items() if k in t}, **t))
    return Batch.from_data_list(samples, attrs={k: v for k, v in attrs.items() if k in samples[0]})


@pytest.mark.parametrize("cid", ["nlist_sizes", "nlist_triclinic", "nlist_slab", "nlist_planted", "nlist_open"])
def test_cpu_compute_edge_index_equals_the_model(cid):
    from e3_layers_amd.data.compute_edge import computeEdgeIndex

    c, ar, inp, want = prep(cid)
    m = inp["model"]
    assert not m["over"]
    batch = _batch(inp)
    assert batch["cell"].shape == (inp["G"], 9)
    new, attrs = computeEdgeIndex(batch.data, batch.attrs, r_max=M.R_MAX)
    assert attrs["edge_cell_shift"] == ("edge", "3x0e") and new["edge_cell_shift"].dtype == torch.int32
    assert np.array_equal(new["edge_index"].numpy(), m["ei"][:, :m["total"]])
    assert np.array_equal(new["edge_cell_shift"].numpy(), m["shift"][:m["total"]])
    assert np.array_equal(batch["_n_edges"].reshape(-1).numpy(), m["n_edges"][:-1])
    if cid == "nlist_open":      # pbc = 0: today's list on the same positions
        plain = _batch(inp, cell=False)
        old, _ = computeEdgeIndex(plain.data, plain.attrs, r_max=M.R_MAX)
        assert torch.equal(old["edge_index"], new["edge_index"]) and torch.equal(plain["_n_edges"], batch["_n_edges"])
        assert "edge_cell_shift" not in old and not new["edge_cell_shift"].any()


def test_pbc_defaults_to_periodic_everywhere():
    from e3_layers_amd.data.compute_edge import computeEdgeIndex

    c, ar, inp, want = prep("nlist_triclinic")
    a, b = _batch(inp), _batch(inp, with_pbc=False)
    assert "pbc" not in b
    new_a, _ = computeEdgeIndex(a.data, a.attrs, r_max=M.R_MAX)
    new_b, _ = computeEdgeIndex(b.data, b.attrs, r_max=M.R_MAX)
    assert torch.equal(new_a["edge_index"], new_b["edge_index"]) and torch.equal(new_a["edge_cell_shift"], new_b["edge_cell_shift"])


def test_a_cell_refuses_criteria_old_edges_and_narrow_cells():
    from e3_layers_amd.data.compute_edge import SequenceOrRandom, computeEdgeIndex

    c, ar, inp, want = prep("nlist_ortho")
    batch = _batch(inp)
    with pytest.raises(ValueError, match="criterion"):
        computeEdgeIndex(batch.data, batch.attrs, r_max=M.R_MAX, criteria=SequenceOrRandom("pos", 0, 0.5))
    with pytest.raises(ValueError, match="criterion"):
        computeEdgeIndex(batch.data, batch.attrs, r_max=M.R_MAX, criteria=lambda data, cand: torch.ones(cand.shape[1], dtype=torch.bool))
    with pytest.raises(ValueError, match="width"):
        computeEdgeIndex(batch.data, batch.attrs, r_max=2.5)
    new, attrs = computeEdgeIndex(batch.data, batch.attrs, r_max=M.R_MAX)
    batch.attrs.update(attrs)
    batch.update(new)
    with pytest.raises(ValueError, match="pre-existing"):
        computeEdgeIndex(batch.data, batch.attrs, r_max=M.R_MAX)


def test_wrap_positions_folds_periodic_axes_only():
    from e3_layers_amd.data.compute_edge import wrap_positions

    c, ar, inp, want = prep("nlist_slab")
    G = inp["G"]
    real = int(inp["node_ptr"][G])
    pos, cell, pbc = torch.from_numpy(inp["pos"][:real]), torch.from_numpy(inp["cell"][:G]), torch.from_numpy(inp["pbc"][:G])
    out = wrap_positions(pos, cell, pbc, torch.from_numpy(inp["node_ptr"][:G + 1]))
    seg = inp["node_seg"][:real]
    frac = np.einsum("nc,nck->nk", out.double().numpy(), np.linalg.inv(inp["cell"][:G].astype(f64))[seg])
    assert (frac[:, :2] > -1e-5).all() and (frac[:, :2] < 1 + 1e-5).all()
    moved = np.einsum("nc,nck->nk", (out - pos).double().numpy(), np.linalg.inv(inp["cell"][:G].astype(f64))[seg])
    assert np.abs(moved - np.rint(moved)).max() < 1e-4 and not np.rint(moved[:, 2]).any() and np.rint(moved[:, :2]).any()


# ---------------------------------------------------------------------------------------------------------------------------------
# the table is sharp
def _disagreeing(mutant):
    out = []
    for cid, c in CASES.items():
        if c["kind"] != "refuse":
            _, ar, inp, want = prep(cid)
            mut = M.expected(c, ar, inp, mutant)
            if any(not np.array_equal(M._words(want[k]), M._words(mut[k])) for k in want):
                out.append(cid)
    return out


MUTANTS = [
    ("plus_rint", {"nlist_sizes", "nlist_ortho", "nlist_triclinic", "nlist_slab", "nlist_G1", "nlist_planted"}),
    ("transposed", {"nlist_triclinic", "nlist_G1", "evf_triclinic", "evf_E257"}),
    ("no_shift", {"evf_E255", "evf_E256", "evf_E257", "evf_no_len", "evf_triclinic"}),
    ("le", {"nlist_planted"}),
    ("wrap_all", {"nlist_slab", "nlist_sizes"}),
]


@pytest.mark.parametrize("mutant,must", MUTANTS, ids=[m[0] for m in MUTANTS])
def test_a_wrong_model_disagrees_on_the_cases_own_inputs(mutant, must):
    noticed = set(_disagreeing(mutant))
    print(f"{mutant}: {len(noticed)} cases disagree: {sorted(noticed)}")
    assert must and must <= noticed, f"{mutant}: not noticed by {sorted(must - noticed)}"
    assert "nlist_open" not in noticed or mutant == "wrap_all"      # pbc = 0: no shift to get wrong
    if mutant == "transposed":
        assert "nlist_ortho" not in noticed      # (a diagonal cell is its own transpose)
    if mutant == "le":
        assert noticed == {"nlist_planted"}
