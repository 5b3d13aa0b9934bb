"""The all-images periodic list on the host (no GPU needed): ``image_ranges`` at its margins; the CPU path of
``computeEdgeIndex(images="all")`` held to the float64 brute force and to the numpy fp32 model of tests/test_gpu_images_matrix.py, as
ordered lists; wide cells (the minimum-image list exactly); the physics in float64 with the oracle (a narrow cell against its
supercell); the refusals; the premises of the GPU tests' fixtures; and the kernels of e3k_images.o and the ``e3k_images_*`` functions of
the header held to the GPU case table.

The supercell bound.  The oracle in float64 on a narrow cell's all-images list and on its supercell's minimum-image list computes the
same sums in another order.  Its own reordering scale is measured here -- the same supercell with its atoms permuted -- and asserted
to be below 1e-12 (normwise); the bound for cell against supercell is 1e-10: float64's 1.1e-16 times the few thousand terms of the
sums over edges and channels, with two orders to spare, and five orders below what a missing or doubled edge would change
(asserted: dropping ONE edge moves the energy by more than 1e-7)."""
import os
import re

import numpy as np
import pytest
import torch

from oracle import e3ref
from tests import test_gpu_images_force_field as F
from tests import test_gpu_images_matrix as M
from tests.test_batch_inventory import _shipped_kernels
from tests.test_gpu_md import _small_tree
from tests.test_virial_host import oracle_strain_gradient

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
def test_the_images_object_ships_exactly_the_two_builder_instances(tmp_path):
    shipped = _shipped_kernels(tmp_path, "e3k_images")
    assert shipped == M.NL_K, sorted(shipped)      # the one builder kernel of e3k_nlist_body.h, no copy of its own
    assert shipped == M.table_kernels()
    for k in shipped:
        assert any(k in c["kernels"] and c["kind"] != "refuse" for c in M.CASES), k
    # ... and the three existing rules' objects ship what they shipped: the trait added no kernel to them
    assert {k for k in _shipped_kernels(tmp_path, "e3k_pbc") if "nlist" in k} == {f"nlist_kernel<{a}, e3k::PeriodicRule>" for a in ("false", "true")}


def test_every_images_function_of_the_header_is_called_and_refused_by_a_case():
    with open(HEADER) as f:
        declared = set(re.findall(r"\b(e3k_images_\w+)\s*\(", f.read()))
    assert declared == {"e3k_images_count", "e3k_images_fill"}, sorted(declared)
    assert declared == M.table_functions()
    for fn in declared:
        assert any(c["kind"] == "nlist" and fn in c["funcs"] for c in M.CASES), fn
        assert any(c["kind"] == "refuse" and fn in c["funcs"] for c in M.CASES), fn
    ids = [c["id"] for c in M.CASES]
    assert len(ids) == len(set(ids)) and all(c["why"] for c in M.CASES)
    from e3_layers_amd.backend import abi
    from e3_layers_amd.data.compute_edge import IMAGES_MAX_RANGE

    assert abi.load().defines["E3K_IMAGES_MAX_RANGE"] == IMAGES_MAX_RANGE == M.MAX_RANGE


@pytest.mark.parametrize("cid", [c["id"] for c in M.CASES])
def test_every_case_prepares_on_the_host(cid):
    """the arena holds every block the model names, the model's words fit, every index is a node of the batch -- and (``M.geometry``,
    asserted where the fixture is made) no candidate is within 1e-4 r_max of the cutoff, the ranges are needed, and the fp32 model's
    list is the float64 brute force's"""
    c, ar, inp, want = prep(cid)
    for name, w in want.items():
        assert name in ar.blocks, name
        assert len(M._words(w)) <= ar.blocks[name][1], (name, len(M._words(w)), ar.blocks[name])
    if c["kind"] == "nlist":
        m = inp["model"]
        assert m["e_cap"] == 0 or (0 <= m["ei"].min() and m["ei"].max() < inp["N"])
        assert len(inp["brute"][0]) == m["total"]


# ---------------------------------------------------------------------------------------------------------------------------------
# premises: the boundaries the cases claim to cross
def _rounds(inp, i, r_max):
    """the 64-candidate rounds in which source i keeps edges"""
    g = int(inp["node_seg"][i])
    beg = int(inp["node_ptr"][g])
    R = M.effective(inp["range"][g], inp["pbc"][g])
    j, _, m = M.source_edges(inp, i, r_max)
    w = 2 * R + 1
    q = (j - beg) * int(w.prod()) + ((m[:, 0] + R[0]) * w[1] + (m[:, 1] + R[1])) * w[2] + (m[:, 2] + R[2])
    assert (np.diff(q) > 0).all()      # the model's list is in ascending candidate order
    return set((q // 64).tolist())


def test_cases_cross_their_boundaries():
    c, ar, inp, want = prep("one_atom")
    m = inp["model"]
    assert m["total"] == 18 and (m["ei"][0, :18] == 0).all() and (m["ei"][1, :18] == 0).all() and tuple(inp["range"][0]) == (2, 2, 2)
    n2 = (m["shift"][:18].astype(np.int64) ** 2).sum(1)
    assert sorted(n2.tolist()) == [1] * 6 + [2] * 12      # 6 at L, 12 at sqrt(2) L: all self images
    assert tuple(prep("two_triclinic")[2]["range"][0]) == (1, 1, 1) and prep("two_triclinic")[2]["N"] == 2 + 5
    inp = prep("slab")[2]
    assert tuple(inp["pbc"][0]) == (1, 1, 0) and not inp["model"]["shift"][:, 2].any() and inp["model"]["shift"][:, :2].any()
    inp = prep("batch3")[2]
    assert [tuple(r) for r in inp["range"][:3]] == [(0, 0, 0), (1, 1, 1), (2, 1, 0)] and all(inp["model"]["n_edges"][:3] > 0)
    inp = prep("unwrapped")[2]
    base = np.rint(np.einsum("nc,nck->nk", inp["pos"][:7].astype(f64), np.linalg.inv(inp["cell"][:2].astype(f64))[inp["node_seg"][:7]]))
    assert np.abs(base).max() >= 2 and np.abs(inp["model"]["shift"]).max() >= 3      # atoms cells apart: large image numbers
    for cid, n, seam in (("n3_M27", 3, 64), ("n5_M27", 5, 128)):
        inp = prep(cid)[2]
        assert tuple(inp["range"][0]) == (1, 1, 1) and (n - 1) * 27 < seam < n * 27
        assert any(len(_rounds(inp, i, M.R_MAX)) >= 2 for i in range(n)), cid      # a source's kept edges cross a lane seam
    assert len(_rounds(prep("n5_M27")[2], 0, M.R_MAX) | _rounds(prep("n5_M27")[2], 1, M.R_MAX)) == 3
    inp = prep("n70_M1")[2]
    assert len(_rounds(inp, 0, M.R_MAX)) == 2 and tuple(inp["range"][1]) == (2, 2, 0)
    m = prep("tail")[2]["model"]
    assert m["e_cap"] - m["total"] == 300 and not m["shift"][m["total"]:].any() and not m["over"]
    m = prep("cut_one_short")[2]["model"]
    assert m["e_cap"] == m["total"] - 1 and m["over"] and m["flag"] == 1 | 32 and m["state"][1] == 6 and m["n_edges"].sum() == m["e_cap"]
    assert m["n_edges"][-1] == 0
    inp = prep("empty_graph")[2]
    assert np.diff(inp["node_ptr"]).tolist()[:3] == [3, 0, 4] and inp["model"]["n_edges"][1] == 0
    m0 = prep("G0")[2]["model"]
    assert m0["total"] == 0 and m0["e_cap"] == 29 and not m0["shift"].any()
    inp = prep("table_malformed")[2]
    assert inp["range"].max() > M.MAX_RANGE and inp["range"].min() < 0 and inp["range"][0][2] != 0 and inp["pbc"][0][2] == 0
    assert (M.effective(inp["range"][:2], inp["pbc"][:2]) >= inp["true_range"][:2]).all()      # still complete
    inp = prep("zero_ranges")[2]
    assert not inp["range"].any() and inp["model"]["shift"].any() and {tuple(p) for p in inp["pbc"][:3]} == {(1, 1, 1), (1, 1, 0)}


# ---------------------------------------------------------------------------------------------------------------------------------
# image_ranges
def test_image_ranges_at_the_margins():
    from e3_layers_amd.data import image_ranges

    r = 4.0
    reach = r * (1 + 1e-3)
    for R in (0, 1, 2, 3, 7):
        threshold = reach / (R + 0.5)
        for axis in range(3):
            for factor, want in ((1 + 1e-6, R), (1 - 1e-6, R + 1)):
                lengths = [30.0, 30.0, 30.0]
                lengths[axis] = threshold * factor
                cell = torch.diag(torch.tensor(lengths, dtype=torch.float64))
                tri = cell.clone()
                tri[axis, (axis + 1) % 3] = 0.3 * threshold      # shearing the axis' own vector along another keeps its perpendicular width
                for c in (cell, tri):
                    both = torch.stack([torch.eye(3, dtype=torch.float64) * 30.0, c])
                    if want > 7:
                        with pytest.raises(ValueError, match=rf"graph 1, axis {'abc'[axis]}.*range of 8.*not served"):
                            image_ranges(both, None, r)
                        continue
                    got = image_ranges(both, None, r)
                    assert got.dtype == torch.int32 and got.shape == (2, 3) and got.device.type == "cpu"
                    expect = [0, 0, 0]
                    expect[axis] = want
                    assert got.tolist() == [[0, 0, 0], expect], (R, axis, factor, got)
                    pbc = torch.ones(2, 3, dtype=torch.int64)
                    pbc[1, axis] = 0
                    assert not image_ranges(both, pbc, r).any()      # the narrow axis is not periodic: range 0
    # a tilted cell: the perpendicular width (4.37 along c: range 1), not the vector's length (10.3: range 0), counts
    tilted = torch.tensor([[30.0, 0, 0], [0, 30.0, 0], [0, 9.0, 5.0]]).reshape(1, 3, 3)
    assert image_ranges(tilted, None, 2.5).tolist() == [[0, 0, 1]]
    # mixed pbc; numpy's restatement of the formula agrees on random triclinic cells
    rng = np.random.default_rng(0)
    for _ in range(50):
        cell = np.diag(rng.uniform(1.0, 9.0, 3)) + rng.uniform(-1, 1, (3, 3)) * (1 - np.eye(3))
        pbc = rng.integers(0, 2, 3)
        assert image_ranges(torch.from_numpy(cell)[None], torch.from_numpy(pbc)[None], r).tolist() == [M.ranges(cell, pbc, r).tolist()]
    # a cell check_cell accepts has range zero
    wide = torch.eye(3).reshape(1, 3, 3) * (2 * reach * 1.0001)
    from e3_layers_amd.data import check_cell

    check_cell(wide, None, r)
    assert not image_ranges(wide, None, r).any()
    # singular and non-finite cells
    assert not image_ranges(torch.zeros(1, 3, 3), torch.zeros(1, 3), r).any()      # no periodic axis: any cell, the zero cell included
    with pytest.raises(ValueError, match="graph 0.*singular"):
        image_ranges(torch.zeros(1, 3, 3), None, r)
    bad = torch.eye(3).reshape(1, 3, 3) * 5.0
    bad[0, 1, 1] = float("nan")
    with pytest.raises(ValueError, match="singular"):
        image_ranges(bad, None, r)
    with pytest.raises(ValueError, match="graph 0, axis b.*not served"):      # the cap
        image_ranges(torch.diag(torch.tensor([5.0, 0.5, 5.0])).reshape(1, 3, 3), None, r)


# ---------------------------------------------------------------------------------------------------------------------------------
# the CPU path of computeEdgeIndex(images="all")
def _batch(inp):
    from e3_layers_amd.data.data import Batch, Data

    attrs = {"pos": ("node", "1x1o"), "cell": ("graph", "3x1o"), "pbc": ("graph", "3x0e")}
    samples = []
    for g in range(inp["G"]):
        a, b = int(inp["node_ptr"][g]), int(inp["node_ptr"][g + 1])
        samples.append(Data(attrs=dict(attrs), pos=torch.from_numpy(inp["pos"][a:b].copy()), cell=torch.from_numpy(inp["cell"][g].reshape(1, 9).copy()),
                            pbc=torch.from_numpy(inp["pbc"][g].reshape(1, 3).astype(np.int64))))
    return Batch.from_data_list(samples, attrs=dict(attrs))


@pytest.mark.parametrize("cid", ["one_atom", "two_triclinic", "slab", "batch3", "unwrapped", "n5_M27", "n70_M1"])
def test_cpu_all_images_list_equals_the_brute_force_as_an_ordered_list(cid):
    from e3_layers_amd.data import computeEdgeIndex

    c, ar, inp, want = prep(cid)
    m, (bs, bd, bn) = inp["model"], inp["brute"]
    assert not m["over"]
    batch = _batch(inp)
    new, attrs = computeEdgeIndex(batch.data, batch.attrs, r_max=c["r_max"], images="all")
    assert attrs["edge_cell_shift"] == ("edge", "3x0e") and new["edge_cell_shift"].dtype == torch.int32
    assert attrs["_image_range"] == ("graph", "3x0e") and np.array_equal(batch["_image_range"].numpy(), inp["true_range"][:inp["G"]])
    ei, shift = new["edge_index"].numpy(), new["edge_cell_shift"].numpy()
    assert np.array_equal(ei[0], bs) and np.array_equal(ei[1], bd) and np.array_equal(shift, bn)      # the float64 brute force
    assert np.array_equal(ei, m["ei"][:, :m["total"]]) and np.array_equal(shift, m["shift"][:m["total"]])      # the fp32 model
    assert np.array_equal(batch["_n_edges"].reshape(-1).numpy(), m["n_edges"][:-1])
    if cid == "one_atom":
        assert ei.shape[1] == 18
    # a batch that carries the table gets the same list without the keyword -- the table is trusted ...
    batch.attrs.update(attrs)
    again, _ = computeEdgeIndex(batch.data, batch.attrs, r_max=c["r_max"])
    assert torch.equal(again["edge_index"], new["edge_index"]) and torch.equal(again["edge_cell_shift"], new["edge_cell_shift"])
    if m["total"] and inp["true_range"].any():
        batch["_image_range"] = torch.zeros_like(batch["_image_range"])
        fewer, _ = computeEdgeIndex(batch.data, batch.attrs, r_max=c["r_max"])
        assert fewer["edge_index"].shape[1] < m["total"]
        # ... and images="all" always recomputes it
        full, _ = computeEdgeIndex(batch.data, batch.attrs, r_max=c["r_max"], images="all")
        assert torch.equal(full["edge_index"], new["edge_index"]) and np.array_equal(batch["_image_range"].numpy(), inp["true_range"][:inp["G"]])


def test_on_wide_cells_the_all_images_list_is_the_minimum_image_list():
    from e3_layers_amd.data import computeEdgeIndex

    c, ar, inp, want = prep("zero_ranges")
    a, b = _batch(inp), _batch(inp)
    new_a, _ = computeEdgeIndex(a.data, a.attrs, r_max=M.R_MAX, images="all")
    new_b, _ = computeEdgeIndex(b.data, b.attrs, r_max=M.R_MAX, images="minimum")
    new_c, _ = computeEdgeIndex(_batch(inp).data, _batch(inp).attrs, r_max=M.R_MAX)
    assert new_a["edge_index"].shape[1] > 500 and new_a["edge_cell_shift"].any()
    for other in (new_b, new_c):
        assert torch.equal(new_a["edge_index"], other["edge_index"]) and torch.equal(new_a["edge_cell_shift"], other["edge_cell_shift"])
    assert torch.equal(a["_n_edges"], b["_n_edges"]) and "_image_range" not in b and not a["_image_range"].any()


def test_the_table_collates_and_pads_like_pbc():
    from e3_layers_amd.data import computeEdgeIndex
    from e3_layers_amd.run.graph_step import pad_batch

    c, ar, inp, want = prep("batch3")
    batch = _batch(inp)
    new, attrs = computeEdgeIndex(batch.data, batch.attrs, r_max=M.R_MAX, images="all")
    batch.attrs.update(attrs)
    batch.update(new)
    padded = pad_batch(batch, 32, 1024)
    assert padded["_image_range"].shape == (4, 3) and padded["_image_range"][:3].tolist() == inp["true_range"][:3].tolist()
    assert not padded["_image_range"][3].any() and not padded["pbc"][3].any() and not padded["cell"][3].any()
    assert padded[[1]]["_image_range"].tolist() == [[1, 1, 1]]


# ---------------------------------------------------------------------------------------------------------------------------------
# refusals
def test_refusals():
    from e3_layers_amd.data import computeEdgeIndex
    from e3_layers_amd.data.compute_edge import SequenceOrRandom
    from e3_layers_amd.run.md import Barostat, ReplayedForceField, VelocityVerlet

    c, ar, inp, want = prep("batch3")
    batch = _batch(inp)
    with pytest.raises(ValueError, match="images must be one of"):
        computeEdgeIndex(batch.data, batch.attrs, r_max=M.R_MAX, images="nearest")
    with pytest.raises(ValueError, match="width"):      # the narrow-cell refusal of the default stays
        computeEdgeIndex(batch.data, batch.attrs, r_max=M.R_MAX)
    with pytest.raises(ValueError, match="width"):
        computeEdgeIndex(batch.data, batch.attrs, r_max=M.R_MAX, images="minimum")
    with pytest.raises(ValueError, match="criterion"):
        computeEdgeIndex(batch.data, batch.attrs, r_max=M.R_MAX, images="all", criteria=SequenceOrRandom("pos", 0, 0.5))
    new, attrs = computeEdgeIndex(batch.data, batch.attrs, r_max=M.R_MAX, images="all")
    batch.attrs.update(attrs)
    batch.update(new)
    with pytest.raises(ValueError, match="pre-existing"):
        computeEdgeIndex(batch.data, batch.attrs, r_max=M.R_MAX, images="all")
    open_batch = F.crystal_batch()
    open_batch.pop("cell")
    with pytest.raises(ValueError, match="needs a periodic batch"):
        computeEdgeIndex(open_batch.data, open_batch.attrs, r_max=4.0, images="all")
    with pytest.raises(ValueError, match="images must be one of"):
        ReplayedForceField(None, F.crystal_batch(), 4.0, images="every")
    with pytest.raises(ValueError, match="needs a periodic batch"):
        ReplayedForceField(None, open_batch, 4.0, images="all")

    class Field:      # what VelocityVerlet looks at before it refuses
        images, cell, pbc, virial_key = "all", F.CELLS, torch.ones(2, 3, dtype=torch.bool), "virial"
        pos, node_ptr = torch.zeros(16, 3), torch.tensor([0, 8, 16])

    with pytest.raises(ValueError, match="images='all' is not served"):
        VelocityVerlet(Field(), torch.ones(16), 0.5, barostat=Barostat(p0=0.0, compressibility=1.0, tau=10.0, mode="berendsen"))


def test_set_cell_beyond_the_cap_changes_nothing():
    """``set_cell`` on a force field with images="all" (its captured state stood in for by host tensors): a range of 9 is refused before
    anything changes; a legal cell overwrites cell, inverse and table in place and leaves the ghost graph's rows zero."""
    from e3_layers_amd.run.md import ReplayedForceField

    ff = object.__new__(ReplayedForceField)
    ff.images, ff.r_max, ff.n_graphs, ff.valid = "all", F.R_MAX, 2, True
    ff.cell = F.CELLS.float().clone()
    ff.pbc = torch.ones(2, 3, dtype=torch.bool)
    ff.volume = None
    ff._base = {"_n_nodes": torch.tensor([[8], [8]])}
    data = {"cell": torch.cat([F.CELLS.float().reshape(2, 9), torch.zeros(1, 9)]), "_inv_cell": torch.zeros(3, 9),
            "_image_range": torch.tensor(F.RANGES + [[0, 0, 0]], dtype=torch.int32)}
    ff.static = type("Static", (), {"data": data})()
    before = {k: v.clone() for k, v in data.items()}
    with pytest.raises(ValueError, match=r"graph 1, axis a.*range of 9.*not served"):
        ff.set_cell(F.CELLS @ torch.diag(torch.tensor([0.19, 1.0, 1.0], dtype=torch.float64)))
    assert all(torch.equal(data[k], before[k]) for k in data) and ff.valid and torch.equal(ff.cell, F.CELLS.float())
    cells, _ = F.strained_cells()
    ff.set_cell(cells)
    assert ff.image_range.tolist() == F.STRAINED_RANGES and data["_image_range"][2].tolist() == [0, 0, 0] and not ff.valid
    assert torch.equal(data["cell"][:2], cells.float().reshape(2, 9)) and not data["cell"][2].any() and not data["_inv_cell"][2].any()
    assert torch.allclose(data["_inv_cell"][:2].reshape(2, 3, 3).double(), torch.linalg.inv(cells.float().double()), rtol=1e-6, atol=1e-7)


# ---------------------------------------------------------------------------------------------------------------------------------
# physics, in float64 with the oracle
def test_the_crystal_fixture_of_the_force_field_tests():
    from e3_layers_amd.data import check_cell, image_ranges

    batch = F.crystal_batch()
    assert image_ranges(batch["cell"], batch["pbc"], F.R_MAX).tolist() == F.RANGES
    ei, shift, n_edges = F.host_list(batch, batch["pos"])
    cell = batch["cell"].reshape(-1, 3, 3).double()
    seg = batch["_node_segment"][ei[0]]
    vec = batch["pos"].double()[ei[1]] - batch["pos"].double()[ei[0]] + torch.einsum("ek,ekc->ec", shift.double(), cell[seg])
    length = vec.norm(dim=1)
    assert float(length.min()) > 1.5 and float(length.max()) < F.R_MAX      # no two atoms, images included, closer than a bond length
    assert (ei[0] == ei[1]).any() and n_edges.reshape(-1).tolist() == [int((seg == g).sum()) for g in (0, 1)]
    for g in (0, 1):      # images on every axis that has a range (that the ranges are NEEDED is shown on tests/test_gpu_images_matrix.py's fixtures)
        assert (shift[seg == g].abs().max(0).values >= torch.tensor(F.RANGES[g]).clamp(max=1)).all()
    cells, _ = F.strained_cells()
    assert image_ranges(cells, None, F.R_MAX).tolist() == F.STRAINED_RANGES
    strained = F.crystal_batch(cells=cells)
    assert F.host_list(strained, strained["pos"])[0].shape[1] > 1.3 * ei.shape[1]      # the list a set_cell to them has to hold
    for g, reps in ((0, (3, 3, 3)), (1, (4, 2, 1))):      # the supercells pass check_cell
        big = F.crystal_batch(graphs=(g,), reps=reps)
        check_cell(big["cell"], big["pbc"], F.R_MAX)
        assert big["pos"].shape[0] == 8 * reps[0] * reps[1] * reps[2]


@pytest.mark.parametrize("g, reps", [(0, (3, 3, 3)), (1, (4, 2, 1))], ids=["111_3x3x3", "210_4x2x1"])
def test_a_narrow_cell_equals_its_supercell_in_float64(g, reps):
    """energy x copies, forces atom by atom and stress of the narrow cell on its all-images list == the supercell's on its
    minimum-image list (3 x 3 x 3 for the cell with ranges (1, 1, 1); 4 x 2 x 1 for the one with (2, 1, 0), whose 3 x 3 x 3
    supercell is 7.1 A wide along a and does not pass check_cell)."""
    torch.manual_seed(0)
    net = e3ref.build(_small_tree()).double().eval().func
    small, big = F.crystal_batch(graphs=(g,)), F.crystal_batch(graphs=(g,), reps=reps)
    k = reps[0] * reps[1] * reps[2]
    e, f, w, s, n = F.oracle_outputs(net, small, small["pos"])
    e_big, f_big, w_big, s_big, n_big = F.oracle_outputs(net, big, big["pos"], images="minimum")
    assert n_big == k * n and float(f.abs().max()) > 1e-3 and float(s.abs().max()) > 1e-5
    rel = lambda a, b: float((a - b).norm() / b.norm())
    errs = [rel(k * e, e_big), rel(f.repeat(k, 1), f_big), rel(s, s_big), rel(k * w, w_big)]
    # the oracle's own reordering scale: the supercell with its atoms permuted
    perm = torch.randperm(big["pos"].shape[0], generator=torch.Generator().manual_seed(1))
    mixed = big.clone()
    mixed["pos"], mixed["species"] = big["pos"][perm], big["species"][perm]
    e_mix, f_mix, _, s_mix, _ = F.oracle_outputs(net, mixed, mixed["pos"], images="minimum")
    own = [rel(e_mix, e_big), rel(f_mix, f_big[perm]), rel(s_mix, s_big)]
    # what one missing edge changes
    ei, shift, _ = F.host_list(small, small["pos"])
    cell = small["cell"].reshape(-1, 3, 3).double()
    e_less = oracle_strain_gradient(net, small, small["pos"], ei[:, 1:], shift[1:], cell)[0]
    print(f"supercell {g}: cell against supercell {errs}, the oracle reordered {own}, one edge dropped {rel(e_less, e):.3g}")
    assert max(own) < 1e-12, own
    assert max(errs) < 1e-10, errs
    assert rel(e_less, e) > 1e-7
