"""Periodic cells in the replayed force field and MD (run/md.py with a ``cell`` in the batch) on the device: against the eager path,
against the float64 oracle on the periodic list, under lattice translations, in a vacuum cell, across a regrowth, and in energy
conservation.  The small tree, the sizes and the tolerances are those of tests/test_gpu_md.py.

The oracle knows no cell: it is given the periodic list (the project's CPU ``computeEdgeIndex``) and a differentiable float64
``edge_vector = pos[dst] - pos[src] + shift @ cell`` built here; ``oracle/e3ref.compute_edge_vector`` keeps a present ``edge_vector``,
and its gradient head differentiates with respect to a ``pos`` that already requires grad as it is, so the forces are
``-dE/dpos`` through that vector.

The three molecules sit across a face of their cells (wrapped into them along the first axis), so that 20-40 % of the edges carry a
non-zero image number (asserted); one cell is orthorhombic, one triclinic, one a slab (pbc = 1, 1, 0)."""
import pytest
import torch

from tests.test_gpu_md import FTOL, REPLAY, TOL, _build, _device_verlet, _oracle, _oracle_verlet, _small_tree
from tests.util import rel_err, zero_shifts

pytestmark = pytest.mark.gpu

R_MAX = 4.0
E_KEY = "energy_total"
# rows = lattice vectors; every perpendicular width along a periodic axis exceeds 2 r_max (1 + 1e-3) = 8.008
CELLS = torch.tensor([[[9.0, 0.0, 0.0], [0.0, 10.0, 0.0], [0.0, 0.0, 9.5]],
                      [[9.5, 0.0, 0.0], [1.5, 10.0, 0.0], [-1.0, 2.0, 11.0]],
                      [[9.25, 0.0, 0.0], [0.0, 9.75, 0.0], [0.0, 0.0, 30.0]]], dtype=torch.float64)
PBC = torch.tensor([[1, 1, 1], [1, 1, 1], [1, 1, 0]], dtype=torch.int64)
# where the molecule's centre goes, in fractional coordinates: a little inside the face a = 0, in the middle of the other two axes
CENTRE = torch.tensor([[0.12, 0.5, 0.5], [0.10, 0.5, 0.5], [0.13, 0.5, 0.5]], dtype=torch.float64)


def _wrap(pos, cell, pbc, seg):
    """float64: fractional coordinates of the periodic axes folded into [0, 1)"""
    inv = torch.linalg.inv(cell)
    frac = torch.einsum("nc,nck->nk", pos, inv[seg])
    frac = torch.where(pbc[seg] != 0, frac - torch.floor(frac), frac)
    return torch.einsum("nk,nkc->nc", frac, cell[seg])


def _periodic_batch(cells=CELLS, pbc=PBC, centre=CENTRE, wrap=True):
    """synth_qm9(7, 3) (the batch of tests/test_gpu_md.py) with a cell per molecule; host batch without a list"""
    from e3_layers_amd.data.synthetic import synth_qm9

    batch = synth_qm9(7, 3)
    for k in ("edge_index", "_n_edges", "_edge_segment"):
        batch.pop(k)
    seg = batch["_node_segment"]
    pos = batch["pos"].double() + torch.einsum("nk,nkc->nc", centre[seg], cells[seg])
    batch["pos"] = (_wrap(pos, cells, pbc, seg) if wrap else pos).float()
    batch.attrs["cell"], batch.attrs["pbc"] = ("graph", "3x1o"), ("graph", "3x0e")
    batch["cell"] = cells.float().reshape(-1, 9)
    batch["pbc"] = pbc.clone()
    return batch


def _host_list(batch, pos):
    """(edge_index, shift) of the project's CPU path at ``pos``"""
    from e3_layers_amd.data import computeEdgeIndex

    b = batch.clone()
    b["pos"] = pos.detach().float().cpu()
    for k in ("edge_index", "_n_edges", "_edge_segment", "edge_cell_shift"):
        b.pop(k)
    new, _ = computeEdgeIndex(b.data, b.attrs, r_max=R_MAX)
    return new["edge_index"], new["edge_cell_shift"], b["_n_edges"]


class _PeriodicOracleField:
    """The oracle as a periodic force field on the host: the periodic list at the given positions, a differentiable
    ``edge_vector`` with the image shifts in it, the network, forces by autograd through that vector."""

    def __init__(self, orc, batch, dtype=torch.float64):
        self.orc, self.batch, self.dtype = orc, batch, dtype
        self.cell = batch["cell"].reshape(-1, 3, 3).to(dtype)
        self.edge_counts, self.shifts = [], []

    def __call__(self, x):
        b = self.batch
        ei, shift, n_edges = _host_list(b, x)
        pos = x.detach().to(self.dtype).clone().requires_grad_(True)
        g = b["_node_segment"][ei[0]]
        vec = pos[ei[1]] - pos[ei[0]] + torch.einsum("ek,ekc->ec", shift.to(self.dtype), self.cell[g])
        data = {"pos": pos, "species": b["species"], "_n_nodes": b["_n_nodes"], "edge_index": ei, "_n_edges": n_edges, "edge_vector": vec}
        attrs = {k: b.attrs[k] for k in ("pos", "species")}
        attrs.update(edge_vector=("edge", "1x1o"), _n_edges=("graph", "1x0e"))
        self.edge_counts.append(int(ei.shape[1]))
        self.shifts.append(shift)
        out, _ = self.orc(data, attrs)
        return out[E_KEY].detach().reshape(-1), out["forces"].detach()


def _eager(prod, batch, pos, dev):
    from e3_layers_amd.data import computeEdgeIndex

    b = batch.clone().to(dev)
    b["pos"] = pos.to(dev, torch.float32)
    new, attrs = computeEdgeIndex(b.data, b.attrs, r_max=R_MAX)
    b.attrs.update(attrs)
    b.update(new)
    return prod(b), new


def _ff(prod, batch, dev, **kw):
    from e3_layers_amd.run.md import ReplayedForceField

    return ReplayedForceField(prod, batch.clone().to(dev), R_MAX, energy_key=E_KEY, forces_key="forces", **kw)


def _list_of(ff):
    """the real edges of the force field's last list: (edge_index [2, E], shift [E, 3], edge_vector [E, 3] or None) on the host"""
    e = int(ff.n_edges)
    return ff.static["edge_index"][:, :e].cpu(), ff.static["edge_cell_shift"][:e].cpu()


def test_the_batch_crosses_its_cells_faces():
    """20-40 % of the edges carry a non-zero image number (host only: the premise of every test below)"""
    batch = _periodic_batch()
    ei, shift, _ = _host_list(batch, batch["pos"])
    share = float((shift != 0).any(1).float().mean())
    print("crossing share", share, int(ei.shape[1]))
    assert 0.2 <= share <= 0.4, share
    assert not shift[batch["_node_segment"][ei[0]] == 2][:, 2].any()      # the slab's third axis is never wrapped


def test_periodic_force_field_equals_eager_and_the_oracle(dev):
    """ff(pos) on moved positions (the edge count changes) == eager computeEdgeIndex + the model on the unpadded periodic batch
    (REPLAY), and within TOL / FTOL of the float64 oracle on the periodic list at every evaluation."""
    tree = _small_tree()
    prod = _build(tree, dev)
    orc = _oracle(prod, tree)
    zero_shifts(prod, orc)
    batch = _periodic_batch()
    field = _PeriodicOracleField(orc, batch)
    ff = _ff(prod, batch, dev)
    assert torch.equal(ff.cell.cpu(), CELLS.float()) and torch.equal(ff.pbc.cpu(), PBC != 0)
    gen = torch.Generator().manual_seed(11)
    counts = []
    for step, scale in enumerate((0.0, 0.25, 0.4, 0.15)):
        pos = batch["pos"] + scale * torch.randn(batch["pos"].shape, generator=gen)
        energy, forces = ff(pos.to(dev))
        ff.check()
        out, new = _eager(prod, batch, pos, dev)
        n_edges = int(new["edge_index"].shape[1])
        counts.append(n_edges)
        assert int(ff.n_edges) == n_edges
        ei, shift = _list_of(ff)
        assert torch.equal(ei, new["edge_index"].cpu()) and torch.equal(shift, new["edge_cell_shift"].cpu())
        assert not ff.static["edge_cell_shift"][n_edges:].any()      # ghost edges: zero shift
        errs = [rel_err(energy, out[E_KEY].reshape(-1)), rel_err(forces, out["forces"])]
        e_ref, f_ref = field(pos)
        assert field.edge_counts[-1] == n_edges
        errs += [rel_err(energy, e_ref), rel_err(forces, f_ref)]
        print("pbc", step, n_edges, errs)
        assert errs[0] < REPLAY and errs[1] < REPLAY, (step, errs)
        assert errs[2] < TOL and errs[3] < FTOL, (step, errs)
    assert len(set(counts)) >= 3, counts                      # the moves changed the edge set


def test_lattice_translations_change_the_image_numbers_and_nothing_else(dev):
    """Positions and cell entries that are multiples of 2^-8 (every operation of the rule is exact); a third of the atoms moved by
    integer lattice vectors: the (src, dst) list is unchanged, the shifts differ by exactly those integers, edge_vector is
    bit-equal, energy and forces within REPLAY."""
    from e3_layers_amd.data import computeEdgeIndex, computeEdgeVector

    prod = _build(_small_tree(), dev)
    q = 256.0
    cells = torch.round(CELLS * q) / q
    batch = _periodic_batch(cells=cells)
    batch["pos"] = torch.round(batch["pos"].double() * q).float() / q
    seg = batch["_node_segment"]
    gen = torch.Generator().manual_seed(5)
    k = torch.randint(-2, 3, (batch["pos"].shape[0], 3), generator=gen)
    k[torch.arange(k.shape[0]) % 3 != 0] = 0
    k[seg == 2, 2] = 0      # (the slab's third axis is not periodic: no translation along it)
    assert (k != 0).any(1).sum() >= 10
    moved = batch.clone()
    moved["pos"] = (batch["pos"].double() + torch.einsum("nk,nkc->nc", k.double(), cells[seg])).float()
    assert torch.equal(moved["pos"].double(), batch["pos"].double() + torch.einsum("nk,nkc->nc", k.double(), cells[seg]))      # exact
    res = []
    for b in (batch, moved):
        d = b.clone().to(dev)
        new, attrs = computeEdgeIndex(d.data, d.attrs, r_max=R_MAX)
        d.attrs.update(attrs)
        d.update(new)
        computeEdgeVector(d.data, d.attrs)
        ff = _ff(prod, b, dev)
        energy, forces = ff(b["pos"].to(dev))
        ff.check()
        ei, shift = _list_of(ff)
        assert torch.equal(ei, new["edge_index"].cpu()) and torch.equal(shift, new["edge_cell_shift"].cpu())
        res.append((new["edge_index"].cpu(), new["edge_cell_shift"].cpu(), d["edge_vector"].cpu(), energy.clone(), forces.clone()))
    (ei0, s0, v0, e0, f0), (ei1, s1, v1, e1, f1) = res
    assert torch.equal(ei0, ei1)
    assert torch.equal(s1 - s0, (k[ei0[0]] - k[ei0[1]]).to(torch.int32)) and (s1 != s0).any()
    assert torch.equal(v0.view(torch.int32), v1.view(torch.int32))
    assert rel_err(e1, e0) < REPLAY and rel_err(f1, f0) < REPLAY


def test_a_cell_that_is_too_narrow_is_refused_before_anything_is_captured(dev):
    from e3_layers_amd.run.md import ReplayedForceField

    prod = _build(_small_tree(), dev)
    narrow = CELLS.clone()
    narrow[0, 1, 1] = 8.004      # 2 r_max (1 + 1e-3) = 8.008
    with pytest.raises(ValueError, match=r"graph 0, axis b.*8\.004.*8\.008"):
        _ff(prod, _periodic_batch(cells=narrow), dev)
    ff = _ff(prod, _periodic_batch(), dev)
    captured = ff.captured
    ff.cell[0, 0, 0] = 8.0      # (what grow() checks is what the builder uses)
    with pytest.raises(ValueError, match=r"graph 0, axis a"):
        ff.grow()
    assert ff.captured is captured      # nothing was captured again


def test_a_vacuum_cell_gives_the_open_boundary_results(dev):
    """Cell widths above the molecule's extent plus r_max: no image is ever inside the cutoff -- the edge list, the energy and the
    forces of the same batch with open boundaries."""
    from e3_layers_amd.data.synthetic import synth_qm9

    prod = _build(_small_tree(), dev)
    open_batch = synth_qm9(7, 3)
    extent = float((open_batch["pos"].max(0).values - open_batch["pos"].min(0).values).max())
    cells = (torch.eye(3, dtype=torch.float64) * (extent + R_MAX + 2.0)).expand(3, 3, 3).clone()
    assert float(cells[0, 0, 0]) > extent + R_MAX
    vac = _periodic_batch(cells=cells, pbc=torch.ones(3, 3, dtype=torch.int64), centre=torch.zeros(3, 3, dtype=torch.float64), wrap=False)
    assert torch.equal(vac["pos"], open_batch["pos"])
    ff_open, ff_vac = _ff(prod, open_batch, dev), _ff(prod, vac, dev)
    gen = torch.Generator().manual_seed(3)
    for scale in (0.0, 0.3):
        pos = (open_batch["pos"] + scale * torch.randn(open_batch["pos"].shape, generator=gen)).to(dev)
        e0, f0 = ff_open(pos)
        ff_open.check()
        e1, f1 = ff_vac(pos)
        ff_vac.check()
        n = int(ff_open.n_edges)
        assert int(ff_vac.n_edges) == n
        assert torch.equal(ff_vac.static["edge_index"][:, :n], ff_open.static["edge_index"][:, :n])
        assert not ff_vac.static["edge_cell_shift"].any()
        assert rel_err(e1, e0) < REPLAY and rel_err(f1, f0) < REPLAY


def test_an_outgrown_periodic_list_is_regrown_and_the_chunk_redone(dev):
    """Thirty velocity-Verlet steps towards the (minimum-image) centroids with a tight first bucket: one regrowth at least, and the
    trajectory of the amply sized run within REPLAY."""
    prod = _build(_small_tree(), dev)
    batch = _periodic_batch()
    x0, seg = batch["pos"].clone(), batch["_node_segment"]
    open_pos = _periodic_batch(wrap=False)["pos"]      # the same molecules unwrapped: their centroids, atom by atom the same image
    cen = torch.zeros(len(batch), 3).index_add_(0, seg, open_pos) / batch["_n_nodes"].float()
    v0 = -0.4 * (open_pos - cen[seg])
    mass = torch.ones(x0.shape[0])
    runs = {}
    for name, kw in (("tight", dict(edge_slack=1.0, edge_multiple=32)), ("ample", dict(edge_slack=2.5))):
        ff = _ff(prod, batch, dev, **kw)
        first_cap = ff.e_cap
        md, e_tot = _device_verlet(ff, x0, v0, mass, 0.02, 30, check_every=5)
        runs[name] = (md, e_tot, first_cap, ff)
    tight, ample = runs["tight"], runs["ample"]
    assert ample[0].regrowths == 0
    assert tight[0].regrowths >= 1 and tight[0].restores >= 1 and tight[3].e_cap > tight[2]
    assert int(tight[3].n_edges) > tight[2]                    # the final list would not have fitted the first bucket
    assert tight[3].static["edge_cell_shift"][:int(tight[3].n_edges)].any()
    assert rel_err(tight[0].x, ample[0].x) < REPLAY and rel_err(tight[0].v, ample[0].v) < REPLAY
    assert rel_err(tight[1], ample[1]) < REPLAY
    assert torch.isfinite(tight[1]).all()


def test_energy_is_conserved_to_second_order_across_cell_faces(dev):
    """As test_energy_is_conserved_to_second_order_across_list_changes of tests/test_gpu_md.py, with its band: dt and the length are
    such that the float64 loop on the periodic list is in the second-order regime (drift(dt) / drift(dt / 2) in [3.5, 4.5], measured
    here first), the float32 loop's drift at dt is >= 10 x its drift at dt / 8; the device must at least halve the drift.  Atoms
    cross cell faces on the way (the cell index of some atom changes) and the image numbers of the list change."""
    tree, dt, n_steps = _small_tree(), 0.16, 8
    prod = _build(tree, dev)
    batch = _periodic_batch()
    x0 = batch["pos"].clone()
    v0 = (0.5 * torch.randn(x0.shape, generator=torch.Generator().manual_seed(1), dtype=torch.float64)).float()
    mass = torch.ones(x0.shape[0])

    def drift(e):
        return float((e - e[0]).abs().max())

    f64 = _PeriodicOracleField(_oracle(prod, tree), batch)
    x_end, _, e_dt = _oracle_verlet(f64, x0, v0, mass, dt, n_steps)
    first, last = f64.shifts[0], f64.shifts[-1]
    assert len(set(f64.edge_counts)) >= 2, f64.edge_counts
    assert first.shape != last.shape or not torch.equal(first, last)      # the image numbers of the list changed
    seg = batch["_node_segment"]
    inv = torch.linalg.inv(CELLS)[seg]
    image = lambda x: torch.floor(torch.einsum("nc,nck->nk", x.double(), inv))
    crossed = (image(x_end) != image(x0)) & (PBC[seg] != 0)
    assert crossed.any(), "no atom crossed a cell face"
    d64 = [drift(e_dt), drift(_oracle_verlet(f64, x0, v0, mass, dt / 2, n_steps * 2)[2])]
    assert 3.5 <= d64[0] / d64[1] <= 4.5, d64
    f32 = _PeriodicOracleField(_oracle(prod, tree, torch.float32), batch, torch.float32)
    d32 = [drift(_oracle_verlet(f32, x0, v0, mass, dt / k, n_steps * k)[2]) for k in (1, 8)]
    assert d32[0] >= 10 * d32[1], d32
    ff = _ff(prod, batch, dev)
    d_dev = [drift(_device_verlet(ff, x0, v0, mass, dt / k, n_steps * k, check_every=8)[1]) for k in (1, 2)]
    print("pbc_energy_drift", dict(device=d_dev, float64=d64, float32=d32, crossed=int(crossed.any(1).sum())))
    assert d_dev[1] < 0.5 * d_dev[0], d_dev
