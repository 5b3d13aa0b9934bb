"""Crystal unit cells in the replayed force field and MD: ``run/md.ReplayedForceField(..., images="all")`` on the device -- against the
float64 oracle on the same all-images list, against the 3 x 3 x 3 supercell with the minimum-image list, against the eager path,
through ``set_cell`` across a change of the image ranges, across an overflow, in five velocity-Verlet steps, and on a wide cell against
``images="minimum"``.  The small tree, ``r_max`` = 4 and the tolerances are those of tests/test_gpu_md.py, tests/test_gpu_pbc_force_field.py
and tests/test_gpu_stress_force_field.py (TOL energy, FTOL forces, virial and stress, REPLAY replay against eager).

The batch: two synthetic crystals of 8 atoms.  Cell 0 is triclinic with image ranges (1, 1, 1), cell 1 orthorhombic with (2, 1, 0):
along its first axis (2.375 A wide) an atom's neighbours are its own images.  Atoms sit on a jittered grid, so that no two atoms, images
included, are closer than 1.5 A (asserted in tests/test_images_host.py, which also checks the premises of this file without a GPU).
The oracle knows no cell: as in tests/test_gpu_pbc_force_field.py it is given the list and a float64 ``edge_vector`` with the shifts in it.

Bit for bit: the list, the image numbers, the energy and the forces.  Virial and stress are held to REPLAY where two runs are compared:
two replays of ONE minimum-image force field at the same moved positions already differ in them by up to 5 (virial) and 8 (stress)
fp32 words with energy and forces bit-equal (measured on the parent's own path while this file was written, three force fields on
the wide-cell batch below), so exact equality of those two outputs is not a property the all-images path can be held to.
"""
import pytest
import torch

from tests.test_gpu_md import FTOL, REPLAY, TOL, _build, _oracle, _small_tree
from tests.test_virial_host import oracle_strain_gradient
from tests.util import record_measured, rel_err, zero_shifts

pytestmark = pytest.mark.gpu

R_MAX = 4.0
E_KEY = "energy_total"
KEYS = dict(virial_key="virial", stress_key="stress")
# (every entry a multiple of 2^-8, and so is every position of crystal_batch: a supercell's positions, pos + copy @ cell, are exact in fp32)
CELLS = torch.tensor([[[5.25, 0.0, 0.0], [0.625, 5.0, 0.0], [-0.375, 0.5, 5.375]],
                      [[2.375, 0.0, 0.0], [0.0, 5.0, 0.0], [0.0, 0.0, 9.0]]], dtype=torch.float64)
RANGES = [[1, 1, 1], [2, 1, 0]]
STRAINED_RANGES = [[1, 1, 1], [3, 1, 0]]      # of strained_cells()
GRIDS = [(2, 2, 2), (1, 2, 4)]
ATTRS = {"pos": ("node", "1x1o"), "species": ("node", "1x0e"), "cell": ("graph", "3x1o"), "pbc": ("graph", "3x0e")}


def crystal_batch(cells=CELLS, reps=(1, 1, 1), jitter=0.04, graphs=(0, 1)):
    """A host batch without a list: per graph the 8 atoms of its grid (fractional, jittered by ``jitter``), repeated ``reps`` times along
    the axes with the cell scaled to match (the supercell: atom a of copy c is node c * 8 + a)."""
    from e3_layers_amd.data.data import Batch, Data
    from e3_layers_amd.data.synthetic import synth_qm9

    kinds = synth_qm9(7, 3)["species"].reshape(-1)
    samples = []
    for g in graphs:
        gen = torch.Generator().manual_seed(100 + g)
        grid = torch.cartesian_prod(*(torch.arange(n, dtype=torch.float64) for n in GRIDS[g])).reshape(-1, 3)
        frac = (grid + 0.5) / torch.tensor(GRIDS[g], dtype=torch.float64) + jitter * (2 * torch.rand(grid.shape, generator=gen, dtype=torch.float64) - 1)
        species = kinds[torch.randint(0, kinds.numel(), (grid.shape[0],), generator=gen)]
        copies = torch.cartesian_prod(*(torch.arange(r, dtype=torch.float64) for r in reps)).reshape(-1, 3)
        one = torch.round(frac @ cells[g] * 256.0) / 256.0
        pos = (one[None] + (copies @ cells[g])[:, None]).reshape(-1, 3).float()
        cell = (cells[g] * torch.tensor(reps, dtype=torch.float64)[:, None]).float()
        samples.append(Data(attrs=dict(ATTRS), pos=pos, species=species.repeat(copies.shape[0]).reshape(-1, 1), cell=cell.reshape(1, 9),
                            pbc=torch.ones(1, 3, dtype=torch.int64)))
    return Batch.from_data_list(samples, attrs=dict(ATTRS))


def host_list(batch, pos, images="all"):
    """(edge_index, shift, n_edges) of the project's CPU path at ``pos``"""
    from e3_layers_amd.data import computeEdgeIndex

    b = batch.clone()
    b["pos"] = pos.detach().float().cpu()
    for k in ("edge_index", "_n_edges", "_edge_segment", "edge_cell_shift", "_image_range"):
        b.pop(k)
    new, _ = computeEdgeIndex(b.data, b.attrs, r_max=R_MAX, images=images)
    return new["edge_index"], new["edge_cell_shift"], b["_n_edges"]


def oracle_outputs(net, batch, pos, images="all"):
    """float64, of the energy network ``net`` (the oracle's ``func``) on the project's list at ``pos``: energy [G], forces [N, 3],
    virial [G, 9], stress [G, 9], the number of edges"""
    ei, shift, _ = host_list(batch, pos, images)
    cell = batch["cell"].reshape(-1, 3, 3).double()
    energy, sg, _, g, _ = oracle_strain_gradient(net, batch, pos.float(), ei, shift, cell)
    forces = torch.zeros(pos.shape[0], 3, dtype=torch.float64).index_add_(0, ei[0], g).index_add_(0, ei[1], -g)
    volume = torch.linalg.det(cell).abs()
    return energy, forces, (-sg).reshape(-1, 9), (sg / volume[:, None, None]).reshape(-1, 9), int(ei.shape[1])


def _models(dev):
    from e3_layers_amd.nn import enable_virial

    tree = _small_tree()
    return tree, enable_virial(_build(tree, dev), "virial", "stress")


def _ff(prod, batch, dev, images="all", **kw):
    from e3_layers_amd.run.md import ReplayedForceField

    return ReplayedForceField(prod, batch.clone().to(dev), R_MAX, energy_key=E_KEY, forces_key="forces", images=images, **KEYS, **kw)


def _eager(prod, batch, pos, dev, images="all"):
    from e3_layers_amd.data import computeEdgeIndex

    b = batch.clone().to(dev)
    b["pos"] = pos.to(dev, torch.float32)
    new, attrs = computeEdgeIndex(b.data, b.attrs, r_max=R_MAX, images=images)
    b.attrs.update(attrs)
    b.update(new)
    return prod(b), new


class _EagerStep:
    """The step a ``ReplayedForceField`` captured, issued eagerly on the same padded batch: the capped builder, then the model --
    what the integrators need of a force field (``pos``, ``node_ptr``, ``evaluate()``, ``check()``)."""

    def __init__(self, ff):
        self.ff, self.pos, self.node_ptr = ff, ff.pos, ff.node_ptr

    def evaluate(self):
        from e3_layers_amd.data import computeEdgeIndexCapped

        ff = self.ff
        work = ff._bucket.view()
        computeEdgeIndexCapped(work.data, work.attrs, r_max=ff.r_max, key=ff.key)
        out = self.out = ff.model(work)
        return out[E_KEY].reshape(-1)[:ff.n_graphs], out["forces"][:ff.n_real]

    def extras(self):
        return tuple(self.out[k].reshape(-1, 9)[:self.ff.n_graphs] for k in ("virial", "stress"))

    def check(self):
        self.ff.check()


def _list_of(ff):
    e = int(ff.n_edges)
    return ff.static["edge_index"][:, :e].cpu(), ff.static["edge_cell_shift"][:e].cpu()


def _positions(batch):
    gen = torch.Generator().manual_seed(11)
    return [batch["pos"] + scale * torch.randn(batch["pos"].shape, generator=gen) for scale in (0.0, 0.15, 0.3)]


def test_all_images_force_field_equals_eager_and_the_oracle(dev):
    """Energy, forces, virial and stress of the replayed force field on two narrow cells, at moved positions (the edge count changes):
    == the eager all-images list + the model (the list exactly, the outputs within REPLAY), and within TOL / FTOL of the float64
    oracle on the same list."""
    tree, prod = _models(dev)
    orc = _oracle(prod, tree)
    zero_shifts(prod, orc)
    batch = crystal_batch()
    ff = _ff(prod, batch, dev)
    assert ff.image_range.dtype == torch.int32 and ff.image_range.cpu().tolist() == RANGES
    assert not ff.static["_image_range"][-1].any()      # the ghost graph's row
    eager_step = _EagerStep(ff)
    counts, worst = [], [0.0] * 8
    for step, pos in enumerate(_positions(batch)):
        energy, forces = ff(pos.to(dev))
        ff.check()
        out, new = _eager(prod, batch, pos, dev)
        n_edges = int(new["edge_index"].shape[1])
        counts.append(n_edges)
        assert int(ff.n_edges) == n_edges
        ei, shift = _list_of(ff)
        assert torch.equal(ei, new["edge_index"].cpu()) and torch.equal(shift, new["edge_cell_shift"].cpu())
        assert (ei[0] == ei[1]).any() and shift[ei[0] == ei[1]].any(1).all()      # an atom's own images, never the atom itself
        assert not ff.static["edge_cell_shift"][n_edges:].any()      # ghost edges: zero shift
        # replay == the same step issued eagerly, exactly
        step_e, step_f = eager_step.evaluate()
        ff.check()
        assert torch.equal(step_e, energy) and torch.equal(step_f, forces)
        assert rel_err(eager_step.extras()[0], ff.virial.reshape(-1, 9)) < REPLAY and rel_err(eager_step.extras()[1], ff.stress.reshape(-1, 9)) < REPLAY
        e_ref, f_ref, w_ref, s_ref, n_ref = oracle_outputs(orc.func, batch, pos)
        assert n_ref == n_edges
        errs = [rel_err(energy, out[E_KEY].reshape(-1)), rel_err(forces, out["forces"]), rel_err(ff.virial.reshape(-1, 9), out["virial"]),
                rel_err(ff.stress.reshape(-1, 9), out["stress"]), rel_err(energy, e_ref), rel_err(forces, f_ref),
                rel_err(ff.virial.reshape(-1, 9), w_ref), rel_err(ff.stress.reshape(-1, 9), s_ref)]
        print("images", step, n_edges, errs)
        worst = [max(a, b) for a, b in zip(worst, errs)]
        assert max(errs[:4]) < REPLAY, (step, errs)
        assert errs[4] < TOL and max(errs[5:]) < FTOL, (step, errs)
    assert len(set(counts)) >= 2, counts
    record_measured("images_replay_vs_eager", energy=worst[0], forces=worst[1], virial=worst[2], stress=worst[3])
    record_measured("images_vs_oracle", energy=worst[4], forces=worst[5], virial=worst[6], stress=worst[7])


def test_a_narrow_cell_equals_its_supercell_on_the_minimum_image_list(dev):
    """27 x the energy of the narrow cell == the energy of its 3 x 3 x 3 supercell replayed with images="minimum" (TOL: both are fp32
    runs of the same physics); the forces of every copy of an atom == the atom's (FTOL); the stress is the same (FTOL)."""
    tree, prod = _models(dev)
    for g in (0, 1):
        reps = (3, 3, 3) if g == 0 else (4, 2, 1)      # wide enough for check_cell: about 15 and 9.5, 10, 9 against 8.008
        small, big = crystal_batch(graphs=(g,)), crystal_batch(graphs=(g,), reps=reps)
        k = reps[0] * reps[1] * reps[2]
        ff, ff_big = _ff(prod, small, dev), _ff(prod, big, dev, images="minimum")
        assert ff_big.image_range is None
        e, f = ff(small["pos"].to(dev))
        ff.check()
        e_big, f_big = ff_big(big["pos"].to(dev))
        ff_big.check()
        assert int(ff_big.n_edges) == k * int(ff.n_edges)
        errs = [rel_err(e_big, k * e), rel_err(f_big, f.repeat(k, 1)), rel_err(ff_big.stress, ff.stress), rel_err(ff_big.virial, k * ff.virial)]
        print("supercell", g, int(ff.n_edges), errs)
        record_measured("images_vs_supercell", graph=g, energy=errs[0], forces=errs[1], stress=errs[2], virial=errs[3])
        assert errs[0] < TOL and max(errs[1:]) < FTOL, errs


def strained_cells():
    """(cells, deformation) compressed to 65 % along x: the second cell's first axis goes from 2.375 to 1.54 A, below
    r_max (1 + 1e-3) / 2.5 = 1.6016, so its range rises from 2 to 3 (M from 15 to 21); the first cell's ranges stay (1, 1, 1)"""
    f = torch.diag(torch.tensor([0.65, 1.0, 1.0], dtype=torch.float64))
    return CELLS @ f, f


def test_set_cell_across_a_change_of_the_ranges_equals_a_fresh_capture(dev):
    tree, prod = _models(dev)
    batch = crystal_batch()
    ff = _ff(prod, batch, dev, edge_slack=3.0)
    ff(batch["pos"].to(dev))
    ff.check()
    captured = ff.captured
    new_cells, f = strained_cells()
    new_pos = (batch["pos"].double() @ f).float()
    ff.set_cell(new_cells)
    assert not ff.valid and ff.image_range.cpu().tolist() == STRAINED_RANGES
    assert not ff.static["_image_range"][-1].any()
    energy, forces = ff(new_pos.to(dev))
    ff.check()
    assert ff.captured is captured      # nothing was captured again
    fresh_batch = crystal_batch(cells=new_cells)
    fresh_batch["pos"] = new_pos
    fresh = _ff(prod, fresh_batch, dev, edge_slack=3.0)
    e1, f1 = fresh(new_pos.to(dev))
    fresh.check()
    assert fresh.image_range.cpu().tolist() == ff.image_range.cpu().tolist()
    (ei, shift), (ei1, shift1) = _list_of(ff), _list_of(fresh)
    assert torch.equal(ei, ei1) and torch.equal(shift, shift1)
    if ff.e_cap == fresh.e_cap:      # the same padded problem: the same bits
        assert torch.equal(energy, e1) and torch.equal(forces, f1)
    errs = [rel_err(energy, e1), rel_err(forces, f1), rel_err(ff.virial, fresh.virial), rel_err(ff.stress, fresh.stress)]
    print("set_cell", int(ff.n_edges), ff.e_cap, fresh.e_cap, errs)
    assert max(errs) < REPLAY, errs
    with pytest.raises(ValueError, match=r"graph 1, axis a.*not served"):      # a range of 8: refused before anything changes
        ff.set_cell(CELLS @ torch.diag(torch.tensor([0.19, 1.0, 1.0], dtype=torch.float64)))
    assert torch.equal(ff.cell.cpu(), new_cells.float()) and ff.image_range.cpu().tolist() == STRAINED_RANGES and ff.valid


def test_an_overflow_after_set_cell_raises_at_check_and_grow_recovers(dev):
    from e3_layers_amd.backend.graph import EdgeCapacityExceeded

    tree, prod = _models(dev)
    batch = crystal_batch()
    ff = _ff(prod, batch, dev, edge_slack=1.0, edge_multiple=32)
    ff(batch["pos"].to(dev))
    ff.check()
    first_cap = ff.e_cap
    new_cells, f = strained_cells()
    new_pos = (batch["pos"].double() @ f).float().to(dev)
    ff.set_cell(new_cells)
    ff(new_pos)
    with pytest.raises(EdgeCapacityExceeded):
        ff.check()
    assert int(ff.n_edges) > first_cap
    ff.grow(pos=new_pos)
    energy, forces = ff(new_pos)
    ff.check()
    assert ff.e_cap > first_cap and ff.image_range.cpu().tolist() == STRAINED_RANGES
    fresh_batch = crystal_batch(cells=new_cells)
    fresh_batch["pos"] = new_pos.cpu()
    out, new = _eager(prod, fresh_batch, new_pos.cpu(), dev)
    ei, shift = _list_of(ff)
    assert torch.equal(ei, new["edge_index"].cpu()) and torch.equal(shift, new["edge_cell_shift"].cpu())
    assert rel_err(energy, out[E_KEY].reshape(-1)) < REPLAY and rel_err(forces, out["forces"]) < REPLAY


def test_five_replayed_verlet_steps_equal_the_eager_loop_bit_for_bit(dev):
    """VelocityVerlet on the replayed all-images force field against the same integrator on the eager step (``_EagerStep``: the
    builder and the model issued launch by launch): x, v and the energy records are the same bits."""
    from e3_layers_amd.run.md import VelocityVerlet

    tree, prod = _models(dev)
    batch = crystal_batch()
    x0 = batch["pos"].to(dev)
    v0 = (0.3 * torch.randn(x0.shape, generator=torch.Generator().manual_seed(2))).to(dev)
    mass = torch.ones(x0.shape[0])
    runs = []
    for eager in (False, True):
        ff = _ff(prod, batch, dev, edge_slack=2.0)
        field = _EagerStep(ff) if eager else ff
        md = VelocityVerlet(field, mass, 0.02)
        md.v.copy_(v0)
        out = md.run(5, check_every=5)
        assert md.regrowths == 0
        runs.append((md.x.clone(), md.v.clone(), out["potential"].clone(), out["kinetic"].clone(), int(ff.n_edges)))
    for a, b in zip(*runs):
        assert torch.equal(a, b) if torch.is_tensor(a) else a == b
    assert not torch.equal(runs[0][0], x0) and torch.isfinite(runs[0][2]).all() and (runs[0][2] != 0).all()


def test_on_a_wide_cell_all_images_equals_minimum_image_bit_for_bit(dev):
    from tests.test_gpu_pbc_force_field import _periodic_batch

    tree, prod = _models(dev)
    batch = _periodic_batch()
    a, b = _ff(prod, batch, dev, images="all"), _ff(prod, batch, dev, images="minimum")
    assert not a.image_range.any() and a.e_cap == b.e_cap
    gen = torch.Generator().manual_seed(11)
    for scale in (0.0, 0.25):
        pos = (batch["pos"] + scale * torch.randn(batch["pos"].shape, generator=gen)).to(dev)
        ea, fa = a(pos)
        a.check()
        eb, fb = b(pos)
        b.check()
        assert int(a.n_edges) == int(b.n_edges)
        assert torch.equal(a.static["edge_index"], b.static["edge_index"]) and torch.equal(a.static["edge_cell_shift"], b.static["edge_cell_shift"])
        assert torch.equal(ea, eb) and torch.equal(fa, fb)
        assert rel_err(a.virial, b.virial) < REPLAY and rel_err(a.stress, b.stress) < REPLAY      # (not bit-reproducible run to run: the docstring)
