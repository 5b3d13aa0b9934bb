"""Virial and stress of the force models on the device: ``GradientOutput(virial=, stress=)`` through ``enable_virial`` on the eager
model, and ``run/md.ReplayedForceField(virial_key=, stress_key=)`` with ``set_cell`` -- against the float64 oracle's
``sum_e v_e (x) dE/dv_e`` on the periodic list (tests/test_virial_host.oracle_strain_gradient), against each other, and with the keys
off.  The small tree, the periodic batch, its three cells (orthorhombic, triclinic, slab) and the tolerances are those of
tests/test_gpu_pbc_force_field.py and tests/test_gpu_md.py.

Definitions (row-vector convention, ``cell``'s): ``virial = -dE/d eps = -sum_e v_e (x) dE/dv_e``; ``stress = -virial / |det cell|``.

Tolerance against the oracle: FTOL, the project's force tolerance (normwise) -- the virial is a linear form of the same per-edge
gradients the forces are, with weights |v| < r_max.  The error relative to the majorant ``sum |v| (x) |dE/dv|`` is recorded beside it.
Two models of the same seed carry the same weights: one with the keys on, one with them off."""
import pytest
import torch

from tests.test_gpu_md import FTOL, REPLAY, _build, _oracle, _small_tree
from tests.test_gpu_pbc_force_field import CELLS, E_KEY, R_MAX, _eager, _ff, _host_list, _list_of, _periodic_batch
from tests.test_virial_host import oracle_strain_gradient
from tests.util import record_measured, rel_err, zero_shifts

pytestmark = pytest.mark.gpu

KEYS = dict(virial_key="virial", stress_key="stress")
VOLUME = torch.linalg.det(CELLS).abs()
SCALES = (0.0, 0.25, 0.4, 0.15)      # the four displaced position sets of the periodic test (seed 11)


def _models(dev, stress="stress"):
    """(keys on, keys off): the same weights"""
    from e3_layers_amd.nn import enable_virial

    tree = _small_tree()
    on, off = enable_virial(_build(tree, dev), "virial", stress), _build(tree, dev)
    assert all(torch.equal(a, b) for a, b in zip(on.state_dict().values(), off.state_dict().values()))
    return tree, on, off


def _positions(batch):
    gen = torch.Generator().manual_seed(11)
    return [batch["pos"] + scale * torch.randn(batch["pos"].shape, generator=gen) for scale in SCALES]


def _oracle_virial(orc, batch, pos):
    """float64 (virial [G, 9], stress [G, 9], majorant [G, 9], edge count) of the oracle on the periodic list at ``pos``"""
    ei, shift, _ = _host_list(batch, pos)
    _, sg, maj, _, _ = oracle_strain_gradient(orc.func, batch, pos.float(), ei, shift, CELLS)
    return (-sg).reshape(-1, 9), (sg / VOLUME[:, None, None]).reshape(-1, 9), maj.reshape(-1, 9), int(ei.shape[1])


def _over_majorant(got, want, maj):
    return float(((got.detach().double().cpu() - want).abs() / maj).max())


def test_eager_virial_and_stress_equal_the_oracle_and_leave_energy_and_forces_alone(dev):
    tree, on, off = _models(dev)
    orc = _oracle(on, tree)
    zero_shifts(on, off, orc)
    batch = _periodic_batch()
    worst = [0.0, 0.0, 0.0]
    for step, pos in enumerate(_positions(batch)):
        out, new = _eager(on, batch, pos, dev)
        plain, _ = _eager(off, batch, pos, dev)
        assert "virial" not in plain and "stress" not in plain
        assert out["virial"].shape == (3, 9) and out["virial"].dtype == torch.float32 and out.attrs["virial"] == ("graph", "3x1o")
        assert out["stress"].shape == (3, 9) and out.attrs["stress"] == ("graph", "3x1o")
        w_ref, s_ref, maj, n_edges = _oracle_virial(orc, batch, pos)
        assert n_edges == int(new["edge_index"].shape[1])
        errs = [rel_err(out["virial"], w_ref), rel_err(out["stress"], s_ref), _over_majorant(out["virial"], w_ref, maj)]
        print("eager virial", step, n_edges, errs)
        worst = [max(a, b) for a, b in zip(worst, errs)]
        assert errs[0] < FTOL and errs[1] < FTOL, (step, errs)
        assert torch.equal(out[E_KEY], plain[E_KEY]) and torch.equal(out["forces"], plain["forces"]), step
        assert torch.allclose(out["stress"].double().cpu(), -out["virial"].double().cpu() / VOLUME[:, None], rtol=1e-6, atol=0)
    record_measured("stress_eager_vs_oracle", virial=worst[0], stress=worst[1], virial_over_majorant=worst[2])


def test_replayed_virial_and_stress_equal_eager_and_leave_energy_and_forces_alone(dev):
    tree, on, off = _models(dev)
    batch = _periodic_batch()
    ff, ff_off = _ff(on, batch, dev, **KEYS), _ff(off, batch, dev)
    assert ff_off.virial is None and ff_off.stress is None
    assert ff.volume.dtype == torch.float64 and torch.allclose(ff.volume.cpu(), VOLUME, rtol=1e-14, atol=0)
    counts, worst = [], [0.0, 0.0]
    for step, pos in enumerate(_positions(batch)):
        energy, forces = ff(pos.to(dev))
        ff.check()
        assert ff.valid and ff.virial.shape == (3, 3, 3) and ff.stress.shape == (3, 3, 3)
        e0, f0 = ff_off(pos.to(dev))
        ff_off.check()
        out, new = _eager(on, batch, pos, dev)
        counts.append(int(new["edge_index"].shape[1]))
        assert int(ff.n_edges) == counts[-1]
        errs = [rel_err(ff.virial.reshape(-1, 9), out["virial"]), rel_err(ff.stress.reshape(-1, 9), out["stress"])]
        print("replayed virial", step, counts[-1], errs)
        worst = [max(a, b) for a, b in zip(worst, errs)]
        assert errs[0] < REPLAY and errs[1] < REPLAY, (step, errs)
        assert torch.equal(energy, e0) and torch.equal(forces, f0), step
    assert len(set(counts)) >= 3, counts                      # the moves changed the edge set
    record_measured("stress_replay_vs_eager", virial=worst[0], stress=worst[1])


def test_open_batch_virial_is_position_times_force_and_a_vacuum_cell_agrees(dev):
    from e3_layers_amd.data.synthetic import synth_qm9
    from e3_layers_amd.nn import enable_virial
    from e3_layers_amd.run.md import ReplayedForceField

    tree, on, _ = _models(dev)
    open_model = enable_virial(_build(tree, dev), "virial", None)
    open_batch = synth_qm9(7, 3)
    ff_open = ReplayedForceField(open_model, open_batch.clone().to(dev), R_MAX, energy_key=E_KEY, forces_key="forces", **KEYS)
    assert ff_open.stress is None and ff_open.volume is None and ff_open.cell is None
    with pytest.raises(ValueError, match="open batch"):
        ff_open.set_cell(CELLS)
    extent = float((open_batch["pos"].max(0).values - open_batch["pos"].min(0).values).max())
    cells = (torch.eye(3, dtype=torch.float64) * (extent + R_MAX + 2.0)).expand(3, 3, 3).clone()
    vac = _periodic_batch(cells=cells, pbc=torch.ones(3, 3, dtype=torch.int64), centre=torch.zeros(3, 3, dtype=torch.float64), wrap=False)
    ff_vac = _ff(on, vac, dev, **KEYS)
    seg = open_batch["_node_segment"]
    gen = torch.Generator().manual_seed(3)
    for scale in (0.0, 0.3):
        pos = open_batch["pos"] + scale * torch.randn(open_batch["pos"].shape, generator=gen)
        _, forces = ff_open(pos.to(dev))
        ff_open.check()
        x, f = pos.double(), forces.double().cpu()
        cen = torch.zeros(3, 3, dtype=torch.float64).index_add_(0, seg, x) / open_batch["_n_nodes"].reshape(-1, 1).double()
        xf = torch.zeros(3, 3, 3, dtype=torch.float64).index_add_(0, seg, (x - cen[seg])[:, :, None] * f[:, None, :])
        err = rel_err(ff_open.virial, xf)
        ff_vac(pos.to(dev))
        ff_vac.check()
        both = rel_err(ff_vac.virial, ff_open.virial)
        print("open virial", scale, err, both)
        assert err < FTOL, err
        assert both < REPLAY, both
        assert torch.isfinite(ff_vac.stress).all() and ff_vac.stress.abs().max() > 0
    record_measured("stress_open_cluster", virial_vs_x_times_f=err, vacuum_vs_open=both)


def test_the_antisymmetric_part_is_rounding_noise(dev):
    tree, on, _ = _models(dev)
    orc = _oracle(on, tree)
    batch = _periodic_batch()
    pos = _positions(batch)[1]
    w_ref = _oracle_virial(orc, batch, pos)[0].reshape(-1, 3, 3)
    ratio64 = (w_ref - w_ref.transpose(1, 2)).flatten(1).norm(dim=1) / w_ref.flatten(1).norm(dim=1)
    assert float(ratio64.max()) < 1e-10, ratio64
    out, _ = _eager(on, batch, pos, dev)
    w = out["virial"].double().cpu().reshape(-1, 3, 3)
    ratio = (w - w.transpose(1, 2)).flatten(1).norm(dim=1) / w.flatten(1).norm(dim=1)
    print("antisymmetric part", ratio.tolist(), ratio64.tolist())
    assert float(ratio.max()) < FTOL, ratio
    record_measured("stress_antisymmetric_part", device=float(ratio.max()), float64=float(ratio64.max()))


def _strained(batch):
    """(cells, positions) under a strain of 1 %: a symmetric part and a shear, the slab's third axis included"""
    eps = torch.tensor([[0.010, 0.004, 0.003], [0.004, -0.006, 0.005], [0.003, 0.005, 0.008]], dtype=torch.float64)
    eps[0, 2] += 0.004      # (a shear: not symmetric)
    f = torch.eye(3, dtype=torch.float64) + eps
    return CELLS @ f, (batch["pos"].double() @ f).float()


def test_set_cell_changes_the_cell_of_the_captured_graph(dev):
    tree, on, _ = _models(dev)
    batch = _periodic_batch()
    ff = _ff(on, batch, dev, **KEYS)
    ff(batch["pos"].to(dev))
    ff.check()
    captured, recaptures, first = ff.captured, ff.recaptures, ff.virial.clone()
    new_cells, new_pos = _strained(batch)
    ff.set_cell(new_cells.to(dev).reshape(3, 9))      # a device [G, 9] tensor
    assert not ff.valid and torch.equal(ff.cell.cpu(), new_cells.float())
    assert torch.allclose(ff.volume.cpu(), torch.linalg.det(new_cells.float().double()).abs(), rtol=1e-14, atol=0)
    assert not ff.static["cell"][-1].any() and not ff.static["_inv_cell"][-1].any()      # the ghost graph's rows stay zero
    energy, forces = ff(new_pos.to(dev))
    ff.check()
    strained = _periodic_batch(cells=new_cells, wrap=False)
    strained["pos"] = new_pos.clone()
    fresh = _ff(on, strained, dev, **KEYS)
    e1, f1 = fresh(new_pos.to(dev))
    fresh.check()
    assert all(torch.equal(a, b) for a, b in zip(_list_of(ff), _list_of(fresh)))
    assert _list_of(ff)[1].any()
    errs = [rel_err(energy, e1), rel_err(forces, f1), rel_err(ff.virial, fresh.virial), rel_err(ff.stress, fresh.stress)]
    print("set_cell", errs, rel_err(ff.virial, first))
    assert max(errs) < REPLAY, errs
    assert rel_err(ff.virial, first) > 1e-3      # (the strain changed it)
    assert ff.captured is captured and ff.recaptures == recaptures      # nothing was captured again
    # a cell that is too narrow: refused on the host before anything changes
    before = (ff.cell.clone(), ff.static["cell"].clone(), ff.static["_inv_cell"].clone(), ff.volume.clone())
    narrow = new_cells.clone()
    narrow[0, 1] = torch.tensor([0.0, 8.004, 0.0])      # 2 r_max (1 + 1e-3) = 8.008
    with pytest.raises(ValueError, match=r"graph 0, axis b"):
        ff.set_cell(narrow)
    with pytest.raises(ValueError, match=r"\[3, 3, 3\]"):
        ff.set_cell(new_cells[:2])
    after = (ff.cell, ff.static["cell"], ff.static["_inv_cell"], ff.volume)
    assert all(torch.equal(a, b) for a, b in zip(before, after))
    record_measured("stress_set_cell_vs_fresh", energy=errs[0], forces=errs[1], virial=errs[2], stress=errs[3])


def test_the_virial_survives_a_regrowth(dev):
    tree, on, _ = _models(dev)
    batch = _periodic_batch()
    ff = _ff(on, batch, dev, **KEYS)
    pos = _positions(batch)[2]
    ff(pos.to(dev))
    ff.check()
    cap = ff.e_cap
    ff.grow()
    assert ff.e_cap > cap
    ff(pos.to(dev))
    ff.check()
    out, _ = _eager(on, batch, pos, dev)
    errs = [rel_err(ff.virial.reshape(-1, 9), out["virial"]), rel_err(ff.stress.reshape(-1, 9), out["stress"])]
    print("after grow()", errs)
    assert max(errs) < REPLAY, errs


def test_refusals(dev):
    from e3_layers_amd.data import computeEdgeIndex
    from e3_layers_amd.run.md import ReplayedForceField

    tree, on, off = _models(dev)
    batch = _periodic_batch()
    on.train()
    with pytest.raises(NotImplementedError, match="training"):
        _eager(on, batch, batch["pos"], dev)
    on.eval()
    b = batch.clone().to(dev)
    new, attrs = computeEdgeIndex(b.data, b.attrs, r_max=R_MAX)
    b.attrs.update(attrs)
    b.update(new)
    b["edge_vector"] = (b["pos"][b["edge_index"][1]] - b["pos"][b["edge_index"][0]]).requires_grad_(True)
    with pytest.raises(NotImplementedError, match="edge_vector"):
        on(b)
    with pytest.raises(KeyError, match="enable_virial"):      # before anything is captured: the model is never called
        ReplayedForceField(off, batch.clone().to(dev), R_MAX, energy_key=E_KEY, virial_key="virial")
    with pytest.raises(KeyError, match="enable_virial"):
        ReplayedForceField(on, batch.clone().to(dev), R_MAX, energy_key=E_KEY, virial_key="virial", stress_key="pressure_tensor")
