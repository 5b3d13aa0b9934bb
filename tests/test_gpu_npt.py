"""Constant-pressure MD on the device (``run/md.Barostat`` on ``Langevin`` / ``VelocityVerlet``) on the real small tree: the periodic
batch of tests/test_gpu_pbc_force_field.py with all three axes periodic, three molecules, 8 to 10 steps per test.  The models, the
force fields, the cells and the tolerances are those of the stress and periodic tests.

The coupling is chosen from the MEASURED pressure of the start (``_coupling``): p0 lies one spread of the graphs' pressures outside
them, on the side asked for, and ``a = compressibility dt / tau`` makes the nearest graph move by ``RATE`` in ln V per step --
0.5 % in length per step, so that over a run every cell moves by more than 1e-3 and the edge count changes (both asserted).

The one-step pressure lag (the barostat of step k uses the virial at x_k and the kinetic energy the previous kick filed) is the
device loop's and the host-driven loop's alike: the comparison is of the SAME algorithm, driven from two sides."""
import pytest
import torch

from tests.test_gpu_md import REPLAY
from tests.test_gpu_pbc_force_field import CELLS, R_MAX, _ff, _list_of, _periodic_batch
from tests.test_gpu_stress_force_field import KEYS, _models
from tests.util import record_measured, rel_err

pytestmark = pytest.mark.gpu

ALL_PERIODIC = torch.ones(3, 3, dtype=torch.int64)
DT, KT, GAMMA, SEED, TAU = 0.02, 0.5, 0.5, (31 << 32) + 5, 1.0
RATE = 0.015      # |d ln V| per step of the graph nearest to p0


def _batch():
    return _periodic_batch(pbc=ALL_PERIODIC)


def _start(dev, model, **kw):
    """(force field, unit masses, thermal velocities): the same start for every run of a test"""
    batch = _batch()
    ff = _ff(model, batch, dev, **KEYS, **kw)
    n = batch["pos"].shape[0]
    v0 = (KT ** 0.5) * torch.randn(n, 3, generator=torch.Generator().manual_seed(2), dtype=torch.float64).float()
    return ff, torch.ones(n), v0.to(dev)


def _initial_pressure(dev, model):
    from e3_layers_amd.run.md import pressure

    ff, mass, v0 = _start(dev, model)
    ff(ff.pos.clone())
    ff.check()
    seg = _batch()["_node_segment"].to(dev)
    kinetic = torch.zeros(3, dtype=torch.float64, device=dev).index_add_(0, seg, 0.5 * (v0.double() ** 2).sum(1))
    return pressure(ff.virial, kinetic, ff.volume).cpu()


def _coupling(p_start, side: str, rate: float = RATE):
    """(p0, compressibility): p0 one spread below (``"expand"``) or above (``"compress"``) every graph's starting pressure"""
    spread = float(p_start.abs().max())
    p0 = float(p_start.min()) - spread if side == "expand" else float(p_start.max()) + spread
    return p0, rate / spread * TAU / DT


def _relative_move(cell, first=CELLS):
    c = cell.detach().double().cpu().reshape(-1, 3, 3)
    return float(((c - first.float().double()).flatten(1).norm(dim=1) / first.flatten(1).norm(dim=1)).min())


def test_device_loop_equals_a_host_driven_loop(dev):
    """Seeded Langevin + scr, one launch per step on the device, against a loop that reads the virial and the kinetic record back
    every step, takes the torch path of ``_barostat`` on the host and calls ``set_cell``."""
    from e3_layers_amd.run import md as MD

    _, on, _ = _models(dev)
    p0, comp = _coupling(_initial_pressure(dev, on), "expand")
    n_steps = 8
    ff, mass, v0 = _start(dev, on)
    md = MD.Langevin(ff, mass, DT, KT, GAMMA, seed=SEED, barostat=MD.Barostat(p0, comp, TAU, "scr"))
    md.v.copy_(v0)
    # the host-driven twin: the same device kernels for the two half steps, the barostat on the host
    hf, _, _ = _start(dev, on)
    hv, hmass = v0.clone(), mass.to(dev)
    a, b = MD.Barostat(p0, comp, TAU, "scr").coefficients(DT, KT)
    node_ptr_host = hf.node_ptr.cpu()
    _, forces = hf(hf.pos.clone())
    hf.check()
    kin = torch.zeros(3, device=dev)
    MD._kick_langevin(hv, None, hmass, hf.node_ptr, 0.0, 1.0, 0.0, 0, 0, 0, kin)
    c, s = md._ou()
    counter = torch.zeros(1, dtype=torch.int32)
    worst = dict(x=0.0, v=0.0, cell=0.0, volume=0.0, pressure=0.0)
    counts = []
    for k in range(n_steps):
        out = md.run(1, check_every=1)
        MD._drift(hf.pos, hv, forces, hmass, DT)
        x, v, cell = hf.pos.cpu(), hv.cpu(), hf.cell.cpu().reshape(3, 9).clone()
        inv = torch.zeros_like(cell)
        vol, prs = torch.zeros(3, dtype=torch.float64), torch.zeros(3, dtype=torch.float64)
        MD._barostat(x, v, cell, inv, torch.ones(3, 3, dtype=torch.int32), hf.virial.cpu(), kin.cpu(), node_ptr_host, p0, a, b,
                     hf.min_width, SEED, k, counter, vol, prs)
        hf.set_cell(cell)
        hv.copy_(v)
        energy, forces = hf(x.to(dev))
        MD._kick_langevin(hv, forces, hmass, hf.node_ptr, DT, c, s, SEED, k, MD.THERMOSTAT_WORD, kin, energy, None)
        hf.check()
        assert int(counter) == 0
        mine, theirs = _list_of(ff), _list_of(hf)
        assert all(torch.equal(p, q) for p, q in zip(mine, theirs)), k      # the same list, image numbers included, at every step
        counts.append(int(ff.n_edges))
        errs = dict(x=rel_err(md.x, hf.pos), v=rel_err(md.v, hv), cell=rel_err(ff.static_cell, hf.cell.reshape(3, 9)),
                    volume=rel_err(out["volume"][0], vol), pressure=rel_err(out["pressure"][0], prs))
        print("npt parity", k, counts[-1], errs)
        worst = {key: max(worst[key], errs[key]) for key in worst}
    record_measured("npt_device_vs_host_driven", steps=n_steps, edges_first=counts[0], edges_last=counts[-1],
                    cell_move=_relative_move(ff.static_cell), **worst)
    assert max(worst.values()) < REPLAY, worst
    assert _relative_move(ff.static_cell) > 1e-3
    assert len(set(counts)) >= 2, counts      # the edge count changed on the way
    assert md.regrowths == 0 and ff.recaptures == hf.recaptures


def test_after_a_run_the_force_field_is_in_step_with_its_buffers(dev):
    from e3_layers_amd.run import md as MD

    _, on, _ = _models(dev)
    p0, comp = _coupling(_initial_pressure(dev, on), "expand")
    ff, mass, v0 = _start(dev, on)
    md = MD.Langevin(ff, mass, DT, KT, GAMMA, seed=SEED, barostat=MD.Barostat(p0, comp, TAU, "scr"))
    md.v.copy_(v0)
    out = md.run(9, check_every=4)
    assert set(out) == {"potential", "kinetic", "volume", "pressure"} and out["volume"].shape == (9, 3)
    assert out["volume"].dtype == torch.float64 and out["pressure"].dtype == torch.float64
    assert torch.equal(ff.cell.reshape(3, 9), ff.static_cell) and _relative_move(ff.cell) > 1e-3
    want = torch.linalg.det(ff.static_cell.double().cpu().reshape(3, 3, 3)).abs()
    assert torch.allclose(ff.volume.cpu(), want, rtol=1e-14, atol=0) and torch.allclose(out["volume"][-1].cpu(), want, rtol=1e-13, atol=0)
    assert not ff.static["cell"][-1].any() and not ff.static["_inv_cell"][-1].any()      # the ghost graph's rows stay zero
    eye = torch.einsum("gij,gjk->gik", ff.static_cell.double().reshape(3, 3, 3), ff.static_inv_cell.double().reshape(3, 3, 3))
    assert float((eye - torch.eye(3, device=dev, dtype=torch.float64)).abs().max()) < 1e-6
    pos = ff.pos.clone()
    energy, forces = ff(pos)
    ff.check()
    fresh_batch = _periodic_batch(cells=ff.cell.cpu().double(), pbc=ALL_PERIODIC, wrap=False)
    fresh_batch["pos"] = pos.cpu().clone()
    fresh = _ff(on, fresh_batch, dev, **KEYS)
    e1, f1 = fresh(pos)
    fresh.check()
    assert all(torch.equal(p, q) for p, q in zip(_list_of(ff), _list_of(fresh)))
    errs = [rel_err(energy, e1), rel_err(forces, f1), rel_err(ff.virial, fresh.virial), rel_err(ff.stress, fresh.stress)]
    print("npt: run's force field against a fresh capture", errs)
    record_measured("npt_run_vs_fresh_capture", energy=errs[0], forces=errs[1], virial=errs[2], stress=errs[3])
    assert max(errs) < REPLAY, errs


def test_a_list_outgrown_under_compression_is_regrown_on_the_last_verified_cell(dev):
    """``edge_slack = 1.0`` on a grid of 8 edges: the compression outgrows the list, the chunk is rolled back -- cell and inverse with
    it -- and the force field grows on the last verified cell.  The end state and all four records are the BITS of a run that never
    overflowed.  That run is given the bucket the tight run ends in (asserted: the same node and edge capacity): the model's
    kernels cut their sums by the padded sizes, so two different buckets agree within REPLAY only, whatever the integrator does
    (tests/test_gpu_md.py compares its regrown run that way) -- measured here in a suite run with the ample run at 2048 slots
    against the tight run's 1048: x, v, cell, inverse, potential, kinetic and volume bit-equal, the pressure record 1.3e-12 off."""
    from e3_layers_amd.run import md as MD

    _, on, _ = _models(dev)
    p0, comp = _coupling(_initial_pressure(dev, on), "compress", rate=0.01)
    probe = _start(dev, on)[0]
    probe(probe.pos.clone())
    probe.check()
    e0 = int(probe.n_edges)      # the edges of the start: the tight capacity is the next multiple of 8 above it
    runs = {}
    for name in ("tight", "ample"):
        # ample: the slack that asks for exactly the capacity the tight run grew to -- int(e0 slack) + 1 = e_cap
        kw = dict(edge_slack=1.0, edge_multiple=8) if name == "tight" else dict(edge_slack=(runs["tight"][1].e_cap - 0.5) / e0, edge_multiple=8)
        ff, mass, v0 = _start(dev, on, **kw)
        first_cap = ff.e_cap
        md = MD.Langevin(ff, mass, DT, KT, GAMMA, seed=SEED, barostat=MD.Barostat(p0, comp, TAU, "berendsen"))
        md.v.copy_(v0)
        out = md.run(10, check_every=4)
        runs[name] = (md, ff, out, first_cap)
    (tight, tff, tout, tcap), (ample, aff, aout, _) = runs["tight"], runs["ample"]
    print("npt regrowth: regrowths", tight.regrowths, "restores", tight.restores, "capacity", tcap, "->", tff.e_cap, "edges",
          int(tff.n_edges), "cell move", _relative_move(tff.cell))
    assert ample.regrowths == 0 and ample.restores == 0 and (aff.e_cap, aff.n_cap) == (tff.e_cap, tff.n_cap)      # the same bucket
    assert tight.regrowths >= 1 and tight.restores >= 1 and tff.e_cap > tcap and int(tff.n_edges) > tcap
    assert _relative_move(tff.cell) > 1e-3
    for name, p, q in (("x", tight.x, ample.x), ("v", tight.v, ample.v), ("cell", tff.static_cell, aff.static_cell),
                       ("inverse", tff.static_inv_cell, aff.static_inv_cell), ("ff.cell", tff.cell, aff.cell)):
        assert torch.equal(p, q), (name, rel_err(p, q))
    for key in ("potential", "kinetic", "volume", "pressure"):
        assert torch.equal(tout[key], aout[key]), (key, rel_err(tout[key], aout[key]))


def test_zero_compressibility_is_the_plain_integrator_and_none_launches_nothing(dev, monkeypatch):
    from e3_layers_amd.run import md as MD

    _, on, _ = _models(dev)
    runs = []
    for baro in (None, MD.Barostat(0.01, 0.0, TAU, "berendsen")):
        ff, mass, v0 = _start(dev, on)
        md = MD.VelocityVerlet(ff, mass, DT, barostat=baro)
        md.v.copy_(v0)
        if baro is None:
            monkeypatch.setattr(MD, "_barostat", lambda *a, **k: pytest.fail("barostat=None launched the barostat"))
        out = md.run(8, check_every=3)
        monkeypatch.undo()
        assert set(out) == ({"potential", "kinetic"} if baro is None else {"potential", "kinetic", "volume", "pressure"})
        runs.append((md.x.clone(), md.v.clone(), out["potential"].clone(), out["kinetic"].clone(), ff.static_cell.clone()))
    for name, p, q in zip(("x", "v", "potential", "kinetic", "cell"), *runs):
        assert torch.equal(p, q), name
    assert torch.equal(runs[1][4].cpu(), CELLS.float().reshape(3, 9))


def test_a_cell_that_would_become_too_narrow_raises_at_the_chunks_check(dev):
    from e3_layers_amd.run import md as MD

    _, on, _ = _models(dev)
    p_start = _initial_pressure(dev, on)
    p0, comp = _coupling(p_start, "compress", rate=0.45)      # exp(-0.45 / 3) = 0.86: the 9.0-wide cell would fall to 7.7 < 8.008
    ff, mass, v0 = _start(dev, on)
    md = MD.Langevin(ff, mass, DT, KT, GAMMA, seed=SEED, barostat=MD.Barostat(p0, comp, TAU, "berendsen"))
    md.v.copy_(v0)
    x0 = ff.pos.clone()
    with pytest.raises(MD.BarostatFailure) as err:
        md.run(4, check_every=2)
    assert err.value.count >= 1 and md.restores == 1 and md.steps_done == 0
    assert torch.equal(ff.cell.cpu(), CELLS.float()) and torch.equal(ff.static_cell.cpu(), CELLS.float().reshape(3, 9))
    assert torch.equal(md.x, x0) and torch.equal(md.v, v0) and int(md._baro_counter) == 0
    p0, comp = _coupling(p_start, "expand")
    md.barostat = MD.Barostat(p0, comp, TAU, "berendsen")
    out = md.run(4, check_every=2)
    assert md.steps_done == 4 and bool((out["volume"] > 0).all()) and _relative_move(ff.cell) > 1e-3
