"""Bond-length constraints on the device (csrc/e3k_md.hip: ``e3k_md_drift_shake``, ``e3k_md_kick_rattle``): single calls
against the float64 torch path converged to 1e-12, with the float32 torch path on the CPU as the yardstick; the drivers through the
kernels on stub fields that live on the device (the host tests' systems and bounds); and on the replayed force field against the
float64 oracle loop."""
import math

import pytest
import torch

from tests.md_constraint_stubs import SIZES, assert_constraints_hold, one_star_type, star_geometry, star_wells
from tests.md_stubs import node_ptr_of
from tests.test_md_constraints_host import DT, KT, _drift_of, _driver, constrained_equipartition_ratio
from tests.util import record_measured, rel_err

pytestmark = pytest.mark.gpu

EPS32 = 2.0 ** -24
TOL = 1e-5


def _single_call_inputs(masses):
    """x (fp32 values), v, f, mass in float64 on the host, the pairs and their lengths at x (fp32 values): the three runs share
    every input bit."""
    pos, pairs, mass, sizes = star_geometry(masses=masses)
    gen = torch.Generator().manual_seed(17)
    x = pos.float().double()
    mass = mass.float().double()
    v = (0.3 * torch.randn(x.shape, generator=gen, dtype=torch.float64) / mass.sqrt()[:, None]).float().double()
    f = (2.0 * torch.randn(x.shape, generator=gen, dtype=torch.float64)).float().double()
    d0 = (x[pairs[:, 0]] - x[pairs[:, 1]]).norm(dim=1).float().double()
    return x, v, f, mass, pairs, d0, sizes


def _constraints(pairs, d0, x, mass, sizes, dtype, device, **kw):
    from e3_layers_amd.run.md import BondConstraints

    return BondConstraints(pairs, d0, pos=x.to(dtype).to(device), node_ptr=node_ptr_of(sizes), masses=mass.to(dtype).to(device), **kw)


@pytest.mark.parametrize("masses", ["hydrogen", "random"])
def test_single_calls_follow_the_converged_float64_projection(dev, masses):
    """One ``e3k_md_drift_shake`` call, then one ``e3k_md_kick_rattle`` call (c = 1, s = 0, with forces) at the float64 result's
    positions.  Lengths after SHAKE: |d - d0| / d0 <= tol + 2 sqrt(3) 2^-23 max|x| / d0 (the stopping rule plus the rounding of the
    two stored end points).  Distance of x and v from the float64 path converged to 1e-12: at most 4 x that of the float32 torch
    path run on the CPU (compiler contraction, the order of the sweeps' roundings)."""
    from e3_layers_amd.run import md as M

    x, v, f, mass, pairs, d0, sizes = _single_call_inputs(masses)
    dt = 0.05
    runs = {}
    for name, dtype, device, kw in (("f64", torch.float64, "cpu", dict(tol=1e-12, max_iter=200)), ("f32", torch.float32, "cpu", {}),
                                    ("dev", torch.float32, dev, {})):
        con = _constraints(pairs, d0, x, mass, sizes, dtype, device, **kw)
        xs, vs, fs, ms = (t.to(dtype).to(device).clone().contiguous() for t in (x, v, f, mass))
        M._drift(xs, vs, fs, ms, dt, con)
        runs[name] = [con, xs.clone(), vs.clone()]
    x_mid = runs["f64"][1].float().double()              # the common input of the second call: the converged positions in fp32
    kin = {}
    for name, dtype, device in (("f64", torch.float64, "cpu"), ("f32", torch.float32, "cpu"), ("dev", torch.float32, dev)):
        con = runs[name][0]
        xs, vs, fs, ms = (t.to(dtype).to(device).clone().contiguous() for t in (x_mid, v, f, mass))
        kin[name] = torch.zeros(len(sizes), dtype=dtype, device=device)
        M._kick_langevin(vs, fs, ms, node_ptr_of(sizes, device), dt, 1.0, 0.0, 0, 0, 0, kin[name], con=con, x=xs)
        runs[name].append(vs.clone())
        assert con.counters.tolist() == [0, 0], (name, con.counters.tolist())
    con, x_dev, v_dev, v2_dev = runs["dev"]
    length = ((x_dev.double().cpu()[pairs[:, 0]] - x_dev.double().cpu()[pairs[:, 1]]).norm(dim=1) - d0).abs() / d0
    bound = TOL + 2 * math.sqrt(3.0) * 2.0 ** -23 * float(x_dev.abs().max()) / d0
    print("shake lengths", masses, float(length.max()), float((length / bound).max()))
    # RATTLE's rule on the stored numbers (the helper's length check sees x_mid, which is converged)
    assert_constraints_hold(con, x_mid, v2_dev, EPS32, "after e3k_md_kick_rattle")

    def dist(name, i):
        return float((runs[name][i].double().cpu() - runs["f64"][i]).norm())

    d = {f"{which}_{name}": dist(name, i) for i, which in ((1, "shake_x"), (2, "shake_v"), (3, "rattle_v")) for name in ("dev", "f32")}
    d["kinetic_dev"], d["kinetic_f32"] = (float((kin[k].double().cpu() - kin["f64"]).abs().max()) for k in ("dev", "f32"))
    print("single calls", masses, d)
    record_measured(f"md_constraints_single_calls_{masses}", worst_length_error=float(length.max()), **d)
    assert bool((length <= bound).all()), float((length / bound).max())
    for which in ("shake_x", "shake_v", "rattle_v"):
        assert d[f"{which}_dev"] <= 4 * d[f"{which}_f32"], (which, d)
    # the free atoms took e3k_md_drift's update, the kinetic energies are those of the written velocities
    free = con.free_atom
    want_v = v[free.cpu()] + 0.5 * dt * f[free.cpu()] / mass[free.cpu(), None]
    assert rel_err(v_dev[free], want_v) < 1e-6 and rel_err(x_dev[free], x[free.cpu()] + dt * want_v) < 1e-6
    per_node = 0.5 * mass[:, None] * v2_dev.double().cpu() ** 2
    want_kin = torch.stack([per_node[a:b].sum() for a, b in zip(node_ptr_of(sizes)[:-1], node_ptr_of(sizes)[1:])])
    n_g = torch.tensor(sizes, dtype=torch.float64)      # a sum of n_g positive terms in fp32, each a few roundings itself
    assert bool(((kin["dev"].double().cpu() - want_kin).abs() <= (n_g + 4) * EPS32 * want_kin).all())


def test_a_projection_leaves_every_stars_momentum_where_it_was(dev):
    """f NULL, c = 1, s = 0: RATTLE's corrections are equal and opposite impulses, so every star's sum of m v stays, up to the
    rounding of the sweeps: 16 2^-24 sum m |v|."""
    from e3_layers_amd.run import md as M

    x, v, _, mass, pairs, d0, sizes = _single_call_inputs("random")
    con = _constraints(pairs, d0, x, mass, sizes, torch.float32, dev)
    xs, vs, ms = (t.float().to(dev).contiguous() for t in (x, v, mass))
    before = vs.clone()
    M._kick_langevin(vs, None, ms, node_ptr_of(sizes, dev), 0.0, 1.0, 0.0, 0, 0, 0, None, con=con, x=xs)
    assert con.counters.tolist() == [0, 0]
    assert_constraints_hold(con, xs, vs, EPS32, "after the projection")
    assert torch.equal(vs[con.free_atom], before[con.free_atom]) and not torch.equal(vs, before)
    idx, valid = con._idx.cpu(), con._valid.cpu()
    m = (mass[idx] * valid)[:, :, None]
    p0, p1 = (m * before.double().cpu()[idx]).sum(1), (m * vs.double().cpu()[idx]).sum(1)
    bound = 16 * EPS32 * (m[:, :, 0] * before.double().cpu()[idx].norm(dim=2)).sum(1)
    worst = float(((p1 - p0).abs().max(dim=1).values / bound).max())
    print("momentum change / bound", worst)
    record_measured("md_constraints_momentum", worst_over_bound=worst)
    assert worst <= 1.0


@pytest.mark.parametrize("cls", ["nve", "langevin"])
def test_an_empty_set_is_the_unconstrained_kernels_bit_for_bit(dev, cls):
    field, mass, con, v0 = star_wells(constrained=False, dtype=torch.float32, device=dev)
    plain, _, _, _ = star_wells(constrained=False, dtype=torch.float32, device=dev)
    a, b = _driver(cls, field, mass, con, DT), _driver(cls, plain, mass, None, DT)
    outs = []
    for md in (a, b):
        md.v.copy_(v0)
        outs.append(md.run(10, check_every=5))
    assert torch.equal(a.x, b.x) and torch.equal(a.v, b.v)
    assert torch.equal(outs[0]["kinetic"], outs[1]["kinetic"]) and torch.equal(outs[0]["potential"], outs[1]["potential"])
    assert bool((outs[0]["kinetic"].sum(1) > 0).all())
    a.thermalize(KT), b.thermalize(KT)
    assert torch.equal(a.v, b.v)


@pytest.mark.parametrize("masses", ["hydrogen", "random"])
def test_constraints_hold_along_an_nve_trajectory_through_the_kernels(dev, masses):
    """The host test on device tensors: 200 steps, the rules checked after every chunk of 20 at fp32's precision."""
    field, mass, con, v0 = star_wells(masses=masses, dtype=torch.float32, device=dev)
    md = _driver("nve", field, mass, con, DT)
    md.v.copy_(v0)
    md.project()
    assert_constraints_hold(con, md.x, md.v, EPS32, "after project()")
    worst = (0.0, 0.0)
    for chunk in range(10):
        out = md.run(20, check_every=20)
        worst = tuple(max(a, b) for a, b in zip(worst, assert_constraints_hold(con, md.x, md.v, EPS32, f"chunk {chunk}")))
        assert bool(torch.isfinite(out["kinetic"]).all()) and con.counters.tolist() == [0, 0]
    print("device nve", masses, worst)
    record_measured(f"md_constraints_nve_{masses}", worst_length_error=worst[0], worst_rv_over_scale=worst[1])
    assert md.restores == 0 and md.steps_done == 200
    assert float((md.x - field.sites).abs().max()) > 0.05


def test_energy_is_conserved_to_second_order_through_the_kernels(dev):
    d = [_drift_of(0.1 / k, 60 * k, dtype=torch.float32, device=dev) for k in (1, 2)]
    print("device energy drift under constraints", d)
    record_measured("md_constraints_energy_drift", device_dt=d[0], device_half_dt=d[1])
    assert d[1] < 0.5 * d[0], d


def test_langevin_reaches_equipartition_through_the_kernels(dev):
    field, mass, con = one_star_type(dtype=torch.float32, device=dev)
    md = _driver("langevin", field, mass, con, DT, seed=0)
    md.thermalize()
    ratio = constrained_equipartition_ratio(md, KT)
    print("constrained equipartition on the device", ratio)
    record_measured("md_constraints_equipartition", ratio=ratio, counting_3n=ratio * 576.0 / 768.0)
    assert con.counters.tolist() == [0, 0]
    assert abs(ratio - 1.0) <= 0.03, ratio


@pytest.mark.parametrize("cls", ["langevin", "nve"])
def test_thermalize_sets_every_graphs_temperature_over_its_own_dof(dev, cls):
    """As ``test_thermalize_sets_every_graphs_temperature`` does for 3n: 2 KE / (dof_g kT) = 1 within 5 sigma of a chi-square
    with dof_g degrees of freedom, for the two large graphs; the drawn velocities satisfy the constraints; a free atom's velocity
    is the unconstrained draw (the noise is indexed by the atom's row, not by its place in the tables)."""
    from e3_layers_amd.data.compute_edge import normal_draw
    from tests.test_gpu_md_integrator_kernels import XI_BOUND

    field, mass, con, _ = star_wells(masses="random", dtype=torch.float32, device=dev)
    md = _driver(cls, field, mass, con, DT, seed=9)
    md.v.fill_(5.0)
    md.thermalize() if cls == "langevin" else md.thermalize(KT)
    assert con.counters.tolist() == [0, 0]
    assert_constraints_hold(con, md.x, md.v, EPS32, "after thermalize()")
    v, m = md.v.double().cpu(), mass.double().cpu()
    ptr, dof = node_ptr_of(SIZES), md.dof.cpu()
    for g in (1, 4):
        a, b = int(ptr[g]), int(ptr[g + 1])
        ratio = float((m[a:b, None] * v[a:b] ** 2).sum()) / (float(dof[g]) * KT)
        print("constrained thermalize", cls, g, int(dof[g]), ratio)
        assert abs(ratio - 1.0) <= 5 * math.sqrt(2.0 / float(dof[g])), (g, ratio)
    free = con.free_atom.cpu()
    amp = (float(torch.tensor(KT ** 0.5, dtype=torch.float32)) / m[free].sqrt())[:, None]
    want = amp * normal_draw(9, 0, free[:, None], 4 + torch.arange(3)[None, :], torch.float64)
    assert bool(((v[free] - want).abs() <= 1e-6 * float(want.abs().max()) + amp * XI_BOUND).all())


def test_a_star_that_does_not_converge_rolls_the_chunk_back_on_the_device(dev):
    from e3_layers_amd.run.md import ConstraintFailure

    graphs = (((1,) * 9, 1), ((), 2), ((1,) * 3, 0))
    field, mass, con, v0 = star_wells(graphs=graphs, max_iter=1, dtype=torch.float32, device=dev)
    md = _driver("nve", field, mass, con, 0.02)
    md.v.copy_(0.01 * v0)
    md.project()
    md.run(4, check_every=2)
    assert con.counters.tolist() == [0, 0] and md.steps_done == 4
    md.v.mul_(300.0)
    x1, v1 = md.x.clone(), md.v.clone()
    with pytest.raises(ConstraintFailure) as err:
        md.run(8, check_every=4)
    assert err.value.shake >= 1
    assert torch.equal(md.x, x1) and torch.equal(md.v, v1)
    assert con.counters.tolist() == [0, 0] and md.steps_done == 4 and md.restores == 1
    assert not bool(md._kin.any()) and not bool(md._pot.any())
    con.max_iter = 32
    md.run(8, check_every=4)
    assert md.steps_done == 12 and con.counters.tolist() == [0, 0]
    assert_constraints_hold(con, md.x, md.v, EPS32, "after the repeated run")


# ---- on the replayed force field ------------------------------------------------------------------------------------
def _molecules(dev):
    from e3_layers_amd.data.synthetic import synth_qm9
    from e3_layers_amd.run.md import hydrogen_bonds
    from tests.test_gpu_md import _build, _oracle, _OracleField, _small_tree

    tree = _small_tree()
    prod = _build(tree, dev)
    batch = synth_qm9(7, 3)
    fields = {dt: _OracleField(_oracle(prod, tree, dt), batch, 4.0, "energy_total", dt) for dt in (torch.float64, torch.float32)}
    light = batch["species"].reshape(-1) == 1
    ptr = node_ptr_of(batch["_n_nodes"].reshape(-1).tolist())
    pairs = hydrogen_bonds(batch["pos"], light, ptr, 1.3)
    mass = torch.where(light, 1.0, 12.0)
    return prod, batch, fields, pairs, mass, ptr


def _force_field(prod, batch, dev, **kw):
    from e3_layers_amd.run.md import ReplayedForceField

    return ReplayedForceField(prod, batch.clone().to(dev), 4.0, energy_key="energy_total", forces_key="forces", **kw)


def test_constrained_trajectory_follows_the_float64_loop_as_closely_as_a_float32_loop_does(dev):
    """20 constrained steps of the small tree on ``synth_qm9`` with its ``hydrogen_bonds`` (H 1, the rest 12; unit-variance
    velocities, projected): the device against ``VelocityVerlet`` on the float64 oracle with the constraints converged to 1e-12;
    yardstick: the same driver on the float32 oracle at the default tol.  The device may be 4 x further away."""
    from e3_layers_amd.run.md import BondConstraints, VelocityVerlet
    from tests.test_gpu_md_thermostat import _HostField

    prod, batch, fields, pairs, mass, ptr = _molecules(dev)
    assert pairs.shape[0] >= 10
    dt, n_steps = 0.02, 20
    x0 = batch["pos"].clone()
    v0 = torch.randn(x0.shape, generator=torch.Generator().manual_seed(1), dtype=torch.float64).float()

    def run(ff, dtype, device, **kw):
        con = BondConstraints(pairs, pos=x0.to(dtype).to(device), node_ptr=ptr, masses=mass.to(dtype).to(device), **kw)
        md = VelocityVerlet(ff, mass, dt, constraints=con)
        md.v.copy_(v0.to(device))
        md.project()
        out = md.run(n_steps, check_every=5)
        assert con.counters.tolist() == [0, 0] and md.regrowths == 0
        return md, (out["potential"].double().sum(1) + out["kinetic"].double().sum(1)).cpu()

    md64, e64 = run(_HostField(fields[torch.float64], batch, x0), torch.float64, "cpu", tol=1e-12, max_iter=200)
    assert len(set(fields[torch.float64].edge_counts)) >= 2, fields[torch.float64].edge_counts      # the list changed on the way
    md32, e32 = run(_HostField(fields[torch.float32], batch, x0), torch.float32, "cpu")
    ff = _force_field(prod, batch, dev)
    ff(x0.to(dev))
    ff.check()
    md, e_dev = run(ff, torch.float32, dev)
    assert_constraints_hold(md.constraints, md.x, md.v, EPS32, "after the device run")
    x64 = md64.x.double()
    d32_x, d32_e = float((md32.x.double() - x64).norm()), float((e32 - e64).abs().max())
    dev_x, dev_e = float((md.x.double().cpu() - x64).norm()), float((e_dev - e64).abs().max())
    print("md_constrained_trajectory", dict(dev_x=dev_x, d32_x=d32_x, dev_e=dev_e, d32_e=d32_e))
    record_measured("md_constrained_trajectory", device_positions=dev_x, float32_positions=d32_x, device_energy=dev_e, float32_energy=d32_e,
                    constraints=int(pairs.shape[0]))
    assert dev_x <= 4 * d32_x, (dev_x, d32_x)
    assert dev_e <= 4 * d32_e, (dev_e, d32_e)


def test_a_regrown_constrained_run_ends_where_an_ample_one_ends(dev):
    """Velocities towards the centroids (projected), no slack and a fine bucket grid: the run regrows its edge capacity, restores
    and redoes a chunk; the kernels are stateless and the counters cleared, so it ends where the run with ample capacity ends."""
    from e3_layers_amd.run.md import BondConstraints, VelocityVerlet

    prod, batch, _, pairs, mass, ptr = _molecules(dev)
    x0, seg = batch["pos"].clone(), batch["_node_segment"]
    cen = torch.zeros(len(batch), 3).index_add_(0, seg, x0) / batch["_n_nodes"].float()
    v0 = -(x0 - cen[seg])
    runs = {}
    for name, kw in (("tight", dict(edge_slack=1.0, edge_multiple=32)), ("ample", dict(edge_slack=2.0))):
        ff = _force_field(prod, batch, dev, **kw)
        ff(x0.to(dev))
        ff.check()
        first_cap = ff.e_cap
        con = BondConstraints(pairs, pos=x0.to(dev), node_ptr=ptr, masses=mass.to(dev))
        md = VelocityVerlet(ff, mass, 0.02, constraints=con)
        md.v.copy_(v0.to(dev))
        md.project()
        out = md.run(12, check_every=4)
        assert con.counters.tolist() == [0, 0]
        runs[name] = (md, out, first_cap, ff)
    tight, ample = runs["tight"], runs["ample"]
    assert ample[0].regrowths == 0
    assert tight[0].regrowths >= 1 and tight[0].restores >= 1 and tight[3].e_cap > tight[2]
    assert_constraints_hold(tight[0].constraints, tight[0].x, tight[0].v, EPS32, "after the regrown run")
    errs = dict(x=rel_err(tight[0].x, ample[0].x), v=rel_err(tight[0].v, ample[0].v),
                kinetic=rel_err(tight[1]["kinetic"], ample[1]["kinetic"]), potential=rel_err(tight[1]["potential"], ample[1]["potential"]))
    print("md_constrained_regrowth", errs)
    record_measured("md_constrained_regrowth", **errs)
    assert torch.equal(tight[0].x, ample[0].x) and torch.equal(tight[0].v, ample[0].v), errs
    assert torch.equal(tight[1]["kinetic"], ample[1]["kinetic"]) and torch.equal(tight[1]["potential"], ample[1]["potential"]), errs
