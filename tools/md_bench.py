#!/usr/bin/env python3
"""Per-step time of velocity-Verlet MD on config_energy_force: the replayed force field (run/md.py: one HIP graph per force
evaluation, the neighbour list rebuilt inside it, two integrator launches beside it) against the eager loop the package offered before it
(computeEdgeIndex on the device + the eager model call + an element-wise torch integrator), on the same start.

    python tools/md_bench.py --molecules 32 64 1 --steps 200 --out profiles/md_replay.json
    python tools/md_bench.py --integrator langevin --out profiles/md_langevin.json      (the thermostatted step against the NVE step)
    python tools/md_bench.py --fire --out profiles/md_fire.json                         (the FIRE iteration against its eager loop)
    python tools/md_bench.py --constraints --out profiles/md_constraints.json           (the SHAKE / RATTLE step against the plain step)
    python tools/md_bench.py --pbc --molecules 32 64 --out profiles/md_pbc.json         (the step in a vacuum cell against the open step)
    python tools/md_bench.py --images --molecules 32 64 --out profiles/md_images.json   (all images: wide cell vs minimum image; narrow cell vs supercell)
    python tools/md_bench.py --stress --out profiles/md_stress.json                    (virial and stress delivered against the same step without)
    python tools/md_bench.py --stress --one-graph --molecules 128                       (... with the molecules as ONE graph of 2 000+ atoms)
    python tools/md_bench.py --npt --molecules 32 64 --out profiles/md_npt.json         (Langevin + scr barostat against the same step without, keys on)
    python tools/md_bench.py --npt --one-graph --molecules 128                          (... one workgroup of the barostat walks every component)
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o s -- python tools/md_bench.py --trace-steps 60 --molecules 32
    python tools/md_bench.py --launches DIR_A/…_kernel_stats.csv 10 DIR_B/…_kernel_stats.csv 60      (launches per replayed step)

Protocol: device events around ``--steps`` steps after a warm-up, the two variants alternating in one process, ``--reps``
repetitions each (min / median / max); host-busy time is the wall time of the enqueue loop before the closing synchronisation,
as bench.py reports it.  No threshold is asserted: the numbers are quoted in README.md and DESIGN.md.
"""
from __future__ import annotations

import argparse
import csv
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "equivariant-nn-zoo_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import torch


def setup(n_mol: int, dev):
    from e3_layers_amd.configs import config_energy_force
    from e3_layers_amd.data.synthetic import synth_qm9
    from e3_layers_amd.utils import build

    tree = config_energy_force.get_config().model_config
    torch.manual_seed(0)
    model = build(tree).to(dev).eval()
    batch = synth_qm9(4000 + n_mol, n_mol, config_energy_force.SHIFTS, r_max=tree.r_max).to(dev)
    x0 = batch["pos"].clone()
    v0 = 0.5 * torch.randn(x0.shape, generator=torch.Generator().manual_seed(1)).to(dev)
    return model, batch, float(tree.r_max), x0, v0


def eager_steps(model, batch, r_max, x0, v0, dt, n_steps):
    """computeEdgeIndex + the eager model + torch element-wise velocity Verlet (unit masses).  The first force evaluation is done
    here; the returned loop does the steps and returns the host-busy seconds."""
    from e3_layers_amd.data import computeEdgeIndex

    def force(x):
        b = batch.view()
        b["pos"] = x
        for k in ("edge_index", "_n_edges", "_edge_segment"):
            b.pop(k)
        new, attrs = computeEdgeIndex(b.data, b.attrs, r_max=r_max)
        b.attrs.update(attrs)
        b.update(new)
        out = model(b)
        return out["energy"], out["forces"]

    x, v = x0.clone(), v0.clone()
    _, f = force(x)

    def loop():
        nonlocal x, v, f
        t0 = time.perf_counter()
        for _ in range(n_steps):
            v = v + 0.5 * dt * f
            x = (x + dt * v).detach()
            _, f = force(x)
            v = v + 0.5 * dt * f
        return time.perf_counter() - t0

    return loop


def eager_fire(model, batch, r_max, x0, fire, n_steps):
    """computeEdgeIndex + the eager model + the torch path of the FIRE iteration on device tensors: every branch of every graph is
    decided on the host, as a minimiser written beside the model would do it."""
    from e3_layers_amd.data import computeEdgeIndex
    from e3_layers_amd.run import md as M

    def force(x):
        b = batch.view()
        b["pos"] = x
        for k in ("edge_index", "_n_edges", "_edge_segment"):
            b.pop(k)
        new, attrs = computeEdgeIndex(b.data, b.attrs, r_max=r_max)
        b.attrs.update(attrs)
        b.update(new)
        out = model(b)
        return out["energy"].reshape(-1), out["forces"]

    x, v, state = x0.clone(), torch.zeros_like(x0), fire.state.clone()
    node_ptr = fire.ff.node_ptr

    def loop():
        t0 = time.perf_counter()
        for _ in range(n_steps):
            energy, f = force(x)
            M._fire_step_torch(x, v, f.detach(), node_ptr, state, fire)
        return time.perf_counter() - t0

    return loop


def replay_fire(fire, ff, n_steps):
    """The launches of ``Fire.run``'s inner loop (the graph + ``e3k_fire_step``), without the chunk's closing synchronisation."""
    from e3_layers_amd.run import md as M

    n_graphs = ff.node_ptr.numel() - 1
    rec = torch.zeros(2, n_steps, n_graphs, device=ff.dev)

    def loop():
        t0 = time.perf_counter()
        for i in range(n_steps):
            energy, forces = ff.evaluate()
            M._fire_step(ff.pos, fire.v, forces, ff.node_ptr, fire.state, fire, energy, rec[0, i], rec[1, i])
        return time.perf_counter() - t0

    return loop


def replay_start(md, ff, x0, v0):
    """Puts the replayed run on the start (verified forces there): outside the timed region."""
    ff.pos.copy_(x0)
    md.v.copy_(v0)
    md._forces = None
    _, md._forces = md._verified_forces()
    if getattr(md, "barostat", None) is not None:      # the kinetic energies the first barostat step reads (run() files them)
        from e3_layers_amd.run import md as M

        M._kick_langevin(md.v, None, md.mass, ff.node_ptr, 0.0, 1.0, 0.0, 0, 0, 0, md._kin0)


def replay_steps(md, ff, n_steps):
    """The launches of ``VelocityVerlet.run``'s inner loop (plain, thermostatted or constrained: what ``md`` is), and nothing else:
    ``run`` closes a chunk with ``check()``, a host synchronisation that would sit between the two events -- the caller checks after
    the closing event instead."""
    from e3_layers_amd.run import md as M

    n_graphs = ff.node_ptr.numel() - 1
    pot = torch.zeros(n_steps, n_graphs, device=ff.dev)
    kin = torch.zeros_like(pot)
    forces, con, (c, s) = md._forces, md.constraints, md._ou()
    baro = getattr(md, "barostat", None)
    if baro is not None:
        vol = torch.zeros(n_steps, n_graphs, dtype=torch.float64, device=ff.dev)
        prs = torch.zeros_like(vol)
        a, b = baro.coefficients(md.dt, getattr(md, "kT", None))

    def loop():
        nonlocal forces
        t0 = time.perf_counter()
        for i in range(n_steps):
            M._drift(ff.pos, md.v, forces, md.mass, md.dt, con)
            if baro is not None:      # e3k_barostat_step: the launch VelocityVerlet._step puts between drift and graph
                M._barostat(ff.pos, md.v if baro.mode == "scr" else None, ff.static_cell, ff.static_inv_cell, ff.static_pbc, ff.virial,
                            kin[i - 1] if i else md._kin0, ff.node_ptr, baro.p0, a, b, ff.min_width, md.seed, i, md._baro_counter,
                            vol[i], prs[i])
            energy, forces = ff.evaluate()
            M._kick_langevin(md.v, forces, md.mass, ff.node_ptr, md.dt, c, s, md.seed, i, M.THERMOSTAT_WORD, kin[i], energy, pot[i],
                             con=con, x=ff.pos)      # e3k_md_kick, e3k_md_kick_langevin or e3k_md_kick_rattle, with draw index i
        return time.perf_counter() - t0

    return loop


def bonds_to_hydrogen(batch, x0, ff, reach=1.3):
    """(constraints, masses) for the benchmark: H 1, the rest 12; every H within ``reach`` of a heavy atom is bound to the nearest
    one.  synth_qm9's geometries are random, not chemistry: a heavy atom that would collect more than four keeps its first four."""
    from e3_layers_amd.run.md import MAX_SATELLITES, BondConstraints, hydrogen_bonds

    light = batch["species"].reshape(-1) == 1
    mass = torch.where(light, 1.0, 12.0).to(x0)
    pairs = hydrogen_bonds(x0, light, ff.node_ptr, reach).cpu()
    order = torch.argsort(pairs[:, 0], stable=True)
    pairs = pairs[order]
    first = torch.searchsorted(pairs[:, 0].contiguous(), pairs[:, 0].contiguous())
    pairs = pairs[torch.arange(pairs.shape[0]) - first < MAX_SATELLITES]
    return BondConstraints(pairs, pos=x0, node_ptr=ff.node_ptr, masses=mass), mass


def bench_constraints(n_mol, steps, warmup, reps, dt, dev):
    """The constrained step against the plain step of the same build on ONE force field, the same masses and the same (projected)
    start: the two differ in their two launches outside the graph."""
    from e3_layers_amd.run.md import ReplayedForceField, VelocityVerlet

    model, batch, r_max, x0, v0 = setup(n_mol, dev)
    ff = ReplayedForceField(model, batch, r_max)
    con, mass = bonds_to_hydrogen(batch, x0, ff)
    mds = {"plain": VelocityVerlet(ff, mass, dt), "constrained": VelocityVerlet(ff, mass, dt, constraints=con)}
    mds["constrained"].v.copy_(v0)
    ff.pos.copy_(x0)
    mds["constrained"].project()
    v0 = mds["constrained"].v.clone()             # both start on the constraint surface
    rows = {k: [] for k in ("plain", "constrained", "plain_host", "constrained_host")}
    for name, md in mds.items():
        replay_start(md, ff, x0, v0)
        md.run(warmup, check_every=warmup)
    for _ in range(reps):
        for name, md in mds.items():
            replay_start(md, ff, x0, v0)
            ms, host = timed(replay_steps(md, ff, steps))
            ff.check()
            rows[name].append(ms / steps)
            rows[name + "_host"].append(1e3 * host / steps)
    failures = con.counters.tolist()
    diff = statistics.median(rows["constrained"]) - statistics.median(rows["plain"])
    return {"molecules": n_mol, "atoms": int(x0.shape[0]), "constraints": con.n_constraints, "stars": con.n_stars, "e_cap": ff.e_cap,
            "steps": steps, "reps": reps, "dt": dt, "tol": con.tol, "max_iter": con.max_iter, "shake_failures": failures[0],
            "rattle_failures": failures[1], "regrowths": sum(md.regrowths for md in mds.values()), "recaptures": ff.recaptures,
            "plain_ms_per_step": mmm(rows["plain"]), "constrained_ms_per_step": mmm(rows["constrained"]),
            "plain_host_busy_ms_per_step": mmm(rows["plain_host"]), "constrained_host_busy_ms_per_step": mmm(rows["constrained_host"]),
            "constrained_minus_plain_us_median": round(1e3 * diff, 2),
            "constrained_over_plain_median": round(statistics.median(rows["constrained"]) / statistics.median(rows["plain"]), 4)}


def bench_pbc(n_mol, steps, warmup, reps, dt, dev):
    """The periodic step against the open-boundary step of the same build: the same batch once without a cell and once in a cubic
    vacuum cell (width: the batch's extent + 2 r_max + 8, so no image is ever inside the cutoff and the two edge sets are
    identical -- asserted at the start).  What differs is the builder's two kernels (the rule of csrc/e3k_pbc.h in the pair loop,
    the image numbers written) and the edge-vector kernel; each variant has its own force field, the two alternate."""
    from e3_layers_amd.run.md import ReplayedForceField, VelocityVerlet

    model, batch, r_max, x0, v0 = setup(n_mol, dev)
    width = float((x0.max(0).values - x0.min(0).values).max()) + 2.0 * r_max + 8.0
    vac = batch.clone()
    vac.attrs["cell"] = ("graph", "3x1o")
    vac["cell"] = (width * torch.eye(3, device=dev)).reshape(1, 9).repeat(len(batch), 1)
    ffs = {"open": ReplayedForceField(model, batch, r_max), "periodic": ReplayedForceField(model, vac, r_max)}
    mds = {k: VelocityVerlet(ff, torch.ones(x0.shape[0]), dt) for k, ff in ffs.items()}
    rows = {k: [] for k in ("open", "periodic", "open_host", "periodic_host")}
    for name, md in mds.items():
        replay_start(md, ffs[name], x0, v0)
        md.run(warmup, check_every=warmup)
    edges = {}
    for name, md in mds.items():      # the same list at the start
        replay_start(md, ffs[name], x0, v0)
        n = int(ffs[name].n_edges)
        edges[name] = ffs[name].static["edge_index"][:, :n].clone()
    if not torch.equal(edges["open"], edges["periodic"]):
        raise RuntimeError("the vacuum cell's edge set differs from the open one")
    for _ in range(reps):
        for name, md in mds.items():
            replay_start(md, ffs[name], x0, v0)
            ms, host = timed(replay_steps(md, ffs[name], steps))
            ffs[name].check()
            rows[name].append(ms / steps)
            rows[name + "_host"].append(1e3 * host / steps)
    end = {k: int(ff.n_edges) for k, ff in ffs.items()}
    diff = statistics.median(rows["periodic"]) - statistics.median(rows["open"])
    return {"molecules": n_mol, "atoms": int(x0.shape[0]), "edges_at_start": int(edges["open"].shape[1]), "edges_at_end": end,
            "cell_width": round(width, 3), "e_cap": {k: ff.e_cap for k, ff in ffs.items()}, "steps": steps, "reps": reps, "dt": dt,
            "regrowths": sum(md.regrowths for md in mds.values()), "recaptures": sum(ff.recaptures for ff in ffs.values()),
            "open_ms_per_step": mmm(rows["open"]), "periodic_ms_per_step": mmm(rows["periodic"]),
            "open_host_busy_ms_per_step": mmm(rows["open_host"]), "periodic_host_busy_ms_per_step": mmm(rows["periodic_host"]),
            "periodic_minus_open_us_median": round(1e3 * diff, 2),
            "periodic_over_open_median": round(statistics.median(rows["periodic"]) / statistics.median(rows["open"]), 4)}


def _alternate(ffs, x0, v0, steps, warmup, reps, dt):
    """the protocol of ``bench_pbc`` for force fields that may differ in size: {name: (ms per step rows, host-busy rows)}"""
    from e3_layers_amd.run.md import VelocityVerlet

    mds = {k: VelocityVerlet(ff, torch.ones(x0[k].shape[0]), dt) for k, ff in ffs.items()}
    rows = {k: ([], []) for k in ffs}
    for name, md in mds.items():
        replay_start(md, ffs[name], x0[name], v0[name])
        md.run(warmup, check_every=warmup)
    for _ in range(reps):
        for name, md in mds.items():
            replay_start(md, ffs[name], x0[name], v0[name])
            ms, host = timed(replay_steps(md, ffs[name], steps))
            ffs[name].check()
            rows[name][0].append(ms / steps)
            rows[name][1].append(1e3 * host / steps)
    return rows, mds


def crystal(model_batch, r_max, reps, dev, side=6.0, grid=3, jitter=0.05):
    """A synthetic crystal for ``bench_images``: ``grid``^3 atoms on a jittered grid in a cubic cell of ``side`` (no two atoms, images
    included, closer than side / grid - 2 sqrt(3) jitter side: 1.48 A as shipped), species drawn from ``model_batch``'s, repeated
    ``reps`` times along every axis with the cell scaled to match.  One graph, on ``dev``, without a list."""
    from e3_layers_amd.data.data import Batch

    gen = torch.Generator().manual_seed(5)
    kinds = model_batch["species"].reshape(-1).cpu()
    g = torch.cartesian_prod(*(torch.arange(grid, dtype=torch.float64),) * 3)
    frac = (g + 0.5) / grid + jitter * (2 * torch.rand(g.shape, generator=gen, dtype=torch.float64) - 1)
    species = kinds[torch.randint(0, kinds.numel(), (g.shape[0],), generator=gen)]
    copies = torch.cartesian_prod(*(torch.arange(reps, dtype=torch.float64),) * 3).reshape(-1, 3)
    pos = (side * (frac[None] + copies[:, None]).reshape(-1, 3)).float()
    attrs = {"pos": ("node", "1x1o"), "species": ("node", "1x0e"), "total_energy": ("graph", "1x0e"), "cell": ("graph", "3x1o")}
    sample = {"pos": pos, "species": species.repeat(copies.shape[0]).reshape(-1, 1).long(), "total_energy": torch.zeros(1, 1),
              "cell": (side * reps * torch.eye(3)).reshape(1, 9), "_n_nodes": torch.tensor([[pos.shape[0]]])}
    return Batch.from_data_list([sample], attrs).to(dev)


def bench_images(n_mol, steps, warmup, reps, dt, dev):
    """The all-images builder (csrc/e3k_images.hip) in the replayed step, in the protocol of ``bench_pbc``.  (a) The wide vacuum cell
    of ``bench_pbc`` with images="all" (every range zero: the same list, asserted) against images="minimum".  (b) One narrow cell
    (``crystal``: 27 atoms in a 6 A cube, ranges (1, 1, 1) at the shipped r_max of 5) with images="all" against its 3 x 3 x 3
    supercell (729 atoms, 18 A) with images="minimum": ms per step and per atom-step."""
    from e3_layers_amd.run.md import ReplayedForceField

    model, batch, r_max, x0, v0 = setup(n_mol, dev)
    vac = batch.clone()
    width = vacuum_cell(vac, x0, r_max, dev)
    ffs = {"minimum": ReplayedForceField(model, vac.clone(), r_max), "all": ReplayedForceField(model, vac.clone(), r_max, images="all")}
    if bool(ffs["all"].image_range.any()):
        raise RuntimeError("the vacuum cell has a nonzero image range")
    rows, mds = _alternate(ffs, {k: x0 for k in ffs}, {k: v0 for k in ffs}, steps, warmup, reps, dt)
    lists = {}
    for name, ff in ffs.items():      # the same list at the start
        replay_start(mds[name], ff, x0, v0)
        lists[name] = ff.static["edge_index"][:, :int(ff.n_edges)].clone()
    if not torch.equal(lists["minimum"], lists["all"]):
        raise RuntimeError("the all-images list of the vacuum cell differs from the minimum-image list")
    med = {k: statistics.median(r[0]) for k, r in rows.items()}
    wide = {"molecules": n_mol, "atoms": int(x0.shape[0]), "edges_at_start": int(lists["all"].shape[1]), "cell_width": round(width, 3),
            "e_cap": {k: ff.e_cap for k, ff in ffs.items()}, "steps": steps, "reps": reps, "dt": dt,
            "regrowths": sum(md.regrowths for md in mds.values()), "recaptures": sum(ff.recaptures for ff in ffs.values()),
            "minimum_ms_per_step": mmm(rows["minimum"][0]), "all_ms_per_step": mmm(rows["all"][0]),
            "minimum_host_busy_ms_per_step": mmm(rows["minimum"][1]), "all_host_busy_ms_per_step": mmm(rows["all"][1]),
            "all_minus_minimum_us_median": round(1e3 * (med["all"] - med["minimum"]), 2),
            "all_over_minimum_median": round(med["all"] / med["minimum"], 4)}
    cells = {"cell": crystal(batch, r_max, 1, dev), "supercell": crystal(batch, r_max, 3, dev)}
    ffs = {"cell": ReplayedForceField(model, cells["cell"], r_max, images="all"), "supercell": ReplayedForceField(model, cells["supercell"], r_max)}
    xs = {k: b["pos"].clone() for k, b in cells.items()}
    gen = torch.Generator().manual_seed(2)
    v_cell = 0.2 * torch.randn(xs["cell"].shape, generator=gen).to(dev)
    vs = {"cell": v_cell, "supercell": v_cell.repeat(27, 1)}      # (the supercell moves as 27 copies of the cell)
    rows, mds = _alternate(ffs, xs, vs, steps, warmup, reps, dt)
    for name, ff in ffs.items():
        replay_start(mds[name], ff, xs[name], vs[name])
    edges = {k: int(ff.n_edges) for k, ff in ffs.items()}
    if edges["supercell"] != 27 * edges["cell"]:
        raise RuntimeError(f"the supercell's list has {edges['supercell']} edges, the cell's {edges['cell']}")
    atoms = {k: int(x.shape[0]) for k, x in xs.items()}
    med = {k: statistics.median(r[0]) for k, r in rows.items()}
    narrow = {"atoms": atoms, "edges_at_start": edges, "image_range": ffs["cell"].image_range.cpu().tolist(), "cell_side": 6.0,
              "e_cap": {k: ff.e_cap for k, ff in ffs.items()}, "steps": steps, "reps": reps, "dt": dt,
              "regrowths": sum(md.regrowths for md in mds.values()), "recaptures": sum(ff.recaptures for ff in ffs.values()),
              "cell_ms_per_step": mmm(rows["cell"][0]), "supercell_ms_per_step": mmm(rows["supercell"][0]),
              "cell_us_per_atom_step_median": round(1e3 * med["cell"] / atoms["cell"], 3),
              "supercell_us_per_atom_step_median": round(1e3 * med["supercell"] / atoms["supercell"], 3),
              "supercell_over_cell_ms_median": round(med["supercell"] / med["cell"], 4)}
    return {"wide": wide, "narrow": narrow}


def vacuum_cell(batch, x0, r_max, dev):
    """``batch`` in the cubic vacuum cell of ``bench_pbc`` (in place), and the cell's width"""
    width = float((x0.max(0).values - x0.min(0).values).max()) + 2.0 * r_max + 8.0
    batch.attrs["cell"] = ("graph", "3x1o")
    batch["cell"] = (width * torch.eye(3, device=dev)).reshape(1, 9).repeat(len(batch), 1)
    return width


def single_graph(n_mol: int, dev):
    """``setup`` with the molecules of the batch laid out on a line, 40 A apart, as ONE graph (the generator's molecules have 29 atoms
    at most: this is how it supplies a graph of thousands of atoms).  The virial kernel then walks every edge in one workgroup."""
    from e3_layers_amd.configs import config_energy_force
    from e3_layers_amd.data import computeEdgeIndex
    from e3_layers_amd.data.data import Batch
    from e3_layers_amd.data.synthetic import synth_qm9_list
    from e3_layers_amd.utils import build

    tree = config_energy_force.get_config().model_config
    torch.manual_seed(0)
    model = build(tree).to(dev).eval()
    lst, attrs = synth_qm9_list(4000 + n_mol, n_mol, config_energy_force.SHIFTS, r_max=None)
    pos = torch.cat([s["pos"] + torch.tensor([40.0 * k, 0.0, 0.0]) for k, s in enumerate(lst)])
    one = {"pos": pos, "species": torch.cat([s["species"] for s in lst]), "total_energy": sum(s["total_energy"] for s in lst),
           "_n_nodes": torch.tensor([[pos.shape[0]]])}
    new, _ = computeEdgeIndex(one, dict(attrs), r_max=float(tree.r_max))
    one["edge_index"] = new["edge_index"]
    one.pop("_n_edges", None)
    batch = Batch.from_data_list([one], dict(attrs)).to(dev)
    x0 = batch["pos"].clone()
    v0 = 0.5 * torch.randn(x0.shape, generator=torch.Generator().manual_seed(1)).to(dev)
    return model, batch, float(tree.r_max), x0, v0


def bench_stress(n_mol, steps, warmup, reps, dt, dev, one_graph=False):
    """The replayed step with virial and stress delivered against the same step without, both in the vacuum cell of ``bench_pbc``:
    two models of the same weights (the keys are attributes of the tree), a force field each, the two alternating.  What differs is
    one launch inside the graph (``e3k_virial_edges``) and the elementwise ops of the stress.  ``one_graph``: the molecules as a
    single graph (``single_graph``): the kernel's one-workgroup walk at its longest."""
    from e3_layers_amd.nn import enable_virial
    from e3_layers_amd.run.md import ReplayedForceField, VelocityVerlet, pressure

    make = single_graph if one_graph else setup
    model, batch, r_max, x0, v0 = make(n_mol, dev)
    keyed = enable_virial(make(n_mol, dev)[0])
    width = vacuum_cell(batch, x0, r_max, dev)
    ffs = {"plain": ReplayedForceField(model, batch, r_max),
           "stress": ReplayedForceField(keyed, batch, r_max, virial_key="virial", stress_key="stress")}
    mds = {k: VelocityVerlet(ff, torch.ones(x0.shape[0]), dt) for k, ff in ffs.items()}
    rows = {k: [] for k in ("plain", "stress", "plain_host", "stress_host")}
    for name, md in mds.items():
        replay_start(md, ffs[name], x0, v0)
        md.run(warmup, check_every=warmup)
    for _ in range(reps):
        for name, md in mds.items():
            replay_start(md, ffs[name], x0, v0)
            ms, host = timed(replay_steps(md, ffs[name], steps))
            ffs[name].check()
            rows[name].append(ms / steps)
            rows[name + "_host"].append(1e3 * host / steps)
    diff = statistics.median(rows["stress"]) - statistics.median(rows["plain"])
    ff = ffs["stress"]
    return {"molecules": n_mol, "graphs": len(batch), "atoms": int(x0.shape[0]), "edges_at_end": int(ff.n_edges), "cell_width": round(width, 3),
            "e_cap": ff.e_cap, "steps": steps, "reps": reps, "dt": dt, "regrowths": sum(md.regrowths for md in mds.values()),
            "recaptures": sum(f.recaptures for f in ffs.values()),
            "plain_ms_per_step": mmm(rows["plain"]), "stress_ms_per_step": mmm(rows["stress"]),
            "plain_host_busy_ms_per_step": mmm(rows["plain_host"]), "stress_host_busy_ms_per_step": mmm(rows["stress_host"]),
            "stress_minus_plain_us_median": round(1e3 * diff, 2),
            "stress_over_plain_median": round(statistics.median(rows["stress"]) / statistics.median(rows["plain"]), 4),
            "virial_pressure_at_end": [round(float(p), 6) for p in pressure(ff.virial, torch.zeros(len(batch)), ff.volume)[:4]]}


def bench_npt(n_mol, steps, warmup, reps, dt, kT, gamma, dev, one_graph=False):
    """The replayed Langevin step with virial and stress delivered and ``barostat=Barostat(mode="scr")`` against the same step without
    the barostat, in the protocol of ``bench_stress`` (the vacuum cell, two force fields of the same keyed model, alternating).  What
    differs is ONE launch outside the graph (``e3k_barostat_step``).  p0 = 0 with a small compressibility: the cells breathe by
    parts in 10^5 over the run, so both sides walk the same lists.  ``one_graph``: one workgroup scales every component."""
    from e3_layers_amd.nn import enable_virial
    from e3_layers_amd.run.md import Barostat, Langevin, ReplayedForceField

    make = single_graph if one_graph else setup
    model, batch, r_max, x0, v0 = make(n_mol, dev)
    keyed = enable_virial(model)
    width = vacuum_cell(batch, x0, r_max, dev)
    ffs = {k: ReplayedForceField(keyed, batch, r_max, virial_key="virial", stress_key="stress") for k in ("keys", "npt")}
    first_cell = ffs["npt"].cell.clone()
    baro = Barostat(p0=0.0, compressibility=1e-2, tau=1.0, mode="scr")
    mds = {"keys": Langevin(ffs["keys"], torch.ones(x0.shape[0]), dt, kT, gamma),
           "npt": Langevin(ffs["npt"], torch.ones(x0.shape[0]), dt, kT, gamma, barostat=baro)}
    rows = {k: [] for k in ("keys", "npt", "keys_host", "npt_host")}
    for name, md in mds.items():
        replay_start(md, ffs[name], x0, v0)
        md.run(warmup, check_every=warmup)
    for _ in range(reps):
        for name, md in mds.items():
            if name == "npt":
                ffs[name].set_cell(first_cell)
            replay_start(md, ffs[name], x0, v0)
            ms, host = timed(replay_steps(md, ffs[name], steps))
            ffs[name].check()
            rows[name].append(ms / steps)
            rows[name + "_host"].append(1e3 * host / steps)
    frozen = int(mds["npt"]._baro_counter.item())
    ff = ffs["npt"]
    ff.sync_cell()
    diff = statistics.median(rows["npt"]) - statistics.median(rows["keys"])
    return {"molecules": n_mol, "graphs": len(batch), "atoms": int(x0.shape[0]), "edges_at_end": int(ff.n_edges), "cell_width": round(width, 3),
            "e_cap": ff.e_cap, "steps": steps, "reps": reps, "dt": dt, "kT": kT, "gamma": gamma, "compressibility": baro.compressibility,
            "tau": baro.tau, "p0": baro.p0, "frozen_graph_steps": frozen, "regrowths": sum(md.regrowths for md in mds.values()),
            "recaptures": sum(f.recaptures for f in ffs.values()),
            "relative_cell_change_max": float(((ff.cell - first_cell).flatten(1).norm(dim=1) / first_cell.flatten(1).norm(dim=1)).max()),
            "keys_ms_per_step": mmm(rows["keys"]), "npt_ms_per_step": mmm(rows["npt"]),
            "keys_host_busy_ms_per_step": mmm(rows["keys_host"]), "npt_host_busy_ms_per_step": mmm(rows["npt_host"]),
            "npt_minus_keys_us_median": round(1e3 * diff, 2),
            "npt_over_keys_median": round(statistics.median(rows["npt"]) / statistics.median(rows["keys"]), 4)}


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    host = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), host


def bench(n_mol, steps, warmup, reps, dt, dev):
    from e3_layers_amd.run.md import ReplayedForceField, VelocityVerlet

    model, batch, r_max, x0, v0 = setup(n_mol, dev)
    ff = ReplayedForceField(model, batch, r_max)
    md = VelocityVerlet(ff, torch.ones(x0.shape[0]), dt)
    replay_start(md, ff, x0, v0)
    md.run(warmup, check_every=warmup)            # the public driver, once: warm-up, and the check that the run fits the bucket
    eager_steps(model, batch, r_max, x0, v0, dt, warmup)()
    rows = {"replay": [], "eager": [], "replay_host": [], "eager_host": []}
    for _ in range(reps):
        replay_start(md, ff, x0, v0)
        ms, host = timed(replay_steps(md, ff, steps))
        ff.check()                                # (after the closing event: an overflowed repetition would raise here)
        rows["replay"].append(ms / steps)
        rows["replay_host"].append(1e3 * host / steps)
        ms, host = timed(eager_steps(model, batch, r_max, x0, v0, dt, steps))
        rows["eager"].append(ms / steps)
        rows["eager_host"].append(1e3 * host / steps)

    return {"molecules": n_mol, "atoms": int(x0.shape[0]), "edges_at_start": int(batch["edge_index"].shape[1]), "e_cap": ff.e_cap,
            "n_cap": ff.n_cap, "steps": steps, "reps": reps, "dt": dt, "regrowths": md.regrowths, "recaptures": ff.recaptures,
            "replay_ms_per_step": mmm(rows["replay"]), "eager_ms_per_step": mmm(rows["eager"]),
            "replay_host_busy_ms_per_step": mmm(rows["replay_host"]), "eager_host_busy_ms_per_step": mmm(rows["eager_host"]),
            "speedup_median": round(statistics.median(rows["eager"]) / statistics.median(rows["replay"]), 3)}


def mmm(v):
    return {"min": round(min(v), 4), "median": round(statistics.median(v), 4), "max": round(max(v), 4)}


def bench_langevin(n_mol, steps, warmup, reps, dt, kT, gamma, dev):
    """The thermostatted step against the NVE step of the same build on ONE force field: the two differ in their second launch."""
    from e3_layers_amd.run.md import Langevin, ReplayedForceField, VelocityVerlet

    model, batch, r_max, x0, v0 = setup(n_mol, dev)
    ff = ReplayedForceField(model, batch, r_max)
    mds = {"nve": VelocityVerlet(ff, torch.ones(x0.shape[0]), dt), "langevin": Langevin(ff, torch.ones(x0.shape[0]), dt, kT, gamma, seed=1)}
    rows = {k: [] for k in ("nve", "langevin", "nve_host", "langevin_host")}
    for name, md in mds.items():
        replay_start(md, ff, x0, v0)
        md.run(warmup, check_every=warmup)
    for _ in range(reps):
        for name, md in mds.items():
            replay_start(md, ff, x0, v0)
            ms, host = timed(replay_steps(md, ff, steps))
            ff.check()
            rows[name].append(ms / steps)
            rows[name + "_host"].append(1e3 * host / steps)
    return {"molecules": n_mol, "atoms": int(x0.shape[0]), "e_cap": ff.e_cap, "steps": steps, "reps": reps, "dt": dt, "kT": kT,
            "gamma": gamma, "regrowths": sum(md.regrowths for md in mds.values()), "recaptures": ff.recaptures,
            "nve_ms_per_step": mmm(rows["nve"]), "langevin_ms_per_step": mmm(rows["langevin"]),
            "nve_host_busy_ms_per_step": mmm(rows["nve_host"]), "langevin_host_busy_ms_per_step": mmm(rows["langevin_host"]),
            "langevin_over_nve_median": round(statistics.median(rows["langevin"]) / statistics.median(rows["nve"]), 4)}


def make_fire(ff):
    from e3_layers_amd.run.md import Fire

    return Fire(ff, ftol=1e-9, dt=0.01, dt_max=0.1, maxstep=0.2)      # (a tolerance nothing reaches: every iteration moves every graph)


def bench_fire(n_mol, steps, warmup, reps, dev):
    from e3_layers_amd.run.md import ReplayedForceField

    model, batch, r_max, x0, _ = setup(n_mol, dev)
    ff = ReplayedForceField(model, batch, r_max)
    fire = make_fire(ff)
    ff.pos.copy_(x0)
    fire.run(warmup, check_every=warmup)
    fire.reset()
    eager_fire(model, batch, r_max, x0, fire, warmup)()
    rows = {k: [] for k in ("replay", "eager", "replay_host", "eager_host")}
    for _ in range(reps):
        ff.pos.copy_(x0)
        fire.reset()
        ms, host = timed(replay_fire(fire, ff, steps))
        ff.check()
        rows["replay"].append(ms / steps)
        rows["replay_host"].append(1e3 * host / steps)
        fire.reset()
        ms, host = timed(eager_fire(model, batch, r_max, x0, fire, steps))
        rows["eager"].append(ms / steps)
        rows["eager_host"].append(1e3 * host / steps)
    return {"molecules": n_mol, "atoms": int(x0.shape[0]), "e_cap": ff.e_cap, "iterations": steps, "reps": reps,
            "regrowths": fire.regrowths, "recaptures": ff.recaptures,
            "replay_ms_per_iteration": mmm(rows["replay"]), "eager_ms_per_iteration": mmm(rows["eager"]),
            "replay_host_busy_ms_per_iteration": mmm(rows["replay_host"]), "eager_host_busy_ms_per_iteration": mmm(rows["eager_host"]),
            "speedup_median": round(statistics.median(rows["eager"]) / statistics.median(rows["replay"]), 3)}


def total_calls(path):
    with open(path) as f:
        return sum(int(r["Calls"]) for r in csv.DictReader(f))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--molecules", type=int, nargs="+", default=[32, 64, 1])
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--dt", type=float, default=0.01)
    ap.add_argument("--out", default=None)
    ap.add_argument("--integrator", choices=("nve", "langevin"), default="nve", help="langevin: the thermostatted step against the NVE step")
    ap.add_argument("--fire", action="store_true", help="the FIRE iteration against its eager loop")
    ap.add_argument("--constraints", action="store_true", help="the step with bonds to hydrogen constrained against the plain step")
    ap.add_argument("--pbc", action="store_true", help="the step in a vacuum cell (periodic builder, same edge set) against the open step")
    ap.add_argument("--images", action="store_true", help="images='all': the wide vacuum cell against images='minimum', and a narrow cell "
                                                          "against its 3 x 3 x 3 supercell")
    ap.add_argument("--stress", action="store_true", help="the step with virial and stress delivered against the step without (vacuum cell)")
    ap.add_argument("--one-graph", action="store_true", help="with --stress / --npt: the molecules as ONE graph (the kernels' longest walk)")
    ap.add_argument("--npt", action="store_true", help="the Langevin step with keys on and an scr barostat against the same step without it")
    ap.add_argument("--kT", type=float, default=0.25, help="thermostat temperature in the model's energy units (v0 has variance 0.25)")
    ap.add_argument("--gamma", type=float, default=1.0)
    ap.add_argument("--trace-steps", type=int, default=0, help="run this many replayed steps and nothing else (under rocprofv3)")
    ap.add_argument("--launches", nargs=4, metavar=("CSV_A", "STEPS_A", "CSV_B", "STEPS_B"), default=None)
    args = ap.parse_args()
    if args.launches:
        a, na, b, nb = args.launches
        per_step = (total_calls(b) - total_calls(a)) / (int(nb) - int(na))
        print(json.dumps({"launches_per_replayed_md_step": per_step, "steps": [int(na), int(nb)]}))
        return
    dev = torch.device("cuda:0")
    if args.trace_steps:
        from e3_layers_amd.run.md import Langevin, ReplayedForceField, VelocityVerlet

        model, batch, r_max, x0, v0 = setup(args.molecules[0], dev)
        if args.pbc or args.stress or args.npt or args.images:      # the vacuum cell of bench_pbc
            vacuum_cell(batch, x0, r_max, dev)
        if args.stress or args.npt:
            from e3_layers_amd.nn import enable_virial

            ff = ReplayedForceField(enable_virial(model), batch, r_max, virial_key="virial", stress_key="stress")
        else:
            ff = ReplayedForceField(model, batch, r_max, **({"images": "all"} if args.images else {}))
        if args.fire:
            make_fire(ff).run(args.trace_steps, check_every=args.trace_steps)
        else:
            mass, kw = torch.ones(x0.shape[0]), {}
            if args.constraints:
                con, mass = bonds_to_hydrogen(batch, x0, ff)
                kw = {"constraints": con}
            if args.npt:
                from e3_layers_amd.run.md import Barostat

                kw = {"barostat": Barostat(p0=0.0, compressibility=1e-2, tau=1.0, mode="scr")}
            md = Langevin(ff, mass, args.dt, args.kT, args.gamma, **kw) if args.integrator == "langevin" or args.npt else \
                VelocityVerlet(ff, mass, args.dt, **kw)
            md.v.copy_(v0)
            if args.constraints:
                md.project()
            md.run(args.trace_steps, check_every=args.trace_steps)
        torch.cuda.synchronize()
        print(json.dumps({"trace_steps": args.trace_steps, "molecules": args.molecules[0], "integrator": args.integrator, "fire": args.fire,
                          "constraints": args.constraints, "pbc": args.pbc, "stress": args.stress, "npt": args.npt, "images": args.images}))
        return
    if args.fire:
        workload = "FIRE relaxation with per-graph state on config_energy_force (as shipped), synth_qm9: replayed iteration vs the eager loop"
        results = [bench_fire(n, args.steps, args.warmup, args.reps, dev) for n in args.molecules]
    elif args.constraints:
        workload = ("velocity-Verlet step with the bonds to hydrogen constrained (SHAKE / RATTLE) vs the plain step, both replayed, on "
                    "config_energy_force (as shipped), synth_qm9, masses 1 (H) and 12")
        results = [bench_constraints(n, args.steps, args.warmup, args.reps, args.dt, dev) for n in args.molecules]
    elif args.npt:
        workload = ("Langevin step with virial and stress delivered and an scr barostat (e3k_barostat_step) vs the same step without the "
                    "barostat, both replayed in a cubic vacuum cell, on config_energy_force (as shipped), synth_qm9" +
                    (" laid out as one graph" if args.one_graph else "") + ", unit masses")
        results = [bench_npt(n, args.steps, args.warmup, args.reps, args.dt, args.kT, args.gamma, dev, args.one_graph) for n in args.molecules]
    elif args.stress:
        workload = ("velocity-Verlet step with virial and stress delivered vs the same step without, both replayed in a cubic vacuum cell, on "
                    "config_energy_force (as shipped), synth_qm9" + (" laid out as one graph" if args.one_graph else "") + ", unit masses")
        results = [bench_stress(n, args.steps, args.warmup, args.reps, args.dt, dev, args.one_graph) for n in args.molecules]
    elif args.images:
        workload = ("velocity-Verlet step with the all-images periodic builder, replayed, on config_energy_force (as shipped), unit masses: "
                    "wide = synth_qm9 in the cubic vacuum cell of --pbc, images='all' (ranges zero, identical list) vs images='minimum'; "
                    "narrow = a 27-atom cubic cell of 6 A (ranges 1, 1, 1) with images='all' vs its 3 x 3 x 3 supercell with images='minimum'")
        results = [bench_images(n, args.steps, args.warmup, args.reps, args.dt, dev) for n in args.molecules]
    elif args.pbc:
        workload = ("velocity-Verlet step in a cubic vacuum cell (periodic builder and edge vectors, identical edge set) vs the "
                    "open-boundary step, both replayed, on config_energy_force (as shipped), synth_qm9, unit masses")
        results = [bench_pbc(n, args.steps, args.warmup, args.reps, args.dt, dev) for n in args.molecules]
    elif args.integrator == "langevin":
        workload = "Langevin step vs velocity-Verlet step, both replayed, on config_energy_force (as shipped), synth_qm9, unit masses"
        results = [bench_langevin(n, args.steps, args.warmup, args.reps, args.dt, args.kT, args.gamma, dev) for n in args.molecules]
    else:
        workload = "velocity Verlet on config_energy_force (as shipped), synth_qm9, unit masses"
        results = [bench(n, args.steps, args.warmup, args.reps, args.dt, dev) for n in args.molecules]
    doc = {"workload": workload, "device": torch.cuda.get_device_name(0), "results": results}
    text = json.dumps(doc, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
