#!/usr/bin/env python3
"""Per-step time of velocity-Verlet MD on config_energy_force: the replayed force field (run/md.py: one HIP graph per force
evaluation, the neighbour list rebuilt inside it, two integrator launches beside it) against the eager loop the package offered before it
(computeEdgeIndex on the device + the eager model call + an element-wise torch integrator), on the same start.

    python tools/md_bench.py --molecules 32 64 1 --steps 200 --out profiles/md_replay.json
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


def replay_start(md, ff, x0, v0):
    """Puts the replayed run on the start (verified forces there): outside the timed region."""
    ff.pos.copy_(x0)
    md.v.copy_(v0)
    md._forces = None
    _, md._forces = md._verified_forces()


def replay_steps(md, ff, n_steps):
    """The launches of ``VelocityVerlet.run``'s inner loop, and nothing else: ``run`` closes a chunk with ``check()``, a host
    synchronisation that would sit between the two events -- the caller checks after the closing event instead."""
    from e3_layers_amd.run import md as M

    n_graphs = ff.node_ptr.numel() - 1
    pot = torch.zeros(n_steps, n_graphs, device=ff.dev)
    kin = torch.zeros_like(pot)
    forces = md._forces

    def loop():
        nonlocal forces
        t0 = time.perf_counter()
        for i in range(n_steps):
            M._drift(ff.pos, md.v, forces, md.mass, md.dt)
            energy, forces = ff.evaluate()
            M._kick(md.v, forces, md.mass, ff.node_ptr, md.dt, kin[i], energy, pot[i])
        return time.perf_counter() - t0

    return loop


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

    def mmm(v):
        return {"min": round(min(v), 4), "median": round(statistics.median(v), 4), "max": round(max(v), 4)}

    return {"molecules": n_mol, "atoms": int(x0.shape[0]), "edges_at_start": int(batch["edge_index"].shape[1]), "e_cap": ff.e_cap,
            "n_cap": ff.n_cap, "steps": steps, "reps": reps, "dt": dt, "regrowths": md.regrowths, "recaptures": ff.recaptures,
            "replay_ms_per_step": mmm(rows["replay"]), "eager_ms_per_step": mmm(rows["eager"]),
            "replay_host_busy_ms_per_step": mmm(rows["replay_host"]), "eager_host_busy_ms_per_step": mmm(rows["eager_host"]),
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
        from e3_layers_amd.run.md import ReplayedForceField, VelocityVerlet

        model, batch, r_max, x0, v0 = setup(args.molecules[0], dev)
        ff = ReplayedForceField(model, batch, r_max)
        md = VelocityVerlet(ff, torch.ones(x0.shape[0]), args.dt)
        md.v.copy_(v0)
        md.run(args.trace_steps, check_every=args.trace_steps)
        torch.cuda.synchronize()
        print(json.dumps({"trace_steps": args.trace_steps, "molecules": args.molecules[0]}))
        return
    results = [bench(n, args.steps, args.warmup, args.reps, args.dt, dev) for n in args.molecules]
    doc = {"workload": "velocity Verlet on config_energy_force (as shipped), synth_qm9, unit masses", "device": torch.cuda.get_device_name(0),
           "results": results}
    text = json.dumps(doc, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
