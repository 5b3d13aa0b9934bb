"""Replayed force evaluation and velocity-Verlet molecular dynamics (the use of a trained ``config_energy_force`` model that the
reference drives from ``torchMD.ipynb``: call the model on moved positions, integrate, repeat).

A force evaluation is forward + one backward through the force block: a hundred-odd launches of 5-100 us, host-bound when issued
eagerly, and the neighbour list changes as the atoms move.  ``ReplayedForceField`` pads the batch once to a bucket
(``run/graph_step.pad_batch``), and captures ``computeEdgeIndexCapped -> model`` in ONE HIP graph (``CapturedStep``: guards,
re-capture on a knot-table veto and flag polling come with it): the list is rebuilt on the device inside the graph, into a buffer of
fixed capacity (``csrc/e3k_nlist.hip``).  More edges than the capacity is a REPORTED condition -- ``check()`` raises
``EdgeCapacityExceeded``, ``grow()`` re-pads to a larger bucket and captures again.

    ff = ReplayedForceField(model, batch, r_max=5.0)
    energy, forces = ff(pos)                  # [G], [N, 3]: static tensors, overwritten by the next call
    ff.check()                                # synchronises; raises if the list overflowed since the last check

    md = VelocityVerlet(ff, masses, dt=0.5)
    out = md.run(1000, check_every=50)        # rolls a chunk back and grows the capacity when the list overflows
"""
from __future__ import annotations

from typing import Optional

import torch

from ..backend import lib as L
from ..backend.graph import EdgeCapacityExceeded
from ..data.compute_edge import check_edge_capacity, computeEdgeIndex, computeEdgeIndexCapped
from .graph_step import GHOST_DEGREE, CapturedStep, bucket_capacity, pad_batch

__all__ = ["EdgeCapacityExceeded", "ReplayedForceField", "VelocityVerlet"]

_EDGE_KEYS = ("edge_index", "edge_vector", "edge_length", "_n_edges", "_edge_segment")


class ReplayedForceField:
    """``model``: a built ``GradientOutput`` tree in eval mode (``config_energy_force``); ``batch``: an unpadded device batch.

    ``edge_slack``: the edge capacity is the present edge count times this, rounded up to a multiple of ``edge_multiple`` (the
    bucket grid of ``bucket_capacity``)."""

    def __init__(self, model, batch, r_max: float, energy_key: str = "energy", forces_key: str = "forces", edge_slack: float = 1.5,
                 key: str = "pos", warmup: int = 3, edge_multiple: int = 1024):
        if not batch[key].is_cuda:
            raise RuntimeError("ReplayedForceField needs a device batch: there is no CPU fallback for graph replay")
        if edge_slack < 1.0:
            raise ValueError("edge_slack must be >= 1")
        carried = [k for k, v in batch.attrs.items() if v[0] == "edge" and k in batch and k not in _EDGE_KEYS]
        if carried:
            raise ValueError(f"the edge attributes {carried} cannot follow a rebuilt neighbour list")
        self.model, self.r_max, self.key = model, float(r_max), key
        self.energy_key, self.forces_key = energy_key, forces_key
        self.edge_slack, self.warmup, self.edge_multiple = float(edge_slack), warmup, int(edge_multiple)
        self.dev = batch[key].device
        self._base = batch.clone()
        for k in _EDGE_KEYS:
            self._base.pop(k)
        self.n_real = int(batch[key].shape[0])
        self.n_graphs = len(batch)
        n = self._base["_n_nodes"].reshape(-1)
        self.node_ptr = torch.zeros(self.n_graphs + 1, dtype=torch.int64, device=self.dev)      # of the real graphs (the integrator's)
        self.node_ptr[1:] = torch.cumsum(n, 0)
        self.e_cap = 0
        self._overflow = False
        self.valid = False       # do the static outputs hold the evaluation of the positions in ``self.pos``?
        self._build(self._base[key], 0)

    # ---- capture ----------------------------------------------------------------------------------------------------
    def _build(self, pos, e_min: int):
        base = self._base.clone()
        base[self.key] = pos.detach().to(torch.float32).clone()
        new, attrs = computeEdgeIndex(base.data, base.attrs, r_max=self.r_max, key=self.key)      # eager: the sizes go to the host once
        base.attrs.update(attrs)
        base.update(new)
        n, e = self.n_real, int(new["edge_index"].shape[1])
        want = max(int(e * self.edge_slack) + 1, int(e_min))
        _, e_cap = bucket_capacity([(n, want)], edge_multiple=self.edge_multiple)
        n_cap = n + max(2, -(-(e_cap - e) // GHOST_DEGREE))      # ghost nodes for the tail as it is NOW (about GHOST_DEGREE edges each)
        n_cap = -(-n_cap // 32) * 32
        static = pad_batch(base, n_cap, e_cap)
        static["_nlist_state"] = torch.zeros(2, dtype=torch.int64, device=self.dev)
        static[self.key] = static[self.key].contiguous()
        self.static, self.n_cap, self.e_cap = static, n_cap, e_cap
        self.pos = static[self.key][:self.n_real]      # the real nodes' positions: write here, then evaluate()
        model = self.model

        def evaluate():
            work = static.view()
            computeEdgeIndexCapped(work.data, work.attrs, r_max=self.r_max, key=self.key)
            out = model(work)
            return out[self.energy_key].reshape(-1)[:self.n_graphs], out[self.forces_key][:self.n_real]

        self.captured = CapturedStep(evaluate, warmup=self.warmup, device=self.dev)
        self.valid = False
        self._check_outputs(self.captured.out)

    @staticmethod
    def _check_outputs(out) -> None:
        # the integrator's kernels read these through raw pointers: dense fp32 rows or nothing (a slice of the leading rows of a
        # contiguous model output is contiguous; anything else is refused here, once per capture, not read wrongly)
        for name, t in zip(("energy", "forces"), out):
            if t.dtype != torch.float32 or not t.is_contiguous():
                raise TypeError(f"the captured {name} output is {t.dtype}, contiguous={t.is_contiguous()}: the MD kernels need "
                                "contiguous float32")

    @property
    def recaptures(self) -> int:
        return self.captured.recaptures

    @property
    def n_edges(self) -> torch.Tensor:
        """Device int64 scalar: the real edges the last evaluation's list needed (more than ``e_cap``: it overflowed)."""
        return self.static["_nlist_state"][0]

    # ---- evaluation -------------------------------------------------------------------------------------------------
    def evaluate(self):
        """Energy [G] and forces [N, 3] at the positions in ``self.pos`` (static tensors of the graph).

        ``CapturedStep`` raises ``EdgeCapacityExceeded`` when an EARLIER replay's flag copy arrives, which can be before this
        call's replay was enqueued (a stale step re-captures first; the deferred flag is read first).  The overflow is remembered
        for ``check()``, and the static tensors are returned marked ``valid = False``: they hold an earlier evaluation, possibly
        of other positions.  Nothing may be taken from them before ``check()`` -- which raises in exactly this case."""
        try:
            out = self.captured()
            if out is not self.captured.out:      # a re-capture replaced the static outputs
                self._check_outputs(out)
            self.valid = True
            return out
        except EdgeCapacityExceeded:
            self._overflow = True
            self.valid = False
            return self.captured.out

    def __call__(self, pos):
        self.pos.copy_(pos)
        return self.evaluate()

    def check(self) -> None:
        """Synchronises; raises ``EdgeCapacityExceeded`` if a list overflowed (or an evaluation was cut short by an earlier
        overflow's report) since the last check, and clears the condition."""
        over, self._overflow = self._overflow, False
        try:
            check_edge_capacity(self.static["_nlist_state"])
        except EdgeCapacityExceeded:
            over = True
        if over:
            raise EdgeCapacityExceeded(f"the neighbour list outgrew its capacity of {self.e_cap} edges since the last check: grow() and "
                                       "redo the steps since then")

    def grow(self, factor: float = 1.5, pos=None) -> None:
        """Re-pads to a bucket of at least ``factor`` times the present capacity (and the slack over the list that ``pos`` --
        default: the positions in ``self.pos`` -- needs) and captures again.  After an overflow the positions in ``self.pos`` were
        integrated on a cut list: pass the last verified ones.  ``self.pos`` is a new tensor afterwards, holding ``pos``."""
        if factor <= 1.0:
            raise ValueError("grow() needs a factor > 1")
        torch.cuda.synchronize(self.dev)
        self._build((self.pos if pos is None else pos).clone(), int(self.e_cap * factor) + 1)


# ---------------------------------------------------------------------------------------------------------------------
# Velocity Verlet.  The two half steps are kernels of csrc/e3k_nlist.hip on device tensors; host tensors (a stub force field in
# the rollback tests) take the same arithmetic in torch.
# ---------------------------------------------------------------------------------------------------------------------
def _drift(x, v, f, mass, dt: float) -> None:
    if x.is_cuda:
        L.check(L.load().e3k_md_drift(L.ptr(x), L.ptr(v), L.ptr(f), L.ptr(mass), x.shape[0], float(dt), L.stream_ptr()), "e3k_md_drift")
        return
    v.add_(f / mass[:, None], alpha=0.5 * dt)
    x.add_(v, alpha=dt)


def _kick(v, f, mass, node_ptr, dt: float, kinetic, energy=None, potential=None) -> None:
    """``kinetic`` [G] takes the graphs' kinetic energies and ``potential`` [G] a copy of ``energy`` [G] (the force field's static
    output) in the same launch; None: not wanted."""
    if v.is_cuda:
        L.check(L.load().e3k_md_kick(L.ptr(v), L.ptr(f), L.ptr(mass), L.ptr(node_ptr), node_ptr.numel() - 1, v.shape[0], float(dt),
                                     L.ptr(kinetic), L.ptr(energy), L.ptr(potential), L.stream_ptr()), "e3k_md_kick")
        return
    v.add_(f / mass[:, None], alpha=0.5 * dt)
    if potential is not None:
        potential.copy_(energy)
    if kinetic is not None:
        per_node = 0.5 * mass * (v * v).sum(1)
        for g in range(node_ptr.numel() - 1):
            kinetic[g] = per_node[int(node_ptr[g]):int(node_ptr[g + 1])].sum()


class VelocityVerlet:
    """``ff``: a ``ReplayedForceField`` (or anything with ``pos``, ``node_ptr``, ``evaluate()``, ``check()``, ``grow()``);
    ``masses`` [N]; ``dt`` in the model's units.  ``v`` [N, 3] starts at zero: set it before ``run``.

    One step = drift kernel, the force field's graph, kick kernel (which also files the step's potential and kinetic energies:
    two launches outside the graph).  Every ``check_every`` steps the list's capacity is checked
    (the one synchronisation); a chunk that overflowed is thrown away -- positions, velocities and records go back to the last
    verified step, the capacity grows, the chunk runs again -- so an overflowed step never reaches the caller."""

    MAX_REGROWTHS_PER_CHUNK = 8

    def __init__(self, ff, masses, dt: float, grow_factor: float = 1.5):
        self.ff, self.dt, self.grow_factor = ff, float(dt), float(grow_factor)
        x = ff.pos
        self.mass = masses.to(device=x.device, dtype=x.dtype).reshape(-1).contiguous()
        if self.mass.numel() != x.shape[0]:
            raise ValueError(f"{self.mass.numel()} masses for {x.shape[0]} atoms")
        self.v = torch.zeros_like(x).contiguous()
        self.regrowths = 0
        self.restores = 0        # how often a snapshot was put back (tests)
        self.steps_done = 0
        self._forces = None      # forces at the present positions (the graph's static tensor), None: not evaluated yet

    @property
    def x(self):
        return self.ff.pos

    def _verified_forces(self):
        """Forces at the present positions on a list that is known to fit."""
        for _ in range(self.MAX_REGROWTHS_PER_CHUNK + 1):
            energy, forces = self.ff.evaluate()
            try:
                self.ff.check()
                return energy, forces
            except EdgeCapacityExceeded:
                self._regrow(self.x.clone())      # (these positions are sound: the overflow is of the list AT them)
        raise EdgeCapacityExceeded("the neighbour list still overflows after repeated growth")

    def _regrow(self, x_keep) -> None:
        """Grows the capacity for the list at ``x_keep`` (never at the positions an overflowed chunk left behind: those were
        integrated on a cut list and can ask for any capacity) and leaves ``x_keep`` as the present positions."""
        self.ff.pos.copy_(x_keep)
        self.ff.grow(self.grow_factor)
        self.regrowths += 1
        self.ff.pos.copy_(x_keep)

    def run(self, n_steps: int, check_every: int = 50):
        """``n_steps`` steps; returns {"potential": [n_steps, G], "kinetic": [n_steps, G]} (per graph, after every step); the state
        is ``self.x``, ``self.v``."""
        if n_steps < 0 or check_every < 1:
            raise ValueError("n_steps >= 0 and check_every >= 1")
        if self._forces is None:
            _, self._forces = self._verified_forces()
        n_graphs = self.ff.node_ptr.numel() - 1
        pot = torch.zeros(n_steps, n_graphs, dtype=self.v.dtype, device=self.v.device)
        kin = torch.zeros_like(pot)
        done = 0
        while done < n_steps:
            chunk = min(check_every, n_steps - done)
            snap_x, snap_v = self.x.clone(), self.v.clone()
            for attempt in range(self.MAX_REGROWTHS_PER_CHUNK + 1):
                forces = self._forces
                for i in range(done, done + chunk):
                    _drift(self.x, self.v, forces, self.mass, self.dt)
                    energy, forces = self.ff.evaluate()
                    _kick(self.v, forces, self.mass, self.ff.node_ptr, self.dt, kin[i], energy, pot[i])
                try:
                    self.ff.check()
                    self._forces = forces
                    break
                except EdgeCapacityExceeded:
                    if attempt == self.MAX_REGROWTHS_PER_CHUNK:
                        raise
                    # back to the last verified step: grow at ITS positions, take the forces there again, redo the chunk
                    self._regrow(snap_x)
                    self.v.copy_(snap_v)
                    self.restores += 1
                    _, self._forces = self._verified_forces()
            done += chunk
            self.steps_done += chunk
        return {"potential": pot, "kinetic": kin}
