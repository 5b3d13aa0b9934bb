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

    Fire(ff, ftol=1e-3).run(500)              # relax first: every molecule at its own pace, the graph + one launch per iteration
    md = Langevin(ff, masses, dt=0.5, kT=0.025, gamma=0.1, seed=7)      # the graph + two launches per step, as NVE
    md.thermalize()                           # Maxwell-Boltzmann velocities at kT
"""
from __future__ import annotations

import math
from typing import Optional

import torch

from ..backend import lib as L
from ..backend.graph import EdgeCapacityExceeded
from ..data.compute_edge import check_edge_capacity, computeEdgeIndex, computeEdgeIndexCapped, normal_draw
from .graph_step import GHOST_DEGREE, CapturedStep, bucket_capacity, pad_batch

__all__ = ["EdgeCapacityExceeded", "ReplayedForceField", "VelocityVerlet", "Langevin", "Fire"]

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
# Integrators and the minimiser.  The per-step updates are kernels of csrc/e3k_nlist.hip on device tensors; host tensors (a stub
# force field in the rollback tests, the float64 oracle loops) take the same arithmetic in torch.
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
    _kick_host(v, f, mass, node_ptr, dt, kinetic, energy, potential)


def _kick_host(v, f, mass, node_ptr, dt: float, kinetic, energy, potential) -> None:
    if f is not None:
        v.add_(f / mass[:, None], alpha=0.5 * dt)
    if potential is not None:
        potential.copy_(energy)
    if kinetic is not None:
        per_node = 0.5 * mass * (v * v).sum(1)
        for g in range(node_ptr.numel() - 1):
            kinetic[g] = per_node[int(node_ptr[g]):int(node_ptr[g + 1])].sum()


THERMOSTAT_WORD, THERMALIZE_WORD = 0, 4      # first hash word of a step's draw and of thermalize()'s: the streams never coincide


def _kick_langevin(v, f, mass, node_ptr, dt: float, c: float, s: float, seed: int, draw: int, word0: int, kinetic, energy=None,
                   potential=None) -> None:
    """``v <- c v + (s / sqrt(m)) xi``, then ``_kick`` (``f`` None: no kick, the records only).  ``xi`` is
    ``normal_draw(seed, draw, node, word0 + component)``: counter-based, the same bits whenever the same step is done again."""
    if v.is_cuda:
        L.check(L.load().e3k_md_kick_langevin(L.ptr(v), L.ptr(f), L.ptr(mass), L.ptr(node_ptr), node_ptr.numel() - 1, v.shape[0],
                                              float(dt), float(c), float(s), seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF,
                                              draw & 0xFFFFFFFF, int(word0), L.ptr(kinetic), L.ptr(energy), L.ptr(potential),
                                              L.stream_ptr()), "e3k_md_kick_langevin")
        return
    node = torch.arange(v.shape[0], dtype=torch.int64)[:, None]
    xi = normal_draw(seed, draw, node, word0 + torch.arange(3, dtype=torch.int64)[None, :], v.dtype)
    v.mul_(c).add_((s / torch.sqrt(mass))[:, None] * xi)
    _kick_host(v, f, mass, node_ptr, dt, kinetic, energy, potential)


def _fire_step(x, v, f, node_ptr, state, fire: "Fire", energy=None, energy_record=None, fmax_record=None) -> None:
    """One FIRE iteration on every graph with the graph's own row of ``state`` [G, 4] = (dt, alpha, n_pos, fmax): the rule in
    ``Fire``'s docstring (``e3k_fire_step``; the torch path walks the graphs one by one with the same arithmetic)."""
    n_graphs = node_ptr.numel() - 1
    if x.is_cuda:
        L.check(L.load().e3k_fire_step(L.ptr(x), L.ptr(v), L.ptr(f), L.ptr(node_ptr), n_graphs, x.shape[0], L.ptr(state), fire.ftol,
                                       fire.dt_max, fire.maxstep, fire.n_min, fire.f_inc, fire.f_dec, fire.alpha, fire.f_alpha,
                                       L.ptr(energy), L.ptr(energy_record), L.ptr(fmax_record), L.stream_ptr()), "e3k_fire_step")
        return
    _fire_step_torch(x, v, f, node_ptr, state, fire, energy, energy_record, fmax_record)


def _fire_step_torch(x, v, f, node_ptr, state, fire, energy=None, energy_record=None, fmax_record=None) -> None:
    """The torch path: graph by graph, every branch decided on the host (on device tensors that is a read-back per decision --
    the eager loop ``tools/md_bench.py --fire`` measures the kernel against)."""
    bounds = node_ptr.tolist()
    for g in range(len(bounds) - 1):
        a, b = bounds[g], bounds[g + 1]
        xg, vg, fg = x[a:b], v[a:b], f[a:b]
        dt, alpha, n_pos = state[g, 0].clone(), state[g, 1].clone(), state[g, 2].clone()
        f2 = (fg * fg).sum(1)
        fmax = torch.sqrt(f2.max()) if b > a else f2.sum()
        if bool(fmax < fire.ftol):
            vg.zero_()
        else:
            if bool((fg * vg).sum() < 0):
                vg.zero_()
                dt, alpha, n_pos = dt * fire.f_dec, torch.full_like(alpha, fire.alpha), torch.zeros_like(n_pos)
            else:
                ff = f2.sum()
                mix = alpha * (torch.sqrt((vg * vg).sum()) / torch.sqrt(ff)) if bool(ff > 0) else torch.zeros_like(alpha)
                vg.mul_(1.0 - alpha).add_(mix * fg)
                if bool(n_pos > fire.n_min):
                    dt, alpha = torch.clamp(dt * fire.f_inc, max=fire.dt_max), alpha * fire.f_alpha
                n_pos = n_pos + 1
            vg.add_(dt * fg)
            norm_dr = dt * torch.sqrt((vg * vg).sum())
            move = dt * (fire.maxstep / norm_dr) if bool(norm_dr > fire.maxstep) else dt
            xg.add_(move * vg)
        state[g, 0], state[g, 1], state[g, 2], state[g, 3] = dt, alpha, n_pos, fmax
        if energy_record is not None:
            energy_record[g] = energy[g]
        if fmax_record is not None:
            fmax_record[g] = fmax


class _ChunkedDriver:
    """What the integrators and the minimiser share: iterations are enqueued in chunks of ``check_every``; the list's capacity is
    checked once per chunk (the one synchronisation); a chunk that overflowed is thrown away -- positions and the driver's own
    tensors go back to the last verified iteration, the capacity grows, the chunk runs again -- so an overflowed iteration never
    reaches the caller.  A subclass gives ``_tensors()`` (what a chunk changes besides the positions), ``_step(i, k)`` (enqueue
    iteration ``i`` of this run, number ``k`` since the driver was made) and, where it carries something between chunks,
    ``_begin_chunk`` / ``_commit_chunk`` / ``_after_restore``; ``_finished()`` may end the run after a verified chunk."""

    MAX_REGROWTHS_PER_CHUNK = 8

    def __init__(self, ff, grow_factor: float):
        self.ff, self.grow_factor = ff, float(grow_factor)
        self.regrowths = 0
        self.restores = 0        # how often a snapshot was put back (tests)
        self.steps_done = 0

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

    def _begin_chunk(self) -> None:
        pass

    def _commit_chunk(self) -> None:
        pass

    def _after_restore(self) -> None:
        pass

    def _finished(self) -> bool:
        return False

    def _run_chunks(self, n_steps: int, check_every: int) -> int:
        """Up to ``n_steps`` iterations; returns how many were done (fewer only when ``_finished()`` said so)."""
        done = 0
        while done < n_steps:
            chunk = min(check_every, n_steps - done)
            snap_x, snaps = self.x.clone(), [t.clone() for t in self._tensors()]
            for attempt in range(self.MAX_REGROWTHS_PER_CHUNK + 1):
                self._begin_chunk()
                for i in range(done, done + chunk):
                    self._step(i, self.steps_done + i - done)
                try:
                    self.ff.check()
                    self._commit_chunk()
                    break
                except EdgeCapacityExceeded:
                    if attempt == self.MAX_REGROWTHS_PER_CHUNK:
                        raise
                    # back to the last verified iteration: grow at ITS positions, redo the chunk
                    self._regrow(snap_x)
                    for t, snap in zip(self._tensors(), snaps):
                        t.copy_(snap)
                    self.restores += 1
                    self._after_restore()
            done += chunk
            self.steps_done += chunk
            if self._finished():
                break
        return done


class VelocityVerlet(_ChunkedDriver):
    """``ff``: a ``ReplayedForceField`` (or anything with ``pos``, ``node_ptr``, ``evaluate()``, ``check()``, ``grow()``);
    ``masses`` [N]; ``dt`` in the model's units.  ``v`` [N, 3] starts at zero: set it, or ``thermalize``, before ``run``.

    One step = drift kernel, the force field's graph, kick kernel (which also files the step's potential and kinetic energies:
    two launches outside the graph).  Every ``check_every`` steps the list's capacity is checked
    (the one synchronisation); a chunk that overflowed is thrown away -- positions, velocities and records go back to the last
    verified step, the capacity grows, the chunk runs again -- so an overflowed step never reaches the caller."""

    def __init__(self, ff, masses, dt: float, grow_factor: float = 1.5, seed: int = 0):
        super().__init__(ff, grow_factor)
        self.dt, self.seed = float(dt), int(seed)
        x = ff.pos
        self.mass = masses.to(device=x.device, dtype=x.dtype).reshape(-1).contiguous()
        if self.mass.numel() != x.shape[0]:
            raise ValueError(f"{self.mass.numel()} masses for {x.shape[0]} atoms")
        self.v = torch.zeros_like(x).contiguous()
        self.thermalizations = 0      # the draw counter of thermalize()
        self._forces = None      # forces at the present positions (the graph's static tensor), None: not evaluated yet

    def thermalize(self, kT: Optional[float] = None) -> None:
        """Maxwell-Boltzmann velocities at ``kT`` (the model's energy units; default: the thermostat's, where there is one):
        ``v = sqrt(kT / m) xi``, one launch.  The draws are ``seed``'s stream of ``thermalize`` words with a counter of their own,
        so a call never repeats a step's noise or an earlier call's."""
        kT = getattr(self, "kT", None) if kT is None else float(kT)
        if kT is None or kT < 0:
            raise ValueError("thermalize() needs kT >= 0")
        _kick_langevin(self.v, None, self.mass, self.ff.node_ptr, 0.0, 0.0, kT ** 0.5, self.seed, self.thermalizations, THERMALIZE_WORD,
                       None)
        self.thermalizations += 1

    def _tensors(self):
        return (self.v,)

    def _begin_chunk(self) -> None:
        self._chunk_forces = self._forces

    def _commit_chunk(self) -> None:
        self._forces = self._chunk_forces

    def _after_restore(self) -> None:
        _, self._forces = self._verified_forces()      # the forces at the snapshot's positions, on the grown list

    def _second_half(self, k: int, forces, energy, kinetic, potential) -> None:
        _kick(self.v, forces, self.mass, self.ff.node_ptr, self.dt, kinetic, energy, potential)

    def _step(self, i: int, k: int) -> None:
        _drift(self.x, self.v, self._chunk_forces, self.mass, self.dt)
        energy, self._chunk_forces = self.ff.evaluate()
        self._second_half(k, self._chunk_forces, energy, self._kin[i], self._pot[i])

    def run(self, n_steps: int, check_every: int = 50):
        """``n_steps`` steps; returns {"potential": [n_steps, G], "kinetic": [n_steps, G]} (per graph, after every step); the state
        is ``self.x``, ``self.v``."""
        if n_steps < 0 or check_every < 1:
            raise ValueError("n_steps >= 0 and check_every >= 1")
        if self._forces is None:
            _, self._forces = self._verified_forces()
        n_graphs = self.ff.node_ptr.numel() - 1
        self._pot = torch.zeros(n_steps, n_graphs, dtype=self.v.dtype, device=self.v.device)
        self._kin = torch.zeros_like(self._pot)
        self._run_chunks(n_steps, check_every)
        return {"potential": self._pot, "kinetic": self._kin}


class Langevin(VelocityVerlet):
    """Velocity Verlet with a Langevin thermostat at ``kT`` (in the MODEL's energy units: no Boltzmann constant is guessed) and
    friction ``gamma`` (inverse time units), in the order of the reference notebook's integrator: half kick + drift, forces, friction
    and noise, half kick -- still the graph + two launches, the second being ``e3k_md_kick_langevin``:

        v <- c v + sqrt((1 - c^2) kT / m) xi,    c = exp(-gamma dt)

    This is the exact Ornstein-Uhlenbeck step, not torchmd's first-order ``v (1 - gamma dt) + sqrt(2 gamma dt kT / m) xi``; the two
    agree to O((gamma dt)^2), the exact form is stable for any ``gamma dt`` and is the plain kick at ``gamma = 0``.

    ``xi`` is counter-based (``data/compute_edge.normal_draw``) with the ABSOLUTE step number as its draw index: a chunk that is
    rolled back and redone after an overflow sees the same noise, and a trajectory does not depend on ``check_every``."""

    def __init__(self, ff, masses, dt: float, kT: float, gamma: float, seed: int = 0, grow_factor: float = 1.5):
        if kT < 0 or gamma < 0:
            raise ValueError("kT >= 0 and gamma >= 0")
        super().__init__(ff, masses, dt, grow_factor, seed)
        self.kT, self.gamma = float(kT), float(gamma)
        self.c = math.exp(-self.gamma * self.dt)                    # (float64 on the host; the kernel takes them as floats)
        self.s = math.sqrt(-math.expm1(-2.0 * self.gamma * self.dt) * self.kT)

    def _second_half(self, k: int, forces, energy, kinetic, potential) -> None:
        _kick_langevin(self.v, forces, self.mass, self.ff.node_ptr, self.dt, self.c, self.s, self.seed, k, THERMOSTAT_WORD, kinetic,
                       energy, potential)


class Fire(_ChunkedDriver):
    """FIRE relaxation (Bitzek et al., PRL 97, 170201, with the step rule of ASE's optimiser) in which EVERY GRAPH carries its own
    adaptive state -- ``state`` [G, 4] = (dt, alpha, n_pos, fmax) on the device -- so a batch of molecules relaxes at each
    molecule's pace with nothing read back.  One iteration = the force field's graph + ONE launch (``e3k_fire_step``).  Per graph,
    with P = sum f.v and fmax = max_i |f_i|:

    * fmax < ``ftol``: v <- 0, the positions are not touched.  The graph is frozen: graphs share no edges, so its forces cannot
      change; it goes on being evaluated and stays frozen.
    * otherwise P < 0: v <- 0, dt <- dt ``f_dec``, alpha <- ``alpha``, n_pos <- 0.
    * otherwise: v <- (1 - alpha) v + alpha |v| f / |f|; if n_pos > ``n_min``: dt <- min(dt ``f_inc``, ``dt_max``),
      alpha <- alpha ``f_alpha``; n_pos <- n_pos + 1.  P = 0 counts as downhill (ASE asks P > 0), so that the first iteration from
      v = 0 does not halve dt.
    * then v <- v + dt f (unit masses: a minimiser has no physical time), dr = dt v scaled to ``maxstep`` where its norm over the
      graph exceeds it, x <- x + dr.

    Every ``check_every`` iterations the host synchronises once: the capacity check, and the state read back -- the run stops when
    every graph's fmax < ``ftol``.  An overflowed chunk is rolled back and redone as in the integrators."""

    def __init__(self, ff, ftol: float, dt: float = 0.05, dt_max: float = 0.5, maxstep: float = 0.2, n_min: int = 5,
                 f_inc: float = 1.1, f_dec: float = 0.5, alpha: float = 0.1, f_alpha: float = 0.99, grow_factor: float = 1.5):
        if not (ftol > 0 and 0 < dt <= dt_max and maxstep > 0 and n_min >= 0):
            raise ValueError("ftol > 0, 0 < dt <= dt_max, maxstep > 0 and n_min >= 0")
        super().__init__(ff, grow_factor)
        self.ftol, self.dt, self.dt_max, self.maxstep, self.n_min = float(ftol), float(dt), float(dt_max), float(maxstep), int(n_min)
        self.f_inc, self.f_dec, self.alpha, self.f_alpha = float(f_inc), float(f_dec), float(alpha), float(f_alpha)
        x = ff.pos
        n_graphs = ff.node_ptr.numel() - 1
        self.v = torch.zeros_like(x).contiguous()
        self.state = torch.zeros(n_graphs, 4, dtype=x.dtype, device=x.device)
        self.reset()

    def reset(self) -> None:
        """Back to rest with the starting step sizes (a new relaxation from other positions)."""
        self.v.zero_()
        self.state.copy_(torch.tensor([self.dt, self.alpha, 0.0, float("inf")], dtype=self.state.dtype).expand_as(self.state))

    def _tensors(self):
        return (self.v, self.state)

    def _step(self, i: int, k: int) -> None:
        energy, forces = self.ff.evaluate()
        _fire_step(self.x, self.v, forces, self.ff.node_ptr, self.state, self, energy, self._energy[i], self._fmax[i])

    def _finished(self) -> bool:
        return bool((self.state[:, 3] < self.ftol).all())      # (after the chunk's check(): the device is idle, one small copy)

    def run(self, max_iter: int, check_every: int = 50):
        """At most ``max_iter`` iterations; returns {"energy": [iterations, G], "fmax": [iterations, G]} (each graph's energy and
        largest force at the positions BEFORE the iteration's move), "converged": bool [G], "iterations": int}; the state is
        ``self.x``."""
        if max_iter < 0 or check_every < 1:
            raise ValueError("max_iter >= 0 and check_every >= 1")
        n_graphs = self.ff.node_ptr.numel() - 1
        self._energy = torch.zeros(max_iter, n_graphs, dtype=self.v.dtype, device=self.v.device)
        self._fmax = torch.zeros_like(self._energy)
        done = self._run_chunks(max_iter, check_every)
        return {"energy": self._energy[:done], "fmax": self._fmax[:done], "converged": self.state[:, 3] < self.ftol, "iterations": done}
