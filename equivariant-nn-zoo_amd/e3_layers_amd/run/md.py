"""Replayed force evaluation and velocity-Verlet molecular dynamics (the use of a trained ``config_energy_force`` model that the
reference drives from ``torchMD.ipynb``: call the model on moved positions, integrate, repeat).

A force evaluation is forward + one backward through the force block: a hundred-odd launches of 5-100 us, host-bound when issued
eagerly, and the neighbour list changes as the atoms move.  ``ReplayedForceField`` pads the batch once to a bucket
(``run/graph_step.pad_batch``), and captures ``computeEdgeIndexCapped -> model`` in ONE HIP graph (``CapturedStep``: guards,
re-capture on a knot-table veto and flag polling come with it): the list is rebuilt on the device inside the graph, into a buffer of
fixed capacity (``csrc/e3k_nlist.hip``); the integrators' kernels are ``csrc/e3k_md.hip``.  More edges than the capacity is a REPORTED condition -- ``check()`` raises
``EdgeCapacityExceeded``, ``grow()`` re-pads to a larger bucket and captures again.

    ff = ReplayedForceField(model, batch, r_max=5.0)
    energy, forces = ff(pos)                  # [G], [N, 3]: static tensors, overwritten by the next call
    ff.check()                                # synchronises; raises if the list overflowed since the last check

    md = VelocityVerlet(ff, masses, dt=0.5)
    out = md.run(1000, check_every=50)        # rolls a chunk back and grows the capacity when the list overflows

    Fire(ff, ftol=1e-3).run(500)              # relax first: every molecule at its own pace, the graph + one launch per iteration
    md = Langevin(ff, masses, dt=0.5, kT=0.025, gamma=0.1, seed=7)      # the graph + two launches per step, as NVE
    md.thermalize()                           # Maxwell-Boltzmann velocities at kT

    bonds = BondConstraints(hydrogen_bonds(pos, species == 1, ff.node_ptr, 1.3), pos=pos, node_ptr=ff.node_ptr, masses=masses)
    md = Langevin(ff, masses, dt=2.0, kT=0.025, gamma=0.1, constraints=bonds)      # SHAKE / RATTLE inside the same two launches

Periodic cells: a batch with ``cell`` ([G, 3, 3], rows = lattice vectors; ``pbc`` [G, 3] optional, ASE's contract) is captured with the
periodic builder (``csrc/e3k_pbc.hip``: minimum image, one image number triple per edge) -- no new argument:

    batch["cell"], batch.attrs["cell"] = cell.reshape(G, 9), ("graph", "3x1o")      # before ReplayedForceField(model, batch, r_max)
    ff.cell, ff.pbc                           # what it uses
    xyz = wrap_positions(ff.pos, ff.cell, ff.pbc, ff.node_ptr)      # for output only

Every cell's perpendicular width along each periodic axis must exceed ``2 r_max (1 + 1e-3)`` (``ValueError`` at construction and at
``grow()``, before anything is captured): a pair then has one image at most.  Positions stay UNWRAPPED -- the minimum image is taken
from differences -- so the integrators, the thermostat, FIRE and the constraints run as they are (fp32: keep atoms within about a
thousand cell widths of the origin).

Virial and stress (``nn.output.GradientOutput``'s definitions: ``virial = -dE/d eps`` in the row-vector convention of ``cell``,
``stress = -virial / V``; one launch more inside the graph, ``csrc/e3k_virial.hip``):

    enable_virial(model)                      # nn.output: sets the keys "virial" / "stress" on the tree's GradientOutput
    ff = ReplayedForceField(model, batch, r_max, virial_key="virial", stress_key="stress")
    ff(pos); ff.check()
    ff.virial, ff.stress, ff.volume           # [G, 3, 3] fp32 static views (stress None on an open batch), float64 [G]
    p = pressure(ff.virial, out["kinetic"][-1], ff.volume)      # (2 K + tr virial) / (3 V)
    ff.set_cell(cell * 1.01); ff(pos * 1.01)  # a host-driven cell scan: nothing is captured again; positions are the caller's to scale

Constant pressure (isotropic; ``csrc/e3k_barostat.hip``: ONE launch more per step, between the drift kernel and the graph, on the
static buffers -- nothing is read back but the chunk's check):

    md = Langevin(ff, masses, dt=0.5, kT=0.025, gamma=0.1, barostat=Barostat(p0=6e-7, compressibility=50.0, tau=500.0))      # mode="scr"
    out = md.run(1000)                        # + "volume", "pressure": [steps, G] float64; ff.cell / ff.volume follow every verified chunk
    VelocityVerlet(ff, masses, dt, barostat=Barostat(p0, compressibility, tau, mode="berendsen"))      # weak coupling, no ensemble

The barostat of step k acts on the pressure of the START of the step -- the virial of the last evaluation (at x_k) and the kinetic
energy the previous kick filed -- and rescales the positions the drift has just produced, so the graph is evaluated at the rescaled
positions in the rescaled cell and both half kicks that use those forces see forces that belong to their positions.  The one-step
lag is deliberate (GROMACS couples its weak-coupling barostats the same way).  A cell that would become narrower than the list allows,
or a pressure that is not finite, freezes that graph's step on the device and is REPORTED at the chunk's check: ``BarostatFailure``.

Narrower cells (crystal unit cells): ``ReplayedForceField(..., images="all")`` captures the all-images list (``csrc/e3k_images.h``: every
image of every pair inside the cutoff, an atom's own included); ``ff.image_range`` is the table of image ranges, ``set_cell`` recomputes
it on the host (ranges above 7 are refused before anything changes), and the integrators, FIRE, constraints, ``virial_key`` and
``stress_key`` run as they are.  On a wide cell the ranges are zero and every output equals ``images="minimum"``'s bit for bit.

Not served: a barostat on a force field with ``images="all"``, semi-isotropic and anisotropic coupling, cell degrees of freedom with momenta
(MTK, Parrinello-Rahman), a barostat together with constraints, variable-cell FIRE (variable cells driven by the host are served
through ``set_cell``), training on stress, the kinetic part of the stress, cell lists (the search stays O(n^2) per graph).
"""
from __future__ import annotations

import math
from typing import Optional

import torch

from ..backend import lib as L
from ..backend.graph import EdgeCapacityExceeded
from ..data.compute_edge import IMAGE_MODES, PBC_MARGIN, _check_candidates, _inverse_cells, check_cell, computeEdgeIndex, image_ranges, computeEdgeIndexCapped, normal_draw, wrap_positions
from .capped import EDGE_KEYS, PERIODIC_REBUILT_KEYS, CappedBucket
from .graph_step import CapturedStep, bucket_capacity

__all__ = ["EdgeCapacityExceeded", "ReplayedForceField", "VelocityVerlet", "Langevin", "Fire", "BondConstraints", "ConstraintFailure",
           "hydrogen_bonds", "wrap_positions", "pressure", "Barostat", "BarostatFailure"]


def pressure(virial, kinetic, volume):
    """``(2 K + tr virial) / (3 V)`` per graph, float64, on whichever device the operands are: ``virial`` [G, 3, 3] or [G, 9] (``ff.virial``),
    ``kinetic`` [G] (a row of the integrators' kinetic record), ``volume`` [G] (``ff.volume``)."""
    w = torch.as_tensor(virial).to(torch.float64).reshape(-1, 9)
    k = torch.as_tensor(kinetic, device=w.device).to(torch.float64).reshape(-1)
    v = torch.as_tensor(volume, device=w.device).to(torch.float64).reshape(-1)
    return (2.0 * k + w[:, 0] + w[:, 4] + w[:, 8]) / (3.0 * v)


class ReplayedForceField:
    """``model``: a built ``GradientOutput`` tree in eval mode (``config_energy_force``); ``batch``: an unpadded device batch.

    ``edge_slack``: the edge capacity is the present edge count times this, rounded up to a multiple of ``edge_multiple`` (the
    bucket grid of ``bucket_capacity``)."""

    def __init__(self, model, batch, r_max: float, energy_key: str = "energy", forces_key: str = "forces", edge_slack: float = 1.5,
                 key: str = "pos", warmup: int = 3, edge_multiple: int = 1024, virial_key: Optional[str] = None,
                 stress_key: Optional[str] = None, images: str = "minimum"):
        if images not in IMAGE_MODES:
            raise ValueError(f"ReplayedForceField: images must be one of {IMAGE_MODES} (got {images!r})")
        if images == "all" and "cell" not in batch:
            raise ValueError("ReplayedForceField: images='all' needs a periodic batch (one with 'cell')")
        if not batch[key].is_cuda:
            raise RuntimeError("ReplayedForceField needs a device batch: there is no CPU fallback for graph replay")
        if edge_slack < 1.0:
            raise ValueError("edge_slack must be >= 1")
        carried = [k for k, v in batch.attrs.items() if v[0] == "edge" and k in batch and k not in EDGE_KEYS + PERIODIC_REBUILT_KEYS]
        if carried:
            raise ValueError(f"the edge attributes {carried} cannot follow a rebuilt neighbour list")
        self.model, self.r_max, self.key = model, float(r_max), key
        self.energy_key, self.forces_key = energy_key, forces_key
        self.virial_key, self.stress_key = virial_key, stress_key
        self.images = images
        if "cell" not in batch:
            self.stress_key = None      # an open batch has no volume: ``stress`` stays None
        self._require_emitted(model, self.virial_key, self.stress_key)      # before anything is captured
        self.edge_slack, self.warmup, self.edge_multiple = float(edge_slack), warmup, int(edge_multiple)
        self.dev = batch[key].device
        self._base = batch.clone()
        for k in EDGE_KEYS + PERIODIC_REBUILT_KEYS + ("_image_range",):      # (the ranges: made by every _build of images="all")
            self._base.pop(k)
        self._base.attrs.pop("_image_range", None)
        # a periodic batch: what the builder uses (None: open boundaries) -- [G, 3, 3] fp32 and bool [G, 3]
        self.cell = self._base["cell"].detach().reshape(-1, 3, 3) if "cell" in self._base else None
        self.pbc = None if self.cell is None else (self._base["pbc"].reshape(-1, 3) != 0 if "pbc" in self._base else
                                                   torch.ones(self.cell.shape[0], 3, dtype=torch.bool, device=self.dev))
        self.volume = None if self.cell is None else self._volume(self.cell)
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
        if self.cell is not None and self.images == "minimum":      # on the host, before anything is captured (construction and every grow())
            check_cell(self.cell, self.pbc, self.r_max)
        base = self._base.clone()
        base[self.key] = pos.detach().to(torch.float32).clone()
        # eager: the sizes go to the host once.  images="all": image_ranges runs here, on the host, where check_cell runs otherwise,
        # and leaves ``_image_range`` in the batch -- the capture below then takes the all-images builder
        new, attrs = computeEdgeIndex(base.data, base.attrs, r_max=self.r_max, key=self.key, images=self.images if self.cell is not None else None)
        base.attrs.update(attrs)
        base.update(new)
        n, e = self.n_real, int(new["edge_index"].shape[1])
        want = max(int(e * self.edge_slack) + 1, int(e_min))
        _, e_cap = bucket_capacity([(n, want)], edge_multiple=self.edge_multiple)
        bucket = self._bucket = CappedBucket.around_list(base, e_cap, self.key)
        self.static, self.n_cap, self.e_cap = bucket.padded, bucket.n_cap, bucket.e_cap
        self.pos = self.static[self.key][:self.n_real]      # the real nodes' positions: write here, then evaluate()
        model = self.model

        def evaluate():
            work = bucket.view()
            computeEdgeIndexCapped(work.data, work.attrs, r_max=self.r_max, key=self.key)
            out = model(work)
            res = (out[self.energy_key].reshape(-1)[:self.n_graphs], out[self.forces_key][:self.n_real])
            # (the model files them for the padded batch's graphs, the ghost graph last: the real graphs' rows)
            return res + tuple(out[k].reshape(-1, 9)[:self.n_graphs] for k in self._extra_keys)

        self.captured = CapturedStep(evaluate, warmup=self.warmup, device=self.dev)
        self.valid = False
        self._out = self.captured.out
        self._check_outputs(self._out)

    @property
    def _extra_keys(self):
        return tuple(k for k in (self.virial_key, self.stress_key) if k is not None)

    @staticmethod
    def _require_emitted(model, virial_key, stress_key) -> None:
        from ..nn.output import GradientOutput

        heads = [m for m in getattr(model, "modules", lambda: [])() if isinstance(m, GradientOutput)]
        for what, key in (("virial", virial_key), ("stress", stress_key)):
            if key is not None and not any(getattr(m, what) == key for m in heads):
                raise KeyError(f"the model does not emit the {what} '{key}': nn.output.enable_virial(model, ...) sets the keys of its "
                               "GradientOutput")

    @staticmethod
    def _volume(cell) -> torch.Tensor:
        """float64 [G] on the cell's device: |det| of the fp32 cell the builder uses, formed on the host."""
        return torch.linalg.det(cell.detach().to("cpu", torch.float64).reshape(-1, 3, 3)).abs().to(cell.device)

    @property
    def virial(self):
        """[G, 3, 3] fp32, ``-dE_g / d eps`` (``GradientOutput``'s definition): a static view, overwritten by the next evaluation and
        covered by ``valid`` / ``check()`` like energy and forces; None without a ``virial_key``."""
        return None if self.virial_key is None else self._out[2].view(-1, 3, 3)

    @property
    def stress(self):
        """[G, 3, 3] fp32, ``-virial / volume``: as ``virial``; None without a ``stress_key`` or without a cell."""
        return None if self.stress_key is None else self._out[len(self._extra_keys) + 1].view(-1, 3, 3)

    @property
    def image_range(self):
        """[G, 3] int32: a view of the captured graph's image ranges (``images="all"``; ``data.image_ranges`` at this ``r_max``), else None"""
        return self.static.data["_image_range"].view(-1, 3)[:self.n_graphs] if self.images == "all" else None

    def set_cell(self, cell) -> None:
        """New cells for the captured graph, ``[G, 3, 3]`` or ``[G, 9]`` (host or device), WITHOUT capturing again: ``check_cell`` (with
        ``images="all"``: ``image_ranges``, whose table is overwritten in place beside the cell; a range that rises may overflow the
        list: ``check()`` / ``grow()``) runs on the host first and raises before anything changes; then the static ``cell`` and its host-made float64 inverse (rounded to
        fp32, as at construction) are overwritten in place -- the pointers stay, the next replay rebuilds the list -- ``cell`` and
        ``volume`` follow and ``valid`` is False.  The ghost graph's rows stay zero.  The positions are the CALLER's to scale (a
        homogeneous strain moves them with the cell: ``pos @ (I + eps)``); an open force field raises ``ValueError``.  For cell scans
        and relaxations driven from the host (one synchronising copy per call); ``pbc`` does not change."""
        if self.cell is None:
            raise ValueError("set_cell: this force field was captured on an open batch (no 'cell'): there is no cell to change")
        new = torch.as_tensor(cell).detach().to("cpu", torch.float64)
        if new.numel() != 9 * self.n_graphs:
            raise ValueError(f"set_cell needs [{self.n_graphs}, 3, 3] (or [{self.n_graphs}, 9]), got {tuple(new.shape)}")
        new = new.reshape(-1, 3, 3).to(torch.float32)      # what the builder uses
        ranges = None
        if self.images == "all":
            ranges = image_ranges(new, self.pbc, self.r_max)
            _check_candidates(self._base["_n_nodes"], ranges)
        else:
            check_cell(new, self.pbc, self.r_max)
        inv = _inverse_cells(new.to(torch.float64)).to(torch.float32)
        static = self.static.data
        if ranges is not None:
            self.image_range.copy_(ranges)
        static["cell"].view(-1, 9)[:self.n_graphs].copy_(new.reshape(-1, 9))
        static["_inv_cell"].view(-1, 9)[:self.n_graphs].copy_(inv.reshape(-1, 9))
        self.cell.copy_(new)      # (a view of the base batch: a grow() captures on it)
        self.volume = self._volume(self.cell)
        self.valid = False

    # ---- what a barostat reads and writes on the device (``Barostat``): the REAL graphs' rows of the static buffers the periodic
    # builder reads through fixed pointers; new tensors after every capture
    @property
    def static_cell(self):
        """[G, 9] fp32: a view of the captured graph's cells"""
        return self.static.data["cell"].view(-1, 9)[:self.n_graphs]

    @property
    def static_inv_cell(self):
        """[G, 9] fp32: a view of the inverses the builder uses"""
        return self.static.data["_inv_cell"].view(-1, 9)[:self.n_graphs]

    @property
    def static_pbc(self):
        """[G, 3] int32"""
        return self.static.data["_pbc_mask"].view(-1, 3)[:self.n_graphs]

    @property
    def min_width(self) -> float:
        """What every periodic perpendicular width must exceed: ``check_cell``'s ``2 r_max (1 + 1e-3)``"""
        return 2.0 * self.r_max * (1.0 + PBC_MARGIN)

    def sync_cell(self) -> None:
        """After a synchronising ``check()``: the cells the device holds (a barostat rescales them in place) become ``cell`` -- the
        base batch's view, what a ``grow()`` captures on -- and ``volume`` follows.  One small copy to the host."""
        if self.cell is None:
            raise ValueError("sync_cell: this force field was captured on an open batch (no 'cell')")
        self.cell.copy_(self.static_cell.view(-1, 3, 3))
        self.volume = self._volume(self.cell)

    @staticmethod
    def _check_outputs(out) -> None:
        # the integrator's kernels read these through raw pointers: dense fp32 rows or nothing (a slice of the leading rows of a
        # contiguous model output is contiguous; anything else is refused here, once per capture, not read wrongly)
        for name, t in zip(("energy", "forces", "virial or stress", "stress"), out):
            if t.dtype != torch.float32 or not t.is_contiguous():
                raise TypeError(f"the captured {name} output is {t.dtype}, contiguous={t.is_contiguous()}: the MD kernels need "
                                "contiguous float32")

    @property
    def recaptures(self) -> int:
        return self.captured.recaptures

    @property
    def n_edges(self) -> torch.Tensor:
        """Device int64 scalar: the real edges the last evaluation's list needed (more than ``e_cap``: it overflowed)."""
        return self._bucket.state[0]

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
            self._out = out
            self.valid = True
            return out[:2]
        except EdgeCapacityExceeded:
            self._overflow = True
            self.valid = False
            self._out = self.captured.out
            return self._out[:2]

    def __call__(self, pos):
        self.pos.copy_(pos)
        return self.evaluate()

    def check(self) -> None:
        """Synchronises; raises ``EdgeCapacityExceeded`` if a list overflowed (or an evaluation was cut short by an earlier
        overflow's report) since the last check, and clears the condition."""
        over, self._overflow = self._overflow, False
        try:
            self._bucket.check()
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
# The minimiser's iteration and the integrators' two half steps.  The per-step updates are kernels of csrc/e3k_md.hip on device
# tensors; host tensors (a stub force field in the rollback tests, the float64 oracle loops) take the same arithmetic in torch.
# ---------------------------------------------------------------------------------------------------------------------
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
        if b <= a or bool(fmax < fire.ftol):      # (an empty graph is frozen whatever ftol is: ftol = 0 is accepted)
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


# ---------------------------------------------------------------------------------------------------------------------
# Bond-length constraints (csrc/e3k_md.hip): SHAKE inside the first half step, RATTLE inside the second.
# ---------------------------------------------------------------------------------------------------------------------
MAX_SATELLITES = 4


class ConstraintFailure(RuntimeError):
    """Stars did not meet their stopping rule within ``max_iter`` sweeps since the last check: ``shake`` and ``rattle`` count them.
    The driver is back at the last verified step and its counters are cleared."""

    def __init__(self, shake: int, rattle: int):
        self.shake, self.rattle = int(shake), int(rattle)
        super().__init__(f"bond constraints not met since the last check: SHAKE failed on {self.shake} stars, RATTLE on "
                         f"{self.rattle}; the state is that of the last verified step (a smaller dt or a larger max_iter)")


def hydrogen_bonds(pos, light, node_ptr, max_length: float):
    """``pairs`` [C, 2] (heavy, light) for ``BondConstraints``: every atom of the boolean mask ``light`` [N] with the nearest
    non-light atom of its own graph within ``max_length`` (ties: the lowest index); a light atom with no partner in range stays
    free.  No species table is guessed: the caller says which atoms are light."""
    x = pos.detach().cpu().double()
    light = torch.as_tensor(light).detach().cpu().reshape(-1).bool()
    if light.numel() != x.shape[0]:
        raise ValueError(f"a mask of {light.numel()} for {x.shape[0]} atoms")
    bounds = node_ptr.detach().cpu().tolist()
    pairs = []
    for a, b in zip(bounds[:-1], bounds[1:]):
        li = torch.nonzero(light[a:b]).reshape(-1) + a
        hv = torch.nonzero(~light[a:b]).reshape(-1) + a
        if li.numel() == 0 or hv.numel() == 0:
            continue
        d = (x[li][:, None, :] - x[hv][None, :, :]).norm(dim=2)
        dmin, j = d.min(dim=1)
        keep = dmin <= max_length
        pairs.append(torch.stack([hv[j[keep]], li[keep]], 1))
    out = torch.cat(pairs) if pairs else torch.zeros(0, 2, dtype=torch.int64)
    return out.to(pos.device)


class BondConstraints:
    """Fixed distances between pairs of atoms, as disjoint STARS: a centre with 1 to 4 satellites, every satellite in exactly one
    constraint, no atom in two stars -- the bonds-to-hydrogen set (CH4 and NH4+ need the four).  Stars share no atom, so one thread
    owns a star: no atomics, the same bits every run.  Anything else is refused with a ``ValueError`` that names the atoms: a pair
    across two graphs, a duplicate or a self pair, two constraints between atoms that each have another (chains, rings, rigid
    water's H-H, an atom that would be a satellite twice), more than four satellites, a length <= 0, a non-positive or non-finite
    mass on a constrained atom.

    ``pairs`` [C, 2] int64 node indices of the unpadded batch; ``lengths`` [C] (None: the present distances in ``pos``).  The atom
    of a pair that has other constraints is the centre (an isolated pair: its first atom).  ``tol``: the relative length error
    SHAKE stops at, and RATTLE's |r.v_rel| <= tol d0 (|v_c| + |v_s|); below 16 ulp of the positions' dtype it is refused (fp32
    cannot reach it).  ``max_iter`` sweeps at most.

    Built once, on ``pos``'s device: ``star_ptr`` [S + 1] into ``star_atom`` / ``star_len`` (centre first, then the satellites,
    each with its length beside it), ``free_atom`` (the atoms in no star), both sorted by graph with ``graph_star_ptr`` /
    ``graph_free_ptr`` [G + 1]; ``dof`` [G] = 3 n_g - c_g; ``counters`` int32 [2]: SHAKE's and RATTLE's failures."""

    def __init__(self, pairs, lengths=None, *, pos, node_ptr, masses, tol: float = 1e-5, max_iter: int = 32):
        dev, dtype = pos.device, pos.dtype
        n = int(pos.shape[0])
        ptr = node_ptr.detach().cpu().to(torch.int64).reshape(-1)
        n_graphs = ptr.numel() - 1
        if n_graphs < 0 or int(ptr[-1]) != n:
            raise ValueError(f"node_ptr ends at {int(ptr[-1]) if ptr.numel() else None} for {n} atoms")
        if not tol >= 16 * torch.finfo(dtype).eps / 2:
            raise ValueError(f"tol = {tol} is below 16 ulp of {dtype} ({16 * torch.finfo(dtype).eps / 2:.3g}): it cannot be reached")
        if max_iter < 1:
            raise ValueError("max_iter >= 1")
        self.tol, self.max_iter, self.n, self.n_graphs = float(tol), int(max_iter), n, n_graphs
        pairs = torch.as_tensor(pairs).detach().cpu().to(torch.int64).reshape(-1, 2)
        a, b = pairs[:, 0], pairs[:, 1]
        n_con = pairs.shape[0]

        def refuse(mask, what):
            if bool(mask.any()):
                rows = pairs[mask][:8].tolist()
                raise ValueError(f"{what}: atoms {', '.join(f'({i}, {j})' for i, j in rows)}" + (" ..." if int(mask.sum()) > 8 else ""))

        refuse((pairs < 0).any(1) | (pairs >= n).any(1), f"constraint between atoms outside 0..{n - 1}")
        refuse(a == b, "an atom constrained to itself")
        seg = torch.bucketize(torch.arange(n), ptr[1:], right=True)
        refuse(seg[a] != seg[b], "a constraint across two graphs")
        key = torch.minimum(a, b) * n + torch.maximum(a, b)
        _, inverse, counts = torch.unique(key, return_inverse=True, return_counts=True)
        refuse(counts[inverse] > 1, "a duplicate constraint")
        deg = torch.bincount(pairs.reshape(-1), minlength=n)
        refuse((deg[a] > 1) & (deg[b] > 1), "not a star (a chain, a ring, or an atom that would be a satellite of two centres): both "
               "ends of a constraint have other constraints")
        centre = torch.where(deg[a] >= deg[b], a, b)
        sat = a + b - centre
        refuse(deg[centre] > MAX_SATELLITES, f"a centre with more than {MAX_SATELLITES} satellites")
        x = pos.detach().cpu().double()
        if lengths is None:
            length = (x[sat] - x[centre]).norm(dim=1)
        else:
            length = torch.as_tensor(lengths).detach().cpu().double().reshape(-1)
            if length.numel() != n_con:
                raise ValueError(f"{length.numel()} lengths for {n_con} constraints")
        refuse(~(length > 0) | ~torch.isfinite(length), "a constraint of length <= 0 (or not finite)")
        m = masses.detach().cpu().double().reshape(-1)
        if m.numel() != n:
            raise ValueError(f"{m.numel()} masses for {n} atoms")
        bad = ~(m > 0) | ~torch.isfinite(m)
        refuse(bad[a] | bad[b], "a constrained atom whose mass is not positive and finite")

        order = torch.argsort(centre, stable=True)      # by centre (so by graph), a star's satellites in the order of ``pairs``
        centre, sat, length = centre[order], sat[order], length[order]
        star_centre, star_of, n_sat = torch.unique_consecutive(centre, return_inverse=True, return_counts=True)
        n_stars = star_centre.numel()
        star_ptr = torch.zeros(n_stars + 1, dtype=torch.int64)
        star_ptr[1:] = torch.cumsum(n_sat + 1, 0)
        first = torch.zeros(n_stars, dtype=torch.int64)
        first[1:] = torch.cumsum(n_sat, 0)[:-1]
        rank = torch.arange(n_con) - first[star_of]      # the satellite's place in its star
        star_atom = torch.zeros(n_stars + n_con, dtype=torch.int64)
        star_len = torch.zeros(n_stars + n_con, dtype=torch.float64)
        star_atom[star_ptr[:-1]] = star_centre
        star_atom[star_ptr[:-1][star_of] + 1 + rank] = sat
        star_len[star_ptr[:-1][star_of] + 1 + rank] = length
        free = torch.nonzero(deg == 0).reshape(-1)

        def graph_ptr(nodes):
            out = torch.zeros(n_graphs + 1, dtype=torch.int64)
            out[1:] = torch.cumsum(torch.bincount(seg[nodes], minlength=n_graphs), 0)
            return out

        self.n_stars, self.n_free, self.n_slots, self.n_constraints = n_stars, int(free.numel()), n_stars + n_con, n_con
        self.max_sat = int(n_sat.max()) if n_stars else 0
        self.star_ptr, self.star_atom = star_ptr.to(dev), star_atom.to(dev)
        self.star_len = star_len.to(dtype).to(dev).contiguous()
        self.free_atom = free.to(dev)
        self.graph_star_ptr, self.graph_free_ptr = graph_ptr(star_centre).to(dev), graph_ptr(free).to(dev)
        self.dof = (3 * (ptr[1:] - ptr[:-1]) - torch.bincount(seg[centre], minlength=n_graphs)).to(dev)
        self.counters = torch.zeros(2, dtype=torch.int32, device=dev)
        self._shake_counter, self._rattle_counter = self.counters[0:1], self.counters[1:2]
        # the same tables padded to [S, 5] for the torch path (a slot behind a star's own holds its centre and is masked out)
        idx = star_centre[:, None].repeat(1, MAX_SATELLITES + 1)
        valid = torch.zeros(n_stars, MAX_SATELLITES + 1, dtype=torch.bool)
        d0 = torch.ones(n_stars, MAX_SATELLITES, dtype=torch.float64)
        valid[:, 0] = True
        idx[star_of, 1 + rank], valid[star_of, 1 + rank], d0[star_of, rank] = sat, True, length
        self._idx, self._valid, self._d0 = idx.to(dev), valid.to(dev), d0.to(dtype).to(dev)

    @property
    def pairs(self):
        """[C, 2] (centre, satellite), in the tables' order."""
        return torch.stack([self._idx[:, :1].expand(-1, MAX_SATELLITES)[self._valid[:, 1:]], self._idx[:, 1:][self._valid[:, 1:]]], 1)

    @property
    def lengths(self):
        return self._d0[self._valid[:, 1:]]


def _table_args(con):
    return (L.ptr(con.star_ptr), L.ptr(con.star_atom), L.ptr(con.star_len), con.n_stars, con.n_slots, L.ptr(con.free_atom), con.n_free)


# ---------------------------------------------------------------------------------------------------------------------
# The two half steps of every integrator: one function each.  On device tensors a function picks the C entry; on host tensors it
# runs one torch sequence of the same arithmetic.
# ---------------------------------------------------------------------------------------------------------------------
THERMOSTAT_WORD, THERMALIZE_WORD = 0, 4      # first hash word of a step's draw and of thermalize()'s: the streams never coincide


def _drift(x, v, f, mass, dt: float, con=None) -> None:
    """First half: ``v += dt/2 f / m``, ``x += dt v``, with SHAKE on the stars of ``con`` (``e3k_md_drift`` /
    ``e3k_md_drift_shake``).  ``f`` None (constrained only): positions only -- the lengths are enforced at the present positions
    along the present bonds, nothing else moves."""
    if x.is_cuda:
        if con is None:
            L.check(L.load().e3k_md_drift(L.ptr(x), L.ptr(v), L.ptr(f), L.ptr(mass), x.shape[0], float(dt), L.stream_ptr()), "e3k_md_drift")
        else:
            L.check(L.load().e3k_md_drift_shake(L.ptr(x), L.ptr(v), L.ptr(f), L.ptr(mass), x.shape[0], float(dt), *_table_args(con),
                                                con.tol, con.max_iter, L.ptr(con._shake_counter), L.stream_ptr()), "e3k_md_drift_shake")
        return
    stars = con is not None and con.n_stars > 0
    if stars:
        idx, valid = con._idx, con._valid
        x0 = x[idx]                                     # [S, 5, 3]: the old positions, before anything moves
    if f is not None:
        v.add_(f / mass[:, None], alpha=0.5 * dt)
        x.add_(v, alpha=dt)
    if not stars:
        return
    ro = x0[:, 1:] - x0[:, :1]                          # the old bond vectors; everything below is relative to the centre's old position
    p = x0 - x0[:, :1]
    vh = v[idx]
    if f is not None:
        p = p + dt * vh
    q = p.clone()
    inv_m = 1.0 / mass[idx]
    on_k, d02 = valid[:, 1:], con._d0 * con._d0
    fail = torch.zeros(con.n_stars, dtype=torch.bool)
    # a pass visits the constraints in stored order and corrects those outside the tolerance; it ends after a pass that found none
    # (a star that is within it is not touched again: the passes are each star's own); pass number max_iter only looks
    for it in range(con.max_iter + 1):
        moved = False
        for k in range(con.max_sat):
            r = p[:, 1 + k] - p[:, 0]
            diff = d02[:, k] - (r * r).sum(-1)
            out = on_k[:, k] & ~(diff.abs() <= 2.0 * con.tol * d02[:, k])
            if not bool(out.any()):
                continue
            moved = True
            rr = (r * ro[:, k]).sum(-1)
            on = out & (rr > 0) if it < con.max_iter else torch.zeros_like(out)
            fail |= out & ~on
            g = torch.where(on, diff / (2.0 * rr * (inv_m[:, 0] + inv_m[:, 1 + k])), torch.zeros_like(rr))
            p[:, 1 + k] += (g * inv_m[:, 1 + k])[:, None] * ro[:, k]
            p[:, 0] -= (g * inv_m[:, 0])[:, None] * ro[:, k]
        if not moved:
            break
    x[idx[valid]] = (x0[:, :1] + p)[valid]
    if f is not None:
        v[idx[valid]] = (vh + (p - q) / dt)[valid]
    con.counters[0] += int(fail.sum())


def _kick_langevin(v, f, mass, node_ptr, dt: float, c: float, s: float, seed: int, draw: int, word0: int, kinetic, energy=None,
                   potential=None, *, con=None, x=None) -> None:
    """Second half: ``v <- c v + (s / sqrt(m)) xi`` (``(c, s) = (1, 0)``: no thermostat, nothing is drawn), then
    ``v += dt/2 f / m`` (``f`` None: no kick), then RATTLE on the stars of ``con`` along the present bonds in ``x``, then the
    records: ``kinetic`` [G] takes the graphs' kinetic energies (of the projected velocities) and ``potential`` [G] a copy of
    ``energy`` [G] (the force field's static output) in the same launch; None: not wanted.  ``xi`` is
    ``normal_draw(seed, draw, node, word0 + component)``: counter-based, the same bits whenever the same step is done again.
    Entries: ``e3k_md_kick_rattle`` with constraints, else ``e3k_md_kick`` for the plain kick with forces and
    ``e3k_md_kick_langevin`` for everything else -- one kernel behind both."""
    plain = c == 1.0 and s == 0.0
    if v.is_cuda:
        lib, n_graphs = L.load(), node_ptr.numel() - 1
        if con is None and plain and f is not None:
            L.check(lib.e3k_md_kick(L.ptr(v), L.ptr(f), L.ptr(mass), L.ptr(node_ptr), n_graphs, v.shape[0], float(dt), L.ptr(kinetic),
                                    L.ptr(energy), L.ptr(potential), L.stream_ptr()), "e3k_md_kick")
            return
        head = (L.ptr(v), L.ptr(f), L.ptr(mass), L.ptr(node_ptr), n_graphs, v.shape[0], float(dt), float(c), float(s),
                *L.seed_words(seed), draw & 0xFFFFFFFF, int(word0), L.ptr(kinetic), L.ptr(energy), L.ptr(potential))
        if con is None:
            L.check(lib.e3k_md_kick_langevin(*head, L.stream_ptr()), "e3k_md_kick_langevin")
        else:
            L.check(lib.e3k_md_kick_rattle(*head, L.ptr(x), *_table_args(con), L.ptr(con.graph_star_ptr), L.ptr(con.graph_free_ptr),
                                           con.tol, con.max_iter, L.ptr(con._rattle_counter), L.stream_ptr()), "e3k_md_kick_rattle")
        return
    if not plain:
        node = torch.arange(v.shape[0], dtype=torch.int64)[:, None]
        xi = normal_draw(seed, draw, node, word0 + torch.arange(3, dtype=torch.int64)[None, :], v.dtype)
        v.mul_(c).add_((s / torch.sqrt(mass))[:, None] * xi)
    if f is not None:
        v.add_(f / mass[:, None], alpha=0.5 * dt)
    if con is not None and con.n_stars:
        idx, valid = con._idx, con._valid
        xs = x[idx]
        r = xs[:, 1:] - xs[:, :1]
        r2 = (r * r).sum(-1)
        u = v[idx]
        inv_m = 1.0 / mass[idx]
        on_k = valid[:, 1:]
        fail = torch.zeros(con.n_stars, dtype=torch.bool)
        for it in range(con.max_iter + 1):      # passes as in _drift
            moved = False
            for k in range(con.max_sat):
                rv = (r[:, k] * (u[:, 1 + k] - u[:, 0])).sum(-1)
                lim = con.tol * con._d0[:, k] * (u[:, 0].norm(dim=-1) + u[:, 1 + k].norm(dim=-1))
                out = on_k[:, k] & ~(rv.abs() <= lim)
                if not bool(out.any()):
                    continue
                moved = True
                on = out & (r2[:, k] > 0) if it < con.max_iter else torch.zeros_like(out)
                fail |= out & ~on
                g = torch.where(on, rv / (r2[:, k] * (inv_m[:, 0] + inv_m[:, 1 + k])), torch.zeros_like(rv))
                u[:, 1 + k] -= (g * inv_m[:, 1 + k])[:, None] * r[:, k]
                u[:, 0] += (g * inv_m[:, 0])[:, None] * r[:, k]
            if not moved:
                break
        v[idx[valid]] = u[valid]
        con.counters[1] += int(fail.sum())
    if potential is not None:
        potential.copy_(energy)
    if kinetic is not None:
        per_node = 0.5 * mass * (v * v).sum(1)
        for g in range(node_ptr.numel() - 1):
            kinetic[g] = per_node[int(node_ptr[g]):int(node_ptr[g + 1])].sum()


# ---------------------------------------------------------------------------------------------------------------------
# Pressure control (csrc/e3k_barostat.hip): one launch between the drift kernel and the force graph.
# ---------------------------------------------------------------------------------------------------------------------
BAROSTAT_SRC = 0xFFFFFFFE      # the draw stream's src word of "a graph's barostat" (csrc/e3k_draw.h); the word is the graph


class BarostatFailure(RuntimeError):
    """Graphs whose barostat step could not be taken since the last check (a singular cell, a pressure that is not finite, a new
    cell narrower than the periodic list allows): ``count`` graph-steps were frozen.  The driver is back at the last verified step
    and the counter is cleared."""

    def __init__(self, count: int):
        self.count = int(count)
        super().__init__(f"the barostat froze {self.count} graph-steps since the last check (a cell that would become narrower than "
                         "2 r_max (1 + 1e-3), a singular cell, or a pressure that is not finite); the state is that of the last "
                         "verified step (a smaller compressibility / tau ratio, another p0, or a supercell)")


class Barostat:
    """Isotropic pressure coupling at ``p0`` (the model's energy per volume) for ``VelocityVerlet`` / ``Langevin(barostat=)``:
    once per step and graph, ``d_eps = a (P - p0) + sqrt(b / V) xi`` in ``eps = ln V`` with ``a = compressibility dt / tau``,
    then cell and positions scale by ``mu = exp(d_eps / 3)``.

    ``mode="scr"``: stochastic cell rescaling (Bernetti & Bussi, J. Chem. Phys. 153, 114107 (2020)), Euler-Maruyama:
    ``b = 2 kT compressibility dt / tau`` with the integrator's ``kT``, velocities scale by ``1 / mu``; it samples the NPT
    volume distribution up to a bias of first order in ``a``.  ``mode="berendsen"``: ``b = 0`` and the velocities are left alone --
    Berendsen's weak coupling to first order in ``a``; it relaxes the volume and samples no ensemble."""

    MODES = ("scr", "berendsen")

    def __init__(self, p0: float, compressibility: float, tau: float, mode: str = "scr"):
        if mode not in self.MODES:
            raise ValueError(f"Barostat: mode must be one of {self.MODES}, got {mode!r}")
        if not tau > 0:
            raise ValueError(f"Barostat: tau must be > 0 (the coupling time), got {tau}")
        if not compressibility >= 0 or not math.isfinite(compressibility):
            raise ValueError(f"Barostat: compressibility must be >= 0 and finite, got {compressibility}")
        self.p0, self.compressibility, self.tau, self.mode = float(p0), float(compressibility), float(tau), mode

    def coefficients(self, dt: float, kT: Optional[float]):
        """``(a, b)`` of one step of length ``dt``"""
        a = self.compressibility * abs(dt) / self.tau
        return a, (2.0 * float(kT) * a if self.mode == "scr" else 0.0)


def _det3(c):
    """``a . (b x c)`` of the rows of ``c`` [G, 9], in the kernel's expression"""
    return c[:, 0] * (c[:, 4] * c[:, 8] - c[:, 5] * c[:, 7]) - c[:, 1] * (c[:, 3] * c[:, 8] - c[:, 5] * c[:, 6]) + \
        c[:, 2] * (c[:, 3] * c[:, 7] - c[:, 4] * c[:, 6])


def _adjugate3(c):
    """[G, 9]: the transposed cofactors of ``c`` [G, 9]; ``inverse = adjugate / det`` (the barostat's rule for ``inv_cell``)"""
    return torch.stack([c[:, 4] * c[:, 8] - c[:, 5] * c[:, 7], c[:, 2] * c[:, 7] - c[:, 1] * c[:, 8], c[:, 1] * c[:, 5] - c[:, 2] * c[:, 4],
                        c[:, 5] * c[:, 6] - c[:, 3] * c[:, 8], c[:, 0] * c[:, 8] - c[:, 2] * c[:, 6], c[:, 2] * c[:, 3] - c[:, 0] * c[:, 5],
                        c[:, 3] * c[:, 7] - c[:, 4] * c[:, 6], c[:, 1] * c[:, 6] - c[:, 0] * c[:, 7], c[:, 0] * c[:, 4] - c[:, 1] * c[:, 3]], 1)


def _barostat(x, v, cell, inv_cell, pbc, virial, kinetic, node_ptr, p0: float, a: float, b: float, min_width: float, seed: int,
              draw: int, counter, volume=None, pressure=None) -> None:
    """One barostat step on every graph, in place (``e3k_barostat_step``; include/e3k.h, "Barostat", states the arithmetic): ``x``
    [N, 3], ``v`` [N, 3] or None (not rescaled), ``cell`` / ``inv_cell`` [G, 9] (rows of a buffer that may be longer),
    ``pbc`` [G, 3] integers, ``virial`` [G, 9] or [G, 3, 3], ``kinetic`` [G], ``counter`` int32 [1] (frozen graphs are added),
    ``volume`` / ``pressure`` float64 [G] or None.  The torch path (host tensors): all graphs at once in float64 -- ``mu`` as the
    kernel forms it, with the same ``xi`` (``normal_draw(seed, draw, 0xFFFFFFFE, g)``) -- and the products in the tensors' own
    dtype, rounded once each: on fp32 tensors it is the kernel's arithmetic but for ``exp`` and the draw's ``log`` / ``cos``."""
    n_graphs = node_ptr.numel() - 1
    if not (a >= 0 and b >= 0 and math.isfinite(a) and math.isfinite(b) and min_width >= 0):
        raise ValueError(f"_barostat: a = {a}, b = {b} and min_width = {min_width} must be >= 0 and finite")
    if x.is_cuda:
        L.check(L.load().e3k_barostat_step(L.ptr(x), L.ptr(v), L.ptr(cell), L.ptr(inv_cell), L.ptr(pbc), L.ptr(virial), L.ptr(kinetic),
                                           L.ptr(node_ptr), n_graphs, x.shape[0], float(p0), float(a), float(b), float(min_width),
                                           *L.seed_words(seed), draw & 0xFFFFFFFF, L.ptr(counter), L.ptr(volume), L.ptr(pressure),
                                           L.stream_ptr()), "e3k_barostat_step")
        return
    f64 = torch.float64
    det = _det3
    vol = det(cell.reshape(-1, 9)[:n_graphs].to(f64)).abs()
    w = virial.reshape(-1, 9)[:n_graphs].to(f64)
    p = (2.0 * kinetic.reshape(-1)[:n_graphs].to(f64) + ((w[:, 0] + w[:, 4]) + w[:, 8])) / (3.0 * vol)
    d_eps = a * (p - p0)
    if b > 0:
        xi = normal_draw(seed, draw & 0xFFFFFFFF, BAROSTAT_SRC, torch.arange(n_graphs, dtype=torch.int64), f64)
        d_eps = d_eps + torch.sqrt(b / vol) * xi
    mu = torch.exp(d_eps / 3.0)
    frozen = (vol == 0) | ~torch.isfinite(p) | ~torch.isfinite(d_eps) | ~torch.isfinite(mu)
    mu_t, inv_mu_t = mu.to(cell.dtype), (1.0 / mu).to(cell.dtype)
    new = cell.reshape(-1, 9)[:n_graphs] * mu_t[:, None]
    c = new.to(f64)
    new_det = det(c)
    adj = _adjugate3(c)
    frozen = frozen | (new_det == 0) | ~torch.isfinite(new_det)
    inv = adj / torch.where(frozen, torch.ones_like(new_det), new_det)[:, None]
    width = 1.0 / torch.sqrt((inv.reshape(-1, 3, 3) ** 2).sum(1))      # [G, 3]: 1 / |column k|
    frozen = frozen | ((pbc.reshape(-1, 3)[:n_graphs] != 0) & ~(width > min_width)).any(1)
    live = ~frozen
    if volume is not None:
        volume.copy_(torch.where(live, new_det.abs(), vol))
    if pressure is not None:
        pressure.copy_(p)
    counter += int(frozen.sum())
    rows = cell.reshape(-1, 9)[:n_graphs]
    rows.copy_(torch.where(live[:, None], new, rows))
    inv_rows = inv_cell.reshape(-1, 9)[:n_graphs]
    inv_rows.copy_(torch.where(live[:, None], inv.to(inv_cell.dtype), inv_rows))
    bounds = node_ptr.clamp(0, x.shape[0])
    counts = (bounds[1:] - bounds[:-1]).clamp(min=0)
    if int(bounds[0]) != 0 or int(bounds[-1]) != x.shape[0] or bool((bounds[1:] < bounds[:-1]).any()):
        for g in range(n_graphs):      # (a table that does not tile the nodes: graph by graph, as the kernel's workgroups)
            if bool(live[g]) and int(counts[g]):
                lo, hi = int(bounds[g]), int(bounds[g + 1])
                x[lo:hi] *= mu_t[g].to(x.dtype)
                if v is not None:
                    v[lo:hi] *= inv_mu_t[g].to(v.dtype)
        return
    one = torch.ones_like(mu)
    seg = torch.repeat_interleave(torch.arange(n_graphs), counts)
    x.mul_(torch.where(live, mu, one).to(x.dtype)[seg][:, None])
    if v is not None:
        v.mul_(torch.where(live, 1.0 / mu, one).to(v.dtype)[seg][:, None])


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

    def _chunk_failure(self, start: int, stop: int):
        """Called where the chunk's capacity check has synchronised: an exception to raise AFTER the chunk (iterations ``start`` to
        ``stop`` of this run) has been rolled back, or None."""
        return None

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
                    failure = self._chunk_failure(done, done + chunk)
                    if failure is not None:      # back to the last verified iteration, and the caller hears of it
                        self.x.copy_(snap_x)
                        for t, snap in zip(self._tensors(), snaps):
                            t.copy_(snap)
                        self.restores += 1
                        self._after_restore()
                        raise failure
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
    two launches outside the graph).  ``constraints``: a ``BondConstraints`` set -- the two launches become ``e3k_md_drift_shake`` and
    ``e3k_md_kick_rattle`` (still two), the kinetic record is that of the projected velocities, ``dof`` counts 3 n - c; a star that
    did not converge is found at the chunk's check: the chunk is rolled back and ``ConstraintFailure`` raised.  ``barostat``: a
    ``Barostat`` -- one launch more (``e3k_barostat_step``) between the drift kernel and the graph, on the pressure of the START of
    the step (a deliberate one-step lag: the module docstring); ``run()`` then also returns "volume" and "pressure" [steps, G]
    float64, the cell and its inverse are chunk state beside ``v`` (rolled back with it; a regrowth captures on the last verified
    cell), ``ff.sync_cell()`` follows every verified chunk, and a frozen graph raises ``BarostatFailure`` at the chunk's check.
    Needs a force field with a cell, every axis periodic and a ``virial_key``; not together with ``constraints``.  Every ``check_every`` steps the list's capacity is checked
    (the one synchronisation); a chunk that overflowed is thrown away -- positions, velocities and records go back to the last
    verified step, the capacity grows, the chunk runs again -- so an overflowed step never reaches the caller."""

    def __init__(self, ff, masses, dt: float, grow_factor: float = 1.5, seed: int = 0, *, constraints=None, barostat=None):
        super().__init__(ff, grow_factor)
        self.dt, self.seed = float(dt), int(seed)
        x = ff.pos
        if barostat is not None:      # refused before anything is allocated, each with its reason
            if constraints is not None:
                raise ValueError("barostat= together with constraints= is not served: scaling every atom about the origin changes the "
                                 "fixed bond lengths, and the constraint forces' virial is not formed")
            if getattr(ff, "cell", None) is None:
                raise ValueError("a barostat needs a periodic force field: this one has no cell")
            if getattr(ff, "images", "minimum") == "all":
                raise ValueError("barostat= on a force field with images='all' is not served: the barostat kernel freezes a graph by one "
                                 "minimum width, which has no meaning for per-axis image ranges")
            if not bool(torch.as_tensor(ff.pbc).all()):
                raise ValueError("a barostat needs every axis periodic: this force field has a non-periodic axis (isotropic scaling "
                                 "of an open direction has no pressure to answer to)")
            if getattr(ff, "virial_key", None) is None:
                raise ValueError("a barostat reads the virial: capture the force field with a virial_key (nn.output.enable_virial)")
            if barostat.mode == "scr" and getattr(self, "kT", None) is None:
                raise ValueError("Barostat(mode='scr') takes kT from the integrator: use Langevin, or mode='berendsen'")
        self.barostat = barostat
        self.mass = masses.to(device=x.device, dtype=x.dtype).reshape(-1).contiguous()
        if self.mass.numel() != x.shape[0]:
            raise ValueError(f"{self.mass.numel()} masses for {x.shape[0]} atoms")
        if constraints is not None:
            con = constraints
            if con.n != x.shape[0] or con.n_graphs != ff.node_ptr.numel() - 1 or con.star_len.dtype != x.dtype or \
                    con.star_len.device != x.device:
                raise ValueError("the constraints were built for another batch, dtype or device")
            if self.dt == 0.0:
                raise ValueError("constrained steps need dt != 0 (the velocity correction divides by it)")
        self.constraints = constraints
        self.v = torch.zeros_like(x).contiguous()
        self.thermalizations = 0      # the draw counter of thermalize()
        self._forces = None      # forces at the present positions (the graph's static tensor), None: not evaluated yet
        if barostat is not None:
            n_graphs = ff.node_ptr.numel() - 1
            self._baro_counter = torch.zeros(1, dtype=torch.int32, device=x.device)      # graph-steps the barostat froze
            self._kin0 = torch.zeros(n_graphs, dtype=x.dtype, device=x.device)           # the kinetic energies a run() starts from

    def thermalize(self, kT: Optional[float] = None) -> None:
        """Maxwell-Boltzmann velocities at ``kT`` (the model's energy units; default: the thermostat's, where there is one):
        ``v = sqrt(kT / m) xi``, one launch.  The draws are ``seed``'s stream of ``thermalize`` words with a counter of their own,
        so a call never repeats a step's noise or an earlier call's."""
        kT = getattr(self, "kT", None) if kT is None else float(kT)
        if kT is None or kT < 0:
            raise ValueError("thermalize() needs kT >= 0")
        # (with constraints: drawn and projected onto them in the one launch)
        _kick_langevin(self.v, None, self.mass, self.ff.node_ptr, 0.0, 0.0, kT ** 0.5, self.seed, self.thermalizations, THERMALIZE_WORD,
                       None, con=self.constraints, x=self.x)
        self.thermalizations += 1

    @property
    def dof(self):
        """[G]: each graph's degrees of freedom, 3 n_g minus its constraints."""
        if self.constraints is not None:
            return self.constraints.dof
        return 3 * (self.ff.node_ptr[1:] - self.ff.node_ptr[:-1])

    def project(self) -> None:
        """Enforces the constraints' lengths at the present positions (moving each star's atoms along its present bonds) and
        projects ``v`` onto them: for sets whose ``lengths`` are not the geometry's own.  Synchronises; raises ``ConstraintFailure``
        if a star did not converge."""
        con = self.constraints
        if con is None:
            raise ValueError("project() needs constraints")
        _drift(self.x, self.v, None, self.mass, 0.0, con)
        _kick_langevin(self.v, None, self.mass, self.ff.node_ptr, 0.0, 1.0, 0.0, 0, 0, 0, None, con=con, x=self.x)
        self._forces = None      # the positions moved
        failure = self._chunk_failure(0, 0)
        if failure is not None:
            raise failure

    def _ou(self):
        return 1.0, 0.0      # (c, s) of the second half step: no thermostat

    def _chunk_failure(self, start: int, stop: int):
        if self.barostat is not None:      # (never together with constraints)
            frozen = int(self._baro_counter.item())      # (the device is idle: the capacity check has synchronised)
            if frozen == 0:
                return None
            self._baro_counter.zero_()
            if stop > start:
                for record in (self._pot, self._kin, self._vol, self._prs):
                    record[start:stop].zero_()
            return BarostatFailure(frozen)
        con = self.constraints
        if con is None:
            return None
        shake, rattle = con.counters.tolist()      # (the device is idle: the capacity check has synchronised)
        if shake == 0 and rattle == 0:
            return None
        con.counters.zero_()
        if stop > start:
            self._pot[start:stop].zero_()
            self._kin[start:stop].zero_()
        return ConstraintFailure(shake, rattle)

    def _tensors(self):
        if self.barostat is not None:      # the cell and its inverse are chunk state beside v: the PRESENT static buffers' rows
            return (self.v, self.ff.static_cell, self.ff.static_inv_cell)
        return (self.v,)

    def _begin_chunk(self) -> None:
        self._chunk_forces = self._forces

    def _commit_chunk(self) -> None:
        self._forces = self._chunk_forces
        if self.barostat is not None:
            self.ff.sync_cell()      # ff.cell is the last VERIFIED cell: what a regrowth captures on

    def _after_restore(self) -> None:
        _, self._forces = self._verified_forces()      # the forces at the snapshot's positions, on the grown list
        if self.constraints is not None:
            self.constraints.counters.zero_()          # what the thrown-away steps counted
        if self.barostat is not None:
            self._baro_counter.zero_()

    def _step(self, i: int, k: int) -> None:
        con = self.constraints
        _drift(self.x, self.v, self._chunk_forces, self.mass, self.dt, con)
        baro = self.barostat
        if baro is not None:
            # the pressure of the START of the step: the virial of the last evaluation (at x_k) and the kinetic energy the last
            # kick filed; the drifted positions are rescaled, and the graph below sees them in the rescaled cell
            ff = self.ff
            a, b = baro.coefficients(self.dt, getattr(self, "kT", None))
            _barostat(self.x, self.v if baro.mode == "scr" else None, ff.static_cell, ff.static_inv_cell, ff.static_pbc, ff.virial,
                      self._kin[i - 1] if i > 0 else self._kin0, ff.node_ptr, baro.p0, a, b, ff.min_width, self.seed, k,
                      self._baro_counter, self._vol[i], self._prs[i])
        energy, self._chunk_forces = self.ff.evaluate()
        c, s = self._ou()
        _kick_langevin(self.v, self._chunk_forces, self.mass, self.ff.node_ptr, self.dt, c, s, self.seed, k, THERMOSTAT_WORD,
                       self._kin[i], energy, self._pot[i], con=con, x=self.x)

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
        if self.barostat is None:
            self._run_chunks(n_steps, check_every)
            return {"potential": self._pot, "kinetic": self._kin}
        self._vol = torch.zeros(n_steps, n_graphs, dtype=torch.float64, device=self.v.device)
        self._prs = torch.zeros_like(self._vol)
        # the kinetic energies of the state the run starts from: a kick with dt = 0 and no forces changes nothing and files them
        _kick_langevin(self.v, None, self.mass, self.ff.node_ptr, 0.0, 1.0, 0.0, 0, 0, 0, self._kin0)
        self._run_chunks(n_steps, check_every)
        return {"potential": self._pot, "kinetic": self._kin, "volume": self._vol, "pressure": self._prs}


class Langevin(VelocityVerlet):
    """Velocity Verlet with a Langevin thermostat at ``kT`` (in the MODEL's energy units: no Boltzmann constant is guessed) and
    friction ``gamma`` (inverse time units), in the order of the reference notebook's integrator: half kick + drift, forces, friction
    and noise, half kick -- still the graph + two launches, the second being ``e3k_md_kick_langevin``:

        v <- c v + sqrt((1 - c^2) kT / m) xi,    c = exp(-gamma dt)

    This is the exact Ornstein-Uhlenbeck step, not torchmd's first-order ``v (1 - gamma dt) + sqrt(2 gamma dt kT / m) xi``; the two
    agree to O((gamma dt)^2), the exact form is stable for any ``gamma dt`` and is the plain kick at ``gamma = 0``.

    ``xi`` is counter-based (``data/compute_edge.normal_draw``) with the ABSOLUTE step number as its draw index: a chunk that is
    rolled back and redone after an overflow sees the same noise, and a trajectory does not depend on ``check_every``."""

    def __init__(self, ff, masses, dt: float, kT: float, gamma: float, seed: int = 0, grow_factor: float = 1.5, *, constraints=None,
                 barostat=None):
        if kT < 0 or gamma < 0:
            raise ValueError("kT >= 0 and gamma >= 0")
        self.kT, self.gamma = float(kT), float(gamma)      # (before the base class: Barostat(mode="scr") asks for kT there)
        super().__init__(ff, masses, dt, grow_factor, seed, constraints=constraints, barostat=barostat)
        self.c = math.exp(-self.gamma * self.dt)                    # (float64 on the host; the kernel takes them as floats)
        self.s = math.sqrt(-math.expm1(-2.0 * self.gamma * self.dt) * self.kT)

    def _ou(self):
        return self.c, self.s


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
