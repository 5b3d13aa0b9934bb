"""The loops of the samplers and the likelihood (``run/sde_sampling``, ``run/likelihood``): one interface over three drivers.

A run is described by a ``StepPlan`` -- the working copy of the batch at its start, the updates of one step (``batch -> batch``:
corrector and predictor, or the ODE's stages), the table of times and the device cells the step header walks -- and driven by

* ``EagerLoop``: plain launches, the neighbour list rebuilt by ``moved`` after every update;
* ``StaticLoop``: the edge set cannot change -- one whole step captured in a HIP graph and replayed;
* ``CappedLoop``: cutoff graphs -- the batch padded to an edge capacity, the list rebuilt inside the captured step.

All three: ``rewind()`` puts back what a run advanced (the moved tensors, the cells, the accumulators, the neighbour-list builder's
draw index), ``run(steps)`` does ``steps`` steps from where the loop stands, ``result()`` returns the batch after the last one.  A new
loop is rewound before its first run (the replayed ones have taken their warm-up step).  ``make_loop`` picks the class.

Every step of every loop begins with ``sampler_begin_step(plan.times, plan.cells, t)``: the time comes from the table, on the device,
and replays are bare.  The header stands still past the table but the updates would repeat the last step, so a loop counts its
steps and ``run()`` past the table does nothing.  Both replayed loops record their step with ``run/graph_step.CapturedStep``: the
deferred index checks, the knot-table guards and the re-recording after a refined table are its business."""
from __future__ import annotations

from dataclasses import dataclass
from functools import partial
from typing import Any, Callable, Optional, Sequence

import torch

from ..backend.graph import TOPO_KEYS, EdgeCapacityExceeded
from ..data.compute_edge import PairCriterion, computeEdgeIndex, computeEdgeIndexCapped
from .capped import EDGE_KEYS, CappedBucket, builder_cells, edge_layer_of, replayable_criterion
from .graph_step import CapturedStep
from .sde_utils import sampler_begin_step

SAMPLER_EDGE_KEYS = EDGE_KEYS + TOPO_KEYS      # what the loop drops after every update: the list and the CSR topology built on it


def check_loop_args(graph, static_edges, edge_capacity, r_max, criteria, norms_served: bool = True) -> None:
    """The refusals every sampler shares for the arguments that choose the loop.  ``norms_served``: whether the updates' batch-wide
    reductions (the corrector's norms), if any, skip the ghost graph's rows."""
    if graph and not static_edges and edge_capacity is None:
        raise ValueError("graph capture needs static_edges=True (a changing edge count changes every launch)")
    if edge_capacity is not None:
        if not graph or static_edges:
            raise ValueError("edge_capacity belongs to graph=True on cutoff graphs (static_edges=False)")
        if not norms_served:
            raise ValueError("edge_capacity: the ghost graph's nodes would enter the corrector's batch-wide norms; only NoneCorrector is served")
        if r_max is None:
            raise ValueError("edge_capacity needs the cutoff of the neighbour list: pass r_max")
        if criteria is not None and not isinstance(criteria, PairCriterion):
            raise ValueError("edge_capacity: criteria must be a data.PairCriterion (the capped builder evaluates it in its kernels)")


def edge_plumbing(preprocess, static_edges: bool):
    """-> (rebuild_edges, moved): what the loops do to a batch's neighbour list, with the dataset's ``preprocess`` functions"""
    def rebuild_edges(batch):
        for k in SAMPLER_EDGE_KEYS:
            batch.pop(k)
        for fn in preprocess:
            new, attrs = fn(batch.data, batch.attrs)
            batch.attrs.update(attrs)
            batch.update(new)
        return batch

    def moved(b):
        # positions changed: the geometry cached in the batch by the model's first layer is stale
        # (the reference pops edge_index / edge_vector here, :236-241)
        if static_edges:
            b.pop("edge_vector")
            b.pop("edge_length")
            return b
        return rebuild_edges(b)

    return rebuild_edges, moved


def static_topology(batch, rebuild_edges) -> None:
    """(``static_edges``: the list and the CSR topology on it are built once, before the loop)"""
    from ..backend.graph import build_topology

    if "edge_index" not in batch:
        rebuild_edges(batch)
    if "_e3k_dst_ptr" not in batch and batch["edge_index"].is_cuda:
        batch.update(build_topology(batch["edge_index"], batch.n_nodes).as_dict())


def reset_criteria(model, criteria) -> None:
    own = edge_layer_of(model)
    for crit in (criteria, own and own.criterion):
        if isinstance(crit, PairCriterion):
            crit.reset()      # build k of this run draws with index k


@dataclass
class StepPlan:
    """What a loop needs to know about a run.

    batch: the working copy at its start state (the prior drawn or the probes attached, ``t`` allocated at [G, 1]).
    updates: ``batch -> batch`` callables, in order.
    keys: the tensors the updates move.
    times: the table the step header walks, one entry per step of the run (contiguous; fp32 on the device, as ``t``).
    cells: int64 [2], next step and step in use.
    zero: accumulators the updates add to (the likelihood's integral): they go back to zero with the cells.
    fixed: the name of conditional sampling's mask field, or None."""
    batch: Any
    updates: Sequence[Callable]
    keys: Sequence[str]
    times: torch.Tensor
    cells: torch.Tensor
    zero: Sequence[torch.Tensor] = ()
    fixed: Optional[str] = None


class _Loop:
    """(what the three drivers share: the step count and the plan's own loop state)"""

    def __init__(self, plan: StepPlan):
        self.plan, self.at = plan, 0

    def _rewind_plan(self) -> None:
        self.plan.cells.zero_()
        for acc in self.plan.zero:
            acc.zero_()
        self.at = 0

    def _take(self, steps: int) -> range:
        """The steps of ``run(steps)`` that lie inside the table."""
        n = max(0, min(int(steps), self.plan.times.numel() - self.at))
        self.at += n
        return range(n)


class EagerLoop(_Loop):
    """Plain launches: the header, then every update with ``moved`` behind it.  ``criteria``: a ``data.PairCriterion`` handed to the
    sampler; it and the one of the model's own ``edge_index`` layer count their builds on the host, so ``rewind()`` resets them."""

    def __init__(self, plan: StepPlan, model, moved, criteria=None):
        super().__init__(plan)
        self.model, self.moved, self.criteria, self.batch = model, moved, criteria, None

    def rewind(self) -> None:
        start = self.plan.batch      # kept pristine: the run works on a view that holds copies of the moved tensors
        self.batch = start.view()
        for k in self.plan.keys:
            self.batch[k] = start[k].clone()
        reset_criteria(self.model, self.criteria)
        self._rewind_plan()

    def run(self, steps: int) -> None:
        plan, b = self.plan, self.batch
        t = b["t"]
        for _ in self._take(steps):
            sampler_begin_step(plan.times, plan.cells, t)
            b["t"] = t
            for update in plan.updates:
                b = self.moved(update(b))
        self.batch = b

    def result(self):
        return self.batch


class StaticLoop(_Loop):
    """The steps as replays of ONE graph on a static edge set.  The static buffers are the diffused tensors (``state``) and ``t``; the
    captured step works on a copy of the batch (model layers add keys) and writes its result back into ``state``.  Noise that an
    update draws inside the graph comes from the default device generator: no other generator is registered with the graph."""

    def __init__(self, plan: StepPlan, model, moved):
        super().__init__(plan)
        batch, keys, t = plan.batch, plan.keys, plan.batch["t"]
        state = self.state = {k: batch[k].clone() for k in keys}
        self.saved = {k: v.clone() for k, v in state.items()}

        def captured():
            sampler_begin_step(plan.times, plan.cells, t)
            work = batch.clone()
            for k in keys:
                work[k] = state[k]
            work["t"] = t
            for update in plan.updates:
                work = moved(update(work))
            for k in keys:
                state[k].copy_(work[k])

        self.step = CapturedStep(captured, warmup=1, device=t.device)

    def rewind(self) -> None:
        """(the warm-up run moved the state: it goes back to the start)"""
        for k, v in self.saved.items():
            self.state[k].copy_(v)
        self._rewind_plan()

    def run(self, steps: int) -> None:
        for _ in self._take(steps):
            self.step()

    def result(self):
        out = self.plan.batch.view()
        for k, v in self.state.items():
            out[k] = v.clone()
        return out


class CappedLoop(_Loop):
    """The steps as replays of ONE graph on cutoff graphs: the batch padded to ``e_cap`` edges, the neighbour list rebuilt inside the
    graph -- by the loop after every update of the plan, or by the model's own ``edge_index`` layer in every model call (it finds
    ``_nlist_state`` in the batch and builds the capped list).  The ghost graph's rows of the diffused tensors are never written back:
    its nodes stay where they are.

    Construction sizes, pads and captures; ``result()`` checks the capacity and unpads.  Padding collates integers as int64, so the
    padded mask of conditional sampling (``plan.fixed``) is made uint8 again here, once -- the form the kernels read, and no conversion
    joins the replayed step."""

    def __init__(self, plan: StepPlan, model, e_cap: int, r_max: float, criteria=None):
        super().__init__(plan)
        batch, keys = plan.batch, plan.keys
        dev = batch["_n_nodes"].device
        own = edge_layer_of(model)
        if own is not None:
            criteria, pos_key, build = replayable_criterion(own), own.key or keys[0], own.layer
        else:
            pos_key = keys[0]
            build = partial(computeEdgeIndex, r_max=r_max, key=pos_key, criteria=criteria)
        for k in SAMPLER_EDGE_KEYS:
            batch.pop(k)
        # eager, once: the sizes of the padded batch.  The same function, the same criterion, the draw of build 0 -- read from the
        # cells, which the eager path never advances, so no draw is consumed
        rng = builder_cells(dev)
        batch.data["_nlist_rng"] = rng
        new, attrs = build(batch.data, batch.attrs)
        batch.data.pop("_nlist_rng")
        batch.attrs.update(attrs)
        batch.update(new)
        n, e = batch.n_nodes, int(new["edge_index"].shape[1])
        if e > e_cap:
            raise EdgeCapacityExceeded(f"the first neighbour list has {e} edges: edge_capacity={e_cap} is too small")
        bucket = self.bucket = CappedBucket.around_list(batch, e_cap, pos_key, rng=rng)      # (the cells the sizing build read)
        padded = bucket.padded
        if plan.fixed is not None:
            padded.data[plan.fixed] = (padded[plan.fixed] != 0).to(torch.uint8)
        state = {k: padded[k] for k in keys}

        def relisted(b):
            # a fresh view of the padded batch with the moved tensors: what the model left in ``b`` (edge vectors, harmonics, radial
            # embeddings of the OLD list) stays behind, as the reference's loop drops it (:236-241)
            fresh = padded.view()
            for k in keys:
                fresh[k] = b[k]
            if own is None:      # in place, on the device, inside the capture (a model that owns its edge layer does this itself)
                computeEdgeIndexCapped(fresh.data, fresh.attrs, r_max=r_max, key=pos_key, criteria=criteria)
            return fresh

        def captured():
            sampler_begin_step(plan.times, plan.cells, padded["t"])
            work = padded.view()
            for update in plan.updates:
                work = relisted(update(work))
            for k in keys:
                state[k][:n].copy_(work[k][:n])

        self.padded, self.state, self.rng, self.n, self.first_edges = padded, state, rng, n, e
        self.saved = {k: v.clone() for k, v in state.items()}
        self.step = CapturedStep(captured, warmup=1, device=dev)

    def rewind(self) -> None:
        """(the warm-up run moved the state and drew: both go back to the start)"""
        for k, v in self.saved.items():
            self.state[k].copy_(v)
        self.rng.zero_()
        self._rewind_plan()

    def run(self, steps: int) -> None:
        for _ in self._take(steps):
            self.step()

    def result(self):
        self.bucket.check()
        out = self.bucket.real_graphs()
        for k, v in self.state.items():
            out[k] = v[:self.n].clone()
        return out


def make_loop(plan: StepPlan, model, moved, *, graph: bool, edge_capacity, r_max, criteria):
    """The loop of a sampler's arguments (``check_loop_args`` has seen them): ``graph`` with ``edge_capacity`` -- ``CappedLoop``, which
    does ``moved``'s work inside its captured step; ``graph`` -- ``StaticLoop``; else ``EagerLoop``."""
    if graph and edge_capacity is not None:
        return CappedLoop(plan, model, int(edge_capacity), float(r_max), criteria)
    if graph:
        return StaticLoop(plan, model, moved)
    return EagerLoop(plan, model, moved, criteria)
