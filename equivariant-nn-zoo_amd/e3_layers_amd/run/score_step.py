"""The protein score nets' training step (``config_diffusion_CA``, ``config_diffusion_backbone``) as replays of ONE HIP graph on a
capped neighbour list ("The replayed score step").

What the step does per batch (``e3_layers/run/sde_utils.py:143-171`` and ``:233-248`` of the reference): draw t per graph and
the noise z, noise the coordinates, run the network -- whose own ``edge_index`` layer rebuilds the neighbour list from the NOISED
coordinates --, the denoising loss, the backward, clip + Adam + EMA.  Eagerly that is host-bound (the list's size is read back, the
pair rule is evaluated over all pairs).  Captured, the list has a fixed capacity, and three things make that safe for training:

* a policy for a list that did not fit: the optimizer launch of the captured step takes the capped builder's overflow counter as a
  device-side VETO (``FusedAdamEMA.step(veto=...)``): from the first overflowed step on nothing is applied -- no weight moves on a
  truncated list -- until the host has looked;
* draws that can be repeated: t and z are counter-based (``sde_utils.sde_perturb_counter``: functions of seed, step number, graph
  / node, component), and so is the pair rule's random subset, so the vetoed steps are redone EAGERLY, in order, on exactly the
  noised batches they were vetoed on.  Dropping them instead would bias training: the largest lists belong to the smallest t;
* a record on the device: the step files its loss in a ring and the number of the first overflowed step (``e3k_score_step_record``);
  the host reads counter, number and ring in one synchronising copy every ``check_every`` steps.

The window protocol itself (``StepWindow``) knows nothing of the device: tests drive it with stub steps.
"""
from __future__ import annotations

import math
from typing import List, Optional, Sequence

import torch

from ..backend.graph import EdgeCapacityExceeded
from ..data.compute_edge import PairCriterion, check_edge_capacity
from .capped import EDGE_KEYS, REBUILT_KEYS, CappedBucket, edge_layer_of, real_graphs, replayable_criterion
from .graph_step import CapturedStep, copy_into, ghost_node_capacity, pad_batch
from .sde_utils import VPSDE, sde_perturb_counter


class StepWindow:
    """Replayed steps in windows of ``check_every``, with the overflowed tail of a window redone eagerly.

    ``device`` supplies four calls: ``replay(batch)`` (enqueue step; no synchronisation), ``read() -> (overflow count, first_bad,
    ring)`` (one synchronising read; ``ring[s % len(ring)]`` is the loss step ``s`` filed, ``first_bad`` the number of the first
    step whose list overflowed or -1), ``clear()`` (counter, ``first_bad`` and flags back to clean) and ``redo(batch, s) -> loss``
    (step ``s`` eagerly on the un-capped list).  Every step from ``first_bad`` to the window's end was vetoed on the device, so
    nothing was applied: those steps are redone in order, each exactly once, with their own step numbers as draw indices."""

    def __init__(self, device, check_every: int = 8, first_step: int = 0):
        self.device = device
        self.check_every = max(1, int(check_every))
        self.step = int(first_step)      # the number of the next step
        self.pending: list = []          # (step number, batch) of the current window
        self.losses: List[float] = []
        self.stats = dict(steps=0, windows=0, overflowed_windows=0, steps_redone=0)

    def __call__(self, batch) -> None:
        self.device.replay(batch)
        self.pending.append((self.step, batch))      # (held until the window is checked: a redone step runs on it)
        self.step += 1
        self.stats["steps"] += 1
        if len(self.pending) >= self.check_every:
            self.flush()

    def flush(self) -> None:
        if not self.pending:
            return
        over, first_bad, ring = self.device.read()
        first_bad = int(first_bad)
        start, count = self.pending[0][0], len(self.pending)
        losses = [float(ring[s % len(ring)]) for s, _ in self.pending]
        self.stats["windows"] += 1
        if int(over) != 0 or first_bad >= 0:
            if not start <= first_bad < start + count:
                raise RuntimeError(f"the device reports an overflow at step {first_bad}, outside the window [{start}, {start + count})")
            self.stats["overflowed_windows"] += 1
            self.device.clear()      # (before the eager steps: their optimizer launches must not find the veto standing)
            for s, batch in self.pending:
                if s >= first_bad:
                    losses[s - start] = float(self.device.redo(batch, s))
                    self.stats["steps_redone"] += 1
        self.losses.extend(losses)
        self.pending = []


def eager_score_step(model, sde: VPSDE, opt, batch, s: int, seed: int = 0, eps: float = 1e-5):
    """Step number ``s`` of a run on the un-padded ``batch``, eagerly: the perturbation kernel at draw index ``s``, the model (its
    own ``edge_index`` layer builds the un-capped list; a ``PairCriterion`` in it draws with index ``s``), the denoising loss with
    uniform weights, the backward, ``opt.step()``.  -> (loss tensor, number of edges of the list)."""
    from ..backend import ops
    from .parallel import backward_parameters

    pert, misc = sde_perturb_counter(sde, batch, seed, int(s), eps)
    own = edge_layer_of(model)
    if own is not None and isinstance(own.criterion, PairCriterion):
        own.criterion.reset(int(s))
    model.train(True)
    result = model(pert)
    loss = _loss_of(ops, sde, result, pert, misc, None)
    opt.grads.zero()
    backward_parameters(loss, opt.params)
    opt.step()
    return loss, int(result["edge_index"].shape[1])


def _loss_of(ops, sde, result, pert, misc, weight):
    total = None
    for key in sde.irreps:
        name = f"score_{key}"
        raw = result[name] if name in result else result["score"]
        term = ops.denoise_loss(raw, pert[key], misc["zs"][key], misc["std"], weight)
        total = term if total is None else total + term
    return total


def score_list_sizes(model, sde: VPSDE, batch, draws: Sequence[int], seed: int = 0, eps: float = 1e-5) -> List[int]:
    """The sizes of the un-capped neighbour lists the model's own ``edge_index`` layer builds for the un-padded ``batch`` noised at
    the draw indices ``draws`` (eager: one host read per draw)."""
    own = edge_layer_of(model)
    sizes = []
    for s in draws:
        pert, _ = sde_perturb_counter(sde, batch, seed, int(s), eps)
        if isinstance(own.criterion, PairCriterion):
            own.criterion.reset(int(s))
        new, _ = own.layer(pert.data, pert.attrs)
        sizes.append(int(new["edge_index"].shape[1]))
    return sizes


def edge_capacity_for(model, sde: VPSDE, batches, quantile: float = 0.99, draws: int = 8, seed: int = 0, eps: float = 1e-5) -> int:
    """``ReplayedScoreStep.capacity_for`` before the step exists (its constructor wants a capacity)."""
    return quantile_capacity([e for b in batches for e in score_list_sizes(model, sde, b, range(int(draws)), seed, eps)], quantile)


def quantile_capacity(sizes: Sequence[int], quantile: float = 0.99, multiple: int = 1024) -> int:
    """The ``quantile`` of the list sizes (the smallest size that at least that share of them does not exceed), rounded up to
    ``multiple``."""
    ordered = sorted(int(v) for v in sizes)
    if not ordered:
        raise ValueError("no list sizes")
    k = min(len(ordered) - 1, max(0, math.ceil(quantile * len(ordered)) - 1))
    return -(-ordered[k] // multiple) * multiple


class ReplayedScoreStep:
    """``step = ReplayedScoreStep(model, sde, opt, example, edge_capacity=...)``; ``step(step.pad(batch))`` per batch; ``step.flush()``
    before the weights are read.

    model: its tree starts with its own ``edge_index`` layer, carrying a ``data.PairCriterion`` or no criterion (a callback is
        refused, as the sampler refuses it); the position key and the cutoff are that layer's.
    example: an un-padded protein batch WITHOUT edges on the device; it fixes the bucket (number of graphs, node capacity).
    edge_capacity: slots of the capped list (``capacity_for`` proposes one).  node_capacity: overrides the sized node capacity.
    seed: of t and z (the pair rule has its own).  check_every: steps per window, i.e. between two synchronising reads.

    ``use_veto`` (class attribute, for tests): False withholds the veto argument from the captured optimizer step."""

    use_veto = True

    def __init__(self, model, sde: VPSDE, opt, example, *, edge_capacity: int, node_capacity: Optional[int] = None, seed: int = 0,
                 check_every: int = 8, eps: float = 1e-5):
        own = edge_layer_of(model)
        if own is None:
            raise ValueError("ReplayedScoreStep needs a model whose tree starts with its own edge_index layer (the protein score nets)")
        crit = replayable_criterion(own)
        if own.r_max is None:
            raise ValueError("the model's edge_index layer carries no cutoff (r_max)")
        self.model, self.sde, self.opt, self.layer, self.crit = model, sde, opt, own.layer, crit
        self.pos_key, self.r_max = own.key or "pos", float(own.r_max)
        self.seed, self.eps = int(seed), float(eps)
        self.dev = example[self.pos_key].device
        self._example = example
        self._node_capacity = node_capacity
        self.grown = 0
        self.window = StepWindow(self, check_every)
        self._capture(int(edge_capacity))

    # ------------------------------------------------------------------ sizes
    def list_sizes(self, batch, draws: Sequence[int]) -> List[int]:
        """The sizes of the un-capped lists of ``batch`` noised at the draw indices ``draws`` (eager: one host read per draw)."""
        return score_list_sizes(self.model, self.sde, batch, draws, self.seed, self.eps)

    def capacity_for(self, batches, quantile: float = 0.99, draws: int = 8) -> int:
        """An edge capacity for ``batches``: their lists built eagerly at the counter draws 0 .. ``draws`` - 1, the ``quantile`` of the
        sizes rounded up to 1024 (``edge_capacity_for`` is the same before there is a step to ask)."""
        return quantile_capacity([e for b in batches for e in self.list_sizes(b, range(int(draws)))], quantile)

    def pad(self, batch):
        """The padded batch of this bucket for a protein batch without edges: an empty edge list and ``e_cap`` ghost edges (the
        in-graph build rewrites all of them).  Raises ValueError for a batch that does not fit the node capacity."""
        b = batch.view()
        for k in EDGE_KEYS:
            b.pop(k)
        dev = b[self.pos_key].device
        b.data["edge_index"] = torch.zeros(2, 0, dtype=torch.int64, device=dev)
        b.attrs["_n_edges"] = ("graph", "1x0e")
        b.data["_n_edges"] = torch.zeros(len(b), 1, dtype=torch.int64, device=dev)
        padded = pad_batch(b, self.n_cap, self.e_cap, key=self.pos_key)
        padded._score_source = batch      # (what a redone step runs on)
        return padded

    # ------------------------------------------------------------------ capture
    def _capture(self, e_cap: int) -> None:
        from ..backend import memo, ops
        from ..backend import lib as L
        from .parallel import backward_parameters

        dev, opt = self.dev, self.opt
        self.e_cap = e_cap
        # eager, once: the example's lists at a few draws -- the smallest sizes the ghost graph, and the first that fits is the draw
        # the warm-up and the recording run at (a warm-up list that overflowed would raise from the eager index checks)
        probe = self.list_sizes(self._example, range(8))
        fits = [s for s, e in enumerate(probe) if e <= e_cap]
        if not fits:
            raise EdgeCapacityExceeded(f"the example's lists at the draws 0..7 have {min(probe)}..{max(probe)} edges: "
                                       f"edge_capacity={e_cap} is too small")
        # the ghost nodes for the smallest list to expect, as the sampler's capped loop sizes them
        self.n_cap = int(self._node_capacity) if self._node_capacity is not None else \
            ghost_node_capacity(int(self._example[self.pos_key].shape[0]), e_cap - min(probe))
        self._padded_example = self.pad(self._example)
        static = self.static = self._padded_example.clone()
        self.keys = [k for k in static.keys() if torch.is_tensor(static[k]) and k not in REBUILT_KEYS]
        ring_len = self.window.check_every
        bucket = CappedBucket(static, self.pos_key, rng=True)
        self.nlist_state, self.nlist_rng = bucket.state, bucket.rng
        self.cells = torch.tensor([self.window.step, -1], dtype=torch.int64, device=dev)      # (step, first_bad)
        self.ring = torch.zeros(ring_len, dtype=torch.float32, device=dev)
        weight = static["_node_weight"]
        lib = L.load()
        warming = self._warming = [False]

        def captured():
            memo.forget(static)      # the static tensors' contents change between replays (the recording rule of backend/memo.py)
            work = bucket.view()
            pert, misc = sde_perturb_counter(self.sde, work, self.seed, self.cells, self.eps)
            self.model.train(True)
            result = self.model(pert)      # (its edge layer finds _nlist_state: the capped build, inside the capture)
            loss = _loss_of(ops, self.sde, result, pert, misc, weight)
            L.check(lib.e3k_score_step_record(L.ptr(loss), L.ptr(self.nlist_state[1:]), L.ptr(self.cells), L.ptr(self.ring), ring_len,
                                              L.stream_ptr()), "e3k_score_step_record")
            opt.grads.zero()
            backward_parameters(loss, opt.params)
            opt.step(veto=self.nlist_state[1:]) if self.use_veto else opt.step()
            if warming[0] and not torch.cuda.is_current_stream_capturing():      # every warm-up run at the draw that fits
                self.nlist_rng.fill_(self._fit_draw)
                self.cells[:1].fill_(self._fit_draw)
            return loss

        assert bucket.n_graphs >= 1
        self._fit_draw = fits[0]
        self._quietly(lambda: setattr(self, "captured", CapturedStep(captured, warmup=2, device=dev)))

    def _quietly(self, record) -> None:
        """``record()`` -- the recording of the step with its eager warm-up runs -- as no step of the run: every warm-up run at the draw
        that fits; afterwards the optimizer, the cells and the draw indices are where the run left them."""
        opt = self.opt
        tensors = [opt.flat, opt.exp_avg, opt.exp_avg_sq, opt.state] + ([opt.ema] if opt.ema is not None else [])
        held = [t.clone() for t in tensors]
        self._warming[0] = True
        self.nlist_rng.fill_(self._fit_draw)
        self.cells.copy_(torch.tensor([self._fit_draw, -1], dtype=torch.int64))
        try:
            record()
        finally:
            self._warming[0] = False
        torch.cuda.synchronize(self.dev)
        with torch.no_grad():
            for t, h in zip(tensors, held):
                t.copy_(h)
            self.nlist_state.zero_()
            self.nlist_rng.fill_(self.window.step)
            self.cells.copy_(torch.tensor([self.window.step, -1], dtype=torch.int64))

    def grow(self, factor: float = 1.25) -> None:
        """Re-pads and re-captures at ``factor`` x the edge capacity, rounded up to 1024 (batches padded before must be padded again).
        The pending window is checked first.  When to call it is the caller's decision (``stats`` says how often windows overflow)."""
        self.flush()
        self.grown += 1
        self.captured = None
        self._capture(-(-int(math.ceil(self.e_cap * float(factor))) // 1024) * 1024)

    # ------------------------------------------------------------------ the device side of StepWindow
    def _load(self, padded) -> None:
        """The padded batch into the static tensors."""
        copy_into(self.static, padded, self.keys, hint="pad() again after grow()")

    def replay(self, padded) -> None:
        if self.captured.stale:
            # a knot table the graph interpolates from was refined: CapturedStep would run this step eagerly and record again.  An
            # eager step on the capped list raises from the index checks when the list does not fit -- possibly half way through; so
            # the window is checked, the step is recorded again on the example as no step of the run, and this step is a replay
            # like any other
            self.window.flush()
            self._load(self._padded_example)
            self.captured.recaptures += 1
            self._quietly(lambda: self.captured._capture(1))
        self._load(padded)
        try:
            self.captured()
        except EdgeCapacityExceeded:
            pass      # (an earlier replay's flag came home while this one was issued: the device cells hold the record, flush() acts)

    def read(self):
        packed = torch.cat([self.nlist_state[1:].double(), self.cells[1:].double(), self.ring.double()]).cpu()      # the one read
        return int(packed[0]), int(packed[1]), packed[2:].tolist()

    def _clear(self) -> None:
        try:
            check_edge_capacity(self.nlist_state)      # the counter, the persistent flag's bit and the flag copies on their way home
        except EdgeCapacityExceeded:
            pass

    def clear(self) -> None:
        self._clear()
        self.cells[1:].fill_(-1)

    def redo(self, padded, s: int):
        source = getattr(padded, "_score_source", None)
        return self.eager_step(source if source is not None else self._unpadded(padded), s)

    def _unpadded(self, padded):
        return real_graphs(padded, drop=REBUILT_KEYS)

    # ------------------------------------------------------------------ the caller's side
    def eager_step(self, batch, s: int):
        """Step number ``s`` on the un-padded ``batch`` (``eager_score_step``); -> the loss tensor."""
        loss, self.last_edges = eager_score_step(self.model, self.sde, self.opt, batch, s, self.seed, self.eps)
        return loss

    def __call__(self, padded) -> None:
        """Copies the padded batch into the static tensors and replays; no host synchronisation, except every ``check_every``-th
        call, which checks the window.  A reference to the batch is kept until then."""
        self.window(padded)

    def flush(self) -> None:
        self.window.flush()

    @property
    def losses(self) -> List[float]:
        """The per-step losses so far, redone steps with their eager values (checks the pending window first)."""
        self.flush()
        return list(self.window.losses)

    @property
    def stats(self) -> dict:
        return dict(self.window.stats, recaptures=self.grown + (self.captured.recaptures if self.captured is not None else 0))
