"""Predictor-corrector sampling of the reverse VP-SDE — the loop of
``e3_layers/run/sde_sampling.py:185-244``, kept on the device.

What the reference does per reverse step (``pc_sampler`` :229-242): set the time, run the corrector
(Langevin, :117-143), drop ``edge_index`` / ``edge_vector``, run the predictor (Euler-Maruyama on the reverse
SDE, :98-105 + ``sde_utils.py:104-119``), drop the edges again — the model's own ``edge_index`` layer (or the
dataset's preprocess functions) rebuilds the neighbour list from the moved positions: 2·N network
evaluations, each latency-bound.

MI355X-first changes, same arithmetic:
* the edge rebuild runs the device radius-graph kernels (``data/compute_edge.py``), no host round trip of
  positions; the CSR topology the fused convolution needs is rebuilt with it;
* when the edge set cannot change (fully connected molecules: ``config_diffusion`` preprocesses with
  ``r_max=9999``) the edges and topology are built once and one whole corrector+predictor step — two
  network evaluations, noise draws and updates — is captured in a HIP graph and replayed N times
  (``graph=True``): the step time falls from launch-bound to GPU-bound;
* the time ``t`` lives in a device tensor that is updated in place, so the captured graph sees it.

Noise comes from ``generator`` (or an injected ``noise_fn(shape)`` — the parity tests feed the oracle the
same draws).  The reference's corrector evaluates the score ``n_steps`` times on the *unchanged* batch
(:131-142 never writes ``x`` back inside the loop); here every inner step sees the updated positions, which
is identical for the default ``n_steps=1``.

``get_pc_sampler(seed=...)`` is the seeded form: the noise of reverse step i is counter-based (``csrc/e3k_draw.h``; the layout is
restated in ``run/sde_utils.py``), the arithmetic around each model call is one HIP launch per diffusion key
(``csrc/e3k_sampler.hip``), and the step's time and number live in device cells that a one-workgroup launch advances -- the host
copies nothing per step.  The corrector forms its batch-wide norms over the real rows only, so the Langevin corrector is served on
the capped replay too, and the eager loop, the static-edge graph and the capped replay see the same draws at one seed.

``get_pc_sampler(fixed="name")`` samples conditionally (inpainting; the replacement method of Song et al. 2021, section I.2): the nodes
whose per-node field ``name`` is not zero keep the values the batch holds on entry.  After the prior and after every corrector and
predictor update their rows are overwritten with the known values perturbed to the step's noise level, and with the known values
themselves when the run ends.  Seeded, the replacement is a branch of the update's own kernel: the replayed step has no launch more.

``get_ode_sampler(method="heun" | "euler", n_steps=K)`` integrates the probability-flow ODE of the same SDE on a fixed grid of K steps
instead (the ``"ode"`` method the reference's ``get_sampling_fn`` dispatches to and never defines, :247-286): no noise after the prior,
one launch per key and stage around each model call, the same three loops -- ``_run_loop`` drives them for both samplers.
"""
from __future__ import annotations

from functools import partial
from typing import Callable, Dict, Optional, Sequence

import torch

from ..backend.graph import TOPO_KEYS, EdgeCapacityExceeded
from ..data.compute_edge import PairCriterion, computeEdgeIndex, computeEdgeIndexCapped
from .capped import EDGE_KEYS, CappedBucket, builder_cells, edge_layer_of, replayable_criterion
from .graph_step import CapturedStep
from .sde_utils import (VPSDE, _node_t, _randn, fixed_rows, get_score_fn, langevin_step_counter, ode_euler_step, ode_heun_finish,
                        prior_sampling, prior_sampling_counter, replace_fixed, reverse_step, reverse_step_counter, sampler_begin_step)

class _Registry(dict):
    """name -> class table with a decorator: ``@table.register(name="langevin")`` (bare ``@table.register`` uses the
    class name); a name is registered once."""

    def __init__(self, kind: str):
        super().__init__()
        self.kind = kind

    def register(self, cls=None, *, name=None):
        def add(c):
            key = name or c.__name__
            if key in self:
                raise ValueError(f"{self.kind} {key!r} is already registered")
            self[key] = c
            return c
        return add if cls is None else add(cls)


_PREDICTORS, _CORRECTORS = _Registry("predictor"), _Registry("corrector")
# the reference's public names (e3_layers/run/sde_sampling.py:14-60)
register_predictor, register_corrector = _PREDICTORS.register, _CORRECTORS.register
get_predictor, get_corrector = _PREDICTORS.__getitem__, _CORRECTORS.__getitem__


class Predictor:
    def __init__(self, sde: VPSDE, score_fn):
        self.sde, self.score_fn = sde, score_fn

    def update_fn(self, batch, generator=None, noise_fn=None):
        raise NotImplementedError


class Corrector:
    def __init__(self, sde: VPSDE, score_fn, snr: float, n_steps: int):
        self.sde, self.score_fn, self.snr, self.n_steps = sde, score_fn, snr, n_steps

    def update_fn(self, batch, generator=None, noise_fn=None):
        raise NotImplementedError


@register_predictor(name="euler_maruyama")
class EulerMaruyamaPredictor(Predictor):
    def update_fn(self, batch, generator=None, noise_fn=None):
        return reverse_step(self.sde, self.score_fn, batch, generator, noise_fn)


@register_predictor(name="none")
class NonePredictor(Predictor):
    def update_fn(self, batch, generator=None, noise_fn=None):
        return batch


@register_corrector(name="langevin")
class LangevinCorrector(Corrector):
    def __init__(self, sde, score_fn, snr, n_steps):
        super().__init__(sde, score_fn, snr, n_steps)
        if not isinstance(sde, VPSDE):
            raise NotImplementedError(f"SDE class {sde.__class__.__name__} not yet supported.")

    def update_fn(self, batch, generator=None, noise_fn=None):
        sde = self.sde
        t = _node_t(batch)
        timestep = (t * (sde.N - 1) / sde.T).long()
        alpha = sde.alphas.to(t.device)[timestep]
        for _ in range(self.n_steps):
            scores = self.score_fn(batch)
            for key in sde.irreps:
                x, grad = batch[key], scores[f"score_{key}"]
                noise = _randn(x, generator, noise_fn)
                grad_norm = torch.norm(grad.reshape(grad.shape[0], -1), dim=-1).mean()
                noise_norm = torch.norm(noise.reshape(noise.shape[0], -1), dim=-1).mean()
                step_size = (self.snr * noise_norm / grad_norm) ** 2 * 2 * alpha
                batch[key] = x + step_size * grad + torch.sqrt(step_size * 2) * noise
        return batch


@register_corrector(name="none")
class NoneCorrector(Corrector):
    def update_fn(self, batch, generator=None, noise_fn=None):
        return batch


SAMPLER_EDGE_KEYS = EDGE_KEYS + TOPO_KEYS      # what the loop drops after every update: the list and the CSR topology built on it


def get_pc_sampler(sde: VPSDE, predictor, corrector, inverse_scaler: Callable = None, snr: float = 0.16,
                   n_steps: int = 1, continuous: bool = True, eps: float = 1e-3,
                   preprocess: Sequence[Callable] = (), static_edges: bool = False, graph: bool = False,
                   n_iter: Optional[int] = None, edge_capacity: Optional[int] = None, r_max: Optional[float] = None,
                   criteria=None, seed: Optional[int] = None, fixed: Optional[str] = None):
    """``pc_sampler(model, batch, generator=None, noise_fn=None) -> (batch, n_function_evaluations)``.

    seed: the seeded form (at most 64 bits).  The prior and every step's noise are counter-based draws of (seed, step, node,
        component) -- ``run/sde_utils.prior_sampling_counter``, ``langevin_step_counter``, ``reverse_step_counter`` -- instead of a
        generator's, so ``generator`` and ``noise_fn`` are refused; the predictor and the corrector are the built-in classes (any
        other class is refused: its ``update_fn`` draws from a generator), ``n_steps`` is 1 with the Langevin corrector (the draw
        layout holds one corrector draw per step).  With ``edge_capacity`` the Langevin corrector is served: its norms run over the real
        rows.  It should differ from the pair criterion's seed, or a node's noise and its pairs' Bernoulli draws share a chain.

    fixed: conditional sampling.  The name of a per-node field of the batch (``("node", "1x0e")``, any dtype): a node whose entry is
        not zero is FIXED.  The known clean values x0 are the batch's own values of the diffused keys on entry, in the model's scaled
        space.  With m(t) = exp(lm(t)), s(t) = sqrt(-expm1(2 lm(t))): the prior's fixed rows are m(T) x0 + s(T) z with the prior's
        own z; after the corrector's and after the predictor's update of step i (time t_i) they become m(t_i) x0 + s(t_i) z with a
        fresh z each (a ``None`` class does nothing, so nothing is replaced after it); when the run ends they are x0, bit for bit.
        The Langevin norms run over all real rows, the fixed ones included.  Served by every loop, seeded (one launch per key, as
        without: the draw layout's blocks 2 and 3) or not (``noise_fn`` sees the prior per key, then per step: corrector per key,
        replacement per key, predictor per key, replacement per key; custom classes included).  The mask and x0 travel in the
        working copy of the batch as node fields (``fixed`` as uint8, ``known_<key>``), so the capped loop pads them with the rest;
        the result carries the caller's fields only.  None: nothing changes, in bits or in launches.

    preprocess: the dataset's ``(data, attrs) -> (data, attrs)`` functions (``data_config.preprocess``) that
        rebuild ``edge_index`` when the model tree has no ``edge_index`` layer of its own.
    static_edges: the edge set does not depend on the positions (fully connected graphs): build it once.
    graph: with ``static_edges``, capture one corrector+predictor step in a HIP graph and replay it.
    edge_capacity: with ``graph`` on CUTOFF graphs (no ``static_edges``): the batch is padded with a ghost graph to this many edges
        (``run/graph_step.pad_batch``) and the captured step rebuilds the neighbour list from the moved positions with the capped
        device builder (``data/compute_edge.computeEdgeIndexCapped``).  A list that outgrew the capacity during the loop raises
        ``EdgeCapacityExceeded`` when the loop ends.  The ghost nodes would take part in batch-wide reductions, so only per-node
        updates are served: a corrector other than ``NoneCorrector`` is refused.  The positions are the first diffusion key of the
        SDE.  A model whose tree starts with an ``edge_index`` layer of its own (the protein score nets) keeps it: the loop does not
        rebuild, the model's layer finds the padded batch and rebuilds through the capped builder, with the layer's own cutoff, key
        and pair criterion -- which must be a ``data.PairCriterion`` (``config_diffusion_CA.pair_criterion()``), not a callback.
    r_max: the cutoff of the capped builder; required with ``edge_capacity`` (``preprocess`` is not consulted for it).  Not
        consulted when the model owns its ``edge_index`` layer.
    criteria: with ``edge_capacity``, a ``data.PairCriterion`` for the list the loop rebuilds itself.  Build k of a run draws with
        index k, counted from 0, replayed or eager (the eager loop resets the criterion it finds here or in the model's layer).
    n_iter: stop after this many of the ``sde.N`` reverse steps (harness addition: benchmarks and parity tests
        time / check the first steps of the N=1000 schedule instead of shrinking N, which changes dt and betas).
    """
    inverse_scaler = inverse_scaler or (lambda b: b)
    predictor = predictor or NonePredictor
    corrector = corrector or NoneCorrector
    _check_loop_args(graph, static_edges, edge_capacity, r_max, criteria,
                     norms_served=corrector is NoneCorrector or (seed is not None and corrector is LangevinCorrector))
    seeded = seed is not None
    if seeded:
        if not 0 <= int(seed) < 1 << 64:
            raise ValueError("seed: at most 64 bits")
        if predictor not in (EulerMaruyamaPredictor, NonePredictor) or corrector not in (LangevinCorrector, NoneCorrector):
            raise ValueError("seed: only the built-in predictors and correctors draw counter-based noise "
                             f"(got {predictor.__name__}, {corrector.__name__})")
        if corrector is LangevinCorrector and n_steps != 1:
            raise ValueError("seed: the draw layout holds one corrector draw per reverse step, and the capped loop would rebuild the "
                             "list between inner corrector steps where the eager loop does not: n_steps must be 1")

    rebuild_edges, moved = _edge_plumbing(preprocess, static_edges)
    steps = sde.N if n_iter is None else min(int(n_iter), sde.N)

    def pc_sampler(model, batch, generator=None, noise_fn=None):
        if seeded and (generator is not None or noise_fn is not None):
            raise ValueError("seed: the noise is counter-based; generator and noise_fn have nothing to feed")
        batch = batch.clone()
        dev = batch["_n_nodes"].device
        batch.attrs["t"] = ("graph", "1x0e")
        given = None if fixed is None else _condition(sde, batch, fixed)
        if seeded:
            batch = prior_sampling_counter(sde, batch, seed, fixed=fixed)
        else:
            batch = prior_sampling(sde, batch, generator, noise_fn)
            if fixed is not None:      # m(T) x0 + s(T) z with the prior's own z
                lm = sde.log_mean_coeff(torch.tensor(float(sde.T)))
                m, s = torch.exp(lm), torch.sqrt(1.0 - torch.exp(2.0 * lm))
                rows = fixed_rows(batch, fixed)
                for key in sde.irreps:
                    z = batch[key]
                    batch[key] = torch.where(rows, m * batch[f"known_{key}"].to(z.dtype) + s * z, z)
        sde.alphas = sde.alphas.to(dev)      # resident before any capture (no pageable host copy inside a graph)
        timesteps = torch.linspace(sde.T, eps, sde.N, device=dev)
        score_fn = get_score_fn(sde, model, train=False)
        pred, corr = predictor(sde, score_fn), corrector(sde, score_fn, snr, n_steps)
        batch["t"] = torch.empty(len(batch), 1, device=dev)
        if static_edges:
            _static_topology(batch, rebuild_edges)
        t_dev = batch["t"]
        keys = list(sde.irreps)
        _reset_criteria(model, criteria)

        if seeded:
            # the step's time and number: device cells (next step, step in use) that the step's first launch advances
            cells = torch.zeros(2, dtype=torch.int64, device=dev)
            times = timesteps.contiguous()
            same = lambda b: b      # noqa: E731  (the None classes)
            corr_fn = (partial(langevin_step_counter, sde, model, seed=seed, draw=cells, snr=snr, fixed=fixed)
                       if corrector is LangevinCorrector else same)
            pred_fn = partial(reverse_step_counter, sde, model, seed=seed, draw=cells, fixed=fixed) if predictor is EulerMaruyamaPredictor else same
        else:
            corr_fn = lambda b: corr.update_fn(b, generator, noise_fn)      # noqa: E731
            pred_fn = lambda b: pred.update_fn(b, generator, noise_fn)      # noqa: E731
            if fixed is not None:      # the replacement follows every update that is one (a None class draws nothing)
                def replaced(update):
                    def fn(b):
                        b = update(b)
                        return replace_fixed(sde, b, fixed, {k: b[f"known_{k}"] for k in keys}, generator, noise_fn)
                    return fn

                corr_fn = corr_fn if corrector is NoneCorrector else replaced(corr_fn)
                pred_fn = pred_fn if predictor is NonePredictor else replaced(pred_fn)

        with torch.no_grad():
            batch = _run_loop(batch, model, [corr_fn, pred_fn], keys, timesteps, steps, moved, t_dev, graph=graph,
                              edge_capacity=edge_capacity, r_max=r_max, criteria=criteria, header=(times, cells) if seeded else None,
                              fixed=fixed)
        if fixed is not None:
            batch = _release(sde, batch, fixed, given)
        return inverse_scaler(batch), steps * (n_steps + 1)

    return pc_sampler


def get_ode_sampler(sde: VPSDE, inverse_scaler: Callable = None, method: str = "heun", *, n_steps: int, eps: float = 1e-3,
                    preprocess: Sequence[Callable] = (), static_edges: bool = False, graph: bool = False,
                    n_iter: Optional[int] = None, edge_capacity: Optional[int] = None, r_max: Optional[float] = None,
                    criteria=None, seed: Optional[int] = None):
    """``ode_sampler(model, batch, generator=None, noise_fn=None) -> (batch, n_function_evaluations)``: fixed-step integration of the
    probability-flow ODE of the VP-SDE, ``dx/dt = -0.5 beta(t) [x + score(x, t)]`` -- the deterministic flow with the reverse SDE's
    marginals.  With the head convention ``score = -raw / s(t) - x`` the drift is ``d(raw, t) = (0.5 beta(t)) (raw / s(t))``
    (``run/sde_utils.ode_euler_step``, ``ode_heun_finish``; ``csrc/e3k_sampler.hip``).

    method: ``"euler"`` (``x + h d1``; one model call per step) or ``"heun"`` (stage A as Euler's, stage B ``x + (0.5 h) (d1 + d2)`` with
        ``d2`` at the stage-A state and ``t_{k+1}``; two model calls per step, every step, the last included: ``s(eps) > 0``).
    n_steps: the steps of the run, required: the grid is ``linspace(sde.T, eps, n_steps + 1)``, step k goes from ``t_k`` to
        ``t_{k+1}``.  It has nothing to do with ``sde.N``, which only names the prior's draw index.  How many steps a trained network
        needs for a given sample quality is not assessed here.
    seed: selects only the prior.  Seeded: ``prior_sampling_counter`` -- the ``x_T`` bits of ``get_pc_sampler(seed=...)`` at the same
        seed; ``generator`` and ``noise_fn`` are refused.  Unseeded: ``prior_sampling`` from ``generator`` / ``noise_fn`` (one draw per
        key).  After the prior the loop is deterministic and the same either way: the step's time and number live in device cells,
        the update is one launch per key and stage.
    preprocess, static_edges, graph, edge_capacity, r_max, criteria, n_iter: the loops of ``get_pc_sampler``, with its meaning and
        its refusals (``n_iter`` stops after this many of the ``n_steps`` steps).  The neighbour list is rebuilt from the moved
        positions after stage A and again after stage B, as that loop does after its corrector and its predictor.  Ghost rows of a
        padded batch never move.

    The log-likelihood of a batch under the same flow -- the divergence of this drift integrated along it, from the data to the prior --
    is ``run/likelihood.get_likelihood_fn``, which drives these loops and step kernels on the ascending grid.

    Out of scope: conditional sampling (there is no ``fixed`` argument: a deterministic replacement rule for the fixed rows is a design
    question of its own)."""
    inverse_scaler = inverse_scaler or (lambda b: b)
    if method not in ("euler", "heun"):
        raise ValueError(f"ODE method {method!r} unknown (euler, heun)")
    if int(n_steps) < 1:
        raise ValueError(f"n_steps: at least one step (got {n_steps})")
    n_steps = int(n_steps)
    _check_loop_args(graph, static_edges, edge_capacity, r_max, criteria)
    if seed is not None and not 0 <= int(seed) < 1 << 64:
        raise ValueError("seed: at most 64 bits")
    rebuild_edges, moved = _edge_plumbing(preprocess, static_edges)
    steps = n_steps if n_iter is None else min(int(n_iter), n_steps)

    def ode_sampler(model, batch, generator=None, noise_fn=None):
        if seed is not None and (generator is not None or noise_fn is not None):
            raise ValueError("seed: the prior is counter-based; generator and noise_fn have nothing to feed")
        batch = batch.clone()
        dev = batch["_n_nodes"].device
        batch.attrs["t"] = ("graph", "1x0e")
        if seed is not None:
            batch = prior_sampling_counter(sde, batch, seed)
        else:
            batch = prior_sampling(sde, batch, generator, noise_fn)
        # fp32 on the device (what the kernels read); torch's default dtype on the host, where float64 is the tests' reference
        times = torch.linspace(sde.T, eps, n_steps + 1, device=dev, dtype=torch.float32 if dev.type == "cuda" else None)
        batch["t"] = torch.empty(len(batch), 1, device=dev, dtype=times.dtype)
        if static_edges:
            _static_topology(batch, rebuild_edges)
        _reset_criteria(model, criteria)
        cells = torch.zeros(2, dtype=torch.int64, device=dev)
        if method == "euler":
            updates = [partial(ode_euler_step, sde, model, times=times, cells_or_step=cells)]
        else:
            kept = {}      # stage A's (x, d1) per key: made and used inside one step (one captured step on the replays)
            updates = [partial(ode_euler_step, sde, model, times=times, cells_or_step=cells, keep=kept),
                       partial(ode_heun_finish, sde, model, kept=kept, times=times, cells_or_step=cells)]
        with torch.no_grad():
            # the step header walks the first n_steps entries: a run replayed past its schedule stands still
            batch = _run_loop(batch, model, updates, list(sde.irreps), times, steps, moved, batch["t"], graph=graph,
                              edge_capacity=edge_capacity, r_max=r_max, criteria=criteria, header=(times[:n_steps], cells))
        return inverse_scaler(batch), steps * len(updates)

    return ode_sampler


def _check_loop_args(graph, static_edges, edge_capacity, r_max, criteria, norms_served: bool = True) -> None:
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


def _edge_plumbing(preprocess, static_edges: bool):
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


def _static_topology(batch, rebuild_edges) -> None:
    """(``static_edges``: the list and the CSR topology on it are built once, before the loop)"""
    from ..backend.graph import build_topology

    if "edge_index" not in batch:
        rebuild_edges(batch)
    if "_e3k_dst_ptr" not in batch and batch["edge_index"].is_cuda:
        batch.update(build_topology(batch["edge_index"], batch.n_nodes).as_dict())


def _reset_criteria(model, criteria) -> None:
    own = edge_layer_of(model)
    for crit in (criteria, own and own.criterion):
        if isinstance(crit, PairCriterion):
            crit.reset()      # build k of this run draws with index k


def _run_loop(batch, model, updates, keys, timesteps, steps: int, moved, t_dev, *, graph: bool, edge_capacity, r_max, criteria,
              header=None, fixed=None, zero=()):
    """The three loop drivers of the samplers: ``steps`` steps, each the ``updates`` (``batch -> batch``: corrector and predictor, or the
    ODE's stages) in order with ``moved`` after every one -- eager; one captured step replayed (``graph``: the edge set is static);
    ``CappedLoop`` (``graph`` with ``edge_capacity``: cutoff graphs, the list rebuilt inside the captured step, which does ``moved``'s
    work itself).  ``keys``: the tensors the updates move; ``t_dev``: the batch's time tensor.

    ``header``: ``(times, cells)`` -- every step begins with ``sampler_begin_step(times, cells, t_dev)`` on the device, and replays
    are bare.  None: the host copies ``timesteps[i]`` into ``t_dev`` before step i.  ``zero``: tensors the updates accumulate into
    (the likelihood's integral): a replayed loop's warm-up step added to them, so they go back to zero with the cells.
    -> the batch after the last step."""
    def one_step(b):
        for update in updates:
            b = moved(update(b))
        return b

    if graph and edge_capacity is not None:
        loop = CappedLoop(batch, model, updates, keys, float(timesteps[0]), int(edge_capacity), float(r_max), criteria, seeded=header,
                          fixed=fixed, zero=zero)
        loop.rewind()
        loop.run(timesteps, steps)
        return loop.result()
    if graph:
        # static buffers: the diffused tensors and t; the step writes its result back into them
        state = {k: batch[k].clone() for k in keys}

        def captured():
            work = batch.clone()           # model layers add keys: work on a copy, keep `batch` pristine
            for k in keys:
                work[k] = state[k]
            work["t"] = t_dev
            if header is not None:
                sampler_begin_step(header[0], header[1], t_dev)
            work = one_step(work)
            for k in keys:
                state[k].copy_(work[k])

        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            saved = {k: v.clone() for k, v in state.items()}
            t_dev.fill_(float(timesteps[0]))
            captured()                     # warm-up (allocations, plan creation) outside the capture
            for k in keys:
                state[k].copy_(saved[k])
            if header is not None:
                header[1].zero_()          # (the warm-up was step 0: the run starts there again)
            for acc in zero:
                acc.zero_()
        torch.cuda.current_stream().wait_stream(side)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            captured()
        for k in keys:                     # the capture pass itself does not execute; restore anyway
            state[k].copy_(saved[k])
        for i in range(steps):
            if header is None:
                t_dev.copy_(timesteps[i].expand_as(t_dev))
            g.replay()
        for k in keys:
            batch[k] = state[k]
        return batch
    for i in range(steps):
        if header is not None:
            sampler_begin_step(header[0], header[1], t_dev)
        else:
            t_dev.copy_(timesteps[i].expand_as(t_dev))
        batch["t"] = t_dev
        batch = one_step(batch)
    return batch


def _condition(sde: VPSDE, batch, fixed: str):
    """Conditional sampling's fields in the sampler's working copy of the batch: ``known_<key>`` = the diffused keys' values on entry
    (with the key's attrs) and the mask ``fixed`` as uint8 [N, 1], the form the kernels read.  -> what the caller held under those
    names, for ``_release``."""
    if fixed not in batch:
        raise ValueError(f"fixed: the batch has no field {fixed!r}")
    if batch.attrs.get(fixed, ("",))[0] != "node":
        raise ValueError(f"fixed: {fixed!r} is not a per-node field (attrs {batch.attrs.get(fixed)!r})")
    missing = [k for k in sde.irreps if k not in batch]
    if missing:
        raise ValueError(f"fixed: the batch holds no known values for {missing}")
    mask = batch[fixed]
    n = int(batch[next(iter(sde.irreps))].shape[0])
    if mask.dim() < 1 or mask.shape[0] != n or mask.numel() != n:
        raise ValueError(f"fixed: {fixed!r} has shape {tuple(mask.shape)} for {n} nodes (one entry per node)")
    names = [fixed] + [f"known_{k}" for k in sde.irreps]
    given = {name: (batch[name], batch.attrs.get(name)) for name in names if name in batch}
    for key in sde.irreps:
        batch.attrs[f"known_{key}"] = batch.attrs[key]
        batch[f"known_{key}"] = batch[key].float() if batch[key].is_cuda else batch[key].clone()
    batch[fixed] = (mask.reshape(-1, 1) != 0).to(torch.uint8)
    return given


def _release(sde: VPSDE, batch, fixed: str, given):
    """The end of a conditioned run: the fixed rows are the known values, bit for bit (one ``torch.where`` per key, outside any
    graph), and the batch carries under ``fixed`` / ``known_<key>`` what the caller put there, nothing else."""
    rows = fixed_rows(batch, fixed)
    for key in sde.irreps:
        batch[key] = torch.where(rows, batch[f"known_{key}"].to(batch[key].dtype), batch[key])
        batch.pop(f"known_{key}")
    for name, (value, attrs) in given.items():
        if attrs is not None:
            batch.attrs[name] = attrs
        batch[name] = value
    return batch


class CappedLoop:
    """The reverse steps as replays of ONE graph on cutoff graphs: the batch padded to ``e_cap`` edges, the neighbour list rebuilt
    inside the graph -- by the loop after every update in ``updates`` (corrector, predictor), or by the model's own ``edge_index``
    layer in every model call (it finds ``_nlist_state`` in the batch and builds the capped list).  The ghost graph's rows of the
    diffused tensors are never written back: its nodes stay where they are.

    Construction sizes, pads and captures (``t0``: the time of the warm-up step); ``rewind()`` puts the state and the draw index
    back on the start, ``run()`` replays, ``result()`` checks the capacity and unpads (``tools/sample_bench.py`` times ``run`` alone)."""

    def __init__(self, batch, model, updates, keys, t0: float, e_cap: int, r_max: float, criteria=None, seeded=None, fixed=None,
                 zero=()):
        """``seeded``: ``(times, cells)`` of the seeded sampler -- the captured step then begins with ``e3k_sampler_begin_step``, which
        sets the time from the table and advances the cells, and ``run`` is replays only.  ``fixed``: the name of conditional
        sampling's mask field; padding collates integers as int64, so the padded mask is made uint8 again here, once -- the form the
        kernels read, and no conversion joins the replayed step.  ``zero``: the tensors the updates accumulate into; ``rewind()`` zeroes
        them."""
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
        batch["t"] = torch.full((len(batch), 1), float(t0), device=dev)
        bucket = self.bucket = CappedBucket.around_list(batch, e_cap, pos_key, rng=rng)      # (the cells the sizing build read)
        padded = bucket.padded
        if fixed is not None:
            padded.data[fixed] = (padded[fixed] != 0).to(torch.uint8)
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
            if seeded is not None:
                sampler_begin_step(seeded[0], seeded[1], padded["t"])
            work = padded.view()
            for update in updates:
                work = relisted(update(work))
            for k in keys:
                state[k][:n].copy_(work[k][:n])

        self.seeded, self.zero = seeded, tuple(zero)
        self.padded, self.state, self.rng, self.keys, self.n, self.first_edges = padded, state, rng, keys, n, e
        self.t_dev = padded["t"]
        self.saved = {k: v.clone() for k, v in state.items()}
        self.t_dev.fill_(float(t0))
        self.step = CapturedStep(captured, warmup=1, device=dev)

    def rewind(self) -> None:
        """(the warm-up run moved the state and drew: both go back to the start)"""
        for k in self.keys:
            self.state[k].copy_(self.saved[k])
        self.rng.zero_()
        if self.seeded is not None:
            self.seeded[1].zero_()
        for acc in self.zero:
            acc.zero_()

    def run(self, timesteps, steps: int) -> None:
        if self.seeded is not None:      # the time comes from the table inside the graph: bare replays
            for _ in range(steps):
                self.step()
            return
        t_dev = self.t_dev
        for i in range(steps):
            t_dev.copy_(timesteps[i].expand_as(t_dev))
            self.step()

    def result(self):
        self.bucket.check()
        out = self.bucket.real_graphs()
        for k in self.keys:
            out[k] = self.state[k][:self.n].clone()
        return out


def get_sampling_fn(config, sde: VPSDE, inverse_scaler, eps: float, **kwargs):
    """``config.sampling.{method, predictor, corrector, snr, n_steps_each}`` → sampler (:247-286: 'pc'; 'ode', which the reference
    dispatches to a sampler it never defines: ``config.sampling.ode_steps`` (required) and ``ode_method`` (default 'heun'))."""
    name = config.sampling.method.lower()
    if name == "ode":
        n_steps = getattr(config.sampling, "ode_steps", None)
        if n_steps is None:
            raise ValueError("config.sampling.ode_steps is required with sampling.method = 'ode' (the steps of the ODE run)")
        return get_ode_sampler(sde=sde, inverse_scaler=inverse_scaler, method=str(getattr(config.sampling, "ode_method", "heun")).lower(),
                               n_steps=n_steps, eps=eps, **kwargs)
    if name != "pc":
        raise ValueError(f"Sampler name {config.sampling.method} unknown.")
    return get_pc_sampler(sde=sde, predictor=get_predictor(config.sampling.predictor.lower()),
                          corrector=get_corrector(config.sampling.corrector.lower()), inverse_scaler=inverse_scaler,
                          snr=config.sampling.snr, n_steps=config.sampling.n_steps_each,
                          continuous=getattr(getattr(config, "training", None), "continuous", True), eps=eps, **kwargs)
