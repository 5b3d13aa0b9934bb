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
one launch per key and stage around each model call, the same three loops.

A sampler is four stages.  ``pc_plan`` / ``ode_plan`` set a run up as a ``run/loops.StepPlan`` (the working copy of the batch with the
prior drawn, the updates of one step, the table of times and the cells every step's first launch walks); ``run/loops.make_loop`` picks the driver
(``EagerLoop``, ``StaticLoop``, ``CappedLoop``: ``rewind()``, ``run(steps)``, ``result()``); the loop runs; the sampler releases the
fixed rows and applies ``inverse_scaler``.  The plans are callable on their own: ``tools/sample_bench.py`` times the loops of the
plans the samplers build.
"""
from __future__ import annotations

from functools import partial
from typing import Callable, Dict, Optional, Sequence

import torch

from .loops import StepPlan, check_loop_args, edge_plumbing, make_loop, static_topology
from .sde_utils import (VPSDE, _node_t, _randn, fixed_rows, get_score_fn, langevin_step_counter, ode_euler_step, ode_heun_finish,
                        prior_sampling, prior_sampling_counter, replace_fixed, reverse_step, reverse_step_counter)

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


def pc_plan(sde: VPSDE, predictor, corrector, model, batch, generator=None, noise_fn=None, *, snr: float = 0.16, n_steps: int = 1,
            eps: float = 1e-3, preprocess: Sequence[Callable] = (), static_edges: bool = False, seed: Optional[int] = None,
            fixed: Optional[str] = None):
    """The set-up of one predictor-corrector run, with ``get_pc_sampler``'s settings (which has checked them; ``predictor`` and
    ``corrector`` are classes): the working copy of ``batch`` with conditional sampling's fields and the prior in it, the table of
    ``sde.N`` times and its cells, and [corrector, predictor] as ``batch -> batch`` updates.
    -> (``StepPlan``, what the caller held under conditional sampling's names -- for ``_release``; None without ``fixed``)"""
    seeded = seed is not None
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
    # fp32 on the device (what the step's first launch reads); torch's default dtype on the host, where float64 is the tests' reference
    times = torch.linspace(sde.T, eps, sde.N, device=dev, dtype=torch.float32 if dev.type == "cuda" else None)
    score_fn = get_score_fn(sde, model, train=False)
    pred, corr = predictor(sde, score_fn), corrector(sde, score_fn, snr, n_steps)
    batch["t"] = torch.empty(len(batch), 1, device=dev, dtype=times.dtype)
    if static_edges:
        static_topology(batch, edge_plumbing(preprocess, static_edges)[0])
    keys = list(sde.irreps)
    # the step's time and number: device cells (next step, step in use) that the step's first launch advances
    cells = torch.zeros(2, dtype=torch.int64, device=dev)
    if seeded:
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
    return StepPlan(batch, [corr_fn, pred_fn], keys, times, cells, fixed=fixed), given


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
    check_loop_args(graph, static_edges, edge_capacity, r_max, criteria,
                    norms_served=corrector is NoneCorrector or (seed is not None and corrector is LangevinCorrector))
    if seed is not None:
        if not 0 <= int(seed) < 1 << 64:
            raise ValueError("seed: at most 64 bits")
        if predictor not in (EulerMaruyamaPredictor, NonePredictor) or corrector not in (LangevinCorrector, NoneCorrector):
            raise ValueError("seed: only the built-in predictors and correctors draw counter-based noise "
                             f"(got {predictor.__name__}, {corrector.__name__})")
        if corrector is LangevinCorrector and n_steps != 1:
            raise ValueError("seed: the draw layout holds one corrector draw per reverse step, and the capped loop would rebuild the "
                             "list between inner corrector steps where the eager loop does not: n_steps must be 1")

    _, moved = edge_plumbing(preprocess, static_edges)
    steps = sde.N if n_iter is None else min(int(n_iter), sde.N)

    def pc_sampler(model, batch, generator=None, noise_fn=None):
        plan, given = pc_plan(sde, predictor, corrector, model, batch, generator, noise_fn, snr=snr, n_steps=n_steps, eps=eps,
                              preprocess=preprocess, static_edges=static_edges, seed=seed, fixed=fixed)
        with torch.no_grad():
            loop = make_loop(plan, model, moved, graph=graph, edge_capacity=edge_capacity, r_max=r_max, criteria=criteria)
            loop.rewind()
            loop.run(steps)
            batch = loop.result()
        if fixed is not None:
            batch = _release(sde, batch, fixed, given)
        return inverse_scaler(batch), steps * (n_steps + 1)

    return pc_sampler


def ode_plan(sde: VPSDE, method: str, model, batch, generator=None, noise_fn=None, *, n_steps: int, eps: float = 1e-3,
             preprocess: Sequence[Callable] = (), static_edges: bool = False, seed: Optional[int] = None) -> StepPlan:
    """The set-up of one run of the probability-flow ODE, with ``get_ode_sampler``'s settings (which has checked them): the working
    copy of ``batch`` with the prior in it, the grid of ``n_steps + 1`` times and its cells, and the method's stages as updates."""
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
        static_topology(batch, edge_plumbing(preprocess, static_edges)[0])
    cells = torch.zeros(2, dtype=torch.int64, device=dev)
    if method == "euler":
        updates = [partial(ode_euler_step, sde, model, times=times, cells_or_step=cells)]
    else:
        kept = {}      # stage A's (x, d1) per key: made and used inside one step (one captured step on the replays)
        updates = [partial(ode_euler_step, sde, model, times=times, cells_or_step=cells, keep=kept),
                   partial(ode_heun_finish, sde, model, kept=kept, times=times, cells_or_step=cells)]
    # the loop walks the first n_steps entries: step k reads t_k and t_{k+1} from the whole grid
    return StepPlan(batch, updates, list(sde.irreps), times[:n_steps], cells)


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
    check_loop_args(graph, static_edges, edge_capacity, r_max, criteria)
    if seed is not None and not 0 <= int(seed) < 1 << 64:
        raise ValueError("seed: at most 64 bits")
    _, moved = edge_plumbing(preprocess, static_edges)
    steps = n_steps if n_iter is None else min(int(n_iter), n_steps)

    def ode_sampler(model, batch, generator=None, noise_fn=None):
        plan = ode_plan(sde, method, model, batch, generator, noise_fn, n_steps=n_steps, eps=eps, preprocess=preprocess,
                        static_edges=static_edges, seed=seed)
        with torch.no_grad():
            loop = make_loop(plan, model, moved, graph=graph, edge_capacity=edge_capacity, r_max=r_max, criteria=criteria)
            loop.rewind()
            loop.run(steps)
            batch = loop.result()
        return inverse_scaler(batch), steps * len(plan.updates)

    return ode_sampler


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
