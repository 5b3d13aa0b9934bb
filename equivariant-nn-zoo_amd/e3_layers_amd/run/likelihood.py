"""The exact log-likelihood of a batch under a score net, through the probability-flow ODE of the VP-SDE (Song et al. 2021, section 4.3
and appendix D.2) -- the ``likelihood`` module that ``train_diffusion`` of the reference imports (``train.py:72``) and never ships.

The flow is the ODE sampler's, run the other way: ``dx/dt = f(x, t) = (0.5 beta(t)) raw(x, t) / s(t)`` with the head convention
``score = -raw / s - x`` (the collapsed drift of ``run/sde_utils.ode_euler_step``).  The ``x`` terms cancel in the divergence as they do
in the drift,

    div f = c(t) tr(d raw / d x),      c(t) = (0.5 beta(t)) / s(t),

and on the grid ``times = linspace(eps, sde.T, n_steps + 1)`` (ascending: data to prior, ``h = t_{k+1} - t_k > 0``), per real graph g,

    log p_eps(x_g(eps)) = log N(x_g(T); 0, I) + integral from eps to T of div f dt.

The integral takes the quadrature of the state's own integrator: Euler ``h div f(x_k, t_k)``; Heun ``(0.5 h) [div f(x_k, t_k) +
div f(x~, t_{k+1})]`` with ``x~`` the stage-A state -- the step's own two model calls.  The trace is Hutchinson's estimate: per model
call and probe one backward pass with respect to the diffused keys jointly, ``eps . grad_x(eps . raw)``; the probes are fixed for the
whole run (draw index ``sde.N + 1 + p`` of the stream of ``csrc/e3k_draw.h``), ``n_probes`` of them share one forward and average.

Device tensors: the step kernels ``e3k_sampler_ode_euler`` / ``e3k_sampler_ode_heun`` unchanged on the ascending table, and three
kernels of ``csrc/e3k_sampler.hip`` -- ``e3k_sampler_probe``, ``e3k_sampler_ode_div`` (the quadrature term into double accumulators, one
launch per key, probe and model call) and ``e3k_sampler_prior_logp``; the loops are the samplers' (``run/loops``: eager, the
static-edge graph, the capped replay), on the plan ``likelihood_plan`` sets up.  The model's backward runs under ``ops.inputs_only_backward()``: with the harmonics
requiring grad a layer takes the force block where its structure is served and the composed per-op path otherwise (the score nets:
un-keyed attributes, composite edge embeddings), inside ``ops.ordered_edge_gradients()``: the harmonics' gradient of an edge is summed
in a fixed order, so a vector-Jacobian product is the same bits run to run (probes' estimates are compared and averaged across runs).
The run freezes the model's parameters (``frozen_parameters``), so that backward
walks only the routes that reach the diffused keys.  CPU tensors: the torch restatement, in the tensors' dtype (float64 is the tests'
reference).

Without trained weights the value of ``logp`` says nothing about a model; that the number is a log-density is pinned by the closed
forms of ``tests/test_likelihood_host.py``."""
from __future__ import annotations

import contextlib
import math
from typing import Callable, Optional, Sequence

import torch

from .loops import StepPlan, check_loop_args, edge_plumbing, make_loop, static_topology
from .sde_utils import VPSDE, _real_graphs, _step_in_use, draw_words, ode_euler_step, ode_heun_finish

_PROBES = {"rademacher": 0, "gaussian": 1}
LN_2PI = math.log(2.0 * math.pi)


def bits_per_dim(logp, dims):
    """nats -> bits per dimension: ``-logp / (dims ln 2)``"""
    return -logp / (dims * math.log(2.0))


def probe_name(p: int, key: str) -> str:
    """(the batch field that carries probe p of a diffused key through the loops)"""
    return f"probe{p}_{key}"


class _Computed:
    """The model call that already happened, in the shape ``sde_utils._raw_scores`` asks for: the step functions take their ``raw`` from
    it instead of calling the network a second time."""

    def __init__(self, result):
        self.result = result

    def train(self, mode=True):
        return self

    def __call__(self, batch):
        return self.result


def make_probes(sde: VPSDE, batch, seed: int, kind: str, n_probes: int, dtype=None):
    """``{(p, key): eps [N, D]}``: probe p of component c of a key is draw index ``sde.N + 1 + p``, word ``word0 + c`` -- Rademacher
    (``data.compute_edge.rademacher_draw``) or Gaussian (``normal_draw``); zero on the rows of a padded batch's ghost graph.  Device:
    one ``e3k_sampler_probe`` launch each (fp32).  CPU: torch, in ``dtype`` (default: the key's)."""
    from ..data.compute_edge import normal_draw, rademacher_draw

    words, _ = draw_words(sde)
    seg = batch.nodeSegment()
    n_real = _real_graphs(batch)
    out = {}
    for p in range(n_probes):
        for key, dim in sde.irreps.items():
            if seg.is_cuda:
                from ..backend import diffusion_ops

                out[p, key] = diffusion_ops.sampler_probe(seg, dim, n_real, seed, sde.N + 1 + p, words[key], _PROBES[kind])
                continue
            dt = batch[key].dtype if dtype is None else dtype
            node = torch.arange(seg.shape[0], dtype=torch.int64).reshape(-1, 1)
            word = words[key] + torch.arange(dim, dtype=torch.int64).reshape(1, -1)
            z = (rademacher_draw if kind == "rademacher" else normal_draw)(seed, sde.N + 1 + p, node, word, dt)
            out[p, key] = torch.where((seg < n_real).reshape(-1, 1), z, torch.zeros((), dtype=dt))
    return out


def div_weight(sde: VPSDE, times, k: int, stage: int) -> float:
    """``w c(t)`` of one quadrature term in double, from the table's entries: stage 0 (Euler) ``w = h``, ``t = t_k``; 1 (Heun A)
    ``w = h / 2``, ``t = t_k``; 2 (Heun B) ``w = h / 2``, ``t = t_{k+1}`` -- ``e3k_sampler_ode_div``'s coefficient."""
    tk, tn = float(times[k]), float(times[k + 1])
    w = tn - tk if stage == 0 else 0.5 * (tn - tk)
    t = tn if stage == 2 else tk
    db = float(sde.beta_1) - float(sde.beta_0)
    lm = t * (-0.25 * db * t - 0.5 * float(sde.beta_0))
    return w * (0.5 * (t * db + float(sde.beta_0))) / math.sqrt(-math.expm1(2.0 * lm))


def _graph_sums(values, batch):
    """float64 [G_real]: the sum of ``values`` [N, D] over the rows of each real graph (CPU)"""
    rows = values.double().sum(dim=1)
    return torch.zeros(len(batch), dtype=torch.float64).index_add_(0, batch.nodeSegment(), rows)[:_real_graphs(batch)]


def prior_logp(sde: VPSDE, batch, row_ptr=None):
    """float64 [G_real]: ``log N(x_g; 0, I)`` over the diffused keys of each real graph.  Device: one ``e3k_sampler_prior_logp`` launch
    per key into one accumulator."""
    n_real = _real_graphs(batch)
    first = batch[next(iter(sde.irreps))]
    if first.is_cuda:
        from ..backend import diffusion_ops

        out = torch.zeros(n_real, dtype=torch.float64, device=first.device)
        row_ptr = diffusion_ops.graph_row_pointers(batch["_n_nodes"]) if row_ptr is None else row_ptr
        for key in sde.irreps:
            diffusion_ops.sampler_prior_logp(out, batch[key], row_ptr, n_real)
        return out
    counts = batch["_n_nodes"].reshape(-1)[:n_real].double()
    out = torch.zeros(n_real, dtype=torch.float64)
    for key, dim in sde.irreps.items():
        x = batch[key].double()
        out += -0.5 * _graph_sums(x * x, batch) - (0.5 * counts * dim) * LN_2PI
    return out


def div_stage(sde: VPSDE, model, batch, acc, times, cells_or_step, stage: int, n_probes: int, row_ptr=None, train: bool = False):
    """One model call of the likelihood's loop: the network at the batch's state and time with the diffused keys requiring grad, per
    probe the vector-Jacobian product ``grad_x(eps . raw)`` over all keys jointly (one backward; under ``ops.inputs_only_backward()`` and
    ``ops.ordered_edge_gradients()``: bit-reproducible),
    and ``acc[g] += w c(t) (1 / n_probes) sum_g(eps . vjp)`` for the real graphs (``div_weight``; device: one ``e3k_sampler_ode_div``
    launch per key and probe, which reads the step from the cells).  The probes are the batch's fields ``probe_name(p, key)``.
    -> the model's result, for the step that follows.

    The keys are differentiated as detached leaves over the batch's own storage, inside ``torch.enable_grad()`` (the loops run under
    ``no_grad``): the step kernels may then update that storage in place, after and outside the graph.  A vector-Jacobian product that
    comes back ``None`` raises: a missing term is never integrated as zero."""
    from ..backend import diffusion_ops, ops

    keys = list(sde.irreps)
    with torch.enable_grad():
        work = batch.view()
        leaves = []
        for key in keys:
            leaf = batch[key].detach().requires_grad_(True)
            work.data[key] = leaf
            leaves.append(leaf)
        model.train(train)
        result = model(work)
        raws = [result[f"score_{key}"] if f"score_{key}" in result else result["score"] for key in keys]
        for key, raw in zip(keys, raws):
            if not raw.requires_grad:
                raise RuntimeError(f"likelihood: the model's output for {key!r} does not depend differentiably on the diffused keys "
                                   "(a layer on its route delivers no input gradient)")
        vjps = {}
        for p in range(n_probes):
            probes = [batch[probe_name(p, key)].to(raw.dtype) for key, raw in zip(keys, raws)]
            with ops.inputs_only_backward(), ops.ordered_edge_gradients():
                grads = torch.autograd.grad(raws, leaves, grad_outputs=probes, retain_graph=p + 1 < n_probes, allow_unused=True)
            for key, g in zip(keys, grads):
                if g is None:
                    raise RuntimeError(f"likelihood: the vector-Jacobian product with respect to {key!r} came back None: the model's "
                                       "output does not reach that key, and its share of the divergence would be missing")
                vjps[p, key] = g.detach()
    detached = result.view()
    for name in {f"score_{key}" for key in keys} | {"score"}:
        if name in detached:
            detached.data[name] = detached[name].detach()
    scale = 1.0 / n_probes
    if leaves[0].is_cuda:
        n_real = _real_graphs(batch)
        for (p, key), g in vjps.items():
            diffusion_ops.sampler_ode_div(acc, batch[probe_name(p, key)], g, row_ptr, times, cells_or_step, n_real, stage, scale,
                                          sde.beta_0, sde.beta_1)
        return detached
    k = _step_in_use(cells_or_step)
    if 0 <= k < times.numel() - 1:
        n_real = _real_graphs(batch)
        coef = div_weight(sde, times, k, stage) * scale
        for (p, key), g in vjps.items():
            acc[:n_real] += coef * _graph_sums(batch[probe_name(p, key)].double() * g.double(), batch)
    return detached


@contextlib.contextmanager
def frozen_parameters(model):
    """No Parameter of ``model`` requires grad inside: the backward of ``div_stage`` then walks only the routes that reach the diffused
    keys.  (``ops.inputs_only_backward()`` skips the Parameter slots of a node, but a tensor made of parameters AND data -- the
    attributes, a function of the time embedding -- still requires grad, and autograd walks its route until it ends in a Linear.)"""
    params = [p for p in model.parameters() if p.requires_grad] if hasattr(model, "parameters") else []
    for p in params:
        p.requires_grad_(False)
    try:
        yield
    finally:
        for p in params:
            p.requires_grad_(True)


def attach_probes(sde: VPSDE, batch, seed: int, kind: str, n_probes: int) -> None:
    """The loop's working copy of the batch: the diffused keys contiguous fp32 on the device (the step kernels update them in place),
    and the probes as node fields ``probe_name(p, key)`` with the key's attrs -- the capped loop pads them like any node tensor."""
    for key in sde.irreps:
        if batch[key].is_cuda:
            batch.data[key] = batch[key].float().contiguous()
        for p in range(n_probes):
            batch.attrs[probe_name(p, key)] = batch.attrs[key]
    for (p, key), z in make_probes(sde, batch, seed, kind, n_probes).items():
        batch.data[probe_name(p, key)] = z


def stage_updates(sde: VPSDE, model, method: str, times, cells, acc, n_probes: int, row_ptr=None):
    """The updates of one step of the likelihood's plan: ``div_stage`` (the model call, its backwards, the quadrature term
    into ``acc``) in front of the sampler's own step function, which takes the model's output from it."""
    def first_stage(b, keep=None):
        done = div_stage(sde, model, b, acc, times, cells, 0 if keep is None else 1, n_probes, row_ptr)
        return ode_euler_step(sde, _Computed(done), b, times=times, cells_or_step=cells, keep=keep)

    if method == "euler":
        return [first_stage]
    kept = {}      # stage A's (x, d1) per key: made and used inside one step

    def second_stage(b):
        done = div_stage(sde, model, b, acc, times, cells, 2, n_probes, row_ptr)
        return ode_heun_finish(sde, _Computed(done), b, kept=kept, times=times, cells_or_step=cells)

    return [lambda b: first_stage(b, kept), second_stage]


def likelihood_plan(sde: VPSDE, method: str, model, batch, *, n_steps: int, eps: float = 1e-3, probe: str = "rademacher",
                    n_probes: int = 1, seed: int, preprocess: Sequence[Callable] = (), static_edges: bool = False):
    """The set-up of one likelihood run, with ``get_likelihood_fn``'s settings (which has checked them): the working copy of ``batch``
    with the probes attached, the ascending grid of ``n_steps + 1`` times and its cells, ``stage_updates`` as the updates, and the
    accumulator of the integral as loop state (``StepPlan.zero``).
    -> (``StepPlan``, ``acc`` float64 [G_real], ``row_ptr``: the graphs' row pointers on the device, else None)"""
    batch = batch.clone()
    dev = batch["_n_nodes"].device
    on_device = dev.type == "cuda"
    batch.attrs["t"] = ("graph", "1x0e")
    attach_probes(sde, batch, seed, probe, n_probes)
    times = torch.linspace(eps, sde.T, n_steps + 1, device=dev, dtype=torch.float32 if on_device else None)
    batch["t"] = torch.empty(len(batch), 1, device=dev, dtype=times.dtype)
    if static_edges:
        static_topology(batch, edge_plumbing(preprocess, static_edges)[0])
    cells = torch.zeros(2, dtype=torch.int64, device=dev)
    acc = torch.zeros(_real_graphs(batch), dtype=torch.float64, device=dev)
    row_ptr = None
    if on_device:
        from ..backend import diffusion_ops

        # the real graphs come first in a padded batch too: one table serves every loop
        row_ptr = diffusion_ops.graph_row_pointers(batch["_n_nodes"].reshape(-1).contiguous())
    updates = stage_updates(sde, model, method, times, cells, acc, n_probes, row_ptr)
    return StepPlan(batch, updates, list(sde.irreps), times[:n_steps], cells, zero=(acc,)), acc, row_ptr


def get_likelihood_fn(sde: VPSDE, method: str = "heun", *, n_steps: int, eps: float = 1e-3, probe: str = "rademacher", n_probes: int = 1,
                      seed: int, scale=None, preprocess: Sequence[Callable] = (), static_edges: bool = False, graph: bool = False,
                      edge_capacity: Optional[int] = None, r_max: Optional[float] = None, criteria=None):
    """``likelihood_fn(model, batch) -> (logp, latent, info)``: the log-likelihood of every graph of ``batch`` (its diffused keys in the
    model's scaled space) under the probability-flow ODE of ``model`` (the module's docstring has the formulas).

    logp: float64 [G], nats, in the model's scaled space; with ``scale`` in the data's units.
    latent: the batch at ``t = T`` (the code of the data under the flow).
    info: ``nfe`` (model calls; each is one forward and ``n_probes`` backwards), ``prior_logp`` and ``delta_logp`` (float64 [G]: the two
        terms of ``logp`` before ``scale``), ``dims`` (int64 [G]: ``n_g D_total``; ``bits_per_dim(logp, dims)``).

    method: ``"heun"`` or ``"euler"``: the state's integrator and, with it, the quadrature of the integral.
    n_steps: the steps of the run, required; the grid is ``linspace(eps, sde.T, n_steps + 1)``.
    probe, n_probes: ``"rademacher"`` or ``"gaussian"`` Hutchinson probes, fixed for the run; ``n_probes`` of them share each forward
        and their estimates average.
    seed: required (at most 64 bits): the probes are counter-based draws, index ``sde.N + 1 + p``.  There is no generator form.
    scale: a float or ``{key: float}``, the data's units per scaled unit (``data.std``): ``logp - n_g sum_key D_key ln scale_key``.
    preprocess, static_edges, graph, edge_capacity, r_max, criteria: the loops of ``get_pc_sampler``, with its meaning and refusals.
        On the replays the accumulators are loop state: the warm-up step's share is zeroed with the cells.

    While ``likelihood_fn`` runs, no Parameter of ``model`` requires grad (``frozen_parameters``; restored when it returns or raises).

    Out of scope: adaptive solvers, exact traces, conditional likelihood, likelihood weighting of the training loss."""
    if method not in ("euler", "heun"):
        raise ValueError(f"likelihood method {method!r} unknown (euler, heun)")
    if probe not in _PROBES:
        raise ValueError(f"probe {probe!r} unknown (rademacher, gaussian)")
    if int(n_steps) < 1:
        raise ValueError(f"n_steps: at least one step (got {n_steps})")
    if int(n_probes) < 1:
        raise ValueError(f"n_probes: at least one probe (got {n_probes})")
    if not 0 <= int(seed) < 1 << 64:
        raise ValueError("seed: at most 64 bits")
    n_steps, n_probes, seed = int(n_steps), int(n_probes), int(seed)
    check_loop_args(graph, static_edges, edge_capacity, r_max, criteria)
    keys = list(sde.irreps)
    if scale is None:
        ln_scale = 0.0
    else:
        per_key = scale if isinstance(scale, dict) else {key: scale for key in keys}
        if set(per_key) != set(keys) or not all(float(v) > 0.0 for v in per_key.values()):
            raise ValueError(f"scale: one positive number per diffusion key {keys} (got {scale!r})")
        ln_scale = sum(dim * math.log(float(per_key[key])) for key, dim in sde.irreps.items())
    _, moved = edge_plumbing(preprocess, static_edges)
    d_total = sum(int(d) for d in sde.irreps.values())

    def likelihood_fn(model, batch):
        names = set(batch.data)
        n_graphs = _real_graphs(batch)      # (a batch the caller padded: its ghost graph has no entry)
        plan, acc, row_ptr = likelihood_plan(sde, method, model, batch, n_steps=n_steps, eps=eps, probe=probe, n_probes=n_probes,
                                             seed=seed, preprocess=preprocess, static_edges=static_edges)
        with torch.no_grad(), frozen_parameters(model):
            loop = make_loop(plan, model, moved, graph=graph, edge_capacity=edge_capacity, r_max=r_max, criteria=criteria)
            loop.rewind()
            loop.run(n_steps)
            latent = loop.result()
        for name in [name for name in latent.data if name.startswith("probe") and name not in names]:
            latent.pop(name)
        prior = prior_logp(sde, latent, row_ptr)
        delta = acc.clone()
        counts = latent["_n_nodes"].reshape(-1)[:n_graphs].to(torch.int64)
        dims = counts * d_total
        logp = prior + delta - counts.double() * ln_scale
        info = {"nfe": n_steps * len(plan.updates), "prior_logp": prior, "delta_logp": delta, "dims": dims}
        return logp, latent, info

    return likelihood_fn
