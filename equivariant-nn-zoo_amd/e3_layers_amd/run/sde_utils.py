"""The VP-SDE arithmetic that drives the diffusion score networks (host-side torch plumbing on
device tensors).  Same formulas as ``e3_layers/run/sde_utils.py``:
``VPSDE.marginal`` (:54-66), ``VPSDE.sde`` (:68-81), ``prior_sampling`` (:83-86), ``reverse`` (:88-123),
``get_score_fn`` (:176-187), the loss of ``get_sde_loss_fn`` (:143-171).  The head key is ``score_{key}`` as those functions expect; a model that emits the
shipped config's plain ``score`` key is mapped onto it.
"""
from __future__ import annotations

from typing import Dict, Tuple

import torch


class VPSDE:
    def __init__(self, diffusion_keys: Dict[str, int], beta_min: float = 0.1, beta_max: float = 20.0, N: int = 1000):
        self.beta_0, self.beta_1, self.N = beta_min, beta_max, N
        self.irreps = dict(diffusion_keys)
        self.discrete_betas = torch.linspace(beta_min / N, beta_max / N, N)
        self.alphas = 1.0 - self.discrete_betas

    @property
    def T(self) -> float:
        return 1.0

    def log_mean_coeff(self, t: torch.Tensor) -> torch.Tensor:
        return -0.25 * t ** 2 * (self.beta_1 - self.beta_0) - 0.5 * t * self.beta_0

    def std(self, batch) -> torch.Tensor:
        t = batch["t"][batch.nodeSegment()]
        return torch.sqrt(1.0 - torch.exp(2.0 * self.log_mean_coeff(t)))

    def marginal(self, batch, return_std: bool = False, generator=None, noise_fn=None):
        """x_t = exp(log_mean) x_0 + std z per diffused key, with the per-graph time broadcast to nodes (``noise_fn(shape)``: an
        injected z, as the sampler's)."""
        if return_std:
            return self.std(batch)
        t = batch["t"][batch.nodeSegment()]
        lm = self.log_mean_coeff(t)
        std = torch.sqrt(1.0 - torch.exp(2.0 * lm))
        zs = {}
        for key in self.irreps:
            x = batch[key]
            z = _randn(x, generator, noise_fn)
            batch[key] = torch.exp(lm) * x + std * z
            zs[key] = z
        return batch, {"zs": zs, "std": std}


def _randn(like: torch.Tensor, generator=None, noise_fn=None) -> torch.Tensor:
    if noise_fn is not None:
        return noise_fn(like.shape).to(like.device, like.dtype)
    return torch.randn(like.shape, device=like.device, dtype=like.dtype, generator=generator)


def _node_t(batch) -> torch.Tensor:
    return batch["t"].reshape(-1, 1)[batch.nodeSegment()]


def fixed_rows(batch, fixed) -> torch.Tensor:
    """The conditional sampler's mask as bool [N, 1]: ``fixed`` names a per-node field of the batch (or is the tensor itself), not
    zero = fixed; the rows of a padded batch's ghost graph are never fixed, whatever their bytes hold."""
    m = (batch[fixed] if isinstance(fixed, str) else fixed).reshape(-1, 1) != 0
    if "_graph_weight" in batch:
        m = m & (batch.nodeSegment() < len(batch) - 1).reshape(-1, 1)
    return m


def replace_fixed(sde: VPSDE, batch, fixed, known, generator=None, noise_fn=None):
    """The replacement step of conditional sampling (Song et al. 2021, section I.2) for the unseeded sampler: the fixed rows of every
    diffused key become the known clean values ``known[key]`` perturbed to the batch's time by ``VPSDE.marginal``, one draw per key
    (all rows of it: the draw does not depend on the mask)."""
    noised = batch.view()
    for key in sde.irreps:
        noised[key] = known[key].to(batch[key].dtype)
    noised, _ = sde.marginal(noised, generator=generator, noise_fn=noise_fn)
    rows = fixed_rows(batch, fixed)
    for key in sde.irreps:
        batch[key] = torch.where(rows, noised[key], batch[key])
    return batch


def vpsde_sde(sde: VPSDE, batch, dt=None, generator=None, noise_fn=None):
    """One Euler-Maruyama step of the FORWARD SDE dx = -beta/2 x dt + sqrt(beta) dw (``VPSDE.sde`` :68-81);
    called with ``dt = -1/N`` by the reverse sampler."""
    if dt is None:
        dt = 1.0 / sde.N
    t = _node_t(batch)
    beta_t = sde.beta_0 + t * (sde.beta_1 - sde.beta_0)
    diffusion = torch.sqrt(beta_t)
    for key in sde.irreps:
        x = batch[key]
        x_mean = x + (-0.5 * beta_t * x) * dt
        batch[key] = x_mean + diffusion * (abs(dt) ** 0.5) * _randn(x, generator, noise_fn)
    return batch


def prior_sampling(sde: VPSDE, batch, generator=None, noise_fn=None):
    """x_T ~ N(0, 1) per diffused key (:83-86), drawn on the batch's device."""
    dev = batch["_n_nodes"].device
    n = batch["_node_segment"].shape[0] if "_node_segment" in batch else int(batch["_n_nodes"].sum())
    for key, dim in sde.irreps.items():
        batch[key] = _randn(torch.empty(n, dim, device=dev), generator, noise_fn)
    return batch


def reverse_step(sde: VPSDE, score_fn, batch, generator=None, noise_fn=None):
    """One step of the reverse-time SDE (``RSDE.sde`` :104-119): forward-SDE Euler step with ``dt = -1/N``,
    then ``x -= dt * beta_t * score``."""
    scores = score_fn(batch)
    t = _node_t(batch)
    beta_t = sde.beta_0 + t * (sde.beta_1 - sde.beta_0)
    dt = -1.0 / sde.N
    batch = vpsde_sde(sde, batch, dt, generator, noise_fn)
    for key in sde.irreps:
        batch[key] = batch[key] - dt * beta_t * scores[f"score_{key}"]
    return batch


def get_score_fn(sde: VPSDE, model, train: bool = False):
    def score_fn(batch):
        model.train(train)
        result = model(batch)
        std = sde.std(batch)
        for key in sde.irreps:
            name = f"score_{key}"
            raw = result[name] if name in result else result["score"]
            result[name] = -raw / std - batch[key]
        return result

    return score_fn


def sde_loss(sde: VPSDE, model, batch, eps: float = 1e-5, train: bool = True, generator=None,
             node_weight=None) -> Tuple[torch.Tensor, dict]:
    """mean over graphs/nodes of (score * std + z)^2, t ~ U(eps, 1) per graph.  ``node_weight`` [N, 1] (sums to 1 over the
    nodes that count): a weighted mean instead -- a batch padded with a ghost graph (run/graph_step.py) gives it weight 0."""
    pert, misc = sde_perturb(sde, batch, eps, generator)
    return sde_loss_of(sde, model, pert, misc, train, node_weight)


def sde_perturb(sde: VPSDE, batch, eps: float = 1e-5, generator=None):
    """First half of ``sde_loss``: t ~ U(eps, 1) per graph and the noised copy of the batch (no model involved) -> (pert, misc).
    A loop that wants the next batch's data-only layers early calls ``model.prepare(pert)`` on the result."""
    dev = batch["_n_nodes"].device
    t = torch.rand(len(batch), device=dev, generator=generator) * (sde.T - eps) + eps
    pert = batch.clone()
    pert.attrs["t"] = ("graph", "1x0e")
    pert["t"] = t
    return sde.marginal(pert, generator=generator)


def sde_perturb_counter(sde: VPSDE, batch, seed: int, draw, eps: float = 1e-5, dtype=None):
    """``sde_perturb`` with counter-based draws: t and z are functions of (``seed``, draw index, graph / node, component), so the same
    ``(seed, draw)`` gives the same noised batch wherever and whenever it is asked for -- a replayed training step whose neighbour
    list overflowed is redone on exactly the batch it was vetoed on (``run/score_step.py``).  -> (pert, misc) as ``sde_perturb``.

    Per real graph g: ``u = (pair_hash(seed, draw, 0xFFFFFFFF, g) >> 8) 2^-24``, ``t = eps + (T - eps) u``; per node i and component c
    (counted over the diffusion keys in order): ``z = normal_draw(seed, draw, i, c)``; ``x_t = exp(lm) x_0 + sqrt(-expm1(2 lm)) z``.
    The rows of a padded batch's ghost graph (``_graph_weight`` present: the last graph) keep their geometry: ``z = 0``, ``std = 1``,
    ``t = 0.5``.

    ``draw``: an int, or an int64 tensor (on device tensors a DEVICE cell, read by the kernel without a host synchronisation).
    Device tensors: one ``e3k_vpsde_perturb`` launch per key (fp32).  CPU tensors: the torch restatement of the same hashes and
    formulas in ``dtype`` (default: the batch's) -- its float64 form is what the kernel test holds the kernel to."""
    from ..data.compute_edge import normal_draw, pair_hash

    keys = list(sde.irreps)
    x_first = batch[keys[0]]
    dev = x_first.device
    seg = batch.nodeSegment()
    n_all = len(batch)
    n_real = n_all - 1 if "_graph_weight" in batch else n_all
    # (device: only whole keys are replaced, so a new container over the same tensors does; host: the clone sde_perturb makes)
    pert = batch.view() if dev.type == "cuda" else batch.clone()
    pert.attrs["t"] = ("graph", "1x0e")
    zs, word0, std = {}, 0, None
    if dev.type == "cuda":
        from ..backend import diffusion_ops

        cell = draw if torch.is_tensor(draw) else torch.tensor([int(draw)], dtype=torch.int64, device=dev)
        for key in keys:
            t, x_t, z, s = diffusion_ops.vpsde_perturb(batch[key], seg, n_real, sde.beta_0, sde.beta_1, eps, sde.T, seed, cell, word0)
            pert[key], zs[key] = x_t, z
            word0 += int(batch[key].shape[1])
            if std is None:
                pert["t"], std = t[:n_all], s.reshape(-1, 1)
        return pert, {"zs": zs, "std": std}
    dtype = x_first.dtype if dtype is None else dtype
    f32 = torch.float32
    g = torch.arange(n_all, dtype=torch.int64)
    u = (pair_hash(seed, draw, 0xFFFFFFFF, g) >> 8).to(dtype) * 2.0 ** -24
    # the parameters as the floats the kernel receives: eps, T - eps, q = -(beta_1 - beta_0) / 4, h = -beta_0 / 2
    eps32, t_end = torch.tensor(eps, dtype=f32), torch.tensor(sde.T, dtype=f32)
    b0, b1 = torch.tensor(sde.beta_0, dtype=f32), torch.tensor(sde.beta_1, dtype=f32)
    span, q, h = (t_end - eps32).to(dtype), (-0.25 * (b1 - b0)).to(dtype), (-0.5 * b0).to(dtype)
    real = g < n_real
    t = torch.where(real, eps32.to(dtype) + span * u, torch.full_like(u, 0.5))
    lm = t * (q * t + h)
    a_g, s_g = torch.exp(lm), torch.sqrt(-torch.expm1(2.0 * lm))
    node_real = real[seg].reshape(-1, 1)
    a = torch.where(node_real, a_g[seg].reshape(-1, 1), torch.ones((), dtype=dtype))
    s = torch.where(node_real, s_g[seg].reshape(-1, 1), torch.ones((), dtype=dtype))
    node = torch.arange(seg.shape[0], dtype=torch.int64).reshape(-1, 1)
    for key in keys:
        x = batch[key].to(dtype)
        d = int(x.shape[1])
        z = normal_draw(seed, draw, node, word0 + torch.arange(d, dtype=torch.int64).reshape(1, -1), dtype)
        z = torch.where(node_real, z, torch.zeros((), dtype=dtype))
        pert.data[key] = torch.where(node_real, a * x + s * z, x)
        zs[key] = z
        word0 += d
    pert.data["t"] = t.reshape(-1, 1)
    return pert, {"zs": zs, "std": s}


# ---------------------------------------------------------------------------------------------------------------------
# The seeded predictor-corrector sampler's steps (run/sde_sampling.get_pc_sampler(seed=...)): counter-based noise in the draw layout
# of csrc/e3k_draw.h.  D_total = the sum of the dimensions of sde.irreps; a key's word0 = the sum of the dimensions before it.
#   reverse step i (from 0), corrector noise of component c:  normal_draw(seed, i, node, word0 + c)
#   reverse step i, predictor noise:                          normal_draw(seed, i, node, D_total + word0 + c)
#   the prior x_T:                                            normal_draw(seed, sde.N, node, word0 + c)      (no step has index sde.N)
# Conditional sampling (``fixed=``: the rows kept on known values x0) adds two blocks of the same draw index; blocks 0 and 1 and the
# prior stay where they are, so an unconditioned seeded run keeps its bits:
#   reverse step i, the replacement after the corrector:      normal_draw(seed, i, node, 2 D_total + word0 + c)
#   reverse step i, the replacement after the predictor:      normal_draw(seed, i, node, 3 D_total + word0 + c)
#   the prior's fixed rows:                                   m(T) x0 + s(T) z with the prior's own z
# The sampler's seed should not be the pair criterion's (data.SequenceOrRandom(seed=...)): a node's noise and the Bernoulli draws of
# its pairs would come from one chain.
# ---------------------------------------------------------------------------------------------------------------------
def draw_words(sde: VPSDE):
    """({key: word0}, D_total) of the sampler's draw layout."""
    words, total = {}, 0
    for key, dim in sde.irreps.items():
        words[key] = total
        total += int(dim)
    return words, total


def _real_graphs(batch) -> int:
    """(a padded batch -- ``_graph_weight`` present -- ends with the ghost graph)"""
    return len(batch) - 1 if "_graph_weight" in batch else len(batch)


def _sampler_cells(draw, dev):
    """The kernels read the step in use from element 1 of the sampler's cells (next step, step in use)."""
    if torch.is_tensor(draw):
        return draw
    return torch.tensor([int(draw) + 1, int(draw)], dtype=torch.int64, device=dev)


def _step_in_use(draw) -> int:
    if torch.is_tensor(draw):
        flat = draw.reshape(-1)
        return int(flat[1] if flat.numel() > 1 else flat[0])
    return int(draw)


def _raw_scores(sde: VPSDE, model, batch, train: bool = False):
    """The score heads' outputs per diffusion key, before ``get_score_fn``'s ``-raw / std - x``."""
    model.train(train)
    result = model(batch)
    return {key: result[f"score_{key}"] if f"score_{key}" in result else result["score"] for key in sde.irreps}


def _host_terms(sde: VPSDE, batch, dtype):
    """(t per node, std per node, real-row mask [N, 1], node index [N, 1]) of the CPU restatements, in ``dtype``"""
    seg = batch.nodeSegment()
    t = batch["t"].reshape(-1).to(dtype)
    q, h = -0.25 * (sde.beta_1 - sde.beta_0), -0.5 * sde.beta_0
    lm = t * (q * t + h)
    s = torch.sqrt(-torch.expm1(2.0 * lm))
    real = (torch.arange(len(batch)) < _real_graphs(batch))[seg].reshape(-1, 1)
    node = torch.arange(seg.shape[0], dtype=torch.int64).reshape(-1, 1)
    return t[seg].reshape(-1, 1), s[seg].reshape(-1, 1), real, node


def _known_of(batch, known, key):
    """(the known clean values travel in the batch as ``known_<key>`` unless the caller hands them in)"""
    return batch[f"known_{key}"] if known is None else known[key]


def _device_mask(batch, fixed) -> torch.Tensor:
    """The mask as the kernels read it, uint8 [N]: the field itself when it already is that (no launch joins a replayed step)."""
    m = (batch[fixed] if isinstance(fixed, str) else fixed).reshape(-1)
    return m if m.dtype == torch.uint8 and m.is_contiguous() else (m != 0).to(torch.uint8)


def _host_replaced(sde: VPSDE, batch, new, terms, fixed, x0, seed: int, draw: int, words):
    """The CPU restatement of the kernels' FIXED branch: the fixed real rows of ``new`` become ``exp(lm) x0 + s z`` with
    ``z = normal_draw(seed, draw, node, words)``; ``terms``: ``_host_terms``' tuple."""
    from ..data.compute_edge import normal_draw

    t, s, real, node = terms
    q, h = -0.25 * (sde.beta_1 - sde.beta_0), -0.5 * sde.beta_0
    m = torch.exp(t * (q * t + h))
    z = normal_draw(seed, draw, node, words, new.dtype)
    mask = (batch[fixed] if isinstance(fixed, str) else fixed).reshape(-1, 1) != 0
    return torch.where(real & mask, m * x0.to(new.dtype) + s * z, new)


def sampler_begin_step(times, cells, t) -> None:
    """The seeded loops' step header: with ``k = cells[0]`` inside the table ``times``, ``t`` (every graph's, the ghost graph's
    included) becomes ``times[k]`` and ``cells`` (int64 [2]) becomes ``(k + 1, k)``; outside the table nothing moves.  Device tensors:
    one ``e3k_sampler_begin_step`` launch, no host synchronisation.  CPU tensors: the same in torch."""
    if t.is_cuda:
        from ..backend import diffusion_ops

        return diffusion_ops.sampler_begin_step(times, cells, t)
    k = int(cells[0])
    if 0 <= k < times.numel():
        t.fill_(float(times[k]))
        cells[1] = k
        cells[0] = k + 1


def prior_sampling_counter(sde: VPSDE, batch, seed: int, draw=None, dtype=None, *, fixed=None, known=None):
    """``prior_sampling`` with counter-based draws: ``x_T = normal_draw(seed, draw, node, word0 + c)`` per diffused key; ``draw``
    defaults to ``sde.N``, the index no reverse step uses.  The ghost rows of a padded batch keep what they hold (zeros where the key
    is new).  Device: one ``e3k_vpsde_perturb`` launch per key (its z output; fp32).  CPU: torch, in ``dtype`` (default: torch's).

    ``fixed`` (conditional sampling: a per-node field's name or the mask itself, not zero = fixed; ``known``: ``{key: x0}``, default
    the batch's ``known_<key>``): the fixed real rows start from ``m(T) x0 + s(T) z`` with the same z -- on the device the same
    launch's ``x_t`` output at ``t = T``."""
    from ..data.compute_edge import normal_draw

    dev = batch["_n_nodes"].device
    seg = batch.nodeSegment()
    n, n_real = int(seg.shape[0]), _real_graphs(batch)
    padded = n_real != len(batch)
    draw = sde.N if draw is None else draw
    words, _ = draw_words(sde)
    if dev.type == "cuda":
        from ..backend import diffusion_ops

        cell = draw if torch.is_tensor(draw) else torch.tensor([int(draw)], dtype=torch.int64, device=dev)
        real = (seg < n_real).reshape(-1, 1) if padded else None
        rows = None if fixed is None else fixed_rows(batch, fixed)
        for key, dim in sde.irreps.items():
            if rows is None:
                zero = torch.zeros(n, dim, device=dev)
                z = diffusion_ops.vpsde_perturb(zero, seg, n_real, sde.beta_0, sde.beta_1, 0.0, sde.T, seed, cell, words[key])[2]
            else:      # eps = T: every graph's time is T, x_t = fma(m(T), x0, s(T) z)
                _, x_t, z, _ = diffusion_ops.vpsde_perturb(_known_of(batch, known, key), seg, n_real, sde.beta_0, sde.beta_1, sde.T, sde.T, seed, cell,
                                                           words[key])
            free = torch.where(real, z, batch[key].float()) if padded and key in batch else z
            batch[key] = free if rows is None else torch.where(rows, x_t, free)
        return batch
    dtype = torch.get_default_dtype() if dtype is None else dtype
    real = (torch.arange(len(batch)) < n_real)[seg].reshape(-1, 1)
    node = torch.arange(n, dtype=torch.int64).reshape(-1, 1)
    for key, dim in sde.irreps.items():
        z = normal_draw(seed, _step_in_use(draw), node, words[key] + torch.arange(dim, dtype=torch.int64).reshape(1, -1), dtype)
        old = batch[key].to(dtype) if key in batch else torch.zeros(n, dim, dtype=dtype)
        new = torch.where(real, z, old)
        if fixed is not None:
            q, h = -0.25 * (sde.beta_1 - sde.beta_0), -0.5 * sde.beta_0
            lm = torch.tensor(sde.T * (q * sde.T + h), dtype=dtype)
            noised = torch.exp(lm) * _known_of(batch, known, key).to(dtype) + torch.sqrt(-torch.expm1(2.0 * lm)) * z
            new = torch.where(fixed_rows(batch, fixed), noised, new)
        batch[key] = new
    return batch


def langevin_step_counter(sde: VPSDE, model, batch, seed: int, draw, snr: float, dtype=None, train: bool = False, *, fixed=None,
                          known=None):
    """One ``LangevinCorrector`` update (``n_steps = 1``) with counter-based noise: per key, ``z = normal_draw(seed, draw, node,
    word0 + c)``, the mean row norms of score and z over the REAL rows, ``step = (snr |z| / |score|)^2 2 alphas[k]`` and
    ``x + step score + sqrt(2 step) z``; the rows of a padded batch's ghost graph stay as they are and enter no norm.

    ``draw``: the reverse step's number, an int, or the sampler's DEVICE cells (int64 [2]: next step, step in use -- read by the kernel,
    no host synchronisation).  Device tensors: the model call and one ``e3k_sampler_langevin`` launch per key (fp32).  CPU tensors: the
    torch restatement of the same hashes and formulas in ``dtype`` (default: the key's) -- float64 is the kernel tests' reference.

    ``fixed`` / ``known`` (conditional sampling, as ``prior_sampling_counter``'s): after the update the fixed real rows become
    ``m(t) x0 + s(t) z'`` with ``z' = normal_draw(seed, draw, node, 2 D_total + word0 + c)``; both norms still run over all real rows.
    Device: ``e3k_sampler_langevin_fixed``, still one launch per key -- the mask is read as it is when it is uint8."""
    raw = _raw_scores(sde, model, batch, train)
    words, total = draw_words(sde)
    dev = batch[next(iter(sde.irreps))].device
    if dev.type == "cuda":
        from ..backend import diffusion_ops

        cells, seg, n_real = _sampler_cells(draw, dev), batch.nodeSegment(), _real_graphs(batch)
        mask = None if fixed is None else _device_mask(batch, fixed)
        for key in sde.irreps:
            batch[key], _ = diffusion_ops.sampler_langevin(batch[key], raw[key], seg, batch["t"], sde.alphas, n_real, sde.beta_0, sde.beta_1,
                                                           sde.T, snr, seed, cells, words[key],
                                                           known=None if mask is None else _known_of(batch, known, key), fixed=mask,
                                                           word_fixed=2 * total + words[key])
        return batch
    from ..data.compute_edge import normal_draw

    step_no = _step_in_use(draw)
    for key, dim in sde.irreps.items():
        x = batch[key] if dtype is None else batch[key].to(dtype)
        t, s, real, node = _host_terms(sde, batch, x.dtype)
        n_alpha = int(sde.alphas.numel())
        k = ((t * (n_alpha - 1)) / sde.T).long().clamp(0, n_alpha - 1)
        alpha = sde.alphas.to(x.dtype)[k]
        score = -(raw[key].to(x.dtype) / s) - x
        z = normal_draw(seed, step_no, node, words[key] + torch.arange(dim, dtype=torch.int64).reshape(1, -1), x.dtype)
        rows = real.reshape(-1)
        grad_norm, noise_norm = torch.norm(score[rows], dim=-1).mean(), torch.norm(z[rows], dim=-1).mean()
        step = ((snr * noise_norm) / grad_norm) ** 2 * 2 * alpha
        new = torch.where(real, x + step * score + torch.sqrt(step * 2) * z, x)
        if fixed is not None:
            new = _host_replaced(sde, batch, new, (t, s, real, node), fixed, _known_of(batch, known, key), seed, step_no,
                                 2 * total + words[key] + torch.arange(dim, dtype=torch.int64).reshape(1, -1))
        batch[key] = new
    return batch


def reverse_step_counter(sde: VPSDE, model, batch, seed: int, draw, dtype=None, train: bool = False, *, fixed=None, known=None):
    """``reverse_step`` with counter-based noise: ``z = normal_draw(seed, draw, node, D_total + word0 + c)`` -- the predictor's words,
    not the corrector's of the same step.  ``draw``, devices, ``dtype`` and the ghost rows as ``langevin_step_counter``'s; device
    tensors: the model call and one ``e3k_sampler_reverse_em`` launch per key.

    ``fixed`` / ``known``: after the update the fixed real rows become ``m(t) x0 + s(t) z''`` at the step's own t, with
    ``z'' = normal_draw(seed, draw, node, 3 D_total + word0 + c)`` (device: ``e3k_sampler_reverse_em_fixed``, one launch per key)."""
    raw = _raw_scores(sde, model, batch, train)
    words, total = draw_words(sde)
    dev = batch[next(iter(sde.irreps))].device
    if dev.type == "cuda":
        from ..backend import diffusion_ops

        cells, seg, n_real = _sampler_cells(draw, dev), batch.nodeSegment(), _real_graphs(batch)
        mask = None if fixed is None else _device_mask(batch, fixed)
        for key in sde.irreps:
            batch[key] = diffusion_ops.sampler_reverse_em(batch[key], raw[key], seg, batch["t"], n_real, sde.beta_0, sde.beta_1, sde.N, seed,
                                                          cells, total + words[key],
                                                          known=None if mask is None else _known_of(batch, known, key), fixed=mask,
                                                          word_fixed=3 * total + words[key])
        return batch
    from ..data.compute_edge import normal_draw

    step_no, dt = _step_in_use(draw), -1.0 / sde.N
    for key, dim in sde.irreps.items():
        x = batch[key] if dtype is None else batch[key].to(dtype)
        t, s, real, node = _host_terms(sde, batch, x.dtype)
        score = -(raw[key].to(x.dtype) / s) - x
        beta = t * (sde.beta_1 - sde.beta_0) + sde.beta_0
        z = normal_draw(seed, step_no, node, total + words[key] + torch.arange(dim, dtype=torch.int64).reshape(1, -1), x.dtype)
        x_mean = x + (-0.5 * beta * x) * dt
        noised = x_mean + (torch.sqrt(beta) * (abs(dt) ** 0.5)) * z
        new = torch.where(real, noised - (dt * beta) * score, x)
        if fixed is not None:
            new = _host_replaced(sde, batch, new, (t, s, real, node), fixed, _known_of(batch, known, key), seed, step_no,
                                 3 * total + words[key] + torch.arange(dim, dtype=torch.int64).reshape(1, -1))
        batch[key] = new
    return batch


# ---------------------------------------------------------------------------------------------------------------------
# The probability-flow ODE sampler's steps (run/sde_sampling.get_ode_sampler): fixed-step Euler and Heun on
#   dx/dt = -0.5 beta(t) [x + score(x, t)],   score = -raw / s(t) - x   =>   d(raw, t) = (0.5 beta(t)) (raw / s(t))
# -- the collapsed drift: the x terms cancel, so it is never formed as x + (-raw / s - x).  ``times`` = linspace(T, eps, n_steps + 1);
# step k goes from t_k = times[k] to t_{k+1} = times[k + 1], h = t_{k+1} - t_k < 0, both read from the table (not from the batch's t):
#   Euler / Heun stage A:  d1 = d(raw(x, t_k), t_k),           x~ = x + h d1,                and the batch's t becomes t_{k+1}
#   Heun stage B:          d2 = d(raw(x~, t_{k+1}), t_{k+1}),  x' = x + (0.5 h) (d1 + d2)
# Ghost rows of a padded batch: x~ = x' = x bit for bit, d1 = 0.  k or k + 1 outside the table: nothing moves.
# ---------------------------------------------------------------------------------------------------------------------
def _ode_host_terms(sde: VPSDE, batch, times, k: int, dtype):
    """(beta(t) / 2, s(t)) at t = times[k] in ``dtype``, the real-row mask [N, 1]: the CPU restatement's terms"""
    t = times[k].to(dtype)
    q, h = -0.25 * (sde.beta_1 - sde.beta_0), -0.5 * sde.beta_0
    lm = t * (q * t + h)
    seg = batch.nodeSegment()
    real = (torch.arange(len(batch)) < _real_graphs(batch))[seg].reshape(-1, 1)
    return 0.5 * (t * (sde.beta_1 - sde.beta_0) + sde.beta_0), torch.sqrt(-torch.expm1(2.0 * lm)), real


def ode_euler_step(sde: VPSDE, model, batch, times, cells_or_step, dtype=None, keep=None, train: bool = False):
    """One Euler step of the probability-flow ODE, which is Heun's stage A: the model call at the batch's state and time, then per
    diffusion key ``x + h d1`` with ``d1 = (0.5 beta(t_k)) (raw / s(t_k))`` (the formulas above); the batch's ``t`` becomes
    ``t_{k+1}``, what the model's next call sees.

    ``times``: the run's table [n_steps + 1].  ``cells_or_step``: the step k as an int, or the sampler's cells (int64 [2]: next step,
    step in use; on device tensors DEVICE cells, read by the kernel without a host synchronisation).  ``keep``: a dict that receives
    ``{key: (x, d1)}`` for ``ode_heun_finish`` (None: the Euler method, nothing is kept and the key is updated in place where it can
    be).  Device tensors: one ``e3k_sampler_ode_euler`` launch per key (fp32); the first key's launch writes the time.  CPU tensors:
    the torch restatement in ``dtype`` (default: the key's) -- float64 is the kernel tests' reference."""
    raw = _raw_scores(sde, model, batch, train)
    keys = list(sde.irreps)
    dev = batch[keys[0]].device
    if dev.type == "cuda":
        from ..backend import diffusion_ops

        cells, seg, n_real = _sampler_cells(cells_or_step, dev), batch.nodeSegment(), _real_graphs(batch)
        for key in keys:
            x = batch[key]
            in_place = keep is None and x.dtype == torch.float32 and x.is_contiguous()
            batch[key], d1 = diffusion_ops.sampler_ode_euler(x, raw[key], seg, times, cells, n_real, sde.beta_0, sde.beta_1,
                                                             t_out=batch["t"] if key == keys[0] else None, want_d=keep is not None,
                                                             out=x if in_place else None)
            if keep is not None:
                keep[key] = (x, d1)
        return batch
    k = _step_in_use(cells_or_step)
    if not 0 <= k < times.numel() - 1:
        if keep is not None:
            keep.update({key: (batch[key], torch.zeros_like(batch[key])) for key in keys})
        return batch
    for key in keys:
        x = batch[key] if dtype is None else batch[key].to(dtype)
        half_beta, s, real = _ode_host_terms(sde, batch, times, k, x.dtype)
        h = (times[k + 1] - times[k]).to(x.dtype)
        d1 = torch.where(real, half_beta * (raw[key].to(x.dtype) / s), torch.zeros((), dtype=x.dtype))
        batch[key] = torch.where(real, x + h * d1, x)
        if keep is not None:
            keep[key] = (x, d1)
    batch["t"].fill_(float(times[k + 1]))
    return batch


def ode_heun_finish(sde: VPSDE, model, batch, kept, times, cells_or_step, dtype=None, train: bool = False):
    """Heun's stage B: the model call at the stage-A state ``x~`` and ``t_{k+1}``, then per diffusion key ``x + (0.5 h) (d1 + d2)``
    with ``d2 = (0.5 beta(t_{k+1})) (raw2 / s(t_{k+1}))`` and ``(x, d1) = kept[key]`` from ``ode_euler_step(keep=kept)`` of the same
    step.  ``times``, ``cells_or_step``, devices and ``dtype`` as there; device tensors: one ``e3k_sampler_ode_heun`` launch per key."""
    raw2 = _raw_scores(sde, model, batch, train)
    keys = list(sde.irreps)
    dev = batch[keys[0]].device
    if dev.type == "cuda":
        from ..backend import diffusion_ops

        cells, seg, n_real = _sampler_cells(cells_or_step, dev), batch.nodeSegment(), _real_graphs(batch)
        for key in keys:
            x0, d1 = kept[key]
            batch[key] = diffusion_ops.sampler_ode_heun(x0, d1, raw2[key], seg, times, cells, n_real, sde.beta_0, sde.beta_1)
        return batch
    k = _step_in_use(cells_or_step)
    for key in keys:
        x0, d1 = kept[key]
        x0 = x0 if dtype is None else x0.to(dtype)
        if not 0 <= k < times.numel() - 1:
            batch[key] = x0
            continue
        half_beta, s, real = _ode_host_terms(sde, batch, times, k + 1, x0.dtype)
        h = (times[k + 1] - times[k]).to(x0.dtype)
        d2 = half_beta * (raw2[key].to(x0.dtype) / s)
        batch[key] = torch.where(real, x0 + (0.5 * h) * (d1.to(x0.dtype) + d2), x0)
    return batch


def sde_loss_of(sde: VPSDE, model, pert, misc, train: bool = True, node_weight=None) -> Tuple[torch.Tensor, dict]:
    """Second half of ``sde_loss``: the score network on the noised batch and the denoising loss."""
    scores = get_score_fn(sde, model, train)(pert)
    losses = {}
    for key in sde.irreps:
        err = torch.square(scores[f"score_{key}"] * misc["std"] + misc["zs"][key])
        per_node = err.reshape(err.shape[0], -1).mean(dim=-1)
        losses[key] = per_node.mean() if node_weight is None else (per_node * node_weight.reshape(-1)).sum()
    total = sum(losses.values())
    losses["total"] = total
    return total, losses
