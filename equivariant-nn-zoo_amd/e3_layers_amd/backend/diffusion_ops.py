"""Launch wrappers of the diffusion kernels (``csrc/e3k_score.hip``, ``csrc/e3k_sampler.hip``): the VP-SDE perturbation, the
samplers' step header, the predictor / corrector / ODE updates and the likelihood's per-graph sums.

None of them is differentiated: each checks its operands, allocates its outputs with torch and enqueues ONE kernel on the current
stream, with no host synchronisation.  (The autograd side of the score nets -- ``denoise_loss`` -- lives in ``backend/ops.py``.)
"""
from __future__ import annotations

import torch

from . import lib as L


# ---- operand checks ------------------------------------------------------------------------------------------------------
def _check_cells(name, cells) -> None:
    if cells.dtype != torch.int64 or cells.numel() < 2 or not cells.is_contiguous():
        raise ValueError(f"{name}: cells must be a contiguous int64 device tensor [2] = (next step, step in use)")


def _check_times(name, times) -> None:
    if times.dtype != torch.float32 or not times.is_contiguous() or times.dim() != 1 or times.numel() < 2:
        raise ValueError(f"{name}: times must be a contiguous fp32 device tensor [n_steps + 1]")


def _sampler_operands(name, x, raw, node_seg, t, n_graphs, cells, out):
    L.require_cuda(x, raw, node_seg, t, cells)
    x, raw, t = L.f32c(x.detach()), L.f32c(raw.detach()), L.f32c(t.detach()).reshape(-1)
    if x.dim() != 2 or raw.shape != x.shape or node_seg.dtype != torch.int64 or node_seg.numel() != x.shape[0] or not node_seg.is_contiguous():
        raise ValueError(f"{name} needs x, raw [N, D] and a contiguous int64 node_seg [N]")
    if t.numel() < int(n_graphs):
        raise ValueError(f"{name}: t holds {t.numel()} times for {int(n_graphs)} graphs")
    _check_cells(name, cells)
    if out is None:
        out = torch.empty_like(x)
    elif out.dtype != torch.float32 or out.shape != x.shape or not out.is_contiguous() or not out.is_cuda:
        raise ValueError(f"{name}: out must be a contiguous fp32 device tensor of x's shape")
    return x, raw, t, out


def _fixed_operands(name, x, known, fixed, out):
    """known [N, D] fp32 and the mask [N] uint8 of the FIXED forms, refused as their siblings' operands are"""
    L.require_cuda(known, fixed)
    known = L.f32c(known.detach())
    if known.shape != x.shape:
        raise ValueError(f"{name}: known must have x's shape {tuple(x.shape)} (got {tuple(known.shape)})")
    if fixed.dtype != torch.uint8 or fixed.numel() != x.shape[0] or not fixed.is_contiguous():
        raise ValueError(f"{name}: fixed must be a contiguous uint8 device tensor [N] (not zero: the row is fixed)")
    if known.data_ptr() == out.data_ptr():
        raise ValueError(f"{name}: out must not be the known values")
    return known


def _ode_operands(name, x, raw, node_seg, times, n_graphs, cells, out):
    """``_sampler_operands`` with the time table where its siblings take t: contiguous fp32 ``times`` [n >= 2] on the device"""
    L.require_cuda(times)
    x, raw, _, out = _sampler_operands(name, x, raw, node_seg, times, 0, cells, out)
    _check_times(name, times)
    if int(n_graphs) < 0:
        raise ValueError(f"{name}: n_graphs = {int(n_graphs)}")
    return x, raw, out


def _per_graph_operands(name, acc, x, row_ptr, n_graphs):
    L.require_cuda(acc, x, row_ptr)
    x = L.f32c(x.detach())
    if x.dim() != 2:
        raise ValueError(f"{name} needs [N, D] operands")
    if acc.dtype != torch.float64 or not acc.is_contiguous() or acc.numel() < int(n_graphs):
        raise ValueError(f"{name}: the accumulator must be a contiguous float64 device tensor of at least {int(n_graphs)} entries")
    if row_ptr.dtype != torch.int32 or not row_ptr.is_contiguous() or row_ptr.numel() < int(n_graphs) + 1 or int(n_graphs) < 0:
        raise ValueError(f"{name}: row_ptr must be a contiguous int32 device tensor [n_graphs + 1]")
    return x


# ---- training: the perturbation ------------------------------------------------------------------------------------------
def vpsde_perturb(x0, node_seg, n_graphs: int, beta_0: float, beta_1: float, eps: float, T: float, seed: int, draw, word0: int = 0):
    """The VP-SDE perturbation with counter-based draws (``csrc/e3k_score.hip``): ``(t [G + 1], x_t, z [N, D], std [N])`` for
    ``x0`` [N, D] and ``node_seg`` [N] int64; rows whose segment is not one of the ``n_graphs`` real graphs (the ghost graph of a
    padded batch) keep ``x0``, with ``z = 0``, ``std = 1`` and ``t = 0.5``.  ``draw``: a DEVICE int64 cell (its first element is the
    draw index; read, not written: a captured step hands in its own step counter).  One launch, no host synchronisation."""
    L.require_cuda(x0, node_seg, draw)
    x0 = L.f32c(x0.detach())
    if x0.dim() != 2 or node_seg.dtype != torch.int64 or node_seg.numel() != x0.shape[0] or not node_seg.is_contiguous():
        raise ValueError("vpsde_perturb needs x0 [N, D] and a contiguous int64 node_seg [N]")
    if draw.dtype != torch.int64 or draw.numel() < 1 or not draw.is_contiguous():
        raise ValueError("vpsde_perturb: draw must be a contiguous int64 device tensor (its first element is the draw index)")
    n, d = x0.shape
    t = torch.empty(n_graphs + 1, device=x0.device, dtype=torch.float32)
    x_t, z = torch.empty_like(x0), torch.empty_like(x0)
    std = torch.empty(n, device=x0.device, dtype=torch.float32)
    L.check(L.load().e3k_vpsde_perturb(L.ptr(x0), L.ptr(node_seg), n, d, int(n_graphs), float(beta_0), float(beta_1), float(eps), float(T),
                                       *L.seed_words(seed), L.ptr(draw), int(word0), L.ptr(t),
                                       L.ptr(x_t), L.ptr(z), L.ptr(std), L.stream_ptr()), "e3k_vpsde_perturb")
    return t, x_t, z, std


# ---- the seeded samplers -------------------------------------------------------------------------------------------------
def sampler_begin_step(times, cells, t) -> None:
    """The seeded sampler's step header (``csrc/e3k_sampler.hip``): with ``k = cells[0]`` inside the table ``times`` [n] fp32, every
    element of ``t`` (fp32, the ghost graph's included) becomes ``times[k]`` and ``cells`` (DEVICE int64 [2]) becomes ``(k + 1, k)``;
    outside the table nothing is written.  One launch, in place, no host synchronisation."""
    L.require_cuda(times, cells, t)
    if times.dtype != torch.float32 or t.dtype != torch.float32 or not times.is_contiguous() or not t.is_contiguous():
        raise ValueError("sampler_begin_step needs contiguous fp32 times [n] and t")
    _check_cells("sampler_begin_step", cells)
    L.check(L.load().e3k_sampler_begin_step(L.ptr(times), times.numel(), L.ptr(cells), L.ptr(t), t.numel(), L.stream_ptr()),
            "e3k_sampler_begin_step")


def sampler_langevin(x, raw, node_seg, t, alphas, n_graphs: int, beta_0: float, beta_1: float, T: float, snr: float, seed: int, cells,
                     word0: int = 0, out=None, known=None, fixed=None, word_fixed: int = 0):
    """One Langevin corrector update of a diffusion key with counter-based noise (``csrc/e3k_sampler.hip``): ``(x', norms [2])`` for
    ``x``, ``raw`` [N, D] (the score head's output: score = -raw / std(t) - x), ``t`` per graph and the ``alphas`` table; ``norms`` =
    (mean score row norm, mean noise row norm) over the rows of the ``n_graphs`` real graphs; the other rows (the ghost graph of a
    padded batch) are copied through.  The noise is draw ``cells[1]``, words ``word0 + c``.  ``out`` may be ``x``.  One launch.

    Conditional sampling (``fixed`` given: ``e3k_sampler_langevin_fixed``): the real rows whose ``fixed`` byte (uint8 [N]) is not zero
    become ``exp(lm(t)) known + std(t) z`` instead, z the draw ``cells[1]``'s words ``word_fixed + c`` (2 D_total + the key's first
    word); the norms run over all real rows all the same.  Still one launch."""
    name = "sampler_langevin" if fixed is None else "sampler_langevin_fixed"
    x, raw, t, out = _sampler_operands(name, x, raw, node_seg, t, n_graphs, cells, out)
    if fixed is not None:
        known = _fixed_operands(name, x, known, fixed, out)
    L.require_cuda(alphas)
    alphas = L.f32c(alphas).reshape(-1)
    n, d = x.shape
    norms = torch.empty(2, device=x.device, dtype=torch.float32)
    if fixed is None:
        L.check(L.load().e3k_sampler_langevin(L.ptr(out), L.ptr(x), L.ptr(raw), L.ptr(node_seg), L.ptr(t), L.ptr(alphas), n, d, int(n_graphs),
                                              alphas.numel(), float(beta_0), float(beta_1), float(T), float(snr), *L.seed_words(seed),
                                              L.ptr(cells), int(word0), L.ptr(norms), L.stream_ptr()), "e3k_sampler_langevin")
    else:
        L.check(L.load().e3k_sampler_langevin_fixed(L.ptr(out), L.ptr(x), L.ptr(raw), L.ptr(known), L.ptr(fixed), L.ptr(node_seg), L.ptr(t),
                                                    L.ptr(alphas), n, d, int(n_graphs), alphas.numel(), float(beta_0), float(beta_1),
                                                    float(T), float(snr), *L.seed_words(seed), L.ptr(cells), int(word0), int(word_fixed),
                                                    L.ptr(norms), L.stream_ptr()), "e3k_sampler_langevin_fixed")
    return out, norms


def sampler_reverse_em(x, raw, node_seg, t, n_graphs: int, beta_0: float, beta_1: float, n_sde: int, seed: int, cells, word0: int,
                       out=None, known=None, fixed=None, word_fixed: int = 0):
    """One Euler-Maruyama step of the reverse VP-SDE (``dt = -1 / n_sde``) of a diffusion key with counter-based noise
    (``csrc/e3k_sampler.hip``); operands as ``sampler_langevin``'s.  ``word0``: D_total + the key's first word (the predictor's words
    of the draw layout, ``csrc/e3k_draw.h``).  ``out`` may be ``x``.  One launch.

    Conditional sampling (``fixed`` given: ``e3k_sampler_reverse_em_fixed``): the fixed rows become ``exp(lm(t)) known + std(t) z`` at
    the step's own t, z at words ``word_fixed + c`` (3 D_total + the key's first word).  Still one launch."""
    name = "sampler_reverse_em" if fixed is None else "sampler_reverse_em_fixed"
    x, raw, t, out = _sampler_operands(name, x, raw, node_seg, t, n_graphs, cells, out)
    n, d = x.shape
    if fixed is None:
        L.check(L.load().e3k_sampler_reverse_em(L.ptr(out), L.ptr(x), L.ptr(raw), L.ptr(node_seg), L.ptr(t), n, d, int(n_graphs),
                                                float(beta_0), float(beta_1), int(n_sde), *L.seed_words(seed), L.ptr(cells), int(word0),
                                                L.stream_ptr()), "e3k_sampler_reverse_em")
    else:
        known = _fixed_operands(name, x, known, fixed, out)
        L.check(L.load().e3k_sampler_reverse_em_fixed(L.ptr(out), L.ptr(x), L.ptr(raw), L.ptr(known), L.ptr(fixed), L.ptr(node_seg), L.ptr(t),
                                                      n, d, int(n_graphs), float(beta_0), float(beta_1), int(n_sde), *L.seed_words(seed),
                                                      L.ptr(cells), int(word0), int(word_fixed), L.stream_ptr()), "e3k_sampler_reverse_em_fixed")
    return out


# ---- the probability-flow ODE --------------------------------------------------------------------------------------------
def sampler_ode_euler(x, raw, node_seg, times, cells, n_graphs: int, beta_0: float, beta_1: float, t_out=None, want_d: bool = True,
                      out=None):
    """One Euler step of the probability-flow ODE of a diffusion key, which is Heun's stage A (``e3k_sampler_ode_euler``):
    ``(x + h d1, d1)`` with ``d1 = (0.5 beta(t_k)) (raw / s(t_k))``, ``k = cells[1]``, ``t_k = times[k]``, ``h = times[k + 1] - t_k``
    read from the table on the device; ``d1`` is None without ``want_d``.  ``t_out`` (contiguous fp32, the batch's t): every element
    becomes ``times[k + 1]`` in the same launch.  Rows outside the ``n_graphs`` real graphs are copied through (``d1 = 0``), and so is
    everything when ``k`` or ``k + 1`` is outside the table.  ``out`` may be ``x``.  One launch."""
    x, raw, out = _ode_operands("sampler_ode_euler", x, raw, node_seg, times, n_graphs, cells, out)
    g1 = 0
    if t_out is not None:
        L.require_cuda(t_out)
        if t_out.dtype != torch.float32 or not t_out.is_contiguous() or t_out.numel() < 1:
            raise ValueError("sampler_ode_euler: t_out must be a contiguous fp32 device tensor")
        g1 = t_out.numel()
    d = torch.empty_like(x) if want_d else None
    n, dim = x.shape
    L.check(L.load().e3k_sampler_ode_euler(L.ptr(out), L.ptr(d), L.ptr(x), L.ptr(raw), L.ptr(node_seg), L.ptr(times),
                                           times.numel(), L.ptr(cells), L.ptr(t_out), g1, n, dim,
                                           int(n_graphs), float(beta_0), float(beta_1), L.stream_ptr()), "e3k_sampler_ode_euler")
    return out, d


def sampler_ode_heun(x0, d1, raw2, node_seg, times, cells, n_graphs: int, beta_0: float, beta_1: float, out=None):
    """Heun's stage B of the same step (``e3k_sampler_ode_heun``): ``x0 + (0.5 h) (d1 + d2)`` with ``d2 = (0.5 beta(t_{k+1}))
    (raw2 / s(t_{k+1}))``; ``x0``, ``d1``: the state before stage A and its drift, ``raw2``: the model's output at the stage-A state.
    Ghost rows and steps outside the table: ``x0``.  ``out`` may be ``x0``, never ``d1``.  One launch."""
    x0, raw2, out = _ode_operands("sampler_ode_heun", x0, raw2, node_seg, times, n_graphs, cells, out)
    L.require_cuda(d1)
    d1 = L.f32c(d1.detach())
    if d1.shape != x0.shape:
        raise ValueError(f"sampler_ode_heun: d1 must have x0's shape {tuple(x0.shape)} (got {tuple(d1.shape)})")
    if d1.data_ptr() == out.data_ptr():
        raise ValueError("sampler_ode_heun: out must not be d1")
    n, dim = x0.shape
    L.check(L.load().e3k_sampler_ode_heun(L.ptr(out), L.ptr(x0), L.ptr(d1), L.ptr(raw2), L.ptr(node_seg), L.ptr(times), times.numel(),
                                          L.ptr(cells), n, dim, int(n_graphs), float(beta_0), float(beta_1), L.stream_ptr()),
            "e3k_sampler_ode_heun")
    return out


# ---- the likelihood ------------------------------------------------------------------------------------------------------
def graph_row_pointers(counts) -> torch.Tensor:
    """int32 [G + 1] row pointers of per-graph node counts (contiguous int64 on the device): one ``e3k_counts_to_ptr`` launch"""
    L.require_cuda(counts)
    n = counts.reshape(-1)
    if n.dtype != torch.int64 or not n.is_contiguous():
        raise ValueError("graph_row_pointers needs contiguous int64 counts")
    ptr = torch.empty(n.numel() + 1, dtype=torch.int32, device=n.device)
    L.check(L.load().e3k_counts_to_ptr(L.ptr(n), n.numel(), L.ptr(ptr), L.stream_ptr()), "e3k_counts_to_ptr")
    return ptr


def sampler_probe(node_seg, dim: int, n_graphs: int, seed: int, draw: int, word0: int, kind: int) -> torch.Tensor:
    """The Hutchinson probe of one diffusion key (``e3k_sampler_probe``): fp32 [N, dim], component c of node i from draw index
    ``draw``, word ``word0 + c`` of the stream of ``csrc/e3k_draw.h`` -- ``kind`` 0: Rademacher (``data.compute_edge.rademacher_draw``),
    1: ``normal_draw``; rows outside the ``n_graphs`` real graphs are 0.  One launch."""
    L.require_cuda(node_seg)
    if node_seg.dtype != torch.int64 or node_seg.dim() != 1 or not node_seg.is_contiguous():
        raise ValueError("sampler_probe needs a contiguous int64 node_seg [N]")
    out = torch.empty(node_seg.numel(), int(dim), device=node_seg.device, dtype=torch.float32)
    L.check(L.load().e3k_sampler_probe(L.ptr(out), L.ptr(node_seg), node_seg.numel(), int(dim), int(n_graphs), *L.seed_words(seed),
                                       int(draw) & 0xFFFFFFFF, int(word0), int(kind), L.stream_ptr()), "e3k_sampler_probe")
    return out


def sampler_ode_div(acc, probe, vjp, row_ptr, times, cells, n_graphs: int, stage: int, scale: float, beta_0: float, beta_1: float) -> None:
    """One quadrature term of the likelihood's integral, in place (``e3k_sampler_ode_div``): ``acc[g] += w c(t) scale sum(probe vjp)``
    over the rows of each of the ``n_graphs`` real graphs; ``acc`` float64 on the device, ``row_ptr`` int32 ``[n_graphs + 1]``, the step
    ``k = cells[1]`` and its times from the table.  ``stage`` 0: ``w = h``, ``t = t_k``; 1: ``h / 2``, ``t_k``; 2: ``h / 2``,
    ``t_{k+1}``; ``c(t) = (0.5 beta(t)) / s(t)`` in double.  Outside the table nothing is written.  One launch."""
    vjp = _per_graph_operands("sampler_ode_div", acc, vjp, row_ptr, n_graphs)
    L.require_cuda(probe, times, cells)
    probe = L.f32c(probe.detach())
    if probe.shape != vjp.shape:
        raise ValueError(f"sampler_ode_div: probe {tuple(probe.shape)} and vjp {tuple(vjp.shape)} differ in shape")
    _check_times("sampler_ode_div", times)
    _check_cells("sampler_ode_div", cells)
    n, dim = vjp.shape
    L.check(L.load().e3k_sampler_ode_div(L.ptr(acc), L.ptr(probe), L.ptr(vjp), L.ptr(row_ptr), L.ptr(times), times.numel(), L.ptr(cells), n,
                                         dim, int(n_graphs), int(stage), float(scale), float(beta_0), float(beta_1), L.stream_ptr()),
            "e3k_sampler_ode_div")


def sampler_prior_logp(out, x, row_ptr, n_graphs: int) -> None:
    """``out[g] += log N(x_g; 0, I)`` over the rows of each real graph, in place (``e3k_sampler_prior_logp``; ``out`` float64)."""
    x = _per_graph_operands("sampler_prior_logp", out, x, row_ptr, n_graphs)
    n, dim = x.shape
    L.check(L.load().e3k_sampler_prior_logp(L.ptr(out), L.ptr(x), L.ptr(row_ptr), n, dim, int(n_graphs), L.stream_ptr()),
            "e3k_sampler_prior_logp")
