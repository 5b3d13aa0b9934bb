"""Edge geometry entry points of the layer graph.

``computeEdgeVector`` mirrors ``e3_layers/data/compute_edge.py:13-36`` (edge_vec = pos[dst] -
pos[src], edge_length) and runs the HIP kernel of ``csrc/e3k_edge.hip``; as the first layer of
every model (``e3_layers/configs/layer_configs.py:43``) it also attaches the per-batch CSR
topology the fused convolution needs (``backend/graph.py``).

``computeEdgeIndex`` mirrors ``e3_layers/data/compute_edge.py:38-113`` with the intent recorded
in SURVEY.md appendix C: per graph all ordered pairs in (src slow, dst fast) order, keep
``|pos_src - pos_dst| < r_max`` (strict, fp32) or ``criteria``, drop self loops, keep
pre-existing edges and carry their edge attributes (zero rows for new edges).  On CPU tensors
(dataset preprocessing, as in the reference) it is vectorised torch integer plumbing; on device
tensors without a ``criteria`` callback it runs the two-pass HIP radius-graph kernels
(``e3k_radius_graph_count/fill``: one wave per source node, ballot compaction keeps the
reference's edge order without a sort) — the per-step edge rebuild of the sampling loop
(``e3_layers/run/sde_sampling.py:237-242``) then never leaves the GPU.  ``criteria`` callbacks are
arbitrary Python over the candidate list and keep the torch path on whichever device holds the data.

``PairCriterion`` / ``SequenceOrRandom`` state the protein nets' pair rule (``e3_layers/configs/config_diffusion_CA.py:58-64``: same
chain and ``|i - j| < 5``, or a 2 % random subset) declaratively: as a ``criteria`` callback it is the torch restatement of the rule, and
the capped builder below evaluates the same rule -- the same counter-based draws, bit for bit -- inside its kernels.

``computeEdgeIndexCapped`` is the same radius graph for loops that call the model over and over while the atoms move (MD, relaxation,
the reverse-diffusion loop on cutoff graphs): it rewrites the FIXED ``[2, e_cap]`` ``edge_index`` of a batch padded by
``run/graph_step.pad_batch`` in place (``csrc/e3k_nlist.hip``), reads nothing back, and is therefore part of a captured HIP graph.
``computeEdgeIndex`` hands a batch that carries ``_nlist_state`` (the marker the capped loops put into their padded batch) over to it:
a model that owns its ``edge_index`` layer gets the capped build inside a capture without knowing of it.
"""
from __future__ import annotations

import math
from typing import Dict, Tuple

import torch
from torch import Tensor

from ..backend import lib as L
from ..backend import memo, ops
from ..backend.graph import (NLIST_OVERFLOW, TOPO_KEYS, EdgeCapacityExceeded, check_indices, get_topology, persistent_flag)
from .data import segment_ids


def computeEdgeVector(data: Dict[str, Tensor], attrs: Dict[str, Tuple[str, str]], key: str = "pos",
                      with_lengths: bool = True):
    attrs["edge_vector"] = ("edge", "1x1o")
    attrs["edge_length"] = ("edge", "1x0e")
    pos = data[key]
    if "edge_vector" in data:
        if with_lengths and "edge_length" not in data:
            data["edge_length"] = torch.linalg.norm(data["edge_vector"], dim=-1)
        return data, attrs
    topo = get_topology(data, pos.shape[0])
    data.update(topo.as_dict())
    vec, length = ops.edge_vector(pos, topo)
    # functions of the input positions alone: no gradient under ops.params_only_backward()
    from_input = pos.grad_fn is None and not isinstance(pos, torch.nn.Parameter)
    ops.mark_data_only(vec, from_input)
    ops.mark_data_only(length, from_input)
    data["edge_vector"] = vec
    if with_lengths:
        data["edge_length"] = length
    return data, attrs


computeEdgeVector.data_only_inputs = ("pos", "edge_index")      # (SequentialGraphNetwork.prepare_data: parameter-free, reads these keys)


# ---------------------------------------------------------------------------------------------------------------------
# Declarative pair criteria: a rule on ordered candidate pairs that the torch path AND the capped builder's kernels evaluate
# ---------------------------------------------------------------------------------------------------------------------
_M32 = 0xFFFFFFFF


def _mix32(h):
    """One round of the "lowbias32" finaliser on int64 values in [0, 2^32): an int64 multiply wraps and keeps the low 32 bits, the
    mask throws the rest away -- the kernel's uint32 arithmetic (``csrc/e3k_draw.h: mix32``), bit for bit."""
    h = h ^ (h >> 16)
    h = (h * 0x7feb352d) & _M32
    h = h ^ (h >> 15)
    h = (h * 0x846ca68b) & _M32
    return h ^ (h >> 16)


def pair_hash(seed, draw, src, dst) -> Tensor:
    """The 32-bit hash of (seed low, seed high, draw index, src, dst) as an int64 tensor in [0, 2^32): ``h = mix(h ^ word)`` over the
    five words (each taken modulo 2^32) from ``0x9E3779B9``.  Every argument is an int or an int64 tensor; they broadcast."""
    dev = next((x.device for x in (src, dst, draw, seed) if torch.is_tensor(x)), None)

    def word(x):
        return torch.as_tensor(x, dtype=torch.int64, device=dev) & _M32

    if torch.is_tensor(seed):
        lo, hi = word(seed), word(torch.as_tensor(seed, dtype=torch.int64, device=dev) >> 32)
    else:
        lo, hi = word(int(seed) & _M32), word((int(seed) >> 32) & _M32)
    h = _mix32(lo ^ 0x9E3779B9)
    for w in (hi, word(draw), word(src), word(dst)):
        h = _mix32(h ^ w)
    return h


def normal_draw(seed, draw, node, word, dtype=torch.float32) -> Tensor:
    """The counter-based standard normal of the device's draw stream (``csrc/e3k_draw.h: normal_draw``) for (seed, draw index,
    node, word): ``u1 = ((h1 >> 8) + 1) 2^-24`` in (0, 1] and ``u2 = (h2 >> 8) 2^-24`` in [0, 1) from
    ``h1, h2 = pair_hash(seed, draw, node, 2 word), pair_hash(seed, draw, node, 2 word + 1)`` -- bit for bit the kernel's -- and
    ``sqrt(-2 ln u1) cos(2 pi u2)`` in ``dtype`` through torch (the kernel: fp32 ``logf``, ``sqrtf``, ``cospif``).  Component c of a
    step's thermostat draw is word c with the step number as draw index; ``thermalize`` uses words 4 + c and a counter of its own.
    The seeded sampler (``run/sde_utils.py``): with ``word0`` the sum of the dimensions of the diffusion keys before a key and
    ``D_total`` the sum over all of them, reverse step i draws index i -- word ``word0 + c`` for the corrector, ``D_total + word0 + c``
    for the predictor -- and the prior draws index ``sde.N``, word ``word0 + c``.
    Arguments as ``pair_hash``'s: ints or int64 tensors, broadcasting."""
    two_w = 2 * (word if torch.is_tensor(word) else int(word))
    u1 = ((pair_hash(seed, draw, node, two_w) >> 8) + 1).to(dtype) * 2.0 ** -24
    u2 = (pair_hash(seed, draw, node, two_w + 1) >> 8).to(dtype) * 2.0 ** -24
    return torch.sqrt(-2.0 * torch.log(u1)) * torch.cos((2.0 * math.pi) * u2)


def rademacher_draw(seed, draw, node, word, dtype=torch.float32) -> Tensor:
    """The counter-based Rademacher draw of the device's stream (``csrc/e3k_draw.h``; ``e3k_sampler_probe`` kind 0) for (seed, draw
    index, node, word): ``+1`` when bit 31 of ``pair_hash(seed, draw, node, 2 word)`` is clear, ``-1`` when it is set -- bit for bit
    the kernel's.  The likelihood's Hutchinson probes (``run/likelihood.py``): probe p of component c of a diffusion key draws index
    ``sde.N + 1 + p``, word ``word0 + c`` (no step and not the prior, index ``sde.N``, uses these indices); the Gaussian probe is
    ``normal_draw`` at the same index and word.  Arguments as ``pair_hash``'s."""
    two_w = 2 * (word if torch.is_tensor(word) else int(word))
    return (1 - 2 * (pair_hash(seed, draw, node, two_w) >> 31)).to(dtype)


class PairCriterion:
    """A pair rule both edge builders recognise.  As a callable it is a ``criteria`` callback of ``computeEdgeIndex``
    (``(data, edge_index) -> bool mask`` over the ordered candidate pairs, global node indices); ``computeEdgeIndexCapped`` does not
    call it: it evaluates the rule's terms (``segment``, ``window``, ``threshold``, ``keep_all``, ``seed``) in its kernels."""

    segment, window, p, seed = None, 0, 0.0, 0

    def __init__(self):
        self._draw = 0

    def reset(self, draw: int = 0) -> None:
        """The draw index the next call WITHOUT device cells uses (the host-side counter; it goes up by one per call)."""
        self._draw = int(draw)

    @property
    def threshold(self) -> int:
        """floor(p 2^32), the bound a pair's hash stays below to be drawn (p = 1 does not fit 32 bits: ``keep_all``)."""
        return min(int(math.floor(self.p * 4294967296.0)), _M32)

    @property
    def keep_all(self) -> bool:
        return self.p >= 1.0

    def predicate(self, data, edge_index: Tensor, draw) -> Tensor:
        """The rule at draw index ``draw`` (an int, or an int64 tensor on the candidates' device): bool [n_candidates]."""
        src, dst = edge_index[0], edge_index[1]
        keep = torch.zeros(src.shape[0], dtype=torch.bool, device=src.device)
        if self.window > 0 and self.segment is not None:
            seg = _segment_key(data, self.segment, None).to(src.device)
            keep = torch.logical_and(seg[src] == seg[dst], (src - dst).abs() < self.window)
        if self.keep_all:
            return torch.ones_like(keep)
        if self.threshold > 0:
            keep = torch.logical_or(keep, pair_hash(self.seed, draw, src, dst) < self.threshold)
        return keep

    def __call__(self, data, edge_index: Tensor) -> Tensor:
        rng = data["_nlist_rng"] if "_nlist_rng" in data else None
        if rng is not None:      # the batch's device cells name the draw (read, never written here: the capped builder advances them)
            return self.predicate(data, edge_index, rng.reshape(-1)[0].to(edge_index.device))
        draw = self._draw
        self._draw += 1
        return self.predicate(data, edge_index, draw)


class SequenceOrRandom(PairCriterion):
    """``(segment[src] == segment[dst] and |src - dst| < window) or bernoulli(p)`` on global node indices -- the shipped protein rule
    is ``SequenceOrRandom("chain_id", 5, 0.02)``.  ``window=0`` switches the sequence term off, ``p=0`` the random one; ``p=1`` keeps
    every candidate.  The Bernoulli draw is counter-based and stateless per pair: ``pair_hash(seed, draw, src, dst) < floor(p 2^32)``,
    where ``draw`` is the number of the list build -- the same for every pair of one build, one more for the next build.  ``seed``
    should differ from the seeded sampler's (``get_pc_sampler(seed=...)``): the two streams share the hash, and with one seed a node's
    noise and the Bernoulli draws of its pairs come from one chain."""

    def __init__(self, segment: str = "chain_id", window: int = 5, p: float = 0.02, seed: int = 0):
        super().__init__()
        if window < 0 or not 0.0 <= p <= 1.0 or not 0 <= int(seed) < 1 << 64:
            raise ValueError("SequenceOrRandom needs window >= 0, 0 <= p <= 1 and a seed of at most 64 bits")
        self.segment, self.window, self.p, self.seed = segment, int(window), float(p), int(seed)

    def __repr__(self):
        return f"SequenceOrRandom(segment={self.segment!r}, window={self.window}, p={self.p}, seed={self.seed})"


def _segment_key(data, name: str, n_nodes) -> Tensor:
    """The criterion's segment field of the batch as int64 [N] (stored as [N] or [N, 1])."""
    if name not in data:
        raise ValueError(f"the pair criterion's segment field {name!r} is not in the batch")
    seg = data[name]
    if seg.dtype != torch.int64 or seg.dim() not in (1, 2) or (seg.dim() == 2 and seg.shape[1] != 1) or \
            (n_nodes is not None and seg.shape[0] != n_nodes):
        raise ValueError(f"the pair criterion's segment field {name!r} must be an int64 tensor of shape [N] or [N, 1] "
                         f"(got {str(seg.dtype).replace('torch.', '')} {tuple(seg.shape)})")
    return seg.reshape(-1)


def _all_pairs(n_nodes: Tensor, device) -> Tensor:
    """[2, sum n_g^2] candidate edges, graphs concatenated, (i, j) lexicographic inside a graph; built on ``device``
    (one host sync for the candidate count when the counts live on the GPU)."""
    dev = torch.device(device)
    n = n_nodes.reshape(-1).to(dev, torch.long)
    if n.numel() == 0:
        return torch.zeros(2, 0, dtype=torch.long, device=dev)
    sq = n * n
    total_sq = int(sq.sum())
    if total_sq == 0:
        return torch.zeros(2, 0, dtype=torch.long, device=dev)
    start = torch.cumsum(n, 0) - n
    graph = segment_ids(sq, total_sq)
    local = torch.arange(total_sq, device=dev) - (torch.cumsum(sq, 0) - sq)[graph]
    ng = n[graph]
    src = torch.div(local, ng, rounding_mode="floor") + start[graph]
    dst = local % ng + start[graph]
    return torch.stack([src, dst])


_STALE = ("_edge_segment",) + TOPO_KEYS + ("edge_vector", "edge_length")


def _radius_graph_device(data, attrs, pos: Tensor, r_max: float):
    """HIP path: edge_index [2,E] int64 in the reference's order, `_n_edges`, carried-over edge attributes."""
    dev = pos.device
    pos = L.f32c(pos.detach())
    n = data["_n_nodes"].reshape(-1).to(dev)
    total = pos.shape[0]
    n_graphs = n.numel()
    gid = segment_ids(n, total)
    ends = torch.cumsum(n, 0)
    g_end = ends[gid].to(torch.int32)
    g_start = (ends - n)[gid].to(torch.int32)
    old_ptr = old_dst = old_id = None
    if "edge_index" in data:
        old = data["edge_index"].to(dev)
        if old.numel() and not bool((gid[old[0]] == gid[old[1]]).all()):
            raise ValueError("an existing edge connects two different graphs")
        old_id = old[0] * total + old[1]
        order = torch.argsort(old_id)
        old_dst = old[1][order].to(torch.int32).contiguous()
        old_ptr = torch.zeros(total + 1, dtype=torch.int32, device=dev)
        old_ptr[1:] = torch.cumsum(torch.bincount(old[0], minlength=total), 0).to(torch.int32)
    lib = L.load()
    counts = torch.empty(total, dtype=torch.int32, device=dev)
    L.check(lib.e3k_radius_graph_count(L.ptr(pos), L.ptr(g_start), L.ptr(g_end), total, float(r_max), L.ptr(old_ptr),
                                       L.ptr(old_dst), L.ptr(counts), L.stream_ptr()), "e3k_radius_graph_count")
    incl = torch.cumsum(counts, 0, dtype=torch.int64)
    offsets = (incl - counts).contiguous()
    n_edge = int(incl[-1].item()) if total else 0          # the one host sync: the size of the output
    edge_index = torch.empty(2, n_edge, dtype=torch.int64, device=dev)
    L.check(lib.e3k_radius_graph_fill(L.ptr(pos), L.ptr(g_start), L.ptr(g_end), total, float(r_max), L.ptr(old_ptr),
                                      L.ptr(old_dst), L.ptr(offsets), n_edge, L.ptr(edge_index), L.stream_ptr()),
            "e3k_radius_graph_fill")
    if old_id is not None:
        where = torch.searchsorted(edge_index[0] * total + edge_index[1], old_id)
        for k in list(attrs.keys()):
            if attrs[k][0] == "edge" and k in data:
                prev = data[k].to(dev)
                fresh = torch.zeros((n_edge,) + tuple(prev.shape[1:]), dtype=prev.dtype, device=dev)
                fresh[where] = prev
                data[k] = fresh
    per_graph = torch.zeros(n_graphs, dtype=torch.int64, device=dev).index_add_(0, gid, counts.to(torch.int64))
    attrs["_n_edges"] = ("graph", "1x0e")
    data["_n_edges"] = per_graph.view(-1, 1)
    for k in _STALE:
        data.pop(k, None)
    return {"edge_index": edge_index}, attrs


def computeEdgeIndex(data, attrs, r_max: float = None, key: str = "pos", criteria=None):
    if "_nlist_state" in data:      # a padded batch of a capped loop: the fixed-size list, rewritten in place inside the capture
        return computeEdgeIndexCapped(data, attrs, r_max=r_max, key=key, criteria=criteria)
    pos = torch.as_tensor(data[key], dtype=torch.get_default_dtype())
    if pos.is_cuda and criteria is None and r_max is not None:
        return _radius_graph_device(data, attrs, pos, r_max)
    n_nodes = data["_n_nodes"]
    total = pos.shape[0]
    cand = _all_pairs(n_nodes, pos.device)
    dist = torch.linalg.norm(pos[cand[0]] - pos[cand[1]], dim=-1)
    keep = dist < r_max
    if criteria is not None:
        keep = torch.logical_or(keep, criteria(data, cand))
    keep = torch.logical_and(keep, cand[0] != cand[1])
    had_edges = "edge_index" in data
    if had_edges:
        old = data["edge_index"]
        old_id = old[0] * total + old[1]
        cand_id = cand[0] * total + cand[1]          # strictly increasing
        at = torch.searchsorted(cand_id, old_id)
        if not bool((cand_id[at.clamp(max=cand_id.numel() - 1)] == old_id).all()):
            raise ValueError("an existing edge connects two different graphs")
        keep[at] = True
    edge_index = cand[:, keep]
    if had_edges:
        where = torch.searchsorted(edge_index[0] * total + edge_index[1], old_id)
        for k in list(attrs.keys()):
            if attrs[k][0] == "edge" and k in data:
                prev = data[k]
                fresh = torch.zeros((edge_index.shape[1],) + tuple(prev.shape[1:]), dtype=prev.dtype, device=pos.device)
                fresh[where] = prev
                data[k] = fresh
    seg = segment_ids(n_nodes.reshape(-1).to(pos.device))
    n_edges = torch.bincount(seg[edge_index[0]], minlength=n_nodes.numel()).view(-1, 1)
    attrs["_n_edges"] = ("graph", "1x0e")
    data["_n_edges"] = n_edges
    # stale per-edge caches belong to the old edge set
    for k in _STALE:
        data.pop(k, None)
    return {"edge_index": edge_index}, attrs


# ---------------------------------------------------------------------------------------------------------------------
# The capped neighbour list: a radius graph of fixed size, rebuilt on the device inside a captured graph
# ---------------------------------------------------------------------------------------------------------------------
def ghost_tail(n_ghost: int, n_edges: int, first_node: int = 0) -> Tensor:
    """The ghost edges that fill the slots behind the real edges of a capped list, [2, n_edges] int64: edge k joins the ghost nodes
    a = k % (n_ghost - 1) and a + 1, from a to a + 1 on even rounds k // (n_ghost - 1) and back on odd ones -- what
    ``run/graph_step.ghost_sample(like, n_ghost, n_edges)`` gives, offset by the ghost graph's first node.  The fill kernel of
    ``csrc/e3k_nlist.hip`` computes exactly this from ``k - E_real``; this restatement is what the host tests hold it to."""
    if n_edges and n_ghost < 2:
        raise ValueError(f"a ghost graph with {n_edges} edges needs at least two nodes (got {n_ghost})")
    k = torch.arange(n_edges, dtype=torch.int64)
    m = max(n_ghost - 1, 1)
    a = k % m
    flip = (k // m) % 2 == 1
    return torch.stack([torch.where(flip, a + 1, a), torch.where(flip, a, a + 1)]) + first_node


_nlist_states: dict = {}      # device index -> int64 [2]: E_real of the last build, overflow count


def nlist_state(device) -> Tensor:
    """The device's bookkeeping cells of the capped builder for batches that carry none of their own (``_nlist_state``):
    int64 [2] = (E_real of the last build, number of builds that overflowed since the last check).  Allocated on first use,
    OUTSIDE a capture."""
    idx = device.index if device.index is not None else torch.cuda.current_device()
    st = _nlist_states.get(idx)
    if st is None:
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("nlist_state() must be called before the capture starts (give the batch a '_nlist_state' tensor)")
        st = _nlist_states[idx] = torch.zeros(2, dtype=torch.int64, device=torch.device("cuda", idx))
    return st


_nlist_rngs: dict = {}        # device index -> int64 [2]: next draw index, draw index in use


def nlist_rng(device) -> Tensor:
    """The device's draw-index cells of the capped builder's criterion form for batches that carry none (``_nlist_rng``): int64 [2] =
    (draw index of the next build, draw index of the build in progress).  Allocated on first use, OUTSIDE a capture."""
    idx = device.index if device.index is not None else torch.cuda.current_device()
    rng = _nlist_rngs.get(idx)
    if rng is None:
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("nlist_rng() must be called before the capture starts (give the batch a '_nlist_rng' tensor)")
        rng = _nlist_rngs[idx] = torch.zeros(2, dtype=torch.int64, device=torch.device("cuda", idx))
    return rng


def check_edge_capacity(state: Tensor = None, device=None) -> None:
    """Blocks until the device is idle, then raises ``EdgeCapacityExceeded`` if a capped build overflowed since the last check (the
    overflow counter of ``state``, the device's persistent flag bit, or a flag copy already on its way home) -- and clears all three."""
    dev = state.device if state is not None else torch.device(device if device is not None else "cuda")
    if dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    state = nlist_state(dev) if state is None else state
    over = False
    while True:      # (every replay since the overflow sent a flagged copy home: each raise hands over one of them)
        try:
            check_indices()
            break
        except EdgeCapacityExceeded:
            over = True
    flag = persistent_flag(dev)
    if int(flag) & NLIST_OVERFLOW:
        over = True
        flag.bitwise_and_(~NLIST_OVERFLOW)
    if int(state[1]) > 0:
        over = True
        state[1:].zero_()
    if over:
        raise EdgeCapacityExceeded(f"a capped neighbour list needed {int(state[0])} edges at its last build and overflowed its capacity "
                                   "since the last check: grow the capacity and redo the steps since then")


def _node_pointers(n_nodes: Tensor) -> Tensor:
    """int64 [G + 2] first node of every graph of a padded batch, remembered on the counts tensor (they do not move with the atoms)."""
    ptr = memo.recall(n_nodes, "nlist_ptr")
    if ptr is None:
        ptr = torch.zeros(n_nodes.numel() + 1, dtype=torch.int64, device=n_nodes.device)
        ptr[1:] = torch.cumsum(n_nodes.reshape(-1), 0)
    return ptr


def computeEdgeIndexCapped(data, attrs, r_max: float = None, key: str = "pos", criteria=None):
    """The radius graph of ``computeEdgeIndex`` on a batch padded by ``run/graph_step.pad_batch`` (recognised by ``_graph_weight``;
    its last graph is the ghost graph), written IN PLACE into the batch's ``edge_index`` [2, e_cap], ``_n_edges`` and ``_edge_segment``:
    the real graphs' edges in the reference's order, then the ghost edges of ``ghost_tail`` -- for positions that fit, bit for bit
    ``pad_batch(batch with computeEdgeIndex's edges, n_cap, e_cap)``.  No host synchronisation, legal under stream capture; the
    per-edge caches of the old list are dropped and every memo on the batch is forgotten (the recording rule of ``backend/memo.py``:
    the CSR build and the knot bins that follow belong to the captured graph).

    More than ``e_cap`` edges: the list is cut (valid indices), bit ``NLIST_OVERFLOW`` of the device's persistent flag is set and the
    overflow counter (``data['_nlist_state'][1]``, else ``nlist_state(device)``) goes up: ``check_edge_capacity`` raises.

    ``criteria``: a ``PairCriterion`` -- a pair is kept inside the cutoff OR by the rule, which the kernels evaluate (the segment field
    is read from the batch; the draw index from ``data['_nlist_rng']``, int64 [2], else ``nlist_rng(device)``: every build draws with
    the first cell and adds one to it).  The list then equals ``computeEdgeIndex(criteria=...)``'s at the same draw index.

    Not served (``computeEdgeIndex`` does both, eagerly): ``criteria`` callbacks that are arbitrary Python, edges kept from before with
    carried attributes."""
    if criteria is not None and not isinstance(criteria, PairCriterion):
        raise ValueError("computeEdgeIndexCapped takes no criteria callback (arbitrary Python over the candidate list), only a "
                         "PairCriterion: use computeEdgeIndex")
    if r_max is None:
        raise ValueError("computeEdgeIndexCapped needs r_max")
    data = getattr(data, "data", data)      # (a Batch: its tensor dict, as the layer graph hands it over)
    if "_graph_weight" not in data or "edge_index" not in data or "_n_edges" not in data:
        raise ValueError("computeEdgeIndexCapped needs a batch padded by run.graph_step.pad_batch (it carries _graph_weight, and the "
                         "edge_index / _n_edges buffers that are rewritten in place)")
    carried = [k for k, v in attrs.items() if v[0] == "edge" and k in data and k not in ("edge_vector", "edge_length")]
    if carried:
        raise ValueError(f"computeEdgeIndexCapped rebuilds the whole list: the edge attributes {carried} cannot be carried over "
                         "(computeEdgeIndex keeps pre-existing edges and their attributes)")
    pos, ei, n_edges = data[key], data["edge_index"], data["_n_edges"]
    seg = data.get("_edge_segment")
    L.require_cuda(pos, ei, n_edges, seg)
    if pos.dtype != torch.float32 or not pos.is_contiguous() or pos.dim() != 2 or pos.shape[1] != 3:
        raise ValueError("positions must be a contiguous fp32 [N, 3] tensor")
    total, e_cap = pos.shape[0], ei.shape[1]
    n_nodes = data["_n_nodes"]
    n_graphs = n_nodes.numel() - 1      # real graphs
    for name, t, numel in (("edge_index", ei, 2 * e_cap), ("_n_edges", n_edges, n_graphs + 1), ("_edge_segment", seg, e_cap)):
        if t is not None and (t.dtype != torch.int64 or not t.is_contiguous() or t.numel() != numel):
            raise ValueError(f"{name} must be a contiguous int64 tensor of {numel} elements to be rewritten in place")
    if n_graphs < 0 or data["_graph_weight"].numel() != n_graphs + 1:
        raise ValueError("_graph_weight and _n_nodes disagree on the number of graphs")
    dev = pos.device
    node_seg = data.get("_node_segment")
    if node_seg is None or node_seg.device != dev or node_seg.numel() != total:
        node_seg = segment_ids(n_nodes.to(dev), total)
    node_seg = node_seg.contiguous()
    node_ptr = _node_pointers(n_nodes)
    state = data["_nlist_state"] if "_nlist_state" in data else nlist_state(dev)
    flag = persistent_flag(dev)
    seg_key = rng = None
    if criteria is not None:
        if criteria.window > 0 and criteria.segment is not None:
            seg_key = _segment_key(data, criteria.segment, total)
            L.require_cuda(seg_key)
            if not seg_key.is_contiguous():
                raise ValueError(f"the pair criterion's segment field {criteria.segment!r} must be contiguous")
        rng = data["_nlist_rng"] if "_nlist_rng" in data else nlist_rng(dev)
        L.require_cuda(rng)
        if rng.dtype != torch.int64 or not rng.is_contiguous() or rng.numel() != 2:
            raise ValueError("_nlist_rng must be a contiguous int64 tensor of 2 elements (next draw index, draw index in use)")
    lib = L.load()
    counts = torch.empty(total, dtype=torch.int32, device=dev)
    offsets = torch.empty(total + 1, dtype=torch.int64, device=dev)
    pos_d = pos.detach()
    if criteria is None:
        L.check(lib.e3k_nlist_count(L.ptr(pos_d), L.ptr(node_seg), L.ptr(node_ptr), total, n_graphs, float(r_max), L.ptr(counts),
                                    L.stream_ptr()), "e3k_nlist_count")
        L.check(lib.e3k_nlist_fill(L.ptr(pos_d), L.ptr(node_seg), L.ptr(node_ptr), total, n_graphs, float(r_max), L.ptr(counts), e_cap,
                                   L.ptr(offsets), L.ptr(ei), L.ptr(n_edges), L.ptr(seg), L.ptr(state), L.ptr(flag), L.stream_ptr()),
                "e3k_nlist_fill")
    else:
        rule = (L.ptr(seg_key), criteria.window, criteria.threshold, int(criteria.keep_all), *L.seed_words(criteria.seed), L.ptr(rng))
        L.check(lib.e3k_nlist_count_crit(L.ptr(pos_d), L.ptr(node_seg), L.ptr(node_ptr), total, n_graphs, float(r_max), *rule,
                                         L.ptr(counts), L.stream_ptr()), "e3k_nlist_count_crit")
        L.check(lib.e3k_nlist_fill_crit(L.ptr(pos_d), L.ptr(node_seg), L.ptr(node_ptr), total, n_graphs, float(r_max), *rule,
                                        L.ptr(counts), e_cap, L.ptr(offsets), L.ptr(ei), L.ptr(n_edges), L.ptr(seg), L.ptr(state),
                                        L.ptr(flag), L.stream_ptr()), "e3k_nlist_fill_crit")
    attrs["_n_edges"] = ("graph", "1x0e")
    for k in TOPO_KEYS + ("edge_vector", "edge_length"):
        data.pop(k, None)
    memo.forget(data)
    memo.remember(n_nodes, "nlist_ptr", node_ptr)
    # (the flag bit stays on the device until somebody fetches the persistent flag: CapturedStep after a replay, the next eager
    #  caller of report_persistent, or check_edge_capacity)
    return {"edge_index": ei}, attrs
