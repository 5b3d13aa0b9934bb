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

Periodic cells (ASE's data contract): a batch with ``cell`` (per graph ``[G, 3, 3]`` fp32, rows = lattice vectors a, b, c; attrs
``("graph", "3x1o")``, stored flat as ``[G, 9]``) and optionally ``pbc`` (``[G, 3]`` integer or bool, ``("graph", "3x0e")``; absent:
periodic on every axis) gets the minimum-image list: ``computeEdgeIndex`` / ``computeEdgeIndexCapped`` return ``edge_index`` and
``edge_cell_shift`` (``[E, 3]`` int32, the image numbers of the destination, ``("edge", "3x0e")``), and ``computeEdgeVector`` forms
``pos[dst] - pos[src] + shift @ cell`` (``csrc/e3k_pbc.hip``; one statement of the arithmetic: ``csrc/e3k_pbc.h``, restated in torch
by ``_periodic_rule``).  The restriction that keeps one slot per ordered pair: every cell's perpendicular width along each periodic
axis exceeds ``2 r_max (1 + 1e-3)`` -- ``check_cell`` raises otherwise, once on the host where a cell enters.  Positions stay unwrapped
(the image is taken from differences; in fp32 that is sound up to about a thousand cell widths from the origin: the error of a
fractional component, about ``|d| / w 2^-22``, must stay below the 5e-4 the margin leaves to the rounding tie); ``wrap_positions``
is for output.  Virial and stress come from the force backward of these vectors (``nn.output.GradientOutput(virial=, stress=)``,
``csrc/e3k_virial.hip``), and a captured force field's cell changes through ``run/md.ReplayedForceField.set_cell``, driven by the host.
Narrower cells (crystal unit cells, several images per pair) are served on request: ``computeEdgeIndex(..., images="all")`` builds the
list of EVERY image of every ordered pair inside the cutoff, an atom's own images included (``src == dst``, shift != 0), in the order
source, destination, image offset (``csrc/e3k_images.h`` states the rule, its premise and the order; ``csrc/e3k_images.hip``;
restated in torch by ``_images_rule``).  ``image_ranges`` computes, on the host in float64, how many images per axis the walk has
to visit (``R_k = ceil(r_max (1 + 1e-3) / w_k + 1/2) - 1``, at most 7); the table stays in the batch as the per-graph field
``_image_range`` (it collates and pads like ``pbc``) and belongs to ONE ``r_max``.  A batch that carries it gets the all-images list
from ``computeEdgeIndex`` and ``computeEdgeIndexCapped`` without the keyword, so a model's own ``edge_index`` layer needs no change;
the capped path trusts the table, an eager call with ``images="all"`` always recomputes it.  On a cell that passes ``check_cell`` the
ranges are zero and the list is the minimum-image list, bit for bit.  Edge vectors, virial, stress and the CSR build work per edge and
take this list as it is.
NOT served: barostats on an all-images force field; training on stress; cell lists (the search stays O(n^2) per graph, O(n^2 M) with
M images per destination); ``criteria`` and pre-existing edges together with a cell; the sampler and score-step loops and
``DeviceDataset`` with a cell.  A batch without ``cell`` takes exactly the paths it took before, and so does a periodic batch that does
not ask for all images (``check_cell``'s refusal of narrow cells included).
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
    if "edge_cell_shift" in data:      # a periodic list: the builder's vectors, recomputed from the stored image numbers
        cell, _, _ = _cell_operands(data)
        vec, length = ops.edge_vector_periodic(pos, topo, _shift_operand(data["edge_cell_shift"], topo.num_edges), _node_segment(data, pos),
                                               cell)
    else:
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
computeEdgeVector.data_only_optional_inputs = ("edge_cell_shift", "cell")      # ... and these where the batch has them (a periodic batch)


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


# ---------------------------------------------------------------------------------------------------------------------
# Periodic cells: the minimum-image rule of csrc/e3k_pbc.h
# ---------------------------------------------------------------------------------------------------------------------
PBC_MARGIN = 1e-3      # every periodic perpendicular width must exceed 2 r_max (1 + PBC_MARGIN)


def _cell_pbc_host(cell, pbc):
    """float64 [G, 3, 3] and bool [G, 3] on the host (``pbc`` None: periodic on every axis)."""
    c = torch.as_tensor(cell).detach().to("cpu", torch.float64).reshape(-1, 3, 3)
    if pbc is None:
        p = torch.ones(c.shape[0], 3, dtype=torch.bool)
    else:
        p = torch.as_tensor(pbc).detach().to("cpu").reshape(-1, 3) != 0
        if p.shape[0] != c.shape[0]:
            raise ValueError(f"pbc names {p.shape[0]} graphs, cell {c.shape[0]}")
    return c, p


def _inverse_cells(c: Tensor) -> Tensor:
    """float64 inverses [G, 3, 3]; an all-zero cell (the ghost graph's, a graph without a periodic axis) has the zero inverse."""
    inv = torch.zeros_like(c)
    live = torch.linalg.det(c) != 0
    if bool(live.any()):
        inv[live] = torch.linalg.inv(c[live])
    return inv


def check_cell(cell, pbc, r_max: float) -> None:
    """Raises ``ValueError`` (naming graph, axis, width and the required minimum) unless the perpendicular width of every cell along
    each PERIODIC axis exceeds ``2 r_max (1 + 1e-3)``: the premise of the one-image-per-pair list.  Widths are computed in float64 on
    the host: along axis k it is ``1 / |column k of cell^-1|``.  Non-periodic axes are ignored (their lattice vector still has to
    make the cell invertible when another axis is periodic)."""
    c, p = _cell_pbc_host(cell, pbc)
    need = 2.0 * float(r_max) * (1.0 + PBC_MARGIN)
    for g in range(c.shape[0]):
        if not bool(p[g].any()):
            continue
        if float(torch.linalg.det(c[g])) == 0.0 or not bool(torch.isfinite(c[g]).all()):
            raise ValueError(f"graph {g}: the cell is singular (or not finite) but has a periodic axis")
        width = 1.0 / torch.linalg.inv(c[g]).norm(dim=0)
        for k in range(3):
            if bool(p[g, k]) and not float(width[k]) > need:
                raise ValueError(f"graph {g}, axis {'abc'[k]}: the cell's perpendicular width {float(width[k]):.6g} does not exceed "
                                 f"2 r_max (1 + {PBC_MARGIN:g}) = {need:.6g}; narrower cells are not served (replicate to a supercell)")


IMAGES_MAX_RANGE = 7      # E3K_IMAGES_MAX_RANGE of include/e3k.h: the kernel clamps to it, the host refuses beyond it
IMAGE_MODES = ("minimum", "all")


def image_ranges(cell, pbc, r_max: float) -> Tensor:
    """The image range of every graph and axis for the all-images list (``csrc/e3k_images.h``), int32 ``[G, 3]`` on the host:
    ``R_k = ceil(r_max (1 + 1e-3) / w_k + 0.5) - 1`` on a periodic axis of perpendicular width ``w_k`` (float64, as ``check_cell``
    computes it: ``1 / |column k of cell^-1|``), 0 on a non-periodic one.  Every image inside the cutoff then has its offset from the
    rounded image in ``[-R_k, R_k]``; a cell that passes ``check_cell`` has ``R = 0`` everywhere.  The table belongs to ONE ``r_max``.
    Raises ``ValueError`` (naming graph and axis) for a singular or non-finite cell that has a periodic axis and for a range above
    ``IMAGES_MAX_RANGE`` = 7 (15 images along the axis)."""
    c, p = _cell_pbc_host(cell, pbc)
    reach = float(r_max) * (1.0 + PBC_MARGIN)
    if not (math.isfinite(reach) and reach > 0.0):
        raise ValueError(f"image_ranges needs a finite r_max > 0 (got {r_max})")
    out = torch.zeros(c.shape[0], 3, dtype=torch.int32)
    for g in range(c.shape[0]):
        if not bool(p[g].any()):
            continue
        if not bool(torch.isfinite(c[g]).all()) or float(torch.linalg.det(c[g])) == 0.0:
            raise ValueError(f"graph {g}: the cell is singular (or not finite) but has a periodic axis")
        width = 1.0 / torch.linalg.inv(c[g]).norm(dim=0)
        for k in range(3):
            if not bool(p[g, k]):
                continue
            x = reach / float(width[k]) + 0.5
            r = math.ceil(x) - 1 if math.isfinite(x) else IMAGES_MAX_RANGE + 1
            if r > IMAGES_MAX_RANGE:
                raise ValueError(f"graph {g}, axis {'abc'[k]}: the cell's perpendicular width {float(width[k]):.6g} needs an image range "
                                 f"of {r if math.isfinite(x) else 'more than 7'} at r_max = {float(r_max):.6g}; ranges above "
                                 f"{IMAGES_MAX_RANGE} are not served (replicate the cell along this axis)")
            out[g, k] = max(r, 0)
    return out


def _check_candidates(n_nodes: Tensor, ranges: Tensor) -> None:
    """(nodes of a graph) x (images per destination) must stay below 2^31: the kernel counts a source's edges in an int32."""
    m = (2 * ranges.to("cpu", torch.int64) + 1).prod(1)
    n = n_nodes.reshape(-1).to("cpu", torch.int64)[:m.numel()]
    bad = torch.nonzero(n * m[:n.numel()] >= 1 << 31).reshape(-1)
    if bad.numel():
        g = int(bad[0])
        raise ValueError(f"graph {g}: {int(n[g])} nodes x {int(m[g])} images per destination is not below 2^31")


def _range_operand(data, n: int, dev) -> Tensor:
    """``_image_range`` of the batch as the kernels read it: int32 [n, 3], contiguous, on ``dev`` (kept in the batch in that form)."""
    r = data["_image_range"]
    if r.numel() != 3 * n:
        raise ValueError(f"_image_range names {r.numel() // 3} graphs, the batch has {n}")
    if r.dtype != torch.int32 or not r.is_contiguous() or r.device != dev or r.dim() != 2:
        if torch.cuda.is_available() and torch.cuda.is_current_stream_capturing():
            raise ValueError("_image_range must be a contiguous int32 [G, 3] tensor on the device before a capture starts")
        r = data["_image_range"] = r.to(dev, torch.int32).reshape(n, 3).contiguous()
    return r


def _cell_operands(data):
    """``(cell, inv_cell, pbc)`` of a batch with ``cell`` as the kernels read them: fp32 [G, 3, 3] (contiguous), its inverse formed on
    the host in float64 and rounded to fp32, int32 [G, 3]; the last two are kept in the batch (``_inv_cell``, ``_pbc_mask``: cells
    do not vary), so that only the first call -- outside a capture -- goes to the host."""
    cell = data["cell"]
    dev = cell.device
    if cell.dtype != torch.float32 or not cell.is_contiguous():
        raise ValueError("cell must be a contiguous fp32 tensor of [G, 3, 3] (stored flat: [G, 9])")
    n = cell.numel() // 9
    inv, mask = data.get("_inv_cell"), data.get("_pbc_mask")
    if inv is None or mask is None or inv.device != dev or inv.numel() != 9 * n or mask.numel() != 3 * n:
        c, p = _cell_pbc_host(cell, data.get("pbc"))
        inv = data["_inv_cell"] = _inverse_cells(c).to(torch.float32).reshape(n, 9).contiguous().to(dev)
        mask = data["_pbc_mask"] = p.to(torch.int32).contiguous().to(dev)
    return cell.reshape(n, 3, 3), inv.reshape(n, 3, 3), mask


def _shift_operand(shift: Tensor, n_edges: int) -> Tensor:
    if shift.dtype != torch.int32 or shift.numel() != 3 * n_edges:
        raise ValueError(f"edge_cell_shift must be an int32 tensor of [E, 3] (got {str(shift.dtype).replace('torch.', '')} "
                         f"{tuple(shift.shape)} for {n_edges} edges)")
    return shift.contiguous()


def _node_segment(data, pos: Tensor) -> Tensor:
    seg = data.get("_node_segment")
    if seg is None or seg.device != pos.device or seg.numel() != pos.shape[0]:
        seg = segment_ids(data["_n_nodes"].reshape(-1).to(pos.device), pos.shape[0])
    return seg.contiguous()


def _fma32(a: Tensor, b: Tensor, c: Tensor) -> Tensor:
    """fmaf on fp32 tensors: the product of two fp32 numbers is exact in float64."""
    return (a.double() * b.double() + c.double()).float()


def _periodic_rule(d: Tensor, cell: Tensor, inv: Tensor, pbc: Tensor):
    """The rule of ``csrc/e3k_pbc.h`` on fp32 displacements ``d`` [P, 3] with each pair's own ``cell``, ``inv`` [P, 3, 3] (fp32) and
    ``pbc`` [P, 3]: the image numbers (int32 [P, 3]), the vectors (fp32 [P, 3]) and their lengths (fp32 [P]), operation by operation."""
    s = _fma32(d[:, 2:3], inv[:, 2, :], _fma32(d[:, 1:2], inv[:, 1, :], d[:, 0:1] * inv[:, 0, :]))
    n = torch.where(pbc != 0, -torch.round(s), torch.zeros_like(s))
    v = _fma32(n[:, 2:3], cell[:, 2, :], _fma32(n[:, 1:2], cell[:, 1, :], _fma32(n[:, 0:1], cell[:, 0, :], d)))
    sq = v * v
    return n.to(torch.int32), v, torch.sqrt((sq[:, 0] + sq[:, 1]) + sq[:, 2])


def _images_rule(d: Tensor, cell: Tensor, inv: Tensor, pbc: Tensor, m: Tensor):
    """The rule of ``csrc/e3k_images.h`` on fp32 displacements ``d`` [P, 3] with each candidate's own ``cell``, ``inv`` [P, 3, 3]
    (fp32), ``pbc`` [P, 3] and image offset ``m`` [P, 3] (integers): the image numbers ``n = base + m`` (int32 [P, 3]; ``base`` the
    rounded image of ``_periodic_rule``), the vectors (fp32 [P, 3]) and their lengths (fp32 [P]), operation by operation."""
    s = _fma32(d[:, 2:3], inv[:, 2, :], _fma32(d[:, 1:2], inv[:, 1, :], d[:, 0:1] * inv[:, 0, :]))
    n = torch.where(pbc != 0, -torch.round(s), torch.zeros_like(s)) + m.to(torch.float32)
    v = _fma32(n[:, 2:3], cell[:, 2, :], _fma32(n[:, 1:2], cell[:, 1, :], _fma32(n[:, 0:1], cell[:, 0, :], d)))
    sq = v * v
    return n.to(torch.int32), v, torch.sqrt((sq[:, 0] + sq[:, 1]) + sq[:, 2])


def _image_candidates(n_nodes: Tensor, ranges: Tensor, device):
    """The candidates of the all-images walk in its order -- graph, source, destination (the source itself included), then the offset
    m with m_0 slowest and m_2 fastest, each from -R_k: (src [P], dst [P], m [P, 3], graph [P]) int64 on ``device``."""
    n = n_nodes.reshape(-1).tolist()
    src, dst, off, graph, start = [], [], [], [], 0
    for g, ng in enumerate(n):
        r = [int(x) for x in ranges[g].tolist()]
        m = torch.cartesian_prod(*(torch.arange(-x, x + 1) for x in r)).reshape(-1, 3)
        i, j, q = torch.meshgrid(torch.arange(ng), torch.arange(ng), torch.arange(m.shape[0]), indexing="ij")
        src.append(i.reshape(-1) + start)
        dst.append(j.reshape(-1) + start)
        off.append(m[q.reshape(-1)])
        graph.append(torch.full((i.numel(),), g, dtype=torch.int64))
        start += ng
    if not src:
        z = torch.zeros(0, dtype=torch.int64, device=device)
        return z, z, torch.zeros(0, 3, dtype=torch.int64, device=device), z
    return tuple(torch.cat(t).to(device) for t in (src, dst, off, graph))


def _images_graph_host(data, attrs, pos: Tensor, r_max: float, ranges: Tensor):
    """The torch restatement of the all-images list on whichever device holds the data: every candidate, the rule, strict ``<``."""
    cell, pbc = data["cell"], data.get("pbc")
    pos = pos.detach().to(torch.float32)
    n_nodes = data["_n_nodes"]
    c64, p = _cell_pbc_host(cell, pbc)
    if c64.shape[0] != n_nodes.numel():
        raise ValueError(f"cell names {c64.shape[0]} graphs, the batch has {n_nodes.numel()}")
    cell32 = torch.as_tensor(cell).detach().to(pos.device, torch.float32).reshape(-1, 3, 3)
    inv32 = _inverse_cells(c64).to(torch.float32).to(pos.device)
    p = p.to(pos.device)
    src, dst, m, g = _image_candidates(n_nodes.to("cpu"), ranges, pos.device)
    shift, _, length = _images_rule(pos[dst] - pos[src], cell32[g], inv32[g], p[g], m)
    keep = length < torch.tensor(float(r_max), dtype=torch.float32, device=pos.device)
    keep = torch.logical_and(keep, torch.logical_or(src != dst, (shift != 0).any(1)))
    attrs["_n_edges"] = ("graph", "1x0e")
    attrs["edge_cell_shift"] = ("edge", "3x0e")
    data["_n_edges"] = torch.bincount(g[keep], minlength=n_nodes.numel()).view(-1, 1)
    for k in _STALE:
        data.pop(k, None)
    return {"edge_index": torch.stack([src[keep], dst[keep]]), "edge_cell_shift": shift[keep].contiguous()}, attrs


def _images_graph(data, attrs, pos: Tensor, r_max: float):
    """``computeEdgeIndex(images="all")``: the ranges on the host (always recomputed: the table in the batch belongs to this
    ``r_max`` afterwards), kept in the batch as the per-graph field ``_image_range``, then the list of either path."""
    ranges = image_ranges(data["cell"], data.get("pbc"), r_max)
    _check_candidates(data["_n_nodes"], ranges)
    attrs["_image_range"] = ("graph", "3x0e")
    data["_image_range"] = ranges.to(pos.device)
    if pos.is_cuda:
        return _periodic_graph_device(data, attrs, pos, r_max, images=True)
    return _images_graph_host(data, attrs, pos, r_max, ranges)


def _refuse_with_cell(who: str, criteria, data=None) -> None:
    """What no builder serves together with a cell: a pair criterion, and (``data`` given: the eager builders) edges kept from before."""
    if criteria is not None:
        raise ValueError(f"{who}: a pair criterion together with a periodic cell is not served")
    if data is not None and "edge_index" in data:
        raise ValueError("computeEdgeIndex: pre-existing edges together with a periodic cell are not served (drop edge_index first)")


def _nlist_pair(stem: str, head, rule, counts: Tensor, fill=None, shift: Tensor = None, passes=("count", "fill")) -> None:
    """The count pass and the scan-and-fill pass of a capped builder through the C ABI.  ``stem``: the entry points' name with ``{}``
    for the pass; ``head``: what the three builders share (pos, node_seg, node_ptr, N, G, r_max); ``rule``: the operands of the pair
    rule, behind the head; ``fill``: (e_cap, offsets, edge_index, n_edges, edge_segment, state, flag) as tensors; ``shift``: the
    periodic builder's image numbers, behind ``edge_index``."""
    lib, stream = L.load(), L.stream_ptr()
    if "count" in passes:
        L.check(getattr(lib, stem.format("count"))(*head, *rule, L.ptr(counts), stream), stem.format("count"))
    if "fill" in passes:
        e_cap, offsets, edge_index, *rest = fill
        out = (L.ptr(edge_index),) + ((L.ptr(shift),) if shift is not None else ())
        L.check(getattr(lib, stem.format("fill"))(*head, *rule, L.ptr(counts), e_cap, L.ptr(offsets), *out, *(L.ptr(t) for t in rest),
                                                  stream), stem.format("fill"))


def _periodic_graph_host(data, attrs, pos: Tensor, r_max: float):
    """The torch restatement on whichever device holds the data: all ordered pairs of a graph, the rule, strict ``<``."""
    cell, pbc = data["cell"], data.get("pbc")
    check_cell(cell, pbc, r_max)
    pos = pos.detach().to(torch.float32)
    n_nodes = data["_n_nodes"]
    c64, p = _cell_pbc_host(cell, pbc)
    cell32 = torch.as_tensor(cell).detach().to(pos.device, torch.float32).reshape(-1, 3, 3)
    inv32 = _inverse_cells(c64).to(torch.float32).to(pos.device)
    p = p.to(pos.device)
    cand = _all_pairs(n_nodes, pos.device)
    cand = cand[:, cand[0] != cand[1]]
    g = segment_ids(n_nodes.reshape(-1).to(pos.device), pos.shape[0])[cand[0]]
    shift, _, length = _periodic_rule(pos[cand[1]] - pos[cand[0]], cell32[g], inv32[g], p[g])
    keep = length < torch.tensor(float(r_max), dtype=torch.float32)
    edge_index = cand[:, keep]
    attrs["_n_edges"] = ("graph", "1x0e")
    attrs["edge_cell_shift"] = ("edge", "3x0e")
    data["_n_edges"] = torch.bincount(g[keep], minlength=n_nodes.numel()).view(-1, 1)
    for k in _STALE:
        data.pop(k, None)
    return {"edge_index": edge_index, "edge_cell_shift": shift[keep].contiguous()}, attrs


def _periodic_graph_device(data, attrs, pos: Tensor, r_max: float, images: bool = False):
    """HIP path: the capped pair of ``csrc/e3k_pbc.hip`` -- ``images``: of ``csrc/e3k_images.hip``, with the batch's ``_image_range``
    -- at exactly the list's size, after one host read of the count."""
    if not images:
        check_cell(data["cell"], data.get("pbc"), r_max)
    dev = pos.device
    pos = L.f32c(pos.detach())
    n = data["_n_nodes"].reshape(-1).to(dev)
    total, n_graphs = pos.shape[0], n.numel()
    cell, inv, mask = _cell_operands(data)
    if cell.shape[0] != n_graphs:
        raise ValueError(f"cell names {cell.shape[0]} graphs, the batch has {n_graphs}")
    attrs["_n_edges"] = ("graph", "1x0e")
    attrs["edge_cell_shift"] = ("edge", "3x0e")
    for k in _STALE:
        data.pop(k, None)
    counts = torch.zeros(max(total, 1), dtype=torch.int32, device=dev)
    if total:
        # an empty ghost graph behind the real ones (the capped builder's layout): its cell, inverse and pbc are zero
        node_ptr = torch.full((n_graphs + 2,), total, dtype=torch.int64, device=dev)
        node_ptr[0] = 0
        node_ptr[1:n_graphs + 1] = torch.cumsum(n, 0)
        rule = (cell, inv, mask) + ((_range_operand(data, n_graphs, dev),) if images else ())
        padded = [torch.cat([t, torch.zeros_like(t[:1])]).contiguous() for t in rule]      # (alive until the fill below)
        geom = tuple(L.ptr(t) for t in padded)
        node_seg = _node_segment(data, pos)
        head = (L.ptr(pos), L.ptr(node_seg), L.ptr(node_ptr), total, n_graphs, float(r_max))
        stem = "e3k_images_{}" if images else "e3k_pbc_nlist_{}"
        _nlist_pair(stem, head, geom, counts, passes=("count",))
    n_edge = int(counts.sum().item())          # the one host sync: the size of the output
    edge_index = torch.empty(2, n_edge, dtype=torch.int64, device=dev)
    shift = torch.empty(n_edge, 3, dtype=torch.int32, device=dev)
    n_edges = torch.zeros(n_graphs + 1, dtype=torch.int64, device=dev)
    if n_edge:
        offsets = torch.empty(total + 1, dtype=torch.int64, device=dev)
        state = torch.zeros(2, dtype=torch.int64, device=dev)
        flag = torch.zeros(1, dtype=torch.int32, device=dev)      # (a list of exactly its own size cannot overflow)
        _nlist_pair(stem, head, geom, counts, (n_edge, offsets, edge_index, n_edges, None, state, flag), shift, passes=("fill",))
    data["_n_edges"] = n_edges[:n_graphs].view(-1, 1)
    return {"edge_index": edge_index, "edge_cell_shift": shift}, attrs


def wrap_positions(pos: Tensor, cell: Tensor, pbc, node_ptr: Tensor) -> Tensor:
    """``pos`` [N, 3] folded into each graph's cell along its periodic axes (fractional coordinates in [0, 1)), for output: the
    force field and the integrators work on unwrapped positions and never need this.  ``cell`` [G, 3, 3] (or [G, 9]), ``pbc`` [G, 3]
    or None (periodic everywhere), ``node_ptr`` [G + 1].  Computed in float64, returned in ``pos``'s dtype."""
    c = cell.detach().reshape(-1, 3, 3).double()
    counts = (node_ptr[1:] - node_ptr[:-1]).to(pos.device)
    g = segment_ids(counts, pos.shape[0])
    p = torch.ones(c.shape[0], 3, dtype=torch.bool, device=pos.device) if pbc is None else torch.as_tensor(pbc).to(pos.device).reshape(-1, 3) != 0
    inv = _inverse_cells(c.cpu()).to(pos.device)
    frac = torch.einsum("nc,nck->nk", pos.double(), inv[g])
    frac = torch.where(p[g], frac - torch.floor(frac), frac)
    return torch.einsum("nk,nkc->nc", frac, c.to(pos.device)[g]).to(pos.dtype)


def computeEdgeIndex(data, attrs, r_max: float = None, key: str = "pos", criteria=None, images: str = None):
    """``images`` (a batch with ``cell``): ``"minimum"`` -- one image per ordered pair, ``check_cell``'s width rule -- or ``"all"`` --
    every image inside the cutoff, an atom's own included, for cells of any width (``csrc/e3k_images.h``); the ranges are computed
    here, on the host, and stay in the batch as ``_image_range``.  Not given: ``"all"`` for a batch that already carries
    ``_image_range`` (the table is trusted: it belongs to the ``r_max`` it was made for), else ``"minimum"``."""
    if images is not None and images not in IMAGE_MODES:
        raise ValueError(f"computeEdgeIndex: images must be one of {IMAGE_MODES} (got {images!r})")
    if "_nlist_state" in data:      # a padded batch of a capped loop: the fixed-size list, rewritten in place inside the capture
        return computeEdgeIndexCapped(data, attrs, r_max=r_max, key=key, criteria=criteria)
    pos = torch.as_tensor(data[key], dtype=torch.get_default_dtype())
    if images == "all" and "cell" not in data:
        raise ValueError("computeEdgeIndex: images='all' needs a periodic batch (one with 'cell')")
    if "cell" in data:      # a periodic batch: the minimum-image list (or every image) and the image numbers
        _refuse_with_cell("computeEdgeIndex", criteria, data)
        if r_max is None:
            raise ValueError("computeEdgeIndex: a periodic cell needs r_max")
        if images == "all":
            return _images_graph(data, attrs, pos, r_max)
        if images is None and "_image_range" in data:
            n_graphs = data["_n_nodes"].numel()
            ranges = _range_operand(data, n_graphs, pos.device)
            if pos.is_cuda:
                return _periodic_graph_device(data, attrs, pos, r_max, images=True)
            return _images_graph_host(data, attrs, pos, r_max, ranges)
        return (_periodic_graph_device if pos.is_cuda else _periodic_graph_host)(data, attrs, pos, r_max)
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

    A batch with ``cell`` (the ghost graph's cell zero; ``_inv_cell`` / ``_pbc_mask`` already in it, as ``run/capped.CappedBucket``
    leaves them) takes the periodic builder (``csrc/e3k_pbc.hip``) and has its ``edge_cell_shift`` [e_cap, 3] int32 rewritten in place
    beside ``edge_index`` (zero on the ghost edges).  The width restriction is NOT checked here (``check_cell``: on the host, where the
    cell enters); a criterion together with a cell is refused.  A batch that also carries ``_image_range`` (int32 [G + 1, 3], the
    ghost graph's row zero; ``computeEdgeIndex(images="all")`` and ``run/capped.CappedBucket`` leave it so) takes the all-images
    builder (``csrc/e3k_images.hip``) instead: every image of every pair inside the cutoff, for cells of any width.  The table is
    trusted -- it cannot go to the host here -- and belongs to the ``r_max`` it was made for.

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
    carried = [k for k, v in attrs.items() if v[0] == "edge" and k in data and k not in ("edge_vector", "edge_length", "edge_cell_shift")]
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
    node_seg = _node_segment(data, pos)
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
    periodic = "cell" in data
    if periodic:
        _refuse_with_cell("computeEdgeIndexCapped", criteria)
        cell, inv, mask = _cell_operands(data)      # (the inverse is in the batch from the bucket's construction on: no host work here)
        shift = data.get("edge_cell_shift")
        L.require_cuda(cell, inv, mask, shift)
        if cell.shape[0] != n_graphs + 1:
            raise ValueError(f"cell names {cell.shape[0]} graphs, the padded batch has {n_graphs + 1} (the ghost graph's cell is zero)")
        if shift is None or shift.dtype != torch.int32 or not shift.is_contiguous() or shift.numel() != 3 * e_cap:
            raise ValueError(f"edge_cell_shift must be a contiguous int32 tensor of {3 * e_cap} elements to be rewritten in place")
        ranges = None
        if "_image_range" in data:      # every image inside the cutoff: the table is trusted (made on the host for this r_max)
            ranges = data["_image_range"]
            L.require_cuda(ranges)
            if ranges.dtype != torch.int32 or not ranges.is_contiguous() or ranges.numel() != 3 * (n_graphs + 1):
                raise ValueError(f"_image_range must be a contiguous int32 tensor of {3 * (n_graphs + 1)} elements (the ghost graph's "
                                 "row zero)")
    counts = torch.empty(total, dtype=torch.int32, device=dev)
    offsets = torch.empty(total + 1, dtype=torch.int64, device=dev)
    if periodic:
        stem, rule = "e3k_pbc_nlist_{}", (L.ptr(cell), L.ptr(inv), L.ptr(mask))
        if ranges is not None:
            stem, rule = "e3k_images_{}", rule + (L.ptr(ranges),)
        attrs["edge_cell_shift"] = ("edge", "3x0e")
    elif criteria is None:
        stem, rule = "e3k_nlist_{}", ()
    else:
        stem = "e3k_nlist_{}_crit"
        rule = (L.ptr(seg_key), criteria.window, criteria.threshold, int(criteria.keep_all), *L.seed_words(criteria.seed), L.ptr(rng))
    head = (L.ptr(pos.detach()), L.ptr(node_seg), L.ptr(node_ptr), total, n_graphs, float(r_max))
    _nlist_pair(stem, head, rule, counts, (e_cap, offsets, ei, n_edges, seg, state, flag), shift if periodic else None)
    attrs["_n_edges"] = ("graph", "1x0e")
    for k in TOPO_KEYS + ("edge_vector", "edge_length"):
        data.pop(k, None)
    memo.forget(data)
    memo.remember(n_nodes, "nlist_ptr", node_ptr)
    # (the flag bit stays on the device until somebody fetches the persistent flag: CapturedStep after a replay, the next eager
    #  caller of report_persistent, or check_edge_capacity)
    if periodic:
        return {"edge_index": ei, "edge_cell_shift": shift}, attrs
    return {"edge_index": ei}, attrs
