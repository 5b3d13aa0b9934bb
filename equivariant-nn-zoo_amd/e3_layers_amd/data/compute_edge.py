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

``computeEdgeIndexCapped`` is the same radius graph for loops that call the model over and over while the atoms move (MD, relaxation,
the reverse-diffusion loop on cutoff graphs): it rewrites the FIXED ``[2, e_cap]`` ``edge_index`` of a batch padded by
``run/graph_step.pad_batch`` in place (``csrc/e3k_nlist.hip``), reads nothing back, and is therefore part of a captured HIP graph.
"""
from __future__ import annotations

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

    Not served (``computeEdgeIndex`` does both, eagerly): ``criteria`` callbacks, edges kept from before with carried attributes."""
    if criteria is not None:
        raise ValueError("computeEdgeIndexCapped takes no criteria callback (arbitrary Python over the candidate list): use computeEdgeIndex")
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
    lib = L.load()
    counts = torch.empty(total, dtype=torch.int32, device=dev)
    offsets = torch.empty(total + 1, dtype=torch.int64, device=dev)
    pos_d = pos.detach()
    L.check(lib.e3k_nlist_count(L.ptr(pos_d), L.ptr(node_seg), L.ptr(node_ptr), total, n_graphs, float(r_max), L.ptr(counts),
                                L.stream_ptr()), "e3k_nlist_count")
    L.check(lib.e3k_nlist_fill(L.ptr(pos_d), L.ptr(node_seg), L.ptr(node_ptr), total, n_graphs, float(r_max), L.ptr(counts), e_cap,
                               L.ptr(offsets), L.ptr(ei), L.ptr(n_edges), L.ptr(seg), L.ptr(state), L.ptr(flag), L.stream_ptr()),
            "e3k_nlist_fill")
    attrs["_n_edges"] = ("graph", "1x0e")
    for k in TOPO_KEYS + ("edge_vector", "edge_length"):
        data.pop(k, None)
    memo.forget(data)
    memo.remember(n_nodes, "nlist_ptr", node_ptr)
    # (the flag bit stays on the device until somebody fetches the persistent flag: CapturedStep after a replay, the next eager
    #  caller of report_persistent, or check_edge_capacity)
    return {"edge_index": ei}, attrs
