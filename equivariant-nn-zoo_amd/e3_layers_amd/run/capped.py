"""What the clients of the capped neighbour list share (``run/md.ReplayedForceField``, ``run/loops.CappedLoop``,
``run/score_step.ReplayedScoreStep``; DESIGN.md section 4, "Capped neighbour list"): the names of the keys a rebuilt list touches,
the model's own ``edge_index`` layer read once, and the padded batch that carries the capped builder's device cells.

A periodic batch (one with ``cell``; ``data/compute_edge.py``) is served through ``run/md.ReplayedForceField`` only: the bucket then
also carries the cell's host-made inverse and the pbc mask -- and, for the all-images list, the image ranges (``_image_range``, a
zero row for the ghost graph) --, and ``edge_cell_shift`` is rebuilt beside ``edge_index``.  The sampler
and score-step loops with a cell are not served."""
from __future__ import annotations

from collections import namedtuple

import torch

from ..data.compute_edge import PairCriterion, _cell_operands, check_edge_capacity
from .graph_step import ghost_node_capacity, pad_batch

REBUILT_KEYS = ("edge_index", "_n_edges", "_edge_segment")      # the in-graph build rewrites all of them: never copied in
EDGE_KEYS = REBUILT_KEYS + ("edge_vector", "edge_length")       # what a rebuilt list invalidates
# a periodic batch (one with ``cell``) adds the image numbers to the rebuilt keys: never carried, absent on open batches (every pop
# of these tolerates that).  (``REBUILT_KEYS`` itself stays what the open clients copy around.)
PERIODIC_REBUILT_KEYS = ("edge_cell_shift",)

# the layer (data, attrs) -> (new, attrs) and what its keywords say: position key, cutoff, pair rule (None: not given to it)
EdgeLayer = namedtuple("EdgeLayer", "layer key r_max criterion")


def edge_layer_of(model):
    """The model's own ``edge_index`` layer as an ``EdgeLayer`` when its tree starts with one (a plain callable, e.g. the protein
    nets' ``partial(computeEdgeIndex, r_max=..., key="CA", criteria=...)``), else None."""
    name, layer = (getattr(model, "layers", None) or [(None, None)])[0]
    if name != "edge_index" or not callable(layer) or isinstance(layer, torch.nn.Module):
        return None
    kw = getattr(layer, "keywords", None) or {}
    return EdgeLayer(layer, kw.get("key"), kw.get("r_max"), kw.get("criteria"))


def replayable_criterion(own):
    """The ``EdgeLayer``'s criterion, a ``PairCriterion`` or None: a callback cannot be replayed and is refused."""
    if own.criterion is not None and not isinstance(own.criterion, PairCriterion):
        raise ValueError("edge_capacity: the model's edge_index layer uses a criteria callback (arbitrary Python, a host "
                         "synchronisation per call); build the tree with a data.PairCriterion to replay it")
    return own.criterion


def builder_cells(device) -> torch.Tensor:
    """Fresh ``_nlist_state`` (edges of the last build, builds that overflowed) or ``_nlist_rng`` (next draw index, draw in use)."""
    return torch.zeros(2, dtype=torch.int64, device=device)


def real_graphs(padded, drop=()):
    """The real graphs of a padded batch as a new batch, without the weight fields and the keys ``drop``."""
    out = padded[list(range(len(padded) - 1))]
    for k in ("_graph_weight", "_node_weight") + tuple(drop):
        out.pop(k)
    return out


class CappedBucket:
    """A padded batch (``pad_batch``) with the builder's cells in it: ``state`` always, ``rng`` when ``rng`` is True (fresh cells) or
    a cell tensor (the one a sizing build has already read)."""

    def __init__(self, padded, key: str = "pos", rng=False):
        self.padded, dev = padded, padded[key].device
        self.state = padded.data["_nlist_state"] = builder_cells(dev)
        self.rng = None if rng is False else builder_cells(dev) if rng is True else rng
        if self.rng is not None:
            padded.data["_nlist_rng"] = self.rng
        if "cell" in padded:      # periodic: the ghost graph's cell, inverse and pbc are zero (pad_batch; a zero cell has the zero inverse)
            padded.data["cell"] = padded.data["cell"].contiguous()
            _cell_operands(padded.data)      # ``_inv_cell`` / ``_pbc_mask``: on the host, once, before anything is captured
            if "edge_cell_shift" not in padded:
                raise ValueError("a periodic batch (one with 'cell') needs the 'edge_cell_shift' of its present list beside 'edge_index'")
            # (collation stores integers as int64; the builder rewrites int32 [e_cap, 3] in place)
            padded.data["edge_cell_shift"] = padded.data["edge_cell_shift"].to(torch.int32).reshape(-1, 3).contiguous()
            if "_image_range" in padded:      # the all-images list: the table beside ``_inv_cell`` / ``_pbc_mask``, the ghost graph's row zero
                padded.data["_image_range"] = padded.data["_image_range"].to(torch.int32).reshape(-1, 3).contiguous()
        self.n_graphs, self.n_cap, self.e_cap = len(padded) - 1, int(padded[key].shape[0]), int(padded["edge_index"].shape[1])

    @property
    def n_real(self) -> int:
        """The real nodes (on a device batch: one host read; construction issues none)."""
        return self.n_cap - int(self.padded["_n_nodes"].reshape(-1)[-1])

    @classmethod
    def around_list(cls, batch, e_cap: int, key: str = "pos", rng=False) -> "CappedBucket":
        """For an unpadded ``batch`` that carries its present list: ghost nodes for the tail as it is NOW, the positions contiguous
        (kernels read them through raw pointers)."""
        n, e = int(batch[key].shape[0]), int(batch["edge_index"].shape[1])
        padded = pad_batch(batch, ghost_node_capacity(n, e_cap - e), e_cap, key=key)
        padded[key] = padded[key].contiguous()
        return cls(padded, key, rng)

    def view(self):
        return self.padded.view()

    def check(self) -> None:
        """Synchronises; raises ``EdgeCapacityExceeded`` if a build overflowed since the last check."""
        check_edge_capacity(self.state)

    def real_graphs(self, drop=()):
        return real_graphs(self.padded, drop)
