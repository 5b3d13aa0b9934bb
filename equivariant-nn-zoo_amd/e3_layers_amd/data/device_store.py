"""A dataset that lives in HBM, and batches padded to a size bucket on the device (``csrc/e3k_collate.hip``).

The reference trains from shuffled epochs over a condensed dataset (``e3_layers/run/trainer.py:358-399`` fed by
``e3_layers/data/dataloader.py:30-118``: worker processes collate ``Data`` objects).  The replayed step of this project
(``run/graph_step.PipelinedBucketedStep``) runs on batches padded to one (n_cap, e_cap) with a ghost graph; padding one on
the host (``pad_batch``: ``Batch.from_data_list`` over Python samples) takes longer than the step it would feed.  Here the
store is uploaded ONCE, and a batch is built on the device from its graph ids alone:

    ds = DeviceDataset(store, device=dev)                       # every per-node / per-edge / per-graph tensor, once
    loader = DeviceLoader(ds, batch_size=256, shuffle=True, seed=rank)
    step = CollatedStep(loader, prepare=model.prepare_data, fn=train_on, warmup=3)      # run/graph_step.py
    for _ in range(n_steps):
        loss = step()

Layout in HBM: every field as the batch will hold it (floats fp32, integers int64: what ``Batch.from_data_list`` casts to),
rows of graph s contiguous at the per-graph offsets ``node_off`` / ``edge_off`` (int64 [S + 1]); ``edge_index`` sample-local
int32 [2, E] (re-based with one add per edge while it is widened to int64).  QM9 (134 k molecules, 36 M directed edges at r_max
5) is about 0.3 GB of edges this way.

Several ranks: every rank holds the whole store and draws its own permutation (``seed=rank``), as ``bench.py`` does; the store
is not sharded.
"""
from __future__ import annotations

from typing import Iterator, List, Optional

import numpy as np
import torch

from .data import _INT_DTYPES, Batch
from .loader import id_batches

_COPIED = ("node", "edge", "graph")
_DERIVED = ("_n_nodes", "_n_edges", "_node_segment", "_edge_segment", "_graph_weight", "_node_weight")


class DeviceDataset:
    """``source``: a condensed host ``Batch`` / ``CondensedDataset`` (every sample in one Batch), uploaded to ``device`` once.

    Fields are what ``pad_batch(source.index_select(ids), ...)`` carries: the described (``attrs``) per-node, per-edge and
    per-graph tensors and ``edge_index``.  ``n_nodes`` / ``n_edges``: host numpy copies of the per-graph counts (the loader
    chooses buckets from them without touching the device)."""

    def __init__(self, source, device):
        if not isinstance(source, Batch):
            raise TypeError("DeviceDataset takes a condensed Batch / CondensedDataset (Batch.from_data_list of the samples)")
        if getattr(source, "preprocess", None):
            raise ValueError("DeviceDataset gathers batches from the condensed tensors; per-sample preprocess hooks need "
                             "DataLoader (worker processes)")
        if "edge_index" not in source.data or "_n_edges" not in source.data:
            raise ValueError("DeviceDataset needs edge_index and _n_edges (a store whose model builds its edges is not served)")
        if "pos" not in source.data:
            raise ValueError("DeviceDataset needs pos (the ghost graph of a padded batch is laid out from it)")
        from ..backend.graph import capture_flag

        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise ValueError("DeviceDataset lives on a HIP device")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        host = source if source["_n_nodes"].device.type == "cpu" else source.clone().to("cpu")
        self.n_nodes = host["_n_nodes"].reshape(-1).numpy().astype(np.int64)
        self.n_edges = host["_n_edges"].reshape(-1).numpy().astype(np.int64)
        self.n_graphs = S = int(self.n_nodes.shape[0])
        node_off = np.zeros(S + 1, dtype=np.int64)
        edge_off = np.zeros(S + 1, dtype=np.int64)
        node_off[1:] = np.cumsum(self.n_nodes)
        edge_off[1:] = np.cumsum(self.n_edges)
        if S >= 2 ** 31 - 1 or node_off[-1] >= 2 ** 31 - 1 or edge_off[-1] >= 2 ** 31 - 1:
            raise ValueError("graph, node and edge ids of the store must fit in int32")
        ei = host["edge_index"].numpy()
        if ei.shape != (2, int(edge_off[-1])):
            raise ValueError(f"edge_index {ei.shape} does not match the store's {int(edge_off[-1])} edges")
        local = ei - np.repeat(node_off[:-1], self.n_edges)[None, :]
        dev = self.device
        self.node_off = torch.from_numpy(node_off).to(dev)
        self.edge_off = torch.from_numpy(edge_off).to(dev)
        self.edge_index = torch.from_numpy(np.ascontiguousarray(local.astype(np.int32))).to(dev)

        rows = {"node": int(node_off[-1]), "edge": int(edge_off[-1]), "graph": S}
        self.keys: List[str] = []       # the store's fields in its order (edge_index among them), as pad_batch orders them
        self.fields = {}                # key -> (kind, device tensor)
        for key, value in host.data.items():
            if key == "edge_index":
                self.keys.append(key)
                continue
            if key in _DERIVED or key.startswith("_e3k_") or key not in host.attrs or host.attrs[key][0] not in _COPIED:
                continue                # (what Batch.get / samples_of leave out of a sample)
            if "index" in key or "face" in key:
                raise ValueError(f"{key}: fields concatenated along their last dimension are not collated on the device")
            kind = host.attrs[key][0]
            if value.dim() == 0 or value.shape[0] != rows[kind]:
                raise ValueError(f"{key}: {tuple(value.shape)} rows do not match the store's {rows[kind]} {kind}s")
            t = value.long() if value.dtype in _INT_DTYPES else value.float()
            self.fields[key] = (kind, t.contiguous().to(dev))
            self.keys.append(key)
        if self.fields["pos"][0] != "node" or tuple(self.fields["pos"][1].shape[1:]) != (3,):
            raise ValueError("pos must be per-node [N, 3]")
        self.attrs = {k: v for k, v in host.attrs.items() if k not in ("_node_segment", "_edge_segment")}
        for k in ("_n_nodes", "_n_edges", "_graph_weight"):
            self.attrs[k] = ("graph", "1x0e")
        self.attrs["_node_weight"] = ("node", "1x0e")
        self._tables = {}
        capture_flag(dev)               # (the persistent flag the plan kernel ORs into: allocated outside any capture)

    def __len__(self) -> int:
        return self.n_graphs

    def ghost_table(self, n_cap: int) -> torch.Tensor:
        """Ghost positions for up to ``n_cap`` ghost nodes (``ghost_positions``: the host's float64 arithmetic, rounded once), kept
        for the life of the store: captured graphs read it."""
        t = self._tables.get(n_cap)
        if t is None:
            from ..run.graph_step import ghost_positions

            t = self._tables[n_cap] = ghost_positions(n_cap, torch.float32).to(self.device)
        return t

    def empty_batch(self, G: int, n_cap: int, e_cap: int) -> Batch:
        """Uninitialised device tensors of a padded batch of ``G`` graphs (the ghost is graph ``G``), keys in ``pad_batch``'s order."""
        dev, i64, f32 = self.device, torch.int64, torch.float32
        cap = {"node": n_cap, "edge": e_cap, "graph": G + 1}
        out = {"_n_nodes": torch.empty(G + 1, 1, dtype=i64, device=dev), "_n_edges": torch.empty(G + 1, 1, dtype=i64, device=dev)}
        for key in self.keys:
            if key == "edge_index":
                out[key] = torch.empty(2, e_cap, dtype=i64, device=dev)
            else:
                kind, t = self.fields[key]
                out[key] = torch.empty((cap[kind],) + tuple(t.shape[1:]), dtype=t.dtype, device=dev)
        out["_node_segment"] = torch.empty(n_cap, dtype=i64, device=dev)
        out["_edge_segment"] = torch.empty(e_cap, dtype=i64, device=dev)
        out["_graph_weight"] = torch.empty(G + 1, 1, dtype=f32, device=dev)
        out["_node_weight"] = torch.empty(n_cap, 1, dtype=f32, device=dev)
        b = Batch.__new__(Batch)
        b.attrs, b.data, b.device = dict(self.attrs), out, dev
        return b

    def collation(self, G: int, n_cap: int, e_cap: int) -> "Collation":
        return Collation(self, G, n_cap, e_cap)

    def collate(self, ids, n_cap: int, e_cap: int) -> Batch:
        """Eager: the padded batch of the graphs ``ids`` (a fresh Batch on the device; ``ids`` on the host or the device)."""
        ids_t = torch.as_tensor(ids)
        if ids_t.dtype != torch.int32:
            host = np.asarray(ids_t.cpu(), dtype=np.int64).reshape(-1)
            if host.size and (host.min() < -2 ** 31 or host.max() >= 2 ** 31):
                raise IndexError("graph ids must fit in int32")
            ids_t = torch.from_numpy(host.astype(np.int32))
        c = Collation(self, int(ids_t.numel()), n_cap, e_cap)
        c.ids.copy_(ids_t.reshape(-1))
        c()
        return c.batch


class Collation:
    """The static buffers of one padded-batch shape: ``ids`` int32 [G] (the only input), ``batch`` (the outputs) and the plan's
    workspace; ``collation()`` enqueues the two launches on the current stream -- capture-safe (fixed shapes, no read-back, no
    memset).  An id outside the store or a batch that does not fit reaches the persistent flag (``backend/graph.py``)."""

    def __init__(self, ds: DeviceDataset, G: int, n_cap: int, e_cap: int):
        from ..backend import lib as L

        if not 1 <= G <= 1024:
            raise ValueError(f"{G} graphs per batch: device collation takes 1 to 1024")
        if n_cap < 2 or e_cap < 0 or n_cap >= 2 ** 31 - 1 or e_cap >= 2 ** 31 - 1:
            raise ValueError(f"bad capacities ({n_cap}, {e_cap})")
        self.ds, self.G, self.n_cap, self.e_cap = ds, int(G), int(n_cap), int(e_cap)
        dev = ds.device
        self.ids = torch.zeros(self.G, dtype=torch.int32, device=dev)
        self.work = torch.zeros(int(L.load().e3k_collate_work_ints(self.G)), dtype=torch.int64, device=dev)
        self.table = ds.ghost_table(self.n_cap)
        self.batch = ds.empty_batch(self.G, self.n_cap, self.e_cap)
        self._describe()

    def renew(self) -> None:
        """New output tensors in the same Batch container (``CollatedStep`` records a buffer again on tensors that carry no memo, ``backend/memo.py``)."""
        fresh = self.ds.empty_batch(self.G, self.n_cap, self.e_cap)
        self.batch.data.clear()
        self.batch.data.update(fresh.data)
        self._describe()

    def _describe(self) -> None:
        from ..backend import lib as L

        ds, out = self.ds, self.batch.data
        K = {k[len("E3K_COLLATE_"):]: v for k, v in L.DEFINES.items() if k.startswith("E3K_COLLATE_")}      # include/e3k.h
        fields = []
        for key in ds.keys:
            if out[key].numel() == 0:
                continue                # (no edges in the bucket: nothing to write)
            if key == "edge_index":
                fields.append(L.CollateField(kind=K["EDGE_INDEX"], src=L.ptr(ds.edge_index), dst=L.ptr(out[key]),
                                             src_ld=ds.edge_index.shape[1], dst_ld=self.e_cap))
                continue
            kind, t = ds.fields[key]
            row_bytes = t.element_size() * int(np.prod(t.shape[1:], dtype=np.int64))
            table = key == "pos"
            fields.append(L.CollateField(kind=K[kind.upper()], ghost=K["GHOST_TABLE"] if table else K["GHOST_FIRST"], row_bytes=row_bytes,
                                         src=L.ptr(t), dst=L.ptr(out[key]), table=L.ptr(self.table) if table else None))
        fields.append(L.CollateField(kind=K["NODE_SEGMENT"], dst=L.ptr(out["_node_segment"])))
        if self.e_cap:
            fields.append(L.CollateField(kind=K["EDGE_SEGMENT"], dst=L.ptr(out["_edge_segment"])))
        fields.append(L.CollateField(kind=K["NODE_WEIGHT"], dst=L.ptr(out["_node_weight"])))
        if len(fields) > K["MAX_FIELDS"]:
            raise ValueError(f"{len(fields)} collated fields: the kernel takes {K['MAX_FIELDS']} (E3K_COLLATE_MAX_FIELDS)")
        self._fields = (L.CollateField * len(fields))(*fields)

    def __call__(self) -> None:
        from ..backend import lib as L
        from ..backend.graph import capture_flag, report_persistent

        ds, out, lib = self.ds, self.batch.data, L.load()
        dev = ds.device
        with torch.cuda.device(dev):
            st = L.stream_ptr()
            L.check(lib.e3k_collate_plan(L.ptr(self.ids), self.G, L.ptr(ds.node_off), L.ptr(ds.edge_off), ds.n_graphs, self.n_cap,
                                         self.e_cap, L.ptr(self.work), L.ptr(out["_n_nodes"]), L.ptr(out["_n_edges"]),
                                         L.ptr(out["_graph_weight"]), L.ptr(capture_flag(dev)), st), "e3k_collate_plan")
            L.check(lib.e3k_collate_gather(self._fields, len(self._fields), self.G, self.n_cap, self.e_cap, L.ptr(self.work), st),
                    "e3k_collate_gather")
            report_persistent(dev)      # (eager: the flag travels home behind the launches; captured: CapturedStep polls it)


class CollatedBatch:
    """What ``DeviceLoader`` yields: the graph ids of one batch (int32, host), its real sizes and its bucket."""
    __slots__ = ("ids", "n", "e", "bucket", "capacity")

    def __init__(self, ids, n, e, bucket, capacity):
        self.ids, self.n, self.e, self.bucket, self.capacity = ids, n, e, bucket, capacity

    @property
    def G(self) -> int:
        return int(self.ids.shape[0])

    @property
    def key(self):
        return (self.G,) + tuple(self.capacity)


class DeviceLoader:
    """The graph ids of every batch of a ``DeviceDataset`` and the size bucket each one is padded to.

    The ids are exactly ``PrefetchLoader.id_batches``' for the same arguments (``loader.id_batches``: one ``torch.Generator``
    seeded with ``seed``, a fresh permutation per epoch, ``drop_last``).  Buckets: ``bucket_capacity`` over every batch of the
    first epoch -- its permutation is known in advance, so the policy costs nothing at run time.  A later batch that does not
    fit opens a new bucket that covers it (with 2 % headroom) and the first epoch (``CollatedStep`` records it when it is first
    used); a batch goes to the smallest bucket it fits.  ``epochs=None``: endless."""

    def __init__(self, ds: DeviceDataset, batch_size: int, shuffle: bool = True, seed: int = 0, drop_last: bool = True,
                 epochs: Optional[int] = None):
        from ..run.graph_step import bucket_capacity

        self.ds, self.batch_size = ds, int(batch_size)
        self.shuffle, self.seed, self.drop_last, self.epochs = bool(shuffle), int(seed), bool(drop_last), epochs
        if not 1 <= self.batch_size <= 1024:
            raise ValueError(f"batch_size {batch_size}: device collation takes 1 to 1024 graphs")
        first = list(id_batches(len(ds), self.batch_size, self.shuffle, self.seed, self.drop_last, 1))
        if not first:
            raise ValueError(f"{len(ds)} graphs cannot fill a batch of {self.batch_size}")
        self._first_sizes = [self.sizes(ids) for ids in first]
        self.buckets = [bucket_capacity(self._first_sizes)]
        self._real = np.zeros(2, dtype=np.int64)      # real / padded nodes and edges of the batches drawn so far
        self._cap = np.zeros(2, dtype=np.int64)

    def sizes(self, ids):
        ids = np.asarray(ids, dtype=np.int64)
        return int(self.ds.n_nodes[ids].sum()), int(self.ds.n_edges[ids].sum())

    def __len__(self) -> int:
        n = len(self.ds)
        per = n // self.batch_size if self.drop_last else -(-n // self.batch_size)
        return per if self.epochs is None else per * self.epochs

    def id_batches(self) -> Iterator[List[int]]:
        return id_batches(len(self.ds), self.batch_size, self.shuffle, self.seed, self.drop_last, self.epochs)

    def bucket_of(self, n: int, e: int) -> int:
        from ..run.graph_step import bucket_capacity

        fits = [i for i, (nc, ec) in enumerate(self.buckets) if n + 2 <= nc and e <= ec]
        if fits:
            return min(fits, key=lambda i: (self.buckets[i][1], self.buckets[i][0]))
        # (2 % headroom over the batch that opens it: without it, a few epochs of 256 molecules opened a bucket per new maximum)
        self.buckets.append(bucket_capacity(self._first_sizes + [(int(n * 1.02) + 1, int(e * 1.02) + 1)]))
        return len(self.buckets) - 1

    @property
    def n_buckets(self) -> int:
        return len(self.buckets)

    @property
    def padding_fraction(self):
        """(nodes, edges): the share of padded rows that are ghost rows, over the batches drawn so far (before the first: over the
        first epoch)."""
        if self._cap[0] == 0:
            n_cap, e_cap = self.buckets[0]
            real = np.array(self._first_sizes, dtype=np.float64).sum(0)
            return 1.0 - real[0] / (n_cap * len(self._first_sizes)), 1.0 - real[1] / max(e_cap * len(self._first_sizes), 1)
        return 1.0 - self._real[0] / self._cap[0], 1.0 - self._real[1] / max(int(self._cap[1]), 1)

    def __iter__(self) -> Iterator[CollatedBatch]:
        for ids in self.id_batches():
            n, e = self.sizes(ids)
            b = self.bucket_of(n, e)
            cap = self.buckets[b]
            self._real += (n, e)
            self._cap += cap
            yield CollatedBatch(np.asarray(ids, dtype=np.int32), n, e, b, cap)
