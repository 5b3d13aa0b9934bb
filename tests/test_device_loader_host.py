"""Host side of device collation (``data/device_store.py``): the loader's id sequence and buckets, the ghost position table,
what the store refuses, the ctypes mirror of ``e3k_collate_field``.  No GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _Counts:
    """What DeviceLoader reads of a DeviceDataset: the host per-graph counts."""

    def __init__(self, n_nodes, n_edges):
        self.n_nodes, self.n_edges = np.asarray(n_nodes, dtype=np.int64), np.asarray(n_edges, dtype=np.int64)

    def __len__(self):
        return len(self.n_nodes)


def _counts(S, seed=0):
    rng = np.random.default_rng(seed)
    n = rng.integers(3, 30, S)
    return _Counts(n, n * rng.integers(4, 16, S))


@pytest.mark.parametrize("shuffle,seed,drop_last,epochs", [(True, 0, True, 1), (True, 7, True, 3), (False, 0, True, 2),
                                                           (True, 3, False, 2), (False, 1, False, 1)])
def test_id_sequence_equals_the_prefetch_loaders(shuffle, seed, drop_last, epochs):
    from e3_layers_amd.data.device_store import DeviceLoader
    from e3_layers_amd.data.loader import PrefetchLoader
    from e3_layers_amd.data.synthetic import synth_qm9

    store = synth_qm9(0, 50)
    ref = PrefetchLoader(store, 8, shuffle=shuffle, seed=seed, drop_last=drop_last, epochs=epochs)
    counts = _Counts(store["_n_nodes"].reshape(-1).numpy(), store["_n_edges"].reshape(-1).numpy())
    dl = DeviceLoader(counts, 8, shuffle=shuffle, seed=seed, drop_last=drop_last, epochs=epochs)
    want = list(ref.id_batches())
    got = [b.ids.tolist() for b in dl]
    assert got == want
    assert len(dl) == len(ref) == len(want)
    assert all(b.dtype == np.int32 for b in (x.ids for x in dl))


def test_endless_loader_keeps_the_sequence():
    from e3_layers_amd.data.device_store import DeviceLoader
    from e3_layers_amd.data.loader import id_batches

    counts = _counts(40)
    it = iter(DeviceLoader(counts, 16, seed=5, epochs=None))
    ref = id_batches(40, 16, True, 5, True, None)
    for _ in range(11):      # 2 batches per epoch: past five epochs
        assert next(it).ids.tolist() == next(ref)


def test_every_batch_fits_its_bucket_and_a_larger_batch_opens_another():
    from e3_layers_amd.data.device_store import DeviceLoader

    counts = _counts(300, seed=2)
    dl = DeviceLoader(counts, 32, seed=1, epochs=4)
    assert dl.n_buckets == 1
    for b in dl:
        n_cap, e_cap = dl.buckets[b.bucket]
        assert (n_cap, e_cap) == b.capacity
        assert b.n == int(counts.n_nodes[b.ids].sum()) and b.e == int(counts.n_edges[b.ids].sum())
        assert b.n + 2 <= n_cap and b.e <= e_cap
    pn, pe = dl.padding_fraction
    assert 0.0 < pn < 1.0 and 0.0 <= pe < 1.0
    n_cap, e_cap = dl.buckets[0]
    assert dl.bucket_of(n_cap - 2, e_cap) == 0                       # (exactly two ghost nodes, no ghost edge: fits)
    big = dl.bucket_of(n_cap - 1, e_cap + 1)                          # larger than anything in the first epoch
    assert big == 1 and dl.n_buckets == 2
    nc, ec = dl.buckets[1]
    assert n_cap - 1 + 2 <= nc and e_cap + 1 <= ec and ec >= e_cap
    assert dl.bucket_of(10, 10) == 0                                  # the smallest bucket that fits
    assert dl.bucket_of(n_cap - 1, e_cap + 1) == 1                    # ... and no third one for the same size


@pytest.mark.parametrize("n", [2, 3, 17, 64, 333])
def test_ghost_position_table_equals_ghost_sample(n):
    from e3_layers_amd.data.synthetic import synth_qm9
    from e3_layers_amd.run.graph_step import ghost_positions, ghost_sample

    like = synth_qm9(1, 2).get(0)
    table = ghost_positions(512, torch.float32)
    pos = ghost_sample(like, n, 3 * n)["pos"]
    assert pos.dtype == torch.float32
    assert torch.equal(table[:n], pos)


def test_store_with_preprocess_hooks_or_without_edges_is_refused():
    from e3_layers_amd.data.device_store import DeviceDataset
    from e3_layers_amd.data.loader import CondensedDataset
    from e3_layers_amd.data.synthetic import synth_qm9

    store = synth_qm9(0, 6)
    hooked = CondensedDataset(data=store.data, attrs=store.attrs, preprocess=[lambda s: s])
    with pytest.raises(ValueError, match="preprocess"):
        DeviceDataset(hooked, device="cuda:0")
    bare = store.clone()
    bare.data.pop("edge_index")
    with pytest.raises(ValueError, match="edge_index"):
        DeviceDataset(bare, device="cuda:0")
    with pytest.raises(TypeError):
        DeviceDataset([store.get(0)], device="cuda:0")


def test_loader_refuses_batches_the_kernel_cannot_take():
    from e3_layers_amd.data.device_store import DeviceLoader

    with pytest.raises(ValueError):
        DeviceLoader(_counts(2000), 1025)
    with pytest.raises(ValueError, match="cannot fill"):
        DeviceLoader(_counts(10), 16)


def test_collate_field_layout_matches_the_c_compiler(tmp_path):
    from e3_layers_amd.backend import lib as L

    src = tmp_path / "collate.c"
    src.write_text(
        '#include <stdio.h>\n#include <stddef.h>\n#include "e3k.h"\n'
        "int main(void){\n"
        'printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu\\n", sizeof(e3k_collate_field), offsetof(e3k_collate_field, ghost), '
        "offsetof(e3k_collate_field, row_bytes), offsetof(e3k_collate_field, src), offsetof(e3k_collate_field, dst), "
        "offsetof(e3k_collate_field, table), offsetof(e3k_collate_field, src_ld), offsetof(e3k_collate_field, dst_ld), "
        "(size_t)E3K_COLLATE_MAX_FIELDS);\n"
        'printf("%d %d %d %d %d %d %d %d %d\\n", E3K_COLLATE_NODE, E3K_COLLATE_EDGE, E3K_COLLATE_GRAPH, E3K_COLLATE_EDGE_INDEX, '
        "E3K_COLLATE_NODE_SEGMENT, E3K_COLLATE_EDGE_SEGMENT, E3K_COLLATE_NODE_WEIGHT, E3K_COLLATE_GHOST_FIRST, "
        "E3K_COLLATE_GHOST_TABLE);\n"
        "return 0;}\n")
    exe = tmp_path / "collate"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    F = L.CollateField
    assert out[:8] == [C.sizeof(F), F.ghost.offset, F.row_bytes.offset, F.src.offset, F.dst.offset, F.table.offset,
                       F.src_ld.offset, F.dst_ld.offset]
    assert out[8] == 16
    assert out[9:] == [0, 1, 2, 3, 4, 5, 6, 0, 1]      # (the kind / ghost codes data/device_store.py passes)
