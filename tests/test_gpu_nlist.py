"""The capped neighbour list (csrc/e3k_nlist.hip, data/compute_edge.computeEdgeIndexCapped) on the device: bit for bit the padded
batch of the eagerly rebuilt edges, inside a captured graph on changing positions, and overflow as a reported condition."""
import pytest
import torch

from oracle import e3ref

pytestmark = pytest.mark.gpu


def _batch(seed, n_mol=5, single_atom=False):
    """synth_qm9 on the host, optionally with a one-atom graph in the middle."""
    from e3_layers_amd.data import Batch, Data
    from e3_layers_amd.data.loader import samples_of
    from e3_layers_amd.data.synthetic import synth_qm9

    batch = synth_qm9(seed, n_mol)
    if not single_atom:
        return batch
    samples = samples_of(batch)
    one = samples[0]
    lone = Data(attrs=dict(one.attrs), pos=one["pos"][:1].clone(), species=one["species"][:1].clone(),
                total_energy=one["total_energy"].clone(), edge_index=torch.zeros(2, 0, dtype=torch.long))
    samples.insert(2, lone)
    return Batch.from_data_list(samples, dict(one.attrs))


def _with_edges(batch, r_max):
    """The batch with computeEdgeIndex's edges at r_max (same device)."""
    from e3_layers_amd.data import computeEdgeIndex

    b = batch.clone()
    for k in ("edge_index", "_n_edges", "_edge_segment"):
        b.pop(k)
    new, attrs = computeEdgeIndex(b.data, b.attrs, r_max=r_max)
    b.attrs.update(attrs)
    b.update(new)
    return b


def _start(batch, n_cap, e_cap, dev):
    """A padded device batch of the bucket whose list is NOT the one asked for (the bonds shorter than 1.2 A)."""
    from e3_layers_amd.run.graph_step import pad_batch

    return pad_batch(_with_edges(batch, 1.2), n_cap, e_cap).to(dev)


def _check(got, want, host_batch, r_max):
    for k in ("edge_index", "_n_edges", "_edge_segment"):
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, k
        assert torch.equal(got[k], want[k]), k
    ref, _ = e3ref.compute_edge_index({"pos": host_batch["pos"].clone(), "_n_nodes": host_batch["_n_nodes"].clone()}, {}, r_max=r_max)
    e_real = ref["edge_index"].shape[1]
    assert torch.equal(got["edge_index"][:, :e_real].cpu(), ref["edge_index"])
    return e_real


@pytest.mark.parametrize("r_max", [2.5, 4.0, 5.0])
@pytest.mark.parametrize("seed,single_atom", [(0, False), (1, False), (2, True), (3, True)])
def test_capped_list_equals_the_padded_eager_rebuild(dev, seed, single_atom, r_max):
    from e3_layers_amd.backend.graph import check_indices
    from e3_layers_amd.data import computeEdgeIndexCapped
    from e3_layers_amd.data.compute_edge import check_edge_capacity
    from e3_layers_amd.run.graph_step import bucket_capacity, pad_batch

    check_indices()
    host = _batch(seed, single_atom=single_atom)
    eager = _with_edges(host.clone().to(dev), r_max)
    n, e = int(host["pos"].shape[0]), int(eager["edge_index"].shape[1])
    # a bucket as the force field picks it; no ghost edge at all with the two ghost nodes pad_batch insists on; ONE ghost edge
    for n_cap, e_cap in (bucket_capacity([(n, e)]), (n + 2, e), (n + 2, e + 1), (n + 3, e + 7)):
        want = pad_batch(eager, n_cap, e_cap)
        got = _start(host, n_cap, e_cap, dev)
        got["_nlist_state"] = torch.zeros(2, dtype=torch.int64, device=dev)
        new, attrs = computeEdgeIndexCapped(got.data, got.attrs, r_max=r_max)
        assert new["edge_index"].data_ptr() == got["edge_index"].data_ptr()      # in place
        assert attrs["_n_edges"] == ("graph", "1x0e")
        assert _check(got, want, host, r_max) == e
        check_edge_capacity(got["_nlist_state"])                                # fits: nothing is reported
        assert got["_nlist_state"].tolist() == [e, 0]


def test_capped_builder_replays_inside_a_captured_graph(dev):
    from e3_layers_amd.data import computeEdgeIndexCapped
    from e3_layers_amd.data.compute_edge import check_edge_capacity
    from e3_layers_amd.run.graph_step import CapturedStep, pad_batch

    r_max = 4.0
    host = _batch(4, n_mol=6, single_atom=True)
    scales = (1.0, 0.75, 1.4, 0.9)
    variants = []
    for s in scales:
        h = host.clone()
        h["pos"] = (host["pos"] * s).float()
        variants.append(h)
    eager = [_with_edges(h.clone().to(dev), r_max) for h in variants]
    counts = [int(b["edge_index"].shape[1]) for b in eager]
    assert len(set(counts)) >= 3, counts
    n, e_cap = int(host["pos"].shape[0]), max(counts) + 5
    n_cap = n + 4
    static = _start(host, n_cap, e_cap, dev)
    static["_nlist_state"] = torch.zeros(2, dtype=torch.int64, device=dev)

    def build():
        work = static.view()
        computeEdgeIndexCapped(work.data, work.attrs, r_max=r_max)
        return work["edge_index"]

    step = CapturedStep(build, warmup=2)
    for h, b, e in zip(variants, eager, counts):
        static["pos"][:n].copy_(h["pos"].to(dev))
        out = step()
        torch.cuda.synchronize()
        assert out.data_ptr() == static["edge_index"].data_ptr()
        assert _check(static, pad_batch(b, n_cap, e_cap), h, r_max) == e
        assert int(static["_nlist_state"][0]) == e
    check_edge_capacity(static["_nlist_state"])


def test_overflow_is_reported_and_stays_inside_the_buffers(dev):
    from e3_layers_amd.backend.graph import NLIST_OVERFLOW, EdgeCapacityExceeded, check_indices, persistent_flag
    from e3_layers_amd.data import computeEdgeIndexCapped
    from e3_layers_amd.data.compute_edge import check_edge_capacity
    from e3_layers_amd.run.graph_step import pad_batch

    check_indices()
    r_max, r_small = 5.0, 2.0
    host = _batch(6, n_mol=5, single_atom=True)
    eager = _with_edges(host.clone().to(dev), r_max)
    small = _with_edges(host.clone().to(dev), r_small)
    n, e, e_small = int(host["pos"].shape[0]), int(eager["edge_index"].shape[1]), int(small["edge_index"].shape[1])
    e_cap = (e + e_small) // 2
    assert e_small + 2 < e_cap < e
    n_cap = n + 5
    got = _start(host, n_cap, e_cap, dev)
    pad, canary = 256, -0x5A5A5A5A5A5A5A5
    buf_ei = torch.full((2 * e_cap + 2 * pad,), canary, dtype=torch.int64, device=dev)
    buf_seg = torch.full((e_cap + 2 * pad,), canary, dtype=torch.int64, device=dev)
    buf_ne = torch.full((len(got) + 2 * pad,), canary, dtype=torch.int64, device=dev)
    ei, seg, ne = buf_ei[pad:-pad].view(2, e_cap), buf_seg[pad:-pad], buf_ne[pad:-pad].view(-1, 1)
    ei.copy_(got["edge_index"]), seg.copy_(got["_edge_segment"]), ne.copy_(got["_n_edges"])
    got.data["edge_index"], got.data["_edge_segment"], got.data["_n_edges"] = ei, seg, ne
    state = got["_nlist_state"] = torch.zeros(2, dtype=torch.int64, device=dev)

    def canaries_intact():
        return all(bool((b[:pad] == canary).all()) and bool((b[-pad:] == canary).all()) for b in (buf_ei, buf_seg, buf_ne))

    computeEdgeIndexCapped(got.data, got.attrs, r_max=r_max)
    torch.cuda.synchronize()
    assert canaries_intact()
    assert int(ei.min()) >= 0 and int(ei.max()) < n                              # cut at e_cap: real edges only, all in range
    assert torch.equal(ei, eager["edge_index"][:, :e_cap])                       # ... and the FIRST e_cap edges of the full list
    assert int(seg.min()) >= 0 and int(seg.max()) < len(got)
    assert int(ne.sum()) == e_cap and int(ne.min()) >= 0 and int(ne[-1]) == 0
    assert state.tolist() == [e, 1]
    assert int(persistent_flag(dev)) & NLIST_OVERFLOW
    with pytest.raises(EdgeCapacityExceeded):
        check_edge_capacity(state)
    assert state.tolist() == [e, 0] and not int(persistent_flag(dev)) & NLIST_OVERFLOW
    check_edge_capacity(state)                                                   # reported once
    # the same buffers, a list that fits: clean, and exact again
    computeEdgeIndexCapped(got.data, got.attrs, r_max=r_small)
    torch.cuda.synchronize()
    assert canaries_intact()
    want = pad_batch(small, n_cap, e_cap)
    for k in ("edge_index", "_n_edges", "_edge_segment"):
        assert torch.equal(got[k], want[k]), k
    check_edge_capacity(state)
    assert state.tolist() == [e_small, 0]


def test_capped_builder_refuses_what_it_does_not_serve(dev):
    from e3_layers_amd.data import computeEdgeIndexCapped

    host = _batch(0, n_mol=2)
    n, e = int(host["pos"].shape[0]), int(host["edge_index"].shape[1])
    got = _start(host, n + 2, e, dev)
    with pytest.raises(ValueError, match="criteria"):
        computeEdgeIndexCapped(got.data, got.attrs, r_max=4.0, criteria=lambda d, c: None)
    plain = host.clone().to(dev)
    with pytest.raises(ValueError, match="pad_batch"):
        computeEdgeIndexCapped(plain.data, plain.attrs, r_max=4.0)
    got.attrs["bond"] = ("edge", "1x0e")
    got.data["bond"] = torch.zeros(e, 1, device=dev)
    with pytest.raises(ValueError, match="carried"):
        computeEdgeIndexCapped(got.data, got.attrs, r_max=4.0)
