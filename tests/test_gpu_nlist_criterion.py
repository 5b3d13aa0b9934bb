"""The capped neighbour list with a declarative pair criterion (csrc/e3k_nlist.hip: e3k_nlist_count_crit / _fill_crit;
data/compute_edge.SequenceOrRandom) on the device: bit for bit the padded batch of the eager rebuild with the same criterion at the
same draw index, inside a captured graph on changing positions, overflow as a reported condition, refusals, and the dispatch
from computeEdgeIndex on a batch that carries ``_nlist_state``."""
import pytest
import torch

pytestmark = pytest.mark.gpu

SIZES = (70, 1, 130)      # two and three ballot rounds of 64 lanes, a lone node
N = sum(SIZES)
TINY, R_CUT = 1e-6, 0.7   # no pair inside the cutoff / about ten neighbours per node (unit Gaussian clouds)
KEYS = ("edge_index", "_n_edges", "_edge_segment")


def _host(seed=0, scale=1.0):
    """70 + 1 + 130 nodes under ``CA``.  Chains: graph 0 = 64 + 6 nodes (a chain boundary between the nodes 63 and 64: the first
    ballot round's last lane and the second round's first), graph 1 = the lone node, graph 2 = 64 + 36 + 30.  The chain ids on both
    sides of either graph boundary are EQUAL (1 | 1 | 1): neighbours in index that the rule must not pair."""
    from e3_layers_amd.data import Batch

    gen = torch.Generator().manual_seed(seed)
    attrs = {"CA": ("node", "1x1o"), "chain_id": ("node", "1x0e"), "id": ("node", "1x0e")}
    chains = ([0] * 64 + [1] * 6, [1], [1] * 64 + [2] * 36 + [0] * 30)
    lst = []
    for n, chain in zip(SIZES, chains):
        lst.append({"CA": (scale * torch.randn(n, 3, generator=gen)).float(), "chain_id": torch.tensor(chain).view(-1, 1),
                    "id": torch.arange(n).view(-1, 1), "_n_nodes": torch.tensor([[n]])})
    b = Batch.from_data_list(lst, attrs)
    b.attrs.pop("_n_edges", None)
    return b


def _eager(batch, r_max, crit, draw):
    """The batch (any device) with computeEdgeIndex's edges under ``crit`` at draw index ``draw``."""
    from e3_layers_amd.data import computeEdgeIndex

    b = batch.clone()
    for k in KEYS:
        b.pop(k)
    crit.reset(draw)
    new, attrs = computeEdgeIndex(b.data, b.attrs, r_max=r_max, key="CA", criteria=crit)
    b.attrs.update(attrs)
    b.update(new)
    return b


def _start(host, n_cap, e_cap, dev, draw=0):
    """A padded device batch of the bucket whose list is NOT the one asked for (a sparse random one), with the builder's cells."""
    from e3_layers_amd.data import SequenceOrRandom
    from e3_layers_amd.run.graph_step import pad_batch

    got = pad_batch(_eager(host, TINY, SequenceOrRandom(None, 0, 0.004, seed=99), 0), n_cap, e_cap, key="CA").to(dev)
    got["_nlist_state"] = torch.zeros(2, dtype=torch.int64, device=dev)
    got.data["_nlist_rng"] = torch.tensor([draw, -1], dtype=torch.int64, device=dev)
    return got


def _same(got, want):
    for k in KEYS:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, k
        assert torch.equal(got[k], want[k]), k


@pytest.mark.parametrize("window,p", [(5, 0.0), (0, 0.02), (5, 0.02), (0, 1.0)])
@pytest.mark.parametrize("r_max", [TINY, R_CUT])
def test_capped_list_with_a_criterion_equals_the_padded_eager_rebuild(dev, r_max, window, p):
    from e3_layers_amd.backend.graph import check_indices
    from e3_layers_amd.data import SequenceOrRandom, computeEdgeIndexCapped
    from e3_layers_amd.data.compute_edge import check_edge_capacity
    from e3_layers_amd.run.graph_step import bucket_capacity, pad_batch

    check_indices()
    host = _host()
    crit = SequenceOrRandom("chain_id", window, p, seed=(3 << 32) + 17)
    draw = 5
    eager = _eager(host.clone().to(dev), r_max, crit, draw)
    e = int(eager["edge_index"].shape[1])
    ei = eager["edge_index"].cpu()
    chain = host["chain_id"].view(-1)
    near = (chain[ei[0]] == chain[ei[1]]) & ((ei[0] - ei[1]).abs() < window)
    if p == 1.0:
        assert e == sum(n * (n - 1) for n in SIZES)
    elif r_max == TINY and p == 0.0:
        # ordered pairs 1 <= |i - j| <= 4 inside each chain (lengths 64, 6 | 1 | 64, 36, 30)
        assert bool(near.all()) and e == sum(2 * sum(max(length - d, 0) for d in range(1, 5)) for length in (64, 6, 1, 64, 36, 30))
        assert not bool(((ei[0] == 63) & (ei[1] == 64)).any()) and bool(((ei[0] == 62) & (ei[1] == 63)).any())      # chain boundary
        assert not bool(((ei[0] == 69) & (ei[1] == 70)).any()) and not bool(((ei[0] == 70) | (ei[1] == 70)).any())  # graph boundary
    elif r_max == TINY:
        assert 300 < int((~near).sum()) < 600      # about 2 % of the 21 600 ordered pairs
    for n_cap, e_cap in (bucket_capacity([(N, e)]), (N + 2, e), (N + 2, e + 1), (N + 3, e + 7)):
        want = pad_batch(eager, n_cap, e_cap, key="CA")
        got = _start(host, n_cap, e_cap, dev, draw)
        new, attrs = computeEdgeIndexCapped(got.data, got.attrs, r_max=r_max, key="CA", criteria=crit)
        assert new["edge_index"].data_ptr() == got["edge_index"].data_ptr()      # in place
        assert attrs["_n_edges"] == ("graph", "1x0e")
        _same(got, want)
        check_edge_capacity(got["_nlist_state"])                                # fits: nothing is reported
        assert got["_nlist_state"].tolist() == [e, 0]
        assert got["_nlist_rng"].tolist() == [draw + 1, draw]                   # one build, one draw


def test_criterion_builder_replays_inside_a_captured_graph(dev):
    from e3_layers_amd.data import SequenceOrRandom, computeEdgeIndexCapped
    from e3_layers_amd.data.compute_edge import check_edge_capacity
    from e3_layers_amd.run.graph_step import CapturedStep, pad_batch

    crit = SequenceOrRandom("chain_id", 5, 0.02, seed=8)
    host = _host(1)
    variants = []
    for s in (1.0, 0.8, 1.3, 0.9):
        h = host.clone()
        h["CA"] = (host["CA"] * s).float()
        variants.append(h)
    eager = [_eager(h.clone().to(dev), R_CUT, crit, k) for k, h in enumerate(variants)]
    counts = [int(b["edge_index"].shape[1]) for b in eager]
    assert len(set(counts)) >= 3, counts
    again = _eager(variants[0].clone().to(dev), R_CUT, crit, 1)
    assert not torch.equal(again["edge_index"], eager[0]["edge_index"])          # another draw on the same positions: another list
    n_cap, e_cap = N + 4, max(counts) + 5
    static = _start(host, n_cap, e_cap, dev)
    rng = static["_nlist_rng"]

    def build():
        work = static.view()
        computeEdgeIndexCapped(work.data, work.attrs, r_max=R_CUT, key="CA", criteria=crit)
        return work["edge_index"]

    step = CapturedStep(build, warmup=2)
    rng.zero_()                                                                  # (the warm-up builds drew)
    kept = []
    for h in variants:                                                           # four replays, nothing read back in between
        static["CA"][:N].copy_(h["CA"].to(dev, non_blocking=True))
        out = step()
        assert out.data_ptr() == static["edge_index"].data_ptr()
        kept.append({k: static[k].clone() for k in KEYS + ("_nlist_state",)})
    torch.cuda.synchronize()
    for k, (b, e) in enumerate(zip(eager, counts)):
        _same(kept[k], pad_batch(b, n_cap, e_cap, key="CA"))                     # replay k == the eager build at draw index k
        assert int(kept[k]["_nlist_state"][0]) == e
    assert rng.tolist() == [4, 3]
    check_edge_capacity(static["_nlist_state"])


def test_overflow_with_a_criterion_is_reported_and_stays_inside_the_buffers(dev):
    from e3_layers_amd.backend.graph import NLIST_OVERFLOW, EdgeCapacityExceeded, check_indices, persistent_flag
    from e3_layers_amd.data import SequenceOrRandom, computeEdgeIndexCapped
    from e3_layers_amd.data.compute_edge import check_edge_capacity
    from e3_layers_amd.run.graph_step import pad_batch

    check_indices()
    crit, sparse = SequenceOrRandom("chain_id", 5, 0.02, seed=4), SequenceOrRandom("chain_id", 2, 0.0)
    host = _host(2)
    eager = _eager(host.clone().to(dev), R_CUT, crit, 0)
    small = _eager(host.clone().to(dev), TINY, sparse, 0)
    e, e_small = int(eager["edge_index"].shape[1]), int(small["edge_index"].shape[1])
    e_cap = (e + e_small) // 2
    assert e_small + 2 < e_cap < e
    n_cap = N + 5
    got = _start(host, n_cap, e_cap, dev)
    pad, canary = 256, -0x5A5A5A5A5A5A5A5
    buf_ei = torch.full((2 * e_cap + 2 * pad,), canary, dtype=torch.int64, device=dev)
    buf_seg = torch.full((e_cap + 2 * pad,), canary, dtype=torch.int64, device=dev)
    buf_ne = torch.full((len(got) + 2 * pad,), canary, dtype=torch.int64, device=dev)
    ei, seg, ne = buf_ei[pad:-pad].view(2, e_cap), buf_seg[pad:-pad], buf_ne[pad:-pad].view(-1, 1)
    ei.copy_(got["edge_index"]), seg.copy_(got["_edge_segment"]), ne.copy_(got["_n_edges"])
    got.data["edge_index"], got.data["_edge_segment"], got.data["_n_edges"] = ei, seg, ne
    state = got["_nlist_state"]

    def canaries_intact():
        return all(bool((b[:pad] == canary).all()) and bool((b[-pad:] == canary).all()) for b in (buf_ei, buf_seg, buf_ne))

    computeEdgeIndexCapped(got.data, got.attrs, r_max=R_CUT, key="CA", criteria=crit)
    torch.cuda.synchronize()
    assert canaries_intact()
    assert int(ei.min()) >= 0 and int(ei.max()) < N
    assert torch.equal(ei, eager["edge_index"][:, :e_cap])                       # the FIRST e_cap edges of the full list
    assert int(seg.min()) >= 0 and int(seg.max()) < len(got)
    assert int(ne.sum()) == e_cap and int(ne.min()) >= 0 and int(ne[-1]) == 0
    assert state.tolist() == [e, 1]
    assert int(persistent_flag(dev)) & NLIST_OVERFLOW
    with pytest.raises(EdgeCapacityExceeded):
        check_edge_capacity(state)
    assert state.tolist() == [e, 0] and not int(persistent_flag(dev)) & NLIST_OVERFLOW
    check_edge_capacity(state)                                                   # reported once
    computeEdgeIndexCapped(got.data, got.attrs, r_max=TINY, key="CA", criteria=sparse)      # the same buffers, a list that fits
    torch.cuda.synchronize()
    assert canaries_intact()
    _same(got, pad_batch(small, n_cap, e_cap, key="CA"))
    check_edge_capacity(state)
    assert state.tolist() == [e_small, 0]


def test_refusals(dev):
    from e3_layers_amd.data import SequenceOrRandom, computeEdgeIndexCapped

    host = _host()
    crit = SequenceOrRandom("chain_id", 5, 0.02)
    got = _start(host, N + 2, 4096, dev)
    with pytest.raises(ValueError, match="criteria"):
        computeEdgeIndexCapped(got.data, got.attrs, r_max=R_CUT, key="CA", criteria=lambda d, c: None)
    before = got["edge_index"].clone()
    for bad in (got["chain_id"].float(), got["chain_id"].to(torch.int32), got["chain_id"].expand(-1, 2).contiguous(),
                got["chain_id"][:-1].contiguous()):
        work = got.view()
        work.data["chain_id"] = bad
        with pytest.raises(ValueError, match="segment"):
            computeEdgeIndexCapped(work.data, work.attrs, r_max=R_CUT, key="CA", criteria=crit)
    work = got.view()
    work.data.pop("chain_id")
    with pytest.raises(ValueError, match="segment"):
        computeEdgeIndexCapped(work.data, work.attrs, r_max=R_CUT, key="CA", criteria=crit)
    work = got.view()
    work.data["_nlist_rng"] = torch.zeros(3, dtype=torch.int64, device=dev)
    with pytest.raises(ValueError, match="_nlist_rng"):
        computeEdgeIndexCapped(work.data, work.attrs, r_max=R_CUT, key="CA", criteria=crit)
    assert torch.equal(got["edge_index"], before) and got["_nlist_rng"].tolist() == [0, -1]      # refused before any launch
    flat = got.view()                                                            # [N] instead of [N, 1] is served
    flat.data["chain_id"] = got["chain_id"].reshape(-1).clone()
    computeEdgeIndexCapped(flat.data, flat.attrs, r_max=R_CUT, key="CA", criteria=crit)
    assert got["_nlist_rng"].tolist() == [1, 0]


def test_compute_edge_index_dispatches_on_the_marker(dev):
    from e3_layers_amd.data import SequenceOrRandom, computeEdgeIndex
    from e3_layers_amd.run.graph_step import pad_batch

    host = _host(3)
    crit = SequenceOrRandom("chain_id", 5, 0.02, seed=6)
    eager = _eager(host.clone().to(dev), R_CUT, crit, 2)
    e = int(eager["edge_index"].shape[1])
    n_cap, e_cap = N + 6, e + 40
    got = _start(host, n_cap, e_cap, dev, draw=2)
    crit.reset(11)                                                               # (the host counter is not what a padded batch draws with)
    new, attrs = computeEdgeIndex(got.data, got.attrs, r_max=R_CUT, key="CA", criteria=crit)
    assert new["edge_index"].data_ptr() == got["edge_index"].data_ptr() and new["edge_index"].shape == (2, e_cap)
    _same(got, pad_batch(eager, n_cap, e_cap, key="CA"))
    assert got["_nlist_state"].tolist() == [e, 0] and crit._draw == 11
    plain = host.clone().to(dev)                                                 # no marker: the eager list, as before
    crit.reset(2)
    new, _ = computeEdgeIndex(plain.data, plain.attrs, r_max=R_CUT, key="CA", criteria=crit)
    assert torch.equal(new["edge_index"], eager["edge_index"]) and crit._draw == 3
    assert torch.equal(plain["_n_edges"], eager["_n_edges"])
    # a padded batch without a criterion takes the plain capped kernels through the same door
    from e3_layers_amd.data import computeEdgeIndexCapped

    a, b = _start(host, n_cap, e_cap, dev), _start(host, n_cap, e_cap, dev)
    computeEdgeIndex(a.data, a.attrs, r_max=R_CUT, key="CA")
    computeEdgeIndexCapped(b.data, b.attrs, r_max=R_CUT, key="CA")
    _same(a, b)
    assert a["_nlist_rng"].tolist() == [0, -1]                                   # no criterion: no draw


def test_a_batch_without_cells_draws_from_the_devices(dev):
    from e3_layers_amd.data import SequenceOrRandom, computeEdgeIndexCapped
    from e3_layers_amd.data.compute_edge import nlist_rng
    from e3_layers_amd.run.graph_step import pad_batch

    host = _host(4)
    crit = SequenceOrRandom("chain_id", 0, 0.02, seed=13)
    cells = nlist_rng(dev)
    assert cells.dtype == torch.int64 and cells.shape == (2,) and nlist_rng(dev) is cells
    first = int(cells[0])
    got = _start(host, N + 4, 1024, dev)
    got.data.pop("_nlist_rng")
    for k in range(2):                                                           # two builds: two consecutive draws of the device's cells
        computeEdgeIndexCapped(got.data, got.attrs, r_max=TINY, key="CA", criteria=crit)
        _same(got, pad_batch(_eager(host.clone().to(dev), TINY, crit, first + k), N + 4, 1024, key="CA"))
    assert cells.tolist() == [first + 2, first + 1]
