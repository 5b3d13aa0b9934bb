"""The declarative pair criterion (data/compute_edge.SequenceOrRandom) on the host: the torch predicate against a plain-Python double
loop, the counter-based hash against Python integers, the rate of its Bernoulli draw, the criterion as ``criteria=`` of
``computeEdgeIndex``, and padding with another position key.  No GPU."""
import math
import random

import pytest
import torch

M32 = 0xFFFFFFFF


def _mix(h):
    h ^= h >> 16
    h = (h * 0x7feb352d) & M32
    h ^= h >> 15
    h = (h * 0x846ca68b) & M32
    return h ^ (h >> 16)


def _hash(seed, draw, src, dst):
    """The pair hash in Python integers."""
    h = 0x9E3779B9
    for w in (seed & M32, (seed >> 32) & M32, draw & M32, src & M32, dst & M32):
        h = _mix(h ^ w)
    return h


def _keeps(c, chain, draw, i, j):
    """The rule on one ordered pair, in plain Python."""
    seq = chain[i] == chain[j] and abs(i - j) < c.window
    rnd = c.p >= 1.0 or _hash(c.seed, draw, i, j) < math.floor(c.p * 2 ** 32)
    return seq or rnd


SIZES = (7, 1, 12)


def _batch():
    """Three graphs of 7, 1 and 12 nodes, two chains per graph (the lone node: one), chain ids that REPEAT across graphs -- the
    pairs (6, 7), (7, 8) straddle graphs with equal ids; (2, 3), (3, 4) and (13, 14) straddle a chain boundary inside a graph."""
    from e3_layers_amd.data import Batch

    gen = torch.Generator().manual_seed(5)
    attrs = {"CA": ("node", "1x1o"), "chain_id": ("node", "1x0e"), "id": ("node", "1x0e")}
    lst = []
    for n, cut in zip(SIZES, (3, 1, 6)):
        chain = (torch.arange(n) >= cut).long().view(-1, 1)
        lst.append({"CA": torch.randn(n, 3, generator=gen), "chain_id": chain, "id": torch.arange(n).view(-1, 1),
                    "_n_nodes": torch.tensor([[n]])})
    b = Batch.from_data_list(lst, attrs)
    b.attrs.pop("_n_edges", None)
    return b


def _candidates():
    out, start = [], 0
    for n in SIZES:
        out += [(start + i, start + j) for i in range(n) for j in range(n)]
        start += n
    return out


@pytest.mark.parametrize("window", [0, 1, 5])
@pytest.mark.parametrize("p", [0.0, 0.3])
def test_predicate_equals_the_python_double_loop(window, p):
    from e3_layers_amd.data import PairCriterion, SequenceOrRandom

    b = _batch()
    chain = b["chain_id"].view(-1).tolist()
    cand = _candidates()
    assert (2, 3) in cand and (13, 14) in cand and (6, 7) not in cand
    ei = torch.tensor(cand).t().contiguous()
    c = SequenceOrRandom("chain_id", window, p, seed=(7 << 32) + 11)
    assert isinstance(c, PairCriterion)
    for draw in (0, 3):
        c.reset(draw)
        got = c(b, ei)
        want = torch.tensor([_keeps(c, chain, draw, i, j) for i, j in cand])
        assert got.dtype == torch.bool and torch.equal(got, want)
        if p == 0.0:
            near = torch.tensor([chain[i] == chain[j] and abs(i - j) < window for i, j in cand])
            assert torch.equal(got, near)      # p = 0: nothing from the random term
            if window == 5:
                assert not got[cand.index((2, 3))] and got[cand.index((0, 2))]      # across the chain boundary / inside a chain
    if window == 0 and p == 0.0:
        assert not got.any()


def test_the_callable_counts_its_draws_or_reads_them_from_the_batch():
    from e3_layers_amd.data import SequenceOrRandom

    b = _batch()
    ei = torch.tensor(_candidates()).t().contiguous()
    c = SequenceOrRandom("chain_id", 0, 0.3, seed=3)
    first, second = c(b, ei), c(b, ei)                # host counter: draws 0 and 1
    assert not torch.equal(first, second)             # consecutive draw indices: different masks
    c.reset()
    assert torch.equal(c(b, ei), first)               # the same index: the same mask
    c.reset(1)
    assert torch.equal(c(b, ei), second)
    b.data["_nlist_rng"] = torch.tensor([1, 0])       # the batch's cells name the draw; the host counter stays where it is
    c.reset(7)
    assert torch.equal(c(b, ei), second) and torch.equal(c(b, ei), second)
    assert b["_nlist_rng"].tolist() == [1, 0] and c._draw == 7


def test_hash_in_torch_equals_python_integers():
    from e3_layers_amd.data.compute_edge import pair_hash

    r = random.Random(1)
    quads = [(r.randrange(1 << 32, 1 << 63), r.randrange(1 << 33), r.randrange(1 << 31), r.randrange(1 << 31)) for _ in range(256)]
    want = torch.tensor([_hash(*q) for q in quads])
    seed, draw, src, dst = (torch.tensor(col) for col in zip(*quads))
    got = pair_hash(seed, draw, src, dst)
    assert got.dtype == torch.int64 and torch.equal(got, want)
    for q, w in zip(quads[:32], want[:32]):           # Python-int seed and draw, as the criterion passes them
        assert int(pair_hash(q[0], q[1], torch.tensor([q[2]]), torch.tensor([q[3]]))) == int(w)
    assert int(pair_hash((1 << 64) - 1, 0, torch.tensor([0]), torch.tensor([0]))) == _hash((1 << 64) - 1, 0, 0, 0)


def test_kept_fraction_is_binomial():
    """p = 0.02 over all ordered pairs of 1536 nodes, 3 seeds x 8 draw indices: within 5 sigma of the binomial."""
    from e3_layers_amd.data import SequenceOrRandom
    from e3_layers_amd.data.compute_edge import pair_hash

    n, p = 1536, 0.02
    sigma = math.sqrt(n * n * p * (1 - p)) / (n * n)
    ar = torch.arange(n)
    worst = 0.0
    for seed in (0, 12345, (9 << 32) + 77):
        c = SequenceOrRandom(None, 0, p, seed=seed)
        for draw in range(8):
            frac = float((pair_hash(seed, draw, ar[:, None], ar[None, :]) < c.threshold).double().mean())
            worst = max(worst, abs(frac - p) / sigma)
            assert abs(frac - p) <= 5 * sigma, (seed, draw, frac)
    print("kept fraction: worst |z| =", worst)
    # the predicate is this comparison
    ei = torch.stack([ar[:64].repeat_interleave(64), ar[:64].repeat(64)])
    assert torch.equal(c.predicate({}, ei, 7), (pair_hash(seed, 7, ar[:64, None], ar[None, :64]) < c.threshold).reshape(-1))


def test_p_one_keeps_every_candidate_and_p_zero_none():
    from e3_layers_amd.data import SequenceOrRandom

    b = _batch()
    ei = torch.tensor(_candidates()).t().contiguous()
    assert SequenceOrRandom("chain_id", 0, 1.0)(b, ei).all()
    assert SequenceOrRandom("chain_id", 5, 1.0, seed=9)(b, ei).all()
    assert not SequenceOrRandom("chain_id", 0, 0.0, seed=9)(b, ei).any()
    assert SequenceOrRandom(p=0.02).threshold == math.floor(0.02 * 2 ** 32)
    with pytest.raises(ValueError):
        SequenceOrRandom(p=1.5)


@pytest.mark.parametrize("r_max", [1e-6, 1.2])
def test_as_criteria_of_compute_edge_index_on_the_host(r_max):
    from e3_layers_amd.data import SequenceOrRandom, computeEdgeIndex

    b = _batch()
    chain, pos = b["chain_id"].view(-1).tolist(), b["CA"]
    c = SequenceOrRandom("chain_id", 3, 0.2, seed=21)
    c.reset(2)
    new, attrs = computeEdgeIndex(b.data, b.attrs, r_max=r_max, key="CA", criteria=c)
    want = [(i, j) for i, j in _candidates()
            if i != j and (float(torch.linalg.norm(pos[i] - pos[j])) < r_max or _keeps(c, chain, 2, i, j))]
    assert new["edge_index"].tolist() == [[i for i, _ in want], [j for _, j in want]]
    starts = [0, 7, 8, 20]
    per_graph = [sum(1 for i, _ in want if lo <= i < hi) for lo, hi in zip(starts[:-1], starts[1:])]
    assert b["_n_edges"].view(-1).tolist() == per_graph and attrs["_n_edges"] == ("graph", "1x0e")
    assert c._draw == 3                               # one call, one draw
    if r_max > 1:
        assert len(want) > sum(1 for i, j in _candidates() if i != j and _keeps(c, chain, 2, i, j))      # the cutoff added pairs


def test_pad_batch_places_the_ghost_positions_under_another_key():
    from e3_layers_amd.data import SequenceOrRandom, computeEdgeIndex
    from e3_layers_amd.data.synthetic import synth_qm9
    from e3_layers_amd.run.graph_step import ghost_positions, pad_batch

    b = _batch()
    assert "pos" not in b
    new, attrs = computeEdgeIndex(b.data, b.attrs, r_max=1e-6, key="CA", criteria=SequenceOrRandom("chain_id", 3, 0.0))
    b.attrs.update(attrs)
    b.update(new)
    n, e = 20, int(new["edge_index"].shape[1])
    padded = pad_batch(b, n + 5, e + 9, key="CA")
    assert torch.equal(padded["CA"][n:], ghost_positions(5)) and torch.equal(padded["CA"][:n], b["CA"])
    assert torch.equal(padded["chain_id"][n:], b["chain_id"][:1].expand(5, 1))
    assert torch.equal(padded["id"][n:], b["id"][:1].expand(5, 1))
    assert padded["_n_nodes"].view(-1).tolist() == [7, 1, 12, 5] and int(padded["_n_edges"][-1]) == 9
    assert int(padded["edge_index"][:, e:].min()) >= n and padded["edge_index"].shape[1] == e + 9
    with pytest.raises(KeyError):
        pad_batch(b, n + 5, e + 9)                    # the default key is "pos"
    q = synth_qm9(0, 3)
    nq, eq = int(q["pos"].shape[0]), int(q["edge_index"].shape[1])
    plain, keyed = pad_batch(q, nq + 3, eq + 4), pad_batch(q, nq + 3, eq + 4, key="pos")
    assert list(plain.keys()) == list(keyed.keys()) and plain.attrs == keyed.attrs
    for k in plain.keys():
        assert torch.equal(plain[k], keyed[k]), k


def test_config_hook_keeps_the_shipped_tree_and_offers_the_rule():
    from e3_layers_amd.configs import config_diffusion_backbone, config_diffusion_CA
    from e3_layers_amd.data import SequenceOrRandom

    rule = config_diffusion_CA.pair_criterion()
    assert isinstance(rule, SequenceOrRandom) and (rule.segment, rule.window, rule.p) == ("chain_id", 5, 0.02)
    for mod in (config_diffusion_CA, config_diffusion_backbone):
        name, layer = mod.get_config().model_config.layers[0]
        assert name == "edge_index" and layer.keywords["criteria"] is config_diffusion_CA.criteria
        name, layer = mod.get_config(edge_criteria=rule).model_config.layers[0]
        assert layer.keywords["criteria"] is rule and layer.keywords["key"] == "CA"
