"""Host side of what the capped-replay clients share (run/capped.py, and the sizing rule and multi-tensor copy of run/graph_step.py);
no GPU."""
import os
import sys
from functools import partial
from types import SimpleNamespace

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "equivariant-nn-zoo_amd"))

from e3_layers_amd.data.synthetic import synth_qm9  # noqa: E402
from e3_layers_amd.run.graph_step import GHOST_DEGREE, bucket_capacity, copy_into, ghost_node_capacity, pad_batch  # noqa: E402


@pytest.mark.parametrize("n", [1, 31, 32, 33, 611])
@pytest.mark.parametrize("ghost_edges", [0, 1, 15, 16, 17, 1024, 3300])
def test_ghost_node_capacity_is_each_of_the_four_rules_it_replaced(n, ghost_edges):
    got = ghost_node_capacity(n, ghost_edges)
    e_cap = 4096
    e = e_min = e_cap - ghost_edges
    # graph_step.bucket_capacity, for one batch
    n_cap = max(n + max(2, -(-(e_cap - e) // GHOST_DEGREE)) for n, e in [(n, e)])
    assert got == -(-n_cap // 32) * 32
    # md.ReplayedForceField._build
    n_cap = n + max(2, -(-(e_cap - e) // GHOST_DEGREE))
    n_cap = -(-n_cap // 32) * 32
    assert got == n_cap
    # loops.CappedLoop.__init__
    assert got == -(-(n + max(2, -(-(e_cap - e) // GHOST_DEGREE))) // 32) * 32
    # score_step.ReplayedScoreStep._sized_node_capacity
    assert got == -(-(n + max(2, -(-max(e_cap - e_min, 0) // GHOST_DEGREE))) // 32) * 32
    assert ghost_node_capacity(n, ghost_edges, multiple=8) == -(-(n + max(2, -(-ghost_edges // GHOST_DEGREE))) // 8) * 8


def test_bucket_capacity_returns_what_it_returned_before_the_rule_moved():
    """The size lists of tests/test_padding.py; the constants are the results before ``ghost_node_capacity`` existed."""
    three = [(517, 7070), (618, 9812), (560, 8300)]
    for batch, sizes in ((synth_qm9(3, 8), [(170, 2726)]), (synth_qm9(4, 4), [(60, 746)])):
        assert [(batch["pos"].shape[0], batch["edge_index"].shape[1])] == sizes
    assert bucket_capacity([(170, 2726)]) == (192, 3072)
    assert bucket_capacity([(60, 746)]) == (96, 1024)
    assert bucket_capacity(three) == (736, 10240)
    assert [bucket_capacity([s]) for s in three] == [(544, 7168), (672, 10240), (640, 9216)]


def test_copy_into_issues_one_multi_tensor_copy_per_dtype(monkeypatch):
    torch.manual_seed(0)
    src = {"a": torch.randn(5, 3), "b": torch.randn(7), "i": torch.randint(0, 9, (2, 6)), "j": torch.randint(0, 9, (4, 1)),
           "strided": torch.randn(3, 6).t(), "other_dtype": torch.randn(4).double()}
    dst = {k: torch.zeros(v.shape, dtype=torch.float32 if k == "other_dtype" else v.dtype) for k, v in src.items()}
    assert not src["strided"].is_contiguous() and dst["strided"].is_contiguous()
    calls, singles = [], []
    foreach = torch._foreach_copy_

    def counted(dsts, srcs, *args, **kwargs):
        calls.append([t.dtype for t in dsts])
        return foreach(dsts, srcs, *args, **kwargs)

    class Recording(torch.Tensor):      # a destination that notes its own copy_
        def copy_(self, other, non_blocking=False):
            singles.append(self.data_ptr())
            return super().copy_(other, non_blocking=non_blocking)

    for k in ("strided", "other_dtype"):
        dst[k] = dst[k].as_subclass(Recording)
    monkeypatch.setattr(torch, "_foreach_copy_", counted)
    copy_into(dst, src, list(src))
    assert sorted(calls, key=str) == [[torch.float32, torch.float32], [torch.int64, torch.int64]]
    assert sorted(singles) == sorted(dst[k].data_ptr() for k in ("strided", "other_dtype"))
    for k, v in src.items():
        assert torch.equal(dst[k].as_subclass(torch.Tensor), v.to(dst[k].dtype)), k

    dst["b"] = torch.zeros(8)
    with pytest.raises(ValueError, match=r"b: \(7,\) does not fit the captured \(8,\) \(another bucket\? pad\(\) again after grow\(\)\)"):
        copy_into(dst, src, list(src), hint="pad() again after grow()")
    with pytest.raises(ValueError, match=r"b: \(7,\) does not fit the captured \(8,\) \(another bucket\?\)"):
        copy_into(dst, src, ["b"])


def test_edge_layer_of_reads_the_models_own_layer_once():
    from e3_layers_amd.configs import config_diffusion_CA, config_energy
    from e3_layers_amd.data import PairCriterion, computeEdgeIndex
    from e3_layers_amd.run.capped import edge_layer_of, replayable_criterion
    from e3_layers_amd.utils import build

    crit = config_diffusion_CA.pair_criterion()
    config = config_diffusion_CA.get_config(l_max=1, num_layers=2, n_dim=8, edge_criteria=crit)
    model = build(config.model_config)
    own = edge_layer_of(model)
    assert own.layer is model.layers[0][1] and own.key == "CA" and own.r_max == 8.0 / config.data_config.std
    assert isinstance(own.criterion, PairCriterion) and own.criterion is crit and replayable_criterion(own) is crit
    with pytest.raises(AttributeError):
        own.key = "pos"      # immutable
    assert edge_layer_of(build(config_energy.get_config(l_max=1, num_layers=2).model_config)) is None
    assert edge_layer_of(SimpleNamespace()) is None and edge_layer_of(SimpleNamespace(layers=[])) is None

    callback = SimpleNamespace(layers=[("edge_index", partial(computeEdgeIndex, r_max=0.3, key="CA", criteria=lambda data, ei: ei))])
    own = edge_layer_of(callback)
    assert own.key == "CA" and own.r_max == 0.3 and callable(own.criterion)
    with pytest.raises(ValueError, match="edge_capacity: the model's edge_index layer uses a criteria callback .*data.PairCriterion"):
        replayable_criterion(own)
    bare = edge_layer_of(SimpleNamespace(layers=[("edge_index", partial(computeEdgeIndex, r_max=0.3))]))
    assert bare.key is None and bare.criterion is None and replayable_criterion(bare) is None


def test_capped_bucket_carries_the_cells_and_unpads():
    from e3_layers_amd.run.capped import EDGE_KEYS, REBUILT_KEYS, CappedBucket

    assert REBUILT_KEYS == ("edge_index", "_n_edges", "_edge_segment")
    assert set(EDGE_KEYS) == set(REBUILT_KEYS) | {"edge_vector", "edge_length"} and len(EDGE_KEYS) == 5
    b = synth_qm9(3, 8)
    n, e, g = b["pos"].shape[0], b["edge_index"].shape[1], len(b)
    bucket = CappedBucket(pad_batch(b, 192, 3072), rng=True)
    assert (bucket.n_cap, bucket.e_cap, bucket.n_real, bucket.n_graphs) == (192, 3072, n, g)
    for name, cells in (("_nlist_state", bucket.state), ("_nlist_rng", bucket.rng)):
        assert bucket.padded[name] is cells and cells.dtype == torch.int64 and cells.tolist() == [0, 0]
    assert bucket.state is not bucket.rng and bucket.view()["_nlist_state"] is bucket.state
    given = torch.tensor([3, 3])
    assert CappedBucket(pad_batch(b, 192, 3072), rng=given).padded["_nlist_rng"] is given
    plain = CappedBucket(pad_batch(b, 192, 3072))
    assert plain.rng is None and "_nlist_rng" not in plain.padded and plain.padded["_nlist_state"].tolist() == [0, 0]

    out = bucket.real_graphs()
    assert len(out) == g and "_graph_weight" not in out and "_node_weight" not in out
    fields = [k for k in b.keys() if torch.is_tensor(b[k])]
    assert "pos" in fields and "edge_index" in fields and "species" in fields
    for k in fields:
        assert torch.equal(out[k], b[k]), k
    assert "edge_index" not in bucket.real_graphs(drop=REBUILT_KEYS) and "pos" in bucket.real_graphs(drop=REBUILT_KEYS)

    # from the batch with its present list: the node capacity is the sizing rule's at the present tail
    sized = CappedBucket.around_list(b, 3072)
    assert (sized.n_cap, sized.e_cap, sized.n_real) == (ghost_node_capacity(n, 3072 - e), 3072, n) and sized.n_cap == 192
    assert sized.padded["pos"].is_contiguous() and sized.rng is None and sized.state.tolist() == [0, 0]
    assert torch.equal(sized.real_graphs()["edge_index"], b["edge_index"])
