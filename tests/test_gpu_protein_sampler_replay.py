"""The protein score nets' reverse-diffusion loop as replays of one HIP graph (run/sde_sampling.get_pc_sampler(graph=True,
edge_capacity=...)): the model's own ``edge_index`` layer, built with the declarative pair criterion, rebuilds the capped list inside
the capture == the eager sampler over the same steps with the same draws.

The small trees are ``score_config(..., l_max=1, n_dim=8)`` with THREE layers (four for the backbone's ``concat3`` behind ``layer3``): the
shared tree's score heads read ``8x0e+8x0o+8x1e+8x1o``, and a two-layer stack does not produce the ``0o`` block yet (it needs a
``1e x 1o`` product, and ``1e`` first appears in the second layer's output)."""
import pytest
import torch

from tests.test_gpu_md import REPLAY      # replay vs eager, the bound of test_pc_sampler_replays_a_graph_on_cutoff_graphs
from tests.util import rel_err

pytestmark = pytest.mark.gpu

STD = 25.83


def _model(dev, keys, num_layers, side_atoms=()):
    from e3_layers_amd.configs.config_dict import ConfigDict
    from e3_layers_amd.configs.config_diffusion_CA import pair_criterion, score_config
    from e3_layers_amd.utils import build

    data = ConfigDict()
    data.std = STD
    cfg = score_config(keys, data, l_max=1, num_layers=num_layers, n_dim=8, side_atoms=side_atoms, edge_criteria=pair_criterion(seed=5))
    torch.manual_seed(2)
    return build(cfg.model_config).to(dev).eval()


def _proteins(sizes, backbone=False):
    from e3_layers_amd.data import Batch
    from e3_layers_amd.data.synthetic import synth_protein

    parts = [synth_protein(10 + k, 1, n_res=n, backbone=backbone) for k, n in enumerate(sizes)]
    b = Batch.from_data_list([p.get(0) for p in parts], dict(parts[0].attrs))
    b.attrs.pop("_n_edges", None)
    assert b["chain_id"].max() == 1                  # two chains per protein
    return b


def _run_both(dev, model, batch, keys):
    """(eager result, replayed result, edge counts of the eager loop's builds) over the 4 steps of VPSDE(N=4), fixed noise."""
    from e3_layers_amd.run.sde_sampling import EulerMaruyamaPredictor, NoneCorrector, get_pc_sampler
    from e3_layers_amd.run.sde_utils import VPSDE

    fixed = torch.randn(4096, 3, generator=torch.Generator().manual_seed(3)).to(dev)

    def noise(shape):
        return fixed[:shape[0]]

    name, layer = model.layers[0]
    assert name == "edge_index"
    seen = []

    def recording(data, attrs):
        new, attrs = layer(data, attrs)
        seen.append(int(new["edge_index"].shape[1]))
        return new, attrs

    recording.keywords = layer.keywords
    model.layers[0] = (name, recording)
    try:
        eager = get_pc_sampler(VPSDE(keys, N=4), EulerMaruyamaPredictor, NoneCorrector)
        out_e, _ = eager(model, batch.clone(), noise_fn=noise)
    finally:
        model.layers[0] = (name, layer)
    assert len(seen) == 4

    def capped(e_cap):
        sampler = get_pc_sampler(VPSDE(keys, N=4), EulerMaruyamaPredictor, NoneCorrector, graph=True, edge_capacity=e_cap,
                                 r_max=8.0 / STD)
        return sampler(model, batch.clone(), noise_fn=noise)[0]

    return out_e, capped, seen


def _compare(out_e, out_g, seen, keys, batch):
    for k in keys:
        assert torch.isfinite(out_e[k]).all()
        assert out_g[k].shape == out_e[k].shape
        err = rel_err(out_g[k], out_e[k])
        print("protein_sampler_replay", k, err, seen)
        assert err < REPLAY, (k, err)
    assert len(set(seen)) > 1, seen                                              # the edge count changed during the loop
    assert len(out_g) == len(batch) and "_graph_weight" not in out_g and "_nlist_state" not in out_g      # unpadded
    assert out_g["edge_index"].shape == (2, seen[-1])                            # ... and carries the last list
    assert out_g["_n_nodes"].view(-1).tolist() == batch["_n_nodes"].view(-1).tolist()
    assert int(out_g["edge_index"].max()) < int(batch["_n_nodes"].sum())


def test_ca_score_net_samples_through_the_replayed_loop(dev):
    from e3_layers_amd.backend.graph import EdgeCapacityExceeded

    keys = {"CA": 3}
    model = _model(dev, keys, num_layers=3)
    batch = _proteins((70, 40)).to(dev)
    out_e, capped, seen = _run_both(dev, model, batch, keys)
    _compare(out_e, capped(max(seen) + 64), seen, keys, batch)
    crit = model.layers[0][1].keywords["criteria"]
    crit.seed += 1                                                               # other draws, another trajectory: the lists matter
    other = capped(max(seen) + 64)
    crit.seed -= 1
    assert rel_err(other["CA"], out_e["CA"]) > REPLAY
    with pytest.raises(EdgeCapacityExceeded):                                    # one edge short of the largest list of the run
        capped(max(seen) - 1)


def test_backbone_score_net_samples_through_the_replayed_loop(dev):
    keys = {"CA": 3, "C": 3, "O": 3, "N": 3}
    model = _model(dev, keys, num_layers=4, side_atoms=("C", "N", "O"))         # (concat3 sits behind layer3)
    batch = _proteins((40,), backbone=True).to(dev)
    out_e, capped, seen = _run_both(dev, model, batch, keys)
    _compare(out_e, capped(max(seen) + 64), seen, keys, batch)


def test_a_callback_in_the_models_layer_is_refused(dev):
    from e3_layers_amd.configs.config_dict import ConfigDict
    from e3_layers_amd.configs.config_diffusion_CA import score_config
    from e3_layers_amd.run.sde_sampling import EulerMaruyamaPredictor, NoneCorrector, get_pc_sampler
    from e3_layers_amd.run.sde_utils import VPSDE
    from e3_layers_amd.utils import build

    data = ConfigDict()
    data.std = STD
    model = build(score_config({"CA": 3}, data, l_max=1, num_layers=3, n_dim=8).model_config).to(dev).eval()      # the shipped callback
    sampler = get_pc_sampler(VPSDE({"CA": 3}, N=4), EulerMaruyamaPredictor, NoneCorrector, graph=True, edge_capacity=4096,
                             r_max=8.0 / STD)
    with pytest.raises(ValueError, match="PairCriterion"):
        sampler(model, _proteins((40,)).to(dev))
    with pytest.raises(ValueError, match="PairCriterion"):
        get_pc_sampler(VPSDE({"CA": 3}, N=4), EulerMaruyamaPredictor, NoneCorrector, graph=True, edge_capacity=4096, r_max=0.3,
                       criteria=lambda d, c: None)
