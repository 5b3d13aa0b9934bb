"""The probability-flow ODE sampler on the device (run/sde_sampling.get_ode_sampler): the eager loop against the float64 oracle loop of
tests/test_gpu_model.py (the textbook drift -0.5 beta (x + score), t held in fp32 as the device's table holds it), and the two
replayed loops -- the static-edge graph, the capped replay on cutoff graphs -- against the eager loop.  Bounds and set-ups are those
of tests/test_gpu_sampler_seeded.py for the same comparisons."""
import pytest
import torch

from tests.test_gpu_md import REPLAY      # replay vs eager
from tests.test_gpu_model import _build_pair, batch_to_oracle
from tests.test_gpu_protein_sampler_replay import STD, _model, _proteins
from tests.util import record_measured, rel_err

pytestmark = pytest.mark.gpu

SEED = 11


@pytest.fixture(scope="module")
def diffusion_pair(dev):
    """(product model, float64 oracle model, batch, the oracle's x_T): built once, left unchanged"""
    from e3_layers_amd.configs import config_diffusion
    from e3_layers_amd.data.compute_edge import normal_draw
    from e3_layers_amd.data.synthetic import synth_qm9_diffusion

    prod, orc = _build_pair(config_diffusion.get_config().model_config, dev)
    prod.eval(), orc.eval()
    batch = synth_qm9_diffusion(5, 3)
    n_atoms = batch["pos"].shape[0]
    x_T = normal_draw(SEED, 1000, torch.arange(n_atoms).reshape(-1, 1), torch.arange(3).reshape(1, -1), torch.float64)
    return prod, orc, batch, x_T


@pytest.mark.parametrize("method", ["heun", "euler"])
def test_eager_sampler_matches_the_float64_oracle_loop(dev, diffusion_pair, method):
    from e3_layers_amd.run.sde_sampling import get_ode_sampler
    from e3_layers_amd.run.sde_utils import VPSDE

    prod, orc, batch, x_T = diffusion_pair
    n_steps, n_iter, eps = 50, 4, 1e-3
    sampler = get_ode_sampler(VPSDE({"pos": 3}, N=1000), method=method, n_steps=n_steps, eps=eps, static_edges=True, n_iter=n_iter, seed=SEED)
    out, nfe = sampler(prod, batch.clone().to(dev))
    assert nfe == n_iter * (2 if method == "heun" else 1)
    data, attrs = batch_to_oracle(batch)

    def drift(x, t):
        d = dict(data)
        d["pos"], d["t"] = x, torch.full((len(batch), 1), t, dtype=torch.float64)
        with torch.no_grad():
            raw = orc(d, dict(attrs))[0]["score"]
        lm = -0.25 * t ** 2 * (20.0 - 0.1) - 0.5 * t * 0.1
        std = (1.0 - torch.exp(torch.tensor(2.0 * lm, dtype=torch.float64))).sqrt()
        score = -raw / std - x
        return -0.5 * (0.1 + t * (20.0 - 0.1)) * (x + score)

    times = torch.linspace(1.0, eps, n_steps + 1, dtype=torch.float32).double().tolist()      # the device's table holds t in fp32
    x = x_T.clone()
    for k in range(n_iter):
        t0, t1 = times[k], times[k + 1]
        h = t1 - t0
        d1 = drift(x, t0)
        if method == "euler":
            x = x + h * d1
        else:
            x = x + 0.5 * h * (d1 + drift(x + h * d1, t1))
    err = rel_err(out["pos"], x)
    print("eager ode sampler vs float64 oracle loop", method, err)
    record_measured("test_gpu_ode_sampler", case=f"eager_{method}_vs_f64_oracle_loop", rel_err=err)
    assert err < 2e-5, err
    # The untrained net's raw output is small: four steps move x by ~1e-5 of its norm, so the bound above alone would not see a wrong
    # drift.  The displacement itself, then.  Its fp32 error: every step ends in ONE rounding of x' (the final fma; stage A's x~ only
    # feeds the model), each at most 2^-24 |x'| per element, so n_iter 2^-24 |x| in norm; the drifts' own relative error (model
    # parity ~1e-5, a few roundings) is charged 1e-3 of the displacement.  The device's displacement is taken from the device's own
    # x_T (n_iter = 0: the prior alone), whose fp32 draw differs from the float64 one; the near-identity map carries that through.
    start, _ = get_ode_sampler(VPSDE({"pos": 3}, N=1000), method=method, n_steps=n_steps, eps=eps, static_edges=True, n_iter=0,
                               seed=SEED)(prod, batch.clone().to(dev))
    moved, want = (out["pos"].double() - start["pos"].double()).cpu(), x - x_T
    shift_err = rel_err(moved, want)
    shift_bound = n_iter * 2.0 ** -24 * float(x.norm()) / float(want.norm()) + 1e-3
    print("... its displacement", method, shift_err, "bound", shift_bound, "moved by", float(want.norm()) / float(x_T.norm()))
    record_measured("test_gpu_ode_sampler", case=f"eager_{method}_displacement", rel_err=shift_err, bound=shift_bound)
    assert shift_bound < 0.25 and shift_err < shift_bound, (shift_err, shift_bound)


@pytest.mark.parametrize("method,nfe_want", [("heun", 12), ("euler", 6)])
def test_static_edge_graph_replay_equals_the_eager_loop(dev, diffusion_pair, method, nfe_want):
    from e3_layers_amd.run.sde_sampling import get_ode_sampler
    from e3_layers_amd.run.sde_utils import VPSDE

    prod, _, batch, _ = diffusion_pair
    outs = []
    for graph in (False, True):
        sampler = get_ode_sampler(VPSDE({"pos": 3}, N=1000), method=method, n_steps=50, static_edges=True, graph=graph, n_iter=6, seed=SEED)
        out, nfe = sampler(prod, batch.clone().to(dev))
        assert nfe == nfe_want
        outs.append(out["pos"].clone())
    assert torch.isfinite(outs[0]).all()
    err = rel_err(outs[1], outs[0])
    print("ode static-edge graph vs eager", method, err)
    record_measured("test_gpu_ode_sampler", case=f"static_graph_{method}_vs_eager", rel_err=err)
    assert err < REPLAY, err
    with pytest.raises(ValueError, match="generator"):
        sampler(prod, batch.clone().to(dev), generator=torch.Generator(device=dev))


def test_capped_replay_equals_the_eager_loop_on_cutoff_graphs(dev):
    from e3_layers_amd.backend.graph import EdgeCapacityExceeded
    from e3_layers_amd.run.sde_sampling import get_ode_sampler
    from e3_layers_amd.run.sde_utils import VPSDE

    keys = {"CA": 3}
    model = _model(dev, keys, num_layers=3)
    batch = _proteins((70, 40)).to(dev)
    n_steps = 4

    def sde():
        return VPSDE(keys, beta_max=2.0)

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
        out_e, nfe = get_ode_sampler(sde(), method="heun", n_steps=n_steps, seed=SEED)(model, batch.clone())
    finally:
        model.layers[0] = (name, layer)
    assert nfe == 8 and len(seen) == 8, seen                                     # a build per model call: stage A and stage B
    assert len(set(seen)) > 1, seen                                              # the edge count changed during the run
    assert torch.isfinite(out_e["CA"]).all()

    def capped(e_cap, seed=SEED):
        sampler = get_ode_sampler(sde(), method="heun", n_steps=n_steps, graph=True, edge_capacity=e_cap, r_max=8.0 / STD, seed=seed)
        out, nfe = sampler(model, batch.clone())
        assert nfe == 8
        return out

    out_g = capped(max(seen) + 64)
    assert out_g["CA"].shape == out_e["CA"].shape and torch.isfinite(out_g["CA"]).all()
    err = rel_err(out_g["CA"], out_e["CA"])
    print("ode capped replay vs eager", err, seen)
    record_measured("test_gpu_ode_sampler", case="capped_heun_vs_eager", rel_err=err, edges=seen)
    assert err < REPLAY, err
    assert len(out_g) == len(batch) and "_graph_weight" not in out_g and "_nlist_state" not in out_g      # unpadded
    assert out_g["_n_nodes"].view(-1).tolist() == batch["_n_nodes"].view(-1).tolist()
    again = capped(max(seen) + 64)
    assert torch.equal(again["CA"], out_g["CA"])                                 # the same seed: the same bits
    other = capped(max(seen) + 4096, seed=SEED + 1)
    assert torch.isfinite(other["CA"]).all() and rel_err(other["CA"], out_e["CA"]) > REPLAY
    with pytest.raises(EdgeCapacityExceeded):                                    # one edge short of the largest list of the run
        capped(max(seen) - 1)
