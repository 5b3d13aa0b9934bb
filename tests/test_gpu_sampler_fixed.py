"""Conditional sampling on the device (run/sde_sampling.get_pc_sampler(seed=..., fixed=...)): the three loops -- eager, the static-edge
graph, the capped replay on cutoff graphs -- see the same counter-based draws with the same rows kept on known values, so they are
compared with each other directly, and the eager loop with the float64 oracle loop of tests/test_gpu_sampler_seeded.py extended by
the conditioned prior and the two replacements, fed the float64 form of the same draws at the layout's words.

Set-ups and bounds are those of tests/test_gpu_sampler_seeded.py (which says why the protein case runs VPSDE(N=4) with beta_max = 2).
The oracle loop keeps that file's 2e-5: the added steps are convex in the state and exact in x0 -- they overwrite rows with
m x0 + s z and amplify nothing."""
import pytest
import torch

from tests.test_gpu_md import REPLAY      # replay vs eager
from tests.test_gpu_model import _build_pair, batch_to_oracle
from tests.test_gpu_protein_sampler_replay import STD, _model, _proteins
from tests.util import record_measured, rel_err

pytestmark = pytest.mark.gpu

SEED = 11
KEYS = {"CA": 3}


def _sde():
    from e3_layers_amd.run.sde_utils import VPSDE

    return VPSDE(KEYS, beta_max=2.0, N=4)


def _with_mask(batch, mask, name="fixed"):
    batch.attrs[name] = ("node", "1x0e")
    batch[name] = mask.to(batch["_n_nodes"].device)
    return batch


def _recorded_eager(model, batch, **kwargs):
    """the seeded eager loop's result and the edge counts of its builds (one per model call)"""
    from e3_layers_amd.run.sde_sampling import EulerMaruyamaPredictor, LangevinCorrector, get_pc_sampler

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
        out, nfe = get_pc_sampler(_sde(), EulerMaruyamaPredictor, LangevinCorrector, seed=SEED, **kwargs)(model, batch.clone())
    finally:
        model.layers[0] = (name, layer)
    assert nfe == 8 and len(seen) == 8, seen
    return out, seen


def _capped(model, batch, e_cap, **kwargs):
    from e3_layers_amd.run.sde_sampling import EulerMaruyamaPredictor, LangevinCorrector, get_pc_sampler

    sampler = get_pc_sampler(_sde(), EulerMaruyamaPredictor, LangevinCorrector, graph=True, edge_capacity=e_cap, r_max=8.0 / STD, seed=SEED,
                             **kwargs)
    return sampler(model, batch.clone())[0]


def _motif(batch):
    """residues 20-39 of the first protein (70 residues; its first chain ends at residue 34, so the motif runs across the chain break)"""
    assert int(batch["_n_nodes"].reshape(-1)[0]) >= 40
    mask = torch.zeros(batch["CA"].shape[0], dtype=torch.bool, device=batch["CA"].device)
    mask[20:40] = True
    return mask


def test_conditioned_capped_replay_equals_the_conditioned_eager_loop(dev):
    from e3_layers_amd.backend.graph import EdgeCapacityExceeded

    model = _model(dev, KEYS, num_layers=3)
    batch = _proteins((70, 40)).to(dev)
    mask = _motif(batch)
    _with_mask(batch, mask.long())
    x0 = batch["CA"].clone()
    out_e, seen = _recorded_eager(model, batch, fixed="fixed")
    assert len(set(seen)) > 1, seen                                              # the edge count changed during the run
    assert torch.isfinite(out_e["CA"]).all()
    out_g = _capped(model, batch, max(seen) + 64, fixed="fixed")
    assert out_g["CA"].shape == out_e["CA"].shape
    err = rel_err(out_g["CA"], out_e["CA"])
    print("conditioned capped replay vs conditioned eager", err, seen)
    record_measured("test_gpu_sampler_fixed", case="capped_vs_eager", rel_err=err, edges=seen)
    assert err < REPLAY, err
    for out in (out_e, out_g):
        assert torch.equal(out["CA"][mask], x0[mask])                            # the motif: x0, bit for bit
        assert (out["CA"][~mask] != x0[~mask]).any(dim=1).all()                  # ... and nothing else is
        assert not [k for k in out.data if k.startswith("known_")]
        assert out["fixed"].dtype == torch.int64 and torch.equal(out["fixed"].reshape(-1), mask.long())      # the caller's own field
    assert torch.equal(batch["CA"], x0) and not [k for k in batch.data if k.startswith("known_")]      # the input is untouched
    assert len(out_g) == len(batch) and "_graph_weight" not in out_g and "_nlist_state" not in out_g      # unpadded
    assert out_g["_n_nodes"].view(-1).tolist() == batch["_n_nodes"].view(-1).tolist()
    assert out_g["edge_index"].shape == (2, seen[-1])
    again = _capped(model, batch, max(seen) + 64, fixed="fixed")
    assert torch.equal(again["CA"], out_g["CA"])                                 # the same seed: the same bits
    with pytest.raises(EdgeCapacityExceeded):                                    # one edge short of the largest list of the run
        _capped(model, batch, max(seen) - 1, fixed="fixed")
    # the conditioning matters to the free rows: the unconditioned run at the same seed is another trajectory
    plain, _ = _recorded_eager(model, batch)
    assert rel_err(plain["CA"][~mask], out_e["CA"][~mask]) > REPLAY


def test_an_all_zero_mask_is_the_unconditioned_sampler_on_the_device(dev):
    model = _model(dev, KEYS, num_layers=3)
    batch = _proteins((70, 40)).to(dev)
    plain, seen = _recorded_eager(model, batch)
    zero = _with_mask(batch.clone(), torch.zeros(batch["CA"].shape[0], dtype=torch.float32))
    out, seen_zero = _recorded_eager(model, zero, fixed="fixed")
    assert seen_zero == seen and torch.equal(out["CA"], plain["CA"])             # eager
    e_cap = max(seen) + 64
    assert torch.equal(_capped(model, zero, e_cap, fixed="fixed")["CA"], _capped(model, batch, e_cap)["CA"])      # capped


def test_conditioned_static_edge_graph_equals_the_conditioned_eager_loop(dev):
    from e3_layers_amd.configs import config_diffusion
    from e3_layers_amd.data.synthetic import synth_qm9_diffusion
    from e3_layers_amd.run.sde_sampling import EulerMaruyamaPredictor, LangevinCorrector, get_pc_sampler
    from e3_layers_amd.run.sde_utils import VPSDE
    from e3_layers_amd.utils import build

    torch.manual_seed(0)
    prod = build(config_diffusion.get_config().model_config).to(dev).eval()
    batch = synth_qm9_diffusion(6, 4).to(dev)
    seg = batch.nodeSegment()
    mask = torch.ones_like(seg, dtype=torch.bool)
    mask[1:] = seg[1:] != seg[:-1]                                               # the first atom of every molecule
    assert int(mask.sum()) == len(batch) and not mask.all()
    _with_mask(batch, mask)
    x0 = batch["pos"].clone()
    outs = []
    for graph in (False, True):
        sampler = get_pc_sampler(VPSDE({"pos": 3}, N=1000), EulerMaruyamaPredictor, LangevinCorrector, snr=0.16, static_edges=True,
                                 graph=graph, n_iter=6, seed=SEED, fixed="fixed")
        out, nfe = sampler(prod, batch.clone())
        assert nfe == 12
        assert torch.equal(out["pos"][mask], x0[mask]) and "known_pos" not in out
        outs.append(out["pos"].clone())
    assert torch.isfinite(outs[0]).all()
    err = rel_err(outs[1], outs[0])
    print("conditioned static-edge graph vs conditioned eager", err)
    record_measured("test_gpu_sampler_fixed", case="static_graph_vs_eager", rel_err=err)
    assert err < REPLAY, err
    with pytest.raises(ValueError, match="no field"):
        sampler(prod, synth_qm9_diffusion(6, 4).to(dev))


def test_conditioned_eager_sampler_matches_the_float64_oracle_loop(dev):
    """test_seeded_eager_sampler_matches_the_float64_oracle_loop's loop and bound with the conditioned prior and the two replacements:
    the prior at draw N (fixed rows m(T) x0 + s(T) z with the same z), step i's corrector at words c, its replacement at 6 + c, its
    predictor at 3 + c, its replacement at 9 + c, and x0 itself at the end.  The mask: the first atom of every molecule."""
    from e3_layers_amd.configs import config_diffusion
    from e3_layers_amd.data.compute_edge import normal_draw
    from e3_layers_amd.data.synthetic import synth_qm9_diffusion
    from e3_layers_amd.run.sde_sampling import EulerMaruyamaPredictor, LangevinCorrector, get_pc_sampler
    from e3_layers_amd.run.sde_utils import VPSDE

    tree = config_diffusion.get_config().model_config
    prod, orc = _build_pair(tree, dev)
    prod.eval(), orc.eval()
    batch = synth_qm9_diffusion(5, 3)
    n_atoms = batch["pos"].shape[0]
    seg = batch.nodeSegment()
    mask = torch.ones(n_atoms, dtype=torch.bool)
    mask[1:] = seg[1:] != seg[:-1]
    assert int(mask.sum()) == len(batch) and not mask.all()
    N, eps, snr, n_iter = 1000, 1e-3, 0.16, 4
    sampler = get_pc_sampler(VPSDE({"pos": 3}, N=N), EulerMaruyamaPredictor, LangevinCorrector, snr=snr, eps=eps, static_edges=True,
                             n_iter=n_iter, seed=SEED, fixed="fixed")
    out, nfe = sampler(prod, _with_mask(batch.clone(), mask).to(dev))
    assert nfe == 2 * n_iter
    node, comp = torch.arange(n_atoms).reshape(-1, 1), torch.arange(3).reshape(1, -1)
    rows = mask.reshape(-1, 1)

    def draw(step, word0):
        return normal_draw(SEED, step, node, word0 + comp, torch.float64)

    data, attrs = batch_to_oracle(batch)
    x0 = batch["pos"].double()

    def log_mean(t):
        return torch.tensor(-0.25 * t ** 2 * (20.0 - 0.1) - 0.5 * t * 0.1, dtype=torch.float64)

    def noised(t, z):      # x0 at the noise level of t
        lm = log_mean(t)
        return torch.exp(lm) * x0 + torch.sqrt(-torch.expm1(2.0 * lm)) * z

    z = draw(N, 0)
    x = torch.where(rows, noised(1.0, z), z)
    alphas = (1.0 - torch.linspace(0.1 / N, 20.0 / N, N)).double()

    def score(x, t):
        d = dict(data)
        d["pos"], d["t"] = x, torch.full((len(batch), 1), t, dtype=torch.float64)
        with torch.no_grad():
            raw = orc(d, dict(attrs))[0]["score"]
        std = (1.0 - torch.exp(2.0 * log_mean(t))).sqrt()
        return -raw / std - x

    for i, t in enumerate(torch.linspace(1.0, eps, N)[:n_iter].tolist()):
        t = float(torch.tensor(t, dtype=torch.float32))            # the device loop holds t in fp32
        grad, noise = score(x, t), draw(i, 0)
        alpha = alphas[int(t * (N - 1))]
        step = (snr * noise.norm(dim=-1).mean() / grad.norm(dim=-1).mean()) ** 2 * 2 * alpha      # (the norms: every row, fixed or not)
        x = x + step * grad + torch.sqrt(step * 2) * noise
        x = torch.where(rows, noised(t, draw(i, 6)), x)
        s, z = score(x, t), draw(i, 3)
        beta, dt = 0.1 + t * (20.0 - 0.1), -1.0 / N
        x = x + (-0.5 * beta * x) * dt + (beta ** 0.5) * (abs(dt) ** 0.5) * z
        x = x - dt * beta * s
        x = torch.where(rows, noised(t, draw(i, 9)), x)
    x = torch.where(rows, x0, x)
    got = out["pos"].cpu()
    assert torch.equal(got[mask], batch["pos"][mask])
    err, err_free = rel_err(got, x), rel_err(got[~mask], x[~mask])
    print("conditioned eager sampler vs float64 oracle loop", err, "free rows", err_free)
    record_measured("test_gpu_sampler_fixed", case="eager_vs_f64_oracle_loop", rel_err=err, rel_err_free_rows=err_free)
    assert err < 2e-5, err
    assert err_free < 2e-5, err_free
