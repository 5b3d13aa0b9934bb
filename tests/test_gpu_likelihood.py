"""The log-likelihood through the probability-flow ODE on the device (run/likelihood.get_likelihood_fn): one vector-Jacobian product and
the eager loop against the float64 oracle, the static-edge graph and the capped replay against the eager loop, the probe count.

Fixtures as tests/test_gpu_ode_sampler.py: ``config_diffusion`` on ``synth_qm9_diffusion(5, 3)`` with static edges, and the 3-layer
protein net of tests/test_gpu_protein_sampler_replay.py on ``_proteins((70, 40))``.

The oracle loop is the host restatement of run/likelihood.py over the oracle network (float64, and float32 as the yardstick of an fp32
path) with the float64 form of the same Rademacher probe -- the same signs, bit for bit.  ``delta_logp`` is compared on its own, per
graph, as a share of the majorant M_g = sum over the model calls of |w| c(t) |eps_g| |vjp_g| (taken from the eager HIP run, whose
``sampler_ode_div`` calls are watched): on an untrained net it is orders of magnitude below the prior term and would vanish in ``logp``."""
import pytest
import torch

from tests.test_gpu_md import REPLAY      # replay vs eager
from tests.test_gpu_model import _build_pair
from tests.test_gpu_protein_sampler_replay import STD, _model, _proteins
from tests.util import oracle_like, record_measured, rel_err

pytestmark = pytest.mark.gpu

SEED = (29 << 32) + 77
N_STEPS = 4
GRAD_TOL, GRAD_TOL_NORMALISED = 5e-5, 1e-4      # gradients against the float64 oracle


class OracleModel:
    """the oracle network behind the product's calling convention (a batch in, the batch with the head's output out), in its dtype"""

    def __init__(self, orc, dtype, head="score"):
        self.orc, self.dtype, self.head = orc, dtype, head

    def train(self, mode=True):
        return self

    def __call__(self, batch):
        data = {k: (v.to(self.dtype) if v.is_floating_point() else v) for k, v in batch.data.items() if not k.startswith("_e3k_")}
        out, attrs = self.orc(data, dict(batch.attrs))
        batch.attrs[self.head] = attrs[self.head]
        batch.data[self.head] = out[self.head]
        return batch


def _host(batch, dtype):
    b = batch.clone()
    for k, v in b.data.items():
        if v.is_floating_point():
            b.data[k] = v.to(dtype)
    return b


@pytest.fixture(scope="module")
def diffusion(dev):
    """(product model, float64 oracle, float32 oracle, batch): built once, left unchanged"""
    from e3_layers_amd.configs import config_diffusion
    from e3_layers_amd.data.synthetic import synth_qm9_diffusion

    tree = config_diffusion.get_config().model_config
    prod, orc = _build_pair(tree, dev)
    prod.eval(), orc.eval()
    orc32 = oracle_like(prod, tree, dtype=torch.float32).eval()
    return prod, orc, orc32, synth_qm9_diffusion(5, 3)


def _sde(n=1000):
    from e3_layers_amd.run.sde_utils import VPSDE

    return VPSDE({"pos": 3}, N=n)


def _watched(monkeypatch, sde, run):
    """-> (run()'s result, M [G] float64): the majorant of delta_logp from the ``sampler_ode_div`` launches of an EAGER device run"""
    from e3_layers_amd.backend import diffusion_ops
    from e3_layers_amd.run.likelihood import div_weight

    launch, major = diffusion_ops.sampler_ode_div, {}

    def spy(acc, probe, vjp, row_ptr, times, cells, n_graphs, stage, scale, beta_0, beta_1):
        ptr, k = row_ptr.cpu().tolist(), int(cells[1])
        coef = abs(div_weight(sde, times.cpu(), k, stage)) * scale
        for g in range(n_graphs):
            rows = slice(ptr[g], ptr[g + 1])
            major[g] = major.get(g, 0.0) + coef * float(probe[rows].double().norm()) * float(vjp[rows].double().norm())
        return launch(acc, probe, vjp, row_ptr, times, cells, n_graphs, stage, scale, beta_0, beta_1)

    monkeypatch.setattr(diffusion_ops, "sampler_ode_div", spy)
    try:
        out = run()
    finally:
        monkeypatch.setattr(diffusion_ops, "sampler_ode_div", launch)
    return out, torch.tensor([major[g] for g in sorted(major)], dtype=torch.float64)


def _vjp(model, batch, key, head, probe, ordered=True):
    """``ordered``: the backward as the likelihood runs it -- the harmonics' gradient summed in a fixed order"""
    import contextlib

    from e3_layers_amd.backend import ops

    b = batch.view()
    x = batch[key].detach().clone().requires_grad_(True)
    b.data[key] = x
    raw = model(b)[head]
    with ops.inputs_only_backward(), (ops.ordered_edge_gradients() if ordered else contextlib.nullcontext()):
        (g,) = torch.autograd.grad([raw], [x], grad_outputs=[probe.to(raw.dtype)])
    return g


def _reproducible(model, on_dev, key, head, eps, got, want):
    """the likelihood's backward gives the same bits pass after pass, and the same numbers as the backward with float atomics"""
    for _ in range(3):
        assert torch.equal(_vjp(model, on_dev, key, head, eps), got)
    atomics = _vjp(model, on_dev, key, head, eps, ordered=False)
    assert rel_err(atomics, want) < GRAD_TOL_NORMALISED and rel_err(atomics, got) < 1e-5


def test_one_vjp_against_the_float64_oracle(dev, diffusion):
    from e3_layers_amd.run.likelihood import make_probes

    prod, orc, _, batch = diffusion
    batch = batch.clone()
    batch.attrs["t"] = ("graph", "1x0e")
    batch["t"] = torch.full((len(batch), 1), 0.5)
    sde = _sde()
    eps64 = make_probes(sde, _host(batch, torch.float64), SEED, "rademacher", 1)[0, "pos"]
    on_dev = batch.clone().to(dev)
    eps = make_probes(sde, on_dev, SEED, "rademacher", 1)[0, "pos"]
    assert torch.equal(eps.cpu().double(), eps64) and set(eps64.unique().tolist()) == {-1.0, 1.0}      # the same signs on both sides
    got = _vjp(prod, on_dev, "pos", "score", eps)
    want = _vjp(OracleModel(orc, torch.float64), _host(batch, torch.float64), "pos", "score", eps64)
    err = rel_err(got, want)
    print("vjp vs float64 oracle (config_diffusion)", err, "norm", float(want.norm()))
    record_measured("test_gpu_likelihood", case="vjp_config_diffusion", rel_err=err)
    assert float(want.norm()) > 0 and err < GRAD_TOL, err
    _reproducible(prod, on_dev, "pos", "score", eps, got, want)


def test_one_vjp_of_the_protein_net_against_the_float64_oracle(dev):
    """the 3-layer normalised protein net; the seeded edge set is built once on the CPU and fed to both sides (tests/test_gpu_model.py)"""
    from e3_layers_amd.configs.config_dict import ConfigDict
    from e3_layers_amd.configs.config_diffusion_CA import pair_criterion, score_config
    from e3_layers_amd.run.likelihood import make_probes
    from e3_layers_amd.run.sde_utils import VPSDE

    keys = {"CA": 3}
    data = ConfigDict()
    data.std = STD
    tree = score_config(keys, data, l_max=1, num_layers=3, n_dim=8, edge_criteria=pair_criterion(seed=5)).model_config
    batch = _proteins((70, 40))
    new, _ = dict(tree.layers)["edge_index"](batch.data, batch.attrs)
    batch["edge_index"] = new["edge_index"]
    tree.layers = [layer for layer in tree.layers if layer[0] != "edge_index"]
    torch.manual_seed(2)
    prod, orc = _build_pair(tree, dev)
    prod.eval(), orc.eval()
    batch.attrs["t"] = ("graph", "1x0e")
    batch["t"] = torch.full((len(batch), 1), 0.5)
    sde = VPSDE(keys, beta_max=2.0)
    eps64 = make_probes(sde, _host(batch, torch.float64), SEED, "rademacher", 1)[0, "CA"]
    on_dev = batch.clone().to(dev)
    eps = eps64.float().to(dev)
    got = _vjp(prod, on_dev, "CA", "score_CA", eps)
    want = _vjp(OracleModel(orc, torch.float64, "score_CA"), _host(batch, torch.float64), "CA", "score_CA", eps64)
    err = rel_err(got, want)
    print("vjp vs float64 oracle (protein net)", err, "norm", float(want.norm()))
    record_measured("test_gpu_likelihood", case="vjp_protein", rel_err=err)
    assert float(want.norm()) > 0 and err < GRAD_TOL_NORMALISED, err
    _reproducible(prod, on_dev, "CA", "score_CA", eps, got, want)


@pytest.mark.parametrize("method", ["heun", "euler"])
def test_eager_loop_against_the_float64_oracle_loop(dev, diffusion, monkeypatch, method):
    from e3_layers_amd.run.likelihood import get_likelihood_fn

    prod, orc, orc32, batch = diffusion
    sde = _sde()
    fn = get_likelihood_fn(sde, method, n_steps=N_STEPS, static_edges=True, seed=SEED)
    (logp, latent, info), major = _watched(monkeypatch, sde, lambda: fn(prod, batch.clone().to(dev)))
    assert info["nfe"] == N_STEPS * (2 if method == "heun" else 1)
    assert logp.dtype == torch.float64 and logp.shape == (len(batch),) and torch.isfinite(logp).all()
    ref, ref_latent, ref_info = fn(OracleModel(orc, torch.float64), _host(batch, torch.float64))
    _, _, f32_info = fn(OracleModel(orc32, torch.float32), _host(batch, torch.float32))
    err = rel_err(latent["pos"], ref_latent["pos"])
    prior_err = float(((info["prior_logp"].cpu() - ref_info["prior_logp"]).abs() / ref_info["prior_logp"].abs()).max())
    delta, want = info["delta_logp"].cpu(), ref_info["delta_logp"]
    hip_share = float(((delta - want).abs() / major).max())
    f32_share = float(((f32_info["delta_logp"] - want).abs() / major).max())
    print("likelihood eager vs float64 oracle loop", method, "latent", err, "prior", prior_err, "delta share: hip", hip_share, "float32 oracle",
          f32_share, "delta", delta.tolist(), "majorant", major.tolist(), "prior_logp", ref_info["prior_logp"].tolist())
    record_measured("test_gpu_likelihood", case=f"eager_{method}_vs_f64_oracle_loop", latent=err, prior=prior_err, delta_share_hip=hip_share,
                    delta_share_f32_oracle=f32_share)
    assert err < 2e-5, err                        # the samplers' bound
    assert prior_err < 1e-6, prior_err
    assert (want.abs() <= major * (1 + 1e-3)).all()                  # (a majorant indeed)
    assert hip_share <= 4.0 * f32_share, (hip_share, f32_share)      # the margin of fp32 paths whose summation orders differ
    assert (delta != 0).all()
    other, _, other_info = get_likelihood_fn(sde, method, n_steps=N_STEPS, static_edges=True, seed=SEED + 1)(prod, batch.clone().to(dev))
    assert ((other_info["delta_logp"].cpu() - delta).abs() > 1e-3 * major).all()      # another seed: another probe
    assert torch.equal(other_info["prior_logp"], info["prior_logp"])                  # ... and the same flow


@pytest.mark.parametrize("method", ["heun", "euler"])
def test_static_edge_graph_replay_equals_the_eager_loop(dev, diffusion, monkeypatch, method):
    from e3_layers_amd.run.likelihood import get_likelihood_fn

    prod, _, _, batch = diffusion
    sde = _sde()
    eager = get_likelihood_fn(sde, method, n_steps=6, static_edges=True, seed=SEED)
    (logp_e, lat_e, info_e), major = _watched(monkeypatch, sde, lambda: eager(prod, batch.clone().to(dev)))
    logp_g, lat_g, info_g = get_likelihood_fn(sde, method, n_steps=6, static_edges=True, graph=True, seed=SEED)(prod, batch.clone().to(dev))
    assert info_g["nfe"] == info_e["nfe"] == 6 * (2 if method == "heun" else 1)
    err = rel_err(lat_g["pos"], lat_e["pos"])
    share = float(((info_g["delta_logp"] - info_e["delta_logp"]).abs().cpu() / major).max())
    print("likelihood static-edge graph vs eager", method, err, share)
    record_measured("test_gpu_likelihood", case=f"static_graph_{method}_vs_eager", latent=err, delta_share=share)
    assert err < REPLAY, err
    assert share < 1e-5, share                    # (the warm-up step's share went back to zero with the cells: it would be O(1 / 6))
    assert torch.isfinite(logp_g).all() and logp_g.shape == (len(batch),)


def test_capped_replay_equals_the_eager_loop_on_cutoff_graphs(dev, monkeypatch):
    from e3_layers_amd.backend.graph import EdgeCapacityExceeded
    from e3_layers_amd.run.likelihood import get_likelihood_fn
    from e3_layers_amd.run.sde_utils import VPSDE

    keys = {"CA": 3}
    model = _model(dev, keys, num_layers=3)
    batch = _proteins((70, 40)).to(dev)
    sde = VPSDE(keys, beta_max=2.0)
    name, layer = model.layers[0]
    assert name == "edge_index"
    seen = []

    def recording(data, attrs):
        new, attrs = layer(data, attrs)
        seen.append(int(new["edge_index"].shape[1]))
        return new, attrs

    recording.keywords = layer.keywords
    eager = get_likelihood_fn(sde, "heun", n_steps=N_STEPS, seed=SEED)
    model.layers[0] = (name, recording)
    try:
        (logp_e, lat_e, info_e), major = _watched(monkeypatch, sde, lambda: eager(model, batch.clone()))
    finally:
        model.layers[0] = (name, layer)
    assert info_e["nfe"] == 8 and len(seen) == 8, seen
    assert torch.isfinite(lat_e["CA"]).all() and torch.isfinite(logp_e).all() and (info_e["delta_logp"] != 0).all()
    logp_e2, lat_e2, _ = eager(model, batch.clone())
    assert torch.equal(lat_e2["CA"], lat_e["CA"])
    eager_bits = torch.equal(logp_e2, logp_e)      # the likelihood's backward is bit-reproducible (ops.ordered_edge_gradients())
    assert eager_bits
    print("two eager runs: logp bit-equal", eager_bits, "worst share", float(((logp_e2 - logp_e).abs().cpu() / major).max()))

    def capped(e_cap):
        fn = get_likelihood_fn(sde, "heun", n_steps=N_STEPS, graph=True, edge_capacity=e_cap, r_max=8.0 / STD, seed=SEED)
        return fn(model, batch.clone())

    logp_g, lat_g, info_g = capped(max(seen) + 64)
    assert info_g["nfe"] == 8
    err = rel_err(lat_g["CA"], lat_e["CA"])
    share = float(((info_g["delta_logp"] - info_e["delta_logp"]).abs().cpu() / major).max())
    print("likelihood capped replay vs eager", err, share, seen)
    record_measured("test_gpu_likelihood", case="capped_heun_vs_eager", latent=err, delta_share=share, edges=seen, eager_bit_equal=float(eager_bits))
    assert err < REPLAY, err
    assert share < 1e-5, share
    # unpadded: an entry per graph of the batch, none for the ghost graph
    assert logp_g.shape == (len(batch),) and info_g["delta_logp"].shape == info_g["prior_logp"].shape == info_g["dims"].shape == (len(batch),)
    assert len(lat_g) == len(batch) and "_graph_weight" not in lat_g and "_nlist_state" not in lat_g
    assert lat_g["CA"].shape == lat_e["CA"].shape and not any(k.startswith("probe") for k in lat_g.data)
    assert info_g["dims"].tolist() == [3 * 70, 3 * 40]
    logp_g2, lat_g2, _ = capped(max(seen) + 64)
    assert torch.equal(lat_g2["CA"], lat_g["CA"])                    # the same seed: the same bits
    assert torch.equal(logp_g2, logp_g)
    with pytest.raises(EdgeCapacityExceeded):                        # one edge short of the largest list of the run
        capped(max(seen) - 1)


def test_probe_count(dev, diffusion, monkeypatch):
    """``n_probes = 2``: ``nfe`` unchanged, ``delta_logp`` the mean of the two single-probe runs within 1e-12 of the majorant.  Three
    separate passes through the model's backward: the bound is that of a bit-reproducible backward, which the likelihood's is
    (``ops.ordered_edge_gradients()``; with the float atomics of ``e3k_tp_bwd_w`` the share was 2.7e-9 to 6.0e-9)."""
    from e3_layers_amd.run.likelihood import get_likelihood_fn

    prod, _, _, batch = diffusion
    singles = []
    for n in (1000, 1001):      # one probe each, at draw indices sde.N + 1 = 1001 and 1002
        _, _, info = get_likelihood_fn(_sde(n), "heun", n_steps=N_STEPS, static_edges=True, seed=SEED)(prod, batch.clone().to(dev))
        singles.append(info["delta_logp"])
    sde = _sde()
    both = get_likelihood_fn(sde, "heun", n_steps=N_STEPS, n_probes=2, static_edges=True, seed=SEED)
    (_, _, info), major = _watched(monkeypatch, sde, lambda: both(prod, batch.clone().to(dev)))
    assert info["nfe"] == 2 * N_STEPS
    mean = 0.5 * (singles[0] + singles[1])
    share = float(((info["delta_logp"] - mean).abs().cpu() / major).max())
    apart = float(((singles[0] - singles[1]).abs().cpu() / major).min())
    print("two probes vs the mean of the single-probe runs", share, "the two runs apart", apart)
    record_measured("test_gpu_likelihood", case="two_probes_vs_mean", delta_share=share)
    assert apart > 1e-3 and share < 1e-12, (share, apart)
