"""Replayed force evaluation and velocity-Verlet MD (run/md.py) on the device, against the eager path and the float64 oracle, and
the sampler's capped-list graph mode (run/sde_sampling.py).

The oracle of the force tree is built as ``test_forces_by_autograd`` builds it (``tests.util.oracle_like`` renames the keys of
sequential trees only: a bare ``GradientOutput`` keeps its network under ``func.mods.``); ``dtype=float32`` gives the yardstick loop."""
import pytest
import torch

from oracle import e3ref
from tests.util import record_measured, rel_err, zero_shifts

pytestmark = pytest.mark.gpu

TOL = 1e-5       # energy: fp32 vs the float64 oracle, normwise, shifts zeroed (tests/test_gpu_model.py)
FTOL = 5e-5      # forces (test_forces_by_autograd)
REPLAY = 1e-5    # replay vs eager (test_pc_sampler_graph_replay_equals_eager)


def _small_tree():
    from e3_layers_amd.configs.layer_configs import addEnergyOutput, addForceOutput, featureModel

    cfg = featureModel(n_dim=16, l_max=2, edge_spherical="1x0e+1x1o+1x2e", node_attrs="16x0e", edge_radial="8x0e",
                       num_types=10, num_layers=3, r_max=4.0)
    return addForceOutput(addEnergyOutput(cfg, None, output_key="energy_total"), y="energy_total")


def _oracle(prod, tree, dtype=torch.float64):
    orc = e3ref.build(tree)
    orc.load_state_dict({k.replace("func.", "func.mods.", 1): v.detach().cpu() for k, v in prod.state_dict().items()})
    return orc.to(dtype).eval()


def _build(tree, dev):
    from e3_layers_amd.utils import build

    torch.manual_seed(0)
    return build(tree).to(dev).eval()


class _OracleField:
    """The oracle as a force field on the host: ``compute_edge_index`` on the given positions, then the network."""

    def __init__(self, orc, batch, r_max, energy_key, dtype):
        self.orc, self.batch, self.r_max, self.energy_key, self.dtype = orc, batch, r_max, energy_key, dtype
        self.edge_counts = []

    def __call__(self, x):
        b = self.batch
        data = {"pos": x.detach().to(self.dtype).clone(), "species": b["species"], "_n_nodes": b["_n_nodes"]}
        new, attrs = e3ref.compute_edge_index(data, {k: b.attrs[k] for k in ("pos", "species")}, r_max=self.r_max)
        data.update(new)
        self.edge_counts.append(int(new["edge_index"].shape[1]))
        out, _ = self.orc(data, attrs)
        return out[self.energy_key].detach().reshape(-1), out["forces"].detach()


def _oracle_verlet(field, x0, v0, mass, dt, n_steps):
    """Velocity Verlet restated on the host in the field's dtype: final x, v and the total energy before and after every step."""
    dt_ = field.dtype
    x, v, m = x0.to(dt_).clone(), v0.to(dt_).clone(), mass.to(dt_)[:, None]
    e, f = field(x)
    total = [float(e.double().sum() + (0.5 * m * v * v).double().sum())]
    for _ in range(n_steps):
        v = v + 0.5 * dt * f / m
        x = x + dt * v
        e, f = field(x)
        v = v + 0.5 * dt * f / m
        total.append(float(e.double().sum() + (0.5 * m * v * v).double().sum()))
    return x, v, torch.tensor(total, dtype=torch.float64)


def _device_verlet(ff, x0, v0, mass, dt, n_steps, check_every=5):
    """The same on the device: final x, v (host, float64) and the total energies [n_steps + 1]."""
    from e3_layers_amd.run.md import VelocityVerlet

    e0, _ = ff(x0.to(ff.dev, torch.float32))
    ff.check()
    md = VelocityVerlet(ff, mass, dt)
    md.v.copy_(v0.to(ff.dev, torch.float32))
    first = float(e0.detach().double().sum().cpu() + (0.5 * mass.double()[:, None] * v0.float().double() ** 2).sum())
    out = md.run(n_steps, check_every=check_every)
    total = (out["potential"].double().sum(1) + out["kinetic"].double().sum(1)).cpu()
    return md, torch.cat([torch.tensor([first], dtype=torch.float64), total])


def _eager(prod, batch, pos, r_max, dev):
    from e3_layers_amd.data import computeEdgeIndex

    b = batch.clone().to(dev)
    b["pos"] = pos.to(dev, torch.float32)
    for k in ("edge_index", "_n_edges", "_edge_segment"):
        b.pop(k)
    new, attrs = computeEdgeIndex(b.data, b.attrs, r_max=r_max)
    b.attrs.update(attrs)
    b.update(new)
    return prod(b), int(new["edge_index"].shape[1])


@pytest.mark.parametrize("which", ["small", "shipped"])
def test_replayed_force_field_equals_eager_and_the_oracle(dev, which):
    """ff(pos) on moved positions (the edge count changes) == computeEdgeIndex + the eager model on the unpadded batch (1e-5), and
    within the forward / force bounds of the float64 oracle at every evaluation."""
    from e3_layers_amd.configs import config_energy_force
    from e3_layers_amd.data.synthetic import synth_qm9
    from e3_layers_amd.run.md import ReplayedForceField

    if which == "small":
        tree, r_max, e_key, batch = _small_tree(), 4.0, "energy_total", synth_qm9(7, 3)
    else:
        tree = config_energy_force.get_config().model_config
        r_max, e_key, batch = 5.0, "energy", synth_qm9(2000, 4, r_max=5.0)
    prod = _build(tree, dev)
    orc = _oracle(prod, tree)
    zero_shifts(prod, orc)
    field = _OracleField(orc, batch, r_max, e_key, torch.float64)
    ff = ReplayedForceField(prod, batch.clone().to(dev), r_max, energy_key=e_key, forces_key="forces")
    gen = torch.Generator().manual_seed(11)
    counts, worst = [], [0.0, 0.0, 0.0, 0.0]
    for step, scale in enumerate((0.0, 0.25, 0.4, 0.15)):
        pos = batch["pos"] + scale * torch.randn(batch["pos"].shape, generator=gen)
        energy, forces = ff(pos.to(dev))
        ff.check()
        out, n_edges = _eager(prod, batch, pos, r_max, dev)
        counts.append(n_edges)
        assert int(ff.n_edges) == n_edges
        errs = [rel_err(energy, out[e_key].reshape(-1)), rel_err(forces, out["forces"])]
        e_ref, f_ref = field(pos)
        errs += [rel_err(energy, e_ref), rel_err(forces, f_ref)]
        print(which, step, n_edges, errs)
        worst = [max(a, b) for a, b in zip(worst, errs)]
        assert errs[0] < REPLAY and errs[1] < REPLAY, (step, errs)
        assert errs[2] < TOL and errs[3] < FTOL, (step, errs)
    assert len(set(counts)) >= 3, counts                      # the moves changed the edge set
    assert counts == field.edge_counts
    record_measured(f"md_force_field_{which}", replay_energy=worst[0], replay_forces=worst[1], oracle_energy=worst[2],
                    oracle_forces=worst[3])


def test_trajectory_follows_the_float64_loop_as_closely_as_a_float32_loop_does(dev):
    """20 velocity-Verlet steps, unit masses, velocities large enough that the neighbour list changes on the way: the device
    trajectory against the same loop on the float64 oracle.  Yardstick: what the oracle loop in float32 makes of it (d32); the
    device may be off by 4 x d32 (other summation orders, the knot table's interpolation -- its guard bounds that at 1e-5 per
    column, below the fp32 error of a force)."""
    from e3_layers_amd.data.synthetic import synth_qm9
    from e3_layers_amd.run.md import ReplayedForceField

    tree, r_max, dt, n_steps = _small_tree(), 4.0, 0.02, 20
    prod = _build(tree, dev)
    batch = synth_qm9(7, 3)
    x0 = batch["pos"].clone()
    v0 = torch.randn(x0.shape, generator=torch.Generator().manual_seed(1), dtype=torch.float64).float()
    mass = torch.ones(x0.shape[0])
    f64 = _OracleField(_oracle(prod, tree), batch, r_max, "energy_total", torch.float64)
    f32 = _OracleField(_oracle(prod, tree, torch.float32), batch, r_max, "energy_total", torch.float32)
    x64, _, e64 = _oracle_verlet(f64, x0, v0, mass, dt, n_steps)
    assert len(set(f64.edge_counts)) >= 2, f64.edge_counts    # the list changed along the reference trajectory
    x32, _, e32 = _oracle_verlet(f32, x0, v0, mass, dt, n_steps)
    ff = ReplayedForceField(prod, batch.clone().to(dev), r_max, energy_key="energy_total", forces_key="forces")
    md, e_dev = _device_verlet(ff, x0, v0, mass, dt, n_steps)
    assert md.regrowths == 0
    d32_x, d32_e = float((x32.double() - x64).norm()), float((e32 - e64).abs().max())
    dev_x, dev_e = float((md.x.double().cpu() - x64).norm()), float((e_dev - e64).abs().max())
    print("md_trajectory", dict(dev_x=dev_x, d32_x=d32_x, dev_e=dev_e, d32_e=d32_e, edges=sorted(set(f64.edge_counts))))
    record_measured("md_trajectory", device_positions=dev_x, float32_positions=d32_x, device_energy=dev_e, float32_energy=d32_e)
    assert dev_x <= 4 * d32_x, (dev_x, d32_x)
    assert dev_e <= 4 * d32_e, (dev_e, d32_e)


def test_an_outgrown_list_is_regrown_and_the_chunk_redone(dev):
    """Velocities towards the centroids: the edge count grows past the first bucket (no slack, a fine bucket grid); the run grows
    the capacity, redoes the chunk, and ends where a run with ample capacity ends."""
    from e3_layers_amd.data.synthetic import synth_qm9
    from e3_layers_amd.run.md import ReplayedForceField

    tree, r_max, dt, n_steps = _small_tree(), 4.0, 0.02, 12
    prod = _build(tree, dev)
    batch = synth_qm9(7, 3)
    x0, seg = batch["pos"].clone(), batch["_node_segment"]
    cen = torch.zeros(len(batch), 3).index_add_(0, seg, x0) / batch["_n_nodes"].float()
    v0 = -(x0 - cen[seg])
    mass = torch.ones(x0.shape[0])
    runs = {}
    for name, kw in (("tight", dict(edge_slack=1.0, edge_multiple=32)), ("ample", dict(edge_slack=2.0))):
        ff = ReplayedForceField(prod, batch.clone().to(dev), r_max, energy_key="energy_total", forces_key="forces", **kw)
        first_cap = ff.e_cap
        md, e_tot = _device_verlet(ff, x0, v0, mass, dt, n_steps, check_every=4)
        runs[name] = (md, e_tot, first_cap, ff)
    tight, ample = runs["tight"], runs["ample"]
    assert ample[0].regrowths == 0
    assert tight[0].regrowths >= 1 and tight[0].restores >= 1 and tight[3].e_cap > tight[2]
    assert int(tight[3].n_edges) > tight[2]                    # the final list would not have fitted the first bucket
    assert rel_err(tight[0].x, ample[0].x) < REPLAY and rel_err(tight[0].v, ample[0].v) < REPLAY
    assert rel_err(tight[1], ample[1]) < REPLAY
    assert torch.isfinite(tight[1]).all()


def test_energy_is_conserved_to_second_order_across_list_changes(dev):
    """The forces are the gradient of the energy the run reports, also where the list changes: halving dt quarters the drift
    max |E_tot(t) - E_tot(0)|.  dt and the length are chosen (on the host, asserted here) so that the float64 loop is in the
    second-order regime (ratio in [3.5, 4.5]) and the float32 loop's drift at dt is >= 10 x its drift at dt / 8 (above the fp32
    floor); the device must at least halve it (4 x expected; the factor 2 is room for fp32 noise on the smaller drift)."""
    from e3_layers_amd.data.synthetic import synth_qm9
    from e3_layers_amd.run.md import ReplayedForceField

    tree, r_max, dt, n_steps = _small_tree(), 4.0, 0.16, 8
    prod = _build(tree, dev)
    batch = synth_qm9(7, 3)
    x0 = batch["pos"].clone()
    v0 = (0.5 * torch.randn(x0.shape, generator=torch.Generator().manual_seed(1), dtype=torch.float64)).float()
    mass = torch.ones(x0.shape[0])

    def drift(e):
        return float((e - e[0]).abs().max())

    f64 = _OracleField(_oracle(prod, tree), batch, r_max, "energy_total", torch.float64)
    d64 = [drift(_oracle_verlet(f64, x0, v0, mass, dt / k, n_steps * k)[2]) for k in (1, 2)]
    assert len(set(f64.edge_counts)) >= 2, f64.edge_counts
    assert 3.5 <= d64[0] / d64[1] <= 4.5, d64
    f32 = _OracleField(_oracle(prod, tree, torch.float32), batch, r_max, "energy_total", torch.float32)
    d32 = [drift(_oracle_verlet(f32, x0, v0, mass, dt / k, n_steps * k)[2]) for k in (1, 8)]
    assert d32[0] >= 10 * d32[1], d32
    ff = ReplayedForceField(prod, batch.clone().to(dev), r_max, energy_key="energy_total", forces_key="forces")
    d_dev = [drift(_device_verlet(ff, x0, v0, mass, dt / k, n_steps * k, check_every=8)[1]) for k in (1, 2)]
    print("md_energy_drift", dict(device=d_dev, float64=d64, float32=d32))
    record_measured("md_energy_drift", device_dt=d_dev[0], device_half_dt=d_dev[1], float64_dt=d64[0], float64_half_dt=d64[1],
                    float32_dt=d32[0], float32_eighth_dt=d32[1])
    assert d_dev[1] < 0.5 * d_dev[0], d_dev


def test_pc_sampler_replays_a_graph_on_cutoff_graphs(dev):
    """graph=True with edge_capacity on the cutoff tree of test_pc_sampler_rebuilds_edges_on_device: the captured step rebuilds
    the list with the capped builder == the eager rebuild loop over the same steps (fixed noise), and the edge set did change.
    The cutoff is an argument of its own, and a corrector with batch-wide norms is refused (the ghost nodes would enter them)."""
    from e3_layers_amd.configs.layer_configs import featureModel
    from e3_layers_amd.data import computeEdgeIndex
    from e3_layers_amd.data.synthetic import synth_qm9
    from e3_layers_amd.nn import PointwiseLinear
    from e3_layers_amd.run.sde_sampling import EulerMaruyamaPredictor, LangevinCorrector, NoneCorrector, get_pc_sampler
    from e3_layers_amd.run.sde_utils import VPSDE
    from e3_layers_amd.utils import build

    lc = featureModel(n_dim=8, l_max=1, edge_spherical="1x0e+1x1o", node_attrs="8x0e", edge_radial="8x0e",
                      num_types=10, num_layers=3, r_max=2.5)
    feats = "8x0e+8x0o+8x1e+8x1o"
    lc.layers = list(lc.layers) + [("score_output", {"module": PointwiseLinear, "irreps_in": (feats, "node_features"),
                                                     "irreps_out": ("1x1o", "score")})]
    torch.manual_seed(1)
    prod = build(lc).to(dev).eval()
    batch = synth_qm9(2, 5).to(dev)
    fixed = torch.randn(4096, 3, generator=torch.Generator().manual_seed(3)).to(dev)
    seen = []

    def preprocess(data, attrs):
        new, attrs = computeEdgeIndex(data, attrs, r_max=2.5)
        seen.append(int(new["edge_index"].shape[1]))
        return new, attrs

    def noise(shape):
        return fixed[:shape[0]]

    with pytest.raises(ValueError, match="static_edges"):
        get_pc_sampler(VPSDE({"pos": 3}, N=4), EulerMaruyamaPredictor, NoneCorrector, graph=True)
    eager = get_pc_sampler(VPSDE({"pos": 3}, N=4), EulerMaruyamaPredictor, NoneCorrector, preprocess=[preprocess])
    out_e, _ = eager(prod, batch.clone(), noise_fn=noise)
    assert len(seen) == 2 * 4 and len(set(seen)) > 1
    with pytest.raises(ValueError, match="r_max"):
        get_pc_sampler(VPSDE({"pos": 3}, N=4), EulerMaruyamaPredictor, NoneCorrector, graph=True, edge_capacity=4096)
    with pytest.raises(ValueError, match="NoneCorrector"):
        get_pc_sampler(VPSDE({"pos": 3}, N=4), EulerMaruyamaPredictor, LangevinCorrector, graph=True, edge_capacity=4096, r_max=2.5)
    capped = get_pc_sampler(VPSDE({"pos": 3}, N=4), EulerMaruyamaPredictor, NoneCorrector, graph=True, edge_capacity=4096, r_max=2.5)
    out_g, _ = capped(prod, batch.clone(), noise_fn=noise)
    assert torch.isfinite(out_e["pos"]).all()
    assert out_g["pos"].shape == out_e["pos"].shape
    assert rel_err(out_g["pos"], out_e["pos"]) < REPLAY
    assert out_g["edge_index"].shape[0] == 2 and out_g["edge_index"].shape[1] == seen[-1]      # the last rebuilt list, unpadded
