"""The replayed loops of run/loops on the device -- ``StaticLoop`` (the static-edge fixture of tests/test_gpu_ode_sampler.py) and
``CappedLoop`` (the smallest protein set-up of tests/test_gpu_protein_sampler_replay.py) -- each on the seeded predictor-corrector
plan and on the ODE's Heun plan, 4 steps: the step is recorded by ``CapturedStep``, a run may be split over two ``run()`` calls, and
the loop of a plan gives what the public sampler gives.

Bounds.  A replayed loop against itself, split or whole, and against the public sampler on the same kind of loop: the capped replay
run twice at one seed is held to equal bits by tests/test_gpu_sampler_seeded.py and tests/test_gpu_ode_sampler.py, so equal bits are
asserted for it here; no test holds the static-edge graph to that, so it gets ``tests.test_gpu_md.REPLAY``, the bound those files
use for replay against eager -- which is also the bound against the public sampler's EAGER loop, for both."""
import pytest
import torch

from tests.test_gpu_md import REPLAY      # replay vs eager
from tests.test_gpu_ode_sampler import diffusion_pair      # noqa: F401  (the static-edge fixture)
from tests.test_gpu_protein_sampler_replay import STD, _model, _proteins
from tests.util import record_measured, rel_err

pytestmark = pytest.mark.gpu

SEED = 11
STEPS = 4


def _plan_and_samplers(kind, sde, model, batch, ode_steps, **loop_args):
    """(a fresh plan, the public sampler on the same loop, the public sampler on the eager loop) at ``n_iter = STEPS``"""
    from e3_layers_amd.run.sde_sampling import (EulerMaruyamaPredictor, LangevinCorrector, get_ode_sampler, get_pc_sampler, ode_plan,
                                                pc_plan)

    static = bool(loop_args.get("static_edges"))
    eager_args = {"static_edges": True} if static else {}
    if kind == "pc":
        plan, _ = pc_plan(sde(), EulerMaruyamaPredictor, LangevinCorrector, model, batch, static_edges=static, seed=SEED)
        make = lambda **kw: get_pc_sampler(sde(), EulerMaruyamaPredictor, LangevinCorrector, n_iter=STEPS, seed=SEED, **kw)      # noqa: E731
    else:
        plan = ode_plan(sde(), "heun", model, batch, n_steps=ode_steps, static_edges=static, seed=SEED)
        make = lambda **kw: get_ode_sampler(sde(), method="heun", n_steps=ode_steps, n_iter=STEPS, seed=SEED, **kw)      # noqa: E731
    return plan, make(**loop_args), make(**eager_args)


def _check(name, loop, plan, model, batch, same_loop, eager, bits):
    from e3_layers_amd.run.graph_step import CapturedStep

    key = plan.keys[0]
    assert isinstance(loop.step, CapturedStep)
    with torch.no_grad():
        loop.rewind()
        loop.run(2)
        assert plan.cells.tolist() == [2, 1]
        loop.run(2)
        split = loop.result()[key].clone()
        loop.rewind()
        assert plan.cells.tolist() == [0, 0]
        loop.run(STEPS)
        whole = loop.result()[key].clone()
        loop.run(1)      # past n_iter: inside the table the loop goes on, at its end it stands
        if plan.times.numel() > STEPS:
            assert plan.cells.tolist() == [STEPS + 1, STEPS]
        else:
            assert plan.cells.tolist() == [STEPS, STEPS - 1] and torch.equal(loop.result()[key], whole)
    assert loop.step.recaptures == 0
    assert torch.isfinite(whole).all()
    public, nfe = same_loop(model, batch.clone())
    assert nfe == 2 * STEPS
    out_e, _ = eager(model, batch.clone())
    diffs = {"split_vs_whole": rel_err(split, whole), "whole_vs_public_same_loop": rel_err(whole, public[key]),
             "whole_vs_public_eager": rel_err(whole, out_e[key])}
    print("sampler loops", name, diffs)
    record_measured("test_gpu_sampler_loops", case=name, **diffs)
    if bits:
        assert torch.equal(split, whole) and torch.equal(whole, public[key])
    assert diffs["split_vs_whole"] < REPLAY and diffs["whole_vs_public_same_loop"] < REPLAY, diffs
    assert diffs["whole_vs_public_eager"] < REPLAY, diffs
    assert rel_err(whole, plan.batch[key]) > 0.0      # (the run moved)


@pytest.mark.parametrize("kind", ["pc", "ode"])
def test_static_loop(dev, diffusion_pair, kind):      # noqa: F811
    from e3_layers_amd.run.loops import StaticLoop, edge_plumbing, make_loop
    from e3_layers_amd.run.sde_utils import VPSDE

    prod, _, batch, _ = diffusion_pair
    batch = batch.clone().to(dev)
    plan, same_loop, eager = _plan_and_samplers(kind, lambda: VPSDE({"pos": 3}, N=1000), prod, batch, 50, static_edges=True, graph=True)
    with torch.no_grad():
        loop = make_loop(plan, prod, edge_plumbing((), True)[1], graph=True, edge_capacity=None, r_max=None, criteria=None)
    assert isinstance(loop, StaticLoop)
    _check(f"static_{kind}", loop, plan, prod, batch, same_loop, eager, bits=False)


@pytest.fixture(scope="module")
def proteins(dev):
    """(model, batch, edge capacity): the CA score net of three layers on two small proteins; built once, left unchanged.  The
    capacity stands above the lists of these runs (around 950 edges), as ``max(seen) + 64`` does in the tests REPLAY is borrowed
    from: the padded sizes decide the model's host-side dispatch, and under a much larger ghost graph (8192) the capped replay and
    the eager loop no longer do the same arithmetic (5e-4 apart, measured, with or without these loops)."""
    return _model(dev, {"CA": 3}, num_layers=3), _proteins((70, 40)).to(dev), 2048


@pytest.mark.parametrize("kind", ["pc", "ode"])
def test_capped_loop(dev, proteins, kind):
    from e3_layers_amd.run.loops import CappedLoop, edge_plumbing, make_loop
    from e3_layers_amd.run.sde_utils import VPSDE

    model, batch, e_cap = proteins
    # the schedules whose replays tests/test_gpu_sampler_seeded.py and tests/test_gpu_ode_sampler.py hold to REPLAY against the eager loop:
    # VPSDE(N=4) with beta_max = 2 (the Langevin step size of a four-step schedule stays real), and a grid of four ODE steps
    sde = lambda: VPSDE({"CA": 3}, beta_max=2.0, N=4) if kind == "pc" else VPSDE({"CA": 3}, beta_max=2.0)      # noqa: E731
    capped = dict(graph=True, edge_capacity=e_cap, r_max=8.0 / STD)
    plan, same_loop, eager = _plan_and_samplers(kind, sde, model, batch, 4, **capped)
    with torch.no_grad():
        loop = make_loop(plan, model, edge_plumbing((), False)[1], criteria=None, **capped)
    assert isinstance(loop, CappedLoop) and loop.first_edges <= e_cap
    _check(f"capped_{kind}", loop, plan, model, batch, same_loop, eager, bits=True)
    assert loop.result()["CA"].shape == batch["CA"].shape      # unpadded


def test_unseeded_static_graph_draws_from_the_default_generator(dev, diffusion_pair):      # noqa: F811
    """the unseeded predictor-corrector plan on the static-edge graph: Euler-Maruyama, no corrector, no generator handed in -- the
    time comes from the step header as on every loop, and the noise from the default device generator inside the graph"""
    from e3_layers_amd.run.graph_step import CapturedStep
    from e3_layers_amd.run.loops import StaticLoop, edge_plumbing, make_loop
    from e3_layers_amd.run.sde_sampling import EulerMaruyamaPredictor, NoneCorrector, pc_plan
    from e3_layers_amd.run.sde_utils import VPSDE

    prod, _, batch, _ = diffusion_pair
    plan, _ = pc_plan(VPSDE({"pos": 3}, N=1000), EulerMaruyamaPredictor, NoneCorrector, prod, batch.clone().to(dev), static_edges=True)
    assert plan.times.dtype == torch.float32 and plan.batch["t"].dtype == torch.float32 and plan.cells.tolist() == [0, 0]
    with torch.no_grad():
        loop = make_loop(plan, prod, edge_plumbing((), True)[1], graph=True, edge_capacity=None, r_max=None, criteria=None)
        assert isinstance(loop, StaticLoop) and isinstance(loop.step, CapturedStep)
        loop.rewind()
        loop.run(STEPS)
        out = loop.result()
    assert plan.cells.tolist() == [STEPS, STEPS - 1] and loop.step.recaptures == 0
    assert torch.equal(out["t"], plan.times[STEPS - 1].expand_as(out["t"]))
    assert torch.isfinite(out["pos"]).all() and rel_err(out["pos"], plan.batch["pos"]) > 0.0
