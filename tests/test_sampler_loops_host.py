"""The loop interface of the samplers and the likelihood on the CPU (run/loops: StepPlan, EagerLoop; run/sde_sampling.pc_plan,
ode_plan; run/likelihood.likelihood_plan): a run may be split over several ``run()`` calls, ``rewind()`` puts everything back, the
loop of a plan is the public sampler's, and ``run()`` past the table does nothing.

Float64 throughout (torch's default dtype for the module), the affine stub model and the batch builder of
tests/test_sampler_seeded_host.py, the two-graph batch of tests/test_ode_sampler_host.py's served cases.  Every comparison is of
bits: the same float64 operations in the same order."""
import pytest
import torch

from tests.test_sampler_seeded_host import BETA_MAX, KEYS, Affine, _batch

SEED = (29 << 32) + 611
STEPS = 5
SIZES = (4, 3)


@pytest.fixture(autouse=True)
def float64_default():
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    yield
    torch.set_default_dtype(old)


def _sde():
    from e3_layers_amd.run.sde_utils import VPSDE

    return VPSDE(KEYS, beta_max=BETA_MAX, N=STEPS)      # (beta_max / N < 1: the Langevin step size stays real)


def _ones(shape):
    return torch.ones(shape)


def _pc_unseeded():
    from e3_layers_amd.run.sde_sampling import EulerMaruyamaPredictor, LangevinCorrector, get_pc_sampler, pc_plan

    sde, model, batch = _sde(), Affine(KEYS), _batch(SIZES)
    plan, _ = pc_plan(sde, EulerMaruyamaPredictor, LangevinCorrector, model, batch, noise_fn=_ones, static_edges=True)
    out, _ = get_pc_sampler(_sde(), EulerMaruyamaPredictor, LangevinCorrector, static_edges=True, n_iter=STEPS)(Affine(KEYS), batch,
                                                                                                              noise_fn=_ones)
    return plan, model, {k: out[k] for k in KEYS}


def _pc_seeded():
    from e3_layers_amd.run.sde_sampling import EulerMaruyamaPredictor, LangevinCorrector, get_pc_sampler, pc_plan

    sde, model, batch = _sde(), Affine(KEYS), _batch(SIZES)
    plan, _ = pc_plan(sde, EulerMaruyamaPredictor, LangevinCorrector, model, batch, static_edges=True, seed=SEED)
    out, _ = get_pc_sampler(_sde(), EulerMaruyamaPredictor, LangevinCorrector, static_edges=True, n_iter=STEPS, seed=SEED)(Affine(KEYS), batch)
    return plan, model, {k: out[k] for k in KEYS}


def _ode_heun():
    from e3_layers_amd.run.sde_sampling import get_ode_sampler, ode_plan

    sde, model, batch = _sde(), Affine(KEYS), _batch(SIZES)
    plan = ode_plan(sde, "heun", model, batch, n_steps=STEPS, static_edges=True, seed=SEED)
    out, _ = get_ode_sampler(_sde(), method="heun", n_steps=STEPS, static_edges=True, n_iter=STEPS, seed=SEED)(Affine(KEYS), batch)
    return plan, model, {k: out[k] for k in KEYS}


def _likelihood_heun():
    from e3_layers_amd.run.likelihood import get_likelihood_fn, likelihood_plan

    sde, model, batch = _sde(), Affine(KEYS), _batch(SIZES)
    plan, acc, _ = likelihood_plan(sde, "heun", model, batch, n_steps=STEPS, static_edges=True, seed=SEED)
    assert plan.zero[0] is acc
    _, latent, info = get_likelihood_fn(_sde(), "heun", n_steps=STEPS, static_edges=True, seed=SEED)(Affine(KEYS), batch)
    return plan, model, dict({k: latent[k] for k in KEYS}, acc=info["delta_logp"])


def _state(loop):
    """(copies of) what a run advanced: the moved tensors, the time, the cells and the accumulators"""
    out = loop.result()
    plan = loop.plan
    state = {k: out[k].clone() for k in plan.keys}
    state.update(t=out["t"].clone(), cells=plan.cells.clone())
    for i, acc in enumerate(plan.zero):
        state["acc" if i == 0 else f"acc{i}"] = acc.clone()
    return state


def _same(a, b, names=None):
    return all(torch.equal(a[k], b[k]) for k in (a if names is None else names))


@pytest.mark.parametrize("case", [_pc_unseeded, _pc_seeded, _ode_heun, _likelihood_heun])
def test_split_runs_rewinding_the_public_sampler_and_the_end_of_the_table(case):
    from e3_layers_amd.run.likelihood import frozen_parameters
    from e3_layers_amd.run.loops import EagerLoop, edge_plumbing, make_loop

    plan, model, public = case()
    assert plan.times.numel() == STEPS and plan.cells.dtype == torch.int64 and plan.cells.shape == (2,)
    assert plan.batch["t"].shape == (len(SIZES), 1)
    _, moved = edge_plumbing((), True)
    start = {k: plan.batch[k].clone() for k in plan.keys}
    with torch.no_grad(), frozen_parameters(model):
        loop = make_loop(plan, model, moved, graph=False, edge_capacity=None, r_max=None, criteria=None)
        assert isinstance(loop, EagerLoop)
        loop.rewind()
        loop.run(STEPS)
        whole = _state(loop)
        # rewound: the start state, the cells and every accumulator at zero
        loop.rewind()
        assert _same(loop.result(), start, plan.keys) and _same(plan.batch, start, plan.keys)
        assert (plan.cells == 0).all() and all((acc == 0).all() for acc in plan.zero)
        # the same run again: the same bits, which are the public sampler's
        loop.run(STEPS)
        again = _state(loop)
        assert _same(again, whole)
        assert plan.cells.tolist() == [STEPS, STEPS - 1]
        assert _same(again, public, public)
        assert any(not torch.equal(again[k], start[k]) for k in plan.keys)      # (the run moved)
        # ... and past the table nothing moves
        loop.run(1)
        loop.run(3)
        assert _same(_state(loop), whole)
        # split in two
        loop.rewind()
        loop.run(2)
        assert plan.cells.tolist() == [2, 1]
        part = _state(loop)
        assert any(not torch.equal(part[k], whole[k]) for k in plan.keys)
        loop.run(3)
        assert _same(_state(loop), whole)
        # a run that asks for more than is left stops at the end of the table
        loop.rewind()
        loop.run(2)
        loop.run(STEPS)
        assert _same(_state(loop), whole)
