"""The protein score nets' training step as replays of one HIP graph (run/score_step.ReplayedScoreStep) == the same steps taken eagerly
on the un-padded batches (eager_score_step), from equal initial weights, with the same counter-based draws.

The trees are those of tests/test_gpu_protein_sampler_replay.py (its docstring says why three layers, four for the backbone); the data
proteins of 70 and 40 residues; Adam with EMA 0.999 and clip 1.0; 12 steps over three alternating batches.

Bounds: per-step losses 1e-6 (relative), the flat gradient of step 0 1e-5, the parameter updates flat - start 2e-3, the EMA 1e-5 --
what tests/test_gpu_model.py holds the padded replay against the un-padded eager loop to for the other configurations.  The eager loop
runs TWICE: where two eager runs of this normalised net differ from each other by more than a quarter of one of these bounds, that
bound is replaced by 4 x the eager-to-eager spread (the kernels that accumulate with atomics make the eager loop itself that
uncertain; a replay cannot be asked to agree with it more closely than it agrees with itself).  Every figure is printed and goes to
the parity log (tests/util.record_measured; profiles/score_train_parity_measured.jsonl holds a run's)."""
import copy

import pytest
import torch

from tests.test_gpu_protein_sampler_replay import STD, _proteins
from tests.util import record_measured, rel_err

pytestmark = pytest.mark.gpu

SEED = (5 << 32) + 77
BOUNDS = dict(loss=1e-6, grad0=1e-5, update=2e-3, ema=1e-5)
ORDER = [0, 1, 2] * 4


def _tree(keys, num_layers, side_atoms=(), criteria="rule"):
    from e3_layers_amd.configs.config_dict import ConfigDict
    from e3_layers_amd.configs.config_diffusion_CA import pair_criterion, score_config

    data = ConfigDict()
    data.std = STD
    kw = {} if criteria == "callback" else dict(edge_criteria=pair_criterion(seed=5))
    return score_config(keys, data, l_max=1, num_layers=num_layers, n_dim=8, side_atoms=side_atoms, **kw)


def _make(dev, base, lr):
    from e3_layers_amd.run.optim import FusedAdamEMA
    from e3_layers_amd.run.parallel import flat_param_order

    model = copy.deepcopy(base)
    opt = FusedAdamEMA(flat_param_order(model), lr=lr, ema_decay=0.999, max_grad_norm=1.0)
    opt.grads.enable_direct_accumulation()
    return model, opt


def _eager_run(dev, base, lr, sde, batches, order):
    """the eager_step loop -> losses, list sizes, the flat gradient of step 0, start, final parameters and EMA"""
    from e3_layers_amd.run.score_step import eager_score_step

    model, opt = _make(dev, base, lr)
    out = dict(losses=[], sizes=[], start=opt.flat.detach().clone())
    try:
        for s, k in enumerate(order):
            loss, e = eager_score_step(model, sde, opt, batches[k], s, SEED)
            out["losses"].append(float(loss))
            out["sizes"].append(e)
            if s == 0:
                torch.cuda.synchronize()
                out["grad0"] = opt.grads.buffer.detach().clone()
        torch.cuda.synchronize()
        out.update(flat=opt.flat.detach().clone(), ema=opt.ema.detach().clone(), steps=opt.steps_taken, ema_updates=opt.ema_updates)
    finally:
        opt.grads.disable_direct_accumulation()
    return out


def _figures(got, ref):
    fig = dict(loss=max(abs(a - b) / abs(b) for a, b in zip(got["losses"], ref["losses"])),
               update=rel_err(got["flat"] - ref["start"], ref["flat"] - ref["start"]), ema=rel_err(got["ema"], ref["ema"]))
    if "grad0" in got:
        fig["grad0"] = rel_err(got["grad0"], ref["grad0"])
    return fig


_REFERENCES = {}


def _reference(dev, name):
    """Computed once per configuration and left unchanged: the base model, the batches, two eager runs, the bounds in force."""
    from e3_layers_amd.run.sde_utils import VPSDE
    from e3_layers_amd.utils import build

    if name in _REFERENCES:
        return _REFERENCES[name]
    if name == "CA":
        keys, cfg = {"CA": 3}, _tree({"CA": 3}, 3)
        batches = [_batch(k).to(dev) for k in range(3)]
        order = ORDER
    else:
        keys = {"CA": 3, "C": 3, "O": 3, "N": 3}
        cfg = _tree(keys, 4, side_atoms=("C", "N", "O"))      # (concat3 sits behind layer3)
        batches = [_proteins((40,), backbone=True).to(dev)]
        order = [0] * 6
    torch.manual_seed(2)
    base = build(cfg.model_config).to(dev).train()
    sde = VPSDE(keys)
    lr = float(cfg.learning_rate)
    ref = _eager_run(dev, base, lr, sde, batches, order)
    again = _eager_run(dev, base, lr, sde, batches, order)
    assert again["sizes"] == ref["sizes"]      # the lists are functions of the data and the draws alone
    spread = _figures(again, ref)
    bounds = {}
    for k, b in BOUNDS.items():
        # (the rule of the module docstring: an eager loop that disagrees with itself by more than a quarter of a bound widens it)
        bounds[k] = b if spread[k] <= 0.25 * b else 4.0 * spread[k]
        record_measured("test_gpu_score_train_replay", case=f"eager_to_eager_{name}", quantity=k, spread=spread[k], issue_bound=b, bound_in_force=bounds[k])
    print(f"score_train_replay {name}: eager-to-eager spread {spread}, bounds in force {bounds}, list sizes {ref['sizes']}")
    _REFERENCES[name] = dict(base=base, sde=sde, lr=lr, batches=batches, order=order, ref=ref, bounds=bounds, keys=keys)
    return _REFERENCES[name]


def _batch(k):
    """batch k of the three: two proteins of 70 and 40 residues of its own (tests/test_gpu_protein_sampler_replay._proteins' recipe)"""
    from e3_layers_amd.data import Batch
    from e3_layers_amd.data.synthetic import synth_protein

    parts = [synth_protein(10 + 2 * k + j, 1, n_res=n) for j, n in enumerate((70, 40))]
    b = Batch.from_data_list([p.get(0) for p in parts], dict(parts[0].attrs))
    b.attrs.pop("_n_edges", None)
    return b


def _replay_run(dev, R, e_cap, check_every=8, cls=None, grow_after=None, with_grad0=True):
    from e3_layers_amd.run.score_step import ReplayedScoreStep

    model, opt = _make(dev, R["base"], R["lr"])
    try:
        step = (cls or ReplayedScoreStep)(model, R["sde"], opt, R["batches"][0], edge_capacity=e_cap, seed=SEED, check_every=check_every)
        assert torch.equal(opt.flat, R["ref"]["start"]) and opt.steps_taken == 0      # the warm-up and the capture left no trace
        padded = [step.pad(b) for b in R["batches"]]
        out = {}
        for s, k in enumerate(R["order"]):
            if grow_after is not None and s == grow_after:
                step.grow()
                padded = [step.pad(b) for b in R["batches"]]
            step(padded[k])
            if s == 0 and with_grad0:
                torch.cuda.synchronize()
                out["grad0"] = opt.grads.buffer.detach().clone()
        out["losses"] = step.losses
        torch.cuda.synchronize()
        out.update(flat=opt.flat.detach().clone(), ema=opt.ema.detach().clone(), steps=opt.steps_taken, ema_updates=opt.ema_updates,
                   stats=step.stats, step=step)
    finally:
        opt.grads.disable_direct_accumulation()
    return out


def _assert_close(name, got, R, keys=("loss", "grad0", "update", "ema")):
    fig = _figures(got, R["ref"])
    print(f"score_train_replay {name}: replay against eager {fig}, bounds {R['bounds']}, stats {got['stats']}")
    for k, v in fig.items():
        record_measured("test_gpu_score_train_replay", case=name, quantity=k, error=v, bound=R["bounds"][k])
    for k in keys:
        if k in fig:
            assert fig[k] <= R["bounds"][k], (k, fig[k], R["bounds"][k])


def test_ample_capacity_replay_equals_the_eager_loop(dev):
    R = _reference(dev, "CA")
    sizes = R["ref"]["sizes"]
    assert len(set(sizes)) > 1, sizes      # the list changes with the draw
    got = _replay_run(dev, R, max(sizes) + 64)
    _assert_close("ample", got, R)
    assert got["stats"]["steps"] == 12 and got["stats"]["overflowed_windows"] == 0 and got["stats"]["steps_redone"] == 0
    assert got["stats"]["windows"] == 2      # 8 + a flushed 4
    assert got["steps"] == 12 and got["ema_updates"] == 12
    step = got["step"]
    assert step.n_cap % 32 == 0 and step.e_cap == max(sizes) + 64
    assert int(step.nlist_state[0]) == sizes[-1]      # the last capped list held the eager loop's last list


def test_tight_capacity_overflowed_steps_are_vetoed_and_redone(dev):
    from e3_layers_amd.run.score_step import ReplayedScoreStep

    R = _reference(dev, "CA")
    sizes = R["ref"]["sizes"]
    ranked = sorted(sizes, reverse=True)
    assert ranked[2] < ranked[1], sizes      # the precondition: the two largest lists stand apart
    e_cap = ranked[2]
    windows = [sizes[w:w + 4] for w in (0, 4, 8)]
    assert any(all(e <= e_cap for e in w) for w in windows), windows      # at least one window whose lists all fit
    over = [s for s, e in enumerate(sizes) if e > e_cap]
    assert len(over) >= 2
    got = _replay_run(dev, R, e_cap, check_every=4, with_grad0=0 not in over)
    st = got["stats"]
    bad_windows = {s // 4 for s in over}
    assert st["windows"] == 3 and st["overflowed_windows"] == len(bad_windows) and 1 <= st["overflowed_windows"] < 3
    assert st["steps_redone"] == sum(4 * (w + 1) - min(s for s in over if s // 4 == w) for w in bad_windows) >= 2
    _assert_close("tight", got, R)
    assert got["steps"] == 12 and got["ema_updates"] == 12

    class NoVeto(ReplayedScoreStep):      # opt.step() inside the capture: the truncated lists' steps are applied, then applied again
        use_veto = False

    bare = _replay_run(dev, R, e_cap, check_every=4, cls=NoVeto, with_grad0=False)
    fig = _figures(bare, R["ref"])
    print(f"score_train_replay tight without the veto: {fig}, steps taken {bare['steps']}")
    assert bare["stats"]["steps_redone"] == st["steps_redone"] and bare["steps"] == 12 + st["steps_redone"]
    assert fig["update"] > R["bounds"]["update"] and fig["ema"] > R["bounds"]["ema"], fig      # the veto is what protects the weights


def test_backbone_net_replays(dev):
    R = _reference(dev, "backbone")
    got = _replay_run(dev, R, max(R["ref"]["sizes"]) + 64)
    _assert_close("backbone", got, R)
    assert got["steps"] == 6 and got["ema_updates"] == 6 and got["stats"]["steps_redone"] == 0


def test_grow_recaptures_and_the_steps_go_on(dev):
    R = _reference(dev, "CA")
    sizes = R["ref"]["sizes"]
    got = _replay_run(dev, R, max(sizes) + 64, grow_after=6)
    _assert_close("grow", got, R)
    step = got["step"]
    assert got["stats"]["recaptures"] >= 1 and step.e_cap >= 1.25 * (max(sizes) + 64) and step.e_cap % 1024 == 0
    assert got["stats"]["windows"] == 2 and got["steps"] == 12      # grow() checked the six pending steps


def test_refusals(dev):
    from e3_layers_amd.run.score_step import ReplayedScoreStep
    from e3_layers_amd.utils import build

    R = _reference(dev, "CA")
    shipped = build(_tree({"CA": 3}, 3, criteria="callback").model_config).to(dev)      # the shipped callback
    model, opt = _make(dev, shipped, R["lr"])
    try:
        with pytest.raises(ValueError, match="PairCriterion"):
            ReplayedScoreStep(model, R["sde"], opt, R["batches"][0], edge_capacity=4096)
    finally:
        opt.grads.disable_direct_accumulation()
    model, opt = _make(dev, R["base"], R["lr"])
    try:
        step = ReplayedScoreStep(model, R["sde"], opt, R["batches"][0], edge_capacity=max(R["ref"]["sizes"]) + 64, node_capacity=128)
        assert step.n_cap == 128
        with pytest.raises(ValueError, match="does not fit"):
            step.pad(_proteins((120, 80)).to(dev))      # 200 nodes
        small = step.pad(_proteins((70, 40)).to(dev))
        assert small["CA"].shape[0] == 128 and small["edge_index"].shape == (2, step.e_cap)
        with pytest.raises(ValueError, match="another bucket"):
            step(ReplayedScoreStep.pad(_Bucket(step, 160), R["batches"][0]))      # padded for another node capacity
    finally:
        opt.grads.disable_direct_accumulation()


class _Bucket:
    """pad() of another bucket: the same edge capacity and key, another node capacity"""

    def __init__(self, step, n_cap):
        self.n_cap, self.e_cap, self.pos_key = n_cap, step.e_cap, step.pos_key
