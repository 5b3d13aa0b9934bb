"""Host side of the replayed score step (run/score_step.py, run/sde_utils.sde_perturb_counter); no GPU.

* the torch restatement of the counter-based perturbation in float64 == an independent numpy float64 computation from pair_hash;
* the window protocol against stub steps (tests/score_stubs.py): the first overflowed step at the start, in the middle and at the end
  of a window, and a flush() on a partial window -- every step moves the weights exactly once, in order;
* capacity_for on planted list sizes."""
import math

import numpy as np
import pytest
import torch

from tests.score_stubs import StubSteps, captured_loss, eager_loss

SEED = (977 << 32) + 20241017      # both seed words in use


def _batch(sizes, ghost=0, dims=(("CA", 3),)):
    from e3_layers_amd.data import Batch

    gen = torch.Generator().manual_seed(4)
    attrs = {k: ("node", "1x1o" if d == 3 else f"{d}x0e") for k, d in dims}
    lst = [dict({k: torch.randn(n, d, generator=gen) for k, d in dims}, _n_nodes=torch.tensor([[n]])) for n in sizes + ((ghost,) if ghost else ())]
    b = Batch.from_data_list(lst, attrs)
    if ghost:
        b["_graph_weight"] = torch.tensor([[1.0 / len(sizes)]] * len(sizes) + [[0.0]])
    return b


@pytest.mark.parametrize("ghost,draw", [(0, 0), (19, 7), (0, (1 << 32) + 7)])
def test_float64_restatement_against_numpy_from_the_pair_hash(ghost, draw):
    from e3_layers_amd.data.compute_edge import pair_hash
    from e3_layers_amd.run.sde_utils import VPSDE, sde_perturb_counter

    sizes, dims = (5, 1, 70), (("CA", 3), ("C", 3), ("O", 1))
    b = _batch(sizes, ghost, dims)
    sde = VPSDE(dict(dims))
    eps = 1e-5
    pert, misc = sde_perturb_counter(sde, b, SEED, draw, eps, dtype=torch.float64)
    n_real, G = sum(sizes), len(sizes)
    seg = np.repeat(np.arange(G), sizes)

    def hashes(src, dst):
        return pair_hash(SEED, draw, torch.as_tensor(src, dtype=torch.int64), torch.as_tensor(dst, dtype=torch.int64)).numpy()

    f32 = np.float32
    u = (hashes(np.full(G, 0xFFFFFFFF), np.arange(G)) >> 8).astype(np.float64) * 2.0 ** -24
    span, q, h = float(f32(1.0) - f32(eps)), float(f32(-0.25) * (f32(20.0) - f32(0.1))), float(f32(-0.5) * f32(0.1))
    t = float(f32(eps)) + span * u
    lm = t * (q * t + h)
    a, s = np.exp(lm), np.sqrt(-np.expm1(2.0 * lm))
    assert np.array_equal(pert["t"].numpy()[:G, 0], t)
    assert np.array_equal(misc["std"].numpy()[:n_real, 0], s[seg])
    word0 = 0
    for key, d in dims:
        i, c = np.meshgrid(np.arange(n_real), np.arange(d), indexing="ij")
        u1 = ((hashes(i, 2 * (word0 + c)) >> 8) + 1).astype(np.float64) * 2.0 ** -24
        u2 = (hashes(i, 2 * (word0 + c) + 1) >> 8).astype(np.float64) * 2.0 ** -24
        z = np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * math.pi * u2)
        got_z, got_x = misc["zs"][key].numpy(), pert[key].numpy()
        assert np.abs(got_z[:n_real] - z).max() <= 1e-14 * 6.0
        want = a[seg][:, None] * b[key].numpy()[:n_real].astype(np.float64) + s[seg][:, None] * z
        assert np.abs(got_x[:n_real] - want).max() <= 1e-14 * np.abs(want).max()
        if ghost:      # the ghost graph's rows: the geometry as it was, no noise, std 1, t 0.5
            assert np.array_equal(got_x[n_real:], b[key].numpy()[n_real:].astype(np.float64)) and not got_z[n_real:].any()
        word0 += d
    if ghost:
        assert float(pert["t"][G]) == 0.5 and bool((misc["std"][n_real:] == 1.0).all())
    assert abs(float(misc["zs"]["CA"].std()) - 1.0) < 0.15
    again, _ = sde_perturb_counter(sde, b, SEED, draw, eps, dtype=torch.float64)
    assert torch.equal(again["CA"], pert["CA"])
    other, m2 = sde_perturb_counter(sde, b, SEED, draw + 1, eps, dtype=torch.float64)
    assert bool((m2["zs"]["CA"][:n_real] != misc["zs"]["CA"][:n_real]).all())
    if draw >> 32:      # the draw index is taken modulo 2^32, as in the kernels
        low, _ = sde_perturb_counter(sde, b, SEED, draw & 0xFFFFFFFF, eps, dtype=torch.float64)
        assert torch.equal(low["CA"], pert["CA"])


def test_the_fp32_restatement_follows_the_float64_one():
    from e3_layers_amd.run.sde_utils import VPSDE, sde_perturb_counter

    b = _batch((33, 4))
    sde = VPSDE({"CA": 3})
    p32, m32 = sde_perturb_counter(sde, b, 3, 5)
    p64, m64 = sde_perturb_counter(sde, b, 3, 5, dtype=torch.float64)
    assert p32["CA"].dtype == torch.float32
    assert float((p32["CA"].double() - p64["CA"]).abs().max()) < 2e-5
    assert float((m32["std"].double() - m64["std"]).abs().max()) < 1e-6


def _run(check_every, n_steps, bad, flush=True):
    from e3_layers_amd.run.score_step import StepWindow

    dev = StubSteps(check_every, bad)
    win = StepWindow(dev, check_every)
    batches = [s % 3 for s in range(n_steps)]      # three alternating batches
    for b in batches:
        win(b)
    if flush:
        win.flush()
    return dev, win, batches


@pytest.mark.parametrize("bad,first", [((4,), 4), ((5, 6), 5), ((7,), 7), ((4, 7), 4)])
def test_first_bad_at_the_start_the_middle_and_the_end_of_a_window(bad, first):
    dev, win, batches = _run(4, 12, bad)
    # every step moved the weights exactly once, in order; the steps from first_bad to the window's end eagerly
    assert [(s, b) for _, s, b in dev.applied] == list(enumerate(batches))
    assert [kind for kind, _, _ in dev.applied] == ["replay" if not first <= s < 8 else "redo" for s in range(12)]
    assert win.losses == [eager_loss(b, s) if first <= s < 8 else captured_loss(b, s) for s, b in enumerate(batches)]
    assert win.stats == dict(steps=12, windows=3, overflowed_windows=1, steps_redone=8 - first)
    assert dev.reads == 3 and dev.clears == 1 and dev.step == 12      # one read per window; the device step cell was not rewound


def test_no_overflow_drops_the_windows():
    dev, win, batches = _run(4, 8, ())
    assert [kind for kind, _, _ in dev.applied] == ["replay"] * 8 and dev.clears == 0
    assert win.stats == dict(steps=8, windows=2, overflowed_windows=0, steps_redone=0) and not win.pending


def test_flush_on_a_partial_window_and_two_overflowed_windows():
    dev, win, batches = _run(4, 6, (1, 5), flush=False)
    assert len(win.pending) == 2 and len(win.losses) == 4      # the first window was checked by the fourth call
    assert [(k, s) for k, s, _ in dev.applied] == [("replay", 0), ("redo", 1), ("redo", 2), ("redo", 3), ("replay", 4)]
    win.flush()
    assert [(k, s) for k, s, _ in dev.applied][5:] == [("redo", 5)] and not win.pending
    assert win.losses == [captured_loss(0, 0), eager_loss(1, 1), eager_loss(2, 2), eager_loss(0, 3), captured_loss(1, 4), eager_loss(2, 5)]
    assert win.stats == dict(steps=6, windows=2, overflowed_windows=2, steps_redone=4)
    win.flush()      # nothing pending: no read
    assert dev.reads == 2


def test_an_overflow_outside_the_window_is_an_error():
    from e3_layers_amd.run.score_step import StepWindow

    dev = StubSteps(4)
    win = StepWindow(dev, 4)
    win(0)
    dev.over, dev.first_bad = 1, 9
    with pytest.raises(RuntimeError, match="outside the window"):
        win.flush()


def test_capacity_for_on_planted_sizes():
    from e3_layers_amd.run.score_step import ReplayedScoreStep, quantile_capacity

    sizes = list(range(1, 101))                      # 1 .. 100
    assert quantile_capacity(sizes, 0.99, multiple=1) == 99
    assert quantile_capacity(sizes, 1.0, multiple=1) == 100
    assert quantile_capacity(sizes, 0.5, multiple=1) == 50
    assert quantile_capacity([1025], 0.99) == 2048 and quantile_capacity([1024], 0.99) == 1024
    assert quantile_capacity([5, 3000, 7], 0.5) == 1024
    with pytest.raises(ValueError):
        quantile_capacity([])
    step = object.__new__(ReplayedScoreStep)        # (no capture: the method under test only needs list_sizes)
    planted = {"a": [900, 1000, 30000, 950], "b": [41000, 26000, 25000, 25500]}
    seen = []

    def list_sizes(batch, draws):
        seen.append((batch, list(draws)))
        return planted[batch][:len(list(draws))]

    step.list_sizes = list_sizes
    assert step.capacity_for(["a", "b"], quantile=0.99, draws=4) == 41984      # the largest of eight, rounded up to 1024
    assert step.capacity_for(["a", "b"], quantile=0.75, draws=4) == 26624      # the sixth of eight: 26000
    assert seen[:2] == [("a", [0, 1, 2, 3]), ("b", [0, 1, 2, 3])]


def test_the_score_object_ships_its_three_kernels_and_the_optimiser_object_no_new_one(tmp_path):
    from tests.test_train_inventory import _shipped_kernels

    score = _shipped_kernels(tmp_path, "e3k_score.o") - {"zero_words_kernel"}      # (e3k_common.h's helper, instantiated in every object)
    assert score == {"vpsde_perturb_kernel", "denoise_loss_kernel", "score_step_record_kernel"}, sorted(score)
    optim = _shipped_kernels(tmp_path, "e3k_optim.o") - {"zero_words_kernel"}
    assert len(optim) == 7, sorted(optim)      # the veto is an argument of the existing ticks
