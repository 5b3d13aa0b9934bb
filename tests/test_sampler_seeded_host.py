"""The seeded predictor-corrector sampler on the CPU (run/sde_sampling.get_pc_sampler(seed=...), run/sde_utils: prior_sampling_counter,
langevin_step_counter, reverse_step_counter): the float64 restatement the kernels of csrc/e3k_sampler.hip are held to.

The model is a stub: a float64 affine map of each diffused key, row by row (a ghost row cannot reach a real one through it).  The
whole module runs with float64 as torch's default dtype, so that the UNSEEDED sampler -- whose time, alphas table and prior take the
default dtype -- is float64 throughout and can be fed the seeded sampler's draws through ``noise_fn``.

The bound of the comparison, 1e-9 relative: the seeded form writes std = sqrt(-expm1(2 lm)), the unseeded one sqrt(1 - exp(2 lm)); in
float64 the two differ by at most 2^-53 / m relative with m = 1 - exp(2 lm) >= 1e-4 at t >= 1e-3, i.e. <= 1e-12; lm = t (q t + h) against
-t^2 (b1 - b0) / 4 - t b0 / 2 and the association of the products differ by a few float64 roundings per step; four steps of a
contracting map amplify none of it by more than 1 / std <= 1e2."""
import pytest
import torch

from tests.util import rel_err

KEYS = {"pos": 3, "aux": 2}
SEED = (31 << 32) + 977
# VPSDE(N=4) with the default beta_max = 20 has discrete betas up to 5: alphas = 1 - beta / N goes negative and the Langevin step size
# with it -- sqrt(2 step) is NaN in the reference's formula, seeded or not.  beta_max / N < 1 keeps the four-step schedule finite.
BETA_MAX = 2.0


@pytest.fixture(autouse=True)
def float64_default():
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    yield
    torch.set_default_dtype(old)


class Affine:
    """raw_key = x_key W_key + b_key (float64), under the head name ``score_{key}``"""

    def __init__(self, keys):
        g = torch.Generator().manual_seed(4)
        self.w = {k: 0.3 * torch.randn(d, d, generator=g, dtype=torch.float64) for k, d in keys.items()}
        self.b = {k: 0.1 * torch.randn(d, generator=g, dtype=torch.float64) for k, d in keys.items()}
        self.calls, self.modes = 0, []

    def train(self, mode=True):
        self.modes.append(mode)
        return self

    def __call__(self, batch):
        self.calls += 1
        for k in self.w:
            batch.attrs[f"score_{k}"] = batch.attrs[k]
            batch[f"score_{k}"] = batch[k].double() @ self.w[k] + self.b[k]
        return batch


def _batch(sizes, keys=KEYS, ghost=0, fill=None):
    from e3_layers_amd.data import Batch

    g = torch.Generator().manual_seed(9)
    attrs = {k: ("node", "1x1o" if d == 3 else f"{d}x0e") for k, d in keys.items()}
    sizes = tuple(sizes) + ((ghost,) if ghost else ())
    lst = [dict({k: torch.randn(m, d, generator=g, dtype=torch.float64) for k, d in keys.items()}, _n_nodes=torch.tensor([[m]])) for m in sizes]
    b = Batch.from_data_list(lst, attrs)
    b.data["edge_index"] = torch.zeros(2, 0, dtype=torch.int64)
    if ghost:
        n = len(sizes) - 1
        b["_graph_weight"] = torch.tensor([[1.0 / n]] * n + [[0.0]])
    return b


def _sde(keys=KEYS, N=4):
    from e3_layers_amd.run.sde_utils import VPSDE

    return VPSDE(keys, beta_max=BETA_MAX, N=N)


def _draw_bank(sde, n_nodes, steps):
    """the float64 draws in the order the unseeded loop asks for them: the prior per key, then per step the corrector's per key and
    the predictor's per key"""
    from e3_layers_amd.data.compute_edge import normal_draw
    from e3_layers_amd.run.sde_utils import draw_words

    words, total = draw_words(sde)
    node = torch.arange(n_nodes).reshape(-1, 1)

    def z(draw, offset, key):
        return normal_draw(SEED, draw, node, offset + words[key] + torch.arange(sde.irreps[key]).reshape(1, -1), torch.float64)

    bank = [z(sde.N, 0, k) for k in sde.irreps]
    for i in range(steps):
        bank += [z(i, 0, k) for k in sde.irreps] + [z(i, total, k) for k in sde.irreps]
    return bank


def test_seeded_float64_equals_the_unseeded_sampler_fed_the_same_draws():
    from e3_layers_amd.run.sde_sampling import EulerMaruyamaPredictor, LangevinCorrector, get_pc_sampler

    batch = _batch((5, 7, 3))
    n = batch["pos"].shape[0]
    sde = _sde()
    seeded = get_pc_sampler(sde, EulerMaruyamaPredictor, LangevinCorrector, static_edges=True, seed=SEED)
    model = Affine(KEYS)
    out_s, nfe = seeded(model, batch)
    assert nfe == 8 and model.calls == 8 and not any(model.modes)
    bank = iter(_draw_bank(sde, n, 4))
    plain = get_pc_sampler(_sde(), EulerMaruyamaPredictor, LangevinCorrector, static_edges=True)
    out_p, _ = plain(Affine(KEYS), batch, noise_fn=lambda shape: next(bank))
    assert next(bank, None) is None      # every draw was asked for, in this order
    for k in KEYS:
        assert out_s[k].dtype == torch.float64 and torch.isfinite(out_s[k]).all()
        err = rel_err(out_s[k], out_p[k])
        print("seeded vs noise-fed", k, err)
        assert err < 1e-9, (k, err)
    # the same seed again: the same bits; another seed: another trajectory
    again, _ = seeded(Affine(KEYS), batch)
    assert all(torch.equal(again[k], out_s[k]) for k in KEYS)
    other, _ = get_pc_sampler(_sde(), EulerMaruyamaPredictor, LangevinCorrector, static_edges=True, seed=SEED + 1)(Affine(KEYS), batch)
    assert rel_err(other["pos"], out_s["pos"]) > 1e-3
    # predictor only, corrector only: the None classes draw nothing and call no model
    from e3_layers_amd.run.sde_sampling import NoneCorrector, NonePredictor

    for pred, corr, calls in ((EulerMaruyamaPredictor, NoneCorrector, 4), (NonePredictor, LangevinCorrector, 4), (NonePredictor, NoneCorrector, 0)):
        m = Affine(KEYS)
        out, _ = get_pc_sampler(_sde(), pred, corr, static_edges=True, seed=SEED)(m, batch)
        assert m.calls == calls and torch.isfinite(out["pos"]).all()


def test_corrector_predictor_steps_and_keys_draw_apart():
    from e3_layers_amd.run.sde_utils import draw_words

    sde = _sde()
    words, total = draw_words(sde)
    assert words == {"pos": 0, "aux": 3} and total == 5
    bank = _draw_bank(sde, 200, 2)
    prior, (c0, p0), (c1, p1) = bank[:2], (bank[2:4], bank[4:6]), (bank[6:8], bank[8:10])
    for a, b in ((c0, p0), (c0, c1), (p0, p1), (prior, c0), (prior, p1)):
        for x, y in zip(a, b):
            assert (x != y).all()
    # the second key's words are not the first's: aux's two components against pos's first two, and against each other's columns
    assert (c0[1] != c0[0][:, :2]).all() and (p0[1] != p0[0][:, :2]).all()
    # ... and the predictor's words of `pos` (5, 6, 7) are not the corrector's of `aux` (3, 4)
    assert (p0[0][:, :2] != c0[1]).all()


def test_ghost_rows_stay_and_real_rows_do_not_see_them():
    from e3_layers_amd.run.sde_sampling import EulerMaruyamaPredictor, LangevinCorrector, get_pc_sampler
    from e3_layers_amd.run.sde_utils import (langevin_step_counter, prior_sampling_counter, reverse_step_counter, sampler_begin_step)

    plain, padded = _batch((5, 7, 3)), _batch((5, 7, 3), ghost=19)
    n = plain["pos"].shape[0]
    for k in KEYS:      # the same real rows (the generator ran on): plant them
        padded[k][:n] = plain[k]
    ghost_rows = {k: padded[k][n:].clone() for k in KEYS}
    sde = _sde()
    times = torch.linspace(1.0, 1e-3, sde.N)
    outs = []
    for b in (plain, padded):
        b = b.clone()
        b.attrs["t"] = ("graph", "1x0e")
        b["t"] = torch.zeros(len(b), 1)
        cells = torch.zeros(2, dtype=torch.int64)
        b = prior_sampling_counter(sde, b, SEED)
        for _ in range(3):
            sampler_begin_step(times, cells, b["t"])
            b = langevin_step_counter(sde, Affine(KEYS), b, SEED, cells, 0.16)
            b = reverse_step_counter(sde, Affine(KEYS), b, SEED, cells)
        assert cells.tolist() == [3, 2] and (b["t"] == times[2]).all()      # the ghost graph's time moves with the others
        outs.append(b)
    for k in KEYS:
        assert torch.equal(outs[1][k][:n], outs[0][k])                       # exactly: the ghost rows enter no norm
        assert torch.equal(outs[1][k][n:], ghost_rows[k])                    # bit for bit
    # the same through the sampler (its prior included)
    sampler = get_pc_sampler(sde, EulerMaruyamaPredictor, LangevinCorrector, static_edges=True, seed=SEED)
    a, _ = sampler(Affine(KEYS), plain)
    b, _ = sampler(Affine(KEYS), padded)
    for k in KEYS:
        assert torch.equal(b[k][:n], a[k]) and torch.equal(b[k][n:], ghost_rows[k])
    # an int as the draw is the step number; beyond the table begin_step moves nothing
    x = prior_sampling_counter(sde, plain.clone(), SEED)
    x.attrs["t"] = ("graph", "1x0e")
    x["t"] = torch.full((3, 1), 0.5)
    y = x.clone()
    cells = torch.tensor([8, 7])
    x = reverse_step_counter(sde, Affine(KEYS), x, SEED, cells)
    y = reverse_step_counter(sde, Affine(KEYS), y, SEED, 7)
    assert torch.equal(x["pos"], y["pos"])
    t = torch.full((3, 1), 0.25)
    sampler_begin_step(times, cells, t)
    assert cells.tolist() == [8, 7] and (t == 0.25).all()


def test_refusals():
    from e3_layers_amd.run.sde_sampling import (EulerMaruyamaPredictor, LangevinCorrector, NoneCorrector, Predictor, Corrector,
                                                get_pc_sampler)

    class MyPredictor(EulerMaruyamaPredictor):
        pass

    class MyCorrector(Corrector):
        pass

    sde = _sde()
    with pytest.raises(ValueError, match="built-in"):
        get_pc_sampler(sde, MyPredictor, LangevinCorrector, seed=1)
    with pytest.raises(ValueError, match="built-in"):
        get_pc_sampler(sde, EulerMaruyamaPredictor, MyCorrector, seed=1)
    assert issubclass(MyPredictor, Predictor)
    get_pc_sampler(sde, MyPredictor, MyCorrector)                                # without a seed any class is taken, as before
    sampler = get_pc_sampler(sde, EulerMaruyamaPredictor, LangevinCorrector, static_edges=True, seed=1)
    with pytest.raises(ValueError, match="generator"):
        sampler(Affine(KEYS), _batch((4,)), generator=torch.Generator())
    with pytest.raises(ValueError, match="noise_fn"):
        sampler(Affine(KEYS), _batch((4,)), noise_fn=lambda shape: torch.zeros(shape))
    capped = dict(graph=True, edge_capacity=1024, r_max=0.3)
    with pytest.raises(ValueError, match="n_steps"):
        get_pc_sampler(sde, EulerMaruyamaPredictor, LangevinCorrector, n_steps=2, seed=1, **capped)
    get_pc_sampler(sde, EulerMaruyamaPredictor, LangevinCorrector, seed=1, **capped)      # served with a seed
    with pytest.raises(ValueError) as info:
        get_pc_sampler(sde, EulerMaruyamaPredictor, LangevinCorrector, **capped)          # ... and refused without, word for word
    assert str(info.value) == ("edge_capacity: the ghost graph's nodes would enter the corrector's batch-wide norms; only NoneCorrector "
                               "is served")
    with pytest.raises(ValueError, match="only NoneCorrector is served"):
        get_pc_sampler(sde, EulerMaruyamaPredictor, MyCorrector, **capped)
    get_pc_sampler(sde, EulerMaruyamaPredictor, NoneCorrector, **capped)
    with pytest.raises(ValueError, match="64 bits"):
        get_pc_sampler(sde, EulerMaruyamaPredictor, NoneCorrector, seed=1 << 64)
