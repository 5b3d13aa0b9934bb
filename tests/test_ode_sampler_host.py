"""The probability-flow ODE sampler on the CPU (run/sde_sampling.get_ode_sampler, run/sde_utils.ode_euler_step / ode_heun_finish): the
float64 restatement the kernels e3k_sampler_ode_euler / e3k_sampler_ode_heun are held to.

The whole module runs with float64 as torch's default dtype (the time grid and the prior take it), with the stub model and the batch
builder of tests/test_sampler_seeded_host.py.

The bound of the comparison with the textbook loop, 1e-9 relative, is that file's for the same kind of comparison: the sampler writes the
collapsed drift (0.5 beta) (raw / s) with s = sqrt(-expm1(2 lm)), the loop -0.5 beta (x + (-raw / std - x)) with std = sqrt(1 - exp(2 lm));
in float64 the stds differ by <= 1e-12 relative at t >= 1e-3, the cancelled x costs 2^-53 |x| / |raw / s|, and a handful of steps of a
map whose factor per step is 1 + O(h beta / s) amplify none of it beyond 1e2."""
import math
from types import SimpleNamespace

import pytest
import torch

from tests.test_sampler_seeded_host import Affine, _batch
from tests.util import rel_err

KEYS = {"pos": 3, "aux": 2}
SEED = (17 << 32) + 4242
EPS = 1e-3
SIGMA0_SQ = 0.25


@pytest.fixture(autouse=True)
def float64_default():
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    yield
    torch.set_default_dtype(old)


def _sde(keys=KEYS, **kw):
    from e3_layers_amd.run.sde_utils import VPSDE

    return VPSDE(keys, **kw)


def _lm(t, b0=0.1, b1=20.0):
    return -0.25 * t ** 2 * (b1 - b0) - 0.5 * t * b0


def _var(t):
    """v(t) = m(t)^2 sigma0^2 + s(t)^2 of data N(0, sigma0^2 I) under the VP-SDE"""
    lm = _lm(t)
    return math.exp(2.0 * lm) * SIGMA0_SQ - math.expm1(2.0 * lm)


class GaussianScore:
    """the exact score of data N(0, sigma0^2 I) as the head's raw output: score = -x / v, raw = -s (score + x) = s x (1 / v - 1)"""

    def __init__(self, keys):
        self.keys, self.calls, self.modes = keys, 0, []

    def train(self, mode=True):
        self.modes.append(mode)
        return self

    def __call__(self, batch):
        self.calls += 1
        t = batch["t"].reshape(-1)[batch.nodeSegment()].reshape(-1, 1).double()
        lm = _lm(t)
        s = torch.sqrt(-torch.expm1(2.0 * lm))
        v = torch.exp(2.0 * lm) * SIGMA0_SQ + s * s
        for k in self.keys:
            batch.attrs[f"score_{k}"] = batch.attrs[k]
            batch[f"score_{k}"] = s * batch[k].double() * (1.0 / v - 1.0)
        return batch


def _prior(sde, batch, seed=SEED):
    from e3_layers_amd.run.sde_utils import prior_sampling_counter

    return prior_sampling_counter(sde, batch.clone(), seed)


def test_closed_form_and_order_of_convergence():
    from e3_layers_amd.run.sde_sampling import get_ode_sampler

    keys = {"pos": 3}
    batch = _batch((5, 7, 3), keys)
    sde = _sde(keys)
    x_T = _prior(sde, batch)["pos"]
    exact = x_T * math.sqrt(_var(EPS) / _var(1.0))
    errs = {}
    for method in ("heun", "euler"):
        for n in (64, 128, 256):
            model = GaussianScore(keys)
            out, nfe = get_ode_sampler(sde, method=method, n_steps=n, eps=EPS, static_edges=True, seed=SEED)(model, batch)
            assert nfe == model.calls == n * (2 if method == "heun" else 1)
            errs[method, n] = float((out["pos"] - exact).norm() / x_T.norm())      # relative to x_T: the table's measure
            print("closed form", method, n, errs[method, n])
    # |x(eps) - exact| / |x_T| of the scalar linear problem, computed in float64 numpy beforehand (the problem is linear, so the figure
    # does not depend on x_T): a wrong h, beta or s misses them outright
    table = {("heun", 64): 3.30e-4, ("heun", 128): 8.41e-5, ("heun", 256): 2.12e-5,
             ("euler", 64): 3.33e-3, ("euler", 128): 1.72e-3, ("euler", 256): 8.76e-4}
    for case, want in table.items():
        assert abs(errs[case] / want - 1.0) < 0.01, (case, errs[case], want)
    for a, b in ((64, 128), (128, 256)):
        assert 3.5 <= errs["heun", a] / errs["heun", b] <= 4.5      # second order
        assert 1.7 <= errs["euler", a] / errs["euler", b] <= 2.3    # first order
    assert errs["heun", 64] < 0.2 * errs["euler", 64]


def _textbook_loop(sde, model, x, seg_t, method, n_steps, steps=None):
    """dx/dt = -0.5 beta (x + score), score = -raw / std - x, written out: float64, per key, the batch's t set per stage"""
    times = torch.linspace(sde.T, EPS, n_steps + 1, dtype=torch.float64)

    def drift(state, t):
        seg_t(state, t)
        raw = model(state)
        std = torch.sqrt(1.0 - torch.exp(2.0 * sde.log_mean_coeff(t)))
        beta = sde.beta_0 + t * (sde.beta_1 - sde.beta_0)
        return {k: -0.5 * beta * (state[k] + (-raw[f"score_{k}"] / std - state[k])) for k in sde.irreps}

    for i in range(n_steps if steps is None else steps):
        t0, t1 = times[i], times[i + 1]
        h = t1 - t0
        d1 = drift(x, t0)
        x0 = {k: x[k] for k in sde.irreps}
        for k in sde.irreps:
            x[k] = x0[k] + h * d1[k]
        if method == "heun":
            d2 = drift(x, t1)
            for k in sde.irreps:
                x[k] = x0[k] + 0.5 * h * (d1[k] + d2[k])
    return x


@pytest.mark.parametrize("method", ["heun", "euler"])
def test_restatement_against_an_independent_float64_loop(method):
    from e3_layers_amd.run.sde_sampling import get_ode_sampler

    batch = _batch((5, 7, 3))
    sde = _sde()
    n_steps = 8
    out, _ = get_ode_sampler(sde, method=method, n_steps=n_steps, eps=EPS, static_edges=True, seed=SEED)(Affine(KEYS), batch)

    def set_t(state, t):
        state["t"] = torch.full((len(state), 1), float(t))

    start = _prior(sde, batch)
    start.attrs["t"] = ("graph", "1x0e")
    ref = _textbook_loop(sde, Affine(KEYS), start, set_t, method, n_steps)
    for k in KEYS:
        assert out[k].dtype == torch.float64 and torch.isfinite(out[k]).all()
        err = rel_err(out[k], ref[k])
        print("ode vs textbook loop", method, k, err)
        assert err < 1e-9, (method, k, err)
        assert rel_err(out[k], _prior(sde, batch)[k]) > 1e-2      # (the run moved)


def test_prior():
    from e3_layers_amd.data.compute_edge import normal_draw
    from e3_layers_amd.run.sde_sampling import get_ode_sampler
    from e3_layers_amd.run.sde_utils import draw_words

    batch = _batch((5, 7, 3))
    n = batch["pos"].shape[0]
    sde = _sde()
    x_T = _prior(sde, batch)
    model = Affine(KEYS)
    start, nfe = get_ode_sampler(sde, n_steps=5, static_edges=True, seed=SEED, n_iter=0)(model, batch)
    assert nfe == 0 and model.calls == 0
    for k in KEYS:
        assert torch.equal(start[k], x_T[k])      # bit for bit: the x_T of a predictor-corrector run at this seed
    sampler = get_ode_sampler(sde, n_steps=5, static_edges=True, seed=SEED)
    out, _ = sampler(Affine(KEYS), batch)
    again, _ = sampler(Affine(KEYS), batch)
    other, _ = get_ode_sampler(sde, n_steps=5, static_edges=True, seed=SEED + 1)(Affine(KEYS), batch)
    assert all(torch.equal(again[k], out[k]) for k in KEYS)
    assert rel_err(other["pos"], out["pos"]) > 1e-3
    # unseeded, fed the same prior draws: one draw per key, nothing after
    words, _ = draw_words(sde)
    node = torch.arange(n).reshape(-1, 1)
    bank = [normal_draw(SEED, sde.N, node, words[k] + torch.arange(d).reshape(1, -1), torch.float64) for k, d in KEYS.items()]
    asked = []

    def noise_fn(shape):
        asked.append(tuple(shape))
        return bank[len(asked) - 1]

    fed, _ = get_ode_sampler(sde, n_steps=5, static_edges=True)(Affine(KEYS), batch, noise_fn=noise_fn)
    assert asked == [(n, d) for d in KEYS.values()]
    for k in KEYS:
        err = rel_err(fed[k], out[k])
        print("noise-fed vs seeded", k, err)
        assert err < 1e-12, (k, err)


@pytest.mark.parametrize("method", ["heun", "euler"])
def test_ghost_rows_stay_and_real_rows_do_not_see_them(method):
    from e3_layers_amd.run.sde_sampling import get_ode_sampler
    from e3_layers_amd.run.sde_utils import ode_euler_step, ode_heun_finish

    plain, padded = _batch((5, 7, 3)), _batch((5, 7, 3), ghost=19)
    n = plain["pos"].shape[0]
    for k in KEYS:
        padded[k][:n] = plain[k]
    ghost_rows = {k: padded[k][n:].clone() for k in KEYS}
    sde = _sde()
    sampler = get_ode_sampler(sde, method=method, n_steps=6, static_edges=True, seed=SEED)
    a, _ = sampler(Affine(KEYS), plain)
    b, _ = sampler(Affine(KEYS), padded)
    for k in KEYS:
        assert torch.equal(b[k][:n], a[k])                 # exactly: nothing batch-wide in the update
        assert torch.equal(b[k][n:], ghost_rows[k])        # bit for bit
        assert rel_err(a[k], plain[k]) > 1e-2
    # the steps themselves: d1 is zero on the ghost rows, an int names the step as the cells do, outside the table nothing moves
    times = torch.linspace(1.0, EPS, 7)
    x = padded.clone()
    x.attrs["t"] = ("graph", "1x0e")
    x["t"] = torch.full((len(x), 1), float(times[2]))
    y = x.clone()
    kept_x, kept_y = {}, {}
    x = ode_euler_step(sde, Affine(KEYS), x, times, torch.tensor([3, 2]), keep=kept_x)
    y = ode_euler_step(sde, Affine(KEYS), y, times, 2, keep=kept_y)
    assert (x["t"] == times[3]).all()                      # the ghost graph's time moves with the others
    for k in KEYS:
        assert torch.equal(x[k], y[k]) and torch.equal(kept_x[k][1], kept_y[k][1])
        assert (kept_x[k][1][n:] == 0).all() and (kept_x[k][1][:n] != 0).all()
        assert torch.equal(x[k][n:], ghost_rows[k])
    x = ode_heun_finish(sde, Affine(KEYS), x, kept_x, times, torch.tensor([3, 2]))
    for k in KEYS:
        assert torch.equal(x[k][n:], ghost_rows[k])
    for step in (-1, 6, 7):
        z = padded.clone()
        z.attrs["t"] = ("graph", "1x0e")
        z["t"] = torch.full((len(z), 1), 0.25)
        kept = {}
        z = ode_euler_step(sde, Affine(KEYS), z, times, step, keep=kept)
        assert (z["t"] == 0.25).all()
        for k in KEYS:
            assert torch.equal(z[k], padded[k]) and (kept[k][1] == 0).all()
        z = ode_heun_finish(sde, Affine(KEYS), z, kept, times, step)
        assert all(torch.equal(z[k], padded[k]) for k in KEYS)


def test_call_counts_and_eval_mode():
    from e3_layers_amd.run.sde_sampling import get_ode_sampler

    batch = _batch((5, 7, 3))
    sde = _sde()
    for method, per_step in (("euler", 1), ("heun", 2)):
        for n_steps, n_iter, ran in ((7, None, 7), (7, 3, 3), (7, 50, 7)):
            model = Affine(KEYS)
            out, nfe = get_ode_sampler(sde, method=method, n_steps=n_steps, static_edges=True, seed=SEED, n_iter=n_iter)(model, batch)
            assert nfe == per_step * ran and model.calls == per_step * ran, (method, n_steps, n_iter, nfe, model.calls)
            assert model.modes and not any(model.modes)      # always eval
            assert torch.isfinite(out["pos"]).all()
    # the grid is n_steps' own: sde.N only names the prior's draw index
    a, _ = get_ode_sampler(_sde(N=1000), n_steps=5, static_edges=True)(Affine(KEYS), batch, noise_fn=lambda s: torch.ones(s))
    b, _ = get_ode_sampler(_sde(N=10), n_steps=5, static_edges=True)(Affine(KEYS), batch, noise_fn=lambda s: torch.ones(s))
    assert torch.equal(a["pos"], b["pos"])


def test_refusals():
    from e3_layers_amd.run.sde_sampling import get_ode_sampler

    sde = _sde()
    with pytest.raises(ValueError, match="method"):
        get_ode_sampler(sde, method="rk45", n_steps=4)
    with pytest.raises(ValueError, match="n_steps"):
        get_ode_sampler(sde, n_steps=0)
    with pytest.raises(TypeError):
        get_ode_sampler(sde)                                                     # n_steps has no default
    with pytest.raises(TypeError):
        get_ode_sampler(sde, n_steps=4, fixed="mask")                            # conditional sampling is out of scope
    with pytest.raises(ValueError, match="static_edges=True"):
        get_ode_sampler(sde, n_steps=4, graph=True)
    with pytest.raises(ValueError, match="r_max"):
        get_ode_sampler(sde, n_steps=4, graph=True, edge_capacity=1024)
    with pytest.raises(ValueError, match="cutoff graphs"):
        get_ode_sampler(sde, n_steps=4, graph=True, static_edges=True, edge_capacity=1024, r_max=0.3)
    with pytest.raises(ValueError, match="cutoff graphs"):
        get_ode_sampler(sde, n_steps=4, edge_capacity=1024, r_max=0.3)           # edge_capacity without graph
    with pytest.raises(ValueError, match="PairCriterion"):
        get_ode_sampler(sde, n_steps=4, graph=True, edge_capacity=1024, r_max=0.3, criteria=lambda *a: None)
    get_ode_sampler(sde, n_steps=4, graph=True, edge_capacity=1024, r_max=0.3)   # served
    with pytest.raises(ValueError, match="64 bits"):
        get_ode_sampler(sde, n_steps=4, seed=1 << 64)
    sampler = get_ode_sampler(sde, n_steps=4, static_edges=True, seed=1)
    with pytest.raises(ValueError, match="generator"):
        sampler(Affine(KEYS), _batch((4,)), generator=torch.Generator())
    with pytest.raises(ValueError, match="noise_fn"):
        sampler(Affine(KEYS), _batch((4,)), noise_fn=lambda shape: torch.zeros(shape))


def test_get_sampling_fn():
    from e3_layers_amd.run import sde_sampling
    from e3_layers_amd.run.sde_sampling import get_ode_sampler, get_pc_sampler, get_sampling_fn

    batch = _batch((5, 7, 3))
    sde = _sde()

    def config(**sampling):
        return SimpleNamespace(sampling=SimpleNamespace(**sampling), training=SimpleNamespace(continuous=True))

    for cfg, method, per_step in ((config(method="ode", ode_steps=6), "heun", 2), (config(method="ODE", ode_steps=6, ode_method="Euler"), "euler", 1)):
        model = Affine(KEYS)
        out, nfe = get_sampling_fn(cfg, sde, None, EPS, static_edges=True, seed=SEED)(model, batch)
        want, _ = get_ode_sampler(sde, method=method, n_steps=6, eps=EPS, static_edges=True, seed=SEED)(Affine(KEYS), batch)
        assert nfe == 6 * per_step == model.calls
        assert all(torch.equal(out[k], want[k]) for k in KEYS)
    with pytest.raises(ValueError, match="ode_steps"):
        get_sampling_fn(config(method="ode"), sde, None, EPS)
    with pytest.raises(ValueError, match="unknown"):
        get_sampling_fn(config(method="ode", ode_steps=6, ode_method="rk45"), sde, None, EPS)
    with pytest.raises(ValueError, match="Sampler name ald unknown"):
        get_sampling_fn(config(method="ald"), sde, None, EPS)
    # "pc": what it built before
    pc_cfg = config(method="pc", predictor="euler_maruyama", corrector="langevin", snr=0.16, n_steps_each=1)
    sde4 = _sde(beta_max=2.0, N=4)
    got, nfe = get_sampling_fn(pc_cfg, sde4, None, EPS, static_edges=True, seed=SEED)(Affine(KEYS), batch)
    want, _ = get_pc_sampler(sde4, sde_sampling.EulerMaruyamaPredictor, sde_sampling.LangevinCorrector, static_edges=True, seed=SEED,
                             eps=EPS)(Affine(KEYS), batch)
    assert nfe == 8 and all(torch.equal(got[k], want[k]) for k in KEYS)
