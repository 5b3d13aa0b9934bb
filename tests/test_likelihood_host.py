"""The log-likelihood through the probability-flow ODE on the CPU (run/likelihood.get_likelihood_fn): the float64 restatement that the
kernels e3k_sampler_probe / e3k_sampler_ode_div / e3k_sampler_prior_logp and the device loops are held to, against closed forms.

The whole module runs with float64 as torch's default dtype, with the batch builder of tests/test_sampler_seeded_host.py and the exact
Gaussian score of tests/test_ode_sampler_host.py (data N(0, sigma0^2 I): raw = s x (1 / v - 1), v = m^2 sigma0^2 + s^2).

Closed form, isotropic: d raw / d x = s (1 / v - 1) I, so a Rademacher probe's estimate eps J eps = s (1 / v - 1) |eps|^2 is the trace
itself -- no statistics enter -- and the exact answer is log N(x; 0, v(eps) I).

Closed form, non-symmetric: raw = s x A.  eps J eps per node is tr(A) + sum_{i<j} eps_i eps_j (A_ij + A_ji): for Rademacher probes its
variance is sum_{i<j} (A_ij + A_ji)^2 = 2 |offdiag(sym A)|_F^2, for Gaussian ones 2 |sym A|_F^2.  c(t) s(t) = beta(t) / 2 is linear in t,
so Heun's quadrature (the trapezoid rule) of it is exact: delta_logp_g = K sum_nodes eps J eps with K = integral of beta / 2."""
import math

import pytest
import torch

from tests.test_ode_sampler_host import EPS, GaussianScore, _lm, _var
from tests.test_sampler_seeded_host import Affine
from tests.test_sampler_seeded_host import _batch as _batch32

KEYS = {"pos": 3, "aux": 2}
SEED = (23 << 32) + 1234


@pytest.fixture(autouse=True)
def float64_default():
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    yield
    torch.set_default_dtype(old)


def _batch(sizes, keys=KEYS, ghost=0):
    """(the builder's fields come out in fp32: the data of these tests is float64)"""
    b = _batch32(sizes, keys, ghost=ghost)
    for k in keys:
        b.data[k] = b[k].double()
    return b


def _sde(keys=KEYS, **kw):
    from e3_layers_amd.run.sde_utils import VPSDE

    return VPSDE(keys, **kw)


def _exact_logp(batch, keys, v=None):
    """log N(x; 0, v I) per graph over the keys; v: v(eps)"""
    seg = batch.nodeSegment()
    v = _var(EPS) if v is None else v
    out = torch.zeros(len(batch))
    for k, d in keys.items():
        out.index_add_(0, seg, -0.5 * (batch[k] ** 2).sum(1) / v - 0.5 * d * math.log(2.0 * math.pi * v))
    return out


def test_closed_form_and_order_of_convergence():
    from e3_layers_amd.run.likelihood import bits_per_dim, get_likelihood_fn

    keys = {"pos": 3}
    batch = _batch((5, 7, 3), keys)
    batch["pos"] = batch["pos"] * math.sqrt(_var(EPS))      # (a draw of the density that is evaluated)
    sde = _sde(keys)
    exact = _exact_logp(batch, keys)
    latent_exact = batch["pos"] * math.sqrt(_var(1.0) / _var(EPS))
    # What the flow converges to is log N(x; 0, (v(eps) / v(T)) I): it takes N(0, I) for the density at T, which is N(0, v(T) I) with
    # v(T) = 1 - 0.75 exp(2 lm(T)) = 1 - 3.2e-5.  That prior mismatch, ~1e-4 nats here, belongs to the method (Song et al. 2021 make the
    # same substitution) and is the floor of the distance to log N(x; 0, v(eps) I): the order against the exact answer is shown at step
    # counts whose error stands two orders above it, and against the flow's own limit at the step counts of tests/test_ode_sampler_host.py.
    ratio = _var(EPS) / _var(1.0)
    limit = torch.zeros(3).index_add_(0, batch.nodeSegment(), -0.5 * (batch["pos"] ** 2).sum(1) / ratio - 1.5 * math.log(2.0 * math.pi * ratio))
    mismatch = float((limit - exact).abs().max())
    assert 0.0 < mismatch < 0.5 * 21 * 2.0 * (1.0 - _var(1.0))      # (n D / 2) |ln v(T)| and |x|^2 (1 - v(T)) / (2 v(eps)), each below this
    errs, lims, lat = {}, {}, {}
    for method in ("heun", "euler"):
        for n in (32, 64, 128, 256):
            model = GaussianScore(keys)
            logp, latent, info = get_likelihood_fn(sde, method, n_steps=n, eps=EPS, static_edges=True, seed=SEED)(model, batch)
            assert info["nfe"] == model.calls == n * (2 if method == "heun" else 1)
            assert model.modes and not any(model.modes)      # always eval
            assert logp.dtype == torch.float64 and logp.shape == (3,)
            assert torch.equal(logp, info["prior_logp"] + info["delta_logp"])
            assert info["dims"].tolist() == [15, 21, 9]
            errs[method, n] = float((logp - exact).abs().max())
            lims[method, n] = float((logp - limit).abs().max())
            lat[method, n] = float((latent["pos"] - latent_exact).norm() / latent_exact.norm())
            print("closed form", method, n, "logp error", errs[method, n], "to the flow's limit", lims[method, n], "latent error", lat[method, n])
    for a, b in ((32, 64), (64, 128)):
        assert errs["heun", b] > 10 * mismatch
        assert 3.5 <= errs["heun", a] / errs["heun", b] <= 4.5      # second order
        assert 1.7 <= errs["euler", a] / errs["euler", b] <= 2.3    # first order
    for a, b in ((64, 128), (128, 256)):
        assert 3.5 <= lims["heun", a] / lims["heun", b] <= 4.5
        assert 1.7 <= lims["euler", a] / lims["euler", b] <= 2.3
        assert 3.5 <= lat["heun", a] / lat["heun", b] <= 4.5
        assert 1.7 <= lat["euler", a] / lat["euler", b] <= 2.3
    assert errs["heun", 64] < 0.2 * errs["euler", 64]
    assert errs["heun", 256] < 1e-3 * float(exact.abs().min())
    # the Gaussian probe estimates the same trace with |eps|^2 in place of n D: not exact, and not the Rademacher number
    g, _, _ = get_likelihood_fn(sde, "heun", n_steps=64, eps=EPS, probe="gaussian", static_edges=True, seed=SEED)(GaussianScore(keys), batch)
    r, _, info = get_likelihood_fn(sde, "heun", n_steps=64, eps=EPS, static_edges=True, seed=SEED)(GaussianScore(keys), batch)
    assert (g - r).abs().min() > 1e-3
    # scale: the data's units per scaled unit
    for scale in (2.5, {"pos": 2.5}):
        shifted, _, info_s = get_likelihood_fn(sde, "heun", n_steps=64, eps=EPS, static_edges=True, seed=SEED, scale=scale)(GaussianScore(keys), batch)
        want = r - info["dims"].double() * math.log(2.5)
        assert (shifted - want).abs().max() <= 4 * 2.0 ** -52 * float(want.abs().max())
        assert torch.equal(info_s["delta_logp"], info["delta_logp"]) and torch.equal(info_s["prior_logp"], info["prior_logp"])
    bpd = bits_per_dim(r, info["dims"])
    assert torch.allclose(bpd, -r / (info["dims"] * math.log(2.0)), rtol=1e-15)


def test_two_keys_and_the_ghost_graph():
    from e3_layers_amd.run.likelihood import get_likelihood_fn

    plain, padded = _batch((5, 7, 3)), _batch((5, 7, 3), ghost=19)
    n = plain["pos"].shape[0]
    for k in KEYS:
        padded[k][:n] = plain[k]
    ghost_rows = {k: padded[k][n:].clone() for k in KEYS}
    sde = _sde()
    limit = _exact_logp(plain, KEYS, _var(EPS) / _var(1.0))      # what the flow converges to (the test above)
    for method, low, high in (("heun", 3.5, 4.5), ("euler", 1.7, 2.3)):
        half, _, _ = get_likelihood_fn(sde, method, n_steps=128, eps=EPS, static_edges=True, seed=SEED)(GaussianScore(KEYS), plain)
        fn = get_likelihood_fn(sde, method, n_steps=256, eps=EPS, static_edges=True, seed=SEED)
        a, lat_a, info_a = fn(GaussianScore(KEYS), plain)
        b, lat_b, info_b = fn(GaussianScore(KEYS), padded)
        assert info_a["dims"].tolist() == [25, 35, 15]
        assert a.shape == b.shape == (3,)                          # the ghost graph has no entry
        assert torch.equal(b, a)                                   # nothing batch-wide: it changes no real graph
        for k in KEYS:
            assert torch.equal(lat_b[k][:n], lat_a[k]) and torch.equal(lat_b[k][n:], ghost_rows[k])
            assert not any(name.startswith("probe") for name in lat_a.data)
        err, err_half = float((a - limit).abs().max()), float((half - limit).abs().max())
        print("two keys", method, err_half, err)
        assert low <= err_half / err <= high                       # both keys' terms are in: the sum converges at the method's order
        again, _, _ = fn(GaussianScore(KEYS), plain)
        assert torch.equal(again, a)
    assert torch.equal(plain["pos"], _batch((5, 7, 3))["pos"])     # the caller's batch is not touched


class Skew:
    """raw = s(t) x A with a fixed non-symmetric 3 x 3 matrix"""

    A = torch.tensor([[0.7, 0.9, -0.4], [-0.2, -0.3, 0.8], [0.5, 0.1, 0.6]], dtype=torch.float64)

    def train(self, mode=True):
        return self

    def __call__(self, batch):
        t = batch["t"].reshape(-1)[batch.nodeSegment()].reshape(-1, 1).double()
        s = torch.sqrt(-torch.expm1(2.0 * _lm(t)))
        batch.attrs["score_pos"] = batch.attrs["pos"]
        batch["score_pos"] = s * (batch["pos"].double() @ self.A)
        return batch


def _beta_integral(sde):
    return 0.5 * (sde.beta_0 * (sde.T - EPS) + 0.5 * (sde.beta_1 - sde.beta_0) * (sde.T ** 2 - EPS ** 2))


@pytest.mark.parametrize("probe", ["rademacher", "gaussian"])
def test_non_symmetric_jacobian_hutchinson_statistics(probe):
    from e3_layers_amd.run.likelihood import get_likelihood_fn

    keys = {"pos": 3}
    sizes = (5, 7, 3)
    batch = _batch(sizes, keys)
    sde = _sde(keys)
    a = Skew.A
    sym = 0.5 * (a + a.T)
    off = sym - torch.diag(torch.diag(sym))
    sigma_node = math.sqrt(2.0 * float(((off if probe == "rademacher" else sym) ** 2).sum()))
    k_int = _beta_integral(sde)
    n_probes = 64
    _, _, info = get_likelihood_fn(sde, "heun", n_steps=3, eps=EPS, probe=probe, n_probes=n_probes, static_edges=True, seed=SEED)(Skew(), batch)
    assert info["nfe"] == 6
    for g, n_g in enumerate(sizes):
        exact = k_int * n_g * float(torch.trace(a))
        cap = 5.0 * k_int * math.sqrt(n_g) * sigma_node / math.sqrt(n_probes)
        got = float(info["delta_logp"][g])
        print("hutchinson", probe, "graph", g, "mean", got, "exact", exact, "cap", cap)
        assert abs(got - exact) <= cap and got != exact


def test_probe_count_is_the_mean_of_the_single_probe_runs():
    from e3_layers_amd.run.likelihood import get_likelihood_fn

    keys = {"pos": 3}
    batch = _batch((5, 7, 3), keys)
    runs = []
    for n in (1000, 1001):      # one probe at draw index N + 1: 1001, then 1002
        _, _, info = get_likelihood_fn(_sde(keys, N=n), "heun", n_steps=4, eps=EPS, static_edges=True, seed=SEED)(Skew(), batch)
        runs.append(info["delta_logp"])
    model = Skew()
    _, lat2, both = get_likelihood_fn(_sde(keys, N=1000), "heun", n_steps=4, eps=EPS, n_probes=2, static_edges=True, seed=SEED)(model, batch)
    assert both["nfe"] == 8
    assert (runs[0] - runs[1]).abs().min() > 1e-3      # (two different probes)
    mean = 0.5 * (runs[0] + runs[1])
    assert ((both["delta_logp"] - mean).abs() <= 1e-12 * mean.abs()).all()


def test_draws():
    from e3_layers_amd.data.compute_edge import normal_draw, pair_hash, rademacher_draw

    n = 100_000
    word = torch.arange(n)
    r = rademacher_draw(SEED, 1001, 7, word, torch.float64)
    assert set(r.tolist()) == {-1.0, 1.0}
    assert torch.equal(r, torch.where((pair_hash(SEED, 1001, 7, 2 * word) >> 31) == 0, 1.0, -1.0))
    assert abs(float(r.mean())) <= 5.0 / math.sqrt(n)                # sigma of the mean of n signs: 1 / sqrt(n)
    z = normal_draw(SEED, 1001, 7, word, torch.float64)
    assert abs(float((r * z).mean())) <= 5.0 / math.sqrt(n)          # Var(r z) = Var(z) = 1
    nodes = rademacher_draw(SEED, 1001, torch.arange(n), 3, torch.float64)      # ... and along the nodes
    assert abs(float(nodes.mean())) <= 5.0 / math.sqrt(n)
    assert not torch.equal(rademacher_draw(SEED, 1002, 7, word), rademacher_draw(SEED, 1001, 7, word))
    assert rademacher_draw(SEED, 1001, 7, word).dtype == torch.float32


def test_probes_layout():
    from e3_layers_amd.data.compute_edge import normal_draw, rademacher_draw
    from e3_layers_amd.run.likelihood import make_probes

    batch = _batch((5, 7, 3), ghost=4)
    sde = _sde()
    node = torch.arange(19).reshape(-1, 1)
    for kind, draw in (("rademacher", rademacher_draw), ("gaussian", normal_draw)):
        probes = make_probes(sde, batch, SEED, kind, 2)
        assert set(probes) == {(0, "pos"), (0, "aux"), (1, "pos"), (1, "aux")}
        for (p, key), z in probes.items():
            word0 = 0 if key == "pos" else 3
            want = draw(SEED, sde.N + 1 + p, node, word0 + torch.arange(KEYS[key]).reshape(1, -1), torch.float64)
            assert torch.equal(z[:15], want[:15]) and (z[15:] == 0).all()


class OneWay(Affine):
    """the head of ``aux`` reads ``pos`` only: d raw_aux / d aux is structurally absent"""

    def __call__(self, batch):
        out = super().__call__(batch)
        out["score_aux"] = out["pos"][:, :2] * 1.0
        out["score_pos"] = out["pos"] * 2.0
        return out


class Constant(Affine):
    def __call__(self, batch):
        out = super().__call__(batch)
        out["score_pos"] = out["score_pos"].detach()
        return out


def test_refusals():
    from e3_layers_amd.run.likelihood import get_likelihood_fn

    sde = _sde()
    ok = dict(n_steps=4, seed=1)
    with pytest.raises(ValueError, match="method"):
        get_likelihood_fn(sde, "rk45", **ok)
    with pytest.raises(ValueError, match="probe"):
        get_likelihood_fn(sde, probe="sphere", **ok)
    with pytest.raises(ValueError, match="n_steps"):
        get_likelihood_fn(sde, n_steps=0, seed=1)
    with pytest.raises(ValueError, match="n_probes"):
        get_likelihood_fn(sde, n_probes=0, **ok)
    with pytest.raises(ValueError, match="64 bits"):
        get_likelihood_fn(sde, n_steps=4, seed=1 << 64)
    with pytest.raises(ValueError, match="64 bits"):
        get_likelihood_fn(sde, n_steps=4, seed=-1)
    with pytest.raises(TypeError):
        get_likelihood_fn(sde, n_steps=4)                                        # the seed has no default
    with pytest.raises(TypeError):
        get_likelihood_fn(sde, seed=1)                                           # nor has n_steps
    with pytest.raises(TypeError):
        get_likelihood_fn(sde, fixed="mask", **ok)                               # conditional likelihood is out of scope
    with pytest.raises(ValueError, match="scale"):
        get_likelihood_fn(sde, scale={"pos": 2.0}, **ok)                         # one number per key
    with pytest.raises(ValueError, match="scale"):
        get_likelihood_fn(sde, scale=0.0, **ok)
    with pytest.raises(ValueError, match="static_edges=True"):
        get_likelihood_fn(sde, graph=True, **ok)
    with pytest.raises(ValueError, match="r_max"):
        get_likelihood_fn(sde, graph=True, edge_capacity=1024, **ok)
    with pytest.raises(ValueError, match="cutoff graphs"):
        get_likelihood_fn(sde, graph=True, static_edges=True, edge_capacity=1024, r_max=0.3, **ok)
    with pytest.raises(ValueError, match="cutoff graphs"):
        get_likelihood_fn(sde, edge_capacity=1024, r_max=0.3, **ok)
    with pytest.raises(ValueError, match="PairCriterion"):
        get_likelihood_fn(sde, graph=True, edge_capacity=1024, r_max=0.3, criteria=lambda *a: None, **ok)
    get_likelihood_fn(sde, graph=True, edge_capacity=1024, r_max=0.3, **ok)      # served
    fn = get_likelihood_fn(sde, static_edges=True, **ok)
    fn(Affine(KEYS), _batch((4, 3)))                                             # served
    with pytest.raises(RuntimeError, match="None"):                              # a missing term is never integrated as zero
        fn(OneWay(KEYS), _batch((4, 3)))
    with pytest.raises(RuntimeError, match="differentiably"):
        fn(Constant(KEYS), _batch((4, 3)))


def test_the_accumulator_returns_to_zero_with_the_cells():
    """what every loop's ``rewind()`` does to the plan's own state (the replayed loops after their warm-up step), on a real loop: the
    accumulators of ``StepPlan.zero`` go back to zero with the cells and the neighbour-list builder's draw index -- here the host
    counter of the ``PairCriterion`` in the model's own ``edge_index`` layer, which the eager loop resets"""
    from functools import partial
    from types import SimpleNamespace

    from e3_layers_amd.data.compute_edge import PairCriterion
    from e3_layers_amd.run.loops import EagerLoop, StepPlan

    batch = _batch((3,), {"pos": 3})
    batch.attrs["t"] = ("graph", "1x0e")
    batch["t"] = torch.zeros(1, 1)
    crit = PairCriterion()
    crit.reset(7)      # (a counter that builds have advanced)
    model = SimpleNamespace(layers=[("edge_index", partial(lambda data, attrs, criteria=None: ({}, attrs), criteria=crit))])
    acc, cells = torch.ones(3), torch.tensor([2, 1])
    plan = StepPlan(batch, [lambda b: b], ["pos"], torch.linspace(1.0, 1e-3, 4), cells, zero=(acc,))
    loop = EagerLoop(plan, model, lambda b: b)
    loop.rewind()
    assert (acc == 0).all() and (cells == 0).all() and crit._draw == 0
    assert torch.equal(loop.result()["pos"], batch["pos"])


def test_parameters_are_frozen_for_the_run_and_restored():
    """no Parameter requires grad while the loop runs (the backward then walks only the routes to the diffused keys); afterwards,
    and after an exception, each is what it was"""
    from e3_layers_amd.run.likelihood import frozen_parameters, get_likelihood_fn

    class Net(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.lin, self.off, self.seen = torch.nn.Linear(3, 3), torch.nn.Linear(3, 3), []
            self.off.bias.requires_grad_(False)      # (frozen by its owner: stays so)

        def forward(self, batch):
            self.seen.append(any(p.requires_grad for p in self.parameters()))
            batch.attrs["score_pos"] = batch.attrs["pos"]
            batch["score_pos"] = self.lin(batch["pos"]) + self.off(batch["pos"])
            return batch

    keys = {"pos": 3}
    net = Net().double()
    before = [p.requires_grad for p in net.parameters()]
    _, _, info = get_likelihood_fn(_sde(keys), "heun", n_steps=2, static_edges=True, seed=SEED)(net, _batch((4, 3), keys))
    assert net.seen == [False] * 4 and info["nfe"] == 4 and (info["delta_logp"] != 0).all()
    assert [p.requires_grad for p in net.parameters()] == before and before.count(False) == 1
    with pytest.raises(KeyError):
        with frozen_parameters(net):
            raise KeyError("inside")
    assert [p.requires_grad for p in net.parameters()] == before
    with frozen_parameters(Skew()):      # a model without parameters
        pass
