"""The Langevin thermostat, ``thermalize`` and the FIRE minimiser of run/md.py on their torch paths (no GPU): the counter-based
normal draws (``data/compute_edge.normal_draw``, whose hashes are the kernel's bit for bit), equipartition, the redo of a rolled-back
chunk with the same noise, gamma = 0 against velocity Verlet, and FIRE with per-graph state on a stub potential."""
import math

import pytest
import torch

from tests.md_stubs import SIZES, WellField, equipartition_ratio, harmonic_oscillators, quartic_wells
from tests.test_nlist_host import _StubField

KT, GAMMA, DT = 0.7, 1.0, 0.05
FIRE_CAP = 250                    # iterations; the float64 run must need at most half of it (measured: 99)
FIRE_KW = dict(ftol=1e-3, dt=0.05, dt_max=0.5, maxstep=0.2)


@pytest.mark.parametrize("seed", [0, 1, 2024, (1 << 60) + 12345])
def test_normal_draws_have_the_moments_and_no_correlations(seed):
    """4 draws x 65 536 nodes x 3 words.  Each statistic is a mean of n independent terms of known variance under the hypothesis
    (xi: 1; xi^2 - 1: 2; xi^4 - 3: 105 - 9 = 96; a product of two independent draws: 1): it must lie within 5 sigma of its
    sampling error.  The 24-bit grid of u1 cuts the tail at |xi| = sqrt(48 ln 2) = 5.77: a bias far below these errors."""
    from e3_layers_amd.data.compute_edge import normal_draw

    draw = torch.arange(4)[:, None, None]
    node = torch.arange(65536)[None, :, None]
    word = torch.arange(3)[None, None, :]
    xi = normal_draw(seed, draw, node, word, torch.float64)
    assert xi.shape == (4, 65536, 3) and float(xi.abs().max()) <= math.sqrt(48 * math.log(2))
    stats = {"mean": (xi, 1.0), "variance": (xi ** 2 - 1, 2.0), "fourth": (xi ** 4 - 3, 96.0), "xy": (xi[..., 0] * xi[..., 1], 1.0),
             "yz": (xi[..., 1] * xi[..., 2], 1.0), "step_to_step": (xi[:-1] * xi[1:], 1.0), "neighbour_nodes": (xi[:, :-1] * xi[:, 1:], 1.0)}
    for name, (terms, var) in stats.items():
        z = float(terms.mean()) / math.sqrt(var / terms.numel())
        print(f"normal_draw seed {seed}: {name} {z:+.2f} sigma, max |xi| {float(xi.abs().max()):.2f}")
        assert abs(z) <= 5.0, (name, z)
    # the same arguments give the same bits; the thermalize words are another stream; the float32 form is the float64 one rounded
    assert torch.equal(normal_draw(seed, draw, node, word, torch.float64), xi)
    other = normal_draw(seed, draw, node, word + 4, torch.float64)
    assert not bool((other == xi).any())
    z = float((other * xi).mean()) * math.sqrt(xi.numel())
    assert abs(z) <= 5.0, z
    assert float((normal_draw(seed, draw, node, word, torch.float32).double() - xi).abs().max()) < 2e-5


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_langevin_reaches_equipartition(dtype):
    """256 independent 3-d harmonic oscillators, k in [0.5, 2], m in [0.5, 4], kT = 0.7, gamma = 1, dt = 0.05, from x = v = 0:
    2 <KE> / (3 N kT) over 1 600 steps after 400 is 1 within 0.03 (5 sigma of the spread over seeds, 0.006, which is what the
    number of independent samples gives: 768 components x 1 600 dt gamma / 2 decorrelation times)."""
    from e3_layers_amd.run.md import Langevin

    ff, mass = harmonic_oscillators(dtype=dtype)
    ratio = equipartition_ratio(Langevin(ff, mass, DT, KT, GAMMA, seed=0), KT)
    print("equipartition", dtype, ratio)
    assert abs(ratio - 1.0) <= 0.03, ratio


def _langevin_on_stub(fail_at=None, check_every=4, gamma=GAMMA, cls=None):
    from e3_layers_amd.run.md import Langevin, VelocityVerlet

    ff = _StubField(fail_at=fail_at)
    mass = torch.linspace(1.0, 3.0, 6, dtype=torch.float64)
    md = VelocityVerlet(ff, mass, dt=0.05) if cls == "nve" else Langevin(ff, mass, 0.05, KT, gamma, seed=11)
    md.v.copy_(torch.randn(6, 3, generator=torch.Generator().manual_seed(9), dtype=torch.float64))
    out = md.run(12, check_every=check_every)
    return ff, md, out


@pytest.mark.parametrize("fail_at", [2, 6, 9])
def test_a_redone_chunk_sees_the_same_noise(fail_at):
    ff0, md0, out0 = _langevin_on_stub()
    ff1, md1, out1 = _langevin_on_stub(fail_at)
    assert md0.restores == 0 and md1.restores == 1 and md1.regrowths == 1 and ff1.grown == 1
    assert md1.steps_done == md0.steps_done == 12
    assert torch.isfinite(out1["potential"]).all()
    for key in ("potential", "kinetic"):
        assert torch.equal(out1[key], out0[key]), key
    assert torch.equal(md1.x, md0.x) and torch.equal(md1.v, md0.v)
    # and the noise is there: the thermostatted run is not the NVE run
    _, nve, _ = _langevin_on_stub(cls="nve")
    assert not torch.equal(nve.v, md0.v)


def test_a_trajectory_does_not_depend_on_check_every():
    _, md3, out3 = _langevin_on_stub(check_every=3)
    _, md50, out50 = _langevin_on_stub(check_every=50)
    assert torch.equal(md3.x, md50.x) and torch.equal(md3.v, md50.v)
    assert torch.equal(out3["kinetic"], out50["kinetic"]) and torch.equal(out3["potential"], out50["potential"])
    # a second run() goes on with the step numbers, not from draw 0: twelve more steps are not the first twelve again
    again = md3.run(12, check_every=3)
    assert md3.steps_done == 24 and not torch.equal(again["kinetic"], out3["kinetic"])


def test_gamma_zero_is_velocity_verlet_bit_for_bit():
    _, lan, out_l = _langevin_on_stub(gamma=0.0)
    _, nve, out_n = _langevin_on_stub(cls="nve")
    assert lan.c == 1.0 and lan.s == 0.0
    assert torch.equal(lan.x, nve.x) and torch.equal(lan.v, nve.v)
    assert torch.equal(out_l["kinetic"], out_n["kinetic"]) and torch.equal(out_l["potential"], out_n["potential"])


def test_thermalize_draws_maxwell_boltzmann_velocities_from_its_own_stream():
    from e3_layers_amd.data.compute_edge import normal_draw
    from e3_layers_amd.run.md import Langevin, VelocityVerlet

    ff, mass = harmonic_oscillators(n=4096)
    md = Langevin(ff, mass, DT, KT, GAMMA, seed=5)
    md.thermalize()
    node = torch.arange(4096)[:, None]
    want = torch.sqrt(KT / mass)[:, None] * normal_draw(5, 0, node, 4 + torch.arange(3)[None, :], torch.float64)
    assert torch.allclose(md.v, want, rtol=1e-14, atol=0)
    ratio = float((mass[:, None] * md.v ** 2).sum()) / (3 * 4096 * KT)
    assert abs(ratio - 1.0) <= 5 * math.sqrt(2.0 / (3 * 4096)), ratio
    first = md.v.clone()
    md.thermalize(2 * KT)                                             # the counter went on: new velocities, at the kT given
    assert md.thermalizations == 2 and not bool((md.v == first).any())
    nve = VelocityVerlet(ff, mass, DT, seed=5)
    with pytest.raises(ValueError):
        nve.thermalize()                                              # no thermostat to take kT from
    nve.thermalize(KT)
    assert torch.equal(nve.v, first)


def _relax(ff, step_by_step=False):
    """FIRE to convergence: the driver, the result, and (step by step) the iteration at which every graph froze with its
    positions then."""
    from e3_layers_amd.run.md import Fire

    fire = Fire(ff, **FIRE_KW)
    if not step_by_step:
        return fire, fire.run(FIRE_CAP, check_every=7), None
    frozen = {}
    for it in range(FIRE_CAP):
        out = fire.run(1, check_every=1)
        for g in range(len(ff.bounds) - 1):
            a, b = ff.bounds[g], ff.bounds[g + 1]
            if g in frozen:
                assert torch.equal(fire.x[a:b], frozen[g][1]), (g, it)      # a frozen graph never moves again
            elif bool(out["converged"][g]):
                frozen[g] = (it, fire.x[a:b].clone())
        if bool(out["converged"].all()):
            break
    return fire, out, frozen


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_fire_relaxes_every_graph_at_its_own_pace(dtype):
    """Per-graph stiffness 0.3 .. 12: the graphs converge at different iterations (measured with the P >= 0 rule, float64 and
    float32 alike: 38 / 85 / 0 / 70 / 98 / 76), the empty graph at once, all within half the cap."""
    ff = quartic_wells(dtype=dtype)
    fire, out, frozen = _relax(ff, step_by_step=True)
    assert bool(out["converged"].all()) and len(frozen) == len(SIZES)
    at = [frozen[g][0] for g in range(len(SIZES))]
    print("fire converged at", dtype, at)
    assert max(at) + 1 <= FIRE_CAP // 2, at
    assert at[SIZES.index(0)] == 0 and len(set(at)) >= 4, at
    d = (fire.x - ff.sites).abs().max()
    assert float(d) < 1e-2                                             # at the sites: |f| < 1e-3 with k >= 0.15
    # the chunked run ends on the same bits, stops at the first check after the last graph froze, and its records say so
    fire7, out7, _ = _relax(quartic_wells(dtype=dtype))
    assert torch.equal(fire7.x, fire.x) and torch.equal(fire7.state, fire.state)
    assert out7["iterations"] == -(-(max(at) + 1) // 7) * 7 and out7["fmax"].shape == (out7["iterations"], len(SIZES))
    for g, it in enumerate(at):
        assert bool((out7["fmax"][it:, g] < FIRE_KW["ftol"]).all()) and bool((out7["fmax"][:it, g] >= FIRE_KW["ftol"]).all())
        assert float(out7["energy"][-1, g]) <= float(out7["energy"][0, g])


def test_fire_on_a_batch_equals_fire_on_each_graph_alone():
    fire, out, _ = _relax(quartic_wells())
    for g in range(len(SIZES)):
        one = quartic_wells(only=g)
        fire1, out1, _ = _relax(one)
        a, b = fire.ff.bounds[g], fire.ff.bounds[g + 1]
        n = out1["iterations"]
        assert n <= out["iterations"]
        assert torch.equal(fire.x[a:b], fire1.x), g
        assert torch.equal(out["fmax"][:n, g], out1["fmax"][:, 0]) and torch.equal(out["energy"][:n, g], out1["energy"][:, 0])
        assert torch.equal(fire.state[g, :3], fire1.state[0, :3])


@pytest.mark.parametrize("fail_at", [3, 30])
def test_fire_redoes_an_overflowed_chunk(fail_at):
    fire0, out0, _ = _relax(quartic_wells())
    fire1, out1, _ = _relax(quartic_wells(fail_at=fail_at))
    assert fire1.restores == 1 and fire1.regrowths == 1 and fire0.restores == 0
    assert torch.equal(fire1.x, fire0.x) and torch.equal(fire1.state, fire0.state)
    assert torch.equal(out1["fmax"], out0["fmax"]) and torch.equal(out1["energy"], out0["energy"])


def test_fire_step_host_path_is_the_rule_of_the_header():
    """The torch path of ``_fire_step`` (what the stub-field tests and the oracle loops run) in float64 on the planted state of the
    kernel's test -- every branch in one call -- against that test's restatement of the contract."""
    import numpy as np

    from e3_layers_amd.run.md import _fire_step
    from tests.test_gpu_md_integrator_kernels import FIRE, _fire_float64, _fire_plant

    n, x, v, f, node_ptr, state, names = _fire_plant(0)
    x64, v64, state64, _ = _fire_float64(n, x, v, f, node_ptr, state)

    class _Params:
        pass

    fire = _Params()
    fire.__dict__.update({k: (float(np.float32(val)) if k != "n_min" else val) for k, val in FIRE.items()})
    xh, vh, sh = x.double().clone(), v.double().clone(), state.double().clone()
    _fire_step(xh[:n], vh[:n], f.double()[:n], node_ptr, sh, fire)
    assert torch.allclose(xh[:n], x64[:n], rtol=1e-13, atol=1e-13) and torch.allclose(vh[:n], v64[:n], rtol=1e-13, atol=1e-13)
    assert torch.allclose(sh, state64, rtol=1e-13, atol=0)
    assert torch.equal(xh[n:], x.double()[n:]) and torch.equal(vh[n:], v.double()[n:])


def test_fire_step_host_path_freezes_an_empty_graph_at_ftol_zero():
    """include/e3k.h: "An empty graph is frozen with fmax = 0" -- also with ftol = 0 (accepted), where fmax = 0 is not below the
    tolerance: (dt, alpha, n_pos) of the empty graphs stay although n_pos > n_min, the graph between them moves (the case
    fire_ftol0_empty of tests/test_gpu_md_matrix.py, on the torch path)."""
    from e3_layers_amd.run.md import _fire_step
    from tests.test_gpu_md_integrator_kernels import FIRE

    class _Params:
        pass

    fire = _Params()
    fire.__dict__.update(FIRE, ftol=0.0)
    gen = torch.Generator().manual_seed(3)
    x, f = torch.randn(3, 3, generator=gen, dtype=torch.float64), torch.randn(3, 3, generator=gen, dtype=torch.float64)
    v = 0.1 * f
    node_ptr = torch.tensor([0, 0, 3, 3])
    state = torch.tensor([[0.3, 0.08, 9.0, math.inf], [0.1, 0.1, 9.0, math.inf], [0.2, 0.05, 7.0, math.inf]], dtype=torch.float64)
    assert FIRE["n_min"] < 7
    x0, want = x.clone(), state.clone()
    record = torch.full((3,), -7.0, dtype=torch.float64)
    _fire_step(x, v, f, node_ptr, state, fire, None, None, record)
    want[:, 3] = 0.0
    assert torch.equal(state[0], want[0]) and torch.equal(state[2], want[2])
    assert float(record[0]) == 0.0 and float(record[2]) == 0.0
    assert float(state[1, 2]) == 10.0 and float(state[1, 0]) > 0.1 and float(state[1, 3]) > 0 and not torch.equal(x, x0)
