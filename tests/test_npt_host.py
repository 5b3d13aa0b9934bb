"""The barostat on the host (no GPU needed): the algorithm through the torch path of ``run/md._barostat`` -- stochastic cell rescaling
samples the NPT volume distribution of an ideal gas, Berendsen's limit relaxes as its closed form says -- the driver's logic
(``barostat=`` on the integrators) on a stub force field with a cell (tests/npt_stubs.py), and the inventory of
csrc/e3k_barostat.hip against the case table of tests/test_gpu_barostat_matrix.py with float32 models and planted mutants.

Sampling.  An ideal gas of N atoms at pressure p0 has the volume density V^N exp(-p0 V / kT): Gamma(N + 1, kT / p0), mean
(N + 1) kT / p0, variance (N + 1) (kT / p0)^2.  The Euler-Maruyama step is biased to first order in a = compressibility dt / tau
(a numpy restatement measured +0.33 % on the mean and +1.4 % on the variance at a = 0.01); the margins, 1.5 % and 5 %, are about four
times that for the statistical spread of another noise stream.  Measured here (printed by the test): mean + 0.41 %, variance + 1.80 %.

Mutants of the sampling test: the drift with an extra kT / V (the term that the Jacobian and the Ito correction cancel in the
eps = ln V form) moves the mean by about a fifth (measured + 20.7 %); velocities not rescaled decouple K from V (the variance
+ 19.6 %, the mean + 0.6 %).  The mutants run 3 000 steps instead of 12 000: their shifts need no long run."""
import re

import numpy as np
import pytest
import torch

from tests import npt_stubs as S

f64 = torch.float64


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. the algorithm
def _moments(vol):
    return float(vol.mean()), float(vol.var())


def test_scr_samples_the_npt_volume_distribution_of_an_ideal_gas():
    n_atoms, kT, p0, a = 4, 1.0, 2.0, 0.01
    mean_want, var_want = (n_atoms + 1) * kT / p0, (n_atoms + 1) * (kT / p0) ** 2
    kw = dict(n_graphs=4096, n_atoms=n_atoms, kT=kT, p0=p0, a=a, steps=12000, gamma_dt=0.02, seed=20201114)
    mean, var = _moments(S.ideal_gas_volumes(**kw))
    print(f"scr: mean {mean:.4f} ({mean / mean_want - 1:+.3%}), variance {var:.4f} ({var / var_want - 1:+.3%})")
    assert abs(mean / mean_want - 1) < 0.015, mean
    assert abs(var / var_want - 1) < 0.05, var
    for name, mutant in (("drift + kT/V", dict(drift_extra=True)), ("v not rescaled", dict(rescale_v=False))):
        m, s2 = _moments(S.ideal_gas_volumes(**{**kw, **mutant, "steps": 3000}))      # (their shifts need no long run)
        print(f"mutant {name}: mean {m:.4f} ({m / mean_want - 1:+.3%}), variance {s2:.4f} ({s2 / var_want - 1:+.3%})")
        assert abs(m / mean_want - 1) > 0.015 or abs(s2 / var_want - 1) > 0.05, name


def _one_cell(edge=3.0, n=2):
    cell = (torch.eye(3, dtype=f64) * edge).reshape(1, 9).clone()
    cell[0, 3] = 0.25
    x = torch.rand(n, 3, dtype=f64, generator=torch.Generator().manual_seed(1)) * edge
    v = torch.randn(n, 3, dtype=f64, generator=torch.Generator().manual_seed(2))
    return x, v, cell, S.inverse_by_adjugate(cell), torch.ones(1, 3, dtype=torch.int32), torch.tensor([0, n])


def test_berendsen_relaxes_to_the_closed_form_at_the_closed_form_rate():
    """fixed K, zero virial: P = 2 K / 3 V, so V* = 2 K / (3 p0); with delta = ln(V / V*), one step is
    delta' = delta + a p0 (exp(-delta) - 1) = delta (1 - a p0) + a p0 O(delta^2): the rate compressibility p0 / tau per unit time"""
    from e3_layers_amd.run.md import Barostat, _barostat

    baro = Barostat(p0=1.5, compressibility=0.04, tau=2.0, mode="berendsen")
    dt = 0.5
    a, b = baro.coefficients(dt, None)
    assert b == 0.0 and a == 0.04 * 0.5 / 2.0
    x, v, cell, inv, pbc, ptr = _one_cell()
    x0, v0 = x.clone(), v.clone()
    kinetic, virial = torch.tensor([7.0], dtype=f64), torch.zeros(1, 9, dtype=f64)
    v_star = 2.0 * 7.0 / (3.0 * baro.p0)
    counter, vol, prs = torch.zeros(1, dtype=torch.int32), torch.zeros(1, dtype=f64), torch.zeros(1, dtype=f64)
    deltas = []
    for k in range(2500):
        _barostat(x, None, cell, inv, pbc, virial, kinetic, ptr, baro.p0, a, b, 0.0, 0, k, counter, vol, prs)
        deltas.append(float(torch.log(vol[0] / v_star)))
    assert int(counter) == 0 and torch.equal(v, v0)
    assert abs(deltas[-1]) < 1e-9, deltas[-1]                      # (1 - a p0)^2500 = 4e-17 of the start
    assert abs(float(torch.linalg.det(cell.view(3, 3))) - v_star) < 1e-8 * v_star
    # the positions kept their fractional coordinates: x / x0 is the cell's linear scale
    scale = (float(vol[0]) / 27.0) ** (1.0 / 3.0)
    assert torch.allclose(x, x0 * scale, rtol=1e-12, atol=0)
    assert torch.allclose((cell.view(3, 3) @ inv.view(3, 3)), torch.eye(3, dtype=f64), atol=1e-14)
    near = [(d0, d1) for d0, d1 in zip(deltas[:-1], deltas[1:]) if 1e-6 < abs(d0) < 1e-3]
    assert len(near) > 50
    for d0, d1 in near:      # |ratio - (1 - a p0)| <= a p0 |delta| (the second-order term, bounded by its full size)
        assert abs(d1 / d0 - (1.0 - a * baro.p0)) <= a * baro.p0 * abs(d0) + 1e-9, (d0, d1)


def test_zero_compressibility_changes_nothing_bit_for_bit():
    from e3_layers_amd.run.md import Barostat, _barostat

    for mode, kT in (("berendsen", None), ("scr", 0.7)):
        a, b = Barostat(p0=3.0, compressibility=0.0, tau=1.0, mode=mode).coefficients(0.5, kT)
        assert (a, b) == (0.0, 0.0)
        x, v, cell, inv, pbc, ptr = _one_cell()
        before = [t.clone() for t in (x, v, cell, inv)]
        counter = torch.zeros(1, dtype=torch.int32)
        _barostat(x, v, cell, inv, pbc, torch.ones(1, 9, dtype=f64), torch.tensor([2.0], dtype=f64), ptr, 3.0, a, b, 0.0, 5, 9, counter)
        assert int(counter) == 0 and all(torch.equal(p, q) for p, q in zip(before, (x, v, cell, inv)))


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. the driver on a stub force field with a cell
def _md(ff, mass, mode="scr", p0=0.05, compressibility=2.0, tau=5.0, **kw):
    from e3_layers_amd.run.md import Barostat, Langevin, VelocityVerlet

    baro = Barostat(p0, compressibility, tau, mode)
    if mode == "scr":
        md = Langevin(ff, mass, dt=0.05, kT=0.3, gamma=0.5, seed=(5 << 32) + 11, barostat=baro, **kw)
        md.thermalize()
    else:
        md = VelocityVerlet(ff, mass, dt=0.05, barostat=baro, **kw)
        md.v.copy_(0.3 * torch.randn(md.v.shape, dtype=md.v.dtype, generator=torch.Generator().manual_seed(4)))
    return md


def _state(md, out):
    ff = md.ff
    return [md.x.clone(), md.v.clone(), ff.static_cell.clone(), ff.static_inv_cell.clone(), ff.cell.clone().reshape(-1, 9)] + \
        [out[k].clone() for k in ("potential", "kinetic", "volume", "pressure")]


@pytest.mark.parametrize("mode", ["scr", "berendsen"])
def test_a_run_does_not_depend_on_check_every_and_moves_the_cells(mode):
    runs = []
    for check_every in (1, 7, 50):
        ff, mass = S.cell_wells()
        first = ff.cell.clone()
        md = _md(ff, mass, mode)
        runs.append(_state(md, md.run(20, check_every=check_every)))
        assert md.restores == 0 and torch.equal(ff.cell.reshape(-1, 9), ff.static_cell)
        assert torch.allclose(ff.volume, runs[-1][7][-1], rtol=1e-13, atol=0)      # ff.volume follows sync_cell()
    for other in runs[1:]:
        assert all(torch.equal(p, q) for p, q in zip(runs[0], other))
    moved = ((runs[0][4].view(-1, 3, 3) - first).flatten(1).norm(dim=1) / first.flatten(1).norm(dim=1))
    print(mode, "relative cell change per graph", moved.tolist())
    assert float(moved.max()) > 1e-3 and float(moved.min()) > 1e-5      # (scr: a random walk, some graphs have come back)
    vol, prs = runs[0][7], runs[0][8]
    assert vol.dtype == f64 and prs.dtype == f64 and vol.shape == (20, len(S.NPT_SIZES)) and bool((vol > 0).all())
    assert bool(torch.isfinite(prs).all())
    # the pressure of step 0 is that of the START: the kinetic energy of the thermalised velocities and the first evaluation's virial
    ff, mass = S.cell_wells()
    md = _md(ff, mass, mode)
    from e3_layers_amd.run.md import pressure

    ff.evaluate()
    kin0 = torch.stack([(0.5 * mass * (md.v * md.v).sum(1))[a:b].sum() for a, b in zip(ff.bounds[:-1], ff.bounds[1:])])
    # (velocities after the first half kick differ, the record is of the START)
    want = pressure(ff.virial, kin0, ff.volume)
    assert torch.allclose(prs[0], want, rtol=1e-12, atol=1e-15)


@pytest.mark.parametrize("mode", ["scr", "berendsen"])
def test_an_overflow_in_the_middle_of_a_chunk_ends_bit_equal_to_the_run_without_it(mode):
    ff, mass = S.cell_wells()
    md = _md(ff, mass, mode)
    want = _state(md, md.run(24, check_every=8))
    ff2, mass = S.cell_wells(fail_at=13)      # evaluation 1 is run()'s own; 13 is step 12 of 24: the middle of the second chunk
    md2 = _md(ff2, mass, mode)
    got = _state(md2, md2.run(24, check_every=8))
    assert md2.restores >= 1 and md2.regrowths >= 1 and ff2.grown >= 1
    for name, p, q in zip(("x", "v", "cell", "inverse", "ff.cell", "potential", "kinetic", "volume", "pressure"), want, got):
        assert torch.equal(p, q), name
    # the regrowth captured on the last VERIFIED cell (after step 8), not on what the overflowed chunk left
    ff3, mass = S.cell_wells()
    md3 = _md(ff3, mass, mode)
    md3.run(8, check_every=8)
    assert torch.equal(ff2.captured_on[1], ff3.cell) and not torch.equal(ff2.captured_on[1], ff2.captured_on[0])
    assert int(md2._baro_counter) == 0


def test_a_too_narrow_outcome_raises_and_leaves_the_last_verified_state():
    from e3_layers_amd.run.md import BarostatFailure

    squeeze = dict(mode="berendsen", p0=40.0, compressibility=0.05, tau=1.0)      # every step shrinks the cells
    ff, mass = S.cell_wells()
    md = _md(ff, mass, **squeeze)
    out = md.run(6, check_every=2)

    def width0(cell9):      # the smallest perpendicular width of any graph
        inv = torch.linalg.inv(cell9.view(-1, 3, 3).double())
        return float((1.0 / inv.norm(dim=1)).min())

    ff4, mass = S.cell_wells()
    md4 = _md(ff4, mass, **squeeze)
    want = _state(md4, md4.run(4, check_every=2))
    w4 = width0(want[2])
    ff5, mass = S.cell_wells()
    md5 = _md(ff5, mass, **squeeze)
    md5.run(5, check_every=5)
    w5 = width0(ff5.static_cell)
    assert w5 < w4
    # the narrowest graph may take four steps and not the fifth: chunks (0, 1) and (2, 3) are verified, chunk (4, 5) fails
    ff6, mass = S.cell_wells(min_width=0.5 * (w4 + w5))
    md6 = _md(ff6, mass, **squeeze)
    with pytest.raises(BarostatFailure) as err:
        md6.run(6, check_every=2)
    count = err.value.count      # the narrowest graph at steps 4 and 5, and whichever others crossed at step 5
    assert 2 <= count < 2 * len(S.NPT_SIZES) and f"froze {count} " in str(err.value)
    assert md6.restores == 1 and md6.steps_done == 4 and int(md6._baro_counter) == 0
    got = [md6.x, md6.v, ff6.static_cell, ff6.static_inv_cell, ff6.cell.reshape(-1, 9)]
    for name, p, q in zip(("x", "v", "cell", "inverse", "ff.cell"), want, got):
        assert torch.equal(p, q), name
    assert not md6._vol[4:].any() and torch.equal(md6._vol[:4], want[7]) and torch.equal(md6._prs[:4], want[8])
    # a sane coupling afterwards works from there
    from e3_layers_amd.run.md import Barostat

    md6.barostat = Barostat(0.05, 0.5, 5.0, "berendsen")
    more = md6.run(3, check_every=2)
    assert bool((more["volume"] > 0).all()) and md6.steps_done == 7


def test_barostat_none_is_the_plain_integrator():
    from e3_layers_amd.run.md import Langevin

    outs = []
    for kw in ({}, {"barostat": None}):
        ff, mass = S.cell_wells()
        md = Langevin(ff, mass, dt=0.05, kT=0.3, gamma=0.5, seed=3, **kw)
        md.thermalize()
        out = md.run(10, check_every=4)
        assert set(out) == {"potential", "kinetic"} and md._tensors() == (md.v,)
        outs.append((md.x.clone(), md.v.clone(), out["potential"], out["kinetic"], ff.static_cell.clone()))
    assert all(torch.equal(p, q) for p, q in zip(*outs))


def test_construction_refusals_name_their_reason():
    from e3_layers_amd.run.md import Barostat, BondConstraints, Langevin, VelocityVerlet
    from tests.md_stubs import WellField

    baro = Barostat(1.0, 0.1, 1.0)
    with pytest.raises(ValueError, match="tau"):
        Barostat(1.0, 0.1, 0.0)
    with pytest.raises(ValueError, match="tau"):
        Barostat(1.0, 0.1, -2.0)
    with pytest.raises(ValueError, match="compressibility"):
        Barostat(1.0, -0.1, 1.0)
    with pytest.raises(ValueError, match="mode"):
        Barostat(1.0, 0.1, 1.0, mode="mtk")
    ff, mass = S.cell_wells()
    with pytest.raises(ValueError, match="kT"):      # scr on an integrator without a temperature
        VelocityVerlet(ff, mass, 0.05, barostat=baro)
    VelocityVerlet(ff, mass, 0.05, barostat=Barostat(1.0, 0.1, 1.0, "berendsen"))
    Langevin(ff, mass, 0.05, kT=0.0, gamma=0.1, barostat=baro)      # (kT = 0 is a temperature: b = 0)
    open_ff = WellField(S.NPT_SIZES, ff.k, ff.sites, ff.pos)
    with pytest.raises(ValueError, match="no cell"):
        Langevin(open_ff, mass, 0.05, 0.3, 0.1, barostat=baro)
    slab, _ = S.cell_wells()
    slab.pbc[1, 2] = False
    with pytest.raises(ValueError, match="non-periodic axis"):
        Langevin(slab, mass, 0.05, 0.3, 0.1, barostat=baro)
    keyless, _ = S.cell_wells()
    keyless.virial_key = None
    with pytest.raises(ValueError, match="virial_key"):
        Langevin(keyless, mass, 0.05, 0.3, 0.1, barostat=baro)
    bonds = BondConstraints(torch.tensor([[0, 1]]), pos=ff.pos, node_ptr=ff.node_ptr, masses=mass)
    with pytest.raises(ValueError, match="constraints"):
        Langevin(ff, mass, 0.05, 0.3, 0.1, constraints=bonds, barostat=baro)


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. inventory: the object, the header and the case table of tests/test_gpu_barostat_matrix.py; its bounds on float32 models
from tests import test_gpu_barostat_matrix as M      # noqa: E402
from tests.test_train_inventory import HEADER, _shipped_kernels      # noqa: E402

LAUNCHING = [c for c in M.CASES if c["kind"] == "step"]
BY_ID = {c["id"]: c for c in M.CASES}
MUTANTS = [("mu_on_v", "G5"), ("inverse_of_old_cell", "G1_n1"), ("inverse_of_old_cell", "G9_garbage_ptr"),
           ("noise_word_without_graph", "G5"), ("noise_word_without_graph", "G9_garbage_ptr"), ("width_on_old_cell", "freeze_narrow"),
           ("width_on_old_cell", "freeze_narrow_noise")]


def test_every_barostat_kernel_has_a_float64_checked_case(tmp_path):
    shipped = _shipped_kernels(tmp_path, "e3k_barostat.o") - {"zero_words_kernel"}      # (e3k_common.h's helper, in every object)
    assert shipped == M.table_kernels() == {"barostat_step_kernel"}, (sorted(shipped), sorted(M.table_kernels()))
    assert any(c["kind"] == "step" and shipped <= c["kernels"] for c in M.CASES)


def test_the_header_declares_exactly_the_barostat_functions_the_cases_call():
    with open(HEADER) as f:
        text = f.read()
    declared = set(re.findall(r"\b(e3k_barostat_\w+)\s*\(", text))
    assert declared == M.table_functions() == {"e3k_barostat_step"}, (sorted(declared), sorted(M.table_functions()))
    kinds = {(c["kind"], c.get("rc")) for c in M.CASES}
    assert {("step", None), ("refuse", M.E3K_ERR_INVALID), ("refuse", M.E3K_OK)} <= kinds
    assert text.index("e3k_barostat_step(") > text.index("e3k_virial_edges(")      # its section is the header's last
    ids = [c["id"] for c in M.CASES]
    assert len(ids) == len(set(ids)) and all(c["why"] for c in M.CASES)


def test_the_case_table_covers_what_the_kernel_can_meet():
    of = LAUNCHING
    assert {len(c["sizes"]) for c in of} >= {1, 5, 9}
    assert set().union(*(c["sizes"] for c in of)) >= {0, 1, 85, 86, 200, 600}
    assert any(c["sizes"][0] == 0 and c["sizes"][-1] == 0 for c in of)
    names = {s.partition("*")[0] for c in of for s in c["cells"]}
    assert names == {"ortho", "tri", "zero", "singular"}
    assert {c["b"] > 0 for c in of} == {True, False} and {c["vnull"] for c in of} == {True, False}
    assert {c["records"] for c in of} == {True, False} and {c["counter0"] for c in of} == {0, 7}
    assert any(c["ptr"] == "garbage" for c in of) and (M.SEED >> 32) and (M.SEED & 0xFFFFFFFF)
    assert {p for c in of for p in c["plants"].values()} == {"nonfinite_virial", "nan_offdiagonal"}
    refused = {k for c in M.CASES if c["kind"] == "refuse" for k in c["change"]}
    assert refused == {"G", "n", "a", "b", "min_width", "x", "cell", "inv_cell", "pbc", "virial", "kinetic", "node_ptr", "counter"}
    want_frozen = {"zero_cell": [1], "freeze_singular": [1], "freeze_nonfinite_virial": [1], "freeze_narrow": [0],
                   "freeze_narrow_noise": [0, 2]}
    for c in of:      # the planted freezes are the only ones, and every width decision is clear of its threshold
        inp = M.inputs(c)
        ref = M.reference(c, inp)
        assert np.flatnonzero(ref["frozen"]).tolist() == want_frozen.get(c["id"], []), c["id"]
        assert ref["margin"] > 1e-3, (c["id"], ref["margin"])
        live = ~ref["frozen"]
        assert (np.abs(ref["mu"][live] - 1.0) > 1e-4).all(), (c["id"], ref["mu"])      # every live graph really moves
    inp = M.inputs(BY_ID["freeze_narrow"])
    assert M.widths(M.exact_inverse(inp["cell"][0])[0]).min() == 9.0      # the 9.0-wide cell ...
    mu0 = float(np.exp((M.reference(BY_ID["freeze_narrow"], inp)["pressure"][0] - 0.6) / 3.0))
    assert 9.0 * mu0 < M.MIN_WIDTH == 8.008      # ... that p0 = 0.6 would take under 8.008


@pytest.mark.parametrize("c", LAUNCHING, ids=[c["id"] for c in LAUNCHING])
def test_a_float32_model_of_the_kernel_stays_inside_the_bounds(c):
    inp = M.inputs(c)
    ref = M.reference(c, inp)
    got = M.model32(c, inp)
    if not c["records"]:
        got["volume"][:], got["pressure"][:] = np.nan, np.nan
    r = M.expected(c, inp, ref, got)
    print(f"{c['id']}: float32 model, worst error / bound {r:.3f}, counter {got['counter']}")
    assert r <= 1.0


def test_the_bounds_are_not_slack():
    worst = max(M.expected(c, M.inputs(c), M.reference(c, M.inputs(c)), M.model32(c, M.inputs(c))) for c in LAUNCHING if c["records"])
    assert 0.2 < worst <= 1.0, worst


@pytest.mark.parametrize("mutant,cid", MUTANTS, ids=[f"{m}-{cid}" for m, cid in MUTANTS])
def test_planted_mutants_leave_the_bounds(mutant, cid):
    c = BY_ID[cid]
    inp = M.inputs(c)
    ref = M.reference(c, inp)
    assert M.expected(c, inp, ref, M.model32(c, inp)) <= 1.0
    r = M.expected(c, inp, ref, M.model32(c, inp, mutant))
    print(f"{mutant} on {cid}: worst error / bound {r:.3g}")
    assert r > 1.0
