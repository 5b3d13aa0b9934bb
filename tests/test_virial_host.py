"""The virial on the host (no GPU needed): the kernel of e3k_virial.o and the ``e3k_virial_*`` functions of the header held to the case
table of tests/test_gpu_virial_matrix.py; that file's bound shown to hold for a numpy float32 model of the kernel in its lane and
reduction order, and to be sharp (a wrong term planted in the float64 reference moves an element by >= 100 bounds on a case's own
inputs, the criterion of tests/test_edge_inventory.py); the definition and the sign in float64 against central differences of the
oracle's energy under a homogeneous strain; ``pressure``; and the refusals of ``GradientOutput`` that need no kernel.

Mutants (planted in the reference, never in the library):
  sign         +sum for -sum
  transposed   g (x) v for v (x) g
  no_g_len     the g_len term dropped
  no_inv_len   g_len vec for g_len vec / len

``oracle_strain_gradient`` is the float64 reference of tests/test_gpu_stress_force_field.py too: the oracle network on a FIXED list with
a differentiable ``edge_vector`` (as ``_PeriodicOracleField`` of tests/test_gpu_pbc_force_field.py builds it), its gradient with
respect to that vector, and ``sum_e v_e (x) g_e`` per graph.
"""
import os
import re

import numpy as np
import pytest
import torch

from oracle import e3ref
from tests import test_gpu_virial_matrix as M
from tests.test_batch_inventory import _shipped_kernels
from tests.test_gpu_md import _small_tree
from tests.test_gpu_pbc_force_field import CELLS, E_KEY, _host_list, _periodic_batch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "e3k.h")
CASES = {c["id"]: c for c in M.CASES}
f32, f64 = np.float32, np.float64


# ---------------------------------------------------------------------------------------------------------------------------------
# inventory
def test_every_virial_kernel_has_a_float64_checked_case(tmp_path):
    shipped = _shipped_kernels(tmp_path, "e3k_virial")
    table = M.table_kernels()
    assert shipped == table == {"virial_edges_kernel"}, (sorted(shipped), sorted(table))
    for k in shipped:
        assert any(k in c["kernels"] and c["kind"] != "refuse" for c in M.CASES), k


def test_every_virial_function_of_the_header_is_called_by_a_case():
    with open(HEADER) as f:
        declared = set(re.findall(r"\b(e3k_virial_\w+)\s*\(", f.read()))
    called = M.table_functions()
    assert declared == called == {"e3k_virial_edges"}, (sorted(declared), sorted(called))
    for fn in declared:      # ... and refused by one
        assert any(c["kind"] == "refuse" and fn in c["funcs"] for c in M.CASES), fn
    ids = [c["id"] for c in M.CASES]
    assert len(ids) == len(set(ids)) and all(c["why"] for c in M.CASES)


def test_cases_sit_on_their_seams():
    for cid, edges in (("E255", 255), ("E256", 256), ("E257", 257), ("E769", 769), ("one_edge", 1), ("G1_E0", 0)):
        assert max(e for _, e in CASES[cid]["graphs"]) == edges
    inp = M.inputs(CASES["shuffled"])
    assert not np.array_equal(inp["src_perm"], np.arange(inp["E"])) and (np.diff(inp["src"][inp["src_perm"]]) >= 0).all()
    assert np.array_equal(M.inputs(CASES["E257"])["src_perm"], np.arange(270))      # (stored by source: the identity)
    for cid in ("g_len_only", "self_loops", "integers"):
        assert (M.inputs(CASES[cid])["len"] == 0).sum() == CASES[cid]["loops"] > 0
    inp = M.inputs(CASES["ghost_third"])
    assert (inp["edge_graph"] == inp["G"] - 1).sum() * 3 == inp["E"]
    assert M.inputs(CASES["g_vec_only"])["g_len"] is None and M.inputs(CASES["g_len_only"])["g_vec"] is None
    want, bound = M.reference(CASES["middle_empty"], M.inputs(CASES["middle_empty"]))
    assert not want[1].any() and not bound[1].any() and want[0].all() and want[2].all()


# ---------------------------------------------------------------------------------------------------------------------------------
# the float32 model: virial_edges_kernel operation for operation
def _fma32(a, b, c):
    return f32(f64(a) * f64(b) + f64(c))      # (the double product of two floats is exact; one rounding)


def model32(inp):
    """out [G, 9] fp32: lane k of 256 takes the slots t0 + k, t0 + k + 256, ... of its graph with nine double accumulators; six
    shuffle-down levels inside each wave of 64 (lane 0 of the wave holds the sum), the four wave partials added in order; -sum rounded"""
    G = inp["G"]
    out = np.zeros((G, 9), f32)
    for g in range(G):
        t0, t1 = (int(inp["src_ptr"][inp["graph_ptr"][k]]) for k in (g, g + 1))
        lanes = np.zeros((256, 9), f64)
        for t in range(t0, t1):
            e = inp["src_perm"][t]
            v = inp["vec"][e]
            grad = [inp["g_vec"][e, k] if inp["g_vec"] is not None else f32(0) for k in range(3)]
            if inp["g_len"] is not None:
                ln = inp["len"][e]
                f = inp["g_len"][e] / ln if ln > 0 else f32(0)
                assert isinstance(f, f32)
                grad = [_fma32(f, v[k], grad[k]) for k in range(3)]
            lanes[(t - t0) % 256] += np.array([f64(v[a]) * f64(grad[b]) for a in range(3) for b in range(3)])
        total = np.zeros(9, f64)
        for w in range(4):
            s = lanes[64 * w:64 * w + 64].copy()
            for off in (32, 16, 8, 4, 2, 1):
                s = s + np.concatenate([s[off:], s[64 - off:]])      # (a lane past the wave's end reads its own value)
            total = total + s[0]
        out[g] = (-total).astype(f32)
    return out


@pytest.mark.parametrize("cid", [c["id"] for c in M.CASES if c["kind"] == "virial"])
def test_the_bound_holds_for_a_float32_model(cid):
    c = CASES[cid]
    inp = M.inputs(c)
    want, bound = M.reference(c, inp)
    got = model32(inp).astype(f64)
    err = np.abs(got - want)
    live = bound > 0
    assert (err <= bound).all() and (got[~live] == 0).all(), float((err[live] / bound[live]).max())
    if c["exact"]:
        assert np.array_equal(got, want)
    if live.any():
        print(cid, "float32 model, worst error / bound:", float((err[live] / bound[live]).max()))


def test_the_bound_is_not_slack():
    """over the cases the float32 model uses more than a twentieth of the bound somewhere: the count of roundings is not a safety factor"""
    worst = 0.0
    for c in M.CASES:
        if c["kind"] == "virial" and not c["exact"] and sum(e for _, e in c["graphs"]):
            inp = M.inputs(c)
            want, bound = M.reference(c, inp)
            live = bound > 0
            worst = max(worst, float((np.abs(model32(inp).astype(f64) - want)[live] / bound[live]).max()))
    assert 0.05 < worst <= 1.0, worst


# ---------------------------------------------------------------------------------------------------------------------------------
# the bound is sharp
MUTANTS = [("sign", "E257"), ("transposed", "shuffled"), ("no_g_len", "self_loops"), ("no_inv_len", "g_len_only")]


@pytest.mark.parametrize("mutant,cid", MUTANTS, ids=[m[0] for m in MUTANTS])
def test_a_planted_mutant_moves_an_element_by_100_bounds(mutant, cid):
    c = CASES[cid]
    inp = M.inputs(c)
    (want, bound), (mut, _) = M.reference(c, inp), M.reference(c, inp, mutant=mutant)
    live = bound > 0
    move = float((np.abs(mut - want)[live] / bound[live]).max())
    print(f"mutant {mutant} on {cid}: {move:.3g} bounds")
    assert move >= 100.0, f"{mutant}: the reference moves by {move} bounds only"


# ---------------------------------------------------------------------------------------------------------------------------------
# definition and sign in float64
def oracle_strain_gradient(net, batch, pos, ei, shift=None, cell=None, strain=None):
    """The energy network ``net`` (the oracle's, float64, WITHOUT its gradient head) on the fixed list ``ei`` with
    ``v_e = (pos[dst] - pos[src] + shift_e @ cell) (I + strain)``: (energy [G], strain_grad [G, 3, 3] = sum_{e in g} v_e (x) dE/dv_e,
    majorant [G, 3, 3] = sum |v_e| (x) |dE/dv_e|, dE/dv [E, 3], v [E, 3])"""
    x = pos.detach().double()
    seg = batch["_node_segment"][ei[0]]
    vec = x[ei[1]] - x[ei[0]]
    if shift is not None:
        vec = vec + torch.einsum("ek,ekc->ec", shift.double(), cell.double().reshape(-1, 3, 3)[seg])
    if strain is not None:
        vec = vec @ (torch.eye(3, dtype=torch.float64) + strain)
    vec = vec.clone().requires_grad_(True)
    G = batch["_n_nodes"].numel()
    n_edges = torch.bincount(seg, minlength=G).reshape(-1, 1)
    data = {"pos": x, "species": batch["species"], "_n_nodes": batch["_n_nodes"], "edge_index": ei, "_n_edges": n_edges, "edge_vector": vec}
    attrs = {k: batch.attrs[k] for k in ("pos", "species")}
    attrs.update(edge_vector=("edge", "1x1o"), _n_edges=("graph", "1x0e"))
    out, _ = net(data, attrs)
    energy = out[E_KEY].reshape(-1)
    (g,) = torch.autograd.grad(energy.sum(), vec)
    v = vec.detach()
    sg = torch.zeros(G, 3, 3, dtype=torch.float64).index_add_(0, seg, v[:, :, None] * g[:, None, :])
    maj = torch.zeros(G, 3, 3, dtype=torch.float64).index_add_(0, seg, v.abs()[:, :, None] * g.abs()[:, None, :])
    return energy.detach(), sg, maj, g, v


def _oracle_net(seed=0):
    torch.manual_seed(seed)
    return e3ref.build(_small_tree()).double().eval()


def test_strain_gradient_equals_central_differences_of_the_energy():
    """x -> x (I + eps), cell -> cell (I + eps) on the periodic batch with the list held fixed: (E(+h) - E(-h)) / 2 h in each of the
    nine components == sum_e v_e (x) dE/dv_e.  First the premise: the differences at h and h / 2 agree so closely that the truncation
    error of the finer one, a third of their distance, is below 1e-7 of the majorant."""
    orc = _oracle_net()
    batch = _periodic_batch()
    ei, shift, _ = _host_list(batch, batch["pos"])
    assert (shift != 0).any()
    _, sg, maj, _, _ = oracle_strain_gradient(orc.func, batch, batch["pos"], ei, shift, CELLS)

    def differences(h):
        out = torch.zeros_like(sg)
        for a in range(3):
            for b in range(3):
                eps = torch.zeros(3, 3, dtype=torch.float64)
                eps[a, b] = h
                ep = oracle_strain_gradient(orc.func, batch, batch["pos"], ei, shift, CELLS, strain=eps)[0]
                em = oracle_strain_gradient(orc.func, batch, batch["pos"], ei, shift, CELLS, strain=-eps)[0]
                out[:, a, b] = (ep - em) / (2 * h)
        return out

    h = 2e-4
    coarse, fine = differences(h), differences(h / 2)
    truncation = float(((coarse - fine).abs() / 3 / maj).max())
    err = float(((fine - sg).abs() / maj).max())
    antisym = float((sg - sg.transpose(1, 2)).norm() / sg.norm())
    print(f"strain gradient: truncation {truncation:.3g}, error {err:.3g} of the majorant; antisymmetric part {antisym:.3g}")
    assert truncation < 1e-7, truncation
    assert err < 1e-6, err
    assert float(sg.abs().max()) > 1e-3 * float(maj.max())      # (not a comparison of zeros)
    assert antisym < 1e-10      # a rotation-invariant energy: the strain gradient is symmetric


def test_open_cluster_virial_is_the_sum_of_position_times_force():
    """-strain_grad = sum_n x_n (x) F_n with the oracle's own forces (its gradient head), to 1e-12 of the majorant"""
    from e3_layers_amd.data.synthetic import synth_qm9

    orc = _oracle_net()
    batch = synth_qm9(7, 3)
    ei = batch["edge_index"]
    _, sg, maj, _, _ = oracle_strain_gradient(orc.func, batch, batch["pos"], ei)
    data = {"pos": batch["pos"].double(), "species": batch["species"], "_n_nodes": batch["_n_nodes"], "edge_index": ei,
            "_n_edges": batch["_n_edges"]}
    out, _ = orc(data, {k: batch.attrs[k] for k in ("pos", "species", "edge_index") if k in batch.attrs})
    x, force = data["pos"], out["forces"].detach()
    seg = batch["_node_segment"]
    xf = torch.zeros_like(sg).index_add_(0, seg, x[:, :, None] * force[:, None, :])
    err = float(((-sg - xf).abs() / maj).max())
    print("open cluster: |(-strain_grad) - sum x (x) F| / majorant", err)
    assert err < 1e-12, err
    assert float(force.abs().max()) > 0


# ---------------------------------------------------------------------------------------------------------------------------------
def test_pressure_of_a_hand_computed_three_atom_case():
    from e3_layers_amd.run.md import pressure

    x = torch.tensor([[0.0, 0, 0], [1, 0, 0], [0, 2, 0]], dtype=torch.float64)
    force = torch.tensor([[-1.0, 0, 0], [1, -0.5, 0], [0, 0.5, 0]], dtype=torch.float64)
    virial = (x[:, :, None] * force[:, None, :]).sum(0)      # xx = 1, xy = -0.5, yy = 1: trace 2
    assert torch.equal(virial, torch.tensor([[1.0, -0.5, 0], [0, 1, 0], [0, 0, 0]], dtype=torch.float64))
    mass, vel = torch.tensor([1.0, 2, 3]), torch.tensor([[1.0, 0, 0], [0, 1, 0], [0, 0, 2]])
    kinetic = 0.5 * (mass * (vel * vel).sum(1)).sum()        # 0.5 (1 + 2 + 12) = 7.5
    p = pressure(virial.reshape(1, 3, 3), kinetic.reshape(1), torch.tensor([10.0]))
    assert p.dtype == torch.float64 and p.shape == (1,)
    assert abs(float(p[0]) - 17.0 / 30.0) < 1e-15      # (2 * 7.5 + 2) / (3 * 10)
    both = pressure(torch.stack([virial, 2 * virial]).reshape(2, 9).float(), torch.tensor([7.5, 0.0]), torch.tensor([10.0, 4.0]))
    assert torch.allclose(both, torch.tensor([17.0 / 30.0, 4.0 / 12.0], dtype=torch.float64), rtol=1e-15, atol=0)


# ---------------------------------------------------------------------------------------------------------------------------------
# GradientOutput: what is refused before any kernel runs
def _cpu_model():
    from e3_layers_amd.utils import build

    torch.manual_seed(0)
    return build(_small_tree()).eval()


def test_gradient_output_keys_and_enable_virial():
    from e3_layers_amd.configs.layer_configs import addEnergyOutput, addForceOutput, featureModel
    from e3_layers_amd.nn import GradientOutput, Pooling, enable_virial

    model = _cpu_model()
    assert isinstance(model, GradientOutput) and model.virial is None and model.stress is None
    assert enable_virial(model) is model and (model.virial, model.stress) == ("virial", "stress")
    enable_virial(model, "w", None)
    assert (model.virial, model.stress) == ("w", None)
    with pytest.raises(ValueError, match="no GradientOutput"):
        enable_virial(Pooling("4x0e", "4x0e", "sum"))
    cfg = featureModel(n_dim=16, l_max=2, edge_spherical="1x0e+1x1o+1x2e", node_attrs="16x0e", edge_radial="8x0e", num_types=10,
                       num_layers=3, r_max=4.0)
    plain = addForceOutput(addEnergyOutput(cfg, None, output_key="energy_total"), y="energy_total")
    assert "virial" not in plain and "stress" not in plain      # the default tree is what it was
    keyed = addForceOutput(addEnergyOutput(cfg, None, output_key="energy_total"), y="energy_total", virial="W", stress="S")
    assert keyed["virial"] == "W" and keyed["stress"] == "S"


def test_stress_without_a_cell_training_mode_and_supplied_edge_vectors_are_refused():
    from e3_layers_amd.data.synthetic import synth_qm9
    from e3_layers_amd.nn import enable_virial

    model = enable_virial(_cpu_model())
    batch = synth_qm9(7, 3)
    with pytest.raises(ValueError, match="no 'cell'"):
        model(batch.clone())
    enable_virial(model, "virial", None)
    model.train()
    with pytest.raises(NotImplementedError, match="training"):
        model(batch.clone())
    model.eval()
    supplied = batch.clone()
    supplied["edge_vector"] = supplied["pos"][supplied["edge_index"][1]] - supplied["pos"][supplied["edge_index"][0]]
    with pytest.raises(NotImplementedError, match="edge_vector"):
        model(supplied)
    assert not batch["pos"].requires_grad
