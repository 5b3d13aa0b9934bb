"""The velocity-Verlet half-step kernels (csrc/e3k_md.hip: e3k_md_drift, e3k_md_kick) called directly, against the same
arithmetic in float64 torch: random masses (the per-node mass indexing), graphs of unequal sizes -- one atom, more than a wave's
64 lanes, an empty graph -- (the per-graph placement of the kinetic energies), and rows behind the real nodes that must not move.

Bounds: every updated component is a handful of fp32 operations on O(1) numbers: 8 ulp of fp32 (1e-6) relative to the largest
component.  A kinetic energy is a sum of <= 150 positive fp32 terms: 150 x 2^-24 < 1e-5 of the sum."""
import pytest
import torch

pytestmark = pytest.mark.gpu

SIZES = (1, 70, 0, 5, 150, 3)      # nodes per graph; 229 real nodes
N_GHOST = 7                        # rows behind them that belong to nobody
DT = 0.37


def _state(dev, seed):
    g = torch.Generator().manual_seed(seed)
    n = sum(SIZES)
    x, v, f = (torch.randn(n + N_GHOST, 3, generator=g) for _ in range(3))
    mass = 0.5 + 11.5 * torch.rand(n + N_GHOST, generator=g)          # 0.5 .. 12: nothing like 1
    node_ptr = torch.tensor([0] + list(torch.tensor(SIZES).cumsum(0)), dtype=torch.int64)
    return n, x, v, f, mass, node_ptr


def _close(got, want, tol):
    return float((got.double().cpu() - want).abs().max()) <= tol * max(float(want.abs().max()), 1e-30)


def test_drift_kernel_uses_each_nodes_mass_and_leaves_the_tail_alone(dev):
    from e3_layers_amd.run.md import _drift

    n, x, v, f, mass, _ = _state(dev, 0)
    xd, vd, fd, md = (t.to(dev).contiguous() for t in (x, v, f, mass))
    _drift(xd[:n], vd[:n], fd[:n], md[:n], DT)
    torch.cuda.synchronize()
    v64 = v[:n].double() + 0.5 * DT * f[:n].double() / mass[:n].double()[:, None]
    x64 = x[:n].double() + DT * v64
    assert _close(vd[:n], v64, 1e-6)
    assert _close(xd[:n], x64, 1e-6)
    assert torch.equal(xd[n:].cpu(), x[n:]) and torch.equal(vd[n:].cpu(), v[n:])      # the rows behind: untouched, bit for bit
    # the masses matter: the same call with unit masses lands elsewhere
    assert not _close(vd[:n], v[:n].double() + 0.5 * DT * f[:n].double(), 1e-3)


def test_kick_kernel_files_kinetic_and_potential_energy_per_graph(dev):
    from e3_layers_amd.run.md import _kick_langevin

    n, _, v, f, mass, node_ptr = _state(dev, 1)
    n_graphs = len(SIZES)
    vd, fd, md, ptr = (t.to(dev).contiguous() for t in (v, f, mass, node_ptr))
    energy = torch.randn(n_graphs, generator=torch.Generator().manual_seed(2)).to(dev)
    record = torch.full((2, n_graphs + 2), -7.0, device=dev)       # [kinetic | potential], a canary on either side of each row
    kin, pot = record[0, 1:-1], record[1, 1:-1]
    _kick_langevin(vd[:n], fd[:n], md[:n], ptr, DT, 1.0, 0.0, 0, 0, 0, kin, energy, pot)
    torch.cuda.synchronize()
    v64 = v[:n].double() + 0.5 * DT * f[:n].double() / mass[:n].double()[:, None]
    per_node = 0.5 * mass[:n].double() * (v64 * v64).sum(1)
    want = torch.stack([per_node[int(node_ptr[g]):int(node_ptr[g + 1])].sum() for g in range(n_graphs)])
    assert _close(vd[:n], v64, 1e-6)
    assert torch.equal(vd[n:].cpu(), v[n:])
    got = kin.double().cpu()
    assert ((got - want).abs() <= 1e-5 * want.abs()).all(), (got, want)              # graph by graph, each against its own sum
    assert float(got[SIZES.index(0)]) == 0.0                                         # the empty graph
    assert torch.equal(pot, energy)
    assert (record[:, 0] == -7.0).all() and (record[:, -1] == -7.0).all()
    # fixed summation order: the same bits on a second run from the same state
    vd2 = v.to(dev).contiguous()
    kin2 = torch.empty(n_graphs, device=dev)
    _kick_langevin(vd2[:n], fd[:n], md[:n], ptr, DT, 1.0, 0.0, 0, 0, 0, kin2)
    assert torch.equal(kin2, kin) and torch.equal(vd2, vd)
