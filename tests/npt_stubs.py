"""Stub force fields with a CELL for the barostat's driver tests (host, float64): ``WellField`` of tests/md_stubs.py with the surface
``run/md.py`` asks of a force field under ``barostat=`` -- ``cell``, ``pbc``, ``virial_key``, ``virial``, the static rows
``static_cell`` / ``static_inv_cell`` / ``static_pbc``, ``min_width``, ``sync_cell()``, ``volume`` -- and an ideal gas for the
sampling test.  ``grow()`` does what the real one does: NEW static buffers, made from ``cell`` (the last synchronised one), the
inverse formed on the host."""
import torch

from tests.md_stubs import WellField, node_ptr_of

NPT_SIZES = (3, 70, 0, 5, 20)      # nodes per graph: more than a wave, an empty graph in the middle


def inverse_by_adjugate(cell):
    """[G, 9] float64: the barostat's own rule, so that a step with mu = 1 rewrites the same bits"""
    from e3_layers_amd.run.md import _adjugate3, _det3

    c = cell.reshape(-1, 9).double()
    return _adjugate3(c) / _det3(c)[:, None]


class CellWellField(WellField):
    """Per-atom wells in per-graph cells.  virial[g] = sum_i x_i (x) f_i over the graph's atoms (what an open cluster's is), float64,
    summed in a fixed order.  ``min_width`` is an attribute here (the real one derives it from r_max)."""

    virial_key = "virial"

    def __init__(self, sizes, k, sites, pos, cell, min_width=0.0, fail_at=None, pbc=None):
        super().__init__(sizes, k, sites, pos, fail_at=fail_at)
        n_graphs = len(sizes)
        self.cell = cell.reshape(n_graphs, 3, 3).to(pos).clone()
        self.pbc = torch.ones(n_graphs, 3, dtype=torch.bool) if pbc is None else pbc
        self.min_width = float(min_width)
        self._capture()
        self._virial = torch.zeros(n_graphs, 9, dtype=pos.dtype)
        self.captured_on = [self.cell.clone()]      # the cell of every capture (tests)

    def _capture(self):
        self._cell = self.cell.reshape(-1, 9).clone()
        self._inv = inverse_by_adjugate(self._cell).to(self._cell.dtype)
        self._pbc = self.pbc.to(torch.int32).clone()
        self.volume = torch.linalg.det(self.cell.double()).abs()

    static_cell = property(lambda self: self._cell)
    static_inv_cell = property(lambda self: self._inv)
    static_pbc = property(lambda self: self._pbc)
    virial = property(lambda self: self._virial.view(-1, 3, 3))

    def sync_cell(self):
        self.cell.copy_(self._cell.view(-1, 3, 3))
        self.volume = torch.linalg.det(self.cell.double()).abs()

    def evaluate(self):
        energy, forces = super().evaluate()
        outer = self.pos[:, :, None] * forces[:, None, :]
        for g, (a, b) in enumerate(zip(self.bounds[:-1], self.bounds[1:])):
            self._virial[g] = outer[a:b].sum(0).reshape(9)
        return energy, forces

    def grow(self, factor):
        super().grow(factor)
        self._capture()
        self.captured_on.append(self.cell.clone())


def cell_wells(sizes=NPT_SIZES, seed=5, fail_at=None, min_width=0.0, box=6.0):
    """(force field, masses): atoms scattered in cubic-ish cells of edge ``box`` .. ``box + 1``, wells of stiffness 0.5 .. 2 about
    sites 0.3 away, float64."""
    g = torch.Generator().manual_seed(seed)
    n, n_graphs = sum(sizes), len(sizes)
    edge = box + torch.rand(n_graphs, generator=g, dtype=torch.float64)
    cell = torch.diag_embed(edge[:, None] * (1.0 + 0.1 * torch.rand(n_graphs, 3, generator=g, dtype=torch.float64)))
    cell[:, 1, 0] = 0.3      # (not orthorhombic: the inverse has an off-diagonal entry)
    seg = torch.repeat_interleave(torch.arange(n_graphs), torch.tensor(sizes))
    sites = torch.rand(n, 3, generator=g, dtype=torch.float64) * edge[seg][:, None]
    k = 0.5 + 1.5 * torch.rand(n, 3, generator=g, dtype=torch.float64)
    pos = sites + 0.3 * torch.randn(n, 3, generator=g, dtype=torch.float64)
    mass = 0.5 + 3.5 * torch.rand(n, generator=g, dtype=torch.float64)
    return CellWellField(sizes, k, sites, pos, cell, min_width=min_width, fail_at=fail_at), mass


def ideal_gas_volumes(n_graphs, n_atoms, kT, p0, a, steps, gamma_dt, seed, *, drift_extra=False, rescale_v=True, every=10, drop=0.25):
    """Volumes [samples, n_graphs] of an ideal gas of unit masses under the host path of ``run/md._barostat`` (zero virial) with an
    exact Ornstein-Uhlenbeck thermostat between the barostat steps; b = 2 kT a.  The mutants: ``drift_extra`` adds kT / V to the
    pressure the barostat sees (through the kinetic energy: 2 (K + 3 kT / 2) / 3 V), ``rescale_v`` False leaves the velocities alone."""
    from e3_layers_amd.run.md import _barostat

    gen = torch.Generator().manual_seed(seed)
    n = n_graphs * n_atoms
    node_ptr = torch.arange(n_graphs + 1, dtype=torch.int64) * n_atoms
    x = torch.zeros(n, 3, dtype=torch.float64)
    v = (kT ** 0.5) * torch.randn(n, 3, generator=gen, dtype=torch.float64)
    edge = ((n_atoms + 1) * kT / p0) ** (1.0 / 3.0)
    cell = (torch.eye(3, dtype=torch.float64) * edge).reshape(1, 9).repeat(n_graphs, 1)
    inv = inverse_by_adjugate(cell)
    pbc = torch.ones(n_graphs, 3, dtype=torch.int32)
    virial = torch.zeros(n_graphs, 9, dtype=torch.float64)
    counter = torch.zeros(1, dtype=torch.int32)
    volume = torch.zeros(n_graphs, dtype=torch.float64)
    c = float(torch.exp(torch.tensor(-gamma_dt, dtype=torch.float64)))
    s = ((1.0 - c * c) * kT) ** 0.5
    out = []
    for k in range(steps):
        v.mul_(c).add_(torch.randn(n, 3, generator=gen, dtype=torch.float64), alpha=s)
        kinetic = 0.5 * (v * v).view(n_graphs, -1).sum(1)      # one segmented sum: every graph has n_atoms unit masses
        if drift_extra:
            kinetic = kinetic + 1.5 * kT
        _barostat(x, v if rescale_v else None, cell, inv, pbc, virial, kinetic, node_ptr, p0, a, 2.0 * kT * a, 0.0, seed, k, counter, volume)
        if k >= drop * steps and k % every == 0:
            out.append(volume.clone())
    assert int(counter) == 0
    return torch.stack(out)
