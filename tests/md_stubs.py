"""Stub force fields for the integrator and minimiser tests (host and device): independent per-atom wells with the interface of
``ReplayedForceField`` (``pos``, ``node_ptr``, ``evaluate()``, ``check()``, ``grow()``), which can report one overflow."""
import torch

SIZES = (1, 70, 0, 5, 150, 3)      # nodes per graph, as tests/test_gpu_md_kernels.py: one atom, more than a wave, an empty graph


def node_ptr_of(sizes, device=None):
    return torch.tensor([0] + [int(v) for v in torch.tensor(sizes).cumsum(0)], dtype=torch.int64, device=device)


class WellField:
    """E = sum over atoms and components of k d^2 / 2 + quartic k d^4 / 8, d = pos - sites; ``k`` [N, 3] or [N, 1].  The energies
    are summed graph by graph in a fixed order (the same bits every run, on either device).  ``fail_at``: the evaluation (counted
    from 1) that returns garbage and makes the next ``check()`` raise ``EdgeCapacityExceeded``, once."""

    def __init__(self, sizes, k, sites, pos, quartic=0.0, fail_at=None):
        self.pos = pos.clone().contiguous()
        self.k, self.sites, self.quartic = k.to(pos), sites.to(pos), float(quartic)
        self.node_ptr = node_ptr_of(sizes, pos.device)
        self.bounds = [int(v) for v in node_ptr_of(sizes)]
        self.fail_at, self.calls, self.pending, self.grown = fail_at, 0, False, 0

    def evaluate(self):
        self.calls += 1
        n_graphs = len(self.bounds) - 1
        if self.fail_at is not None and self.calls == self.fail_at:
            self.pending, self.fail_at = True, None
            return torch.full((n_graphs,), float("nan")).to(self.pos), torch.full_like(self.pos, 1e6)      # a cut list: garbage
        d = self.pos - self.sites
        per_atom = (0.5 * self.k * d * d + (0.125 * self.quartic) * self.k * d ** 4).sum(1)
        energy = torch.stack([per_atom[a:b].sum() for a, b in zip(self.bounds[:-1], self.bounds[1:])])
        return energy, (-(self.k * d + (0.5 * self.quartic) * self.k * d ** 3)).contiguous()

    def check(self):
        from e3_layers_amd.run.md import EdgeCapacityExceeded

        if self.pos.is_cuda:
            torch.cuda.synchronize()
        if self.pending:
            self.pending = False
            raise EdgeCapacityExceeded("stub")

    def grow(self, factor):
        self.grown += 1
        self.pos = self.pos.clone()      # as the real one: a new static tensor with the same positions


def harmonic_oscillators(n=256, seed=0, dtype=torch.float64, device="cpu"):
    """The equipartition system: ``n`` independent 3-d oscillators in one graph, k in [0.5, 2], m in [0.5, 4], from x = 0."""
    g = torch.Generator().manual_seed(seed)
    k = (0.5 + 1.5 * torch.rand(n, 1, generator=g, dtype=torch.float64)).to(dtype)
    mass = (0.5 + 3.5 * torch.rand(n, generator=g, dtype=torch.float64)).to(dtype)
    zero = torch.zeros(n, 3, dtype=dtype, device=device)
    return WellField((n,), k.to(device), zero, zero), mass.to(device)


def equipartition_ratio(md, kT, burn_in=400, steps=1600):
    """2 <KE> / (3 N kT) over ``steps`` steps after ``burn_in``."""
    md.run(burn_in, check_every=200)
    kinetic = md.run(steps, check_every=200)["kinetic"].double().sum(1).mean()
    return 2.0 * float(kinetic) / (3.0 * md.v.shape[0] * kT)


def quartic_wells(sizes=SIZES, seed=3, dtype=torch.float64, device="cpu", fail_at=None, only=None):
    """The FIRE stub potential: per-atom anisotropic wells k d^2 / 2 + k d^4 / 8 about random sites, per-graph stiffness
    0.3 .. 12 (the graphs converge at different iterations), every atom starting 0.8 off its site.  ``only``: that graph alone
    (the same atoms, sites and stiffness as in the batch)."""
    g = torch.Generator().manual_seed(seed)
    n, n_graphs = sum(sizes), len(sizes)
    sites = torch.randn(n, 3, generator=g, dtype=torch.float64)
    stiff = torch.logspace(torch.log10(torch.tensor(0.3)).item(), torch.log10(torch.tensor(12.0)).item(), n_graphs, dtype=torch.float64)
    seg = torch.repeat_interleave(torch.arange(n_graphs), torch.tensor(sizes))
    k = stiff[seg][:, None] * (0.5 + torch.rand(n, 3, generator=g, dtype=torch.float64))
    off = torch.randn(n, 3, generator=g, dtype=torch.float64)
    pos = sites + 0.8 * off / off.norm(dim=1, keepdim=True)
    if only is not None:
        keep = seg == only
        sizes, k, sites, pos = (sizes[only],), k[keep], sites[keep], pos[keep]
    return WellField(sizes, k.to(dtype).to(device), sites.to(dtype).to(device), pos.to(dtype).to(device), quartic=1.0, fail_at=fail_at)
