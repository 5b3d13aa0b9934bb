"""Host-side logic of the capped neighbour list and the MD driver (no GPU): the ghost-tail formula the fill kernel of
csrc/e3k_nlist.hip computes in-kernel, restated in Python, against ``ghost_sample``; the rollback of ``VelocityVerlet`` with a stub
force field that reports one overflow."""
import pytest
import torch


def _like():
    from e3_layers_amd.data.synthetic import synth_qm9
    from e3_layers_amd.data.loader import samples_of

    return samples_of(synth_qm9(0, 1))[0]


@pytest.mark.parametrize("n_ghost", [2, 3, 4, 7, 32, 65])
def test_ghost_tail_formula_equals_ghost_sample(n_ghost):
    from e3_layers_amd.data.compute_edge import ghost_tail
    from e3_layers_amd.run.graph_step import ghost_sample

    like = _like()
    m = n_ghost - 1
    for n_edges in sorted({0, 1, m, m + 1, 2 * m, 2 * m + 1, 3 * m + 2, 5 * m + 3, 1024}):
        want = ghost_sample(like, n_ghost, n_edges)["edge_index"]
        got = ghost_tail(n_ghost, n_edges)
        assert got.dtype == torch.int64 and got.shape == (2, n_edges)
        assert torch.equal(got, want), (n_ghost, n_edges)
        assert torch.equal(ghost_tail(n_ghost, n_edges, first_node=40), want + 40)
        if n_edges:
            assert int(got.min()) >= 0 and int(got.max()) < n_ghost and bool((got[0] != got[1]).all())


def test_ghost_tail_needs_two_nodes_for_an_edge():
    from e3_layers_amd.data.compute_edge import ghost_tail

    assert ghost_tail(1, 0).shape == (2, 0)
    with pytest.raises(ValueError):
        ghost_tail(1, 3)


def test_edge_capacity_exceeded_is_a_value_error():
    from e3_layers_amd.run.md import EdgeCapacityExceeded

    assert issubclass(EdgeCapacityExceeded, ValueError)


class _StubField:
    """Harmonic wells on the host with the force field's interface; reports an overflow at the ``fail_at``-th evaluation, once."""

    def __init__(self, n=6, fail_at=None):
        g = torch.Generator().manual_seed(5)
        self.pos = torch.randn(n, 3, generator=g, dtype=torch.float64)
        self.node_ptr = torch.tensor([0, 2, n])
        self.k = torch.linspace(0.5, 2.0, n, dtype=torch.float64)[:, None]
        self.fail_at, self.calls, self.pending, self.grown, self.checks = fail_at, 0, False, 0, 0

    def evaluate(self):
        self.calls += 1
        if self.fail_at is not None and self.calls == self.fail_at:
            self.pending, self.fail_at = True, None
            return torch.full((2,), float("nan"), dtype=torch.float64), torch.full_like(self.pos, 1e6)      # a cut list: garbage forces
        e = 0.5 * (self.k * self.pos ** 2).sum(1)
        return torch.stack([e[:2].sum(), e[2:].sum()]), -self.k * self.pos

    def check(self):
        from e3_layers_amd.run.md import EdgeCapacityExceeded

        self.checks += 1
        if self.pending:
            self.pending = False
            raise EdgeCapacityExceeded("stub")

    def grow(self, factor):
        self.grown += 1
        self.pos = self.pos.clone()      # as the real one: a new static tensor with the same positions


@pytest.mark.parametrize("fail_at", [2, 6, 9])
def test_velocity_verlet_rolls_an_overflowed_chunk_back(fail_at):
    from e3_layers_amd.run.md import VelocityVerlet

    def run(fail):
        ff = _StubField(fail_at=fail)
        md = VelocityVerlet(ff, torch.linspace(1.0, 3.0, 6, dtype=torch.float64), dt=0.05)
        md.v.copy_(torch.randn(6, 3, generator=torch.Generator().manual_seed(9), dtype=torch.float64))
        out = md.run(12, check_every=4)
        return ff, md, out

    ff0, md0, out0 = run(None)
    ff1, md1, out1 = run(fail_at)
    assert md0.regrowths == 0 and md0.restores == 0
    assert md1.regrowths == 1 and ff1.grown == 1 and md1.restores == 1      # the snapshot went back once
    assert md1.steps_done == md0.steps_done == 12
    assert torch.isfinite(out1["potential"]).all()                           # the overflowed chunk never reaches the caller
    for key in ("potential", "kinetic"):
        assert torch.equal(out1[key], out0[key]), key
    assert torch.equal(md1.x, md0.x) and torch.equal(md1.v, md0.v)
    # energy conservation of the stub trajectory: the integrator is velocity Verlet
    tot = (out0["potential"] + out0["kinetic"]).sum(1)
    assert float((tot - tot[0]).abs().max()) < 1e-2 * float(tot[0].abs())
