"""Star systems for the bond-constraint tests (host and device): graphs of stars with 1..4 satellites and free atoms, every atom
in a well of its own (``md_stubs.WellField``), so the constraints carry force.  Built in float64 on the host once per call, with
a fixed seed; ``dtype`` / ``device`` only convert."""
import math

import torch

from tests.md_stubs import WellField, node_ptr_of

# per graph: (satellite counts of its stars, free atoms).  One atom; every star size, shuffled; an empty graph; one CH4; more than
# 64 stars (a lane of the graph's wave takes two) of every size; free atoms only; pairs only.
GRAPHS = (
    ((), 1),
    ((4,) * 6 + (3,) * 5 + (2,) * 4 + (1,) * 3, 2),
    ((), 0),
    ((4,), 0),
    ((2,) * 40 + (1,) * 20 + (3,) * 10 + (4,) * 5, 23),
    ((), 3),
    ((1,) * 9, 1),
)
SIZES = tuple(sum(k + 1 for k in stars) + free for stars, free in GRAPHS)
TETRAHEDRON = torch.tensor([[1.0, 1.0, 1.0], [1.0, -1.0, -1.0], [-1.0, 1.0, -1.0], [-1.0, -1.0, 1.0]], dtype=torch.float64) / math.sqrt(3.0)


def _rotation(gen):
    q, r = torch.linalg.qr(torch.randn(3, 3, generator=gen, dtype=torch.float64))
    return q * torch.sign(torch.diagonal(r))[None, :]


def star_geometry(graphs=GRAPHS, seed=0, masses="hydrogen", spread=12.0):
    """(pos [N, 3] float64 with coordinates of magnitude ~``spread``, pairs [C, 2] (in a shuffled order, centre and satellite in
    either place), mass [N] float64, sizes).  The atoms of a graph are shuffled, so the tables are no identity.  Satellites sit
    0.9 .. 1.5 from their centre along tetrahedral directions (randomly rotated, jittered by 0.15).  ``masses``: "hydrogen" --
    centres 12 or 16, satellites 1, free atoms 12; "random" -- 0.5 .. 4."""
    gen = torch.Generator().manual_seed(seed)
    pos, pairs, mass, base = [], [], [], 0
    for stars, free in graphs:
        n = sum(k + 1 for k in stars) + free
        perm = torch.randperm(n, generator=gen) + base
        x = torch.zeros(n, 3, dtype=torch.float64)
        m = torch.full((n,), 12.0, dtype=torch.float64)
        at = 0
        for s, k in enumerate(stars):
            centre = spread * (2.0 * torch.rand(3, generator=gen, dtype=torch.float64) - 1.0)
            dirs = TETRAHEDRON[:k] @ _rotation(gen).T + 0.15 * torch.randn(k, 3, generator=gen, dtype=torch.float64)
            dirs = dirs / dirs.norm(dim=1, keepdim=True)
            x[at] = centre
            x[at + 1:at + 1 + k] = centre + (0.9 + 0.6 * torch.rand(k, 1, generator=gen, dtype=torch.float64)) * dirs
            m[at] = 12.0 if s % 2 == 0 else 16.0
            m[at + 1:at + 1 + k] = 1.0
            for j in range(k):
                pair = (int(perm[at]), int(perm[at + 1 + j]))
                pairs.append(pair if (s + j) % 2 == 0 else pair[::-1])
            at += k + 1
        x[at:] = spread * (2.0 * torch.rand(n - at, 3, generator=gen, dtype=torch.float64) - 1.0)
        if masses == "random":
            m = 0.5 + 3.5 * torch.rand(n, generator=gen, dtype=torch.float64)
        full_x, full_m = torch.zeros_like(x), torch.zeros_like(m)
        full_x[perm - base], full_m[perm - base] = x, m
        pos.append(full_x)
        mass.append(full_m)
        base += n
    pairs = torch.tensor(pairs, dtype=torch.int64).reshape(-1, 2)
    pairs = pairs[torch.randperm(pairs.shape[0], generator=gen)]
    return torch.cat(pos), pairs, torch.cat(mass), tuple(sum(k + 1 for k in stars) + free for stars, free in graphs)


def star_wells(graphs=GRAPHS, seed=0, masses="hydrogen", dtype=torch.float64, device="cpu", quartic=0.0, offset=0.25, tol=1e-5,
               max_iter=32, constrained=True, fail_at=None):
    """(field, mass, constraints, v0): every atom in a well of stiffness 0.5 .. 2 whose site lies ``offset`` from the atom's
    starting position (the wells pull on the bonds), starting velocities of 0.3 / sqrt(m) per component -- NOT yet projected:
    ``md.project()`` does that.  ``constrained`` False: the same system with an empty constraint set."""
    from e3_layers_amd.run.md import BondConstraints

    pos, pairs, mass, sizes = star_geometry(graphs, seed, masses)
    gen = torch.Generator().manual_seed(seed + 1000)
    n = pos.shape[0]
    k = 0.5 + 1.5 * torch.rand(n, 3, generator=gen, dtype=torch.float64)
    off = torch.randn(n, 3, generator=gen, dtype=torch.float64)
    sites = pos + offset * off / off.norm(dim=1, keepdim=True)
    v0 = 0.3 * torch.randn(n, 3, generator=gen, dtype=torch.float64) / mass.sqrt()[:, None]
    pos_d = pos.to(dtype).to(device)
    field = WellField(sizes, k.to(dtype).to(device), sites.to(dtype).to(device), pos_d, quartic=quartic, fail_at=fail_at)
    mass_d = mass.to(dtype).to(device)
    con = BondConstraints(pairs if constrained else pairs[:0], pos=pos_d, node_ptr=node_ptr_of(sizes), masses=mass_d, tol=tol,
                          max_iter=max_iter)
    return field, mass_d, con, v0.to(dtype).to(device)


def bond_errors(con, x, v):
    """In float64 from the stored numbers: (relative length errors |d - d0| / d0 [C], |r.v_rel| [C], d0 (|v_c| + |v_s|) [C],
    |r| (|v_c| + |v_s|) [C])."""
    pairs, d0 = con.pairs.cpu(), con.lengths.double().cpu()
    x, v = x.detach().double().cpu(), v.detach().double().cpu()
    r = x[pairs[:, 1]] - x[pairs[:, 0]]
    speed = v[pairs[:, 0]].norm(dim=1) + v[pairs[:, 1]].norm(dim=1)
    return (r.norm(dim=1) - d0).abs() / d0, (r * (v[pairs[:, 1]] - v[pairs[:, 0]])).sum(1).abs(), d0 * speed, r.norm(dim=1) * speed


def assert_constraints_hold(con, x, v, eps, where=""):
    """Every bond within the stopping rules at precision ``eps`` (the unit roundoff of the run's dtype):
    lengths: |d^2 - d0^2| <= 2 tol d0^2 gives |d - d0| / d0 <= tol (1 + tol); to that, the rounding of the two stored end points,
    2 sqrt(3) (2 eps) max|x| / d0 (the bound of the issue: 2^-23 is 2 eps of fp32);
    velocities: |r.v_rel| <= tol d0 (|v_c| + |v_s|) as the sweeps evaluated it; recomputed in float64 from the stored numbers it
    differs by the rounding of a three-term dot product and of r and v_rel themselves: at most 8 eps |r| (|v_c| + |v_s|).
    Returns the worst length error and the worst |r.v_rel| / (d0 (|v_c| + |v_s|))."""
    length, rv, scale, rscale = bond_errors(con, x, v)
    if length.numel() == 0:
        return 0.0, 0.0
    d0 = con.lengths.double().cpu()
    xmax = float(x.detach().abs().max())
    bound = con.tol * (1 + con.tol) + 2 * math.sqrt(3.0) * 2 * eps * xmax / d0
    assert bool((length <= bound).all()), (where, float((length / bound).max()), float(length.max()))
    assert bool((rv <= con.tol * scale + 8 * eps * rscale).all()), (where, float((rv / (con.tol * scale + 8 * eps * rscale)).max()))
    return float(length.max()), float((rv / scale.clamp_min(1e-300)).max())


def one_star_type(n_stars=64, n_sat=3, seed=5, dtype=torch.float64, device="cpu", tol=1e-5):
    """The equipartition system: ``n_stars`` stars of 1 + ``n_sat`` atoms in ONE graph, every atom in an isotropic well of its own
    about its starting position, k in [0.5, 2], centres of mass 12 or 16 and satellites of mass 1 (heavy centres: the sweeps
    converge in a few passes, which is what keeps 2 600 steps of the torch path quick): (field, mass, constraints)."""
    from e3_layers_amd.run.md import BondConstraints

    graphs = (((n_sat,) * n_stars, 0),)
    pos, pairs, mass, sizes = star_geometry(graphs, seed, "hydrogen")
    gen = torch.Generator().manual_seed(seed + 2000)
    k = 0.5 + 1.5 * torch.rand(pos.shape[0], 1, generator=gen, dtype=torch.float64)
    pos_d = pos.to(dtype).to(device)
    field = WellField(sizes, k.to(dtype).to(device), pos_d, pos_d)
    mass_d = mass.to(dtype).to(device)
    return field, mass_d, BondConstraints(pairs, pos=pos_d, node_ptr=node_ptr_of(sizes), masses=mass_d, tol=tol)
