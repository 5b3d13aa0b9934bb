"""The thermostat kick and the FIRE iteration (csrc/e3k_md.hip: e3k_md_kick_langevin, e3k_fire_step) called directly, against
float64 restatements on the shapes of tests/test_gpu_md_kernels.py: graphs of one atom, more than a wave's 64 lanes, none, and rows
behind the real nodes that must not move.

The bound on a normal draw, XI_BOUND.  xi = r cos(2 pi u2), r = sqrt(-2 ln u1); u = 2^-24 is half an fp32 ulp, relative.
  * u1, u2 and 2 u2 are exact (24-bit integers times powers of two), so neither function sees a rounded argument.
  * logf is within ULP_LOG ulp: relative 2 u ULP_LOG on ln u1; the factor -2 is exact; the correctly rounded square root halves the
    relative error and adds u: r is within r u (ULP_LOG + 1).
  * cospif is within ULP_COS ulp of a value of magnitude <= 1: absolute 2 u ULP_COS (ULP_COS = 4, the project's constant for the
    cosine and OpenCL full profile's for cospi).
  * the product rounds once: u |xi| <= u r.
  |xi - xi64| <= r u (ULP_LOG + 1) + r 2 u ULP_COS + r u <= R_MAX u (ULP_LOG + 2 + 2 ULP_COS),  R_MAX = sqrt(48 ln 2) = 5.77
  (u1 >= 2^-24).  With ULP_LOG = 3: 4.5e-6.  ULP_LOG is measured here through torch on the device, on every u1 the kernel can
  form, as tests/test_gpu_edge_matrix.py measures sin and cos (measured on an MI355X: 1.88 ulp); the constant is the integer
  above the measurement, which is OpenCL full profile's 3, and the measurement must stay at or below it.

The full kick adds c v and dt/2 f / m to that: the existing kick test's 1e-6 max |v'| plus (s / sqrt(m_i)) XI_BOUND, node by node;
kinetic energies as there (1e-5).

FIRE: a lane sums at most 3 nodes of 3 products and the butterfly adds 6 levels: a sum of positive terms is within 15 u, the mixing
factor alpha |v| / |f| within (15 + 15) / 2 u + 3 u, and an updated component is three such terms: within 32 u = 1.9e-6 of the
graph's largest component.  The planted P are >= 1e-3 |f| |v| from zero and the planted |dr| >= 1 % from maxstep (asserted on the
float64 side), so fp32 cannot flip a branch."""
import math

import numpy as np
import pytest
import torch

from tests.test_gpu_edge_matrix import ULP_COS, _worst_ulp
from tests.test_gpu_md_kernels import DT, N_GHOST, SIZES, _close, _state
from tests.util import record_measured

pytestmark = pytest.mark.gpu

U24 = 2.0 ** -24
ULP_LOG = 3
R_MAX = math.sqrt(48 * math.log(2))
XI_BOUND = R_MAX * U24 * (ULP_LOG + 2 + 2 * ULP_COS)
SEED = (977 << 32) + 20241017      # both seed words in use


def test_device_logf_is_within_ulp_log(dev):
    """Every u1 = (k + 1) 2^-24 the kernel can form, through torch.log on the device, against numpy float64."""
    u1 = (np.arange(1, 2 ** 24 + 1, dtype=np.float64) * U24).astype(np.float32)
    worst = _worst_ulp(torch.log(torch.from_numpy(u1).to(dev)).cpu().numpy(), np.log(u1.astype(np.float64)))
    print(f"device math library: log worst {worst:.3f} ulp on (0, 1], constant {ULP_LOG}")
    record_measured("test_gpu_md_integrator_kernels", case="device_math_library", family="log", worst_ulp=worst, constant=ULP_LOG)
    assert worst <= ULP_LOG and ULP_LOG <= 3, worst      # (3: the OpenCL full-profile limit)


@pytest.mark.parametrize("word0", [0, 4])
def test_kernel_draws_are_the_float64_formula_on_the_same_hashes(dev, word0):
    """c = 0, s = 1, unit masses, no forces: v = xi.  One graph of 40 000 nodes (625 walks per lane) and the small graphs, three
    draw indices (one beyond 2^32: taken modulo 2^32) -- element by element within XI_BOUND."""
    from e3_layers_amd.data.compute_edge import normal_draw
    from e3_layers_amd.run.md import _kick_langevin

    sizes = SIZES + (40000,)
    n = sum(sizes)
    ptr = torch.tensor([0] + list(np.cumsum(sizes)), dtype=torch.int64, device=dev)
    mass = torch.ones(n + N_GHOST, device=dev)
    worst = 0.0
    for draw in (0, 7, (1 << 32) + 7, 123456789):
        v = torch.full((n + N_GHOST, 3), 3.0, device=dev)
        _kick_langevin(v[:n], None, mass[:n], ptr, 0.0, 0.0, 1.0, SEED, draw, word0, None)
        want = normal_draw(SEED, draw, torch.arange(n)[:, None], word0 + torch.arange(3)[None, :], torch.float64)
        err = float((v[:n].double().cpu() - want).abs().max())
        worst = max(worst, err)
        assert err <= XI_BOUND, (draw, err, XI_BOUND)
        assert bool((v[n:] == 3.0).all())
        if draw == (1 << 32) + 7:
            assert torch.equal(v, last)                     # the draw index is taken modulo 2^32
        last = v
    assert float(want.abs().max()) > 4.0                    # the tails were reached
    print(f"normal draws word0 {word0}: worst |xi - xi64| {worst:.3e}, bound {XI_BOUND:.3e}")
    record_measured("test_gpu_md_integrator_kernels", case=f"xi_word{word0}", worst_abs=worst, bound=XI_BOUND)


def _kick_case(dev, seed):
    n, _, v, f, mass, node_ptr = _state(dev, seed)
    g = torch.Generator().manual_seed(100 + seed)
    c, s = float(torch.rand(1, generator=g)), float(0.2 + torch.rand(1, generator=g))
    energy = torch.randn(len(SIZES), generator=g)
    return n, v, f, mass, node_ptr, c, s, energy


@pytest.mark.parametrize("seed", [1, 2])
def test_thermostat_kick_against_float64(dev, seed):
    from e3_layers_amd.data.compute_edge import normal_draw
    from e3_layers_amd.run.md import _kick_langevin

    n, v, f, mass, node_ptr, c, s, energy = _kick_case(dev, seed)
    n_graphs, draw = len(SIZES), 41
    fd, md, ptr, ed = (t.clone().to(dev).contiguous() for t in (f, mass, node_ptr, energy))

    def run(draw, forces=fd, s=s):
        vd = v.clone().to(dev).contiguous()
        record = torch.full((2, n_graphs + 2), -7.0, device=dev)      # [kinetic | potential], a canary on either side of each row
        _kick_langevin(vd[:n], None if forces is None else forces[:n], md[:n], ptr, DT, c, s, SEED, draw, 0, record[0, 1:-1], ed,
                       record[1, 1:-1])
        torch.cuda.synchronize()
        return vd, record

    vd, record = run(draw)
    c32, s32 = float(np.float32(c)), float(np.float32(s))               # (the kernel takes them as floats)
    xi = normal_draw(SEED, draw, torch.arange(n)[:, None], torch.arange(3)[None, :], torch.float64)
    amp = s32 / mass[:n].double().sqrt()
    v64 = c32 * v[:n].double() + amp[:, None] * xi + 0.5 * DT * f[:n].double() / mass[:n].double()[:, None]
    bound = 1e-6 * float(v64.abs().max()) + amp[:, None] * XI_BOUND
    err = (vd[:n].double().cpu() - v64).abs()
    assert bool((err <= bound).all()), float((err / bound).max())
    per_node = 0.5 * mass[:n].double() * (v64 * v64).sum(1)
    want = torch.stack([per_node[int(node_ptr[g]):int(node_ptr[g + 1])].sum() for g in range(n_graphs)])
    got = record[0, 1:-1].double().cpu()
    assert ((got - want).abs() <= 1e-5 * want.abs()).all(), (got, want)
    assert float(got[SIZES.index(0)]) == 0.0
    assert torch.equal(record[1, 1:-1], ed)
    assert (record[:, 0] == -7.0).all() and (record[:, -1] == -7.0).all()
    assert torch.equal(vd[n:].cpu(), v[n:])                             # the rows behind: untouched, bit for bit
    vd2, record2 = run(draw)
    assert torch.equal(vd2, vd) and torch.equal(record2, record)        # the same bits on a second run
    vd3, _ = run(draw + 1)
    assert not _close(vd3[:n], v64, 1e-3)                               # another draw index lands elsewhere
    # without forces: friction and noise only
    vd4, _ = run(draw, None)
    v64_4 = c32 * v[:n].double() + amp[:, None] * xi
    assert bool(((vd4[:n].double().cpu() - v64_4).abs() <= 1e-6 * float(v64_4.abs().max()) + amp[:, None] * XI_BOUND).all())
    # friction without noise: s = 0 at the case's c, with forces -- nothing is drawn, so the bound's noise term is zero
    vd5, record5 = run(draw, fd, 0.0)
    v64_5 = c32 * v[:n].double() + 0.5 * DT * f[:n].double() / mass[:n].double()[:, None]
    err5 = (vd5[:n].double().cpu() - v64_5).abs()
    print(f"friction alone seed {seed}: worst |v - v64| {float(err5.max()):.3e}, bound {1e-6 * float(v64_5.abs().max()):.3e}")
    assert bool((err5 <= 1e-6 * float(v64_5.abs().max())).all()), float(err5.max())
    per_node5 = 0.5 * mass[:n].double() * (v64_5 * v64_5).sum(1)
    want5 = torch.stack([per_node5[int(node_ptr[g]):int(node_ptr[g + 1])].sum() for g in range(n_graphs)])
    got5 = record5[0, 1:-1].double().cpu()
    assert ((got5 - want5).abs() <= 1e-5 * want5.abs()).all(), (got5, want5)


def test_thermostat_kick_without_thermostat_is_the_plain_kick_bit_for_bit(dev):
    from e3_layers_amd.backend import lib as L

    n, _, v, f, mass, node_ptr = _state(dev, 3)
    fd, md, ptr = (t.clone().to(dev).contiguous() for t in (f, mass, node_ptr))
    va, vb = v.clone().to(dev).contiguous(), v.clone().to(dev).contiguous()
    ka, kb = torch.empty(len(SIZES), device=dev), torch.empty(len(SIZES), device=dev)
    L.check(L.load().e3k_md_kick(L.ptr(va[:n]), L.ptr(fd[:n]), L.ptr(md[:n]), L.ptr(ptr), len(SIZES), n, DT, L.ptr(ka), None, None,
                                 L.stream_ptr()), "e3k_md_kick")
    L.check(L.load().e3k_md_kick_langevin(L.ptr(vb[:n]), L.ptr(fd[:n]), L.ptr(md[:n]), L.ptr(ptr), len(SIZES), n, DT, 1.0, 0.0,
                                          *L.seed_words(SEED), 5, 0, L.ptr(kb), None, None, L.stream_ptr()), "e3k_md_kick_langevin")
    assert torch.equal(va, vb) and torch.equal(ka, kb)


@pytest.mark.parametrize("word0", [0, 4])
def test_score_step_noise_is_the_thermostat_stream_bit_for_bit(dev, word0):
    """``e3k_vpsde_perturb``'s z (D = 3, every node in a real graph) and ``e3k_md_kick_langevin``'s velocities at c = 0, s = 1, unit
    masses, no forces -- 0 v + 1 xi is xi exactly -- for the same seed, draw index and first word: one stream (csrc/e3k_draw.h), so
    ``torch.equal``.  The draw index is a device cell there and an argument here; both take it modulo 2^32."""
    from e3_layers_amd.backend import diffusion_ops
    from e3_layers_amd.run.md import _kick_langevin

    n = sum(SIZES)
    ptr = torch.tensor([0] + list(np.cumsum(SIZES)), dtype=torch.int64, device=dev)
    node_seg = torch.repeat_interleave(torch.arange(len(SIZES), device=dev), torch.tensor(SIZES, device=dev)).contiguous()
    x0 = torch.randn(n, 3, generator=torch.Generator().manual_seed(11)).to(dev)
    mass = torch.ones(n, device=dev)
    for draw in (7, (1 << 32) + 7):
        cell = torch.tensor([draw], dtype=torch.int64, device=dev)
        _, _, z, _ = diffusion_ops.vpsde_perturb(x0, node_seg, len(SIZES), 0.1, 20.0, 1e-3, 1.0, SEED, cell, word0)
        v = torch.full((n, 3), 3.0, device=dev)
        _kick_langevin(v, None, mass, ptr, 0.0, 0.0, 1.0, SEED, draw, word0, None)
        assert float(z.abs().max()) > 1.0                       # (something was drawn)
        assert torch.equal(z, v), (draw, float((z - v).abs().max()))


# ---- FIRE -----------------------------------------------------------------------------------------------------------------------
FIRE = dict(ftol=1e-3, dt_max=0.5, maxstep=0.2, n_min=5, f_inc=1.1, f_dec=0.5, alpha=0.1, f_alpha=0.99)
# what is planted per graph: (name, sign of P, |v|, |f|, state row (dt, alpha, n_pos)); |dr| = dt' |v'| against maxstep = 0.2
CASES = (("downhill_young", +1, 0.5, 2.0, (0.1, 0.1, 2.0)),          # n_pos <= n_min: dt, alpha stay; 0.1 * ~0.6: not clipped
         ("downhill_old", +1, 5.0, 2.0, (0.1, 0.07, 9.0)),           # dt -> 0.11, alpha -> 0.0693; 0.11 * ~5: clipped
         ("uphill", -1, 5.0, 30.0, (0.2, 0.05, 9.0)),                # v <- 0, dt -> 0.1, alpha -> 0.1, n_pos -> 0; 0.1 * 3: clipped
         ("at_rest_capped", 0, 0.0, 0.5, (0.47, 0.1, 7.0)),          # P = 0 is downhill; dt -> min(0.517, 0.5); 0.25 * 0.5: not clipped
         ("frozen", +1, 5.0, None, (0.1, 0.1, 3.0)))                 # fmax = ftol / 2: v <- 0, x and the state's first three stay


def _fire_plant(layout):
    """Case ``(j + layout) % 5`` on the j-th non-empty graph: every case meets graphs of several sizes over the layouts."""
    n, x, v, f, _, node_ptr = _state(None, 20 + layout)
    x, v, f = x.clone(), v.clone(), f.clone()
    state = torch.zeros(len(SIZES), 4)
    state[:, 3] = float("inf")
    names, j = [], 0
    for g, size in enumerate(SIZES):
        a, b = int(node_ptr[g]), int(node_ptr[g + 1])
        if size == 0:
            state[g, :3] = torch.tensor([0.3, 0.08, 4.0])
            names.append("empty")
            continue
        name, sign, vnorm, fnorm, row = CASES[(j + layout) % len(CASES)]
        j += 1
        names.append(name)
        fg = f[a:b]
        if fnorm is None:
            fg *= 0.5 * FIRE["ftol"] / fg.norm(dim=1).max()
        else:
            fg *= fnorm / fg.norm()
        if sign == 0:
            v[a:b] = 0.0
        else:
            r = v[a:b]
            r = r + sign * 0.5 * r.norm() * fg / fg.norm() - (r * fg).sum() * fg / (fg * fg).sum()      # cos(f, v) = +- 0.45
            v[a:b] = r * (vnorm / r.norm())
        state[g, :3] = torch.tensor(row)
    return n, x, v, f, node_ptr, state, names


def _fire_float64(n, x, v, f, node_ptr, state):
    """The contract of include/e3k.h in float64 on the fp32 inputs, with the parameters as the floats the kernel receives."""
    p = {k: (float(np.float32(val)) if k != "n_min" else val) for k, val in FIRE.items()}
    x, v, f, state = x.double().clone(), v.double().clone(), f.double(), state.double().clone()
    branch = []
    for g in range(len(SIZES)):
        a, b = int(node_ptr[g]), int(node_ptr[g + 1])
        fg, vg = f[a:b], v[a:b]
        dt, alpha, n_pos = (float(t) for t in state[g, :3])
        fmax = float(fg.norm(dim=1).max()) if b > a else 0.0
        state[g, 3] = fmax
        if fmax < p["ftol"]:
            v[a:b] = 0.0
            branch.append(("frozen", None))
            continue
        power, fn, vn = float((fg * vg).sum()), float(fg.norm()), float(vg.norm())
        assert power == 0.0 and vn == 0.0 or abs(power) >= 1e-3 * fn * vn
        if power < 0:
            vg = torch.zeros_like(vg)
            dt, alpha, n_pos = dt * p["f_dec"], p["alpha"], 0.0
        else:
            vg = (1.0 - alpha) * vg + alpha * vn * fg / fn
            if n_pos > p["n_min"]:
                dt, alpha = min(dt * p["f_inc"], p["dt_max"]), alpha * p["f_alpha"]
            n_pos += 1.0
        vg = vg + dt * fg
        dr = dt * vg
        norm = float(dr.norm())
        assert abs(norm / p["maxstep"] - 1.0) >= 0.01
        if norm > p["maxstep"]:
            dr = dr * (p["maxstep"] / norm)
        v[a:b], x[a:b] = vg, x[a:b] + dr
        state[g, :3] = torch.tensor([dt, alpha, n_pos], dtype=torch.float64)
        branch.append(("up" if power < 0 else "down", norm > p["maxstep"]))
    return x, v, state, branch


@pytest.mark.parametrize("layout", [0, 1, 2])
def test_fire_step_against_float64(dev, layout):
    from e3_layers_amd.run.md import Fire, _fire_step

    n, x, v, f, node_ptr, state, names = _fire_plant(layout)
    x64, v64, state64, branch = _fire_float64(n, x, v, f, node_ptr, state)
    # every branch of the contract occurs in this one call
    assert set(names) == {c[0] for c in CASES} | {"empty"}
    assert {b for b in branch} >= {("frozen", None), ("up", True), ("down", True), ("down", False)}
    capped = names.index("at_rest_capped")
    assert float(state64[capped, 0]) == float(np.float32(FIRE["dt_max"])) and float(state64[names.index("downhill_old"), 0]) < 0.2

    class _Params:
        pass

    fire = _Params()
    fire.__dict__.update(FIRE)
    xd, vd, fd, ptr, sd = (t.clone().to(dev).contiguous() for t in (x, v, f, node_ptr, state))
    n_graphs = len(SIZES)
    energy = torch.randn(n_graphs, generator=torch.Generator().manual_seed(4)).to(dev)
    record = torch.full((2, n_graphs + 2), -7.0, device=dev)            # [energy | fmax], a canary on either side of each row
    _fire_step(xd[:n], vd[:n], fd[:n], ptr, sd, fire, energy, record[0, 1:-1], record[1, 1:-1])
    torch.cuda.synchronize()
    tol = 32 * U24
    for g, name in enumerate(names):
        a, b = int(node_ptr[g]), int(node_ptr[g + 1])
        got_x, got_v = xd[a:b].double().cpu(), vd[a:b].double().cpu()
        if name == "frozen":
            assert torch.equal(xd[a:b].cpu(), x[a:b]) and bool((got_v == 0).all())
        elif name != "empty":
            assert float((got_v - v64[a:b]).abs().max()) <= tol * float(v64[a:b].abs().max()), name
            assert float((got_x - x64[a:b]).abs().max()) <= tol * float(x64[a:b].abs().max()), name
            assert not torch.equal(xd[a:b].cpu(), x[a:b])
        row, want = sd[g].double().cpu(), state64[g]
        assert bool(((row - want).abs() <= 4 * U24 * want.abs()).all()), (name, row, want)
        assert float(row[2]) == float(want[2])                          # n_pos: small integers, exact
    assert float(sd[names.index("empty"), 3]) == 0.0
    assert torch.equal(record[0, 1:-1], energy) and torch.equal(record[1, 1:-1], sd[:, 3])
    assert (record[:, 0] == -7.0).all() and (record[:, -1] == -7.0).all()
    assert torch.equal(xd[n:].cpu(), x[n:]) and torch.equal(vd[n:].cpu(), v[n:])      # the rows behind: untouched
    # the same bits on a second run from the same state, with no records wanted
    xd2, vd2, sd2 = (t.clone().to(dev).contiguous() for t in (x, v, state))
    _fire_step(xd2[:n], vd2[:n], fd[:n], ptr, sd2, fire)
    assert torch.equal(xd2, xd) and torch.equal(vd2, vd) and torch.equal(sd2, sd)
