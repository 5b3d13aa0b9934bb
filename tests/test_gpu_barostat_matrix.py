"""``e3k_barostat_step`` (csrc/e3k_barostat.hip, one kernel) through the C ABI against float64 / exact arithmetic on the CPU, element by
element.  One case per call; every output word is compared, none masked; every launching case runs twice and the two results must be
the same bits.  Rows behind the real nodes and the ghost graph's rows of cell / inv_cell hold sentinels that must not move.

Reference (``reference``; u = 2^-24, eps = 2^-53).  float64 numpy restates include/e3k.h, "Barostat": V, P, d_eps, mu per graph with
``xi = normal_draw(seed, draw, 0xFFFFFFFE, g)`` in float64; x, v, cell = mu x, v / mu, mu cell in float64.  Which graphs freeze is
decided on the reference's own new cell ``f32(f32(mu) cell)`` with exact rational arithmetic (``fractions``), and every case is
asserted to sit at least 1e-3 (relative) off ``min_width`` on every periodic axis, so that fp32 cannot flip the decision.

Bounds, derived:
  * x, v, cell: the factor is rounded to fp32 (u), 1 / mu once more in double (nothing), the product once (u): 3 u of the magnitude
    covers both, plus the draw: the device's fp32 xi is within XI_BOUND (tests/test_gpu_md_integrator_kernels.py, analytic) of the
    float64 one, d_eps moves by sigma XI_BOUND with sigma = sqrt(b / V), and mu by the factor exp(sigma XI_BOUND / 3).  The double
    arithmetic up to mu (a determinant, a division, an exp) adds 64 eps relative: counted.
  * inv_cell: against the EXACT inverse of the fp32 cell the device wrote (what the periodic builder will read): one fp32 rounding,
    u |inv_ij|, plus the double adjugate and determinant: each cofactor is two products and a difference, 3 eps of its majorant
    |p| + |q|; the determinant 8 eps of its own majorant, relative to |det|; the division eps.  Where the exact inverse is zero and
    its majorant is zero too (both products of the cofactor vanish) the output must be exactly zero.
  * volume, pressure: 1e-14 of their majorants (the sum of the absolute products of the determinant; (2 K + sum |w_kk|) / 3 V).
  * a frozen graph's rows of x, v, cell, inv_cell are the input's bits; volume = the old V; pressure = the computed P (not finite
    where the plant makes it so); the counter = its start + the frozen graphs.

``CASES`` is a plain table; tests/test_npt_host.py holds it to the kernels e3k_barostat.o ships and to the header, shows the bounds
to hold for a float32 numpy model of the kernel (products unfused) and to be sharp against planted mutants -- no GPU needed there."""
import math
import zlib
from fractions import Fraction

import numpy as np
import pytest
import torch

from tests.test_gpu_pbc_force_field import CELLS
from tests.util import record_measured

E3K_OK, E3K_ERR_INVALID = 0, -1
U24, EPS = 2.0 ** -24, 2.0 ** -53
f32, f64 = np.float32, np.float64
SEED = (977 << 32) + 20241017      # both seed words in use
MIN_WIDTH = 2.0 * 4.0 * (1.0 + 1e-3)      # r_max = 4: 8.008
BAROSTAT_SRC = 0xFFFFFFFE
FN, KERNEL = "e3k_barostat_step", "barostat_step_kernel"


def _xi_bound():
    from tests.test_gpu_md_integrator_kernels import XI_BOUND

    return XI_BOUND


def case(id_, why, sizes, cells, b=0.0, vnull=False, records=True, counter0=0, p0=0.1, a=1.0, draw=3, ptr=None, plants=None):
    """``sizes``: nodes per graph; ``cells``: per graph "ortho" (CELLS[0], 9.0 wide), "tri" (CELLS[1]) -- a trailing number scales it,
    "ortho*1.3" -- "zero" (all zero, no periodic axis) or "singular" (two equal rows, periodic); ``plants``: {graph: "nonfinite_virial"
    | "nan_offdiagonal"}; ``ptr``: "garbage": the first entry of node_ptr is -3 and the last n + 2"""
    assert len(sizes) == len(cells)
    return dict(id=id_, kind="step", why=why, sizes=tuple(sizes), cells=tuple(cells), b=float(b), vnull=vnull, records=records,
                counter0=counter0, p0=float(p0), a=float(a), draw=draw, ptr=ptr, plants=plants or {}, funcs={FN}, kernels={KERNEL})


def refuse(id_, why, rc=E3K_ERR_INVALID, **change):
    c = case(id_, why, (3, 4), ("ortho", "tri"), b=0.5)
    c.update(kind="refuse", rc=rc, change=change, kernels=set())
    return c


ALT = ("ortho*1.1", "tri", "ortho*1.25", "tri*1.15", "ortho", "tri*1.3", "ortho*1.2", "tri*1.05", "ortho*1.4")
CASES = [
    case("G1_n1", "one graph of one atom: three live lanes", (1,), ("ortho",)),
    case("G1_n0", "an empty graph: its cell is still rescaled, nothing else is touched", (0,), ("tri",), b=0.8),
    case("G1_n85", "255 components: one short of the workgroup's trip; noise; v NULL, records NULL, the counter starts at 7", (85,),
         ("tri",), b=1.0, vnull=True, records=False, counter0=7),
    case("G1_n86", "258 components: lanes 0 and 1 take a second trip", (86,), ("ortho*1.2",), b=1.0),
    case("G5", "five graphs, an empty one first and last, noise: every graph its own draw", (0, 200, 85, 600, 0), ALT[:5], b=1.0),
    case("G5_berendsen", "the same shapes, b = 0 and v NULL: the deterministic limit", (0, 200, 85, 600, 0), ALT[:5], vnull=True),
    case("G9_garbage_ptr", "nine graphs; node_ptr starts at -3 and ends at n + 2: clamped to [0, n], the rows behind n stay",
         (0, 1, 86, 85, 200, 1, 600, 3, 0), ALT, b=0.6, ptr="garbage", counter0=7),
    case("zero_cell", "an all-zero cell without a periodic axis between two live graphs: V = 0, frozen and counted, the zero inverse "
         "stays; the neighbours move", (86, 5, 200), ("ortho*1.1", "zero", "tri"), b=1.0),
    case("freeze_singular", "V = 0 with periodic axes (two equal lattice vectors): frozen, counted, P not finite", (85, 7, 86),
         ("tri", "singular", "ortho*1.1"), b=1.0),
    case("freeze_nonfinite_virial", "an infinite diagonal virial word freezes its graph; a NaN in an off-diagonal word is never read",
         (20, 86, 9, 200), ("ortho*1.1", "tri", "ortho*1.3", "tri*1.2"), b=0.5, plants={1: "nonfinite_virial", 2: "nan_offdiagonal"},
         records=True, counter0=7),
    case("freeze_narrow", "p0 = 0.6 shrinks every cell by a seventh: the 9.0-wide one would fall under 8.008 and is frozen, the wider "
         "ones follow the pressure", (86, 200, 1), ("ortho", "tri*1.2", "ortho*1.3"), p0=0.6),
    case("freeze_narrow_noise", "the same under noise at p0 = 0.7, two narrow cells, the counter from 7", (5, 86, 85, 3), ("ortho", "tri*1.3",
         "ortho", "ortho*1.4"), p0=0.7, b=0.05, counter0=7, vnull=True),
    refuse("noop_G0", "G == 0: E3K_OK and no launch", rc=E3K_OK, G=0),
    refuse("refuse_G_negative", "G < 0", G=-1),
    refuse("refuse_n_negative", "n < 0", n=-1),
    refuse("refuse_a_negative", "a < 0", a=-0.5),
    refuse("refuse_a_nan", "a not a number", a=float("nan")),
    refuse("refuse_a_inf", "a infinite", a=float("inf")),
    refuse("refuse_b_negative", "b < 0", b=-1.0),
    refuse("refuse_b_nan", "b not a number", b=float("nan")),
    refuse("refuse_b_inf", "b infinite", b=float("inf")),
    refuse("refuse_min_width_negative", "min_width < 0", min_width=-1.0),
] + [refuse(f"refuse_null_{k}", f"{k} NULL with G > 0", **{k: None}) for k in
     ("x", "cell", "inv_cell", "pbc", "virial", "kinetic", "node_ptr", "counter")]


def table_kernels():
    return set().union(*(c["kernels"] for c in CASES))


def table_functions():
    return set().union(*(c["funcs"] for c in CASES))


# ---------------------------------------------------------------------------------------------------------------------------------
# exact 3 x 3 arithmetic on fp32 / float64 values
def _frac(c9):
    return [Fraction(float(v)) for v in c9]


def _det_exact(c):
    return c[0] * (c[4] * c[8] - c[5] * c[7]) - c[1] * (c[3] * c[8] - c[5] * c[6]) + c[2] * (c[3] * c[7] - c[4] * c[6])


_COF = ((4, 8, 5, 7), (2, 7, 1, 8), (1, 5, 2, 4), (5, 6, 3, 8), (0, 8, 2, 6), (2, 3, 0, 5), (3, 7, 4, 6), (1, 6, 0, 7), (0, 4, 1, 3))


def exact_inverse(c9):
    """(inverse [9] float64, its majorant [9], |det| float64, the determinant's majorant) of a cell given as 9 floats: rational
    arithmetic, rounded once; None where the determinant is zero"""
    c = _frac(c9)
    det = _det_exact(c)
    a = [abs(v) for v in c]
    det_maj = a[0] * (a[4] * a[8] + a[5] * a[7]) + a[1] * (a[3] * a[8] + a[5] * a[6]) + a[2] * (a[3] * a[7] + a[4] * a[6])
    if det == 0:
        return None, None, 0.0, float(det_maj)
    inv = [float((c[p] * c[q] - c[r] * c[s]) / det) for p, q, r, s in _COF]
    maj = [float((a[p] * a[q] + a[r] * a[s]) / abs(det)) for p, q, r, s in _COF]
    return np.array(inv), np.array(maj), float(abs(det)), float(det_maj)


def widths(inv9):
    m = np.asarray(inv9, f64).reshape(3, 3)
    with np.errstate(divide="ignore"):
        return 1.0 / np.sqrt((m * m).sum(0))


def _cell_of(spec):
    name, _, scale = spec.partition("*")
    if name == "zero":
        return np.zeros(9, f32)
    if name == "singular":
        return np.array([9.0, 0.5, 0.0, 9.0, 0.5, 0.0, 0.0, 0.0, 10.0], f32)
    base = CELLS[0] if name == "ortho" else CELLS[1]
    return (base.numpy().reshape(9) * float(scale or 1.0)).astype(f32)


def inputs(c):
    """numpy operands: x, v [n + 2, 3] (two sentinel rows behind), cell, inv_cell [G + 1, 9], pbc [G + 1, 3] (a sentinel ghost row),
    virial [G, 9], kinetic [G] fp32, node_ptr [G + 1] int64"""
    rng = np.random.default_rng(zlib.crc32(c["id"].encode()))
    sizes = np.array(c["sizes"], np.int64)
    G, n = len(sizes), int(sizes.sum())
    x = np.concatenate([rng.uniform(-12.0, 12.0, (n, 3)), np.full((2, 3), 555.0)]).astype(f32)
    v = np.concatenate([rng.standard_normal((n, 3)), np.full((2, 3), -555.0)]).astype(f32)
    cell = np.stack([_cell_of(s) for s in c["cells"]] + [np.full(9, 77.0, f32)])
    inv = np.full((G + 1, 9), 66.0, f32)
    for g in range(G):
        e = exact_inverse(cell[g])[0]
        inv[g] = 0.0 if e is None else e.astype(f32)
    pbc = np.ones((G + 1, 3), np.int32)
    for g, s in enumerate(c["cells"]):
        if s == "zero":
            pbc[g] = 0
    virial = (50.0 * rng.standard_normal((G, 9))).astype(f32)
    kinetic = rng.uniform(100.0, 300.0, G).astype(f32)
    for g, plant in c["plants"].items():
        if plant == "nonfinite_virial":
            virial[g, 4] = np.inf
        elif plant == "nan_offdiagonal":
            virial[g, 1] = virial[g, 5] = np.nan
    node_ptr = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    if c["ptr"] == "garbage":
        node_ptr[0], node_ptr[-1] = -3, n + 2
    return dict(x=x, v=v, cell=cell, inv_cell=inv, pbc=pbc, virial=virial, kinetic=kinetic, node_ptr=node_ptr, G=G, n=n,
                bounds=np.clip(node_ptr, 0, n))


def draws(c, G, with_graph=True):
    """float64 xi [G] of the case's (seed, draw)"""
    from e3_layers_amd.data.compute_edge import normal_draw

    word = torch.arange(G, dtype=torch.int64) if with_graph else torch.zeros(G, dtype=torch.int64)
    return normal_draw(SEED, c["draw"], BAROSTAT_SRC, word, torch.float64).numpy()


def reference(c, inp):
    """per graph: mu (float64; 1 where frozen), frozen, P, the old V, sigma -- and the margin of the width decisions"""
    G = inp["G"]
    xi = draws(c, G) if c["b"] > 0 else np.zeros(G)
    mu, frozen, prs, vol, sigma = np.ones(G), np.zeros(G, bool), np.zeros(G), np.zeros(G), np.zeros(G)
    margin = np.inf
    for g in range(G):
        old = inp["cell"][g]
        vol[g] = exact_inverse(old)[2]
        w = inp["virial"][g].astype(f64)
        with np.errstate(all="ignore"):
            prs[g] = (2.0 * f64(inp["kinetic"][g]) + ((w[0] + w[4]) + w[8])) / (3.0 * vol[g])
            sigma[g] = math.sqrt(c["b"] / vol[g]) if vol[g] > 0 else np.inf
            d_eps = c["a"] * (prs[g] - c["p0"]) + (sigma[g] * xi[g] if c["b"] > 0 else 0.0)
            m = np.exp(d_eps / 3.0)
        if vol[g] == 0 or not np.isfinite(prs[g]) or not np.isfinite(d_eps) or not np.isfinite(m):
            frozen[g] = True
            continue
        new = (f32(m) * old).astype(f32)
        inv = exact_inverse(new)[0]
        assert inv is not None
        w_new = widths(inv)
        periodic = inp["pbc"][g] != 0
        if periodic.any():
            margin = min(margin, float(np.abs(w_new[periodic] / MIN_WIDTH - 1.0).min()))
        if (periodic & ~(w_new > MIN_WIDTH)).any():
            frozen[g] = True
            continue
        mu[g] = m
    return dict(mu=mu, frozen=frozen, pressure=prs, volume=vol, sigma=sigma, margin=margin)


def expected(c, inp, ref, got):
    """worst error / bound over every output word of ``got`` (dict of numpy arrays as ``_call`` returns); inf where a word that has
    no tolerance (a frozen row, a sentinel, an exact zero, the counter) is wrong"""
    G, n, bounds = inp["G"], inp["n"], inp["bounds"]
    worst = 0.0

    def same(a, b):
        return a.shape == b.shape and np.array_equal(a.view(np.int32), b.view(np.int32))

    def close(a, want, bound):
        nonlocal worst
        err = np.abs(np.asarray(a, f64) - want)
        if not np.isfinite(np.asarray(a, f64)).all():
            worst = np.inf
            return
        live = bound > 0
        if (err[~live] != 0).any():
            worst = np.inf
        if live.any():
            worst = max(worst, float((err[live] / bound[live]).max()))

    if got["counter"] != c["counter0"] + int(ref["frozen"].sum()):
        return np.inf
    if not (same(got["x"][n:], inp["x"][n:]) and same(got["cell"][G:], inp["cell"][G:]) and same(got["inv_cell"][G:], inp["inv_cell"][G:])):
        return np.inf
    if c["vnull"]:
        if not same(got["v"], inp["v"]):
            return np.inf
    elif not same(got["v"][n:], inp["v"][n:]):
        return np.inf
    touched = np.zeros(n, bool)
    for g in range(G):
        lo, hi = int(bounds[g]), int(max(bounds[g], bounds[g + 1]))
        touched[lo:hi] = True
        rows = slice(lo, hi)
        if ref["frozen"][g]:
            if not (same(got["x"][rows], inp["x"][rows]) and same(got["v"][rows], inp["v"][rows]) and
                    same(got["cell"][g], inp["cell"][g]) and same(got["inv_cell"][g], inp["inv_cell"][g])):
                return np.inf
            if c["records"]:
                if got["volume"][g] != ref["volume"][g]:
                    return np.inf
                p = ref["pressure"][g]
                if np.isfinite(p):
                    w = np.abs(inp["virial"][g].astype(f64))
                    close(got["pressure"][g:g + 1], np.array([p]), np.array([1e-14 * (2.0 * inp["kinetic"][g] + w[0] + w[4] + w[8]) /
                                                                            (3.0 * ref["volume"][g])]))
                elif np.isfinite(got["pressure"][g]):
                    return np.inf
            continue
        mu = ref["mu"][g]
        rel = 3.0 * U24 + 64.0 * EPS + math.expm1(ref["sigma"][g] * _xi_bound() / 3.0) * (1.0 if c["b"] > 0 else 0.0)
        for name, factor in (("x", mu), ("v", 1.0 / mu)):
            if name == "v" and c["vnull"]:
                continue
            want = factor * inp[name][rows].astype(f64)
            close(got[name][rows], want, rel * np.abs(want))
        want = mu * inp["cell"][g].astype(f64)
        close(got["cell"][g], want, rel * np.abs(want))
        inv, maj, det, det_maj = exact_inverse(got["cell"][g])
        if inv is None:
            return np.inf
        close(got["inv_cell"][g], inv, U24 * np.abs(inv) + EPS * (3.0 * maj + (8.0 * det_maj / det + 1.0) * np.abs(inv)))
        if c["records"]:
            close(got["volume"][g:g + 1], np.array([det]), np.array([1e-14 * det_maj]))
            w = np.abs(inp["virial"][g].astype(f64))
            close(got["pressure"][g:g + 1], ref["pressure"][g:g + 1], np.array([1e-14 * (2.0 * inp["kinetic"][g] + w[0] + w[4] + w[8]) /
                                                                                (3.0 * ref["volume"][g])]))
    if not (same(got["x"][:n][~touched], inp["x"][:n][~touched]) and same(got["v"][:n][~touched], inp["v"][:n][~touched])):
        return np.inf
    return worst


# ---------------------------------------------------------------------------------------------------------------------------------
# the float32 model (tests/test_npt_host.py): the kernel operation for operation, products unfused, mu in numpy float64
def model32(c, inp, mutant=None):
    """mutants: "mu_on_v" (v scaled by mu), "inverse_of_old_cell", "noise_word_without_graph", "width_on_old_cell" """
    G, bounds = inp["G"], inp["bounds"]
    out = {k: inp[k].copy() for k in ("x", "v", "cell", "inv_cell")}
    out.update(volume=np.full(G, np.nan), pressure=np.full(G, np.nan), counter=c["counter0"])
    xi = draws(c, G, with_graph=mutant != "noise_word_without_graph").astype(f32) if c["b"] > 0 else np.zeros(G, f32)
    for g in range(G):
        old = inp["cell"][g]
        o = old.astype(f64)
        vol = abs(o[0] * (o[4] * o[8] - o[5] * o[7]) - o[1] * (o[3] * o[8] - o[5] * o[6]) + o[2] * (o[3] * o[7] - o[4] * o[6]))
        w = inp["virial"][g].astype(f64)
        with np.errstate(all="ignore"):
            p = (2.0 * f64(inp["kinetic"][g]) + ((w[0] + w[4]) + w[8])) / (3.0 * vol)
            noise = np.sqrt(c["b"] / vol) * f64(xi[g]) if c["b"] > 0 else 0.0
            d_eps = c["a"] * (p - c["p0"]) + noise
            mu = np.exp(d_eps / 3.0)
        frozen = vol == 0 or not np.isfinite(p) or not np.isfinite(d_eps) or not np.isfinite(mu)
        new_vol = vol
        if not frozen:
            mu_f, inv_mu_f = f32(mu), f32(1.0 / mu)
            new = (mu_f * old).astype(f32)
            src = (old if mutant == "inverse_of_old_cell" else new).astype(f64)
            det = src[0] * (src[4] * src[8] - src[5] * src[7]) - src[1] * (src[3] * src[8] - src[5] * src[6]) + \
                src[2] * (src[3] * src[7] - src[4] * src[6])
            if det == 0 or not np.isfinite(det):
                frozen = True
            else:
                inv = np.array([src[p_] * src[q] - src[r] * src[s] for p_, q, r, s in _COF]) / det
                tested = inp["inv_cell"][g].astype(f64) if mutant == "width_on_old_cell" else inv
                if ((inp["pbc"][g] != 0) & ~(widths(tested) > MIN_WIDTH)).any():
                    frozen = True
                new_vol = abs(det)
        if frozen:
            out["counter"] += 1
            out["volume"][g], out["pressure"][g] = vol, p
            continue
        out["volume"][g], out["pressure"][g] = new_vol, p
        out["cell"][g], out["inv_cell"][g] = new, inv.astype(f32)
        rows = slice(int(bounds[g]), int(max(bounds[g], bounds[g + 1])))
        out["x"][rows] = (mu_f * inp["x"][rows]).astype(f32)
        if not c["vnull"]:
            out["v"][rows] = ((mu_f if mutant == "mu_on_v" else inv_mu_f) * inp["v"][rows]).astype(f32)
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
def _call(c, inp, dev):
    """(status, outputs as numpy: x, v, cell, inv_cell, volume, pressure, counter)"""
    from e3_layers_amd.backend import lib as L

    change = c.get("change", {})
    names = ("x", "v", "cell", "inv_cell", "pbc", "virial", "kinetic", "node_ptr")
    t = {k: torch.from_numpy(inp[k].copy()).to(dev) for k in names}
    t["counter"] = torch.full((1,), c["counter0"], dtype=torch.int32, device=dev)
    t["volume"] = torch.full((max(inp["G"], 1),), float("nan"), dtype=torch.float64, device=dev)
    t["pressure"] = torch.full_like(t["volume"], float("nan"))
    arg = {k: L.ptr(v) for k, v in t.items()}
    if c["vnull"]:
        arg["v"] = None
    if not c["records"]:
        arg["volume"] = arg["pressure"] = None
    for k, v in change.items():
        if v is None:
            arg[k] = None
    lo, hi = L.seed_words(SEED)
    status = L.load().e3k_barostat_step(arg["x"], arg["v"], arg["cell"], arg["inv_cell"], arg["pbc"], arg["virial"], arg["kinetic"],
                                        arg["node_ptr"], change.get("G", inp["G"]), change.get("n", inp["n"]), c["p0"],
                                        change.get("a", c["a"]), change.get("b", c["b"]), change.get("min_width", MIN_WIDTH), lo, hi,
                                        c["draw"], arg["counter"], arg["volume"], arg["pressure"], L.stream_ptr())
    torch.cuda.synchronize()
    out = {k: t[k].cpu().numpy() for k in ("x", "v", "cell", "inv_cell", "volume", "pressure")}
    out["counter"] = int(t["counter"].item())
    return status, out


@pytest.mark.gpu
@pytest.mark.parametrize("cid", [c["id"] for c in CASES])
def test_barostat_step_case(dev, cid):
    c = next(c for c in CASES if c["id"] == cid)
    inp = inputs(c)
    status, got = _call(c, inp, dev)
    if c["kind"] == "refuse":
        assert status == c["rc"], status
        for k in ("x", "v", "cell", "inv_cell"):      # nothing was launched
            assert np.array_equal(got[k].view(np.int32), inp[k].view(np.int32)), k
        assert got["counter"] == c["counter0"] and np.isnan(got["volume"]).all() and np.isnan(got["pressure"]).all()
        return
    assert status == E3K_OK, status
    ref = reference(c, inp)
    assert ref["margin"] > 1e-3, ref["margin"]
    if not c["records"]:
        assert np.isnan(got["volume"]).all() and np.isnan(got["pressure"]).all()
    worst = expected(c, inp, ref, got)
    print(f"{cid}: worst error / bound {worst:.3g}; frozen {np.flatnonzero(ref['frozen']).tolist()}, counter {got['counter']}, "
          f"mu {np.round(ref['mu'], 4).tolist()}")
    assert worst <= 1.0, worst
    status2, again = _call(c, inp, dev)
    assert status2 == E3K_OK and again["counter"] == got["counter"]
    for k in ("x", "v", "cell", "inv_cell", "volume", "pressure"):      # the same bits
        assert np.array_equal(got[k].view(np.uint8), again[k].view(np.uint8)), k
    record_measured(f"barostat_step_{cid}", worst_over_bound=worst)


@pytest.mark.gpu
def test_the_python_launch_site_is_the_kernel(dev):
    """``run/md._barostat`` on device tensors == the raw call on the same operands"""
    from e3_layers_amd.run.md import _barostat

    c = next(c for c in CASES if c["id"] == "G5")
    inp = inputs(c)
    _, raw = _call(c, inp, dev)
    t = {k: torch.from_numpy(inp[k].copy()).to(dev) for k in ("x", "v", "cell", "inv_cell", "pbc", "virial", "kinetic", "node_ptr")}
    counter = torch.zeros(1, dtype=torch.int32, device=dev)
    vol, prs = torch.zeros(inp["G"], dtype=torch.float64, device=dev), torch.zeros(inp["G"], dtype=torch.float64, device=dev)
    _barostat(t["x"][:inp["n"]], t["v"][:inp["n"]], t["cell"][:inp["G"]], t["inv_cell"][:inp["G"]], t["pbc"], t["virial"], t["kinetic"],
              t["node_ptr"], c["p0"], c["a"], c["b"], MIN_WIDTH, SEED, c["draw"], counter, vol, prs)
    torch.cuda.synchronize()
    for k in ("x", "v", "cell", "inv_cell"):
        assert np.array_equal(t[k].cpu().numpy().view(np.int32), raw[k].view(np.int32)), k
    assert np.array_equal(vol.cpu().numpy(), raw["volume"]) and np.array_equal(prs.cpu().numpy(), raw["pressure"])
    with pytest.raises(ValueError, match="finite"):
        _barostat(t["x"], t["v"], t["cell"], t["inv_cell"], t["pbc"], t["virial"], t["kinetic"], t["node_ptr"], 0.1, float("nan"), 0.0,
                  MIN_WIDTH, SEED, 0, counter)
