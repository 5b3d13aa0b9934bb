"""The all-images builder of csrc/e3k_images.hip -- nlist_kernel<FILL, ImagesRule> (with e3k_nlist.hip's nlist_scan_kernel between its two
passes) -- through the C ABI, word for word against a numpy fp32 model of the rule in csrc/e3k_images.h, and against a float64 brute
force over the box of R + 1 images.

A case lays its operands out in ONE arena of 4-byte words (the Arena of tests/test_gpu_rtable_matrix.py); after the calls the WHOLE
arena is compared: what a call writes against the model, exactly, everything else bit for bit.  The model (``images_rule``) is the
header's statement operation by operation, on top of the minimum-image model of tests/test_gpu_pbc_matrix.py (``fmaf`` as
``float32(float64 * float64 + float64)``, ``rint`` ties to even, every square rounded on its own, strict ``<``).  ``inv_cell`` and
``image_range`` are INPUTS of the ABI: the cases form them with numpy in float64 (``ranges``, the formula of the header restated here,
not imported from the package).

Fixtures.  Every geometry is made from a seed for which NO candidate of the float64 brute force lies within 1e-4 r_max of the cutoff
(asserted where it is made: ``geometry``), so the fp32 model and float64 agree on every candidate, and -- the one-atom case apart --
for which a kept edge has |m_k| = R_k on every periodic axis of every graph: the range is needed.  (The one-atom case of the issue,
r_max = 1.6 L, has R = 2 and keeps |m| <= 1 only: R covers a base image at the edge of [-1/2, 1/2], and a single atom's own
displacement is 0.  It is held to its 18 edges instead.)  tests/test_images_host.py runs everything here that needs no GPU.
"""
import zlib

import numpy as np
import pytest
import torch

from tests.test_gpu_batch_matrix import SENT, SENT64, _i64, _words, ghost_edges
from tests.test_gpu_pbc_matrix import fma32, widths
from tests.test_gpu_rtable_matrix import Arena, Check

pytestmark = pytest.mark.gpu

f32, f64 = np.float32, np.float64
E3K_OK, E3K_ERR_INVALID = 0, -1
R_MAX = 1.875
MARGIN = 1e-3
MAX_RANGE = 7
NEAR = 1e-4      # no candidate within NEAR r_max of the cutoff
NL_K = {"nlist_kernel<false, e3k::ImagesRule>", "nlist_kernel<true, e3k::ImagesRule>"}      # (+ nlist_scan_kernel of e3k_nlist.o)
FUNCS = {"e3k_images_count", "e3k_images_fill"}


# ---------------------------------------------------------------------------------------------------------------------------------
# the table.  A graph is (atoms, kind): kinds are the image ranges wanted, as "R0R1R2", with a suffix: "t" triclinic, "s" slab
# (pbc = (1, 1, 0)), "o" open (pbc = 0), "1" the one-atom cube of side 1 (r_max = 1.6)
def nlist(id_, why, graphs, ghost=5, e_cap="fit", eseg=True, flag0=0, spread=0, r_max=R_MAX, table=None, pbc_too=False, needed=True):
    return dict(id=id_, kind="nlist", why=why, graphs=list(graphs), ghost=ghost, e_cap=e_cap, eseg=eseg, flag0=flag0, spread=spread,
                r_max=r_max, table=table, pbc_too=pbc_too, needed=needed, kernels=set(NL_K), funcs=set(FUNCS))


def refuse(id_, why, fn, **over):
    return dict(id=id_, kind="refuse", why=why, fn=fn, over=over, kernels=set(), funcs={"e3k_images_" + fn})


_COUNT_NULLS = ("pos", "seg", "ptr", "cell", "inv", "pbc", "range", "counts")
_FILL_NULLS = _COUNT_NULLS + ("offsets", "ei", "shift", "n_edges", "state", "flag")
CASES = [
    nlist("one_atom", "one atom in a cube of side L, r_max = 1.6 L: exactly 18 edges, 6 at L and 12 at sqrt(2) L, all self images",
          [(1, "1")], r_max=1.6, needed=False),
    nlist("two_triclinic", "two atoms in a triclinic cell, R = (1, 1, 1)", [(2, "111t")]),
    nlist("slab", "pbc = (1, 1, 0): the third axis has no images", [(6, "110s")]),
    nlist("batch3", "three graphs with ranges (0, 0, 0), (1, 1, 1) and (2, 1, 0): M = 1, 27, 15 in one launch", [(9, "000"), (4, "111t"), (5, "210")]),
    nlist("unwrapped", "positions unwrapped by up to 3 cells: the base image is nonzero", [(4, "111t"), (3, "210")], spread=3),
    nlist("n3_M27", "3 atoms x 27 images = 81 candidates per source: the walk crosses 64", [(3, "111")]),
    nlist("n5_M27", "5 atoms x 27 images = 135 candidates per source: the walk crosses 128; a source's kept edges cross a lane seam",
          [(5, "111")]),
    nlist("n70_M1", "70 atoms with every range zero (M = 1: two rounds of plain destinations) beside a graph with M = 25",
          [(70, "000"), (3, "220")]),
    nlist("tail", "e_cap above the list: the ghost tail behind it, its shifts zero", [(4, "111"), (3, "210")], e_cap=("fit", 300), ghost=6),
    nlist("cut_one_short", "e_cap one short: the list is cut, flag bit 32, the counter rises, the last edge is missing", [(4, "111"), (3, "210")],
          e_cap=("fit", -1), flag0=1),
    nlist("no_eseg", "edge_segment NULL", [(3, "111t")], eseg=False, e_cap=("fit", 7)),
    nlist("empty_graph", "an empty graph between two others", [(3, "111"), (0, "111"), (4, "210")], e_cap=("fit", 5)),
    nlist("G0", "the ghost graph alone: nothing is searched, the whole buffer is tail", [], ghost=4, e_cap=("fit", 29)),
    nlist("table_malformed", "range entries 100 (clamped to 7), -3 (clamped to 0, on an axis that needs none) and 5 on a non-periodic axis "
          "(ignored): the list is the brute force's", [(3, "110s"), (3, "100")], table="malformed"),
    nlist("zero_ranges", "wide cells, every range zero: counts, offsets, edge_index, edge_cell_shift, _n_edges, _edge_segment, state and flag "
          "equal e3k_pbc_nlist_count / _fill's on the same batch (called beside it), bit for bit", [(40, "000"), (65, "000t"), (30, "000s")],
          pbc_too=True, e_cap=("fit", 11), spread=2),
    *[refuse(f"refuse_count_null_{k}", f"{k} NULL", "count", **{k: None}) for k in _COUNT_NULLS],
    refuse("refuse_count_N0", "no nodes", "count", N=0),
    refuse("refuse_count_N_2_31", "N = 2^31", "count", N=2 ** 31),
    refuse("refuse_count_G_negative", "G < 0", "count", G=-1),
    *[refuse(f"refuse_fill_null_{k}", f"{k} NULL", "fill", **{k: None}) for k in _FILL_NULLS],
    refuse("refuse_fill_N0", "no nodes", "fill", N=0),
    refuse("refuse_fill_N_2_31", "N = 2^31", "fill", N=2 ** 31),
    refuse("refuse_fill_G_negative", "G < 0", "fill", G=-1),
    refuse("refuse_fill_e_cap_negative", "e_cap < 0", "fill", e_cap=-1),
    refuse("refuse_fill_e_cap_2_31", "e_cap = 2^31", "fill", e_cap=2 ** 31),
]


def table_kernels():
    return set().union(*(c["kernels"] for c in CASES))


def table_functions():
    return set().union(*(c["funcs"] for c in CASES))


# ---------------------------------------------------------------------------------------------------------------------------------
# the model
def ranges(cell, pbc, r_max):
    """csrc/e3k_images.h: R_k = ceil(r_max (1 + 1e-3) / w_k + 0.5) - 1 on a periodic axis, 0 elsewhere (float64 cell [3, 3])"""
    pbc = np.asarray(pbc) != 0
    if not pbc.any():
        return np.zeros(3, np.int32)
    return np.where(pbc, np.ceil(r_max * (1.0 + MARGIN) / widths(cell) + 0.5) - 1, 0).astype(np.int32)


def effective(table, pbc):
    """what the kernel makes of a table row: clamped to [0, 7], zero where pbc is"""
    return np.where(np.asarray(pbc) != 0, np.clip(table, 0, MAX_RANGE), 0).astype(np.int64)


def offsets_of(R):
    """[M, 3] the offsets m in walk order: m_0 slowest, m_2 fastest, each from -R_k"""
    g = np.meshgrid(*(np.arange(-int(r), int(r) + 1) for r in R), indexing="ij")
    return np.stack([a.ravel() for a in g], 1).astype(np.int64)


def images_rule(d, cell, inv, pbc, m, r_max):
    """d [P, 3] fp32 = pos[j] - pos[i]; cell, inv [3, 3] fp32, pbc [3]; m [P, 3] integer offsets: (n int32 [P, 3], v fp32, length fp32, keep
    WITHOUT the self-image exclusion)"""
    d, cell, inv = np.asarray(d, f32), np.asarray(cell, f32)[None], np.asarray(inv, f32)[None]
    s = fma32(d[:, 2:3], inv[:, 2, :], fma32(d[:, 1:2], inv[:, 1, :], d[:, 0:1] * inv[:, 0, :]))
    assert s.dtype == f32
    base = np.where(np.asarray(pbc)[None] != 0, -np.rint(s), f32(0)).astype(f32)
    n = (base + m.astype(f32)).astype(f32)
    v = fma32(n[:, 2:3], cell[:, 2, :], fma32(n[:, 1:2], cell[:, 1, :], fma32(n[:, 0:1], cell[:, 0, :], d)))
    sq = v * v
    length = np.sqrt((sq[:, 0] + sq[:, 1]) + sq[:, 2])
    assert length.dtype == f32
    return n.astype(np.int32), v, length, length < f32(r_max)


def source_edges(inp, i, r_max):
    """(dst [K], shift [K, 3], m [K, 3]) of source i in walk order"""
    g = int(inp["node_seg"][i])
    beg, end = int(inp["node_ptr"][g]), int(inp["node_ptr"][g + 1])
    offs = offsets_of(effective(inp["range"][g], inp["pbc"][g]))
    M = len(offs)
    j = np.repeat(np.arange(beg, end, dtype=np.int64), M)
    m = np.tile(offs, (end - beg, 1))
    n, _, _, keep = images_rule(inp["pos"][j] - inp["pos"][i], inp["cell"][g], inp["inv"][g], inp["pbc"][g], m, r_max)
    keep &= ~((j == i) & (n == 0).all(1))
    return j[keep], n[keep], m[keep]


def images_model(inp, e_cap, r_max, state1=0, flag0=0):
    """counts, offsets, edge_index [2, e_cap], shift [e_cap, 3], edge_seg, n_edges [G + 1], state, flag of include/e3k.h's all-images capped
    list (the layout of tests/test_gpu_pbc_matrix.nlist_model).  e_cap: an int or ("fit", k): the list's size + k."""
    node_seg, node_ptr, G, N = inp["node_seg"], inp["node_ptr"], inp["G"], inp["N"]
    src, dst, seg, shifts, ms, counts = [], [], [], [], [], np.zeros(N, np.int32)
    for i in range(N):
        g = int(node_seg[i])
        if g < 0 or g >= G:
            continue
        j, n, m = source_edges(inp, i, r_max)
        counts[i] = len(j)
        src += [i] * len(j)
        dst += list(j)
        seg += [g] * len(j)
        shifts.append(n)
        ms.append(m)
    offsets = _i64(np.concatenate([[0], np.cumsum(counts.astype(np.int64))]))
    total = int(counts.sum())
    if not isinstance(e_cap, int):
        e_cap = total + (0 if e_cap == "fit" else e_cap[1])
    n_real = min(total, e_cap)
    gs = int(node_ptr[G])
    n_ghost = N - gs
    ei = np.empty((2, e_cap), np.int64)
    ei[0, :n_real], ei[1, :n_real] = src[:n_real], dst[:n_real]
    ei[:, n_real:] = ghost_edges(e_cap - n_real, n_ghost, gs) if n_ghost >= 2 else N - 1
    shift = np.zeros((e_cap, 3), np.int32)
    all_shift = np.concatenate(shifts) if shifts else np.zeros((0, 3), np.int32)
    shift[:n_real] = all_shift[:n_real]
    eseg = _i64(seg[:n_real] + [G] * (e_cap - n_real))
    cut = lambda v: min(int(offsets[int(v)]), e_cap)
    n_edges = _i64([max(cut(node_ptr[g + 1]) - cut(node_ptr[g]), 0) for g in range(G)] + [e_cap - n_real])
    over = total > e_cap or (total < e_cap and n_ghost < 2)
    return dict(counts=counts, offsets=offsets, ei=ei, shift=shift, eseg=eseg, n_edges=n_edges, state=_i64([total, state1 + over]),
                flag=np.int32(flag0 | (32 if over else 0)), e_cap=e_cap, over=over, total=total, src=np.array(src, np.int64),
                dst=np.array(dst, np.int64), all_shift=all_shift, m=np.concatenate(ms) if ms else np.zeros((0, 3), np.int64))


def brute_force(inp, r_max):
    """float64: every (i, j, n) of a real graph, n over the box of R + 1 images around the rounded one on the periodic axes (R: the
    formula's ranges of the graph), with |pos_j - pos_i + n . cell| < r_max and not (i == j and n == 0); ordered by (i, j, n).  Returns
    (src, dst, n [E, 3], the smallest | |v| - r_max | over ALL candidates)."""
    pos, G = inp["pos"].astype(f64), inp["G"]
    out, nearest = [], np.inf
    for g in range(G):
        beg, end = int(inp["node_ptr"][g]), int(inp["node_ptr"][g + 1])
        cell, on = inp["cell"][g].astype(f64), inp["pbc"][g] != 0
        inv = np.linalg.inv(cell) if on.any() else np.zeros((3, 3))
        box = offsets_of((inp["true_range"][g] + 1) * on)
        for i in range(beg, end):
            for j in range(beg, end):
                d = pos[j] - pos[i]
                base = -np.floor(d @ inv + 0.5) * on
                n = base[None] + box
                length = np.linalg.norm(d[None] + n @ cell, axis=1)
                live = ~((n == 0).all(1) & (i == j))
                nearest = min(nearest, float(np.abs(length[live] - r_max).min()) if live.any() else np.inf)
                for q in np.flatnonzero((length < r_max) & live):
                    out.append((i, j) + tuple(int(x) for x in n[q]))
    out.sort()
    a = np.array(out, np.int64).reshape(-1, 5)
    return a[:, 0], a[:, 1], a[:, 2:], nearest


def make_cell(kind, rng, r_max):
    """(cell float64 [3, 3] whose entries are fp32 numbers, pbc [3]) with the image ranges the kind names"""
    if kind == "1":
        return np.eye(3), np.array([1, 1, 1], np.int32)
    want = np.array([int(ch) for ch in kind[:3]])
    pbc = np.array([1, 1, 0] if kind.endswith("s") else [0, 0, 0] if kind.endswith("o") else [1, 1, 1], np.int32)
    reach = r_max * (1 + MARGIN)
    # R = 0: a width check_cell accepts.  R > 0: inside the range's interval [reach / (R + 1/2), reach / (R - 1/2)) and below
    # r_max / R, so that (in an orthorhombic cell) an atom's own image at |m| = R is kept
    lo = np.where(want == 0, 2.05 * reach, 1.03 * reach / (want + 0.5))
    hi = np.where(want == 0, 2.6 * reach, 0.97 * np.minimum(reach / np.maximum(want - 0.5, 0.5), r_max / np.maximum(want, 1)))
    for _ in range(1000):
        cell = np.diag(rng.uniform(lo, hi))
        if kind.endswith("t"):
            cell += rng.uniform(-0.25, 0.25, (3, 3)) * (1 - np.eye(3)) * np.diag(cell).min()
        if kind.endswith("s"):
            cell[2] = [0.0, 0.0, 6.0]
        cell = cell.astype(f32).astype(f64)
        if (ranges(cell, pbc, r_max) == want * (pbc != 0)).all():
            return cell, pbc
    raise AssertionError(f"no cell with the ranges {kind}")


def _geometry(c, rng):
    graphs, cells, pbcs = [], [], []
    for n, kind in c["graphs"]:
        cell, pbc = make_cell(kind, rng, c["r_max"])
        frac = rng.uniform(0, 1, (n, 3))
        if c["spread"]:
            frac += rng.integers(-c["spread"], c["spread"] + 1, (n, 3))
        graphs.append((frac @ cell).astype(f32).reshape(n, 3))
        cells.append(cell)
        pbcs.append(pbc)
    sizes = [len(g) for g in graphs]
    G = len(sizes)
    graphs.append(rng.uniform(0, 1.0, (c["ghost"], 3)).astype(f32))      # (ghost nodes inside the cutoff of each other: not searched)
    pos = np.concatenate(graphs, 0)
    N = len(pos)
    node_ptr = _i64(np.concatenate([[0], np.cumsum(sizes), [N]]))
    node_seg = _i64(np.repeat(np.arange(G + 1), sizes + [c["ghost"]]))
    cell, inv = np.zeros((G + 1, 3, 3), f32), np.zeros((G + 1, 3, 3), f32)
    pbc, true = np.zeros((G + 1, 3), np.int32), np.zeros((G + 1, 3), np.int32)
    for g in range(G):
        cell[g], inv[g], pbc[g] = cells[g], np.linalg.inv(cells[g]).astype(f32), pbcs[g]
        true[g] = ranges(cells[g], pbcs[g], c["r_max"])
    table = true.copy()
    if c["table"] == "malformed":
        assert G == 2 and tuple(true[0]) == (1, 1, 0) and tuple(pbc[0]) == (1, 1, 0) and tuple(true[1]) == (1, 0, 0)
        table[0] = [100, 1, 5]      # above the cap (clamped to 7: still complete); 5 on the non-periodic axis (ignored)
        table[1] = [1, -3, -2 ** 31]      # negative where no image is needed (clamped to 0)
        table[G] = [9, 9, 9]      # the ghost graph's row: never read as a range (the ghost graph is not searched)
    return dict(pos=pos, node_seg=node_seg, node_ptr=node_ptr, G=G, N=N, cell=cell, inv=inv, pbc=pbc, range=table, true_range=true)


_geometries = {}


def geometry(c):
    """The case's geometry from the FIRST seed (counted up from the case's own) whose float64 brute force has no candidate within
    NEAR r_max of the cutoff and (``needed``) a kept edge with |m_k| = R_k on every periodic axis of every non-empty graph; both are
    asserted here.  Also the model's list is held to the brute force: the same ordered list.  Shared by every test of a case."""
    if c["id"] in _geometries:
        return _geometries[c["id"]]
    seed0 = zlib.crc32(c["id"].encode())
    for seed in range(seed0, seed0 + 200):
        inp = _geometry(c, np.random.default_rng(seed))
        bs, bd, bn, nearest = brute_force(inp, c["r_max"])
        if not nearest > NEAR * c["r_max"]:
            continue
        m = images_model(inp, "fit", c["r_max"])
        needed = all((np.abs(m["m"][inp["node_seg"][m["src"]] == g][:, k]) == inp["true_range"][g][k]).any()
                     for g in range(inp["G"]) if inp["node_ptr"][g + 1] > inp["node_ptr"][g] for k in range(3) if inp["pbc"][g][k])
        if c["needed"] and not needed:
            continue
        break
    assert nearest > NEAR * c["r_max"], (c["id"], nearest)
    assert needed or not c["needed"], c["id"]
    # the fp32 model's list IS the float64 brute force's, as an ordered list
    assert np.array_equal(m["src"], bs) and np.array_equal(m["dst"], bd) and np.array_equal(m["all_shift"], bn), c["id"]
    inp["seed"], inp["brute"] = seed, (bs, bd, bn)
    _geometries[c["id"]] = inp
    return inp


# ---------------------------------------------------------------------------------------------------------------------------------
def _arena(c):
    return Arena(zlib.crc32(c["id"].encode()))


def prepare_nlist(c):
    ar = _arena(c)
    inp = dict(geometry(c))
    N, G = inp["N"], inp["G"]
    inp["model"] = images_model(inp, c["e_cap"], c["r_max"], 5, c["flag0"])
    e_cap = inp["e_cap"] = inp["model"]["e_cap"]
    ar.alloc("pos", 3 * N, inp["pos"]).alloc("seg", 2 * N, inp["node_seg"], align=2).alloc("ptr", 2 * (G + 2), inp["node_ptr"], align=2)
    ar.alloc("cell", 9 * (G + 1), inp["cell"]).alloc("inv", 9 * (G + 1), inp["inv"]).alloc("pbc", 3 * (G + 1), inp["pbc"])
    ar.alloc("range", 3 * (G + 1), inp["range"])
    for sfx in ("", "_pbc")[:2 if c["pbc_too"] else 1]:
        ar.alloc("state" + sfx, 4, _i64([SENT64, 5]), align=2).alloc("flag" + sfx, 1, np.int32(c["flag0"]))
        ar.alloc("counts" + sfx, N, np.int32(SENT)).alloc("offsets" + sfx, 2 * (N + 1), np.int32(SENT), align=2)
        ar.alloc("ei" + sfx, max(4 * e_cap, 1), np.int32(SENT), align=2).alloc("n_edges" + sfx, 2 * (G + 1), np.int32(SENT), align=2)
        ar.alloc("shift" + sfx, max(3 * e_cap, 1), np.int32(SENT))
        if c["eseg"]:
            ar.alloc("eseg" + sfx, max(2 * e_cap, 1), np.int32(SENT), align=2)
    return ar, inp


def model_nlist(c, inp):
    m = inp["model"]
    names = ("counts", "offsets", "ei", "shift", "n_edges", "state", "flag") + (("eseg",) if c["eseg"] else ())
    out = {k: m[k] for k in names}
    if c["pbc_too"]:      # e3k_pbc_nlist_* beside it: the same words
        out.update({k + "_pbc": m[k] for k in names})
    return out


def launch_nlist(c, ar, inp, lib, st):
    N, G, e_cap = inp["N"], inp["G"], inp["e_cap"]
    head = (ar.p("pos"), ar.p("seg"), ar.p("ptr"), N, G, c["r_max"])
    geom = (ar.p("cell"), ar.p("inv"), ar.p("pbc"))
    assert lib.e3k_images_count(*head, *geom, ar.p("range"), ar.p("counts"), st) == E3K_OK
    assert lib.e3k_images_fill(*head, *geom, ar.p("range"), ar.p("counts"), e_cap, ar.p("offsets"), ar.p("ei"), ar.p("shift"), ar.p("n_edges"),
                               ar.p("eseg") if c["eseg"] else None, ar.p("state"), ar.p("flag"), st) == E3K_OK
    if c["pbc_too"]:
        assert lib.e3k_pbc_nlist_count(*head, *geom, ar.p("counts_pbc"), st) == E3K_OK
        assert lib.e3k_pbc_nlist_fill(*head, *geom, ar.p("counts_pbc"), e_cap, ar.p("offsets_pbc"), ar.p("ei_pbc"), ar.p("shift_pbc"),
                                      ar.p("n_edges_pbc"), ar.p("eseg_pbc") if c["eseg"] else None, ar.p("state_pbc"), ar.p("flag_pbc"),
                                      st) == E3K_OK


# refusals: a small valid problem, one argument replaced; nothing is launched, the arena stays as it was
REFUSE_GEOMETRY = nlist("refuse_geometry", "the valid problem every refusal starts from", [(3, "111"), (2, "210")], ghost=3)


def prepare_refuse(c):
    ar = _arena(c)
    geo = geometry(REFUSE_GEOMETRY)
    N, G, e_cap = geo["N"], geo["G"], 400
    ar.alloc("pos", 3 * N, geo["pos"]).alloc("seg", 2 * N, geo["node_seg"], align=2).alloc("ptr", 2 * (G + 2), geo["node_ptr"], align=2)
    ar.alloc("cell", 9 * (G + 1), geo["cell"]).alloc("inv", 9 * (G + 1), geo["inv"]).alloc("pbc", 3 * (G + 1), geo["pbc"])
    ar.alloc("range", 3 * (G + 1), geo["range"])
    ar.alloc("counts", N, np.zeros(N, np.int32)).alloc("offsets", 2 * (N + 1), align=2).alloc("ei", 4 * e_cap, align=2)
    ar.alloc("shift", 3 * e_cap, np.zeros(3 * e_cap, np.int32)).alloc("n_edges", 2 * (G + 1), align=2).alloc("state", 4, align=2)
    ar.alloc("flag", 1, np.int32(0))
    return ar, dict(geo, e_cap=e_cap)


def model_refuse(c, inp):
    return {}


def launch_refuse(c, ar, inp, lib, st):
    a = dict(inp, **{k: k for k in ar.blocks})
    a.update(c["over"])
    p = lambda k: ar.p(a[k])
    head = (p("pos"), p("seg"), p("ptr"), a["N"], a["G"], R_MAX, p("cell"), p("inv"), p("pbc"), p("range"))
    if c["fn"] == "count":
        rc = lib.e3k_images_count(*head, p("counts"), st)
    else:
        rc = lib.e3k_images_fill(*head, p("counts"), a["e_cap"], p("offsets"), p("ei"), p("shift"), p("n_edges"), None, p("state"), p("flag"), st)
    assert rc == E3K_ERR_INVALID, f"return code {rc}"


PREPARE = dict(nlist=prepare_nlist, refuse=prepare_refuse)
MODEL = dict(nlist=model_nlist, refuse=model_refuse)
LAUNCH = dict(nlist=launch_nlist, refuse=launch_refuse)


def prepared(c):
    """(arena with its host image, inputs) of a case: everything but the device"""
    ar, inp = PREPARE[c["kind"]](c)
    ar.x0 = ar.rng.standard_normal(ar.n + 32).astype(f32).view(np.int32)
    for name, init in ar.inits:
        off, n = ar.blocks[name]
        v = np.asarray(init)
        ar.x0[off:off + n] = _words(v) if v.ndim else np.full(n, v).astype(v.dtype).view(np.int32)
    return ar, inp


def expected(c, ar, inp):
    return MODEL[c["kind"]](c, inp)


@pytest.mark.parametrize("c", CASES, ids=[c["id"] for c in CASES])
def test_images_case_against_the_host_model(dev, c):
    from e3_layers_amd.backend import lib as L

    lib = L.load()
    ar, inp = prepared(c)
    want = expected(c, ar, inp)
    ar.buf = torch.from_numpy(ar.x0.copy()).to(dev)
    ar.base = ar.buf.data_ptr()
    assert ar.base % 64 == 0
    torch.cuda.synchronize()
    LAUNCH[c["kind"]](c, ar, inp, lib, L.stream_ptr())
    ck = Check(ar, c)
    for name, w in want.items():
        if np.asarray(w).size:
            ck.exact(name, w)
    if c["kind"] == "nlist" and not inp["model"]["over"]:      # ... and the device's list is the float64 brute force's, as an ordered list
        total = inp["model"]["total"]
        bs, bd, bn = inp["brute"]
        ei = ck.dev("ei", np.int64)[:2 * inp["e_cap"]].reshape(2, -1)
        assert np.array_equal(ei[0, :total], bs) and np.array_equal(ei[1, :total], bd)
        assert np.array_equal(ck.dev("shift")[:3 * total].reshape(-1, 3), bn)
    ck.unchanged()
