"""The periodic kernels of csrc/e3k_pbc.hip -- nlist_kernel<FILL, PeriodicRule> (with e3k_nlist.hip's nlist_scan_kernel between its two passes) and
pbc_edge_vector_fwd_kernel -- through the C ABI, word for word against a numpy fp32 model of the rule in csrc/e3k_pbc.h.

A case lays its operands out in ONE arena of 4-byte words (the Arena of tests/test_gpu_rtable_matrix.py: slack on both sides of every
block, integer outputs start as a sentinel); after the calls the WHOLE arena is compared: what a call writes against the model, exactly,
everything else bit for bit.  The model (``pbc_rule``) is the header's statement operation by operation: fp32 differences, ``fmaf`` as
``float32(float64 * float64 + float64)`` (the product of two fp32 numbers is exact in float64), ``rint`` (ties to even, as ``rintf``),
every square rounded on its own, a correctly rounded square root, strict ``<``.  ``inv_cell`` is an INPUT of the ABI: the cases form it
with numpy in float64 and round it to fp32.  tests/test_pbc_host.py holds the model to a float64 brute force over the 27 neighbouring
images and to the project's torch restatement, holds ``CASES`` to the kernels and functions the library ships, and shows the table to be
sharp (wrong models disagree on the cases' own inputs).

Cut-off 1.875 = 15 / 8: 1.125^2 + 1.5^2 = 0.25^2 + 1.25^2 + 1.375^2 = 1.875^2 exactly, so pairs can be planted EXACTLY on the cutoff
through a face, an edge and a corner image of the cell diag(4, 4.5, 5) (dropped: strict <) and one ulp inside (kept).  Every cell's
perpendicular widths exceed 2 r_max (1 + 1e-3) = 3.75375 (asserted where the cells are made).

edge_len: bit-equal to the model AND within 3 x 2^-24 |v| of the float64 length of the fp32 vector -- d2 carries at most three
roundings per term (product, two sums: 3 u), the square root halves that and adds its own: 2.5 u <= 3 u (the bound of the ``evf`` cases
of tests/test_gpu_edge_matrix.py, counted the same way).
"""
import numpy as np
import pytest
import torch

from tests.test_gpu_batch_matrix import SENT, SENT64, _i64, _words, ghost_edges
from tests.test_gpu_rtable_matrix import Arena, Check

pytestmark = pytest.mark.gpu

f32, f64 = np.float32, np.float64
E3K_OK, E3K_ERR_INVALID = 0, -1
R_MAX = 1.875
MIN_WIDTH = 2.0 * R_MAX * (1.0 + 1e-3)
U24 = 2.0 ** -24
NL_K = {"nlist_kernel<false, e3k::PeriodicRule>", "nlist_kernel<true, e3k::PeriodicRule>"}     # (+ nlist_scan_kernel of e3k_nlist.o, between the two)
EV_K = {"pbc_edge_vector_fwd_kernel"}
PLANT_CELL = np.diag([4.0, 4.5, 5.0])
# (image, |v| components): the destination sits one lattice vector along each named axis minus these components from the source
PLANTS = (("face", (1.875, 0.0, 0.0)), ("edge", (1.125, 1.5, 0.0)), ("corner", (0.25, 1.25, 1.375)))


# ---------------------------------------------------------------------------------------------------------------------------------
# the table
def nlist(id_, why, sizes, cells, ghost=5, e_cap="fit", planted=False, eseg=True, flag0=0, open_too=False, spread=3):
    return dict(id=id_, kind="nlist", why=why, sizes=list(sizes), cells=cells, ghost=ghost, e_cap=e_cap, planted=planted, eseg=eseg,
                flag0=flag0, open_too=open_too, spread=spread, kernels=set(NL_K), funcs={"e3k_pbc_nlist_count", "e3k_pbc_nlist_fill"})


def evf(id_, why, E, cells="mixed", with_len=True):
    return dict(id=id_, kind="evf", why=why, E=E, cells=cells, with_len=with_len, kernels=set(EV_K), funcs={"e3k_pbc_edge_vector_fwd"})


def refuse(id_, why, fn, **over):
    return dict(id=id_, kind="refuse", why=why, fn=fn, over=over, kernels=set(), funcs={"e3k_pbc_" + fn})


SIZES = [2, 3, 64, 65, 129, 200]
CASES = [
    nlist("nlist_sizes", "graphs of 2, 3, 64, 65, 129 and 200 atoms (sources that keep pairs in more than one 64-wide round), a different "
          "cell per graph -- orthorhombic, triclinic, slab --, atoms up to 3 cells outside the box; e_cap equal to the total: no tail",
          SIZES, "mixed"),
    nlist("nlist_ortho", "orthorhombic cells only", [40, 65, 90], "ortho"),
    nlist("nlist_triclinic", "triclinic cells only: the transposed cell is another cell", [40, 65, 90], "tri"),
    nlist("nlist_slab", "pbc = (1, 1, 0): the third axis is never wrapped, atoms spread along it", [50, 70], "slab"),
    nlist("nlist_N1025", "1 025 nodes: the scan's carry past its first 1 024", [200] * 5 + [20], "mixed", ghost=5),
    nlist("nlist_N2100", "about 2 100 nodes: three nodes per scan thread", [200] * 10 + [97], "mixed", ghost=3),
    nlist("nlist_G1", "one real graph", [65], "tri"),
    nlist("nlist_G0", "the ghost graph alone: nothing is searched, the whole buffer is tail, every shift zero", [], "mixed", ghost=4,
          e_cap=("fit", 37)),
    nlist("nlist_planted", "pairs exactly on the cutoff through a face, an edge and a corner image (dropped) and one ulp inside (kept)",
          [30], "ortho", planted=True),
    nlist("nlist_overflow_cut", "the list is cut inside a source's row: flag bit 32, the counter rises, shifts valid below the cut",
          [64, 65, 129], "mixed", e_cap="cut", flag0=1),
    nlist("nlist_tail_3000", "a long ghost tail: ghost edges flip every n_ghost - 1, their shifts are zero", [65, 20], "mixed", ghost=7,
          e_cap=("fit", 3000)),
    nlist("nlist_no_eseg", "edge_segment NULL", [64, 3], "mixed", eseg=False, e_cap=("fit", 9)),
    nlist("nlist_open", "pbc = 0 everywhere: edge_index, _n_edges, _edge_segment, state and flag equal e3k_nlist_fill's on the same batch "
          "(called beside it), every shift zero", [2, 65, 129], "open", open_too=True, e_cap=("fit", 11), spread=0),
    *[evf(f"evf_E{E}", "E at the 256-lane block seams, one edge, none; vec bit-equal to the builder's rule, len within the bound", E)
      for E in (0, 1, 255, 256, 257)],
    evf("evf_no_len", "edge_len NULL: vec alone is written", 300, with_len=False),
    evf("evf_triclinic", "triclinic cells", 700, cells="tri"),
    refuse("refuse_count_null_cell", "cell NULL", "nlist_count", cell=None),
    refuse("refuse_count_null_inv", "inv_cell NULL", "nlist_count", inv=None),
    refuse("refuse_count_N0", "no nodes", "nlist_count", N=0),
    refuse("refuse_count_G_negative", "G < 0", "nlist_count", G=-1),
    refuse("refuse_fill_null_shift", "edge_cell_shift NULL", "nlist_fill", shift=None),
    refuse("refuse_fill_null_pbc", "pbc NULL", "nlist_fill", pbc=None),
    refuse("refuse_fill_e_cap_negative", "e_cap < 0", "nlist_fill", e_cap=-1),
    refuse("refuse_fill_e_cap_2_31", "e_cap = 2^31", "nlist_fill", e_cap=2 ** 31),
    refuse("refuse_evf_null_shift", "edge_cell_shift NULL", "edge_vector_fwd", shift=None),
    refuse("refuse_evf_null_seg", "node_seg NULL", "edge_vector_fwd", seg=None),
    refuse("refuse_evf_E_negative", "E < 0", "edge_vector_fwd", E=-1),
    refuse("refuse_evf_no_cells", "n_cells = 0 with edges", "edge_vector_fwd", n_cells=0),
]


def table_kernels():
    return set().union(*(c["kernels"] for c in CASES))


def table_functions():
    return set().union(*(c["funcs"] for c in CASES))


# ---------------------------------------------------------------------------------------------------------------------------------
# the model
def fma32(a, b, c):
    """fmaf: one rounding (the float64 product of two float32 is exact; the sum's double rounding is below 2^-52)"""
    return (np.asarray(a, f64) * np.asarray(b, f64) + np.asarray(c, f64)).astype(f32)


def pbc_rule(d, cell, inv, pbc, r_max=R_MAX, mutant=None):
    """d [P, 3] fp32 = pos[j] - pos[i]; cell, inv [P, 3, 3] fp32, pbc [P, 3]: (image numbers int32 [P, 3], vectors fp32 [P, 3], lengths
    fp32 [P], keep).  mutants: "plus_rint", "transposed" (cell used transposed), "no_shift" (shift ignored in the vector), "le",
    "wrap_all" (a non-periodic axis wrapped)."""
    d, cell, inv = np.asarray(d, f32), np.asarray(cell, f32), np.asarray(inv, f32)
    if mutant == "transposed":
        cell = cell.transpose(0, 2, 1)
    s = fma32(d[:, 2:3], inv[:, 2, :], fma32(d[:, 1:2], inv[:, 1, :], d[:, 0:1] * inv[:, 0, :]))
    assert s.dtype == f32
    r = np.rint(s)
    on = np.ones_like(pbc, bool) if mutant == "wrap_all" else np.asarray(pbc) != 0
    n = np.where(on, r if mutant == "plus_rint" else -r, f32(0)).astype(f32)
    v = fma32(n[:, 2:3], cell[:, 2, :], fma32(n[:, 1:2], cell[:, 1, :], fma32(n[:, 0:1], cell[:, 0, :], d)))
    sq = v * v
    length = np.sqrt((sq[:, 0] + sq[:, 1]) + sq[:, 2])
    assert length.dtype == f32
    keep = length <= f32(r_max) if mutant == "le" else length < f32(r_max)
    if mutant == "no_shift":
        v = d.copy()
    return n.astype(np.int32), v, length, keep


def widths(cell):
    """perpendicular widths of a float64 cell [3, 3]: 1 / |column k of the inverse|"""
    return 1.0 / np.linalg.norm(np.linalg.inv(np.asarray(cell, f64)), axis=0)


def make_cell(kind, rng):
    """(cell float64 [3, 3] whose entries are fp32 numbers, pbc [3])"""
    pbc = np.array([1, 1, 1], np.int32)
    if kind == "open":
        return np.diag(rng.uniform(4.2, 5.5, 3)).astype(f32).astype(f64), np.zeros(3, np.int32)
    for _ in range(100):
        cell = np.diag(rng.uniform(4.2, 5.5, 3))
        if kind in ("tri", "slab"):
            cell += rng.uniform(-1.2, 1.2, (3, 3)) * (1 - np.eye(3))
        if kind == "slab":
            cell[2] = [0.0, 0.0, 20.0]
            pbc = np.array([1, 1, 0], np.int32)
        cell = cell.astype(f32).astype(f64)
        if (widths(cell)[pbc != 0] > MIN_WIDTH * 1.01).all():
            return cell, pbc
    raise AssertionError("no cell of the wanted widths")


def geometry(c, rng):
    """pos [N, 3] fp32, node_seg, node_ptr, G, cell / inv [G + 1, 3, 3] fp32, pbc [G + 1, 3] int32 (the ghost graph's: zero)"""
    kinds = {"mixed": ("ortho", "tri", "slab"), "ortho": ("ortho",), "tri": ("tri",), "slab": ("slab",), "open": ("open",)}[c["cells"]]
    graphs, cells, pbcs = [], [], []
    for k, n in enumerate(c["sizes"]):
        cell, pbc = make_cell(kinds[k % len(kinds)], rng)
        frac = rng.uniform(0, 1, (n, 3))
        if c["spread"]:
            frac += rng.integers(-c["spread"], c["spread"] + 1, (n, 3))
        graphs.append((frac @ cell).astype(f32))
        cells.append(cell)
        pbcs.append(pbc)
    if c["planted"]:
        pos = []
        for k, (name, comp) in enumerate(PLANTS):
            comp = np.array(comp)
            for inside in (False, True):
                a = np.array([0.5, 0.5 + 0.03125 * k, 0.5 + (0.0625 if inside else 0.0)]) + 0.015625 * k
                b = a + np.where(comp > 0, np.diag(PLANT_CELL) - comp, 0.0)
                a32, b32 = a.astype(f32), b.astype(f32)
                assert (a32 == a).all() and (b32 == b).all()
                if inside:      # one ulp along the longest component: |v| shrinks
                    ax = int(np.argmax(comp))
                    b32[ax] = np.nextafter(b32[ax], f32(np.inf))
                pos += [a32, b32]
        graphs.append(np.array(pos, f32))
        cells.append(PLANT_CELL.copy())
        pbcs.append(np.array([1, 1, 1], np.int32))
    sizes = [len(g) for g in graphs]
    G = len(sizes)
    graphs.append(rng.uniform(0, 1.0, (c["ghost"], 3)).astype(f32))      # (ghost nodes inside the cutoff of each other: not searched)
    pos = np.concatenate(graphs, 0)
    N = len(pos)
    node_ptr = _i64(np.concatenate([[0], np.cumsum(sizes), [N]]))
    node_seg = _i64(np.repeat(np.arange(G + 1), sizes + [c["ghost"]]))
    cell = np.zeros((G + 1, 3, 3), f32)
    inv = np.zeros((G + 1, 3, 3), f32)
    pbc = np.zeros((G + 1, 3), np.int32)
    for g in range(G):
        assert (widths(cells[g])[pbcs[g] != 0] > MIN_WIDTH).all()
        cell[g], inv[g], pbc[g] = cells[g], np.linalg.inv(cells[g]).astype(f32), pbcs[g]
    return dict(pos=pos, node_seg=node_seg, node_ptr=node_ptr, G=G, N=N, cell=cell, inv=inv, pbc=pbc)


def nlist_model(inp, e_cap, state1=0, flag0=0, mutant=None):
    """counts, offsets, edge_index [2, e_cap], shift [e_cap, 3], edge_seg, n_edges [G + 1], state, flag of include/e3k.h's periodic capped
    list (the layout of tests/test_gpu_batch_matrix.nlist_model).  e_cap: an int, ("fit", k) or "cut"."""
    pos, node_seg, node_ptr, G, N = inp["pos"], inp["node_seg"], inp["node_ptr"], inp["G"], inp["N"]
    src, dst, seg, shifts, vecs, counts = [], [], [], [], [], np.zeros(N, np.int32)
    for i in range(N):
        g = int(node_seg[i])
        if g < 0 or g >= G:
            continue
        j = np.arange(int(node_ptr[g]), int(node_ptr[g + 1]), dtype=np.int64)
        P = len(j)
        n, v, _, keep = pbc_rule(pos[j] - pos[i], np.broadcast_to(inp["cell"][g], (P, 3, 3)), np.broadcast_to(inp["inv"][g], (P, 3, 3)),
                                 np.broadcast_to(inp["pbc"][g], (P, 3)), mutant=mutant)
        keep &= j != i
        counts[i] = keep.sum()
        src += [i] * int(keep.sum())
        dst += list(j[keep])
        seg += [g] * int(keep.sum())
        shifts.append(n[keep])
        vecs.append(v[keep])
    offsets = _i64(np.concatenate([[0], np.cumsum(counts.astype(np.int64))]))
    total = int(counts.sum())
    if e_cap == "cut":      # inside the row of a source with at least four edges, about the middle of the list
        i = next(i for i in np.argsort(np.abs(offsets[:-1] - total // 2)) if counts[i] >= 4)
        e_cap = int(offsets[i] + counts[i] // 2)
        assert offsets[i] < e_cap < offsets[i + 1]
    elif not isinstance(e_cap, int):
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
    vec = np.concatenate(vecs) if vecs else np.zeros((0, 3), f32)
    eseg = _i64(seg[:n_real] + [G] * (e_cap - n_real))
    cut = lambda v: min(int(offsets[int(v)]), e_cap)
    n_edges = _i64([max(cut(node_ptr[g + 1]) - cut(node_ptr[g]), 0) for g in range(G)] + [e_cap - n_real])
    over = total > e_cap or (total < e_cap and n_ghost < 2)
    return dict(counts=counts, offsets=offsets, ei=ei, shift=shift, vec=vec[:n_real], eseg=eseg, n_edges=n_edges,
                state=_i64([total, state1 + over]), flag=np.int32(flag0 | (32 if over else 0)), e_cap=e_cap, over=over, total=total)


# ---------------------------------------------------------------------------------------------------------------------------------
# capped list
def _arena(c):
    import zlib

    return Arena(zlib.crc32(c["id"].encode()))


def prepare_nlist(c):
    ar = _arena(c)
    inp = geometry(c, ar.rng)
    N, G = inp["N"], inp["G"]
    inp["model"] = nlist_model(inp, c["e_cap"], 5, c["flag0"])
    e_cap = inp["e_cap"] = inp["model"]["e_cap"]
    ar.alloc("pos", 3 * N, inp["pos"]).alloc("seg", 2 * N, inp["node_seg"], align=2).alloc("ptr", 2 * (G + 2), inp["node_ptr"], align=2)
    ar.alloc("cell", 9 * (G + 1), inp["cell"]).alloc("inv", 9 * (G + 1), inp["inv"]).alloc("pbc", 3 * (G + 1), inp["pbc"])
    for sfx in ("", "_open")[:2 if c["open_too"] else 1]:
        ar.alloc("state" + sfx, 4, _i64([SENT64, 5]), align=2).alloc("flag" + sfx, 1, np.int32(c["flag0"]))
        ar.alloc("counts" + sfx, N, np.int32(SENT)).alloc("offsets" + sfx, 2 * (N + 1), np.int32(SENT), align=2)
        ar.alloc("ei" + sfx, 4 * e_cap, np.int32(SENT), align=2).alloc("n_edges" + sfx, 2 * (G + 1), np.int32(SENT), align=2)
        if c["eseg"]:
            ar.alloc("eseg" + sfx, 2 * e_cap, np.int32(SENT), align=2)
    ar.alloc("shift", 3 * e_cap, np.int32(SENT))
    return ar, inp


def model_nlist(c, inp, mutant=None):
    m = inp["model"] if mutant is None else nlist_model(inp, inp["e_cap"], 5, c["flag0"], mutant)
    names = ("counts", "offsets", "ei", "n_edges", "state", "flag") + (("eseg",) if c["eseg"] else ())
    out = {k: m[k] for k in names + ("shift",)}
    if c["open_too"]:      # e3k_nlist_fill beside it: the same words
        out.update({k + "_open": m[k] for k in names})
    return out


def launch_nlist(c, ar, inp, lib, st):
    N, G, e_cap = inp["N"], inp["G"], inp["e_cap"]
    head = (ar.p("pos"), ar.p("seg"), ar.p("ptr"), N, G, R_MAX)
    geom = (ar.p("cell"), ar.p("inv"), ar.p("pbc"))
    assert lib.e3k_pbc_nlist_count(*head, *geom, ar.p("counts"), st) == E3K_OK
    assert lib.e3k_pbc_nlist_fill(*head, *geom, ar.p("counts"), e_cap, ar.p("offsets"), ar.p("ei"), ar.p("shift"), ar.p("n_edges"),
                                  ar.p("eseg") if c["eseg"] else None, ar.p("state"), ar.p("flag"), st) == E3K_OK
    if c["open_too"]:
        assert lib.e3k_nlist_count(*head, ar.p("counts_open"), st) == E3K_OK
        assert lib.e3k_nlist_fill(*head, ar.p("counts_open"), e_cap, ar.p("offsets_open"), ar.p("ei_open"), ar.p("n_edges_open"),
                                  ar.p("eseg_open") if c["eseg"] else None, ar.p("state_open"), ar.p("flag_open"), st) == E3K_OK


# ---------------------------------------------------------------------------------------------------------------------------------
# edge vectors
def prepare_evf(c):
    ar = _arena(c)
    geo = geometry(dict(sizes=[40, 50, 33], cells=c["cells"], planted=False, ghost=4, spread=3), ar.rng)
    m = nlist_model(geo, ("fit", 6))
    E = c["E"]
    assert m["e_cap"] >= E
    pick = np.sort(ar.rng.permutation(m["e_cap"])[:E])      # real edges and (where E allows) ghost edges with their zero shift
    inp = dict(geo, E=E, src=m["ei"][0][pick].astype(np.int32), dst=m["ei"][1][pick].astype(np.int32), shift=m["shift"][pick],
               real=pick < m["total"], want_vec=m["vec"][pick[pick < m["total"]]])
    N, G = geo["N"], geo["G"]
    ar.alloc("pos", 3 * N, geo["pos"]).alloc("seg", 2 * N, geo["node_seg"], align=2).alloc("cell", 9 * (G + 1), geo["cell"])
    ar.alloc("src", max(E, 1), inp["src"] if E else np.int32(0)).alloc("dst", max(E, 1), inp["dst"] if E else np.int32(0))
    ar.alloc("shift", max(3 * E, 1), inp["shift"] if E else np.int32(0))
    ar.alloc("vec", max(3 * E, 1), f32(np.nan))
    if c["with_len"]:
        ar.alloc("len", max(E, 1), f32(np.nan))
    return ar, inp


def model_evf(c, inp, mutant=None):
    """vec and len of the rule from the STORED shifts: for the builder's real edges these are the builder's own vectors"""
    g = inp["node_seg"][inp["src"]]
    d = inp["pos"][inp["dst"]] - inp["pos"][inp["src"]]
    cell = inp["cell"][g]
    if mutant == "transposed":
        cell = cell.transpose(0, 2, 1)
    n = inp["shift"].astype(f32)
    v = fma32(n[:, 2:3], cell[:, 2, :], fma32(n[:, 1:2], cell[:, 1, :], fma32(n[:, 0:1], cell[:, 0, :], d))) if mutant != "no_shift" else d
    sq = v * v
    out = dict(vec=v.astype(f32))
    if c["with_len"]:
        out["len"] = np.sqrt((sq[:, 0] + sq[:, 1]) + sq[:, 2]).astype(f32)
    return out


def launch_evf(c, ar, inp, lib, st):
    assert lib.e3k_pbc_edge_vector_fwd(ar.p("pos"), ar.p("src"), ar.p("dst"), ar.p("shift"), ar.p("seg"), ar.p("cell"), inp["G"] + 1, inp["N"],
                                       inp["E"], ar.p("vec"), ar.p("len") if c["with_len"] else None, st) == E3K_OK


# ---------------------------------------------------------------------------------------------------------------------------------
# refusals: a small valid problem of every entry point, one argument replaced; nothing is launched, the arena stays as it was
def prepare_refuse(c):
    ar = _arena(c)
    geo = geometry(dict(sizes=[5, 4], cells="ortho", planted=False, ghost=3, spread=1), ar.rng)
    N, G, E, e_cap = geo["N"], geo["G"], 10, 40
    ar.alloc("pos", 3 * N, geo["pos"]).alloc("seg", 2 * N, geo["node_seg"], align=2).alloc("ptr", 2 * (G + 2), geo["node_ptr"], align=2)
    ar.alloc("cell", 9 * (G + 1), geo["cell"]).alloc("inv", 9 * (G + 1), geo["inv"]).alloc("pbc", 3 * (G + 1), geo["pbc"])
    ar.alloc("counts", N, np.zeros(N, np.int32)).alloc("offsets", 2 * (N + 1), align=2).alloc("ei", 4 * e_cap, align=2)
    ar.alloc("shift", 3 * e_cap, np.zeros(3 * e_cap, np.int32)).alloc("n_edges", 2 * (G + 1), align=2).alloc("state", 4, align=2)
    ar.alloc("flag", 1, np.int32(0)).alloc("src", E, np.zeros(E, np.int32)).alloc("dst", E, np.ones(E, np.int32))
    ar.alloc("vec", 3 * E).alloc("len", E)
    return ar, dict(geo, E=E, e_cap=e_cap, n_cells=G + 1)


def model_refuse(c, inp, mutant=None):
    return {}


def launch_refuse(c, ar, inp, lib, st):
    a = dict(inp, **{k: k for k in ar.blocks})
    a.update(c["over"])
    p = lambda k: ar.p(a[k])
    head = (p("pos"), p("seg"), p("ptr"), a["N"], a["G"], R_MAX, p("cell"), p("inv"), p("pbc"))
    if c["fn"] == "nlist_count":
        rc = lib.e3k_pbc_nlist_count(*head, p("counts"), st)
    elif c["fn"] == "nlist_fill":
        rc = lib.e3k_pbc_nlist_fill(*head, p("counts"), a["e_cap"], p("offsets"), p("ei"), p("shift"), p("n_edges"), None, p("state"),
                                    p("flag"), st)
    else:
        assert c["fn"] == "edge_vector_fwd"
        rc = lib.e3k_pbc_edge_vector_fwd(p("pos"), p("src"), p("dst"), p("shift"), p("seg"), p("cell"), a["n_cells"], a["N"], a["E"],
                                         p("vec"), p("len"), st)
    assert rc == E3K_ERR_INVALID, f"return code {rc}"


PREPARE = dict(nlist=prepare_nlist, evf=prepare_evf, refuse=prepare_refuse)
MODEL = dict(nlist=model_nlist, evf=model_evf, refuse=model_refuse)
LAUNCH = dict(nlist=launch_nlist, evf=launch_evf, refuse=launch_refuse)


def prepared(c):
    """(arena with its host image, inputs) of a case: everything but the device"""
    ar, inp = PREPARE[c["kind"]](c)
    ar.x0 = ar.rng.standard_normal(ar.n + 32).astype(f32).view(np.int32)
    for name, init in ar.inits:
        off, n = ar.blocks[name]
        v = np.asarray(init)
        ar.x0[off:off + n] = _words(v) if v.ndim else np.full(n, v).astype(v.dtype).view(np.int32)
    return ar, inp


def expected(c, ar, inp, mutant=None):
    return MODEL[c["kind"]](c, inp, mutant)


@pytest.mark.parametrize("c", CASES, ids=[c["id"] for c in CASES])
def test_pbc_case_against_the_host_model(dev, c):
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
    if c["kind"] == "evf" and inp["E"]:
        got = ck.dev("vec", f32)[:3 * inp["E"]].reshape(-1, 3)
        assert np.array_equal(got[inp["real"]].view(np.int32), inp["want_vec"].view(np.int32))      # the BUILDER's vectors, bit for bit
        if c["with_len"]:
            ref = np.sqrt((got.astype(f64) ** 2).sum(-1))
            err = np.abs(ck.dev("len", f32)[:inp["E"]].astype(f64) - ref)
            print(f"{c['id']}: len worst error / bound {float((err / (3 * U24 * ref)).max()):.3f}")
            assert (err <= 3 * U24 * ref).all()
            assert (ck.dev("len", f32)[:inp["E"]][inp["real"]] < f32(R_MAX)).all()      # what the builder kept is inside the cutoff
    ck.unchanged()
