"""``e3k_virial_edges`` (csrc/e3k_virial.hip, one kernel) against float64 on the CPU, element by element, at the seams of its work order.

One case per C-ABI call.  The output buffer is NaN before every call; after it every element is compared, none masked; every case is
run twice and the two results must be the same bits (no atomics: a fixed order of summation).

Reference.  float64 numpy: ``out[g, 3 a + b] = -sum_{e in g} v_e[a] (g_vec_e[b] + (len_e > 0 ? g_len_e / len_e : 0) v_e[b])`` over the
edges whose SOURCE node lies in graph g (``reference``).  MAJORANT ``M[g, a, b] = sum |v_a| (|g_vec_b| + |g_len / len| |v_b|)``.

Bound (u = 2^-24).  The per-edge gradient is formed in fp32 as e3k_edge_vector_bwd forms it: one division and one FMA, 2 u of
``|g_vec_b| + |f| |v_b|`` (with g_vec alone it is exact; the bound does not use that).  The factor v_a is an input: exact.  The product
of two floats is exact in double, and the double sum of n terms adds (n + 2) 2^-53 of the majorant: nothing at these sizes, but
counted.  The store to fp32: u of the sum, at most u M.  Together ``(3 u / (1 - 3 u) + (n + 2) 2^-53) M``; where M is zero (a graph
without edges, self-loops under g_len alone) the output must be exactly zero.  Small-integer inputs (``exact``): every operation is
exact and the output must EQUAL the reference.

``CASES`` is a plain table; tests/test_virial_host.py holds it to the kernels e3k_virial.o ships and to the header, shows the bound to
hold for a float32 model of the kernel in its lane and reduction order, and to be sharp against planted mutants (no GPU needed there).
"""
import zlib

import numpy as np
import pytest
import torch

from tests.util import record_measured

E3K_OK, E3K_ERR_INVALID = 0, -1
U24 = 2.0 ** -24
f32, f64 = np.float32, np.float64


def case(id_, why, graphs, g_vec=True, g_len=True, shuffle=False, loops=0, exact=False):
    """``graphs``: (nodes, edges) per graph, in order; ``shuffle``: the edges are stored in shuffled order (src_perm is not the
    identity); ``loops``: that many edges of the first graph with edges are self-loops (vec = 0, len = 0)"""
    return dict(id=id_, kind="virial", why=why, graphs=graphs, g_vec=g_vec, g_len=g_len, shuffle=shuffle, loops=loops, exact=exact,
                funcs={"e3k_virial_edges"}, kernels={"virial_edges_kernel"})


def refuse(id_, why, **null):
    return dict(id=id_, kind="refuse", why=why, graphs=[(4, 9), (3, 5)], g_vec=True, g_len=True, shuffle=False, loops=0, exact=False,
                null=null, funcs={"e3k_virial_edges"}, kernels=set())


SMALL = (5, 13)      # the small graph beside the one under test
CASES = [
    case("G1_E0", "one graph, no edge: nine zeros from the one launch", [(3, 0)]),
    case("middle_empty", "three graphs, the middle one without edges (and without nodes' edges): zeros between two sums",
         [(6, 20), (4, 0), (5, 17)]),
    case("one_edge", "a single edge: 255 idle lanes, three idle waves", [(2, 1)]),
    case("E255", "one slot short of the lane stride", [(40, 255), SMALL]),
    case("E256", "exactly one round of the 256 lanes", [(40, 256), SMALL]),
    case("E257", "lane 0 takes a second slot", [(40, 257), SMALL]),
    case("E769", "the fourth round begins", [SMALL, (60, 769)]),
    case("g_vec_only", "no g_len: the gradient is g_vec itself", [(30, 300), SMALL], g_len=False),
    case("g_len_only", "no g_vec: the gradient is (g_len / len) vec, self-loops contribute nothing", [(30, 300), SMALL], g_vec=False,
         loops=7),
    case("self_loops", "edges of length zero beside g_vec: the division is skipped, g_vec still counts", [(30, 300), SMALL], loops=7),
    case("shuffled", "edges stored in shuffled order: the walk goes through src_perm", [(25, 270), (9, 40), (14, 300)], shuffle=True),
    case("ghost_third", "a trailing ghost graph holding a third of the edges", [(12, 100), (12, 100), (8, 100)], shuffle=True),
    case("integers", "small integers: every operation exact, the output equals the reference", [(20, 260), (6, 30)], exact=True,
         shuffle=True, loops=3),
    refuse("refuse_null_out", "out NULL", out=None),
    refuse("refuse_null_graph_ptr", "graph_ptr NULL", graph_ptr=None),
    refuse("refuse_null_src_ptr", "src_ptr NULL", src_ptr=None),
    refuse("refuse_null_src_perm", "src_perm NULL with E > 0", src_perm=None),
    refuse("refuse_null_vec", "edge_vec NULL with E > 0", vec=None),
    refuse("refuse_no_gradient", "g_vec and g_len NULL", g_vec=None, g_len=None),
    refuse("refuse_g_len_without_len", "g_len without edge_len", len=None),
    refuse("refuse_E_negative", "E < 0", E=-1),
    refuse("refuse_G_negative", "G < 0", G=-1),
]


def table_kernels():
    return set().union(*(c["kernels"] for c in CASES))


def table_functions():
    return set().union(*(c["funcs"] for c in CASES))


_INTEGER_VECTORS = np.array([[3, 4, 0], [0, -3, 4], [2, 0, 0], [1, -2, 2], [-4, 0, 3], [0, 0, -1], [2, 2, 1], [-6, 0, 8]], f32)


def inputs(c):
    """numpy operands of the case: vec, len, g_vec, g_len [E, ...] fp32, src [E], src_ptr [N + 1], src_perm [E], graph_ptr [G + 1]
    int32, N, E, G and ``edge_graph`` [E] (the graph of each edge's source)"""
    rng = np.random.default_rng(zlib.crc32(c["id"].encode()))
    nodes = np.array([n for n, _ in c["graphs"]], np.int64)
    graph_ptr = np.concatenate([[0], np.cumsum(nodes)]).astype(np.int32)
    src = np.concatenate([rng.integers(graph_ptr[g], graph_ptr[g + 1], e) for g, (_, e) in enumerate(c["graphs"])] +
                         [np.zeros(0, np.int64)]).astype(np.int32)
    E, N, G = len(src), int(graph_ptr[-1]), len(nodes)
    src = rng.permutation(src) if c["shuffle"] else np.sort(src, kind="stable")
    if c["exact"]:
        vec = _INTEGER_VECTORS[rng.integers(0, len(_INTEGER_VECTORS), E)] * rng.choice(np.array([1, -1], f32), (E, 1))
        g_vec = rng.integers(-4, 5, (E, 3)).astype(f32)
    else:
        vec = (2.0 * rng.standard_normal((E, 3))).astype(f32)
        g_vec = rng.standard_normal((E, 3)).astype(f32)
    if c["loops"]:
        first = next(g for g, (_, e) in enumerate(c["graphs"]) if e)
        mine = np.flatnonzero((src >= graph_ptr[first]) & (src < graph_ptr[first + 1]))
        vec[mine[:c["loops"]]] = 0
    ln = np.sqrt((vec[:, 0] * vec[:, 0] + vec[:, 1] * vec[:, 1]) + vec[:, 2] * vec[:, 2]).astype(f32)
    g_len = (ln * rng.integers(-3, 4, E).astype(f32)) if c["exact"] else rng.standard_normal(E).astype(f32)
    if c["loops"]:
        g_len[ln == 0] = 1.5      # (must not matter)
    if c["exact"]:
        assert (ln == np.rint(ln)).all()
    src_perm = np.argsort(src, kind="stable").astype(np.int32)
    src_ptr = np.concatenate([[0], np.cumsum(np.bincount(src, minlength=N))]).astype(np.int32)
    edge_graph = np.searchsorted(graph_ptr, src, side="right") - 1
    return dict(vec=vec, len=ln, g_vec=g_vec if c["g_vec"] else None, g_len=g_len if c["g_len"] else None, src=src, src_ptr=src_ptr,
                src_perm=src_perm, graph_ptr=graph_ptr, N=N, E=E, G=G, edge_graph=edge_graph)


def reference(c, inp, mutant=None):
    """(out [G, 9] float64, bound [G, 9]).  mutants: "sign" (+sum), "transposed" (g (x) v), "no_g_len" (the g_len term dropped),
    "no_inv_len" (g_len vec instead of g_len vec / len)"""
    E, G = inp["E"], inp["G"]
    v = inp["vec"].astype(f64)
    g, mag = np.zeros((E, 3)), np.zeros((E, 3))
    if inp["g_vec"] is not None:
        g += inp["g_vec"].astype(f64)
        mag += np.abs(inp["g_vec"].astype(f64))
    if inp["g_len"] is not None and mutant != "no_g_len":
        ln = inp["len"].astype(f64)
        with np.errstate(divide="ignore", invalid="ignore"):
            f = np.where(ln > 0, inp["g_len"].astype(f64) / (1.0 if mutant == "no_inv_len" else ln), 0.0)
        g += f[:, None] * v
        mag += np.abs(f[:, None] * v)
    terms = g[:, :, None] * v[:, None, :] if mutant == "transposed" else v[:, :, None] * g[:, None, :]
    out, maj = np.zeros((G, 3, 3)), np.zeros((G, 3, 3))
    np.add.at(out, inp["edge_graph"], terms)
    np.add.at(maj, inp["edge_graph"], np.abs(v)[:, :, None] * mag[:, None, :])
    n = np.bincount(inp["edge_graph"], minlength=G).astype(f64)
    bound = (3 * U24 / (1 - 3 * U24) + (n + 2) * 2.0 ** -53)[:, None, None] * maj
    return (out if mutant == "sign" else -out).reshape(G, 9), bound.reshape(G, 9)


_ARG_ORDER = ("g_vec", "g_len", "vec", "len", "src_ptr", "src_perm", "graph_ptr")


def _call(c, inp, dev):
    """(status, out [G, 9] fp32 host array: NaN where nothing was written)"""
    from e3_layers_amd.backend import lib as L

    null = c.get("null", {})
    t = {k: (None if inp[k] is None or (k in null and null[k] is None) else torch.from_numpy(inp[k]).to(dev)) for k in _ARG_ORDER}
    out = torch.full((max(inp["G"], 1), 9), float("nan"), device=dev, dtype=torch.float32)
    status = L.load().e3k_virial_edges(*(L.ptr(t[k]) for k in _ARG_ORDER), inp["N"], null.get("E", inp["E"]), null.get("G", inp["G"]),
                                       None if "out" in null else L.ptr(out), L.stream_ptr())
    torch.cuda.synchronize()
    return status, out.cpu().numpy()[:inp["G"]]


@pytest.mark.gpu
@pytest.mark.parametrize("cid", [c["id"] for c in CASES])
def test_virial_edges_case(dev, cid):
    c = next(c for c in CASES if c["id"] == cid)
    inp = inputs(c)
    status, got = _call(c, inp, dev)
    if c["kind"] == "refuse":
        assert status == E3K_ERR_INVALID, status
        assert np.isnan(got).all()      # nothing was launched
        return
    assert status == E3K_OK, status
    want, bound = reference(c, inp)
    err = np.abs(got.astype(f64) - want)
    assert np.isfinite(got).all(), got
    live = bound > 0
    worst = float((err[live] / bound[live]).max()) if live.any() else 0.0
    print(f"{cid}: worst error / bound {worst:.3g}, edges per graph {[e for _, e in c['graphs']]}")
    assert (got[~live] == 0).all(), got[~live]
    if c["exact"]:
        assert np.array_equal(got.astype(f64), want), np.abs(got - want).max()
    assert (err <= bound).all(), f"{cid}: {int((err > bound).sum())} elements outside the bound, worst {worst}"
    status2, again = _call(c, inp, dev)
    assert status2 == E3K_OK and np.array_equal(got.view(np.int32), again.view(np.int32))      # the same bits
    record_measured(f"virial_edges_{cid}", worst_over_bound=worst)


@pytest.mark.gpu
def test_ops_edge_virial_is_the_kernel(dev):
    """``ops.edge_virial`` on a GraphTopo built by the project == the raw call on the same operands, and its checks"""
    from e3_layers_amd.backend import ops
    from e3_layers_amd.backend.graph import GraphTopo

    c = next(c for c in CASES if c["id"] == "shuffled")
    inp = inputs(c)
    t = {k: torch.from_numpy(inp[k]).to(dev) for k in _ARG_ORDER}
    dummy = t["src_perm"]
    topo = GraphTopo(torch.from_numpy(inp["src"]).to(dev), dummy, t["src_ptr"], dummy, t["src_ptr"], t["src_perm"])
    got = ops.edge_virial(t["g_vec"], t["g_len"], t["vec"], t["len"], topo, t["graph_ptr"], inp["G"])
    _, raw = _call(c, inp, dev)
    assert got.shape == (inp["G"], 9) and got.dtype == torch.float32
    assert np.array_equal(got.cpu().numpy().view(np.int32), raw.view(np.int32))
    with pytest.raises(ValueError, match="g_vec or g_len"):
        ops.edge_virial(None, None, t["vec"], t["len"], topo, t["graph_ptr"], inp["G"])
    with pytest.raises(ValueError, match="int32"):
        ops.edge_virial(t["g_vec"], None, t["vec"], t["len"], topo, t["graph_ptr"].long(), inp["G"])
    with pytest.raises(ValueError, match="shape"):
        ops.edge_virial(t["g_vec"][:-1], None, t["vec"], t["len"], topo, t["graph_ptr"], inp["G"])
