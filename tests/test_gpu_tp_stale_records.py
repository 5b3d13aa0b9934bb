"""The backward walks read their edge records (e3k_edge_records, 64 bytes per edge) with SCALAR loads (load_rec, csrc/e3k_tp_body.h):
the scalar cache is not coherent with a kernel's own stores, so this rests on the records being written by earlier launches only.  The
risk is a walk that meets a STALE record -- one an earlier launch left in the same buffer.

Tiny graphs through the C entries: 6 nodes, 14 edges, 64-channel groups, l_max 2.  Two edge lists A and B over the same nodes; in
each, one node has no out-edge, one exactly one, and the last node's edges end at the last record of the buffer (the walk's
``t + 1 < end ? t + 1 : t`` prefetch then stops at the buffer's last record).  The records of A are built into ONE buffer and every
backward walk that exists for the plan runs on it -- the dense walk with and without the weight gradient (tp_bwd_x_kernel MODE 5 / 4)
where ``e3k_tp_table_supported`` says so (channel-complete plans: not the scalar-head product), the masked and the scalar walk where
``e3k_tp_masked_supported`` / ``e3k_tp_scalar_supported`` do -- then the records of B are built into the SAME buffer and the walks run
again.  Both results

* equal, bit for bit, the results with records built into fresh buffers,
* meet the float64 oracle of tests/test_gpu_tp_matrix.py at the bound tests/test_gpu_tp_masked_matrix.py uses (GTOL).

The same sequence runs once inside a captured graph: {records -> walks}, replayed after the inputs of B were copied over those of A.

Plans: the dense layer below the last convolution of config_energy at l_max 2 with the shipped half-live masks as its masked form
(tests/test_gpu_tp_masked_matrix.py), and the scalar-head product (tests/test_gpu_tp_scalar_matrix.py).
"""
import ctypes as C

import pytest
import torch

from tests.test_gpu_tp_masked_matrix import DENSE_MASKS, LEFT, OUT, SHIPPED_LMAX2, _pruned
from tests.test_gpu_tp_matrix import GTOL, SH9, _check_packing, _Oracle, _packed_w64
from tests.util import rel_err

N, E = 6, 14
# (src, dst).  A: node 2 sends nothing, node 3 one edge, node 5 (the last) owns the last three records.
EDGES_A = ([0, 0, 0, 0, 1, 1, 1, 3, 4, 4, 4, 5, 5, 5], [1, 2, 3, 5, 0, 2, 4, 3, 0, 1, 5, 0, 2, 4])
# B: node 0 sends nothing, node 4 one edge, node 5 owns the last TWO records: every row pointer but the first and last moves.
EDGES_B = ([1, 1, 1, 1, 1, 2, 2, 2, 3, 3, 3, 4, 5, 5], [0, 2, 3, 4, 5, 0, 1, 5, 1, 2, 4, 2, 3, 1])
SCALAR_LEFT = "64x0e+64x1o+64x2e"
KNOTS = 128


def _bits(t):
    return t.contiguous().view(torch.int32)


def _inputs(plan, edges, seed, dev):
    """the inputs of one edge list (edge ids shuffled, so the records' order is not the edges'), host and device"""
    from e3_layers_amd.backend import radial_table
    from e3_layers_amd.backend.graph import build_topology

    g = torch.Generator().manual_seed(seed)
    ei = torch.tensor(edges, dtype=torch.long)[:, torch.randperm(E, generator=g)]
    out_deg = torch.bincount(ei[0], minlength=N)
    assert int((out_deg == 0).sum()) == 1 and int((out_deg == 1).sum()) == 1 and int(out_deg[N - 1]) >= 2
    rnd = lambda *shape: torch.randn(*shape, dtype=torch.float64, generator=g).float()
    x, gm, sh = rnd(N, plan.d_in), rnd(N, plan.d_mid), rnd(E, 9)
    radius = torch.rand(E, dtype=torch.float64, generator=g).float() * 5.0
    radius[:2] = torch.tensor([0.0, 5.0])
    topo = build_topology(ei.to(dev), N)
    bins = radial_table.build_bins(radius.to(dev), 5.0, KNOTS)
    assert int(topo.src_ptr[N]) == E and int(topo.src_ptr[N - 1]) < E      # the last node's list ends at record E - 1
    return dict(ei=ei, x=x, g=gm, sh=sh, topo=topo, bins=bins, X=x.to(dev), G=gm.to(dev), SH=sh.to(dev))


def _table(plan, knots, dev):
    from e3_layers_amd.backend import radial_table

    W = plan.w_numel
    rows_r = torch.arange(knots + 1, dtype=torch.float64) * (5.0 / knots)
    cols = torch.arange(W, dtype=torch.float64)
    smooth = (torch.sin(rows_r[:, None] * (1.0 + 5.0 * cols[None, :] / W)) * torch.exp(-0.2 * rows_r[:, None])).float().to(dev)
    packed = radial_table.pack_raw(smooth, knots)
    _check_packing(smooth, packed, knots)
    return packed


def _records(lib, L, s, rec):
    """the source-walk records of the inputs s into rec, on the current stream"""
    t, b = s["topo"], s["bins"]
    L.check(lib.e3k_edge_records(L.ptr(t.src_perm), L.ptr(t.dst), L.ptr(b.bin), L.ptr(b.coef), L.ptr(s["SH"]), 9, E, L.ptr(rec),
                                 L.stream_ptr()), "e3k_edge_records")


def _walks(lib, L, plan, masked, dev):
    """name -> (route prefix, run(s, rec, outs), output shapes, the columns of the plan's g_w an output holds or None)"""
    h = plan.handle(dev)
    d_in, W = plan.d_in, plan.w_numel
    walks = {}

    def dense5(s, rec, o):
        L.check(lib.e3k_tp_bwd_xw_ptable(h, L.ptr(s["X"]), L.ptr(s["packed"]), L.ptr(rec), L.ptr(s["G"]), L.ptr(s["topo"].src_ptr), N, E,
                                         L.ptr(o[0]), L.ptr(o[1]), L.stream_ptr()), "e3k_tp_bwd_xw_ptable")

    def dense4(s, rec, o):
        L.check(lib.e3k_tp_bwd_x_ptable(h, L.ptr(s["packed"]), L.ptr(rec), L.ptr(s["G"]), L.ptr(s["topo"].src_ptr), N, E, L.ptr(o[0]),
                                        L.stream_ptr()), "e3k_tp_bwd_x_ptable")

    if lib.e3k_tp_table_supported(h) == 1:      # (the packed-table walks of the dispatch table: channel-complete plans)
        walks["dense_mode5"] = ("tp_bwd_x_kernel<2, 2, false, true, 5>", dense5, [(N, d_in), (E, W)], None)
        walks["dense_mode4"] = ("tp_bwd_x_kernel<2, 2, false, true, 4>", dense4, [(N, d_in)], None)
    if masked is not None:
        hm, cols, w_live, live_w = masked
        assert lib.e3k_tp_masked_supported(hm) == 1

        def run_masked(s, rec, o):
            o[0].zero_()      # (the entry's contract: the caller zero-fills what no live group owns)
            L.check(lib.e3k_tp_bwd_xw_masked_ptable(hm, L.ptr(s["X"]), L.ptr(s["packed"]), W, cols, L.ptr(rec), L.ptr(s["G"]),
                                                    L.ptr(s["topo"].src_ptr), N, E, L.ptr(o[0]), L.ptr(o[1]), L.stream_ptr()),
                    "e3k_tp_bwd_xw_masked_ptable")

        walks["masked"] = ("tp_bwd_xw_masked_kernel", run_masked, [(N, d_in), (E, w_live)], live_w)
    elif lib.e3k_tp_masked_supported(h) == 1:
        def run_masked_all(s, rec, o):
            L.check(lib.e3k_tp_bwd_xw_masked_ptable(h, L.ptr(s["X"]), L.ptr(s["packed"]), 0, None, L.ptr(rec), L.ptr(s["G"]),
                                                    L.ptr(s["topo"].src_ptr), N, E, L.ptr(o[0]), L.ptr(o[1]), L.stream_ptr()),
                    "e3k_tp_bwd_xw_masked_ptable")

        walks["masked"] = ("tp_bwd_xw_masked_kernel", run_masked_all, [(N, d_in), (E, W)], None)
    if lib.e3k_tp_scalar_supported(h) == 1:
        def run_scalar(s, rec, o):
            L.check(lib.e3k_tp_bwd_xw_scalar_ptable(h, L.ptr(s["X"]), L.ptr(s["packed"]), 0, None, L.ptr(rec), L.ptr(s["G"]),
                                                    L.ptr(s["topo"].src_ptr), N, E, L.ptr(o[0]), L.ptr(o[1]), L.stream_ptr()),
                    "e3k_tp_bwd_xw_scalar_ptable")

        walks["scalar"] = ("tp_bwd_xw_scalar_kernel", run_scalar, [(N, d_in), (E, W)], None)
    return walks


def _run_all(lib, walks, s, rec, outs=None, check_route=True):
    """every walk on the records rec; fresh NaN outputs unless given"""
    res = {}
    for name, (route, run, shapes, _) in walks.items():
        o = outs[name] if outs is not None else [torch.full(sh, float("nan"), device=rec.device) for sh in shapes]
        run(s, rec, o)
        if check_route:
            r = lib.e3k_tp_last_route()
            assert r is not None and r.decode().startswith(route), (name, r)
        res[name] = o
    return res


def _check(walks, got, fresh, ref, what):
    PGx, RGw = ref
    for name, (_, _, _, cols) in walks.items():
        for a, b in zip(got[name], fresh[name]):
            assert torch.equal(_bits(a), _bits(b)), f"{what} {name}: differs from the run on records in a fresh buffer"
        gx = got[name][0].detach().double().cpu()
        err = rel_err(gx, PGx)
        print(f"{what} {name} g_x: rel err {err:.3e} (bound {GTOL:.0e})")
        assert err < GTOL, f"{what} {name} g_x: rel err {err:.3e}"
        if len(got[name]) > 1:
            gw = got[name][1].detach().double().cpu()
            want = RGw if cols is None else RGw[:, cols]
            err = rel_err(gw, want)
            print(f"{what} {name} g_w: rel err {err:.3e} (bound {GTOL:.0e})")
            assert err < GTOL, f"{what} {name} g_w: rel err {err:.3e}"


def _plans(dev):
    from e3_layers_amd.backend import lib as L
    from e3_layers_amd.backend import ops
    from e3_layers_amd.nn.core import UVUTensorProduct

    dense = UVUTensorProduct(LEFT, SH9, OUT)
    assert tuple(g.mask for g in dense.plan.groups) == DENSE_MASKS
    groups, live_col, mid, w_live = _pruned(dense.plan, SHIPPED_LMAX2)
    live_mid = torch.zeros(dense.plan.d_mid, dtype=torch.bool)
    for off, mul in mid:
        live_mid[off:off + mul] = True
    live_w = torch.zeros(dense.plan.w_numel, dtype=torch.bool)
    for off in live_col:
        live_w[off:off + 64] = True
    pruned = ops.TpPlan(groups, dense.plan.d_in, 9, w_live, dense.plan.d_mid)
    masked = (pruned.handle(dev), (C.c_int32 * len(live_col))(*live_col), w_live, live_w)
    scalar = UVUTensorProduct(SCALAR_LEFT, SH9, "1x0e")
    # (pruned is returned to keep its handle alive)
    return [("layer", dense, LEFT, OUT, masked, live_mid, pruned), ("scalar_head", scalar, SCALAR_LEFT, "1x0e", None, None, None)]


@pytest.mark.gpu
@pytest.mark.parametrize("which", [0, 1], ids=["layer", "scalar_head"])
def test_walks_read_the_records_of_the_launch_before_them(dev, which):
    from e3_layers_amd.backend import lib as L

    lib = L.load()
    name, tpm, left, out, masked, live_mid, _keep = _plans(dev)[which]
    plan = tpm.plan
    packed = None
    sets = []
    for edges, seed in ((EDGES_A, 71 + which), (EDGES_B, 83 + which)):
        s = _inputs(plan, edges, seed, dev)
        if live_mid is not None:      # the masked form's dead columns of g_mid are zero for every walk: one oracle for all of them
            s["g"][:, ~live_mid] = 0.0
            s["G"] = s["g"].to(dev)
        if packed is None:
            packed = _table(plan, s["bins"].knots, dev)
        assert packed.shape[0] == s["bins"].knots + 1
        s["packed"] = packed
        orc = _Oracle(left, SH9, out, tpm.irreps_mid_simplified, s["ei"], N)
        PGx, _, RGw = orc.G(s["x"].double(), s["sh"].double(), _packed_w64(packed, s["bins"]), s["g"].double())
        s["ref"] = (PGx, RGw)
        sets.append(s)
    A, B = sets
    assert not torch.equal(A["topo"].src_ptr, B["topo"].src_ptr)
    walks = _walks(lib, L, plan, masked, dev)
    assert set(walks) >= ({"dense_mode5", "dense_mode4", "masked"} if name == "layer" else {"scalar"}), sorted(walks)
    first = next(iter(walks))

    # ---- records in fresh buffers
    fresh = []
    for s in sets:
        rec = torch.empty(E, 16, dtype=torch.int32, device=dev)
        _records(lib, L, s, rec)
        fresh.append(_run_all(lib, walks, s, rec))
    torch.cuda.synchronize()
    assert not torch.equal(_bits(fresh[0][first][0]), _bits(fresh[1][first][0]))

    # ---- ONE buffer: records of A, the walks, records of B over them, the walks
    shared = torch.empty(E, 16, dtype=torch.int32, device=dev)      # exactly E records: the last node's list ends at the buffer's end
    got = []
    for s in sets:
        _records(lib, L, s, shared)
        got.append(_run_all(lib, walks, s, shared))
    torch.cuda.synchronize()
    for s, g_, f_, what in zip(sets, got, fresh, ("A", "B over A")):
        _check(walks, g_, f_, s["ref"], f"{name} {what}")

    # ---- the same inside a captured graph: static inputs, {records -> walks}; replayed on A, then on B copied over A
    keys = ("X", "G", "SH")
    st = {k: A[k].clone() for k in keys}
    st["packed"] = packed
    st["topo"] = type("T", (), {k: getattr(A["topo"], k).clone() for k in ("src_ptr", "src_perm", "dst")})()
    st["bins"] = type("Bn", (), {"bin": A["bins"].bin.clone(), "coef": A["bins"].coef.clone()})()
    rec_g = torch.empty(E, 16, dtype=torch.int32, device=dev)
    outs = {k: [torch.full(sh, float("nan"), device=dev) for sh in v[2]] for k, v in walks.items()}

    def load(s):
        for k in keys:
            st[k].copy_(s[k])
        for k in ("src_ptr", "src_perm", "dst"):
            getattr(st["topo"], k).copy_(getattr(s["topo"], k))
        st["bins"].bin.copy_(s["bins"].bin)
        st["bins"].coef.copy_(s["bins"].coef)

    def body():
        _records(lib, L, st, rec_g)
        _run_all(lib, walks, st, rec_g, outs, check_route=False)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        body()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        body()
    for s, f_, what in ((A, fresh[0], "replay A"), (B, fresh[1], "replay B over A"), (A, fresh[0], "replay A over B")):
        load(s)
        for o in outs.values():
            for t in o:
                t.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        _check(walks, outs, f_, s["ref"], f"{name} {what}")
