"""The scalar-output input-gradient walk (csrc/e3k_tp_scalar.hip: e3k_tp_bwd_xw_scalar_ptable) and the column spread that follows
it (e3k_expand_columns) against float64 on the CPU.

A case is a plan whose every group enables exactly the slot (l2 = l1, l3 = 0): what ``UVUTensorProduct(left, sh, "1x0e")`` builds.
The reference is the float64 oracle of tests/test_gpu_tp_matrix.py on that product (its g_out is the 0e block, so every column of it
is live), with the path weights decoded from the packed table on the host.  Each case runs twice:

* plain: the packed table has the plan's own columns (table_off = NULL);
* embedded: as the layer executor calls it -- the plan's input blocks, its 0e block of g_out and its columns of the packed table sit
  inside wider rows at shifted offsets.  Everything of g_out outside the live block is NaN (the walk must not read it), the rest of
  g_x keeps its sentinel (the walk must not write it), and the dead columns of the table are NaN as well.  Same bits as the plain run.

Both outputs lie in sentinel-filled buffers with a margin in front and behind: the margins keep their bits.  Two runs give the same
bits.  A plan with a slot of l3 > 0 is refused with E3K_ERR_UNSUPPORTED and writes nothing.

``CASES`` and ``KERNELS`` are plain tables; tests/test_tp_scalar_inventory.py holds them to the kernels the object ships.
"""
import ctypes as C

import pytest
import torch

from tests.test_gpu_tp_matrix import (E3K_ERR_UNSUPPORTED, GTOL, SH9, PlainRef, _check_packing, _graph, _Oracle, _packed_fields, _packed_w64,
                                      reference, w_packed, within)
from tests.util import record_measured, rel_err

ROUTE = "tp_bwd_xw_scalar_kernel"
# n = 37: below the N >= 64 work-order threshold; 203: above it and not a multiple of 8
CASES = [
    {"id": "l012_n37", "left": "64x0e+64x1o+64x2e", "n": 37, "kernel": ROUTE, "why": "the three slots of an l_max 2 layer; node-major order"},
    {"id": "l012_n203", "left": "64x0e+64x1o+64x2e", "n": 203, "kernel": ROUTE, "why": "... group-major inside the XCD slices"},
    {"id": "two_chunks", "left": "128x0e+128x1o", "n": 203, "kernel": ROUTE, "why": "128-channel groups: two 64-channel chunks each"},
    {"id": "l0_only", "left": "64x0e", "n": 37, "kernel": ROUTE, "why": "a single group, l1 = 0"},
    {"id": "l2_only", "left": "64x2e", "n": 203, "kernel": ROUTE, "why": "a single group, l1 = 2"},
]
EXPAND_CASES = [
    {"id": "three_ranges", "rows": 17, "w_src": 192, "w_dst": 1920, "ranges": [(0, 0, 64), (64, 448, 64), (128, 1216, 64)],
     "kernel": "expand_columns_kernel"},
    {"id": "one_range_all", "rows": 5, "w_src": 64, "w_dst": 64, "ranges": [(0, 0, 64)], "kernel": "expand_columns_kernel"},
    {"id": "unordered_uneven", "rows": 513, "w_src": 200, "w_dst": 332, "ranges": [(136, 4, 64), (0, 196, 136)], "kernel": "expand_columns_kernel"},
]
KERNELS = {c["kernel"] for c in CASES} | {c["kernel"] for c in EXPAND_CASES}
MARGIN = 256      # floats of sentinel in front of and behind every output
SENTINEL = -7.25


def _framed(rows, cols, dev):
    """(whole buffer, the [rows, cols] view MARGIN floats into it), all SENTINEL"""
    buf = torch.full((2 * MARGIN + rows * cols,), SENTINEL, device=dev)
    return buf, buf[MARGIN:MARGIN + rows * cols].view(rows, cols)


def _margins_intact(buf):
    return bool((buf[:MARGIN] == SENTINEL).all()) and bool((buf[-MARGIN:] == SENTINEL).all())


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=[c["id"] for c in CASES])
def test_scalar_walk_against_float64(dev, case):
    from e3_layers_amd.backend import lib as L
    from e3_layers_amd.backend import ops, radial_table
    from e3_layers_amd.backend.graph import build_topology
    from e3_layers_amd.nn.core import UVUTensorProduct, tp_slots

    lib = L.load()
    torch.manual_seed(2000 + CASES.index(case))
    n = case["n"]
    tpm = UVUTensorProduct(case["left"], SH9, "1x0e")
    plan = tpm.plan
    h = plan.handle(dev)
    assert lib.e3k_tp_scalar_supported(h) == 1
    ei = _graph(n, 7 + n)
    orc = _Oracle(case["left"], SH9, "1x0e", tpm.irreps_mid_simplified, ei, n)
    e, d_in, W, d_mid = ei.shape[1], plan.d_in, plan.w_numel, plan.d_mid
    assert orc.tp.weight_numel == W and d_mid == W
    topo = build_topology(ei.to(dev), n)
    e_hub = torch.cat([(ei[1] == 0).nonzero().flatten(), (ei[0] == 1).nonzero().flatten()])
    node_rows, no_out = [0, 1], [n - 1, n - 3]

    def rnd(*shape):
        return torch.randn(*shape, dtype=torch.float64).float()

    x, g, sh = rnd(n, d_in), rnd(n, d_mid), rnd(e, 9)
    X, Gm, SH = x.to(dev), g.to(dev), sh.to(dev)
    knots = 128
    radius = torch.rand(e, dtype=torch.float64).float() * 5.2
    radius[:3] = torch.tensor([0.0, 5.0, 0.01])
    bins = radial_table.build_bins(radius.to(dev), 5.0, knots)
    rows_r = torch.arange(bins.knots + 1, dtype=torch.float64) * bins.spacing
    cols = torch.arange(W, dtype=torch.float64)
    smooth = (torch.sin(rows_r[:, None] * (1.0 + 5.0 * cols[None, :] / W)) * torch.exp(-0.2 * rows_r[:, None])).float().to(dev)
    packed = radial_table.pack_raw(smooth, bins.knots)
    _check_packing(smooth, packed, bins.knots)
    erec = bins.records(topo, SH, "src")
    w_pk = _packed_w64(packed, bins)
    PGx, _, RGw = orc.G(x.double(), sh.double(), w_pk, g.double())

    def route():
        r = lib.e3k_tp_last_route()
        return r.decode() if r is not None else None

    def check(name, gx, gw):
        gx, gw = gx.detach().double().cpu(), gw.detach().double().cpu()
        assert bool(torch.isfinite(gx).all()) and bool(torch.isfinite(gw).all()), f"{name}: an element is not finite"
        for what, got, ref, rows in (("g_x", gx, PGx, node_rows), ("g_w", gw, RGw, e_hub)):
            err, err_r = rel_err(got, ref), rel_err(got[rows], ref[rows])
            print(f"{case['id']} {name} {what}: rel err {err:.3e}, on the hub rows {err_r:.3e} (bound {GTOL:.0e})")
            assert err < GTOL and err_r < GTOL, f"{name} {what}: rel err {err:.3e} / {err_r:.3e}"
        for r in no_out:
            assert bool((gx[r] == 0).all()), f"{name}: row {r} of a node without out-edges is not exactly zero"

    # ---- plain: the table has the plan's own columns
    def plain():
        bx, gx = _framed(n, d_in, dev)
        bw, gw = _framed(e, W, dev)
        L.check(lib.e3k_tp_bwd_xw_scalar_ptable(h, L.ptr(X), L.ptr(packed), 0, None, L.ptr(erec), L.ptr(Gm), L.ptr(topo.src_ptr), n, e,
                                                gx.data_ptr(), gw.data_ptr(), L.stream_ptr()), "e3k_tp_bwd_xw_scalar_ptable")
        torch.cuda.synchronize()
        assert route() == ROUTE, route()
        assert _margins_intact(bx) and _margins_intact(bw), "a word outside an output changed"
        return gx, gw

    gx1, gw1 = plain()
    check("plain", gx1, gw1)
    # element by element: the plain reference over the plan's paths and its bound gamma_k M (tests/test_gpu_tp_matrix.py: the chain
    # of tp_bwd_x_kernel<..., 5> on one slot per group -- yt, packed_mix * coeff, one fmaf per out-edge; the dot, * coeff)
    plain_ref = PlainRef(plan, ei.numpy(), n, True)
    pk = w_packed([f.numpy() for f in _packed_fields(packed)], bins.bin.cpu().numpy(), bins.coef.cpu().numpy())
    refs = reference(plain_ref, "bwd_xw_ptable", {"x": x.double().numpy(), "sh": sh.double().numpy(), "g": g.double().numpy()}, pk)
    for what, got in (("g_x", gx1), ("g_w", gw1)):
        ratio = within(f"{case['id']} {what}", got, refs[what])
        print(f"{case['id']} {what}: worst error / bound {ratio:.3f}")
        record_measured("test_gpu_tp_scalar_matrix", case=case["id"], output=what, error_over_bound=ratio)
    gx2, gw2 = plain()
    assert torch.equal(gx1.view(torch.int32), gx2.view(torch.int32)) and torch.equal(gw1.view(torch.int32), gw2.view(torch.int32)), \
        "two runs differ"

    # ---- embedded: wider rows of x / g_x, g_out and the table, the plan's blocks at shifted offsets
    pad = 64
    wide_groups, table_off, live_x = [], [], []
    tab_w = W + pad * (len(plan.groups) + 1)
    wide_tab = torch.zeros(bins.knots + 1, tab_w, device=dev)
    for i, grp in enumerate(plan.groups):
        (q,) = [q for q in range(8) if (grp.mask >> q) & 1]
        assert tp_slots(grp.l1)[q] == (grp.l1, 0)
        wg = L.TpGroup()
        C.memmove(C.byref(wg), C.byref(grp), C.sizeof(L.TpGroup))
        wg.x_off, wg.out_off[q] = grp.x_off + pad, grp.out_off[q] + pad
        wide_groups.append(wg)
        table_off.append(grp.w_off[q] + pad * (i + 1))
        wide_tab[:, table_off[-1]:table_off[-1] + grp.mul] = smooth[:, grp.w_off[q]:grp.w_off[q] + grp.mul]
        live_x.append((grp.x_off, (2 * grp.l1 + 1) * grp.mul))
    wide = ops.TpPlan(wide_groups, d_in + 2 * pad, 9, W, d_mid + 2 * pad)
    hw = wide.handle(dev)
    assert lib.e3k_tp_scalar_supported(hw) == 1
    Xw = torch.full((n, d_in + 2 * pad), float("nan"), device=dev)
    Xw[:, pad:pad + d_in] = X
    Gw_ = torch.full((n, d_mid + 2 * pad), float("nan"), device=dev)
    Gw_[:, pad:pad + d_mid] = Gm
    packed_w = radial_table.pack_raw(wide_tab, bins.knots)
    dead = torch.ones(tab_w, dtype=torch.bool, device=dev)
    for off, grp in zip(table_off, plan.groups):
        dead[off:off + grp.mul] = False
    flat = packed_w.view(bins.knots + 1, 3 * tab_w)      # a row: its tab_w (d0, d1) pairs, then its tab_w f16 pairs
    flat[:, :2 * tab_w].view(bins.knots + 1, tab_w, 2)[:, dead] = 0x7FC00000      # NaN in every record of a dead column
    flat[:, 2 * tab_w:][:, dead] = 0x7E007E00
    offs = (C.c_int32 * len(table_off))(*table_off)
    bx, gxw = _framed(n, d_in + 2 * pad, dev)
    bw, gww = _framed(e, W, dev)
    L.check(lib.e3k_tp_bwd_xw_scalar_ptable(hw, L.ptr(Xw), L.ptr(packed_w), tab_w, offs, L.ptr(erec), L.ptr(Gw_), L.ptr(topo.src_ptr), n, e,
                                            gxw.data_ptr(), gww.data_ptr(), L.stream_ptr()), "e3k_tp_bwd_xw_scalar_ptable (embedded)")
    torch.cuda.synchronize()
    assert route() == ROUTE and _margins_intact(bx) and _margins_intact(bw)
    inner = gxw[:, pad:pad + d_in]
    assert torch.equal(inner.contiguous().view(torch.int32), gx1.contiguous().view(torch.int32)), "embedded g_x differs from the plain run"
    assert torch.equal(gww.view(torch.int32), gw1.view(torch.int32)), "embedded g_w differs from the plain run"
    assert bool((gxw[:, :pad] == SENTINEL).all()) and bool((gxw[:, pad + d_in:] == SENTINEL).all()), "g_x written outside the groups' blocks"
    assert sum(wd for _, wd in live_x) == d_in

    # ---- refusals: nothing launched, outputs keep their bits
    dense = UVUTensorProduct("64x0e+64x1o", SH9, "1x0e+1x1o").plan
    hd = dense.handle(dev)
    assert lib.e3k_tp_scalar_supported(hd) == 0
    bx, gx = _framed(n, dense.d_in, dev)
    bw, gw = _framed(e, dense.w_numel, dev)
    r0 = route()
    rc = lib.e3k_tp_bwd_xw_scalar_ptable(hd, L.ptr(X), L.ptr(packed), 0, None, L.ptr(erec), L.ptr(Gm), L.ptr(topo.src_ptr), n, e,
                                         gx.data_ptr(), gw.data_ptr(), L.stream_ptr())
    torch.cuda.synchronize()
    assert rc == E3K_ERR_UNSUPPORTED and route() == r0
    assert bool((bx == SENTINEL).all()) and bool((bw == SENTINEL).all()), "a refused call wrote an output"


@pytest.mark.gpu
@pytest.mark.parametrize("case", EXPAND_CASES, ids=[c["id"] for c in EXPAND_CASES])
def test_expand_columns(dev, case):
    from e3_layers_amd.backend import lib as L

    lib = L.load()
    rows, w_src, w_dst, ranges = case["rows"], case["w_src"], case["w_dst"], case["ranges"]
    torch.manual_seed(7)
    src = torch.randn(rows, w_src, device=dev)
    buf, dst = _framed(rows, w_dst, dev)
    arr = lambda k: (C.c_int32 * len(ranges))(*[r[k] for r in ranges])
    L.check(lib.e3k_expand_columns(L.ptr(src), rows, w_src, w_dst, arr(0), arr(1), arr(2), len(ranges), dst.data_ptr(), L.stream_ptr()),
            "e3k_expand_columns")
    torch.cuda.synchronize()
    want = torch.zeros(rows, w_dst, device=dev)
    for s, d, ln in ranges:
        want[:, d:d + ln] = src[:, s:s + ln]
    assert torch.equal(dst.view(torch.int32), want.view(torch.int32))
    assert _margins_intact(buf)
    # refused: overlapping destination ranges, a column that is no multiple of four -- nothing written
    buf2, dst2 = _framed(rows, w_dst, dev)
    two = (C.c_int32 * 2)
    assert lib.e3k_expand_columns(L.ptr(src), rows, w_src, w_dst, two(0, 0), two(0, 4), two(8, 8), 2, dst2.data_ptr(), L.stream_ptr()) == -1
    assert lib.e3k_expand_columns(L.ptr(src), rows, w_src, w_dst, two(0, 0), two(2, 0), two(4, 0), 1, dst2.data_ptr(), L.stream_ptr()) == E3K_ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert bool((buf2 == SENTINEL).all())
