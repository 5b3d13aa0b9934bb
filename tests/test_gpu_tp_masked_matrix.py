"""The masked input-gradient walk (csrc/e3k_tp_masked.hip: e3k_tp_bwd_xw_masked_ptable) through its C entry, against float64 on the
CPU and, bit for bit, against the dense walk (e3k_tp_bwd_xw_ptable).

The dense plan is the tensor product of the layer below the last convolution of config_energy at l_max 2: six 64-channel groups
(l1 = 0, 0, 1, 1, 2, 2) with every slot up to l3 = 2, 30 slots, 1 920 weight columns, 6 528 columns of mid
(tests/test_live_chain_host.py holds ``SHIPPED_LMAX2`` to the model).  A case is a set of live slots, one mask per dense group; the
pruned plan keeps the live groups with their masks and numbers the weight columns compactly, as NativeLayer.narrow builds it.

Graph: 23 nodes, 157 edges; node 22 has no out-edge, node 21 exactly one (one more case: 203 nodes, above the N >= 64 work-order
threshold).  Per case:

* g_x [N, d_in] and g_w [E, w_live] against the float64 oracle of tests/test_gpu_tp_matrix.py (path weights decoded from the packed
  table on the host, g_mid zero on the dead columns) at that file's bound GTOL, over everything and on the rows of the two special
  nodes / their edges -- the comparison tests/test_gpu_tp_scalar_matrix.py makes;
* both bit for bit against the dense walk run on a g_mid whose dead columns are zero (the live columns of its g_w);
* the masked call gets NaN in every dead column of g_mid and in every record of a dead column of the packed table: neither is read;
* g_w lies in a sentinel-filled buffer with a margin in front and behind, g_x likewise (its inside zero-filled, as the entry's
  contract asks): the margins keep their bits; two runs give the same bits.

The l_max 3 layer (l1 = 3 groups, a split plan) has no masked form: e3k_tp_masked_supported refuses it, which the last test checks
on a plan with an l3 = 3 slot.
"""
import ctypes as C

import pytest
import torch

import numpy as np

from tests.test_gpu_tp_matrix import (E3K_ERR_UNSUPPORTED, GTOL, SH9, PlainRef, _check_packing, _Oracle, _packed_fields, _packed_w64, reference,
                                      w_packed, within)
from tests.test_gpu_tp_scalar_matrix import SENTINEL, _framed, _margins_intact
from tests.util import record_measured, rel_err

ROUTE = "tp_bwd_xw_masked_kernel"
LEFT = "64x0e+64x0o+64x1o+64x1e+64x2e+64x2o"
OUT = "1x0e+1x0o+1x1o+1x1e+1x2e+1x2o"
DENSE_MASKS = (7, 7, 63, 63, 119, 119)
# the live slots of that layer when the last layer's narrow backward hands it a gradient on columns (0, 64), (320, 512), (512, 832)
SHIPPED_LMAX2 = (7, 0, 36, 27, 83, 36)


def _single(group, q):
    return tuple((1 << q) if gi == group else 0 for gi in range(6))


CASES = ([{"id": "shipped_lmax2", "masks": SHIPPED_LMAX2, "n": 23, "e": 157},
          {"id": "shipped_lmax2_n203", "masks": SHIPPED_LMAX2, "n": 203, "e": 1203}]
         + [{"id": f"l1_1_slot{q}", "masks": _single(2, q), "n": 23, "e": 157} for q in range(6)]
         + [{"id": f"l1_2_slot{q}", "masks": _single(4, q), "n": 23, "e": 157} for q in (0, 1, 2, 4, 5, 6)])
KERNELS = {ROUTE}
_SETUPS = {}


def _edges(n, e, seed):
    """node n - 1 sends nothing, node n - 2 exactly one edge; everyone receives"""
    g = torch.Generator().manual_seed(seed)
    src = torch.randint(0, n - 2, (e,), generator=g)
    dst = torch.randint(0, n, (e,), generator=g)
    src[e // 2] = n - 2
    return torch.stack([src, dst]).long()


def _setup(n, e, dev):
    """everything the cases of one graph share: inputs, the packed table, the dense plan and the float64 oracle (left unchanged)"""
    key = (n, e, str(dev))
    if key in _SETUPS:
        return _SETUPS[key]
    from e3_layers_amd.backend import radial_table
    from e3_layers_amd.backend.graph import build_topology
    from e3_layers_amd.nn.core import UVUTensorProduct

    torch.manual_seed(4100 + n)
    tpm = UVUTensorProduct(LEFT, SH9, OUT)
    plan = tpm.plan
    assert tuple(g.mask for g in plan.groups) == DENSE_MASKS and plan.w_numel == 1920 and plan.d_mid == 6528
    ei = _edges(n, e, 11 + n)
    orc = _Oracle(LEFT, SH9, OUT, tpm.irreps_mid_simplified, ei, n)
    topo = build_topology(ei.to(dev), n)
    rnd = lambda *shape: torch.randn(*shape, dtype=torch.float64).float()
    x, g, sh = rnd(n, plan.d_in), rnd(n, plan.d_mid), rnd(e, 9)
    radius = torch.rand(e, dtype=torch.float64).float() * 5.2
    radius[:3] = torch.tensor([0.0, 5.0, 0.01])
    bins = radial_table.build_bins(radius.to(dev), 5.0, 128)
    rows_r = torch.arange(bins.knots + 1, dtype=torch.float64) * bins.spacing
    cols = torch.arange(plan.w_numel, dtype=torch.float64)
    smooth = (torch.sin(rows_r[:, None] * (1.0 + 5.0 * cols[None, :] / plan.w_numel)) * torch.exp(-0.2 * rows_r[:, None])).float().to(dev)
    packed = radial_table.pack_raw(smooth, bins.knots)
    _check_packing(smooth, packed, bins.knots)
    s = dict(plan=plan, ei=ei, orc=orc, topo=topo, x=x, g=g, sh=sh, X=x.to(dev), bins=bins, packed=packed,
             erec=bins.records(topo, sh.to(dev), "src"), w_pk=_packed_w64(packed, bins))
    _SETUPS[key] = s
    return s


def _pruned(plan, masks):
    """(live groups with their masks and compact weight columns, the live slots' dense columns in (group, slot) order, live
    columns of mid)"""
    from e3_layers_amd.backend import lib as L
    from e3_layers_amd.nn.core import tp_slots

    groups, live_col, mid, pos = [], [], [], 0
    for g, m in zip(plan.groups, masks):
        assert m & ~g.mask == 0
        if not m:
            continue
        n = L.TpGroup()
        n.l1, n.x_off, n.mul, n.mask = g.l1, g.x_off, g.mul, m
        for t in range(4):
            n.y_off[t] = g.y_off[t]
        for q in range(8):
            if (m >> q) & 1:
                n.w_off[q], n.out_off[q], n.out_stride[q], n.coeff[q] = pos, g.out_off[q], g.out_stride[q], g.coeff[q]
                pos += g.mul
                live_col.append(g.w_off[q])
                mid += [(g.out_off[q] + k * g.out_stride[q], g.mul) for k in range(2 * tp_slots(g.l1)[q][1] + 1)]
        groups.append(n)
    return groups, live_col, mid, pos


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=[c["id"] for c in CASES])
def test_masked_walk_against_float64_and_the_dense_walk(dev, case):
    from e3_layers_amd.backend import lib as L
    from e3_layers_amd.backend import ops

    lib = L.load()
    n, e = case["n"], case["e"]
    s = _setup(n, e, dev)
    plan, topo, X, packed, erec = s["plan"], s["topo"], s["X"], s["packed"], s["erec"]
    d_in, W, d_mid = plan.d_in, plan.w_numel, plan.d_mid
    groups, live_col, mid, w_live = _pruned(plan, case["masks"])
    live_mid = torch.zeros(d_mid, dtype=torch.bool)
    for off, mul in mid:
        assert not bool(live_mid[off:off + mul].any())
        live_mid[off:off + mul] = True
    live_w = torch.zeros(W, dtype=torch.bool)
    for off in live_col:
        live_w[off:off + 64] = True
    assert int(live_w.sum()) == w_live
    if case["masks"] == SHIPPED_LMAX2:
        assert len(live_col) == 15 and w_live == 960 and int(live_mid.sum()) == 3264
    g_zero = s["g"].clone()
    g_zero[:, ~live_mid] = 0.0
    g_nan = s["g"].clone()
    g_nan[:, ~live_mid] = float("nan")
    Gz, Gn = g_zero.to(dev), g_nan.to(dev)
    # every record of a dead column of the table is NaN for the masked call (a row: its W (d0, d1) pairs, then its W f16 pairs)
    packed_m = packed.clone()
    flat = packed_m.view(packed.shape[0], 3 * W)
    dead_w = (~live_w).to(dev)
    flat[:, :2 * W].view(packed.shape[0], W, 2)[:, dead_w] = 0x7FC00000
    flat[:, 2 * W:][:, dead_w] = 0x7E007E00

    def route():
        r = lib.e3k_tp_last_route()
        return r.decode() if r is not None else None

    # ---- the dense walk on the zeroed g_mid
    hd = plan.handle(dev)
    gx_d = torch.full((n, d_in), SENTINEL, device=dev)
    gw_d = torch.full((e, W), SENTINEL, device=dev)
    L.check(lib.e3k_tp_bwd_xw_ptable(hd, L.ptr(X), L.ptr(packed), L.ptr(erec), L.ptr(Gz), L.ptr(topo.src_ptr), n, e, gx_d.data_ptr(),
                                     gw_d.data_ptr(), L.stream_ptr()), "e3k_tp_bwd_xw_ptable")
    torch.cuda.synchronize()
    assert route().startswith("tp_bwd_x_kernel<2, 2, false, true, 5>"), route()

    # ---- the masked walk on the pruned plan
    pruned = ops.TpPlan(groups, d_in, 9, w_live, d_mid)
    hm = pruned.handle(dev)
    assert lib.e3k_tp_masked_supported(hm) == 1
    cols = (C.c_int32 * len(live_col))(*live_col)

    def masked():
        bx, gx = _framed(n, d_in, dev)
        gx.zero_()      # (the entry's contract: the caller zero-fills what no live group owns)
        bw, gw = _framed(e, w_live, dev)
        L.check(lib.e3k_tp_bwd_xw_masked_ptable(hm, L.ptr(X), L.ptr(packed_m), W, cols, L.ptr(erec), L.ptr(Gn), L.ptr(topo.src_ptr), n, e,
                                                gx.data_ptr(), gw.data_ptr(), L.stream_ptr()), "e3k_tp_bwd_xw_masked_ptable")
        torch.cuda.synchronize()
        assert route() == ROUTE, route()
        assert _margins_intact(bx) and _margins_intact(bw), "a word outside an output changed"
        return gx, gw

    gx1, gw1 = masked()
    gx2, gw2 = masked()
    assert torch.equal(gx1.view(torch.int32), gx2.view(torch.int32)) and torch.equal(gw1.view(torch.int32), gw2.view(torch.int32)), \
        "two runs differ"
    assert bool(torch.isfinite(gx1).all()) and bool(torch.isfinite(gw1).all()), "an element is not finite: a dead column was read"

    # ---- bit for bit against the dense walk
    assert torch.equal(gx1.contiguous().view(torch.int32), gx_d.view(torch.int32)), "g_x differs from the dense walk's bits"
    assert torch.equal(gw1.contiguous().view(torch.int32), gw_d[:, live_w.to(dev)].contiguous().view(torch.int32)), \
        "g_w differs from the live columns of the dense walk's"
    assert bool((gw_d[:, dead_w] == 0).all())

    # ---- float64
    PGx, _, RGw = s["orc"].G(s["x"].double(), s["sh"].double(), s["w_pk"], g_zero.double())
    assert bool((RGw[:, ~live_w] == 0).all()) and bool((RGw[:, live_w] != 0).any())
    RGw = RGw[:, live_w]
    lone, none = n - 2, n - 1
    e_lone = (s["ei"][0] == lone).nonzero().flatten()
    assert len(e_lone) == 1 and not bool((s["ei"][0] == none).any())
    gx, gw = gx1.detach().double().cpu(), gw1.detach().double().cpu()
    for what, got, ref, rows in (("g_x", gx, PGx, [lone, 0, 1]), ("g_w", gw, RGw, e_lone)):
        err, err_r = rel_err(got, ref), rel_err(got[rows], ref[rows])
        print(f"{case['id']} {what}: rel err {err:.3e}, on the special rows {err_r:.3e} (bound {GTOL:.0e})")
        assert err < GTOL and err_r < GTOL, f"{what}: rel err {err:.3e} / {err_r:.3e}"
    assert bool((gx[none] == 0).all()), "the row of the node without out-edges is not exactly zero"

    # ---- element by element: the plain reference over the PRUNED plan's paths (the dead columns of g_mid and of the table are no
    # operand of it, so they add nothing to M; g_w is w_live wide) and its bound gamma_k M (tests/test_gpu_tp_matrix.py)
    assert live_col == sorted(live_col)      # (the compact columns are the live dense columns in their order)
    plain_ref = PlainRef(pruned, s["ei"].numpy(), n, True)
    w_d, M_d, k_w = w_packed([f.numpy() for f in _packed_fields(packed)], s["bins"].bin.cpu().numpy(), s["bins"].coef.cpu().numpy())
    lw = live_w.numpy()
    refs = reference(plain_ref, "bwd_xw_ptable", {"x": s["x"].double().numpy(), "sh": s["sh"].double().numpy(), "g": g_zero.double().numpy()},
                     (np.ascontiguousarray(w_d[:, lw]), np.ascontiguousarray(M_d[:, lw]), k_w))
    assert refs["g_w"][0].shape == (e, w_live)
    for what, got in (("g_x", gx1), ("g_w", gw1)):
        ratio = within(f"{case['id']} {what}", got.contiguous(), refs[what])
        print(f"{case['id']} {what}: worst error / bound {ratio:.3f}")
        record_measured("test_gpu_tp_masked_matrix", case=case["id"], output=what, error_over_bound=ratio)


@pytest.mark.gpu
def test_unsupported_plans_are_refused_and_write_nothing(dev):
    from e3_layers_amd.backend import lib as L
    from e3_layers_amd.nn.core import UVUTensorProduct

    lib = L.load()
    n, e = 23, 157
    s = _setup(n, e, dev)
    bad = UVUTensorProduct("64x2e", SH9, "1x2e+1x3e").plan      # a slot with l3 = 3
    assert any((g.mask >> 7) & 1 or (g.mask >> 3) & 1 for g in bad.groups)
    hb = bad.handle(dev)
    assert lib.e3k_tp_masked_supported(hb) == 0
    bx, gx = _framed(n, bad.d_in, dev)
    bw, gw = _framed(e, bad.w_numel, dev)
    r0 = lib.e3k_tp_last_route()
    rc = lib.e3k_tp_bwd_xw_masked_ptable(hb, L.ptr(s["X"]), L.ptr(s["packed"]), 0, None, L.ptr(s["erec"]), L.ptr(s["g"].to(dev)),
                                         L.ptr(s["topo"].src_ptr), n, e, gx.data_ptr(), gw.data_ptr(), L.stream_ptr())
    torch.cuda.synchronize()
    assert rc == E3K_ERR_UNSUPPORTED and lib.e3k_tp_last_route() == r0
    assert bool((bx == SENTINEL).all()) and bool((bw == SENTINEL).all()), "a refused call wrote an output"
