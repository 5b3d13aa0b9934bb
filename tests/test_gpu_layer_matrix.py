"""The kernels csrc/e3k_layer.hip launches itself (gather_rows_kernel, scatter_rows_kernel, the zero fill) and the entries that reach
them -- e3k_kw_stack_fwd / e3k_kw_stack_bwd, and e3k_layer_fwd / e3k_layer_bwd with have_m = 0 -- through the C ABI, element by element.

Layer handles are the library's own: conv_native.native_layer(plan).handle(dev) on the plans of small built models (no
e3k_layer_desc is written by hand) -- the 64-channel model of tests/test_gpu_head_backward.py (V = 20, ld_m 12 288 .. 36 864), a
16-channel one (ld_m 768 .. 2 304; its radial MLP keeps 32 hidden units, the narrowest the executor's fused hidden chain takes, so
that the layers have a plan at all) and the 16-channel one with node_attrs = "1x0e" (V = 1), on which n_keys * V -- the element count
the gather / scatter grids are sized by -- takes the values 1, 255, 256, 257 and 700 (three blocks).

Every buffer of a case sits in ONE NaN-filled arena with slack round every buffer (tests/test_gpu_node_matrix.py's).  Every word
include/e3k.h says a call writes is claimed by exactly one comparison, every other word must keep its bits:

* a_rep: the bits of node_attrs[reps[k]] (the gather is a copy);
* M, the weight gradients and ga: the float64 reference and the per-element bounds of tests/test_gpu_node_matrix.py (kw_reference:
  gamma_V |a| |W|, gamma_{K + 1} (|a|^T |g_M| + |old|), gamma_{total + 1} |g_M| |W|; integer cases are exact and compared with ==);
* g_attrs: zero except the representative rows of the keys that HAVE rows, which hold the values of the device's own ga rows (the
  scatter adds each value once into zero).  A key with no rows (bounds[2k + 1] == 0, reps[k] == 0) carries a NONZERO g_M row in the
  stack cases, so its ga row is not zero: row 0 of g_attrs must still receive nothing from it;
* gm on the have_m = 0 route: the keyed weight-gradient GEMM into a buffer the executor zero-fills, against float64 of the call's own
  operands with the bound of tests/test_gpu_wgrad_rider.py ((n + 8) u |A|^T |G|), and exactly zero where no problem writes;
* the executor's other outputs on that route (conv, x1, mid, y; g_conv, g_mid: the GEMM, gate and tensor-product kernels' work,
  held element by element by their own matrices) are claimed and must be finite; the layer runs without edges (E = 0: mid is
  exactly zero), which leaves the keyed route -- gather, keyed weights, keyed GEMMs, their backward, scatter -- whole.

Refusals return their code and leave every word of the arena as it was.
"""
import ctypes as C
import zlib

import numpy as np
import pytest
import torch

from tests.test_gpu_node_matrix import (E3K_ERR_INVALID, E3K_ERR_UNSUPPORTED, E3K_OK, FL, Arena, Check as _Check, gamma, kw_inputs, kw_layout,
                                        kw_reference)
from tests.test_gpu_wgrad_rider import _wgrad_set_reference
from tests.util import record_measured

pytestmark = pytest.mark.gpu
f32 = np.float32
GATHER, SCATTER, ZERO = "gather_rows_kernel", "scatter_rows_kernel", "zero_words_kernel"
WORST = {}


class Check(_Check):
    def finish(self):
        self.unchanged()
        for family, r in self.ratios.items():
            print(f"{self.case['id']}: {family} worst error / bound {r:.3f}")
            WORST[family] = max(WORST.get(family, 0.0), r)
            record_measured("test_gpu_layer_matrix", case=self.case["id"], family=family, error_over_bound=r)


# ---------------------------------------------------------------------------------------------------------------------------------
# the models whose plans the handles come from
_MODELS = {}


def _tree(n_dim, node_attrs):
    from e3_layers_amd.configs.layer_configs import addEnergyOutput, featureModel

    cfg = featureModel(n_dim=n_dim, l_max=2, edge_spherical="1x0e+1x1o+1x2e", node_attrs=node_attrs, edge_radial="8x0e", num_types=10,
                       num_layers=3, r_max=4.0)
    for _, lay in cfg.layers:      # (the fused hidden chain takes 32 or 64 units: a 16-unit MLP has no executor layer)
        if isinstance(lay, dict) and "convolution" in lay:
            lay["convolution"]["invariant_neurons"] = max(32, n_dim)
    return addEnergyOutput(cfg, None)


MODEL_TREES = {"d64": (64, "20x0e"), "d16": (16, "20x0e"), "v1": (16, "1x0e")}


def model(name):
    """(the three MessagePassing layers, their plans) of a built model; built once, on the host"""
    if name not in _MODELS:
        from e3_layers_amd.utils import build

        torch.manual_seed(0)
        m = build(_tree(*MODEL_TREES[name]))
        layers = [m.layer0, m.layer1, m.layer2]
        plans = [lay._block_plan() for lay in layers]
        assert all(p is not None and p.sc_spec is not None for p in plans)
        _MODELS[name] = (layers, plans)
    return _MODELS[name]


def kw_instr(plan):
    """[(u, w_out)] of a plan's keyed-weight instructions, in the layout tests/test_gpu_node_matrix.py's reference assumes"""
    from e3_layers_amd.backend import ops

    arr = ops._kw_array(plan.sc_spec, plan.sc_m_off)
    instr = [(int(k.u), int(k.w_out)) for k in arr]
    lay, n_w, total = kw_layout(instr, plan.sc_spec.v)
    assert [(int(k.w_off), int(k.m_off)) for k in arr] == [(w, m) for w, m, _, _ in lay] and total == plan.sc_ld_m
    return instr, n_w, total


# ---------------------------------------------------------------------------------------------------------------------------------
# the case table
def kws(id_, why, model_, layers, K, N, empty=(), ends=False, ga="together", null_w=(), acc=0, exact=False, shift=0):
    """shift: words by which ga starts behind a 16-byte boundary (the zero fill's head and tail words)"""
    kernels = {GATHER} | ({SCATTER, ZERO} if ga != "none" else set())
    return dict(id=id_, why=why, kind="kws", rc=E3K_OK, model=model_, layers=list(layers), K=K, N=N, empty=tuple(empty), ends=ends, ga=ga,
                null_w=tuple(null_w), acc=acc, exact=exact, shift=shift, kernels=kernels)


def lay(id_, why, model_, layer, K, N, empty=(), ends=False, attrs=True, acc=0):
    return dict(id=id_, why=why, kind="layer", rc=E3K_OK, model=model_, layers=[layer], K=K, N=N, empty=tuple(empty), ends=ends, attrs=attrs,
                acc=acc, exact=False, kernels={GATHER, ZERO} | ({SCATTER} if attrs else set()))


def refuse(id_, why, fn, rc, **over):
    return dict(id=id_, why=why, kind="refuse", fn=fn, rc=rc, over=over, kernels=set(), K=3, N=7)


CASES = [
    # ---- the gather / scatter grids: n_keys * V elements, 256 per block
    kws("kws_v1_1", "one element, one block", "v1", [0], 1, 3, exact=True),
    kws("kws_v1_255", "one short of a block; a key without rows", "v1", [0], 255, 300, empty=(0, 17, 254), exact=True),
    kws("kws_v1_256", "exactly one block", "v1", [0], 256, 256, exact=True, ga="apart"),
    kws("kws_v1_257", "one element in the second block; representatives at row 0 and at row N - 1", "v1", [0], 257, 300, ends=True, exact=True, shift=3),
    kws("kws_v1_700", "three blocks; keys without rows in each", "v1", [0], 700, 811, empty=(3, 255, 256, 699), exact=True, acc=1),
    kws("kws_v20_ends", "two keys, their representatives the first and the last row", "d16", [0], 2, 9, ends=True, exact=True),
    # ---- the stack entries
    kws("kws_1_together", "one layer; ga and g_attrs in one allocation", "d16", [0], 5, 23, empty=(2,)),
    kws("kws_3_apart", "three layers of different ld_m; two allocations; a frozen middle layer", "d16", [0, 1, 2], 5, 23, empty=(0, 4), ga="apart", null_w=(1,), shift=1),
    kws("kws_3_none", "three layers, the attributes need no gradient", "d16", [0, 1, 2], 5, 23, empty=(1,), ga="none", acc=1),
    kws("kws_3_only_attrs", "every layer's weights frozen: the attribute gradient alone", "d16", [0, 1, 2], 4, 11, null_w=(0, 1, 2)),
    kws("kws_8", "eight layers (the limit), accumulated into known values, some frozen", "d16", [0, 1, 2, 0, 1, 2, 0, 1], 6, 40, empty=(5,), acc=1, null_w=(0, 7)),
    kws("kws_8_exact", "eight layers, integers", "d16", [2, 1, 0, 2, 1, 0, 2, 1], 3, 8, exact=True),
    kws("kws_64", "the 64-channel layers", "d64", [0, 1, 2], 4, 9, empty=(3,), acc=1),
    # ---- the executor's own keyed-weight route (have_m = 0)
    lay("layer_v1_1", "n_keys * V = 1", "v1", 0, 1, 4),
    lay("layer_v1_255", "n_keys * V = 255; keys without rows", "v1", 0, 255, 300, empty=(0, 254)),
    lay("layer_v1_256", "n_keys * V = 256", "v1", 0, 256, 256),
    lay("layer_v1_257", "n_keys * V = 257; representatives at row 0 and at row N - 1", "v1", 0, 257, 300, ends=True),
    lay("layer_v1_700", "three blocks", "v1", 0, 700, 811, empty=(3, 256), acc=1),
    lay("layer_v20", "V = 20", "d16", 0, 5, 23, empty=(2,)),
    lay("layer_v20_weights_only", "the attributes need no gradient: no scatter, no ga", "d16", 1, 5, 23, attrs=False, acc=1),
    lay("layer_v20_64", "a 64-channel layer with three keyed instructions", "d64", 1, 4, 9, ends=True),
    # ---- refusals
    refuse("kws_fwd_n0", "no layer", "fwd", E3K_ERR_INVALID, n=0), refuse("kws_fwd_n9", "nine layers", "fwd", E3K_ERR_INVALID, n=9),
    refuse("kws_bwd_n0", "no layer", "bwd", E3K_ERR_INVALID, n=0), refuse("kws_bwd_n9", "nine layers", "bwd", E3K_ERR_INVALID, n=9),
    refuse("kws_fwd_V", "a layer with another V", "fwd", E3K_ERR_UNSUPPORTED, other_v=True),
    refuse("kws_bwd_V", "a layer with another V", "bwd", E3K_ERR_UNSUPPORTED, other_v=True),
    refuse("kws_fwd_no_sc", "a layer without a self-connection", "fwd", E3K_ERR_UNSUPPORTED, no_sc=True),
    refuse("kws_bwd_no_sc", "a layer without a self-connection", "bwd", E3K_ERR_UNSUPPORTED, no_sc=True),
    refuse("kws_bwd_ga_alone", "ga without g_attrs", "bwd", E3K_ERR_INVALID, g_attrs=None),
    refuse("kws_bwd_g_attrs_alone", "g_attrs without ga", "bwd", E3K_ERR_INVALID, ga=None),
    refuse("kws_bwd_no_reps", "g_attrs without reps", "bwd", E3K_ERR_INVALID, reps=None),
    refuse("kws_bwd_no_bounds", "g_attrs without bounds", "bwd", E3K_ERR_INVALID, bounds=None),
    refuse("narrow_bwd_own_radial", "a narrow layer asked for its own last-layer gradient", "narrow_bwd", E3K_ERR_UNSUPPORTED, gb_last=True),
    refuse("narrow_bwd_no_compact_table_gradient", "a narrow layer without g_T_live", "narrow_bwd", E3K_ERR_UNSUPPORTED, g_T_live=None),
    refuse("narrow_fwd", "a narrow layer describes a backward", "narrow_fwd", E3K_ERR_UNSUPPORTED),
]


def table_kernels():
    return set().union(*[c["kernels"] for c in CASES])


# ---------------------------------------------------------------------------------------------------------------------------------
def _rng(c, tag=""):
    return np.random.default_rng(zlib.crc32((c["id"] + tag).encode()))


def key_structure(c):
    """reps int64 [K], bounds int32 [2K] (start, count), perm int32 [N]: the rows grouped by key; a key in c['empty'] has no rows,
    reps = 0 and count 0; with c['ends'] key 0's representative is row 0 and key 1's is row N - 1"""
    K, N, rng = c["K"], c["N"], _rng(c, ":keys")
    live = [k for k in range(K) if k not in c["empty"]]
    assert len(live) <= N and live
    rows = rng.permutation(N)
    if c["ends"]:
        assert live[:2] == [0, 1] and N >= 2
        rows = np.array([0, N - 1] + [r for r in rows if r not in (0, N - 1)])
    # every live key one row first (its representative), the remaining rows dealt out at random
    owner = np.concatenate([np.array(live), rng.choice(live, N - len(live))]) if N > len(live) else np.array(live)
    reps, bounds, perm, pos = np.zeros(K, np.int64), np.zeros(2 * K, np.int32), np.zeros(N, np.int32), 0
    for k in range(K):
        mine = rows[:len(owner)][owner == k]
        bounds[2 * k], bounds[2 * k + 1] = pos, len(mine)
        perm[pos:pos + len(mine)] = mine
        pos += len(mine)
        reps[k] = mine[0] if len(mine) else 0
    assert pos == N and all(bounds[2 * k + 1] == 0 for k in c["empty"])
    if c["ends"]:
        assert reps[0] == 0 and reps[1] == N - 1
    return reps, bounds, perm


def draw(c, rng, *shape):
    if c["exact"]:
        return rng.integers(-4, 5, shape, dtype=np.int8).astype(f32)
    return rng.standard_normal(shape, dtype=f32)


def handles_of(dev, c):
    from e3_layers_amd.backend import conv_native

    _, plans = model(c["model"])
    chosen = [plans[i] for i in c["layers"]]
    hs = [conv_native.native_layer(p).handle(dev) for p in chosen]
    return chosen, (C.c_void_p * max(len(hs), 1))(*hs)


def scatter_reference(ga_dev, reps, bounds, N, V):
    want = np.zeros((N, V), np.float64)
    for k, r in enumerate(reps):
        if bounds[2 * k + 1] > 0:
            want[r] += ga_dev[k]
    return want


def run_kws(dev, c, L):
    lib, st = L.load(), L.stream_ptr()
    plans, handles = handles_of(dev, c)
    n, K, N, V = len(plans), c["K"], c["N"], plans[0].sc_spec.v
    reps, bounds, _ = key_structure(c)
    rng = _rng(c)
    attrs = draw(c, rng, N, V)
    a_rep = attrs[reps]
    ar = Arena(zlib.crc32(c["id"].encode()) ^ 0x1A7E)
    ar.alloc("attrs", N * V, attrs).alloc("reps", 2 * K, reps.view(np.int32)).alloc("bounds", 2 * K, bounds).out("a_rep", K * V)
    layers = []
    for i, p in enumerate(plans):
        instr, n_w, total = kw_instr(p)
        inp = kw_inputs(dict(c, V=V), instr, tag=f":{i}")
        inp = dict(inp, a=a_rep, old_ga=np.zeros((K, V), f32))
        acc = c["acc"]
        ar.alloc(f"W{i}", n_w, inp["W"]).out(f"M{i}", K * total).alloc(f"gM{i}", K * total, inp["gM"])
        ar.alloc(f"gW{i}", n_w, inp["old_gW"] if acc else None)      # (acc = 0: the NaN sentinel)
        layers.append((instr, n_w, total, inp, kw_reference(dict(c, V=V), inp, instr, acc=acc)))
    ws_n = int(lib.e3k_kw_stack_bwd_workspace(handles, n, K))
    assert ws_n == sum((t + 255) // 256 for _, _, t, _, _ in layers) * K * V
    if c["ga"] == "together":      # ga directly in front of g_attrs
        ar.alloc("ga", K * V, None, 4, c["shift"])
        ar.blocks["g_attrs"] = (ar.blocks["ga"][0] + K * V, N * V)
        ar.n += N * V
    elif c["ga"] == "apart":
        ar.alloc("ga", K * V, None, 4, c["shift"]).out("g_attrs", N * V)
    ar.out("ws", max(ws_n, 1)).upload(dev)
    if c["ga"] == "apart":
        assert ar.p("g_attrs") != ar.p("ga") + 4 * K * V
    items = (L.KwStackItem * n)()
    for i in range(n):
        items[i].w_sc, items[i].m = ar.p(f"W{i}"), ar.p(f"M{i}")
    assert lib.e3k_kw_stack_fwd(handles, items, n, ar.p("attrs"), ar.p("reps"), K, ar.p("a_rep"), st) == E3K_OK
    for i in range(n):
        items[i].m = ar.p(f"gM{i}")
        items[i].gb_sc, items[i].acc_sc = (None if i in c["null_w"] else ar.p(f"gW{i}")), c["acc"]
    with_a = c["ga"] != "none"
    rc = lib.e3k_kw_stack_bwd(handles, items, n, ar.p("a_rep"), ar.p("reps"), ar.p("bounds"), N, K, ar.p("ga") if with_a else None,
                              ar.p("g_attrs") if with_a else None, ar.p("ws") if with_a else None, st)
    assert rc == E3K_OK
    ck = Check(ar, c)
    ck.exact("a_rep", a_rep)
    ga, S = np.zeros((K, V)), np.zeros((K, V))
    for i, (instr, n_w, total, inp, ref) in enumerate(layers):
        ga = ga + ref["g_a"][0]
        if not c["exact"]:
            S = S + (ref["g_a"][1] - FL) / gamma(total + 1)
        for name, key in ((f"M{i}", "M"), (f"gW{i}", "g_W")):
            if key == "g_W" and i in c["null_w"]:
                continue      # (not claimed: the sentinel, or the known values, must still be there)
            ck.equal(name, ref[key][0]) if c["exact"] else ck.close(name, *ref[key], "kw_stack_" + key)
    if with_a:
        total_all = sum(t for _, _, t, _, _ in layers)
        ck.equal("ga", ga) if c["exact"] else ck.close("ga", ga, gamma(total_all + 1) * S + FL, "kw_stack_g_a")
        ga_dev = ck.dev("ga", np.float32).astype(np.float64).reshape(K, V)
        for k in c["empty"]:
            assert np.abs(ga_dev[k]).max() > 0, "the ga row of a key without rows is zero here: the bounds check would not be exercised"
        ck.equal("g_attrs", scatter_reference(ga_dev, reps, bounds, N, V))
        ck.free("ws", ws_n)
    ck.finish()


def run_layer(dev, c, L):
    """e3k_layer_fwd and e3k_layer_bwd with have_m = 0 on a batch without edges"""
    from e3_layers_amd.backend import conv_native, ops

    lib, st = L.load(), L.stream_ptr()
    (plan,), handles = handles_of(dev, c)
    layer_mod = model(c["model"])[0][c["layers"][0]]
    d = conv_native.native_layer(plan).desc
    K, N, V, ld = c["K"], c["N"], int(d.V), int(d.ld_m)
    instr, n_w, total = kw_instr(plan)
    assert total == ld and n_w == layer_mod.conv.sc.weight.numel()
    n_lin1, n_post = layer_mod.conv.linear_1.weight.numel(), layer_mod.conv.tp.linear.weight.numel()
    reps, bounds, perm = key_structure(c)
    rng = _rng(c)
    attrs = rng.standard_normal((N, V), dtype=f32)
    w_sc = (0.2 * rng.standard_normal(n_w)).astype(f32)
    old_gw = rng.standard_normal(n_w, dtype=f32)
    kw_arr = ops._kw_array(plan.sc_spec, plan.sc_m_off)
    ws_n = int(lib.e3k_keyed_weights_bwd_workspace(kw_arr, len(instr), K, V)) if c["attrs"] else 0
    ar = Arena(zlib.crc32(c["id"].encode()) ^ 0x1A7E)
    ar.alloc("x", N * d.d_in, rng.standard_normal(N * d.d_in, dtype=f32)).alloc("attrs", N * V, attrs)
    ar.alloc("reps", 2 * K, reps.view(np.int32)).alloc("bounds", 2 * K, bounds).alloc("perm", N, perm)
    ar.alloc("w_lin1", n_lin1, (0.2 * rng.standard_normal(n_lin1)).astype(f32)).alloc("w_post", n_post, (0.2 * rng.standard_normal(n_post)).astype(f32))
    ar.alloc("w_sc", n_w, w_sc).alloc("gy", N * d.d_out, rng.standard_normal(N * d.d_out, dtype=f32))
    ar.alloc("sh", 16, np.zeros(16, f32)).alloc("w", 16, np.zeros(16, f32)).alloc("edges", 8, np.zeros(8, np.int32))
    ar.alloc("dst_ptr", N + 1, np.zeros(N + 1, np.int32))
    for name, size in (("a_rep", K * V), ("m", K * ld), ("conv", N * d.d_conv), ("x1", N * d.d_x1), ("mid", N * d.d_mid), ("y", N * d.d_out),
                       ("g_conv", N * d.d_conv), ("g_mid", N * d.d_mid), ("gm", K * ld)):
        ar.out(name, size)
    ar.alloc("gb_sc", n_w, old_gw) if c["acc"] else ar.out("gb_sc", n_w)
    if c["attrs"]:
        ar.out("ga", K * V).out("g_attrs", N * V).out("kw_ws", max(ws_n, 1))
    ar.upload(dev)
    f = L.LayerFwdArgs()
    f.N, f.E, f.in_cf, f.out_cf, f.keep, f.fork, f.has_w, f.n_keys, f.have_m = N, 0, 1, 1, 1, 0, 0, K, 0
    f.main = f.side = f.side2 = st
    f.x, f.node_attrs, f.sh = ar.p("x"), ar.p("attrs"), ar.p("sh")
    f.src, f.dst_ptr, f.dst_perm = ar.p("edges"), ar.p("dst_ptr"), ar.p("edges")
    f.perm, f.bounds, f.reps = ar.p("perm"), ar.p("bounds"), ar.p("reps")
    f.w_lin1, f.w_post, f.w_sc = ar.p("w_lin1"), ar.p("w_post"), ar.p("w_sc")
    f.rad.w = ar.p("w")
    f.a_rep, f.m, f.conv, f.x1, f.mid, f.y = (ar.p(k) for k in ("a_rep", "m", "conv", "x1", "mid", "y"))
    assert lib.e3k_layer_fwd(handles[0], C.byref(f)) == E3K_OK
    b = L.LayerBwdArgs()
    b.N, b.E, b.in_cf, b.out_cf, b.fork, b.n_keys = N, 0, 1, 1, 0, K
    b.need_x, b.need_attrs, b.need_radial, b.acc_sc, b.have_m, b.fuse_xw = 0, int(c["attrs"]), 0, c["acc"], 0, 1
    b.main = b.side = b.side2 = b.side3 = st
    b.x_cf, b.sh, b.x1, b.mid, b.conv, b.a_rep, b.m = (ar.p(k) for k in ("x", "sh", "x1", "mid", "conv", "a_rep", "m"))
    b.src = b.dst = b.dst_perm = b.src_perm = ar.p("edges")
    b.dst_ptr = b.src_ptr = ar.p("dst_ptr")
    b.perm, b.bounds, b.reps = ar.p("perm"), ar.p("bounds"), ar.p("reps")
    b.w_lin1, b.w_post, b.w_sc = ar.p("w_lin1"), ar.p("w_post"), ar.p("w_sc")
    b.rad.w = ar.p("w")
    b.gy, b.gb_sc = ar.p("gy"), ar.p("gb_sc")
    b.g_conv, b.g_mid, b.gm = ar.p("g_conv"), ar.p("g_mid"), ar.p("gm")
    if c["attrs"]:
        b.g_attrs, b.ga, b.kw_ws = ar.p("g_attrs"), ar.p("ga"), ar.p("kw_ws")
    assert lib.e3k_layer_bwd(handles[0], C.byref(b)) == E3K_OK
    ck = Check(ar, c)
    a_rep = attrs[reps]
    ck.exact("a_rep", a_rep)
    for name in ("conv", "x1", "y", "g_conv", "g_mid"):
        ck._claim(name)
        assert np.isfinite(ck.dev(name, np.float32)).all(), f"{name} is not finite"
    # gm: the keyed weight-gradient GEMM on a buffer the executor zero-filled, against float64 of the call's own operands (x and the
    # g_conv it wrote) with the bound of tests/test_gpu_wgrad_rider.py; where no problem writes, the fill's zero
    touched, want, bnd = _wgrad_set_reference(d.sc_wgrad, ar.host("x").astype(np.float64), ck.dev("g_conv", np.float32).astype(np.float64), N,
                                              K * ld, (perm, bounds, ld))
    assert touched.any() and (bnd[~touched] == 0).all() and (want[~touched] == 0).all()
    ck.close("gm", want, bnd, "layer_gm")
    ck._claim("mid")
    assert (ck.dev("mid", np.float32) == 0).all(), "the tensor product of a batch without edges is not zero"
    gm = ck.dev("gm", np.float32).reshape(K, ld)
    for k in c["empty"]:
        assert (gm[k] == 0).all(), "the gm row of a key without rows"
    kc = dict(c, V=V)
    inp = dict(a=a_rep, W=w_sc, gM=gm, old_ga=np.zeros((K, V), f32), old_gW=old_gw)
    ref = kw_reference(kc, inp, instr, acc=c["acc"])
    ck.close("m", *ref["M"], "layer_M")
    ck.close("gb_sc", *ref["g_W"], "layer_g_W")
    if c["attrs"]:
        ck.close("ga", *ref["g_a"], "layer_g_a")
        ga_dev = ck.dev("ga", np.float32).astype(np.float64).reshape(K, V)
        ck.equal("g_attrs", scatter_reference(ga_dev, reps, bounds, N, V))
        ck.free("kw_ws", ws_n)
    ck.finish()


def _narrow_handle(dev):
    from e3_layers_amd.backend import conv_native

    _, plans = model("d64")
    nl = conv_native.native_layer(plans[2]).narrow(((0, 64),))      # (the columns a 1x0e head reads: tests/test_gpu_half_live_backward.py)
    assert nl is not None and nl.form == "scalar" and nl.desc.w_live > 0
    return nl, nl.handle(dev)


def run_refuse(dev, c, L):
    """a small valid problem, one argument replaced: the return code, and the arena bit-identical"""
    from e3_layers_amd.backend import conv_native

    lib, st = L.load(), L.stream_ptr()
    o = dict(n=2, other_v=False, no_sc=False, ga="ga", g_attrs="g_attrs", reps="reps", bounds="bounds", gb_last=False, g_T_live="g_T_live")
    o.update(c["over"])
    K, N = c["K"], c["N"]
    ar = Arena(zlib.crc32(c["id"].encode()) ^ 0x1A7E)
    if c["fn"] in ("fwd", "bwd"):
        _, plans = model("d16")
        chosen = [plans[0], plans[1]]
        if o["other_v"]:
            chosen[1] = model("v1")[1][0]
        if o["no_sc"]:
            chosen[1] = model("d16")[0][1]._block_plan(addend=True)
            assert chosen[1] is not None and chosen[1].sc_spec is None
        hs = [conv_native.native_layer(p).handle(dev) for p in chosen]
        handles = (C.c_void_p * 9)(*[hs[i % 2] for i in range(9)])
        V = plans[0].sc_spec.v
        kc = dict(c, ends=False, empty=(1,))
        reps, bounds, _ = key_structure(kc)
        ar.alloc("attrs", N * V).alloc("reps", 2 * K, reps.view(np.int32)).alloc("bounds", 2 * K, bounds).alloc("a_rep", K * V)
        ar.alloc("ga", K * V).alloc("g_attrs", N * V).alloc("ws", 4 * K * V * 16)
        sizes = [(plans[i % 2].sc_spec, kw_instr(plans[i % 2])) for i in range(9)]
        for i in range(9):
            _, (_, n_w, total) = sizes[i]
            if i < 2:
                ar.alloc(f"W{i}", n_w).alloc(f"M{i}", K * total).alloc(f"gW{i}", n_w)
        ar.upload(dev)
        items = (L.KwStackItem * 9)()
        for i in range(9):
            items[i].w_sc, items[i].m, items[i].gb_sc = ar.p(f"W{i % 2}"), ar.p(f"M{i % 2}"), ar.p(f"gW{i % 2}")
        if c["fn"] == "fwd":
            rc = lib.e3k_kw_stack_fwd(handles, items, o["n"], ar.p("attrs"), ar.p("reps"), K, ar.p("a_rep"), st)
        else:
            rc = lib.e3k_kw_stack_bwd(handles, items, o["n"], ar.p("a_rep"), ar.p(o["reps"]), ar.p(o["bounds"]), N, K, ar.p(o["ga"]),
                                      ar.p(o["g_attrs"]), ar.p("ws"), st)
    else:
        nl, handle = _narrow_handle(dev)
        d, N, E, R = nl.desc, 3, 5, 9
        for name, size in (("conv", N * d.d_conv), ("gy", N * d.d_out), ("g_conv", N * d.d_conv), ("g_mid", N * d.d_mid), ("x", N * d.d_in),
                           ("x1", N * d.d_x1), ("mid", N * d.d_mid), ("y", N * d.d_out), ("g_x1", N * d.d_x1), ("g_xcf", N * d.d_in),
                           ("g_w", E * d.w_live), ("g_T", R * d.W), ("g_T_live", R * d.w_live), ("table_ws", 4096), ("gb_last", 64 * d.W),
                           ("T", R * d.W), ("P", 3 * R * d.W), ("small", 64)):
            ar.alloc(name, size)
        ar.upload(dev)
        if c["fn"] == "narrow_fwd":
            f = L.LayerFwdArgs()
            f.N, f.E, f.in_cf, f.out_cf = N, 0, 1, 1
            f.main = f.side = f.side2 = st
            f.x, f.sh, f.x1, f.mid, f.conv, f.y = (ar.p(k) for k in ("x", "small", "x1", "mid", "conv", "y"))
            f.rad.w = ar.p("small")
            rc = lib.e3k_layer_fwd(handle, C.byref(f))
        else:
            # the route a narrow layer exists on (fused packed-table walk, the rows from the radial stack), but for one argument
            b = L.LayerBwdArgs()
            b.N, b.E, b.in_cf, b.out_cf, b.fork, b.need_x, b.have_m, b.fuse_xw = N, E, 1, 1, 0, 1, 2, 1
            b.main = b.side = b.side2 = b.side3 = st
            b.x_cf, b.x1, b.mid, b.conv, b.gy = (ar.p(k) for k in ("x", "x1", "mid", "conv", "gy"))
            b.rad.R, b.rad.E, b.rad.use_table, b.rad.have_rows, b.rad.in_kernel, b.rad.packed = R, E, 1, 1, 1, 1
            b.rad.T, b.rad.P = ar.p("T"), ar.p("P")
            b.g_conv, b.g_mid, b.g_x1, b.g_xcf, b.g_w, b.g_T, b.table_ws = (ar.p(k) for k in ("g_conv", "g_mid", "g_x1", "g_xcf", "g_w", "g_T", "table_ws"))
            b.g_T_live = ar.p(o["g_T_live"])
            if o["gb_last"]:
                b.gb_last = ar.p("gb_last")
            rc = lib.e3k_layer_bwd(handle, C.byref(b))
    assert rc == c["rc"], (rc, c["rc"])
    Check(ar, c).finish()


RUNNERS = dict(kws=run_kws, layer=run_layer, refuse=run_refuse)


@pytest.mark.parametrize("c", CASES, ids=[c["id"] for c in CASES])
def test_layer_case(dev, c):
    from e3_layers_amd.backend import lib as L

    RUNNERS[c["kind"]](dev, c, L)


def test_zz_worst_ratio_per_family(dev):
    """prints what the cases of this run measured"""
    for family in sorted(WORST):
        print(f"worst error / bound, {family}: {WORST[family]:.3f}")
