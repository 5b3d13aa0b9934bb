"""e3k_wgrad_with_table_bwd (csrc/e3k_wgrad_rider.hip): the weight-gradient GEMM and the knot-table transpose in one launch.

Every buffer of a case -- the GEMM problems' arena of tests/test_gpu_gemm_matrix.py, the radii, the per-edge weights, the knot
lists, g_w, scale, the transpose's workspace and g_T -- sits in ONE float32 arena whose gaps are NaN.  The same start state goes
through the two separate calls (e3k_gemm_multi with wgrad = 1, then e3k_rtable_interp_bwd) and through the fused entry:

* g_T and the workspace of per-segment partial sums: the same bits (the per-segment sums and the combine order are the
  stand-alone kernels': csrc/e3k_rtable_bwd.h is one text for both);
* every weight gradient against float64 with the bound of tests/test_gpu_gemm_matrix.py (a sum of n row products formed by fp32 FMA
  chains and atomics in some order: (n + 8) u (|alpha| |A|^T |G| + |B_old|) per element);
* every word outside the weight gradients, the workspace and g_T: the bits it had.
"""
import numpy as np
import pytest
import torch

from tests.test_gpu_gemm_matrix import E3K_ERR_INVALID, E3K_ERR_UNSUPPORTED, E3K_OK, MAX_ROWS, _problem, materialise, pr, reference, seg

pytestmark = pytest.mark.gpu

FUSED = "gemm_wgrad2_with_table_bwd_kernel"
W2 = "gemm_wgrad2_kernel"
K_KNOTS = 16
H_INV = 4.0
PLAN_W = 1920      # path weights of layers 3 and 4 of the l_max 2, 64-channel plan bench.py trains (192 / 960 / 1 728 / 1 920 / 1 920): 7.5 chunks
# edges per knot: knots 2 .. 11 hold these; 0, 1 and 12 .. 16 none.  150 = three segments (64 + 64 + 22), 65 = 64 + 1
KNOT_COUNTS = {2: 0, 3: 1, 4: 3, 5: 4, 6: 7, 7: 8, 8: 12, 9: 64, 10: 65, 11: 150}

GEMM_FULL = [seg(pr(777, 5, 192, 128)), seg(pr(1000, 3, 64, 64)),
             seg(pr(0, 3, 64, 64), pr(0, 3, 128, 64), keys=dict(sizes=[0, 7, 64, 30, 101], spare=9))]
GEMM_ONE_TILE = [seg(pr(100, 1, 64, 64))]
GEMM_ONE_WORKGROUP = [seg(pr(40, 1, 64, 64))]                      # one tile, one split: one add per element, the same bits every run
GEMM_NOT_ELIGIBLE = [seg(pr(40, 1, 64, 64, g=False), pr(10, 3, 64, 1))]      # G not 16-byte-loadable; one output column (one workgroup each)


def _radii(rng, counts):
    r = np.concatenate([(i + rng.uniform(0.05, 0.95, n)) / H_INV for i, n in counts.items()] + [np.zeros(0)]).astype(np.float32)
    return r[rng.permutation(len(r))]


class Setup:
    """One arena on the device, binned, ready for either route.  Offsets in elements."""

    def __init__(self, dev, L, gemm_segs, counts, W, scale, accumulate, seed=0, name="rider"):
        self.L, self.lib, self.dev = L, L.load(), dev
        rng = np.random.default_rng(seed)
        self.case = dict(id=name, segs=gemm_segs, rc=E3K_OK, wgrad=True)
        ar, self.segs = materialise(self.case)
        xg = ar.rng.standard_normal(ar.n + 16).astype(np.float32)
        self.g_idx, self.g_want, self.g_bnd, _ = reference(self.segs, xg.astype(np.float64), True)
        r = _radii(rng, counts)
        self.E, self.K, self.W, self.acc = len(r), K_KNOTS, W, accumulate
        E, K = self.E, self.K
        self.n_ws = int(self.lib.e3k_rtable_bwd_workspace_floats(E, K, W))
        n_bws = int(self.lib.e3k_rtable_bins_workspace_ints(E, K))
        self.off, n = {}, 0
        for key, size in (("gemm", len(xg)), ("r", E), ("coef", 4 * E), ("bin", E), ("ptr", K + 2), ("seg", K + 2), ("perm", E),
                          ("bws", n_bws), ("gw", E * W), ("scale", E), ("ws", self.n_ws), ("gT", (K + 1) * W)):
            n = (n + 8 + 3) // 4 * 4      # a NaN gap in front of every block
            self.off[key] = n
            n += size
        self.size = dict(gemm=len(xg), ws=self.n_ws, gT=(K + 1) * W)
        x = np.full(n + 8, np.nan, np.float32)
        x[self.off["gemm"]:self.off["gemm"] + len(xg)] = xg
        x[self.off["r"]:self.off["r"] + E] = r
        x[self.off["gw"]:self.off["gw"] + E * W] = rng.standard_normal(E * W).astype(np.float32)
        x[self.off["scale"]:self.off["scale"] + E] = rng.uniform(0.5, 2.0, E).astype(np.float32)
        if accumulate:
            x[self.off["gT"]:self.off["gT"] + (K + 1) * W] = rng.standard_normal((K + 1) * W).astype(np.float32)
        self.use_scale = scale
        buf = torch.from_numpy(x).to(dev)
        p = lambda k: buf.data_ptr() + 4 * self.off[k]
        L.check(self.lib.e3k_rtable_bins(p("r"), E, H_INV, K, p("bin"), p("coef"), p("ptr"), p("seg"), p("perm"), p("bws"), L.stream_ptr()),
                "e3k_rtable_bins")
        torch.cuda.synchronize()
        self.start = buf
        self.keep = []
        self._keys = [None if s["keys"] is None else (torch.from_numpy(s["keys"]["perm"]).to(dev), torch.from_numpy(s["keys"]["groups"]).to(dev))
                      for s in self.segs]

    def segments(self, base):
        L, ms = self.L, []
        for s, kd in zip(self.segs, self._keys):
            arr = (L.GemmProblem * len(s["descs"]))(*[_problem(L, d, base + 4 * self.off["gemm"], False, False) for d in s["descs"]])
            g = L.GemmSegment()
            g.templates, g.n_templates = arr, len(s["descs"])
            g.a_base = g.a2_base = g.b_base = g.c_base = g.bias_base = None
            g.M1 = -1
            if kd is not None:
                g.n_keys, g.perm, g.groups_dev, g.b_key_stride = len(s["keys"]["groups"]) // 2, kd[0].data_ptr(), kd[1].data_ptr(), s["descs"][0]["ks"]
            else:
                g.n_keys, g.perm, g.groups_dev, g.b_key_stride = 0, None, None, 0
            self.keep.append(arr)
            ms.append(g)
        marr = (L.GemmSegment * max(len(ms), 1))(*ms)
        self.keep.append(marr)
        return marr, len(ms)

    def table_args(self, base, **over):
        p = lambda k: base + 4 * self.off[k]
        a = dict(gw=p("gw"), coef=p("coef"), scale=p("scale") if self.use_scale else None, ptr=p("ptr"), seg=p("seg"), perm=p("perm"),
                 E=self.E, K=self.K, W=self.W, ws=p("ws"), gT=p("gT"), acc=self.acc)
        a.update(over)
        return [a[k] for k in ("gw", "coef", "scale", "ptr", "seg", "perm", "E", "K", "W", "ws", "gT", "acc")]

    def separate(self):
        buf = self.start.clone()
        marr, n = self.segments(buf.data_ptr())
        st = self.L.stream_ptr()
        rc = self.lib.e3k_gemm_multi(marr, n, 1, st)
        route = self.lib.e3k_gemm_last_routes().decode()
        assert rc == E3K_OK
        assert self.lib.e3k_rtable_interp_bwd(*self.table_args(buf.data_ptr()), st) == E3K_OK
        torch.cuda.synchronize()
        return buf, route

    def fused(self, table_over=None, seg_edit=None):
        buf = self.start.clone()
        marr, n = self.segments(buf.data_ptr())
        if seg_edit is not None:
            marr, n = seg_edit(marr, n)
        rc = self.lib.e3k_wgrad_with_table_bwd(marr, n, *self.table_args(buf.data_ptr(), **(table_over or {})), self.L.stream_ptr())
        torch.cuda.synchronize()
        return buf, rc, self.lib.e3k_gemm_last_routes().decode()

    def region(self, buf, key):
        return buf[self.off[key]:self.off[key] + self.size[key]].view(torch.int32)

    def outputs_mask(self):
        m = np.zeros(self.start.numel(), bool)
        m[self.off["gemm"] + self.g_idx] = True
        for k in ("ws", "gT"):
            m[self.off[k]:self.off[k] + self.size[k]] = True
        return m

    def check_fused(self, got, ref):
        assert torch.equal(self.region(got, "gT"), self.region(ref, "gT")), "g_T differs from the separate calls'"
        assert torch.equal(self.region(got, "ws"), self.region(ref, "ws")), "per-segment partial sums differ"
        assert not torch.isnan(got[self.off["gT"]:self.off["gT"] + self.size["gT"]]).any(), "a table row was not written"
        g, s0 = got.cpu().numpy(), self.start.cpu().numpy()
        m = self.outputs_mask()
        same = g.view(np.int32)[~m] == s0.view(np.int32)[~m]
        assert same.all(), f"{int((~same).sum())} words outside the outputs changed, e.g. at {np.flatnonzero(~m)[~same][:5]}"
        for name, x in (("fused", g), ("separate", ref.cpu().numpy())):
            v = x[self.off["gemm"] + self.g_idx].astype(np.float64)
            err = np.abs(v - self.g_want)
            print(f"{name}: weight gradients max err / bound = {float((err / np.maximum(self.g_bnd, 1e-300)).max()):.3f} over {len(v)} elements")
            ok = np.isfinite(v) & (err <= self.g_bnd)
            assert ok.all(), f"{name}: {int((~ok).sum())} of {len(v)} weight-gradient elements outside the bound"


@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("scale", [False, True], ids=["noscale", "scale"])
@pytest.mark.parametrize("W", [64, 320, PLAN_W])
def test_entry_equals_the_two_calls(dev, W, scale, accumulate):
    """W = 64: one chunk with dead lanes; 320: a partly live second chunk; the plan's: several chunks."""
    from e3_layers_amd.backend import lib as L

    s = Setup(dev, L, GEMM_FULL, KNOT_COUNTS, W, scale, accumulate, seed=W + 2 * scale + accumulate)
    ref, route_sep = s.separate()
    assert route_sep == f"{W2}[4]"
    got, rc, route = s.fused()
    assert rc == E3K_OK and route == f"{FUSED}[4]", (rc, route)
    s.check_fused(got, ref)


@pytest.mark.parametrize("which", ["one_tile_gemm_150_edge_knot", "full_gemm_one_edge"])
def test_both_imbalances(dev, which):
    from e3_layers_amd.backend import lib as L

    if which == "one_tile_gemm_150_edge_knot":
        s = Setup(dev, L, GEMM_ONE_TILE, KNOT_COUNTS, PLAN_W, False, 0, seed=11)
        n = 1
    else:
        s = Setup(dev, L, GEMM_FULL, {6: 1}, 320, True, 1, seed=12)
        n = 4
    ref, _ = s.separate()
    got, rc, route = s.fused()
    assert rc == E3K_OK and route == f"{FUSED}[{n}]", (rc, route)
    s.check_fused(got, ref)


def test_repeatable(dev):
    from e3_layers_amd.backend import lib as L

    s = Setup(dev, L, GEMM_FULL, KNOT_COUNTS, PLAN_W, True, 1, seed=21)
    a, rc_a, _ = s.fused()
    b, rc_b, _ = s.fused()
    assert rc_a == E3K_OK and rc_b == E3K_OK
    assert torch.equal(s.region(a, "gT"), s.region(b, "gT")) and torch.equal(s.region(a, "ws"), s.region(b, "ws"))


@pytest.mark.parametrize("which", ["no_edges", "no_eligible_problem", "no_problem"])
def test_fallbacks_equal_the_two_calls_exactly(dev, which):
    """The GEMM problems here are summed by one workgroup per tile (one add per element): the separate calls give the same bits
    every run, and the entry -- which makes those two calls -- must give exactly them."""
    from e3_layers_amd.backend import lib as L

    if which == "no_edges":
        s = Setup(dev, L, GEMM_ONE_WORKGROUP, {}, 64, False, 1, seed=31)
        want_route = f"{W2}[1]"
    elif which == "no_eligible_problem":
        s = Setup(dev, L, GEMM_NOT_ELIGIBLE, KNOT_COUNTS, 320, True, 0, seed=32)
        want_route = "wgrad_n1_kernel;gemm_wgrad_kernel<false, 1>[1]"
    else:
        s = Setup(dev, L, [], KNOT_COUNTS, 64, False, 0, seed=33)
        want_route = ""
    ref, route_sep = s.separate()
    got, rc, route = s.fused()
    assert rc == E3K_OK and route == route_sep == want_route, (rc, route, route_sep)
    assert torch.equal(got.view(torch.int32), ref.view(torch.int32))


def _edit_problem(**fields):
    def edit(marr, n):
        p = marr[0].templates[0]
        for k, v in fields.items():
            setattr(p, k, v)
        return marr, n
    return edit


def _edit_segment(_seg=0, _problem=None, **fields):
    def edit(marr, n):
        for k, v in fields.items():
            setattr(marr[_seg], k, v)
        for k, v in (_problem or {}).items():
            setattr(marr[_seg].templates[0], k, v)
        return marr, n
    return edit


TABLE_REFUSALS = [
    ("E_negative", dict(E=-1), E3K_ERR_INVALID), ("K_below_4", dict(K=3), E3K_ERR_INVALID), ("W_zero", dict(W=0), E3K_ERR_INVALID),
    ("W_not_multiple_of_4", dict(W=322), E3K_ERR_UNSUPPORTED), ("E_past_int32", dict(E=2 ** 31 - 1), E3K_ERR_UNSUPPORTED),
    ("gT_null", dict(gT=None), E3K_ERR_INVALID), ("ptr_null", dict(ptr=None), E3K_ERR_INVALID), ("seg_null", dict(seg=None), E3K_ERR_INVALID),
    ("ws_null", dict(ws=None), E3K_ERR_INVALID), ("gw_null", dict(gw=None), E3K_ERR_INVALID), ("coef_null", dict(coef=None), E3K_ERR_INVALID),
    ("perm_null", dict(perm=None), E3K_ERR_INVALID),
]
GEMM_REFUSALS = [
    ("n_segments_negative", lambda m, n: (m, -1), E3K_ERR_INVALID),
    ("segments_null", lambda m, n: (None, n), E3K_ERR_INVALID),
    ("n_templates_negative", _edit_segment(n_templates=-1), E3K_ERR_INVALID),
    ("templates_null", _edit_segment(templates=None), E3K_ERR_INVALID),
    ("more_than_64_problems", _edit_segment(n_templates=65), E3K_ERR_INVALID),
    ("keyed_without_perm", _edit_segment(n_keys=3), E3K_ERR_INVALID),
    ("M2_zero", _edit_problem(M2=0), E3K_ERR_INVALID), ("N_zero", _edit_problem(N=0), E3K_ERR_INVALID),
    ("K_zero", _edit_problem(K=0), E3K_ERR_INVALID), ("M1_negative", _edit_problem(M1=-1), E3K_ERR_INVALID),
    ("rows_past_limit", _edit_problem(M1=MAX_ROWS // 5 + 1), E3K_ERR_UNSUPPORTED),
    ("A_null", _edit_problem(A=None), E3K_ERR_INVALID), ("B_null", _edit_problem(B=None), E3K_ERR_INVALID),
    ("G_null", _edit_problem(C=None), E3K_ERR_INVALID),
    ("V_past_limit", _edit_problem(V=33), E3K_ERR_UNSUPPORTED), ("V_without_A2", _edit_problem(V=4), E3K_ERR_INVALID),
    ("bias_on_a_weight_gradient", _edit_problem(bias=4096), E3K_ERR_INVALID),
    ("activation_on_a_weight_gradient", _edit_problem(act=1), E3K_ERR_INVALID),
    ("chain_on_a_weight_gradient", _edit_problem(chain=1), E3K_ERR_INVALID),
    ("K_not_a_multiple_of_V", _edit_problem(V=5, A2=4096), E3K_ERR_INVALID),
    ("activation_out_of_range", _edit_problem(act=2), E3K_ERR_INVALID), ("activation_negative", _edit_problem(act=-1), E3K_ERR_INVALID),
    ("chain_negative", _edit_problem(chain=-1), E3K_ERR_INVALID), ("chain_past_the_batch", _edit_problem(chain=20), E3K_ERR_INVALID),
    ("keyed_without_groups", _edit_segment(2, groups_dev=None), E3K_ERR_INVALID),
    ("keyed_without_its_perm", _edit_segment(2, perm=None), E3K_ERR_INVALID),
    ("segment_rows_past_int32", _edit_segment(M1=2 ** 31), E3K_ERR_INVALID),
    ("rebased_A2_without_base", _edit_segment(M1=777, _problem=dict(A2=9)), E3K_ERR_INVALID),
    ("rebased_bias_without_base", _edit_segment(M1=777, _problem=dict(bias=9)), E3K_ERR_INVALID),
]


@pytest.fixture(scope="module")
def refusal_setup(dev):
    from e3_layers_amd.backend import lib as L

    return Setup(dev, L, GEMM_FULL, KNOT_COUNTS, 320, True, 1, seed=41)


@pytest.mark.parametrize("name,over,want", TABLE_REFUSALS, ids=[r[0] for r in TABLE_REFUSALS])
def test_table_side_refusals_leave_everything_untouched(refusal_setup, name, over, want):
    s = refusal_setup
    _, before = s.separate()      # (a call that launched: the refusal has a record to clear)
    assert before != ""
    got, rc, route = s.fused(table_over=over)
    assert rc == want and route == "", (rc, route)
    assert torch.equal(got.view(torch.int32), s.start.view(torch.int32))


@pytest.mark.parametrize("name,edit,want", GEMM_REFUSALS, ids=[r[0] for r in GEMM_REFUSALS])
def test_gemm_side_refusals_leave_everything_untouched(refusal_setup, name, edit, want):
    s = refusal_setup
    _, before = s.separate()      # (a call that launched: the refusal has a record to clear)
    assert before != ""
    got, rc, route = s.fused(seg_edit=edit)
    assert rc == want and route == "", (rc, route)
    assert torch.equal(got.view(torch.int32), s.start.view(torch.int32))


# ---------------------------------------------------------------------------------------------------------------------------------
# the layer executor
U24 = 2.0 ** -24
_ARG_PTRS = ("x_cf", "mid", "g_conv", "g_x1", "gb_lin1", "gb_post", "gm", "perm", "bounds")


def _resolve(ptr, tensors, dtype):
    """The flat view, from the address `ptr` to its tensor's end, of the one tensor among `tensors` that holds it."""
    for t in tensors:
        beg = t.data_ptr()
        if t.dtype == dtype and t.is_contiguous() and beg <= ptr < beg + t.numel() * t.element_size():
            return t.view(-1)[(ptr - beg) // t.element_size():]
    raise AssertionError(f"no tensor holds {ptr:#x}")


def _wgrad_set_reference(gs, A, G, N, n_out, keyed=None):
    """Float64 values and the bound of test 1 for one template set of weight gradients (include/e3k.h, rebased templates: pointer
    fields are byte offsets, M1 is the segment's): B[k, n] += alpha sum_rows A[row, k] G[row, n], the rounds of a set accumulating;
    keyed: rows = the nodes of key t through perm, B of key t at + t * key_stride.  B starts at zero here, so the bound is
    (n + 8) u |alpha| (|A|^T |G|) with n the rows summed into the element.  Returns (touched mask, want, bound)."""
    want, mag, rows = np.zeros(n_out), np.zeros(n_out), np.zeros(n_out)
    for j in range(gs.n):
        p = gs.p[j]
        assert p.V == 0 and not p.bias and not p.act and not p.chain
        groups = [(0, np.arange(N))]
        if keyed is not None:
            perm, bounds, ks = keyed
            groups = [(t, perm[b0:b0 + min(cnt, N)]) for t, (b0, cnt) in enumerate(bounds.reshape(-1, 2)) if cnt > 0]
        k, n = np.arange(p.K), np.arange(p.N)
        for t, nd in groups:
            n1, r2 = np.repeat(nd, p.M2).astype(np.int64), np.tile(np.arange(p.M2), len(nd))
            Am = A[((p.A or 0) // 4 + n1 * p.a_r1 + r2 * p.a_r2)[:, None] + k[None, :] * p.a_k]
            Gm = G[((p.C or 0) // 4 + n1 * p.c_r1 + r2 * p.c_r2)[:, None] + n[None, :] * p.c_n]
            bidx = (p.B or 0) // 4 + (t * keyed[2] if keyed is not None else 0) + k[:, None] * p.b_k + n[None, :] * p.b_n
            assert len(np.unique(bidx)) == bidx.size
            want[bidx] += p.alpha * (Am.T @ Gm)
            mag[bidx] += abs(p.alpha) * (np.abs(Am).T @ np.abs(Gm))
            rows[bidx] += len(n1)
    return rows > 0, want, (rows + 8) * U24 * mag


def test_executor_takes_the_fused_launch_on_one_stream(dev, monkeypatch):
    """The convolution layers of the l_max 2 plan on 3 molecules (51 nodes, 742 edges; 16 knot intervals, so that a knot holds more
    than 64 edges), backward on one stream (the transpose rides with every layer's weight gradients), forked (separate launches on
    their streams) and on one stream while profiled for the transpose (separate launches, timed).  g_T and every layer's input
    gradient: the same bits every way.  Weight gradients (trailing Linear, keyed self-connection, linear_1 -- what the launch in
    question computes): every element of every route against float64 with the bound of test 1, per element.  The operands are the
    layer's own fp32 buffers of that run (x_cf, mid, g_conv, g_x1, read back after the backward) and the problems are the
    layer's own templates (NativeLayer.desc), evaluated in numpy as include/e3k.h states them."""
    from e3_layers_amd.backend import conv_native, ops, radial_table
    from e3_layers_amd.backend import lib as L
    from e3_layers_amd.configs.layer_configs import addEnergyOutput, featureModel
    from e3_layers_amd.data.synthetic import synth_qm9
    from e3_layers_amd.nn import message_passing as mp
    from e3_layers_amd.utils import build

    cfg = featureModel(n_dim=64, l_max=2, edge_spherical="1x0e+1x1o+1x2e", node_attrs="20x0e", edge_radial="8x0e", num_types=10,
                       num_layers=3, r_max=4.0)
    torch.manual_seed(0)
    model = build(addEnergyOutput(cfg, None)).to(dev)
    batch = synth_qm9(5, 3)
    target = batch["total_energy"].to(dev)
    # 16 knot intervals of 0.25 A so that this small batch takes the table path with more than one segment in a knot (the guard's
    # accuracy bound is not this test's subject: every route reads the same table)
    sc = type(model.layer0.conv.sc)      # (51 nodes: the keyed self-connection of the bench path, which starts at 256 nodes)
    monkeypatch.setattr(sc, "KEY_MIN_ROWS", 0)
    monkeypatch.setattr(sc, "KEY_MIN_ROWS_PER_KEY", 0)
    monkeypatch.setattr(radial_table, "KNOTS", 16)
    monkeypatch.setattr(radial_table, "MIN_EDGES_PER_KNOT", 0)
    monkeypatch.setattr(radial_table, "GUARD_TOL", 1e9)
    monkeypatch.setattr(radial_table, "GUARD_TOL_COL", 1e9)
    ei, pos = batch["edge_index"], batch["pos"]
    knot = ((pos[ei[0]] - pos[ei[1]]).norm(dim=1) * 4.0).floor().long().clamp(1, 14)
    assert int(torch.bincount(knot).max()) > 64, "no knot with more than one segment"
    lib = L.load()
    real_bwd = conv_native.NativeConvBlockFn.backward
    real_layer_bwd = lib.e3k_layer_bwd
    real_alloc = conv_native._Carve.alloc
    seen, scratch, calls = [], [], []

    def alloc_spy(self, device):
        t = real_alloc(self, device)
        scratch.append(t)
        return t

    def layer_bwd_spy(layer, ref):
        a = ref._obj
        calls.append(dict({k: getattr(a, k) for k in _ARG_PTRS}, N=int(a.N), n_keys=int(a.n_keys), have_m=int(a.have_m)))
        rc = real_layer_bwd(layer, ref)
        calls[-1]["route"] = lib.e3k_gemm_last_routes().decode()
        return rc

    def check_weight_gradients(ctx, out, c, label):
        """every weight gradient of this layer call against float64, per element"""
        plan, groups = ctx.cfg[0], ctx.cfg[2]
        desc = conv_native.native_layer(plan).desc
        pool = [t for t in list(ctx.saved_tensors) + list(out) + scratch + [groups.perm, groups.bounds] if isinstance(t, torch.Tensor)]
        f64 = lambda name: _resolve(c[name], pool, torch.float32).cpu().numpy().astype(np.float64)
        N = c["N"]
        sets = [("post", desc.post_wgrad, "mid", "g_conv", "gb_post", None), ("lin1", desc.lin1_wgrad, "x_cf", "g_x1", "gb_lin1", None)]
        assert c["have_m"] and c["gm"], "the keyed self-connection's weights come from the stack in the bench path"
        keyed = (_resolve(c["perm"], pool, torch.int32).cpu().numpy(), _resolve(c["bounds"], pool, torch.int32).cpu().numpy()[:2 * c["n_keys"]],
                 int(desc.ld_m))
        sets.append(("sc", desc.sc_wgrad, "x_cf", "g_conv", "gm", keyed))
        checked = 0
        for name, gs, a_key, g_key, b_key, kd in sets:
            if not c[b_key]:
                continue
            assert gs.n_rounds == 1, "one e3k_gemm_multi call per set: the route record of the layer call is that call's"
            got = f64(b_key)
            touched, want, bnd = _wgrad_set_reference(gs, f64(a_key), f64(g_key), N, len(got), kd)
            err = np.abs(got - want)[touched]
            print(f"{label} {name}: {int(touched.sum())} elements, max err / bound {float((err / np.maximum(bnd[touched], 1e-300)).max()):.3f}")
            ok = np.isfinite(got[touched]) & (err <= bnd[touched])
            assert ok.all(), f"{label} {name}: {int((~ok).sum())} of {int(touched.sum())} weight-gradient elements outside the bound"
            checked += int(touched.sum())
        assert checked > 0
        return checked

    def spy(ctx, *grads):
        n_calls = len(calls)
        scratch.clear()
        out = real_bwd(ctx, *grads)
        assert len(calls) == n_calls + 1
        ops.join_side_streams()
        torch.cuda.synchronize()
        c = calls[-1]
        table = ctx.cfg[7] is not None
        seen.append(dict(route=c["route"], g_x=None if out[0] is None else out[0].clone(), g_T=None if out[12] is None else out[12].clone(),
                         table=table, checked=check_weight_gradients(ctx, out, c, f"{label[0]} call {len(seen)}")))
        return out

    label = [""]

    def run(name, fork, profiled=False):
        label[0] = name
        monkeypatch.setattr(mp, "FORK_MIN_EDGES", 0 if fork else 10 ** 9)
        monkeypatch.setattr(mp, "FORK_MIN_EDGES_TABLE", 0 if fork else 10 ** 9)
        for lay in conv_native._LAYERS:
            lay.profile(4 if profiled else 0, ["rtable_bwd"] if profiled else None)
        for p in model.parameters():
            p.grad = None
        seen.clear()
        out = model(batch.clone().to(dev))
        loss = 1e3 * torch.nn.functional.mse_loss(out["total_energy"], target)
        monkeypatch.setattr(conv_native.NativeConvBlockFn, "backward", staticmethod(spy))
        monkeypatch.setattr(conv_native._Carve, "alloc", alloc_spy)
        monkeypatch.setattr(lib, "e3k_layer_bwd", layer_bwd_spy)
        try:
            loss.backward()
        finally:
            monkeypatch.setattr(conv_native.NativeConvBlockFn, "backward", staticmethod(real_bwd))
            monkeypatch.setattr(conv_native._Carve, "alloc", real_alloc)
            monkeypatch.setattr(lib, "e3k_layer_bwd", real_layer_bwd)
        ops.join_side_streams()
        torch.cuda.synchronize()
        timed = sum(len(lay.profile_read("rtable_bwd")) for lay in conv_native._LAYERS) if profiled else 0
        return list(seen), timed

    one, _ = run("one stream", False)
    fork, _ = run("forked", True)
    prof, timed = run("profiled", False, profiled=True)
    for lay in conv_native._LAYERS:
        lay.profile(0)
    assert len(one) == len(fork) == len(prof) == 3
    print("routes, one stream:", [s["route"] for s in one])
    print("routes, forked:    ", [s["route"] for s in fork])
    print("routes, profiled:  ", [s["route"] for s in prof], "timed transposes:", timed)
    for i in range(3):      # every layer is on the table, hands g_T to the radial stack, and rides on one stream only
        assert one[i]["table"] and one[i]["g_T"] is not None, i
        assert one[i]["route"].startswith(FUSED + "["), (i, one[i]["route"])
        for other in (fork, prof):
            assert FUSED not in other[i]["route"] and W2 in other[i]["route"], (i, other[i]["route"])
            assert torch.equal(one[i]["g_T"].view(torch.int32), other[i]["g_T"].view(torch.int32)), f"g_T of layer call {i}"
            assert (one[i]["g_x"] is None) == (other[i]["g_x"] is None)
            if one[i]["g_x"] is not None:
                assert torch.equal(one[i]["g_x"].view(torch.int32), other[i]["g_x"].view(torch.int32)), f"input gradient of layer call {i}"
            assert one[i]["checked"] == other[i]["checked"]
    assert any(s["g_x"] is not None for s in one)
    assert timed == 3
