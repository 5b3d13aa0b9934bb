"""The layer backward under every subset of wanted gradients (backend/conv_native.py: NativeConvBlockFn / RadialStackFn / KwStackFn
.backward and the needs_input_grad branches of backend/ops.py; csrc/e3k_layer.hip: e3k_layer_bwd, e3k_radial_stack_bwd,
e3k_kw_stack_bwd).

Set-up of tests/test_gpu_head_backward.py (its helpers are used): the 3-layer featureModel(n_dim=64, l_max=2) + addEnergyOutput on
synth_qm9(5, 3) (51 nodes, 742 edges), loss 1e3 * mse(total_energy, target), 512 knot intervals with the guard on (the table's
error, 4e-6, is below the gradient bound), keyed self-connection from the first row.

FORMS x stream modes x (autograd | gradient sink) are the parametrised cases; inside one case ONE model instance goes through every
freeze pattern of PATTERNS in turn (requires_grad_ set before the forward), so a memo that survives a pattern change is exposed.
Per (form, mode, sink, pattern):

1. a frozen parameter has grad None and is in no gradient sink;
2. every trainable parameter's gradient against the float64 oracle (one oracle backward per model serves every pattern: freezing
   changes which walk forms a sum, not the sum) with the rule of tests/test_gpu_head_backward.py::_against_oracle and GTOL of
   tests/test_gpu_model.py;
3. every buffer the backward takes uninitialised (conv_native._Carve.alloc, torch.empty / torch.empty_like called from conv_native
   and conv_block) is NaN for the duration of the backward: every returned gradient, every sink slice, every layer call's g_x and
   g_pre must be finite.  test_the_poison_bites shows that a descriptor that skips a needed write is caught by it;
4. the tensor-product walk and the weight-gradient launch of every layer call are the ones route_model() -- a pure-Python model of
   e3k_layer_bwd's decisions, fed with the arguments the call received -- predicts;
5. over all cases every branch of the model that Python can reach is predicted once or more (test_zz_every_reachable_branch_ran);
   UNREACHABLE names the others with the condition that excludes them, and tests/test_layer_inventory.py runs the model over
   a hand-written argument tuple for every branch, reachable or not.

What the tensor-product route record can show: the LAST tensor-product launch of the calling thread.  A layer call that runs a walk
and then the separate weight-gradient pass shows the latter; one that launches no tensor-product kernel leaves the record as it
was (asserted: unchanged).

Measured on an MI355X (a record, not a threshold; test_zz_every_reachable_branch_ran prints a run's own): worst parameter-gradient
error against float64 over all patterns and stream modes 1.8e-6 for bench, bench_own_kw, in_kernel, materialised and composed, 1.7e-6
for per_edge and per_edge_stack, 3.9e-6 for addend, 1.3e-6 for bench at l_max 3 (bound 5e-5); a frozen pattern's gradient is at
most 3.0e-7 from the all-trainable run's.  No defect was found by these cases.
"""
import collections
import contextlib

import pytest
import torch

from tests.test_gpu_head_backward import _against_oracle, _oracle_grads, _patch, _tree
from tests.test_gpu_model import GTOL
from tests.test_gpu_wgrad_rider import _ARG_PTRS, FUSED
from tests.util import record_measured, rel_err

pytestmark = pytest.mark.gpu

# ---------------------------------------------------------------------------------------------------------------------------------
# what the e3k_layer_bwd spy reads off the argument struct (the rider test's list, extended)
ARG_PTRS = _ARG_PTRS + tuple(k for k in ("x1", "gb_sc", "gb_last", "g_w", "g_T", "g_T_live", "table_ws") if k not in _ARG_PTRS)
ARG_INTS = ("N", "E", "n_keys", "need_x", "need_attrs", "need_radial", "have_m", "fuse_xw", "fork")
RAD_FIELDS = ("use_table", "in_kernel", "have_rows", "P", "w")
# the inputs of route_model (all truthy / falsy except E, have_m, w_live and narrow_form)
ROUTE_KEYS = ("need_x", "need_attrs", "need_radial", "gb_lin1", "gb_post", "gb_sc", "gb_last", "gb_hidden", "have_m", "gm", "g_w", "g_T",
              "g_T_live", "table_ws", "x1", "fuse_xw", "side_is_main", "side3_is_main", "use_table", "in_kernel", "P", "have_rows", "w", "E",
              "w_live", "narrow_form", "has_sc", "timed")

Route = collections.namedtuple("Route", "branch shows wst transpose fused_launch labels")

# branch = the walk of e3k_layer_bwd's eight-way chain (or none), ">bwd_w" behind it when the separate weight-gradient pass runs
BRANCHES = ("unsupported", "scalar", "masked", "xw_ptable", "xw_streamed", "x_ptable", "x_ptable>bwd_w", "x_table", "x_table>bwd_w",
            "x_stream", "x_stream>bwd_w", "bwd_w", "none")
# branches no Python caller reaches, and why (DESIGN.md section 4 repeats this)
UNREACHABLE = {
    "unsupported": "NativeConvBlockFn.backward picks the narrow layer under the executor's own condition and runs the dense one otherwise",
    "x_ptable>bwd_w": "fuse_xw is always 1 and g_w / x1 are always handed over with need_radial_side: the packed walk with a radial side is the fused one",
    "x_table": "every in-kernel layer gets a packed table (rad.P) from the stack or from its own forward: the unpacked table walk has no caller",
    "x_table>bwd_w": "as x_table",
}
OTHER_LABELS = ("bwd_w@side", "bwd_w@main", "transpose:rides+wgrad", "transpose:rides_alone", "transpose:own", "radial:last", "radial:hidden",
                "wgrads:early", "wgrads:late_lin1", "wgrads:one_call", "kw:own", "kw:gm", "attrs:scatter")
# (the executor's own radial branch with the transpose riding: ride needs have_rows when a radial gradient is wanted -- never both)
REACHABLE = {"branch:" + b for b in BRANCHES if b not in UNREACHABLE} | set(OTHER_LABELS)

VARIANTS = ("ride_without_side3", "fused_xw_without_radial_side", "wst_ignores_fused_xw", "need_x1_is_need_x")


def route_model(a, variant=None):
    """What e3k_layer_bwd (csrc/e3k_layer.hip) does with these arguments: the conditions in the executor's order and names.
    ``variant``: one of VARIANTS, a deliberately wrong model (tests/test_layer_inventory.py shows each disagrees somewhere)."""
    g = lambda k: bool(a[k])
    side_is_main, side3_is_main = g("side_is_main"), g("side3_is_main")
    need_last, need_hidden, need_radial = g("gb_last"), g("gb_hidden"), g("need_radial")
    need_radial_side = need_last or need_hidden or need_radial or (g("have_rows") and (g("g_w") or g("g_T")))
    need_post, need_lin1 = g("gb_post"), g("gb_lin1")
    want_sc = g("has_sc") and (g("gm") if a["have_m"] else (g("gb_sc") or g("need_attrs")))
    need_x1 = g("need_x") if variant == "need_x1_is_need_x" else (g("need_x") or need_lin1)
    in_kernel = g("use_table") and g("in_kernel")
    edges = a["E"] > 0
    fused_xw = (g("fuse_xw") and need_x1 and in_kernel and g("P") and edges and g("g_w") and g("x1")
                and (need_radial_side or variant == "fused_xw_without_radial_side"))
    narrow = a["w_live"] > 0
    if narrow and not (fused_xw and g("use_table") and g("have_rows") and g("g_T") and g("g_T_live") and g("table_ws")
                       and not need_last and not need_hidden and not need_radial):
        return Route("unsupported", None, None, None, False, frozenset({"branch:unsupported"}))
    fused_xw_s = (g("fuse_xw") and not fused_xw and need_x1 and not in_kernel and need_radial_side and edges and g("g_w") and g("x1")
                  and g("w") and side_is_main)
    ride = (fused_xw and g("use_table") and side_is_main and (side3_is_main or variant == "ride_without_side3") and not g("timed")
            and g("g_T") and g("table_ws") and (g("have_rows") or not (need_last or need_hidden or need_radial)))
    if not need_x1:
        walk = None
    elif narrow:
        walk = a["narrow_form"]
    elif fused_xw:
        walk = "xw_ptable"
    elif fused_xw_s:
        walk = "xw_streamed"
    elif in_kernel and g("P"):
        walk = "x_ptable"
    elif in_kernel:
        walk = "x_table"
    else:
        walk = "x_stream"
    radial = need_radial_side and edges
    bwd_w = radial and not fused_xw and not fused_xw_s
    wst = None
    if radial:
        wst = "side" if (not side_is_main and (not fused_xw or variant == "wst_ignores_fused_xw")) else "main"
    transpose = None
    if radial and g("use_table"):
        transpose = "rides" if ride else "own"
    fused_launch = ride and (need_post or need_lin1 or want_sc)
    branch = (walk or "") + (">bwd_w" if (walk and bwd_w) else ("bwd_w" if bwd_w else "")) or "none"
    labels = {"branch:" + branch}
    if bwd_w:
        labels.add("bwd_w@" + wst)
    if transpose == "rides":
        labels.add("transpose:rides+wgrad" if fused_launch else "transpose:rides_alone")
    elif transpose:
        labels.add("transpose:own")
    if radial and need_last and not g("have_rows"):
        labels.add("radial:last")
    if radial and (need_hidden or need_radial) and not g("have_rows"):
        labels.add("radial:hidden")
    if not side3_is_main:
        if need_post or want_sc:
            labels.add("wgrads:early")
        if need_lin1:
            labels.add("wgrads:late_lin1")
    elif need_post or need_lin1 or want_sc:
        labels.add("wgrads:one_call")
    if want_sc:
        labels.add("kw:gm" if a["have_m"] else "kw:own")
        if not a["have_m"] and g("need_attrs"):
            labels.add("attrs:scatter")
    return Route(branch, "bwd_w" if bwd_w else walk, wst, transpose, bool(fused_launch), frozenset(labels))


def shown_family(route):
    """the family of a tensor-product route record (e3k_tp_last_route), in route_model's names"""
    if route is None:
        return None
    if route.startswith("tp_bwd_xw_scalar_kernel"):
        return "scalar"
    if route.startswith("tp_bwd_xw_masked_kernel"):
        return "masked"
    if route.startswith("tp_bwd_w_kernel<false"):
        return "bwd_w"
    if route.startswith("tp_bwd_x_kernel<"):      # the last template argument is the mode (csrc/e3k_tp.hip: kBwdX...)
        return {"0": "x_stream", "1": "x_table", "4": "x_ptable", "5": "xw_ptable", "6": "xw_streamed"}.get(route[:-1].split(", ")[-1], route)
    return route


# ---------------------------------------------------------------------------------------------------------------------------------
# forms and freeze patterns
FORMS = {
    # table: radial_table.ENABLED; tp_table: conv_native.TP_TABLE; keyed: KEY_MIN_ROWS = 0; block: conv_block.ENABLED
    "bench": dict(table=1, tp_table=1, radial_stack=1, kw_stack=1, keyed=True, block=1),
    "bench_own_kw": dict(table=1, tp_table=1, radial_stack=1, kw_stack=0, keyed=True, block=1),
    "in_kernel": dict(table=1, tp_table=1, radial_stack=0, kw_stack=1, keyed=True, block=1),
    "materialised": dict(table=1, tp_table=0, radial_stack=0, kw_stack=1, keyed=True, block=1),
    "per_edge": dict(table=0, tp_table=1, radial_stack=0, kw_stack=1, keyed=True, block=1),
    "per_edge_stack": dict(table=0, tp_table=1, radial_stack=1, kw_stack=1, keyed=True, block=1),
    "addend": dict(table=1, tp_table=1, radial_stack=1, kw_stack=1, keyed=False, block=1),
    "composed": dict(table=1, tp_table=1, radial_stack=1, kw_stack=1, keyed=True, block=0),
}
_RADIAL = ".conv.fc."
_BESSEL = "radial_basis."
_HEAD = "output_linear."
PATTERNS = {      # name -> is this parameter trainable
    "all": lambda n: True,
    "radial_only": lambda n: _RADIAL in n or n.startswith(_BESSEL),
    "node_only": lambda n: not (_RADIAL in n or n.startswith(_BESSEL)),
    "last_layer_only": lambda n: n.startswith("layer2."),
    "first_layer_only": lambda n: n.startswith("layer0."),
    "head_only": lambda n: n.startswith(_HEAD),
    "sc_only": lambda n: ".conv.sc." in n,
    "sc_frozen": lambda n: ".conv.sc." not in n,
    "lin1_only": lambda n: ".conv.linear_1." in n,
    "post_only": lambda n: ".conv.tp.linear." in n,
    "radial_last_only": lambda n: n.endswith(".conv.fc.layer3.weight"),
    "radial_hidden1_only": lambda n: n.endswith(".conv.fc.layer1.weight"),
    "bessel_frozen": lambda n: not n.startswith(_BESSEL),
    "bessel_only": lambda n: n.startswith(_BESSEL),
    "middle_layer_frozen": lambda n: not n.startswith("layer1."),
}
# (form, forked, WGRAD_SIDE when forked, sink, l_max)
CASES = ([(f, fork, 1, False, 2) for f in FORMS for fork in (False, True)]
         + [("bench", True, 0, False, 2)]
         + [(f, fork, 1, True, 2) for f in ("bench", "in_kernel", "per_edge") for fork in (False, True)]
         + [("bench", fork, 1, False, 3) for fork in (False, True)])


def case_id(c):
    form, fork, wside, sink, l_max = c
    return "-".join([form, ("fork" if wside else "fork_wgrad_on_main") if fork else "one_stream", "sink" if sink else "autograd"]
                    + (["lmax3"] if l_max == 3 else []))


CASE_IDS = [case_id(c) for c in CASES]
SEEN, RAN, WORST = set(), set(), {}
_ORACLE = {}


# ---------------------------------------------------------------------------------------------------------------------------------
def _nan(t):
    if t.is_floating_point():
        t.fill_(float("nan"))
    return t


class _PoisonTorch:
    """stands in for the ``torch`` name of a module: empty / empty_like hand out NaN, everything else is torch's"""

    def __init__(self, real):
        self.__dict__["_real"] = real

    def __getattr__(self, name):
        return getattr(self._real, name)

    def empty(self, *args, **kwargs):
        return _nan(self._real.empty(*args, **kwargs))

    def empty_like(self, *args, **kwargs):
        return _nan(self._real.empty_like(*args, **kwargs))


@contextlib.contextmanager
def poisoned():
    from e3_layers_amd.backend import conv_block, conv_native

    real_alloc = conv_native._Carve.alloc
    proxy = _PoisonTorch(torch)

    def alloc(carve, device):
        return _nan(real_alloc(carve, device))

    conv_native._Carve.alloc = alloc
    conv_native.torch = conv_block.torch = proxy
    try:
        yield
    finally:
        conv_native._Carve.alloc = real_alloc
        conv_native.torch = conv_block.torch = torch


class LayerSpy:
    """Per e3k_layer_bwd call: route_model's inputs, read off the argument struct and the layer object, the tensor-product record
    before and after the call and the GEMM record after it; per NativeConvBlockFn.backward call: g_x and g_pre."""

    def __init__(self):
        from e3_layers_amd.backend import conv_native
        from e3_layers_amd.backend import lib as L

        self.cn, self.lib = conv_native, L.load()
        self.calls, self.outs = [], []
        self.real_bwd, self.real_layer_bwd = conv_native.NativeConvBlockFn.backward, self.lib.e3k_layer_bwd

    def _layer_of(self, handle):
        for top in self.cn._LAYERS:
            for lay in top._all():
                if handle in lay.handles.values():
                    return lay
        raise AssertionError("e3k_layer_bwd on a layer no NativeLayer owns")

    def _tp(self):
        r = self.lib.e3k_tp_last_route()
        return r.decode() if r else None

    def layer_bwd(self, layer, ref):
        a = ref._obj
        lay = self._layer_of(layer if isinstance(layer, int) else layer.value)
        d = lay.desc
        rec = {k: getattr(a, k) for k in ARG_PTRS}
        rec.update({k: int(getattr(a, k)) for k in ARG_INTS})
        rec.update({k: getattr(a.rad, k) for k in RAD_FIELDS})
        rec.update(gb_hidden=any(a.gb_hidden[i] for i in range(4)), side_is_main=not a.fork or a.side == a.main,
                   side3_is_main=not a.fork or a.side3 == a.main, w_live=int(d.w_live), narrow_form=getattr(lay, "form", None),
                   has_sc=d.sc_fwd.n > 0, timed=False,
                   one_round=all(gs.n_rounds <= 1 for gs in (d.post_wgrad, d.lin1_wgrad, d.sc_wgrad)))
        before = self._tp()
        rc = self.real_layer_bwd(layer, ref)
        rec.update(rc=rc, tp_before=before, tp_after=self._tp(), gemm_after=self.lib.e3k_gemm_last_routes().decode())
        self.calls.append(rec)
        return rc

    def block_bwd(self, ctx, *grads):
        out = self.real_bwd(ctx, *grads)
        self.outs.append((out[0], out[12]))
        return out

    @contextlib.contextmanager
    def installed(self):
        self.cn.NativeConvBlockFn.backward = staticmethod(self.block_bwd)
        self.lib.e3k_layer_bwd = self.layer_bwd
        try:
            yield self
        finally:
            self.cn.NativeConvBlockFn.backward = staticmethod(self.real_bwd)
            self.lib.e3k_layer_bwd = self.real_layer_bwd


def check_routes(label, calls):
    """assertion 4: every layer call took the walk and the weight-gradient launch the model predicts"""
    seen = set()
    for i, c in enumerate(calls):
        assert c["rc"] == 0, (label, i, c["rc"])
        want = route_model(c)
        got = shown_family(c["tp_after"])
        if want.shows is None:
            assert c["tp_after"] == c["tp_before"], f"{label} call {i}: a tensor-product launch where the model predicts none: {c['tp_after']}"
        else:
            assert got == want.shows, f"{label} call {i}: route {c['tp_after']} ({got}), the model predicts {want.shows} (branch {want.branch})"
        if c["one_round"]:      # (one e3k_gemm_multi call per set: the record after the layer call is the weight gradients')
            assert (FUSED in c["gemm_after"]) == want.fused_launch, \
                f"{label} call {i}: GEMM record {c['gemm_after']!r}, the model predicts fused launch = {want.fused_launch} (branch {want.branch})"
        seen |= want.labels
    return seen


def _setup(dev, monkeypatch, form, fork, wside, l_max):
    from e3_layers_amd.data.synthetic import synth_qm9
    from e3_layers_amd.utils import build

    tree = _tree(l_max)
    torch.manual_seed(0)
    model = build(tree).to(dev)
    batch = synth_qm9(5, 3)
    _apply_form(monkeypatch, model, form, fork, wside)
    key = (l_max,)
    if key not in _ORACLE:      # (the seed fixes the parameters: one float64 backward per model serves every case and pattern)
        target = batch["total_energy"]
        loss_of = lambda out: 1e3 * torch.nn.functional.mse_loss(out["total_energy"], target.to(out["total_energy"]))
        _ORACLE[key] = ({k: v.detach().clone() for k, v in model.state_dict().items()}, _oracle_grads(model, tree, batch, loss_of))
    state, ref = _ORACLE[key]
    for k, v in model.state_dict().items():
        assert torch.equal(v.cpu(), state[k].cpu()), f"{k}: the seeded build is not reproducible"
    return model, batch, ref


def _apply_form(monkeypatch, model, form, fork, wside):
    from e3_layers_amd.backend import conv_block, conv_native, ops, radial_table
    from e3_layers_amd.nn import message_passing as mp

    f = FORMS[form]
    sc = type(model.layer0.conv.sc)
    key_defaults = (sc.KEY_MIN_ROWS, sc.KEY_MIN_ROWS_PER_KEY)
    _patch(monkeypatch, model, knots=512)
    if not f["keyed"]:      # 51 nodes are below the keyed form's default threshold: the self-connection as the block's addend
        monkeypatch.setattr(sc, "KEY_MIN_ROWS", key_defaults[0])
        monkeypatch.setattr(sc, "KEY_MIN_ROWS_PER_KEY", key_defaults[1])
        assert key_defaults[0] > 51
    monkeypatch.setattr(conv_block, "ENABLED", f["block"])
    monkeypatch.setattr(conv_native, "ENABLED", 1)
    monkeypatch.setattr(conv_native, "TP_TABLE", f["tp_table"])
    monkeypatch.setattr(radial_table, "ENABLED", f["table"])
    monkeypatch.setattr(mp, "RADIAL_STACK", f["radial_stack"])
    monkeypatch.setattr(mp, "KW_STACK", f["kw_stack"])
    monkeypatch.setattr(mp, "STACK_MAX_EDGES", 10 ** 9)
    monkeypatch.setattr(mp, "KW_STACK_MAX_EDGES", 10 ** 9)
    monkeypatch.setattr(mp, "FWD_FORK", 1)
    monkeypatch.setattr(mp, "FORK_MIN_EDGES", 0 if fork else 10 ** 9)
    monkeypatch.setattr(mp, "FORK_MIN_EDGES_TABLE", 0 if fork else 10 ** 9)
    monkeypatch.setattr(ops, "WGRAD_SIDE", wside)


def freeze(model, pattern):
    trainable = PATTERNS[pattern]
    for name, p in model.named_parameters():
        p.requires_grad_(bool(trainable(name)))
        p.grad = None
    return [name for name, p in model.named_parameters() if p.requires_grad]


def run_pattern(model, batch, dev, pattern, sink, spy, poison=True):
    """one forward + backward under ``pattern``; returns {name: gradient} of the trainable parameters"""
    from e3_layers_amd.backend import ops
    from e3_layers_amd.run.parallel import FlatGradients, flat_param_order

    names = freeze(model, pattern)
    spy.calls.clear()
    spy.outs.clear()
    flat = None
    if sink:
        flat = FlatGradients(flat_param_order(model))
        flat.enable_direct_accumulation()
        flat.zero()
    try:
        target = batch["total_energy"].to(dev)
        out = model(batch.clone().to(dev))
        loss = 1e3 * torch.nn.functional.mse_loss(out["total_energy"], target)
        with spy.installed(), (poisoned() if poison else contextlib.nullcontext()):
            loss.backward()
            ops.join_side_streams()
            torch.cuda.synchronize()
        grads = {}
        for name, p in model.named_parameters():
            if p.requires_grad:
                assert p.grad is not None, (pattern, name)
                grads[name] = p.grad.detach().clone()
                assert bool(torch.isfinite(grads[name]).all()), f"{pattern}: {name} is not finite"
                if sink:
                    assert ops._sink_for(p) is not None
            else:
                assert p.grad is None, f"{pattern}: the frozen {name} received a gradient"
                assert ops._sink_for(p) is None, f"{pattern}: the frozen {name} is in the gradient sink"
        if sink:
            assert bool(torch.isfinite(flat.buffer).all()), f"{pattern}: the flat gradient is not finite"
        for i, (g_x, g_pre) in enumerate(spy.outs):
            for what, t in (("g_x", g_x), ("g_pre", g_pre)):
                assert t is None or bool(torch.isfinite(t).all()), f"{pattern}: {what} of layer call {i} is not finite"
        assert sorted(grads) == sorted(names)
        return grads
    finally:
        if flat is not None:
            flat.disable_direct_accumulation()
        for p in model.parameters():
            p.grad = None


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_every_freeze_pattern(dev, monkeypatch, case):
    form, fork, wside, sink, l_max = case
    label = case_id(case)
    model, batch, ref = _setup(dev, monkeypatch, form, fork, wside, l_max)
    spy = LayerSpy()
    base, worst, worst_vs_all = None, 0.0, 0.0
    try:
        for pattern in PATTERNS:
            grads = run_pattern(model, batch, dev, pattern, sink, spy)
            calls = list(spy.calls)
            if pattern == "all":
                base = grads
                assert len(grads) == len(ref)
            if pattern == "head_only":
                assert not spy.outs and not calls, "no layer backward may run when only the head is trainable"
            elif FORMS[form]["block"]:
                assert len(spy.outs) == len(calls) and 1 <= len(calls) <= 3, (pattern, len(spy.outs), len(calls))
                SEEN.update(check_routes(f"{label} {pattern}", calls))
            else:
                assert not calls
            _against_oracle(f"{label} {pattern}", grads, ref)
            worst = max([worst] + [rel_err(g, ref[k]) for k, g in grads.items() if float(ref[k].norm()) > 0])
            away = max([0.0] + [rel_err(g, base[k]) for k, g in grads.items() if float(base[k].norm()) > 0])
            worst_vs_all = max(worst_vs_all, away)
            print(f"{label} {pattern}: {len(grads)} trainable parameters, {len(calls)} layer calls "
                  f"{[route_model(c).branch for c in calls]}, worst distance from the all-trainable run {away:.3e} (printed, not asserted)")
    finally:
        freeze(model, "all")
    print(f"{label}: worst parameter-gradient rel err vs float64 over {len(PATTERNS)} patterns {worst:.3e} (bound {GTOL:.0e})")
    record_measured("test_gpu_needs_matrix", case=label, worst_rel_err=worst, worst_vs_all_trainable=worst_vs_all)
    WORST[label] = worst
    RAN.add(label)


@pytest.mark.parametrize("fork", [False, True], ids=["one_stream", "fork"])
def test_one_layer_stack_hands_back_its_only_input_gradient(dev, monkeypatch, fork):
    """RadialStackFn.backward returns g_rad[0] when ONE layer handed rows back and g_rad.sum(0) otherwise.  In the three-layer model
    every layer's rows require grad as soon as any radial input does, so all three are live in every pattern above; the single-layer
    branch is a one-layer model's: the Bessel frequencies' gradient of it against float64, alone and with everything trainable."""
    from e3_layers_amd.backend import conv_native
    from e3_layers_amd.configs.layer_configs import addEnergyOutput, featureModel
    from e3_layers_amd.data.synthetic import synth_qm9
    from e3_layers_amd.utils import build
    from tests.util import batch_to_oracle, oracle_like

    cfg = featureModel(n_dim=64, l_max=2, edge_spherical="1x0e+1x1o+1x2e", node_attrs="20x0e", edge_radial="8x0e", num_types=10,
                       num_layers=1, r_max=4.0)
    cfg.node_features = dict(cfg.layers)["layer0"]["output_features"][0]      # (the head reads what one layer produces: 0e + 1o + 2e)
    tree = addEnergyOutput(cfg, None)
    torch.manual_seed(0)
    model = build(tree).to(dev)
    batch = synth_qm9(5, 3)
    _apply_form(monkeypatch, model, "bench", fork, 1)
    orc = oracle_like(model, tree)
    data, attrs = batch_to_oracle(batch)
    out, _ = orc(data, attrs)
    (1e3 * torch.nn.functional.mse_loss(out["total_energy"], batch["total_energy"].to(out["total_energy"]))).backward()
    ref = {k[len("mods."):]: p.grad for k, p in orc.named_parameters()}
    spy = LayerSpy()
    try:
        for pattern in ("all", "bessel_only", "radial_only", "node_only"):
            n0 = conv_native.STACK_STATS[0]
            grads = run_pattern(model, batch, dev, pattern, False, spy)
            assert conv_native.STACK_STATS[0] == n0 + 1 and conv_native.STACK_STATS[1] == 1, "one stack evaluation of one layer"
            assert len(spy.calls) == 1
            check_routes(f"one layer {pattern}", spy.calls)
            _against_oracle(f"one layer, {'fork' if fork else 'one stream'}, {pattern}", grads, ref)
    finally:
        freeze(model, "all")


def test_the_poison_bites(dev, monkeypatch):
    """Every Linear of this model covers its input row (post_spec.in_covered, lin1_spec.in_covered and sc_spec.in_covered are True on
    all three layers, and on the l_max 3 and 16-channel models), so no zero fill can be switched off by a flag here.  The narrow
    layer has the same contract in another place -- post_in_covered = 1 because the masked walk reads only the columns of g_mid its
    pruned trailing Linear writes -- so the corrupted descriptor is a test-local copy of layer 1's masked form whose trailing Linear
    lost its last live instruction: the walk then reads one block of g_mid nobody wrote.  Indices and sizes are the real ones.  With
    the poison that block is NaN, and NaN arrives in the layer's input gradient."""
    import dataclasses

    from e3_layers_amd.backend import conv_native

    model, batch, _ = _setup(dev, monkeypatch, "bench", False, 1, 2)
    monkeypatch.setattr(conv_native, "LIVE_GRAD", 1)
    spy = LayerSpy()
    run_pattern(model, batch, dev, "all", False, spy)      # (builds the narrow forms; finite with the right descriptors)
    assert [route_model(c).branch for c in spy.calls] == ["scalar", "masked", "xw_ptable"]
    plan = model.layer1._block_plan()
    real = conv_native.native_layer(plan)
    (cols, good), = [(k, v) for k, v in real.narrows.items() if v is not None]
    assert good.form == "masked" and good.desc.post_in_covered == 1
    local = conv_native.NativeLayer(plan.replace(), narrow_of=real)
    live_sets = local.live_sets
    local.live_sets = lambda c: (lambda ls: dataclasses.replace(ls, post=ls.post[:-1]))(live_sets(c))
    bad = local.narrow(cols)
    assert bad is not None and bad.form == "masked" and bad.desc.w_live == good.desc.w_live
    assert bad.desc.post_dgrad.n < good.desc.post_dgrad.n
    real.narrows[cols] = bad
    try:
        freeze(model, "all")
        target = batch["total_energy"].to(dev)
        loss = 1e3 * torch.nn.functional.mse_loss(model(batch.clone().to(dev))["total_energy"], target)
        spy.calls.clear()
        spy.outs.clear()
        with spy.installed(), poisoned():
            loss.backward()
            torch.cuda.synchronize()
    finally:
        real.narrows[cols] = good
        for p in model.parameters():
            p.grad = None
    assert [route_model(c).branch for c in spy.calls] == ["scalar", "masked", "xw_ptable"]
    g_x = spy.outs[1][0]
    assert bool(torch.isnan(g_x).any()), "the unwritten block of g_mid did not reach the masked layer's input gradient"
    assert bool(torch.isfinite(spy.outs[0][0]).all()), "the layer above runs before the corrupted one"


@pytest.mark.parametrize("pattern", ["radial_only", "node_only"])
def test_frozen_parameters_keep_their_bits_through_an_optimiser_step(dev, monkeypatch, pattern):
    """assertion 1 on the bench form: FusedAdamEMA built over a partly frozen model takes the trainable parameters only; after one
    step every frozen parameter holds the bits it had and has no gradient, every trainable one with a gradient has moved"""
    from e3_layers_amd.backend import ops
    from e3_layers_amd.run.optim import FusedAdamEMA
    from e3_layers_amd.run.parallel import flat_param_order

    model, batch, ref = _setup(dev, monkeypatch, "bench", False, 1, 2)
    names = freeze(model, pattern)
    before = {k: p.detach().clone() for k, p in model.named_parameters()}
    opt = FusedAdamEMA(flat_param_order(model), lr=1e-3, ema_decay=0.99)
    assert len(opt.params) == len(names) < len(before)
    opt.grads.enable_direct_accumulation()
    try:
        target = batch["total_energy"].to(dev)
        loss = 1e3 * torch.nn.functional.mse_loss(model(batch.clone().to(dev))["total_energy"], target)
        opt.zero_grad()
        with poisoned():
            loss.backward()
        grads = {k: p.grad.detach().clone() for k, p in model.named_parameters() if p.requires_grad}
        opt.step()
        torch.cuda.synchronize()
        _against_oracle(f"optimiser {pattern}", grads, ref)
        for k, p in model.named_parameters():
            if k in names:
                assert ops._sink_for(p) is not None
                assert float(ref[k].norm()) == 0.0 or not torch.equal(p.detach(), before[k]), f"{k} did not move"
            else:
                assert p.grad is None and ops._sink_for(p) is None, k
                assert torch.equal(p.detach().view(torch.int32), before[k].view(torch.int32)), f"the frozen {k} changed"
    finally:
        opt.grads.disable_direct_accumulation()
        freeze(model, "all")


def test_bucketed_replay_of_a_partly_frozen_model_equals_eager(dev, monkeypatch):
    """tests/test_gpu_model.py::test_bucketed_graph_replay_with_fresh_padded_batches_equals_eager (its batches, its BucketedStep, its
    bounds) with the model in radial_only and then in node_only, and the optimiser inside the captured step: the replayed flat
    gradient against the eager one on the un-padded batch with the parameters the replay started from, and every frozen parameter
    bit-unchanged after the three replayed optimiser steps."""
    from e3_layers_amd.backend import ops, radial_table
    from e3_layers_amd.data.synthetic import synth_qm9
    from e3_layers_amd.run.graph_step import BucketedStep, bucket_capacity, pad_batch
    from e3_layers_amd.run.optim import FusedAdamEMA
    from e3_layers_amd.run.parallel import flat_param_order
    from e3_layers_amd.utils import build
    from tests.test_gpu_model import _energy_tree

    monkeypatch.setattr(radial_table, "KNOTS", 512)
    monkeypatch.setattr(radial_table, "GUARD_TOL", 1.0)
    monkeypatch.setattr(radial_table, "MIN_EDGES_PER_KNOT", 1)
    host = [synth_qm9(21, 24), synth_qm9(22, 24), synth_qm9(23, 24)]
    n_cap, e_cap = bucket_capacity([(b["pos"].shape[0], b["edge_index"].shape[1]) for b in host])
    padded = [pad_batch(b, n_cap, e_cap).to(dev) for b in host]
    for pattern in ("radial_only", "node_only"):
        torch.manual_seed(11)
        model = build(_energy_tree(2, 64, 3)).to(dev).train()
        names = freeze(model, pattern)
        frozen0 = {k: p.detach().clone() for k, p in model.named_parameters() if k not in names}
        assert frozen0 and names
        opt = FusedAdamEMA(flat_param_order(model), lr=1e-3, ema_decay=0.99)
        flat = opt.grads
        flat.enable_direct_accumulation()
        energies = []
        try:
            def train_on(batch):
                target = batch["total_energy"]
                out = model(batch)["total_energy"]
                energies.append(out)
                loss = 1e3 * (((out - target) ** 2) * batch["_graph_weight"]).sum()
                flat.zero()
                loss.backward()
                opt.step()
                return loss

            step = BucketedStep(train_on, padded[0], warmup=2)
            e_static = energies[-1]
            for p, b in zip((padded[1], padded[2], padded[0]), (host[1], host[2], host[0])):
                start = opt.flat.detach().clone()
                loss_g = step(p)
                ops.join_side_streams()
                torch.cuda.synchronize()
                loss_g, e_g, g_g, after = float(loss_g), e_static.detach().clone(), flat.gather().clone(), opt.flat.detach().clone()
                assert not torch.equal(after, start), "the replayed optimiser step moved nothing"
                with torch.no_grad():
                    opt.flat.copy_(start)      # the eager step on the parameters the replay started from
                db = b.clone().to(dev)
                target = db["total_energy"]            # (the model writes its prediction under the same key)
                out = model(db)["total_energy"]
                loss = 1e3 * torch.nn.functional.mse_loss(out, target)
                flat.zero()
                loss.backward()
                ops.join_side_streams()
                torch.cuda.synchronize()
                assert rel_err(e_g[:-1], out) < 1e-6
                assert bool(torch.isfinite(e_g).all())
                assert abs(loss_g - float(loss)) <= 1e-5 * abs(float(loss))
                err = rel_err(g_g, flat.gather())
                print(f"{pattern}: replayed flat gradient against the eager one {err:.3e} (bound 1e-05)")
                assert err < 1e-5
                with torch.no_grad():
                    opt.flat.copy_(after)
            for k, p in model.named_parameters():
                if k in frozen0:
                    assert p.grad is None, k
                    assert torch.equal(p.detach().view(torch.int32), frozen0[k].view(torch.int32)), f"{pattern}: the frozen {k} changed"
        finally:
            flat.disable_direct_accumulation()
            for p in model.parameters():
                p.grad = None


def test_zz_every_reachable_branch_ran(dev):
    """assertion 5, from the records of the cases above.  (With a selection of the cases: what ran must lie inside the model.)"""
    assert SEEN <= REACHABLE | {"branch:" + b for b in UNREACHABLE}, sorted(SEEN - REACHABLE)
    assert not (SEEN & {"branch:" + b for b in UNREACHABLE}), "a branch listed as unreachable from Python was reached: move it"
    for label in sorted(WORST):
        print(f"worst rel err vs float64, {label}: {WORST[label]:.3e}")
    if RAN >= set(CASE_IDS):
        assert SEEN == REACHABLE, f"never predicted: {sorted(REACHABLE - SEEN)}"
