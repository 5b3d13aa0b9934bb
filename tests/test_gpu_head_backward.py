"""The narrow backward of the last convolution layer in front of a scalar head (backend/conv_native.py: NativeLayer.narrow;
csrc/e3k_layer.hip; csrc/e3k_tp_scalar.hip) inside a model.

Set-up of tests/test_gpu_wgrad_rider.py's executor test: a 3-layer featureModel + addEnergyOutput on synth_qm9(5, 3) (51 nodes, 742
edges), 16 knot intervals so that this batch takes the packed-table path, keyed self-connection from the first row.

Which walk a layer's backward took is read from the library's route record (e3k_tp_last_route) right behind the layer's call.
Parameter gradients are compared with the float64 oracle at tests/test_gpu_model.py's bound for this model's parameter gradients
(GTOL = 5e-5, normwise per parameter), and a parameter whose oracle gradient is exactly zero must be exactly zero here.

Knot counts.  On 16 knot intervals the table is no stand-in for the radial MLP the oracle evaluates exactly (the rider test switches
the guard off for that reason): the DENSE backward is then 6.1e-2 away from float64 on embedding.linear.weight (l_max 2; 1.3e-2 at
l_max 3), the narrow one the same 6.1e-2 -- printed, and asserted to be more than 100 times the bound, by the first test.  So every
case runs twice: on 16 intervals -- routes, narrow against dense, the zeros -- and on 512 intervals, where the table's error (4e-6,
tests/test_gpu_model.py) is below the bound -- the same checks and float64.
"""
import numpy as np
import pytest
import torch

from tests.test_gpu_model import GTOL
from tests.test_gpu_wgrad_rider import _ARG_PTRS, _resolve, _wgrad_set_reference
from tests.util import batch_to_oracle, oracle_like, rel_err, to_cf

pytestmark = pytest.mark.gpu

SCALAR = "tp_bwd_xw_scalar_kernel"
# two fp32 runs of the same sums with the weight-gradient GEMMs' fp32 atomics in another order, normwise per parameter (the bound
# tests/test_gpu_model.py::test_bucketed_graph_replay_with_fresh_padded_batches_equals_eager holds the same comparison to, there over
# the whole flat gradient)
REPLAY_TOL = 1e-5


def _tree(l_max):
    from e3_layers_amd.configs.layer_configs import addEnergyOutput, featureModel

    return addEnergyOutput(featureModel(n_dim=64, l_max=l_max, edge_spherical="1x0e+1x1o+1x2e", node_attrs="20x0e", edge_radial="8x0e",
                                        num_types=10, num_layers=3, r_max=4.0), None)


def _patch(monkeypatch, model, knots=16):
    """knots = None: the default knot count and thresholds, at which this batch is below the table threshold"""
    from e3_layers_amd.backend import radial_table

    sc = type(model.layer0.conv.sc)
    monkeypatch.setattr(sc, "KEY_MIN_ROWS", 0)
    monkeypatch.setattr(sc, "KEY_MIN_ROWS_PER_KEY", 0)
    if knots is not None:
        monkeypatch.setattr(radial_table, "KNOTS", knots)
        monkeypatch.setattr(radial_table, "MIN_EDGES_PER_KNOT", 0)
        monkeypatch.setattr(radial_table, "GUARD_TOL", 1e9 if knots < 512 else 1.0)
        monkeypatch.setattr(radial_table, "GUARD_TOL_COL", 1e9 if knots < 512 else 1.0)


class _Spy:
    """Records, per NativeConvBlockFn.backward call (last layer first): the tensor-product route, g_x and g_T."""

    def __init__(self, monkeypatch):
        from e3_layers_amd.backend import conv_native
        from e3_layers_amd.backend import lib as L

        self.calls, lib, real = [], L.load(), conv_native.NativeConvBlockFn.backward

        def spy(ctx, *grads):
            out = real(ctx, *grads)
            route = lib.e3k_tp_last_route()
            self.calls.append(dict(route=route.decode() if route else None, g_x=None if out[0] is None else out[0].clone(),
                                   g_T=None if out[12] is None else out[12].clone()))
            return out

        monkeypatch.setattr(conv_native.NativeConvBlockFn, "backward", staticmethod(spy))


def _backward(model, batch, dev, loss_of, live, monkeypatch, spy):
    from e3_layers_amd.backend import conv_native, ops

    monkeypatch.setattr(conv_native, "LIVE_GRAD", 1 if live else 0)
    for p in model.parameters():
        p.grad = None
    spy.calls.clear()
    out = model(batch.clone().to(dev))
    loss_of(out).backward()
    ops.join_side_streams()
    torch.cuda.synchronize()
    return {k: p.grad.detach().clone() for k, p in model.named_parameters()}, list(spy.calls)


def _oracle_grads(model, tree, batch, loss_of, last_input=None):
    """float64 parameter gradients by name; ``last_input`` (a list): receives the gradient of the last layer's input features"""
    orc = oracle_like(model, tree)
    data, attrs = batch_to_oracle(batch)
    kept = []

    def keep(_mod, _inp, out):
        out[0]["output_features"].retain_grad()
        kept.append(out[0]["output_features"])

    h = orc.mods.layer1.register_forward_hook(keep)
    out, _ = orc(data, attrs)
    h.remove()
    loss_of(out).backward()
    if last_input is not None:
        last_input.append(kept[0].grad)
    return {k[len("mods."):]: p.grad for k, p in orc.named_parameters()}


def _against_oracle(label, grads, ref):
    worst = 0.0
    for name, g in grads.items():
        r = ref[name]
        if float(r.norm()) == 0.0:
            assert float(g.norm()) == 0.0, (label, name)
            continue
        err = rel_err(g, r)
        worst = max(worst, err)
        assert err < GTOL, (label, name, err)
    print(f"{label}: worst parameter-gradient rel err vs float64 {worst:.3e} (bound {GTOL:.0e})")
    assert worst > 0.0


def _dead_entries_are_zero(model, grads, narrow_layer):
    """the weight blocks of the last layer's instructions the derivation calls dead: exactly zero"""
    ls, plan = narrow_layer.live, model.layer2._block_plan()
    conv, checked = model.layer2.conv, 0
    for pname, instr, live, width in (
            ("layer2.conv.tp.linear.weight", plan.post_spec.instr, ls.post, lambda i: i.mul_in * i.mul_out),
            ("layer2.conv.linear_1.weight", plan.lin1_spec.instr, ls.lin1, lambda i: i.mul_in * i.mul_out),
            ("layer2.conv.sc.weight", plan.sc_spec.instr, [i for _, i in ls.sc], lambda i: i.mul_in * plan.sc_spec.v * i.mul_out)):
        g, live_ids = grads[pname].flatten(), {id(i) for i in live}
        for ins in instr:
            if id(ins) not in live_ids:
                assert bool((g[ins.w_off:ins.w_off + width(ins)] == 0).all()), (pname, ins.out_off)
                checked += width(ins)
    assert checked > 0 and conv is not None
    return checked


@pytest.mark.parametrize("knots", [16, 512])
@pytest.mark.parametrize("l_max", [2, 3])
def test_last_layer_takes_the_narrow_route_and_matches_dense_and_float64(dev, monkeypatch, l_max, knots):
    from e3_layers_amd.backend import conv_native
    from e3_layers_amd.data.synthetic import synth_qm9
    from e3_layers_amd.utils import build

    tree = _tree(l_max)
    torch.manual_seed(0)
    model = build(tree).to(dev)
    batch = synth_qm9(5, 3)
    target = batch["total_energy"]
    _patch(monkeypatch, model, knots)
    spy = _Spy(monkeypatch)
    loss_of = lambda out: 1e3 * torch.nn.functional.mse_loss(out["total_energy"], target.to(out["total_energy"]))
    g_live, c_live = _backward(model, batch, dev, loss_of, True, monkeypatch, spy)
    g_dense, c_dense = _backward(model, batch, dev, loss_of, False, monkeypatch, spy)
    print("routes, live:", [c["route"] for c in c_live], " dense:", [c["route"] for c in c_dense])
    assert len(c_live) == len(c_dense) == 3
    assert c_live[0]["route"] == SCALAR and all(c["route"] != SCALAR for c in c_live[1:] + c_dense)
    gx_ref = []
    ref = _oracle_grads(model, tree, batch, loss_of, gx_ref)
    if knots == 512:
        _against_oracle("narrow", g_live, ref)
        _against_oracle("dense", g_dense, ref)
        # the last layer's input gradient against float64 (its table gradient has no float64 counterpart -- the oracle has no table --
        # and is held to float64 through the radial MLP's parameter gradients above, which are formed from it)
        want = to_cf(gx_ref[0], model.layer2.conv.irreps_in["input_features"]) if model.layer1._emit_cf else gx_ref[0]
        for label, c in (("narrow", c_live[0]), ("dense", c_dense[0])):
            err = rel_err(c["g_x"], want)
            print(f"l_max {l_max}: last layer's g_x, {label} against float64: {err:.3e} (bound {GTOL:.0e})")
            assert err < GTOL, (label, err)
    else:
        # why float64 is not asked on 16 intervals: the DENSE backward -- the code as it was -- misses the bound there by orders of
        # magnitude (the table's interpolation error, not this change); the narrow one is the same distance away
        name = "embedding.linear.weight"
        e_dense, e_live = rel_err(g_dense[name], ref[name]), rel_err(g_live[name], ref[name])
        print(f"l_max {l_max}, 16 knot intervals, {name} against float64: dense {e_dense:.3e}, narrow {e_live:.3e} (bound {GTOL:.0e})")
        assert e_dense > 100 * GTOL, "the 16-interval table has become a stand-in for the MLP: compare with float64 here as well"
        assert abs(e_live - e_dense) < GTOL
    narrow = [n for n in conv_native.native_layer(model.layer2._block_plan()).narrows.values() if n is not None]
    assert len(narrow) == 1
    for grads in (g_live, g_dense):
        n_dead = _dead_entries_are_zero(model, grads, narrow[0])
    print(f"l_max {l_max}: {n_dead} structurally dead weight entries of the last layer, exactly zero in both runs")
    # the last layer's input gradient and table gradient: the narrow walk adds the live slots' terms in the dense walk's order and
    # the dense walk adds exact zeros for the others; the transpose sums the same columns in the same order
    a, b = c_live[0], c_dense[0]
    live_w = torch.zeros(a["g_T"].shape[1], dtype=torch.bool, device=dev)
    for off, mul in narrow[0].live.w:
        live_w[off:off + mul] = True
    assert torch.equal(a["g_T"][:, live_w].contiguous().view(torch.int32), b["g_T"][:, live_w].contiguous().view(torch.int32)), \
        "the live columns of the last layer's g_T differ from the dense run's bits"
    assert bool((a["g_T"][:, ~live_w] == 0).all()) and bool((b["g_T"][:, ~live_w] == 0).all()) and bool((a["g_T"][:, live_w] != 0).any())
    assert rel_err(a["g_x"], b["g_x"]) < 1e-6, rel_err(a["g_x"], b["g_x"])      # (the GEMMs' K-chains drop links: other roundings)
    for name in g_live:
        assert rel_err(g_live[name], g_dense[name]) < REPLAY_TOL or float(g_dense[name].norm()) == 0.0, name


@pytest.mark.parametrize("which,knots", [("second_consumer", 16), ("second_consumer", 512), ("hook", 16), ("hook", 512), ("inplace_write", 16),
                                         ("inplace_write", 512), ("below_table_threshold", None)])
def test_fallbacks_route_dense_and_match_float64(dev, monkeypatch, which, knots):
    from e3_layers_amd.data.synthetic import synth_qm9
    from e3_layers_amd.utils import build

    tree = _tree(2)
    torch.manual_seed(0)
    model = build(tree).to(dev)
    batch = synth_qm9(5, 3)
    target = batch["total_energy"]
    _patch(monkeypatch, model, knots)
    spy = _Spy(monkeypatch)
    energy = lambda out: 1e3 * torch.nn.functional.mse_loss(out["total_energy"], target.to(out["total_energy"]))
    loss_of, hooks = energy, []
    if which == "second_consumer":
        loss_of = lambda out: energy(out) + out["node_features"].square().sum()
    elif which in ("hook", "inplace_write"):
        # on the product only: the oracle applies the same scaling to node_features' gradient through its loss
        def loss_of(out):
            nf = out["node_features"]
            if nf.is_cuda:
                if which == "hook":
                    hooks.append(nf.register_hook(lambda g: g * 2.0))
                else:
                    hooks.append(nf.register_hook(lambda g: g.mul_(2.0)))
            return energy(out)
    g, calls = _backward(model, batch, dev, loss_of, True, monkeypatch, spy)
    print(which, "routes:", [c["route"] for c in calls])
    assert len(calls) == 3 and all(c["route"] != SCALAR for c in calls)
    assert all(c["route"].endswith("6>" if knots is None else "5>") for c in calls), "the table path, except below its threshold"
    if knots == 16:
        return
    if which in ("hook", "inplace_write"):
        # node_features' gradient doubled == the parameters below the head see twice the energy loss; the head's own do not
        ref1 = _oracle_grads(model, tree, batch, energy)
        ref = {k: (v if k.startswith(("output_linear", "reduce")) else 2.0 * v) for k, v in ref1.items()}
    else:
        ref = _oracle_grads(model, tree, batch, loss_of)
    _against_oracle(which, g, ref)


class _OperandSpy:
    """Per NativeConvBlockFn.backward call of an EAGER step: the executor's argument pointers, the route, and DETACHED aliases of every
    tensor the call used or returned (saved activations, scratch, outputs: the operands tests/test_gpu_wgrad_rider.py's executor
    test reads back).  Detached, because a retained tensor with autograd history keeps its step's graph alive, and with it the
    parameters' AccumulateGrad nodes, which a later backward then reuses on the stream they were made on: records of an eager step on
    the default stream that are still alive when a step is captured make the engine order the default stream behind an event
    recorded inside the capture (autograd's own warning: "may ... break CUDA graph capture if the AccumulateGrad node's stream is the
    default stream").  For the same reason install this spy behind the last capture of a test."""

    def __init__(self, monkeypatch):
        from e3_layers_amd.backend import conv_native
        from e3_layers_amd.backend import lib as L

        self.calls, self.scratch, self.args = [], [], []
        lib, real_bwd, real_alloc, real_layer_bwd = L.load(), conv_native.NativeConvBlockFn.backward, conv_native._Carve.alloc, L.load().e3k_layer_bwd

        def alloc(carve, device):
            t = real_alloc(carve, device)
            self.scratch.append(t)
            return t

        def layer_bwd(layer, ref):
            a = ref._obj
            self.args.append(dict({k: getattr(a, k) for k in _ARG_PTRS}, N=int(a.N), n_keys=int(a.n_keys), have_m=int(a.have_m)))
            return real_layer_bwd(layer, ref)

        def spy(ctx, *grads):
            self.scratch, n = [], len(self.args)
            out = real_bwd(ctx, *grads)
            assert len(self.args) == n + 1
            route = lib.e3k_tp_last_route()
            alias = lambda ts: [t.detach() for t in ts if isinstance(t, torch.Tensor)]
            self.calls.append(dict(self.args[-1], route=route.decode() if route else None, out=alias(out), saved=alias(ctx.saved_tensors),
                                   scratch=alias(self.scratch), plan=ctx.cfg[0], groups=ctx.cfg[2]))
            return out

        monkeypatch.setattr(conv_native.NativeConvBlockFn, "backward", staticmethod(spy))
        monkeypatch.setattr(conv_native._Carve, "alloc", alloc)
        monkeypatch.setattr(lib, "e3k_layer_bwd", layer_bwd)


def _check_layer_weight_gradients(c, extra, label):
    """Every weight gradient of one layer call (trailing Linear, linear_1, the keyed self-connection's gM) against float64 formed
    from the call's OWN fp32 operands, per element, with the bound of tests/test_gpu_wgrad_rider.py: (n + 8) u |alpha| |A|^T |G|.
    The problems are the DENSE layer's templates: a weight block the narrow form does not compute must hold the exact zero the
    dense sums give on these operands."""
    from e3_layers_amd.backend import conv_native

    desc, groups = conv_native.native_layer(c["plan"]).desc, c["groups"]
    pool = [t for t in c["saved"] + list(c["out"]) + c["scratch"] + [groups.perm, groups.bounds] + extra if isinstance(t, torch.Tensor)]
    f64 = lambda name: _resolve(c[name], pool, torch.float32).detach().cpu().numpy().astype(np.float64)
    assert c["have_m"] and c["gm"] and c["gb_post"] and c["gb_lin1"]
    keyed = (_resolve(c["perm"], pool, torch.int32).detach().cpu().numpy(),
             _resolve(c["bounds"], pool, torch.int32).detach().cpu().numpy()[:2 * c["n_keys"]], int(desc.ld_m))
    worst, checked = 0.0, 0
    for name, gs, a_key, g_key, b_key, kd in (("post", desc.post_wgrad, "mid", "g_conv", "gb_post", None),
                                              ("lin1", desc.lin1_wgrad, "x_cf", "g_x1", "gb_lin1", None),
                                              ("sc", desc.sc_wgrad, "x_cf", "g_conv", "gm", keyed)):
        got = f64(b_key)
        touched, want, bnd = _wgrad_set_reference(gs, f64(a_key), f64(g_key), c["N"], len(got), kd)
        err = np.abs(got - want)[touched]
        ok = np.isfinite(got[touched]) & (err <= bnd[touched])
        assert ok.all(), f"{label} {name}: {int((~ok).sum())} of {int(touched.sum())} weight-gradient elements outside the bound"
        worst = max(worst, float((err / np.maximum(bnd[touched], 1e-300)).max()))
        checked += int(touched.sum())
    print(f"{label}: {checked} weight-gradient elements, worst err / bound {worst:.3f}")
    return checked


def test_bucketed_replay_equals_the_eager_narrow_step(dev, monkeypatch):
    """BucketedStep capture and two replays on the padded batch against the eager narrow step on the same padded batch.

    * What no atomic touches -- every layer's input gradient g_x and table gradient g_T, copied inside the captured pass so that the
      copies hold each replay's values -- : the eager step's bits, after each replay.
    * The flat gradient, per parameter against the eager step: normwise REPLAY_TOL, and the same entries exactly zero (the narrow
      layer's dead slices among them).
    * The eager step's weight gradients that the GEMMs' fp32 atomics form (trailing Linear, linear_1, gM of every layer, the narrow
      last layer included): per element against float64 of the step's own operands, the rider test's bound.

    The per-element bound is applied to the eager step only.  It needs a step's operands; a replay's live in the graph's private pool,
    and reading them back means keeping every activation and scratch buffer of the captured pass alive, which takes the block reuse
    out of the captured step: a different graph from the one a user replays.  The replays are tied to the eager step instead by what
    no atomic touches (bit for bit) and per parameter; the eager step runs the same kernels on the same batch.  The eager step comes
    BEHIND the capture, and nothing with autograd history is kept from it (see _OperandSpy)."""
    from e3_layers_amd.backend import conv_native, ops
    from e3_layers_amd.data.synthetic import synth_qm9
    from e3_layers_amd.run.graph_step import BucketedStep, bucket_capacity, pad_batch
    from e3_layers_amd.run.parallel import FlatGradients, flat_param_order
    from e3_layers_amd.utils import build

    torch.manual_seed(0)
    model = build(_tree(2)).to(dev).train()
    _patch(monkeypatch, model)
    monkeypatch.setattr(conv_native, "LIVE_GRAD", 1)
    host = synth_qm9(5, 3)
    n_cap, e_cap = bucket_capacity([(host["pos"].shape[0], host["edge_index"].shape[1])])
    padded = pad_batch(host, n_cap, e_cap).to(dev)
    flat = FlatGradients(flat_param_order(model))
    flat.enable_direct_accumulation()
    names = {id(p): k for k, p in model.named_parameters()}
    spy = _Spy(monkeypatch)
    try:
        def train_on(batch):
            target = batch["total_energy"]           # (the model writes its prediction under the same key)
            out = model(batch)["total_energy"]
            loss = 1e3 * (((out - target) ** 2) * batch["_graph_weight"]).sum()
            flat.zero()
            loss.backward()
            return loss

        def finish():
            ops.join_side_streams()
            torch.cuda.synchronize()

        # ---- capture (two eager warm-up passes, then the captured one), two replays
        step = BucketedStep(train_on, padded, warmup=2)
        assert len(spy.calls) == 9 and [c["route"] == SCALAR for c in spy.calls] == 3 * [True, False, False], [c["route"] for c in spy.calls]
        captured = spy.calls[-3:]      # (their g_x / g_T are copies made INSIDE the graph: every replay refills them)
        replays = []
        for _ in range(2):
            loss = step(padded)
            finish()
            replays.append(dict(loss=float(loss), flat=flat.buffer.clone(), g_x=[None if c["g_x"] is None else c["g_x"].clone() for c in captured],
                                g_T=[c["g_T"].clone() for c in captured]))
        # ---- the eager narrow step on the same padded batch, its operands read back
        ospy = _OperandSpy(monkeypatch)
        spy.calls.clear()
        loss_e = train_on(padded.clone())
        finish()
        eager_calls, eager = spy.calls[-3:], flat.buffer.clone()
        assert float(loss_e) > 0 and float(eager.norm()) > 0 and all(float(c["g_T"].norm()) > 0 for c in eager_calls)
        assert [c["route"] == SCALAR for c in eager_calls] == [True, False, False], [c["route"] for c in eager_calls]
        for i, c in enumerate(ospy.calls[-3:]):
            assert _check_layer_weight_gradients(c, [flat.buffer], f"eager call {i}") > 0
        for r, rep in enumerate(replays):
            assert abs(rep["loss"] - float(loss_e)) <= 1e-6 * abs(float(loss_e))
            for i, c in enumerate(eager_calls):
                assert torch.equal(rep["g_T"][i].view(torch.int32), c["g_T"].view(torch.int32)), f"replay {r}: g_T of layer call {i}"
                assert (rep["g_x"][i] is None) == (c["g_x"] is None)
                if c["g_x"] is not None:
                    assert torch.equal(rep["g_x"][i].view(torch.int32), c["g_x"].view(torch.int32)), f"replay {r}: g_x of layer call {i}"
            got = rep["flat"]
            assert bool(((got == 0) == (eager == 0)).all()), f"replay {r}: an entry is zero in one of the two steps only"
            worst = 0.0
            for prm, off in zip(flat.params, flat.offsets):
                a, b = got[off:off + prm.numel()], eager[off:off + prm.numel()]
                if float(b.norm()) == 0.0:
                    continue
                err = rel_err(a, b)
                worst = max(worst, err)
                assert err < REPLAY_TOL, (r, names[id(prm)], err)
            print(f"replay {r} vs the eager narrow step: worst per-parameter rel err {worst:.3e} (bound {REPLAY_TOL:.0e}); g_x and g_T bit-identical")
    finally:
        flat.disable_direct_accumulation()
