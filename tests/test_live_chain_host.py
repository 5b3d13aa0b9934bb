"""The chain of narrow backwards below a scalar head (backend/conv_native.py: NativeLayer.live_sets / narrow, live_input_cols),
checked on the CPU without the kernels, on config_energy's 5-layer model at l_max 2 and 3.

* The last layer's narrow form is the scalar one; the mark it emits on its input gradient -- the union of the input blocks of its
  live linear_1 and self-connection instructions -- names columns (0, 64), (320, 512), (512, 832) of 1 152.
* Propagated through the layer below, that set leaves the live / total counts asserted here (l_max 2: 15 of 30 path slots, 960 of
  1 920 weight columns, 3 264 of 6 528 columns of mid, 51 of 102 gathered rows, 4 of 7 trailing-Linear, 5 of 6 linear_1 and 4 of 7
  self-connection instructions; the groups keep 3 / 0 / 2 / 4 / 4 / 2 slots).  At l_max 2 that layer gets the MASKED narrow form with
  the masks tests/test_gpu_tp_masked_matrix.py runs the kernel on; at l_max 3 (18 of 48 slots, 64 of 212 rows) its live groups reach
  l1 = 3, which the masked walk does not carry: it stays dense.
* The layer two below keeps 91 of 93 gathered rows (share 0.98 > 3/4): no narrow form.
* The structural claim, in the float64 oracle (the scheme of tests/test_live_columns_host.py): a g_y supported on those columns is
  backpropagated through the layer below the last; every mid, path-weight and x1 column and every weight block the derivation calls
  dead is EXACTLY zero, every live one is not -- and so is every column of the layer's input gradient outside the mark it would emit.
* A plan with an addend gets no narrow form.
"""
import pytest
import torch

from oracle import e3ref
from tests.test_gpu_tp_masked_matrix import DENSE_MASKS, SHIPPED_LMAX2
from tests.test_live_columns_host import _ranges_mask
from tests.util import to_cf

LAST_MARK = ((0, 64), (320, 512), (512, 832))
# layer below the last, per l_max: live / total of (slots, weight columns, mid columns, gathered rows, post, lin1, sc instructions)
COUNTS = {2: ((15, 30), (960, 1920), (3264, 6528), (51, 102), (4, 7), (5, 6), (4, 7)),
          3: ((18, 48), (1152, 3072), None, (64, 212), None, None, None)}
_MODELS = {}


def _model(l_max):
    if l_max not in _MODELS:
        from e3_layers_amd.configs import config_energy
        from e3_layers_amd.utils import build

        tree = config_energy.get_config(l_max=l_max).model_config
        torch.manual_seed(0)
        _MODELS[l_max] = (tree, build(tree))
    return _MODELS[l_max]


def _rows(groups, slots=None):
    from e3_layers_amd.nn.core import tp_slots

    if slots is None:
        slots = [(gi, q) for gi, g in enumerate(groups) for q in range(len(tp_slots(g.l1))) if (g.mask >> q) & 1]
    return sum(2 * tp_slots(groups[gi].l1)[q][1] + 1 for gi, q in slots)


@pytest.mark.parametrize("l_max", [2, 3])
def test_chain_numbers_and_forms(l_max):
    from e3_layers_amd.backend import conv_native

    _, model = _model(l_max)
    head = model.output_linear.linear.spec("e3nn", "e3nn")
    cols = tuple(sorted({(i.in_off, i.in_off + i.mul_in * i.dim) for i in head.instr}))
    assert cols == ((0, 64),)
    last = conv_native.native_layer(model.layer4._block_plan())
    n4 = last.narrow(cols)
    assert n4 is not None and n4.form == "scalar" and n4.desc.n_live == 3
    # the mark the narrow last layer emits == the union of its live input blocks
    ls4 = n4.live
    union = sorted({(i.in_off, i.in_off + i.mul_in * i.dim) for i in ls4.lin1} | {(i.in_off, i.in_off + i.mul_in * i.dim) for _, i in ls4.sc})
    mark = conv_native.live_input_cols(ls4)
    assert mark == tuple(union) == LAST_MARK
    assert (len(ls4.lin1), len(model.layer4._block_plan().lin1_spec.instr)) == (3, 6 if l_max == 2 else 8)
    assert len(ls4.sc) == 1
    assert model.layer4._block_plan().lin1_spec.d_in == (1152 if l_max == 2 else 2048)

    # ---- the layer below
    plan = model.layer3._block_plan()
    nl = conv_native.native_layer(plan)
    ls = nl.live_sets(mark)
    groups = plan.tp_plan.groups
    want = COUNTS[l_max]
    got = ((len(ls.slots), sum(bin(g.mask).count("1") for g in groups)), (sum(m for _, m in ls.w), plan.last_spec.d_out),
           (sum(b - a for a, b in ls.mid), plan.post_spec.d_in), (_rows(groups, ls.slots), _rows(groups)),
           (len(ls.post), len(plan.post_spec.instr)), (len(ls.lin1), len(plan.lin1_spec.instr)), (len(ls.sc), len(plan.sc_spec.instr)))
    print(f"l_max {l_max}, layer below the last: (live, total) slots / w / mid / rows / post / lin1 / sc = {got}")
    for g_, w_ in zip(got, want):
        assert w_ is None or g_ == w_, (got, want)
    n3 = nl.narrow(mark)
    if l_max == 2:
        assert tuple(g.mask for g in groups) == DENSE_MASKS and [g.l1 for g in groups] == [0, 0, 1, 1, 2, 2]
        per_group = [sum(1 << q for gj, q in ls.slots if gj == gi) for gi in range(len(groups))]
        assert tuple(per_group) == SHIPPED_LMAX2 and [bin(m).count("1") for m in per_group] == [3, 0, 2, 4, 4, 2]
        assert n3 is not None and n3.form == "masked" and n3.desc.w_live == 960 and n3.desc.n_live == 15
        live_groups = n3.plan.tp_plan.groups
        assert [(g.l1, g.mask, g.x_off) for g in live_groups] == [(g.l1, m, g.x_off) for g, m in zip(groups, SHIPPED_LMAX2) if m]
        # compact columns in (group, slot) order, the dense column of each in live_col
        pos = 0
        for i, (gi, q) in enumerate(ls.slots):
            lg = [g for g in live_groups if g.x_off == groups[gi].x_off][0]
            assert lg.w_off[q] == pos and n3.desc.live_col[i] == groups[gi].w_off[q] and n3.desc.live_len[i] == groups[gi].mul
            pos += groups[gi].mul
        assert pos == 960
        # pruned template sets: only the live problems
        assert (n3.desc.post_wgrad.n, n3.desc.lin1_wgrad.n, n3.desc.sc_wgrad.n) == (4, 5, 4)
        assert n3.desc.post_in_covered == 1
    else:
        assert n3 is None and any(groups[gi].l1 == 3 for gi, _ in ls.slots)

    # ---- the layer two below: nearly everything is live
    mark3 = conv_native.live_input_cols(ls)
    plan2 = model.layer2._block_plan()
    nl2 = conv_native.native_layer(plan2)
    ls2 = nl2.live_sets(mark3)
    share = _rows(plan2.tp_plan.groups, ls2.slots) / _rows(plan2.tp_plan.groups)
    print(f"l_max {l_max}, two below the last: live share of gathered rows {share:.3f}")
    assert share > conv_native.NARROW_MAX_SHARE and nl2.narrow(mark3) is None
    if l_max == 2:
        assert (len(ls2.slots), sum(bin(g.mask).count("1") for g in plan2.tp_plan.groups)) == (25, 27)
        assert (_rows(plan2.tp_plan.groups, ls2.slots), _rows(plan2.tp_plan.groups)) == (91, 93)


def test_a_plan_with_an_addend_gets_no_narrow_form():
    from e3_layers_amd.backend import conv_native

    _, model = _model(2)
    plan = model.layer3._block_plan(addend=True)
    assert plan is not None and plan.addend
    assert conv_native.native_layer(plan).narrow(LAST_MARK) is None


@pytest.mark.parametrize("l_max", [2, 3])
def test_dead_sets_of_the_layer_below_have_zero_gradient_and_live_sets_do_not(l_max):
    from e3_layers_amd.backend import conv_native

    tree, model = _model(l_max)
    mp = model.layer3
    plan = mp._block_plan()
    ls = conv_native.native_layer(plan).live_sets(LAST_MARK)
    mark = conv_native.live_input_cols(ls)

    orc = e3ref.build(tree)
    orc.load_state_dict({"mods." + k: v.detach() for k, v in model.state_dict().items()})
    layer = orc.mods.layer3.double()
    conv = layer.conv
    f_in = conv.irreps_in["input_features"]
    n, e = 23, 157
    g = torch.Generator().manual_seed(1)
    rnd = lambda *s: torch.randn(*s, dtype=torch.float64, generator=g)
    x_in = rnd(n, e3ref.irreps_dim(f_in)).requires_grad_(True)
    data = {"input_features": x_in, "node_attrs": rnd(n, 20), "edge_radial": rnd(e, 8),
            "edge_spherical": rnd(e, 9), "edge_index": torch.randint(0, n, (2, e), generator=g)}
    kept = {}

    def keep(name):
        def hook(_mod, _inp, out):
            out.retain_grad()
            kept[name] = out
        return hook

    hooks = [conv.tp.tp.register_forward_hook(keep("mid")), conv.fc.register_forward_hook(keep("w")),
             conv.linear_1.register_forward_hook(keep("x1"))]
    out, _ = layer(data, {"input_features": ("node", f_in)})
    y = out["output_features"]
    g_y = torch.zeros_like(y)
    live_y = _ranges_mask(LAST_MARK, y.shape[1])
    g_y[:, live_y] = rnd(n, int(live_y.sum()))
    y.backward(g_y)
    for h in hooks:
        h.remove()

    def columns(name, grad, ranges):
        live = _ranges_mask(ranges, grad.shape[1])
        mag = grad.abs().sum(0)
        assert bool((mag[~live] == 0).all()), f"{name}: {int((mag[~live] != 0).sum())} columns called dead carry a gradient"
        assert bool((mag[live] > 0).all()), f"{name}: {int((mag[live] == 0).sum())} columns called live carry none"
        return int(live.sum()), int((~live).sum())

    simp = mp.conv.tp.tp.irreps_mid_simplified      # (the product's layout of mid: merged channel-fastest blocks)
    n_mid = columns("mid", to_cf(kept["mid"].grad, simp), ls.mid)
    n_w = columns("path weights", kept["w"].grad, [(off, off + mul) for off, mul in ls.w])
    n_x1 = columns("x1", to_cf(kept["x1"].grad, f_in), ls.x1)
    # the mark the narrow layer would emit: block ranges are the same in both layouts of the row
    n_x = columns("layer input", x_in.grad, mark)
    print(f"l_max {l_max}: mid {n_mid}, path weights {n_w}, x1 {n_x1}, layer input {n_x} (live, dead) columns")
    assert n_w[0] == COUNTS[l_max][1][0] and n_w[0] + n_w[1] == COUNTS[l_max][1][1]
    if l_max == 2:
        assert n_mid == (3264, 3264) and n_w == (960, 960)

    def blocks(name, grad, all_instr, live_instr, width):
        live_ids = {id(i) for i in live_instr}
        for ins in all_instr:
            blk = grad[ins.w_off:ins.w_off + width(ins)]
            if id(ins) in live_ids:
                assert bool((blk != 0).any()), f"{name}: the weights of a live instruction (out {ins.out_off}) carry no gradient"
            else:
                assert bool((blk == 0).all()), f"{name}: the weights of a dead instruction (out {ins.out_off}) carry a gradient"
        return len(live_ids), len(all_instr) - len(live_ids)

    lin_w = lambda ins: ins.mul_in * ins.mul_out
    n_post = blocks("trailing Linear", conv.tp.linear.weight.grad.flatten(), plan.post_spec.instr, ls.post, lin_w)
    n_lin1 = blocks("linear_1", conv.linear_1.weight.grad.flatten(), plan.lin1_spec.instr, ls.lin1, lin_w)
    v = plan.sc_spec.v
    n_sc = blocks("self-connection", conv.sc.weight.grad.flatten(), plan.sc_spec.instr, [i for _, i in ls.sc], lambda ins: ins.mul_in * v * ins.mul_out)
    print(f"l_max {l_max}: instructions (live, dead): trailing Linear {n_post}, linear_1 {n_lin1}, self-connection {n_sc}")
    if l_max == 2:
        assert (n_post, n_lin1, n_sc) == ((4, 3), (5, 1), (4, 3))
