"""The structural claim behind the narrow backward (backend/conv_native.py: NativeLayer.live_sets), checked without the kernels.

The last convolution layer of an energy model is built in the float64 oracle, a random g_y supported on the head's live columns
(what an o3.Linear to 1x0e hands back: the 0e block) is backpropagated through it, and every quantity the derivation sorts into
live and dead is read off autograd:

* every column of the tensor product's output gradient, of the per-edge path-weight gradient and of the tensor product's input
  gradient that the derivation calls dead is EXACTLY zero, and every one it calls live is not;
* every weight block of a Linear or self-connection instruction it calls dead has gradient exactly zero, every live one has not.

Runs on the CPU: the product side contributes descriptors only (no device handle is made)."""
import pytest
import torch

from oracle import e3ref
from tests.util import to_cf


def _ranges_mask(ranges, width):
    m = torch.zeros(width, dtype=torch.bool)
    for a, b in ranges:
        m[a:b] = True
    return m


@pytest.mark.parametrize("l_max", [2, 3])
def test_dead_sets_have_zero_gradient_and_live_sets_do_not(l_max):
    from e3_layers_amd.backend import conv_native
    from e3_layers_amd.configs.layer_configs import addEnergyOutput, featureModel
    from e3_layers_amd.utils import build

    cfg = featureModel(n_dim=64, l_max=l_max, edge_spherical="1x0e+1x1o+1x2e", node_attrs="20x0e", edge_radial="8x0e", num_types=10,
                       num_layers=3, r_max=4.0)
    tree = addEnergyOutput(cfg, None)
    torch.manual_seed(0)
    model = build(tree)
    mp = model.layer2
    plan = mp._block_plan()
    assert plan is not None
    nl = conv_native.native_layer(plan)
    # the mark ops.StridedLinearFn.backward would put on the head's input gradient: the input blocks of its instructions
    head = model.output_linear.linear.spec("e3nn", "e3nn") if hasattr(model.output_linear, "linear") else None
    assert head is not None and not head.in_covered
    cols = tuple(sorted({(i.in_off, i.in_off + i.mul_in * i.dim) for i in head.instr}))
    assert cols == ((0, 64),)
    ls = nl.live_sets(cols)
    groups = plan.tp_plan.groups
    # the issue's numbers for l_max 2: three paths, 192 of the weight columns, 192 columns of mid
    assert len(ls.slots) == 3 and sum(m for _, m in ls.w) == 192 and sum(b - a for a, b in ls.mid) == 192
    assert sorted(groups[gi].l1 for gi, _ in ls.slots) == [0, 1, 2]
    narrow = nl.narrow(cols)
    assert narrow is not None and narrow.desc.w_live == 192 and narrow.desc.n_live == 3
    assert [narrow.desc.live_col[i] for i in range(3)] == [off for off, _ in ls.w]

    # ---- the same layer in float64
    orc = e3ref.build(tree)
    orc.load_state_dict({"mods." + k: v.detach() for k, v in model.state_dict().items()})
    layer = orc.mods.layer2.double()
    conv = layer.conv
    f_in = conv.irreps_in["input_features"]
    n, e = 23, 157
    g = torch.Generator().manual_seed(1)
    rnd = lambda *s: torch.randn(*s, dtype=torch.float64, generator=g)
    data = {"input_features": rnd(n, e3ref.irreps_dim(f_in)), "node_attrs": rnd(n, 20), "edge_radial": rnd(e, 8),
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
    live_y = _ranges_mask(cols, y.shape[1])
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
    print(f"l_max {l_max}: mid {n_mid}, path weights {n_w}, x1 {n_x1} (live, dead) columns")
    assert n_mid[0] == 192 and n_w[0] == 192

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
    assert n_post[1] > 0 and n_lin1[1] > 0 and n_sc[1] > 0
