"""The float kernels of the training path that no element-wise test reached, every one against float64 on the CPU, element by element,
at the C ABI: the fused hidden chain of the radial MLP (csrc/e3k_mlp.hip, all ten kernels), the squared-error loss and the fused
clip + Adam + EMA step with its device state block (csrc/e3k_optim.hip, all seven), and the forward-mode tangent of the radial MLP per
knot with its float64 reverse sweep (csrc/e3k_slope.hip, all three).

``CASES`` is a plain table in the form of tests/test_gpu_node_matrix.py: each case makes C-ABI calls through backend/lib.py on buffers
inside a NaN-filled arena with slack round every buffer, claims every word a call may write with exactly one comparison (``Check.free``
for scratch whose contents are not ABI) and requires every other word of the arena to keep its bits.  tests/test_train_inventory.py
holds the table to the kernels the three gfx950 code objects ship and to the functions include/e3k.h declares, shows on the CPU that
models of the kernels stay inside the bounds below and that planted mutants do not.  The input, reference and bound builders below run
without a GPU.

Radial MLP.  The references and bounds are those of tests/test_gpu_node_passes.py, unchanged (its activation models extended to the
identity, ssp and abs): z and out from float64 with K + 3 roundings per layer, the backward FROM the fp32 pre-activations the forward
left, weight gradients with R + 4 roundings of sum |h| |gz| -- and, where g_weights is handed over non-zero, the old value as one more
term of the same order-independent sum: (R + 5) u |old|.  The shapes are MLP_NEW, each at one 16-row-tile and one 64-row-tile size
chosen from the dispatch rule (64-row tiles once ceil(E / 64) * nets >= 256; the persistent backward runs 768 / nets workgroups):
    8 nets x 1984 rows   16-row tiles, 124 tiles on 96 workgroups         8 nets x 6145 rows   64-row tiles, 97 on 96
    1 net x 16320 rows   16-row tiles, 1020 on 768                        1 net: 1, 15, 16, 17, 63, 65 rows
A call with 9 or 16 nets is two launches.  At 1984 rows a launch of 8 nets has 31 * 8 = 248 < 256 tiles and runs 16-row tiles like
the launch behind it, so the 9-net case uses 2049 rows: 33 * 8 tiles of 64 rows for the first eight nets, 16-row tiles for the ninth.
Exact cases (integer x, W, g in [-3, 3], identity and abs, power-of-two alphas, cst = 1: every partial sum is a small dyadic number)
are compared with ==.  z, out and g_x of two identical calls agree bit for bit; the weight gradients meet in atomics and need not.

Optimiser.  ``EV`` of the node matrix replays the kernels' operations: u |a op b| per operation, the square sum of the gradient and
the loss in any order (gamma_n), rsqrtf within 2 ulp (the OpenCL requirement for single precision; no HIP math accuracy table is shipped
with the ROCm install).  Every case takes three consecutive steps and checks, after each, p, m, v and ema per
element and the 16 words of the state block: [0] steps, [6] skip flag, [8] EMA updates exact; [1], [2] within one ulp of
float32(1 - beta^t) (the device takes pow in double); [9] the effective EMA decay, [7] the gradient norm, [4] the clip coefficient by
their bounds; [5] zero again; [3] and [10..15] keep the bits they were given.  The per-element replay takes the state words the
device left (they have just been checked), so its bound is that of the update alone.  A skipped step (NaN in the last tail element,
+-inf in the body, finite gradients whose square sum overflows) leaves p, m, v with their bits, moves the EMA, does not advance [0]
and sets [6]; the step behind it has t and the EMA count apart.  ``adam_tick_pair`` pins tick_both_kernel against tick_kernel +
ema_tick_kernel: the same inputs without a norm and with a max_grad_norm that never clips leave every word equal but [7].

Slope.  Both sides compute in float64, the device then rounds once to fp32 (hp) or casts float64 partial sums (gradients).  The
reference is explicit float64 numpy: the basis b, b', db/dw, db'/dw from autograd of the definition the edge kernels are tested against
(tests/test_gpu_edge_matrix.py rad_derivatives), the chain and its reverse sweep written out layer by layer; tests/test_train_inventory.py
checks that sweep against torch float64 autograd of <g_hp, H'>.  Bounds:
    hp           u |ref| + 2^-126 + F64;  a row with r >= r_max is +-0.0 exactly (bound 0)
    g_hidden[l]  at most eight float64 partial sums S_r over the row ranges per = ceil(ceil(R / 8) / 16) * 16, each cast to fp32 and
                 added onto the old value with atomics: u sum |S_r| + gamma_(parts + 1) (|old| + sum |S_r|) + F64, order-independent
    g_bessel[f]  one float64 sum over all nets and rows, cast once, added once: u |S| + u |old + S| + F64
F64 is a running bound (class D64, unit roundoff 2^-53 on either side) on what two float64 evaluations of the same formulas differ by,
with 16 ulp allowed to each of the device's double exp, log1p, tanh, sin, cos, pow -- the loosest requirement OpenCL puts on any of
them (pow); no HIP math accuracy table is shipped with the ROCm install.  It exists for cancelling elements: sin(w r) / r and its slope at the first knot
(1e-6 h), the end of the cutoff, 1 - tanh^2 and 1 - sigmoid in saturation.  Condition, checked on the CPU for every case: F64 is below
1 % of the fp32 term on at least 99 % of the elements of hp.  It decided three things about the cases: random radii stay below
0.8 r_max but for planted rows (r_max, its fp32 predecessor, 1.5 r_max); the cases on the table's own knots use the symmetric cutoff
-- under the polynomial cutoff (p = 6: 1 - 28 x^6 + 48 x^7 - 21 x^8) every row within about 7 % of r_max has F64 above that 1 %, one
knot row in twelve; slope_R129_polynomial_knots runs that cutoff on the knots from 1e-6 h to 0.89 r_max, so what is NOT held element
by element is the polynomial cutoff on knot rows between 0.89 r_max and r_max; and the four-layer cases
draw weights of mean 0.5, whose sums cancel less.  The scratch is handed over NaN-filled (write-before-read) and claimed as free.
e3k_slope_tangent_fwd / _bwd cast R to int: R >= 2^31 - 1 is now E3K_ERR_UNSUPPORTED (csrc/e3k_slope.hip), as e3k_edge_records does;
that is the only change to the library.

Worst error / bound per family on an MI355X (a record, not a threshold; printed by test_zz_worst_ratio_per_family): see MEASURED
below -- 0.995 .. 1.000 for Adam's four streams and the slope's hp (a single rounding against its own bound), 0.83 for the
squared-error gradient and g_bessel, 0.43 and below for the MLP's order-independent sums.
"""
import ctypes as C
import zlib

import numpy as np
import pytest
import torch

from tests.test_gpu_node_matrix import EV, FL, U, Arena, Check as _Check, fma, gamma, sum_ev
from tests.test_gpu_node_passes import _mlp_backward_ref, _mlp_forward_ref
from tests.util import record_measured

pytestmark = pytest.mark.gpu

# worst error / bound per family as printed by a full run on an MI355X (profiles/train_matrix_measured.jsonl holds it per case)
MEASURED = {
    "adam_ema": 0.995, "adam_m": 0.998, "adam_p": 0.999, "adam_state4": 0.003, "adam_state7": 0.273,
    "adam_state9": 0.208, "adam_v": 1.000, "mlp_g_w": 0.113, "mlp_g_x": 0.059, "mlp_out": 0.234,
    "mlp_z": 0.431, "slope_g_bessel": 0.832, "slope_g_hidden": 0.525, "slope_hp": 0.998, "sq_error_grad": 0.832,
    "sq_error_loss": 0.147,
}

E3K_OK, E3K_ERR_INVALID, E3K_ERR_UNSUPPORTED = 0, -1, -3
f32, f64 = np.float32, np.float64
FLT_MAX = float(np.finfo(np.float32).max)
ULP_RSQRT = 2      # rsqrtf: the OpenCL single-precision requirement


def _rng(c, tag=""):
    return np.random.default_rng(zlib.crc32((c["id"] + tag).encode()))


def _f(v):
    return float(f32(v))


# ---------------------------------------------------------------------------------------------------------------------------------
# the table's vocabulary
MLP_NEW = [(8, 64, 1, 1), (16, 64, 4, 4), (64, 32, 2, 2), (48, 64, 2, 0), (7, 64, 3, 5), (1, 32, 1, 2), (33, 64, 2, 1), (63, 32, 4, 2)]
MLP_MAXNETS, MLP_FILL, MLP_MAXBLOCKS = 8, 256, 768


def mlp_tile(rows, nets):
    """the dispatch rule of csrc/e3k_mlp.hip for one launch"""
    return 16 if -(-rows // 64) * nets < MLP_FILL else 64


def mlp_launches(rows, nets):
    return [(n, mlp_tile(rows, n)) for n in (min(MLP_MAXNETS, nets - b) for b in range(0, nets, MLP_MAXNETS))]


def mlp(id_, why, shape, rows, nets=1, op="both", z="all", gw="all", gx=True, prefill=False, exact=False, repeat=False, multi=None):
    k0, h, nl, a = shape
    multi = nets > 1 if multi is None else multi
    assert z == "all" or op == "fwd"
    kernels, funcs = set(), {"e3k_mlp_tile_rows"}
    for n, tile in mlp_launches(rows, nets):
        kernels.add("mlp_hidden_fwd16_kernel" if tile == 16 else "mlp_hidden_fwd_kernel")
        if op == "both":
            kernels.add(f"mlp_hidden_bwd16_kernel<{nl}>" if tile == 16 else f"mlp_hidden_bwd_kernel<{nl}>")
    funcs.add("e3k_mlp_hidden_fwd_multi" if multi else "e3k_mlp_hidden_fwd")
    if op == "both":
        funcs.add("e3k_mlp_hidden_bwd_multi" if multi else "e3k_mlp_hidden_bwd")
    return dict(kind="mlp", id=id_, why=why, k0=k0, h=h, nl=nl, act=a, rows=rows, nets=nets, op=op, z=z, gw=gw, gx=gx, prefill=prefill,
                exact=exact, repeat=repeat, multi=multi, kernels=tuple(sorted(kernels)), funcs=tuple(sorted(funcs)))


def sq(id_, why, n, w_group=None, scale=0.37):
    return dict(kind="sq", id=id_, why=why, n=n, w_group=w_group, scale=scale, kernels=("sq_error_kernel",), funcs=("e3k_sq_error",))


def adam_kernels(ema, max_norm, skip):
    have_norm = max_norm > 0 or skip
    k = ["adam_ema_kernel<true>" if ema else "adam_ema_kernel<false>"]
    k += ["sumsq_kernel"] if have_norm else []
    k += ["tick_both_kernel"] if ema and not have_norm else ["tick_kernel"] + (["ema_tick_kernel"] if ema else [])
    return tuple(sorted(k))


def adam(id_, why, n, ema=True, max_norm=0.0, skip=0, wd=0.0, use_num=1, steps=("ok", "ok", "ok"), decay=0.999, v0=False):
    return dict(kind="adam", id=id_, why=why, n=n, ema=ema, max_norm=max_norm, skip=skip, wd=wd, use_num=use_num, steps=steps, decay=decay, v0=v0,
                kernels=adam_kernels(ema, max_norm, skip), funcs=("e3k_adam_ema_step",))


def adam_pair(id_, why, n):
    return dict(kind="adam_pair", id=id_, why=why, n=n, ema=True, skip=0, wd=0.01, use_num=1, decay=0.999, steps=("ok", "ok", "ok"),
                kernels=tuple(sorted(set(adam_kernels(True, 0.0, 0)) | set(adam_kernels(True, 1.0, 0)))), funcs=("e3k_adam_ema_step",))


def refuse(id_, why, fn, rc, **over):
    return dict(kind="refuse", id=id_, why=why, fn=fn, rc=rc, over=over, kernels=(), funcs=(fn,))


def slope(id_, why, R, H, k0, nh, a, nets=1, cut=0, oor=1, r_min=0.0, p=6.0, r_max=4.0, radii="random", sat=False, op="both", null_gh=(),
          gb=True, prefill=True, wbias=0.0, seed=0):
    kernels = ("slope_tangent_kernel<false>",) + (() if op == "fwd" else ("slope_tangent_kernel<true>", "slope_wgrad_kernel"))
    funcs = ("e3k_slope_tangent_fwd",) + (() if op == "fwd" else ("e3k_slope_tangent_bwd", "e3k_slope_tangent_bwd_scratch"))
    return dict(kind="slope", id=id_, why=why, R=R, H=H, k0=k0, nh=nh, act=a, nets=nets, cut=cut, oor=oor, r_min=r_min, p=p, r_max=r_max, radii=radii,
                sat=sat, op=op, null_gh=tuple(null_gh), gb=gb, prefill=prefill, wbias=wbias, seed=seed, kernels=kernels, funcs=funcs)


S, A, B, D = MLP_NEW, (1984, 8), (6145, 8), (16320, 1)
CASES = []
# ---- radial MLP: every new shape at one 16-row-tile and one 64-row-tile size
for _i, _s in enumerate(MLP_NEW):
    _r16 = (A, D)[_i % 2]
    _tag = "k{}_h{}_l{}_a{}".format(*_s)
    CASES.append(mlp(f"mlp_{_tag}_t16", f"16-row tiles, {_r16[1]} net(s) x {_r16[0]} rows: more tiles than persistent workgroups", _s, *_r16))
    CASES.append(mlp(f"mlp_{_tag}_t64", "64-row tiles, 8 nets x 6145 rows: 97 tiles on 96 workgroups, the last tile one row", _s, *B))
CASES += [
    mlp(f"mlp_rows{r}", f"{r} row(s): the edges of one and two tiles", MLP_NEW[(i + 3) % 8], r) for i, r in enumerate((1, 15, 16, 17, 63, 65))
] + [
    mlp("mlp_z_null", "forward without pre-activations (inference): z == NULL", S[6], 65, op="fwd", z="none"),
    mlp("mlp_z1_null", "one z[l] NULL in the forward: the others are still written", S[4], 17, op="fwd", z=1),
    mlp("mlp_z_null_t64", "z == NULL through the 64-row kernel", S[2], 6145, 8, op="fwd", z="none"),
    mlp("mlp_gw_null", "g_weights == NULL: only g_x", S[6], 65, gw="none"),
    mlp("mlp_gw1_null", "g_weights[1] NULL: the other layer's gradient still arrives", S[3], 65, gw=1),
    mlp("mlp_gw0_null_t64", "g_weights[0] NULL per net in the multi entry, 64-row tiles", S[2], 6145, 8, gw=0),
    mlp("mlp_gx_null", "g_x == NULL: layer 0 skips its dgrad, the weight gradients are complete", S[6], 65, gx=False),
    mlp("mlp_gx_null_t64", "g_x == NULL, 64-row tiles", S[7], 6145, 8, gx=False),
    mlp("mlp_gw_accumulate", "g_weights handed over non-zero: ADDED to, the old value one more term", S[6], 65, prefill=True),
    mlp("mlp_gw_accumulate_t64", "accumulation through the 64-row kernel's atomics", S[3], 6145, 8, prefill=True),
    mlp("mlp_nets9", "9 nets: two launches, 64-row tiles for eight nets and 16-row tiles for the ninth", S[6], 2049, 9),
    mlp("mlp_nets16", "16 nets at 1984 rows: two launches of eight", S[1], 1984, 16),
    mlp("mlp_multi_one_net", "the multi entry with a single net", S[0], 63, 1, multi=True),
    mlp("mlp_exact_identity_t16", "integers, identity: == catches any indexing error", (33, 64, 2, 0), 1984, 8, exact=True),
    mlp("mlp_exact_abs_t64", "integers, abs (sign(0) = 0 in the backward), 64-row tiles", (7, 32, 2, 5), 6145, 8, exact=True),
    mlp("mlp_exact_k64_rows65", "integers, k0 = 64 > h = 32: the second k block of layer 0", (64, 32, 2, 0), 65, exact=True),
    mlp("mlp_repeat_t16", "two identical calls: z, out, g_x bit for bit", S[6], 1984, 8, repeat=True),
    mlp("mlp_repeat_t64", "two identical calls, 64-row tiles", S[1], 6145, 8, repeat=True),
    refuse("mlp_refuse_k0_0", "k0 = 0", "e3k_mlp_hidden_fwd", E3K_ERR_UNSUPPORTED, k0=0),
    refuse("mlp_refuse_k0_65", "k0 = 65", "e3k_mlp_hidden_bwd", E3K_ERR_UNSUPPORTED, k0=65),
    refuse("mlp_refuse_h48", "h = 48", "e3k_mlp_hidden_fwd", E3K_ERR_UNSUPPORTED, h=48),
    refuse("mlp_refuse_layers0", "no layer", "e3k_mlp_hidden_fwd_multi", E3K_ERR_UNSUPPORTED, nl=0),
    refuse("mlp_refuse_layers5", "five layers", "e3k_mlp_hidden_bwd_multi", E3K_ERR_UNSUPPORTED, nl=5),
    refuse("mlp_refuse_act6", "activation 6", "e3k_mlp_hidden_fwd", E3K_ERR_INVALID, act=6),
    refuse("mlp_refuse_nets0_fwd", "n_nets = 0", "e3k_mlp_hidden_fwd_multi", E3K_ERR_INVALID, nets=0),
    refuse("mlp_refuse_nets0_bwd", "n_nets = 0", "e3k_mlp_hidden_bwd_multi", E3K_ERR_INVALID, nets=0),
    refuse("mlp_refuse_tile_rows_9", "e3k_mlp_tile_rows describes ONE launch: at most 8 nets", "e3k_mlp_tile_rows", E3K_ERR_INVALID, nets=9),
    refuse("mlp_refuse_w1_null", "weights[1] NULL", "e3k_mlp_hidden_fwd", E3K_ERR_INVALID, null="w1"),
    refuse("mlp_refuse_w1_null_multi", "weights[1] NULL in a net of the multi entry", "e3k_mlp_hidden_bwd_multi", E3K_ERR_INVALID, null="w1"),
    refuse("mlp_refuse_out_null", "out NULL", "e3k_mlp_hidden_fwd", E3K_ERR_INVALID, null="out"),
    refuse("mlp_refuse_out_null_multi", "out NULL", "e3k_mlp_hidden_fwd_multi", E3K_ERR_INVALID, null="out"),
    refuse("mlp_refuse_bwd_z_null", "the backward needs the pre-activations", "e3k_mlp_hidden_bwd", E3K_ERR_INVALID, null="z"),
    refuse("mlp_refuse_bwd_z1_null", "... every one of them", "e3k_mlp_hidden_bwd_multi", E3K_ERR_INVALID, null="z1"),
    refuse("mlp_refuse_rows_negative", "E < 0", "e3k_mlp_hidden_fwd", E3K_ERR_UNSUPPORTED, rows=-1),
    refuse("mlp_rows0_fwd", "E = 0: OK, nothing launched, nothing written", "e3k_mlp_hidden_fwd", E3K_OK, rows=0),
    refuse("mlp_rows0_bwd_multi", "E = 0: OK, nothing written", "e3k_mlp_hidden_bwd_multi", E3K_OK, rows=0),
]
# ---- optimiser
CASES += [sq(f"sq_n{n}", f"{n} entries, the mean (weight NULL)", n) for n in (1, 63, 64, 65, 1023, 1024, 1025, 5000)] + [
    sq("sq_weight_group1", "one weight per entry", 1025, w_group=1),
    sq("sq_weight_group3", "one weight per three entries (force components)", 5000 // 3 * 3, w_group=3),
    sq("sq_weight_group3_n65", "a group straddles the 64-lane boundary", 66, w_group=3),
    sq("sq_weight_group_n", "a single weight for all entries", 1023, w_group=1023),
    refuse("sq_refuse_n0", "n = 0", "e3k_sq_error", E3K_ERR_INVALID, n=0),
    refuse("sq_refuse_pred_null", "pred NULL", "e3k_sq_error", E3K_ERR_INVALID, null="pred"),
    refuse("sq_refuse_target_null", "target NULL", "e3k_sq_error", E3K_ERR_INVALID, null="target"),
    refuse("sq_refuse_loss_null", "loss NULL", "e3k_sq_error", E3K_ERR_INVALID, null="loss"),
    refuse("sq_refuse_grad_null", "grad NULL", "e3k_sq_error", E3K_ERR_INVALID, null="grad"),
    refuse("sq_refuse_group0", "w_group = 0 with a weight", "e3k_sq_error", E3K_ERR_INVALID, w_group=0),
] + [adam(f"adam_n{n}", f"n = {n}: " + ("tail only" if n < 4 else "one float4 and a tail" if n & 3 else "no tail"), n, ema=True, max_norm=1e4, wd=0.01)
     for n in (1, 2, 3, 4, 5, 7)] + [
    adam("adam_plain", "no EMA, no norm: tick_kernel alone, adam_ema_kernel<false>", 1027, ema=False),
    adam("adam_eps_placement", "every seventh element has v = 0 and g = 0 but m != 0: the denominator is eps alone", 1027, ema=False, v0=True),
    adam("adam_plain_wd", "... with weight decay", 5, ema=False, wd=0.01),
    adam("adam_plain_clip", "no EMA, a clip that bites", 1027, ema=False, max_norm=0.5),
    adam("adam_ema", "EMA, no norm: tick_both_kernel; decay from the update count", 1027, use_num=1),
    adam("adam_ema_fixed_decay", "ema_use_num_updates = 0: the plain decay from the first update", 7, use_num=0),
    adam("adam_ema_clip_bites", "EMA + a clip that bites, weight decay applied AFTER the clip scale", 1027, max_norm=0.5, wd=0.01),
    adam("adam_ema_clip_loose", "a clip that does not bite: coefficient exactly 1", 1027, max_norm=1e4, use_num=0),
    adam("adam_skip_nan_tail", "NaN only in the LAST tail element: the norm must see it; the step behind a skipped one", 1027, skip=1, steps=("ok", "nan_tail", "ok")),
    adam("adam_skip_inf_body", "+-inf in the float4 body, no clip", 1027, skip=1, steps=("inf_body", "ok", "inf_body")),
    adam("adam_skip_overflow", "finite gradients whose square sum overflows; with a clip", 1027, skip=1, max_norm=0.5, steps=("ok", "overflow", "ok")),
    adam("adam_skip_no_ema", "skip without an EMA: nothing but the state block moves", 7, ema=False, skip=1, steps=("nan_tail", "ok", "ok")),
    adam("adam_skip_finite", "skip_nonfinite with finite gradients: an ordinary step, the norm recorded", 5, skip=1, wd=0.01),
    adam("adam_norm_stride", "n = 524288 + 5: sumsq_kernel's grid-stride loop (512 workgroups of 1024 elements) and its tail", 524288 + 5, ema=False, max_norm=0.5),
    adam("adam_update_stride", "n = 2097152 + 7: the update's grid-stride loop and its tail together", 2097152 + 7, max_norm=0.5, wd=0.01),
    adam_pair("adam_tick_pair", "tick_both_kernel leaves what tick_kernel + ema_tick_kernel leave: every word but [7]", 1027),
    refuse("adam_refuse_misaligned", "param 4 bytes past a 16-byte boundary", "e3k_adam_ema_step", E3K_ERR_INVALID, shift="p"),
    refuse("adam_refuse_misaligned_ema", "ema misaligned", "e3k_adam_ema_step", E3K_ERR_INVALID, shift="ema"),
    refuse("adam_refuse_beta1", "beta1 = 1", "e3k_adam_ema_step", E3K_ERR_INVALID, b1=1.0),
    refuse("adam_refuse_lr", "lr < 0", "e3k_adam_ema_step", E3K_ERR_INVALID, lr=-1e-3),
    refuse("adam_refuse_decay", "ema_decay > 1 with an ema", "e3k_adam_ema_step", E3K_ERR_INVALID, decay=1.5),
    refuse("adam_refuse_state_null", "state NULL", "e3k_adam_ema_step", E3K_ERR_INVALID, null="state"),
    refuse("adam_refuse_n_negative", "n < 0", "e3k_adam_ema_step", E3K_ERR_INVALID, n=-1),
    refuse("adam_n0", "n = 0: OK, nothing written (the state block included)", "e3k_adam_ema_step", E3K_OK, n=0),
]

# ---- slope: forward-mode tangent per knot and its reverse sweep
CASES += [
    slope("slope_R1", "one row: the clamped second row of the only workgroup; identity, k0 = 1", 1, 32, 1, 1, 0, oor=0),
    slope("slope_R2", "two rows, ssp, symmetric cutoff / r", 2, 64, 8, 2, 1, cut=1),
    slope("slope_R3", "odd R, k0 = 31, three layers of silu, p = 2.5", 3, 32, 31, 3, 2, p=2.5, seed=2),
    slope("slope_R17", "17 rows: two 16-row tiles of slope_wgrad_kernel in one range; k0 = H = 32, four layers of tanh, r_min 0.5",
          17, 32, 32, 4, 4, cut=1, oor=0, r_min=0.5, wbias=0.5),
    slope("slope_R37_nets5", "37 rows x 5 nets, k0 = 33; g_hidden with NULL entries", 37, 64, 33, 2, 2, nets=5, oor=0, null_gh=((0, 1), (3, 0), (4, 0), (4, 1))),
    slope("slope_R129_k48", "the table's own knots (first at 1e-6 h, rows at and beyond r_max), k0 = 48 at H = 64: g_bessel per frequency",
          129, 64, 48, 2, 1, radii="knots", r_max=3.75, cut=1),
    slope("slope_R129_k64", "k0 = H = 64: the frequencies 32.. of g_bessel once were dropped", 129, 64, 64, 2, 2, radii="knots", r_max=3.75, cut=1, oor=0, r_min=0.5),
    slope("slope_R129_polynomial_knots", "the polynomial cutoff (p = 6) on the table's knots from 1e-6 h to 0.89 r_max, with 1 / r",
          129, 64, 8, 2, 1, radii="knots_inside", r_max=4.5, r_min=0.5),
    slope("slope_R641_production", "641 knots of a production table, five nets, ssp, three layers", 641, 64, 8, 3, 1, nets=5, radii="knots", r_max=5.0, r_min=0.5, cut=1),
    slope("slope_nets16", "16 nets, one layer", 37, 32, 8, 1, 4, nets=16, cut=1),
    slope("slope_sat_ssp", "|al z| reaches 20: saturated sigmoid, ssp's tail", 129, 64, 8, 2, 1, sat=True),
    slope("slope_sat_silu", "|al z| reaches 20, silu", 129, 64, 8, 3, 2, sat=True, p=2.5, oor=0),
    slope("slope_sat_tanh", "|al z| reaches 20, tanh: 1 - t^2 cancels", 129, 32, 8, 2, 4, sat=True, cut=1),
    slope("slope_gb_null", "g_bessel NULL: the hidden gradients still arrive", 37, 64, 8, 2, 1, gb=False),
    slope("slope_from_zero", "gradients handed over zero", 17, 64, 8, 2, 2, prefill=False),
    slope("slope_fwd_only", "the forward alone, identity through four layers", 37, 64, 8, 4, 0, op="fwd", oor=0, wbias=0.5),
] + [refuse(f"slope_refuse_{fn[-3:]}_{k}", why, fn, rc, **over) for fn in ("e3k_slope_tangent_fwd", "e3k_slope_tangent_bwd") for k, why, rc, over in (
    ("nets0", "n_nets = 0", E3K_ERR_INVALID, dict(nets=0)), ("nets17", "n_nets = 17", E3K_ERR_INVALID, dict(nets=17)),
    ("hidden0", "n_hidden = 0", E3K_ERR_INVALID, dict(nh=0)), ("hidden5", "n_hidden = 5", E3K_ERR_INVALID, dict(nh=5)),
    ("R0", "R = 0", E3K_ERR_INVALID, dict(R=0)), ("H48", "H = 48", E3K_ERR_UNSUPPORTED, dict(H=48)),
    ("k0_0", "k0 = 0", E3K_ERR_UNSUPPORTED, dict(k0=0)), ("k0_above_H", "k0 > H", E3K_ERR_UNSUPPORTED, dict(k0=33, H=32)),
    ("act3", "tanhlu has no second derivative here", E3K_ERR_UNSUPPORTED, dict(act=3)), ("act5", "abs", E3K_ERR_UNSUPPORTED, dict(act=5)),
    ("cut2", "cutoff kind 2", E3K_ERR_INVALID, dict(cut=2)), ("r_max_le_r_min", "r_max <= r_min", E3K_ERR_INVALID, dict(r_min=4.0)),
    ("R_2p31", "R = 2^31: the kernels index rows with int", E3K_ERR_UNSUPPORTED, dict(R=2 ** 31)),
    ("R_2p31_m1", "R = 2^31 - 1", E3K_ERR_UNSUPPORTED, dict(R=2 ** 31 - 1)),
    ("w_null", "w_hidden NULL", E3K_ERR_INVALID, dict(null="W")), ("w01_null", "w_hidden[0 * 4 + 1] NULL", E3K_ERR_INVALID, dict(null="W01")),
    ("alphas_null", "alphas NULL", E3K_ERR_INVALID, dict(null="alphas")), ("knots_null", "knots NULL", E3K_ERR_INVALID, dict(null="r")),
    ("bessel_null", "bessel_w NULL", E3K_ERR_INVALID, dict(null="w")), ("io_null", "hp / g_hp NULL", E3K_ERR_INVALID, dict(null="io")),
    ("io1_null", "hp[1] / g_hp[1] NULL", E3K_ERR_INVALID, dict(null="io1")))
] + [
    refuse("slope_refuse_bwd_acc_null", "scratch NULL", "e3k_slope_tangent_bwd", E3K_ERR_INVALID, null="acc"),
    refuse("slope_refuse_bwd_g_hidden_null", "the array g_hidden NULL (its entries may be)", "e3k_slope_tangent_bwd", E3K_ERR_INVALID, null="gh"),
]


def table_kernels():
    return {k for c in CASES for k in c["kernels"]}


def table_functions():
    return {f for c in CASES for f in c["funcs"]}


# ---------------------------------------------------------------------------------------------------------------------------------
# radial MLP: inputs and references
def mlp_inputs(c):
    rng, k0, h, nl, rows, nets = _rng(c), c["k0"], c["h"], c["nl"], c["rows"], c["nets"]
    if c["exact"]:
        draw = lambda *s: rng.integers(-3, 4, s).astype(f32)
        alphas, cst = [0.5, 0.25, 0.5, 0.25][:nl], 1.0
    else:
        draw = lambda *s: rng.standard_normal(s).astype(f32)
        alphas, cst = [_f(1.0 / np.sqrt(k0))] + [_f(1.0 / np.sqrt(h))] * (nl - 1), _f(1.3)
    inp = dict(x=draw(rows, k0), alphas=alphas, cst=cst, W=[], g=[], old=[])
    for _ in range(nets):
        inp["W"].append([draw(k0 if l == 0 else h, h) for l in range(nl)])
        inp["g"].append(draw(rows, h))
        inp["old"].append([draw(k0 if l == 0 else h, h) if c["prefill"] else np.zeros((k0 if l == 0 else h, h), f32) for l in range(nl)])
    return inp


def mlp_forward(c, inp, i):
    """(zs, dzs, out, dout) of net i in float64"""
    return _mlp_forward_ref(inp["x"].astype(f64), [w.astype(f64) for w in inp["W"][i]], inp["alphas"], c["act"], inp["cst"])


def mlp_backward(c, inp, i, z32):
    """from the fp32 pre-activations z32 the forward left: ([(g_W, bound)], (g_x, bound)); the old value of an accumulated g_W is one
    more term of the order-independent sum"""
    R = c["rows"]
    gWs, dgWs, gx, dgx = _mlp_backward_ref(inp["x"].astype(f64), [w.astype(f64) for w in inp["W"][i]], inp["alphas"], c["act"], inp["cst"],
                                           [z.astype(f64) for z in z32], inp["g"][i].astype(f64))
    olds = [o.astype(f64) for o in inp["old"][i]]
    return [(o + g, d + (R + 5) * U * np.abs(o)) for o, g, d in zip(olds, gWs, dgWs)], (gx, dgx)


def mlp_exact_ok(c, inp, i):
    """every partial sum of an exact case is a multiple of 2^-3 below 2^20: exact in fp32 in any order"""
    x, Ws, al = inp["x"].astype(f64), [np.abs(w.astype(f64)) for w in inp["W"][i]], inp["alphas"]
    prev, worst = np.abs(x), 0.0
    for W, a in zip(Ws, al):
        prev = a * (prev @ W)
        worst = max(worst, float(prev.max()) / a)
    g = np.abs(inp["g"][i].astype(f64))
    hs = [np.abs(x)]
    for W, a in zip(Ws, al):
        hs.append(a * (hs[-1] @ W))
    for l in range(len(Ws) - 1, -1, -1):
        worst = max(worst, float((hs[l].T @ g).max()) + float(np.abs(inp["old"][i][l]).max()), float((g @ Ws[l].T).max()))
        g = al[l] * (g @ Ws[l].T)
    return worst < 2.0 ** 20


# ---------------------------------------------------------------------------------------------------------------------------------
# optimiser: inputs and references
def sq_inputs(c):
    rng, n = _rng(c), c["n"]
    out = dict(pred=rng.standard_normal(n).astype(f32), target=rng.standard_normal(n).astype(f32), w=None)
    if c["w_group"]:
        w = rng.uniform(0.0, 2.0, -(-n // c["w_group"])).astype(f32)
        w[::5] = 0.0      # ghost entries of a padded batch
        out["w"] = w
    return out


def sq_reference(c, inp, mutant=None):
    """grad[i] = ((2 scale) w_i) d_i and loss = scale * sum_i (w_i d_i) d_i, the sum in any order"""
    n, scale = c["n"], _f(c["scale"])
    d = EV(inp["pred"].astype(f64)) - EV(inp["target"].astype(f64))
    if inp["w"] is None:
        wi = EV(np.full(n, float(f32(1.0) / f32(n))))
    else:
        idx = np.arange(n) if mutant == "weight_by_i" else np.arange(n) // c["w_group"]
        wi = EV(inp["w"].astype(f64)[np.minimum(idx, len(inp["w"]) - 1)])
    grad = (EV(2.0 * scale) * wi) * d
    loss = EV(scale) * sum_ev((wi * d) * d, 0)
    return dict(grad=grad.pair(), loss=loss.pair())


HP = dict(lr=_f(1e-3), b1=_f(0.9), b2=_f(0.999), eps=_f(1e-8))
KEEP_WORDS = (3, 10, 11, 12, 13, 14, 15)      # no kernel touches them
SENTINEL = 7.25


def adam_hp(c, **over):
    hp = dict(HP, wd=_f(c.get("wd", 0.0)), decay=_f(c.get("decay", 0.999)), use_num=c.get("use_num", 1), max_norm=_f(c.get("max_norm", 0.0)),
              skip=c.get("skip", 0), ema=c.get("ema", True))
    hp.update(over)
    return hp


def adam_inputs(c):
    rng, n = _rng(c), c["n"]
    p = rng.standard_normal(n).astype(f32)
    state = np.zeros(16, f32)
    state[list(KEEP_WORDS)] = SENTINEL
    v = (0.01 * rng.standard_normal(n) ** 2).astype(f32)
    if c.get("v0"):
        v[::7] = 0.0
    return dict(p=p, m=(0.1 * rng.standard_normal(n)).astype(f32), v=v, ema=(p + 0.01 * rng.standard_normal(n).astype(f32)).astype(f32), state=state)


def adam_grad(c, step):
    rng, n, kind = _rng(c, f":g{step}"), c["n"], c["steps"][step]
    g = rng.standard_normal(n).astype(f32)
    if c.get("v0"):
        g[::7] = 0.0
    if kind == "nan_tail":
        g[n - 1] = np.nan
    elif kind == "inf_body":
        assert n >= 16
        g[(n // 8) * 4 + 1], g[(n // 16) * 4 + 2] = np.inf, -np.inf
    elif kind == "overflow":
        assert n >= 16
        g[rng.permutation(n - (n & 3))[:8]] = 1.5e19
    else:
        assert kind == "ok"
    return g


def _ulp32(v):
    return float(np.spacing(np.abs(f32(v))))


def tick_reference(sw, g, hp, mutant=None):
    """the state block after the tick(s) from the 16 words before: {word: ("exact", value) | ("nan",) | ("ulp", value) |
    ("close", value, bound)}; words not listed keep their bits"""
    have_norm = hp["max_norm"] > 0 or bool(hp["skip"])
    out, bad, norm = {}, False, None
    if have_norm:
        g64 = g.astype(f64)
        if not np.isfinite(g64).all():
            bad, norm = True, ("nan",) if np.isnan(g64).any() else ("exact", np.inf)
        else:
            ssq = sum_ev(EV(g64) * EV(g64), 0)
            lo, hi = float(ssq.v - ssq.e), float(ssq.v + ssq.e)
            assert lo > 1.0001 * FLT_MAX or hi < 0.9999 * FLT_MAX, "the square sum must overflow in every order or in none"
            if lo > FLT_MAX:
                bad, norm = True, ("exact", np.inf)
            else:
                nv = ssq.sqrt()
                norm = ("close", float(nv.v), float(nv.e))
    skip = bool(hp["skip"]) and bad
    t = float(sw[0]) + (0.0 if skip else 1.0)
    out[0], out[6], out[5] = ("exact", t), ("exact", 1.0 if skip else 0.0), ("exact", 0.0)
    tb = max(t, 1.0) - (1.0 if mutant == "bias_t_minus_1" else 0.0)
    out[1], out[2] = ("ulp", float(f32(1.0 - hp["b1"] ** tb))), ("ulp", float(f32(1.0 - hp["b2"] ** tb)))
    out[7] = norm if have_norm else ("exact", 0.0)
    out[4] = ("exact", 1.0)
    if hp["max_norm"] > 0 and have_norm and not bad:
        cq = EV(hp["max_norm"]) / (EV(norm[1], norm[2]) + _f(1e-6))
        assert abs(float(cq.v) - 1.0) > 4 * float(cq.e), "the clip decision must not hinge on rounding"
        if float(cq.v) < 1.0:
            out[4] = ("close", float(cq.v), float(cq.e))
    if hp["ema"]:
        k = float(sw[8]) + 1.0
        out[8] = ("exact", k)
        d = EV(hp["decay"])
        if hp["use_num"]:
            kk = k - 1.0 if mutant == "ema_k_off_by_one" else k
            alt = (EV(1.0) + kk) / (EV(10.0) + kk)
            d = alt if float(alt.v) < hp["decay"] else d
        out[9] = ("close", float(d.v), float(d.e))
    return out


def adam_reference(p, g, m, v, ema, sw, hp, mutant=None):
    """adam_ema_kernel's operations replayed on EV from exact fp32 inputs and the state words sw the tick left: {name: (want, bound)}"""
    p, g, m, v = (EV(a.astype(f64)) for a in (p, g, m, v))
    skip = float(sw[6]) != 0.0
    out = {}
    p1 = p
    if not skip:
        step = EV(hp["lr"]) / EV(float(sw[1]))
        isb = 1.0 / np.sqrt(float(sw[2]))
        isb = EV(isb, ULP_RSQRT * 2 * U * isb)
        gs, wd = EV(float(sw[4])), hp["wd"]
        if mutant == "wd_before_clip":
            gv = (fma(wd, p, g) if wd != 0.0 else g) * gs
        else:
            gv = g * gs
            if wd != 0.0:
                gv = fma(wd, p, gv)
        m1 = fma(hp["b1"], m, (EV(1.0) - hp["b1"]) * gv)
        v1 = fma(hp["b2"], v, ((EV(1.0) - hp["b2"]) * gv) * gv)
        den = (v1 + hp["eps"]).sqrt() * isb if mutant == "eps_under_root" else v1.sqrt() * isb + hp["eps"]
        p1 = p - step * (m1 / den)
        out.update(p=p1.pair(), m=m1.pair(), v=v1.pair())
    if ema is not None:
        e0 = EV(ema.astype(f64))
        omd = EV(1.0) - float(sw[9])
        out["ema"] = (e0 - omd * (e0 - (p if mutant == "ema_from_old_p" else p1))).pair()
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# slope: float64 on both sides.  D64 carries a float64 value and a bound on |device float64 result - value|
U64 = 2.0 ** -53
R64 = 2 * U64          # one rounding on either side
ULP64 = 16             # the device's double exp, log1p, tanh, sin, cos, pow: no HIP math table is shipped with the ROCm install: OpenCL's loosest double bound
FN64 = (ULP64 + 1) * 2 * U64      # (an ulp is at most 2 u |f|; numpy's own function within one)
SL_SPLIT = 8           # row ranges of slope_wgrad_kernel


class D64:
    __slots__ = ("v", "e")

    def __init__(self, v, e=0.0):
        self.v = np.asarray(v, f64)
        self.e = np.zeros_like(self.v) + e

    @staticmethod
    def of(x):
        return x if isinstance(x, D64) else D64(x)

    @staticmethod
    def _r(v, e):
        return D64(v, e + R64 * np.abs(v))

    def __add__(self, o):
        o = D64.of(o)
        return D64._r(self.v + o.v, self.e + o.e)

    __radd__ = __add__

    def __sub__(self, o):
        o = D64.of(o)
        return D64._r(self.v - o.v, self.e + o.e)

    def __rsub__(self, o):
        return D64.of(o) - self

    def __mul__(self, o):
        o = D64.of(o)
        return D64._r(self.v * o.v, np.abs(self.v) * o.e + np.abs(o.v) * self.e + self.e * o.e)

    __rmul__ = __mul__

    def __truediv__(self, o):
        o = D64.of(o)
        with np.errstate(divide="ignore", invalid="ignore"):
            v = self.v / o.v
            den = np.abs(o.v) - o.e
            e = np.where(den > 0, (self.e + np.abs(v) * o.e) / np.where(den > 0, den, 1.0), np.inf)
        return D64._r(v, e)

    def __rtruediv__(self, o):
        return D64.of(o) / self

    def where(self, cond):
        """zero (exactly) where cond does not hold"""
        return D64(np.where(cond, self.v, 0.0), np.where(cond, self.e, 0.0))


def mm64(a, b):
    """a @ b in FMA chains of K terms (either operand may carry an error)"""
    a, b = D64.of(a), D64.of(b)
    K = a.v.shape[1]
    return D64(a.v @ b.v, a.e @ np.abs(b.v) + np.abs(a.v) @ b.e + a.e @ b.e + (K + 1) * R64 * (np.abs(a.v) @ np.abs(b.v)))


def sig64(x):
    """1 / (1 + exp(-x)): the exponential's relative error reaches s scaled by 1 - s; a sum and a quotient"""
    with np.errstate(over="ignore"):
        s = 1.0 / (1.0 + np.exp(-x.v))
    return D64(s, s * (1.0 - s) * x.e + 0.1 * x.e ** 2 + (FN64 + 3 * R64) * s)


def act64(a, x):
    """(f, f', f'') of csrc/e3k_slope.hip's act64 with their float64 discrepancy bounds"""
    if a == 1:
        s = sig64(x)
        with np.errstate(over="ignore"):
            f = np.maximum(x.v, 0.0) + np.log1p(np.exp(-np.abs(x.v))) - np.log(2.0)
        return D64(f, s.v * x.e + 0.2 * x.e ** 2 + (2 * FN64 + 4 * R64) * (np.abs(x.v) + 1.4)), s, s * (1.0 - s)
    if a == 2:
        s = sig64(x)
        return x * s, s * (1.0 + x * (1.0 - s)), s * (1.0 - s) * (2.0 + x * (1.0 - 2.0 * s))
    if a == 4:
        t = np.tanh(x.v)
        t = D64(t, (1.0 - t * t) * x.e + 0.8 * x.e ** 2 + FN64 * np.abs(t))
        d1 = 1.0 - t * t
        return t, d1, -2.0 * t * d1
    assert a == 0
    return x, D64(np.ones_like(x.v)), D64(np.zeros_like(x.v))


def slope_params(c):
    from tests.test_gpu_edge_matrix import rad_params

    return rad_params(c)      # (asserts that r_max - r_min is exact in fp32)


def slope_radii(c, rng):
    R, r_max = c["R"], c["r_max"]
    if c["radii"] == "knots":
        if c["R"] == 641:      # the production table: the radii the library itself builds
            from e3_layers_amd.backend.radial_table import knot_radii

            r = knot_radii(r_max, 640, "cpu").numpy()
            assert len(r) == R and r[-1] == f32(r_max)
            return r
        h = 2.0 ** -5
        r = np.arange(R) * h
        r[0] = 1e-6 * h
        assert r[-1] > r_max and (r == r_max).any()      # rows at and beyond r_max
        return r.astype(f32)
    if c["radii"] == "knots_inside":      # the same knots under a cutoff that ends behind the last of them
        h = 2.0 ** -5
        r = np.arange(R) * h
        r[0] = 1e-6 * h
        assert 0.85 * r_max < r[-1] < 0.9 * r_max
        return r.astype(f32)
    # away from the end of the cutoff, where it cancels and float64 rounding of its own shows in every element of a row (the knot
    # cases have those rows; here only the planted ones)
    r = (rng.uniform(0.05, 0.8, R) * r_max).astype(f32)
    if R >= 3:
        r[R - 1] = r_max
    if R >= 100:
        r[R // 2], r[R // 3] = np.nextafter(f32(r_max), f32(0)), 1.5 * r_max
    return r


def slope_plain_forward(r, w, Ws, alphas, cst, prm, a, dt=f64, mutant=None):
    """the kernel's formulas written out in numpy at precision dt (float64: the CPU model; longdouble: what the bounds are held to):
    per layer (a, a', al z, z', f', f'') and the basis' frequency derivatives"""
    r, w = r.astype(dt)[:, None], w.astype(dt)[None, :]
    r_max, p, kind = dt(prm["r_max"]), dt(prm["p"]), prm["cut"]
    if mutant == "cutoff_swapped":
        kind = 1 - kind
    delta = r_max if mutant == "delta_is_r_max" else r_max - dt(prm["r_min"])
    pref, x = dt(2) / delta, r / r_max
    one = dt(1)
    with np.errstate(all="ignore"):
        if kind == 1:
            q = x * x - one
            cc, dc = np.where(np.abs(x) < 1, q * q, 0), np.where(np.abs(x) < 1, 4 * q * x / r_max, 0)
        else:
            c0, c1, c2 = (p + 1) * (p + 2) / 2, p * (p + 2), p * (p + 1) / 2
            xs = np.where(x < 1, x, 0)
            xp = xs ** p
            cc = np.where(x < 1, one - c0 * xp + c1 * xp * xs - c2 * xp * xs * xs, 0)
            xpm1 = np.where(xs != 0, xp / np.where(xs != 0, xs, one), 0)
            dc = np.where(x < 1, (-c0 * p * xpm1 + c1 * (p + 1) * xp - c2 * (p + 2) * xp * xs) / r_max, 0)
        A, dA = (pref * cc / r, pref * (dc / r - cc / (r * r))) if prm["oor"] else (pref * cc, pref * dc)
    th = w * r / delta
    sn, cs = np.sin(th), np.cos(th)
    lv = [dict(a=A * sn, da=dA * sn + A * (w / delta) * cs)]
    bw, dbw = A * (r / delta) * cs, dA * (r / delta) * cs + A * (cs / delta - (w / delta) * (r / delta) * sn)
    for W, al in zip(Ws, alphas):
        W, al, L = W.astype(dt), dt(al), lv[-1]
        z, dz = L["a"] @ W, L["da"] @ W
        xx = al * z
        with np.errstate(over="ignore"):
            if a in (1, 2):
                s = one / (one + np.exp(-xx))
            if a == 1:
                f, d1, d2 = np.maximum(xx, 0) + np.log1p(np.exp(-np.abs(xx))) - np.log(dt(2)), s, s * (one - s)
            elif a == 2:
                f, d1, d2 = xx * s, s * (one + xx * (one - s)), s * (one - s) * (2 + xx * (one - 2 * s))
            elif a == 4:
                t = np.tanh(xx)
                f, d1 = t, one - t * t
                d2 = -2 * t * d1
            else:
                f, d1, d2 = xx, np.ones_like(xx), np.zeros_like(xx)
        L.update(dz=dz, d1=d1, d2=d2, al=al)
        lv.append(dict(a=dt(cst) * f, da=dt(cst) * d1 * al * dz))
    return lv, bw, dbw


def slope_split(R):
    per = -(-(-(-R // SL_SPLIT)) // 16) * 16
    return [(b, min(b + per, R)) for b in range(0, R, per)]


def slope_plain_backward(lv, bw, dbw, Ws, cst, g_hp, dt=f64, mutant=None):
    """the reverse sweep written out: per layer the partial sums of g_W over the kernel's row ranges, and the Bessel terms per row"""
    R = g_hp.shape[0]
    g_t, g_v = g_hp.astype(dt), np.zeros(g_hp.shape, dt)
    rows = slice(0, R - 1) if mutant == "last_odd_row_dropped" and R % 2 else slice(0, R)
    ranges = slope_split(R)
    if mutant == "last_range_dropped" and len(ranges) > 1:
        ranges = ranges[:-1]
    parts = [None] * len(Ws)
    for l in range(len(Ws) - 1, -1, -1):
        L, W = lv[l], Ws[l].astype(dt)
        al, cs_ = L["al"], dt(cst)
        gdz = g_t * cs_ * L["d1"] * al
        gz = g_v * cs_ * L["d1"] + (0 if mutant == "no_d2" else g_t * cs_ * L["d2"] * al * L["dz"])
        gz = gz if mutant == "alpha_once" else gz * al
        keep = np.zeros(R, bool)
        keep[rows] = True
        parts[l] = [L["a"][b:e][keep[b:e]].T @ gz[b:e][keep[b:e]] + L["da"][b:e][keep[b:e]].T @ gdz[b:e][keep[b:e]] for b, e in ranges]
        g_v, g_t = gz @ W.T, gdz @ W.T
    terms = g_v * bw + g_t * dbw
    return parts, terms[rows].sum(0)


def slope_inputs(c):
    rng, R, H, k0, nh, nets = _rng(c, f":{c['seed']}" if c["seed"] else ""), c["R"], c["H"], c["k0"], c["nh"], c["nets"]
    prm = slope_params(c)
    r = slope_radii(c, rng)
    w = (np.arange(1, k0 + 1) * np.pi * (1.0 + 0.05 * rng.standard_normal(k0))).astype(f32)
    alphas = [_f(1.0 / np.sqrt(k0))] + [_f(1.0 / np.sqrt(H))] * (nh - 1)
    cst = _f(1.3)
    Ws, g_hp, old = [], [], []
    for i in range(nets):
        W = [(c["wbias"] + rng.standard_normal((k0 if l == 0 else H, H))).astype(f32) for l in range(nh)]
        if c["sat"] and i == 0:      # unit 0 of the first layer reaches |al z| = 20: saturated sigmoid / tanh, ssp's tail
            for l in (0,):
                lv, _, _ = slope_plain_forward(r, w, W, alphas, cst, prm, c["act"])
                top = float(np.abs(lv[l]["al"] * (lv[l]["a"] @ W[l].astype(f64)))[:, 0].max())
                W[l][:, 0] = (W[l][:, 0].astype(f64) * (20.0 / top)).astype(f32)
        Ws.append(W)
        g = rng.standard_normal((R, H)).astype(f32)
        g[r >= f32(prm["r_max"])] = 0.0
        g_hp.append(g)
        old.append([rng.standard_normal(Wl.shape).astype(f32) if c["prefill"] else np.zeros(Wl.shape, f32) for Wl in W])
    old_b = rng.standard_normal(k0).astype(f32) if c["prefill"] else np.zeros(k0, f32)
    return dict(prm=prm, r=r, w=w, alphas=alphas, cst=cst, W=Ws, g_hp=g_hp, old=old, old_b=old_b)


def slope_basis_replay(r, w, prm):
    """basis64 of csrc/e3k_slope.hip replayed on D64: the bound on what two float64 evaluations of b, b', db/dw, db'/dw differ by.  r, w,
    r_max, delta and p are exact inputs; where the two terms of b' cancel (r -> 0 with one_over_r) the bound is that of the terms"""
    r, w = D64(r[:, None]), D64(w[None, :])
    r_max, p = prm["r_max"], prm["p"]
    delta = r_max - prm["r_min"]
    pref, x = 2.0 / delta, r / r_max
    if prm["cut"] == 1:
        inside = np.abs(x.v) < 1.0
        q = x * x - 1.0
        cc, dc = (q * q).where(inside), (4.0 * q * x / r_max).where(inside)
    else:
        inside = x.v < 1.0
        xs = np.where(inside, x.v, 0.0)
        c0, c1, c2 = (p + 1.0) * (p + 2.0) * 0.5, p * (p + 2.0), p * (p + 1.0) * 0.5
        # pow's own error reaches c and c' through ONE value x^p: c = 1 - x^p P(x), c' = x^p Q(x) / r_max, so its share is
        # e_pow |P| and e_pow |Q| / r_max (P(1) = 1 while c0 + c1 + c2 = 97 at p = 6); the roundings of the products and sums of the
        # form the kernel evaluates are replayed on the exact x^p
        xp = D64(xs ** p)
        e_pow = (FN64 + p * R64) * xs ** p
        safe = np.where(xs != 0, xs, 1.0)
        xpm1 = (xp / D64(safe, R64 * xs)).where(xs != 0)
        xx = D64(xs, R64 * xs)
        cc = (1.0 - c0 * xp + c1 * xp * xx - c2 * xp * xx * xx).where(inside)
        dc = ((-c0 * p * xpm1 + c1 * (p + 1.0) * xp - c2 * (p + 2.0) * xp * xx) / r_max).where(inside)
        cc = D64(cc.v, cc.e + np.where(inside, e_pow * np.abs(c0 - c1 * xs + c2 * xs * xs), 0.0))
        dc = D64(dc.v, dc.e + np.where(inside & (xs != 0), e_pow * np.abs(-c0 * p / safe + c1 * (p + 1.0) - c2 * (p + 2.0) * xs) / r_max, 0.0))
    if prm["oor"]:
        A, dA = pref * cc / r, pref * (dc / r - cc / (r * r))
    else:
        A, dA = pref * cc, pref * dc
    th = w * r / delta
    sn, cs = np.sin(th.v), np.cos(th.v)
    sn, cs = D64(sn, np.abs(cs) * th.e + th.e ** 2 + FN64 * np.abs(sn)), D64(cs, np.abs(sn) * th.e + th.e ** 2 + FN64 * np.abs(cs))
    rd, wd = r / delta, w / delta
    return A * sn, dA * sn + A * wd * cs, A * rd * cs, dA * rd * cs + A * (cs / delta - wd * rd * sn)


def slope_basis64(c, inp):
    """b, b', db/dw, db'/dw on (row, frequency): the VALUES from the definition the edge kernels are tested against (autograd of
    rad_formula), the float64 allowance from the replay above.  The two float64 evaluations must agree within 3 of those allowances;
    the device is within one allowance of the replay, so within that plus the gap between the two of the values used"""
    from tests.test_gpu_edge_matrix import rad_derivatives

    r, w, prm = inp["r"].astype(f64), inp["w"].astype(f64), inp["prm"]
    d = rad_derivatives(r, w, prm, second=True)
    out = []
    for k, q in zip(("out", "fR", "fW", "fRW"), slope_basis_replay(r, w, prm)):
        assert np.isfinite(q.v).all() and np.isfinite(q.e).all() and np.isfinite(d[k]).all()
        gap = np.abs(q.v - d[k])
        assert (gap <= 3.0 * q.e).all(), f"{k}: the two float64 references differ by {float((gap / np.maximum(q.e, 1e-300)).max()):.1f} allowances"
        out.append(D64(d[k], q.e + gap))
    return out


def slope_reference(c, inp):
    """{"hp": [(want, bound, F64)], "gw": {(net, layer): (want, bound, F64)}, "gb": (want, bound, F64)}: explicit float64 formulas with a
    running bound F64 on what two float64 evaluations may differ by; the fp32 terms on top are those of the kernel's casts"""
    R, H, k0, nh, a = c["R"], c["H"], c["k0"], c["nh"], c["act"]
    b, db, bw, dbw = slope_basis64(c, inp)
    cst, ranges = inp["cst"], slope_split(R)
    out = dict(hp=[], gw={}, gb=None)
    gb_v, gb_e = np.zeros(k0), np.zeros(k0)
    for i in range(c["nets"]):
        Ws = [W.astype(f64) for W in inp["W"][i]]
        lv = [dict(a=b, da=db)]
        for W, al in zip(Ws, inp["alphas"]):
            L = lv[-1]
            z, dz = mm64(L["a"], W), mm64(L["da"], W)
            f, d1, d2 = act64(a, al * z)
            L.update(dz=dz, d1=d1, d2=d2, al=al)
            lv.append(dict(a=cst * f, da=cst * d1 * al * dz))
        hp = lv[-1]["da"]
        beyond = inp["r"] >= f32(inp["prm"]["r_max"])
        assert (hp.v[beyond] == 0).all() and (hp.e[beyond] == 0).all()
        # (a row at or beyond r_max: exactly +0.0 or -0.0, compared with == 0)
        out["hp"].append((hp.v, np.where(beyond[:, None], 0.0, U * np.abs(hp.v) + FL + hp.e), hp.e))
        if c["op"] == "fwd":
            continue
        g_t, g_v = D64(inp["g_hp"][i].astype(f64)), D64(np.zeros((R, H)))
        for l in range(nh - 1, -1, -1):
            L, al = lv[l], lv[l]["al"]
            gdz = g_t * cst * L["d1"] * al
            gz = (g_v * cst * L["d1"] + g_t * cst * L["d2"] * al * L["dz"]) * al
            old = inp["old"][i][l].astype(f64)
            S = [mm64(D64(L["a"].v[lo:hi].T, L["a"].e[lo:hi].T), D64(gz.v[lo:hi], gz.e[lo:hi]))
                 + mm64(D64(L["da"].v[lo:hi].T, L["da"].e[lo:hi].T), D64(gdz.v[lo:hi], gdz.e[lo:hi])) for lo, hi in ranges]
            want = old + sum(s.v for s in S)
            mag = np.abs(old) + sum(np.abs(s.v) for s in S)
            f64e = sum(s.e for s in S) + (len(S) + 1) * R64 * mag      # (the reference's own sum over the ranges and the old value)
            # one rounding per cast, then len(S) atomic additions onto the old value in any order
            out["gw"][(i, l)] = (want, U * (mag - np.abs(old)) + gamma(len(S) + 1) * mag + FL + f64e, f64e)
            g_v, g_t = mm64(gz, Ws[l].T), mm64(gdz, Ws[l].T)
        t = g_v * bw + g_t * dbw
        gb_v += t.v.sum(0)
        gb_e += t.e.sum(0) + (R * c["nets"] + 1) * R64 * np.abs(t.v).sum(0)
    if c["op"] != "fwd":
        old = inp["old_b"].astype(f64)
        gb_e = gb_e + 2 * R64 * (np.abs(old) + np.abs(gb_v))
        out["gb"] = (old + gb_v, U * np.abs(gb_v) + U * np.abs(old + gb_v) + FL + gb_e, gb_e)
    return out


def slope_f64_share(c, ref):
    """the share of the elements whose F64 is below 1 % of the fp32 term (the condition: >= 99 % on every case)"""
    want = np.concatenate([w.ravel() for w, _, _ in ref["hp"]])
    e = np.concatenate([e.ravel() for _, _, e in ref["hp"]])
    return float((e <= 0.01 * (U * np.abs(want) + FL)).mean())


# ---------------------------------------------------------------------------------------------------------------------------------
# running the cases
WORST = {}


class Check(_Check):
    def claim_at(self, name, idx):
        """single words of a block (the state block: the words a kernel does not touch must keep their bits)"""
        off = self.ar.blocks[name][0]
        at = off + np.asarray(idx)
        assert not self.claimed[at].any(), name
        self.claimed[at] = True

    def finish(self):
        self.unchanged()
        for family, r in self.ratios.items():
            print(f"{self.case['id']}: {family} worst error / bound {r:.3f}")
            WORST[family] = max(WORST.get(family, 0.0), r)
            record_measured("test_gpu_train_matrix", case=self.case["id"], family=family, error_over_bound=r)

    def rebase(self):
        """the next call starts from what this one left"""
        self.ar.x0 = self.got.copy()


def _arena(c):
    return Arena(zlib.crc32(c["id"].encode()) ^ 0x7A7A)


def _poke(ar, name, values):
    off, n = ar.blocks[name]
    w = np.ascontiguousarray(values).ravel().view(np.int32)
    assert len(w) == n
    ar.x0[off:off + n] = w
    ar.buf[off:off + n].copy_(torch.from_numpy(w.copy()))


def _vp(vals):
    return (C.c_void_p * max(len(vals), 1))(*vals)


def _mlp_alloc(ar, c, inp, sfx=""):
    k0, h, nl, rows = c["k0"], c["h"], c["nl"], c["rows"]
    for i in range(c["nets"]):
        for l in range(nl):
            ar.alloc(f"z{sfx}{i}_{l}", rows * h)
            ar.alloc(f"gw{sfx}{i}_{l}", (k0 if l == 0 else h) * h, inp["old"][i][l])
        ar.alloc(f"out{sfx}{i}", rows * h).alloc(f"gx{sfx}{i}", rows * k0)


def _mlp_call(c, inp, ar, L, sfx=""):
    lib, st, p = L.load(), L.stream_ptr(), ar.p
    k0, h, nl, rows, nets = c["k0"], c["h"], c["nl"], c["rows"], c["nets"]
    al = (C.c_float * nl)(*inp["alphas"])
    zn = lambda i, l: None if c["z"] == "none" or c["z"] == l else p(f"z{sfx}{i}_{l}")
    gn = lambda i, l: None if c["gw"] == "none" or c["gw"] == l else p(f"gw{sfx}{i}_{l}")
    for n, tile in mlp_launches(rows, nets):
        assert lib.e3k_mlp_tile_rows(rows, n) == tile
    args = (p("x"), rows, k0, h, nl)
    if not c["multi"]:
        W = _vp([p(f"W0_{l}") for l in range(nl)])
        rc = lib.e3k_mlp_hidden_fwd(*args, W, al, c["act"], inp["cst"], None if c["z"] == "none" else _vp([zn(0, l) for l in range(nl)]),
                                    p(f"out{sfx}0"), st)
        assert rc == E3K_OK
        if c["op"] == "both":
            rc = lib.e3k_mlp_hidden_bwd(*args, W, al, c["act"], inp["cst"], _vp([zn(0, l) for l in range(nl)]), p("g0"),
                                        None if c["gw"] == "none" else _vp([gn(0, l) for l in range(nl)]), p(f"gx{sfx}0") if c["gx"] else None, st)
            assert rc == E3K_OK
        return
    arr = (L.MlpNet * nets)()
    for i in range(nets):
        for l in range(nl):
            arr[i].weights[l], arr[i].z[l], arr[i].g_weights[l] = p(f"W{i}_{l}"), zn(i, l), gn(i, l)
        arr[i].out, arr[i].g_out, arr[i].g_x = p(f"out{sfx}{i}"), p(f"g{i}"), p(f"gx{sfx}{i}") if c["gx"] else None
    assert lib.e3k_mlp_hidden_fwd_multi(arr, nets, *args, al, c["act"], inp["cst"], st) == E3K_OK
    if c["op"] == "both":
        assert lib.e3k_mlp_hidden_bwd_multi(arr, nets, *args, al, c["act"], inp["cst"], st) == E3K_OK


def run_mlp(dev, c, L):
    inp = mlp_inputs(c)
    k0, h, nl, rows, nets = c["k0"], c["h"], c["nl"], c["rows"], c["nets"]
    ar = _arena(c)
    ar.alloc("x", rows * k0, inp["x"])
    for i in range(nets):
        for l in range(nl):
            ar.alloc(f"W{i}_{l}", inp["W"][i][l].size, inp["W"][i][l])
        ar.alloc(f"g{i}", rows * h, inp["g"][i])
    _mlp_alloc(ar, c, inp)
    if c["repeat"]:
        _mlp_alloc(ar, c, inp, "r")
    ar.upload(dev)
    _mlp_call(c, inp, ar, L)
    if c["repeat"]:
        _mlp_call(c, inp, ar, L, "r")
    ck = Check(ar, c)
    cmp_ = (lambda name, want, bound, fam: ck.equal(name, want)) if c["exact"] else ck.close
    for i in range(nets):
        if c["exact"]:
            assert mlp_exact_ok(c, inp, i)
        zs, dzs, out, dout = mlp_forward(c, inp, i)
        for l in range(nl):
            if c["z"] != "none" and c["z"] != l:
                cmp_(f"z{i}_{l}", zs[l], dzs[l], "mlp_z")
        cmp_(f"out{i}", out, dout, "mlp_out")
        if c["op"] == "both":
            z32 = [ck.dev(f"z{i}_{l}", f32).reshape(rows, h) for l in range(nl)]
            gws, (gx, dgx) = mlp_backward(c, inp, i, z32)
            for l in range(nl):
                if c["gw"] != "none" and c["gw"] != l:
                    cmp_(f"gw{i}_{l}", *gws[l], "mlp_g_w")
            if c["gx"]:
                cmp_(f"gx{i}", gx, dgx, "mlp_g_x")
        if c["repeat"]:
            for name in [f"z{{}}{i}_{l}" for l in range(nl)] + [f"out{{}}{i}", f"gx{{}}{i}"]:
                ck.exact(name.format("r"), ck.dev(name.format("")))
            for l in range(nl):
                ck.close(f"gwr{i}_{l}", *gws[l], "mlp_g_w")
    ck.finish()


def run_sq(dev, c, L):
    inp, n = sq_inputs(c), c["n"]
    ar = _arena(c)
    ar.alloc("pred", n, inp["pred"], align=1).alloc("target", n, inp["target"], align=1)
    if inp["w"] is not None:
        ar.alloc("w", len(inp["w"]), inp["w"], align=1)
    ar.alloc("loss", 1, align=1).alloc("grad", n, align=1).upload(dev)
    rc = L.load().e3k_sq_error(ar.p("pred"), ar.p("target"), ar.p("w") if inp["w"] is not None else None, c["w_group"] or 0, n, _f(c["scale"]),
                               ar.p("loss"), ar.p("grad"), L.stream_ptr())
    assert rc == E3K_OK
    ck, ref = Check(ar, c), sq_reference(c, inp)
    ck.close("grad", *ref["grad"], "sq_error_grad")
    ck.close("loss", *ref["loss"], "sq_error_loss")
    ck.finish()


def check_state(ck, before, ref):
    """the 16 words against tick_reference; returns them"""
    got = ck.dev("state", f32).copy()
    ck.claim_at("state", sorted(ref))
    for w, r in ref.items():
        gv = float(got[w])
        if r[0] == "exact":
            assert gv == r[1], f"state[{w}] = {gv!r}, want {r[1]!r}"
        elif r[0] == "nan":
            assert np.isnan(gv), f"state[{w}] = {gv!r}, want NaN"
        elif r[0] == "ulp":
            assert abs(gv - r[1]) <= _ulp32(r[1]), f"state[{w}] = {gv!r}, want {r[1]!r} within one ulp"
        else:
            assert np.isfinite(gv) and abs(gv - r[1]) <= r[2], f"state[{w}] = {gv!r}, want {r[1]!r} +- {r[2]:.3e}"
            if r[2] > 0:
                ck.ratio(f"adam_state{w}", abs(gv - r[1]) / r[2])
    return got


def _adam_arena(c, inp, dev, shift=None):
    n = c["n"]
    ar = _arena(c)
    for k in ("p", "g", "m", "v") + (("ema",) if c["ema"] else ()):
        ar.alloc(k, n, inp[k] if k != "g" else np.zeros(n, f32), align=4, shift=1 if shift == k else 0)
    return ar.alloc("state", 16, inp["state"]).upload(dev)


def _adam_call(c, hp, ar, L, n=None, state=True):
    return L.load().e3k_adam_ema_step(ar.p("p"), ar.p("g"), ar.p("m"), ar.p("v"), ar.p("ema") if hp["ema"] else None, c["n"] if n is None else n,
                                      hp["lr"], hp["b1"], hp["b2"], hp["eps"], hp["wd"], hp["decay"], hp["use_num"], hp["max_norm"], hp["skip"],
                                      ar.p("state") if state else None, L.stream_ptr())


def run_adam(dev, c, L):
    inp, hp = adam_inputs(c), adam_hp(c)
    ar = _adam_arena(c, inp, dev)
    for step in range(len(c["steps"])):
        g = adam_grad(c, step)
        _poke(ar, "g", g)
        before = {k: ar.host(k).copy() for k in ("p", "m", "v", "state") + (("ema",) if c["ema"] else ())}
        assert _adam_call(c, hp, ar, L) == E3K_OK
        ck = Check(ar, c)
        sw = check_state(ck, before["state"], tick_reference(before["state"], g, hp))
        expect_skip = c["steps"][step] != "ok" and c["skip"]
        assert (sw[6] != 0) == bool(expect_skip)
        ref = adam_reference(before["p"], g, before["m"], before["v"], before.get("ema"), sw, hp)
        for k in ("p", "m", "v"):
            if expect_skip:
                ck.exact(k, before[k])
            else:
                assert np.isfinite(ref[k][1]).all()
                ck.close(k, *ref[k], "adam_" + k)
        if c["ema"]:
            ck.close("ema", *ref["ema"], "adam_ema")
        ck.finish()
        ck.rebase()


def run_adam_pair(dev, c, L):
    inp = adam_inputs(c)
    got = []
    for max_norm in (0.0, 1e30):
        hp = adam_hp(c, max_norm=_f(max_norm))
        ar = _adam_arena(c, inp, dev)
        for step in range(3):
            _poke(ar, "g", adam_grad(c, step))
            assert _adam_call(c, hp, ar, L) == E3K_OK
        torch.cuda.synchronize()
        got.append((ar, ar.buf.cpu().numpy()))
    (ar, one), (_, two) = got
    w7 = ar.blocks["state"][0] + 7
    assert one[w7] == 0 and two.view(f32)[w7] > 0
    differ = np.flatnonzero(one != two)
    assert list(differ) == [w7], f"words that differ between the one-launch tick and the two ticks: {differ[:8]} (blocks: {ar.blocks})"
    written = np.zeros(len(one), bool)      # (either run against what it was handed: nothing outside p, m, v, ema and the state block moved)
    for k in ("p", "m", "v", "ema", "state"):
        written[ar.blocks[k][0]:ar.blocks[k][0] + ar.blocks[k][1]] = True
    for a_, got_ in got:
        assert (got_[~written] == a_.x0[~written]).all(), "words outside the outputs changed"
    st = one.view(f32)[ar.blocks["state"][0]:][:16]
    assert st[0] == 3 and st[8] == 3 and st[4] == 1 and st[6] == 0


def run_refuse(dev, c, L):
    """a small valid problem of the entry point, one argument replaced: the return code, and the arena bit-identical"""
    lib, st, fn, o = L.load(), L.stream_ptr(), c["fn"], c["over"]
    ar = _arena(c)
    if fn.startswith("e3k_mlp"):
        k0, h, nl, rows, nets = o.get("k0", 8), o.get("h", 64), o.get("nl", 2), o.get("rows", 20), 2 if "multi" in fn else 1
        one = lambda name, n: ar.alloc(name, n, np.ones(n, f32))
        one("x", 20 * 64)
        for i in range(nets):
            for l in range(4):
                one(f"W{i}_{l}", 64 * 64), one(f"z{i}_{l}", 20 * 64), one(f"gw{i}_{l}", 64 * 64)
            one(f"out{i}", 20 * 64), one(f"g{i}", 20 * 64), one(f"gx{i}", 20 * 64)
        ar.upload(dev)
        p, null = ar.p, o.get("null")
        al = (C.c_float * 4)(0.5, 0.5, 0.5, 0.5)
        W = lambda i: [None if null == f"w{l}" else p(f"W{i}_{l}") for l in range(4)]
        Z = lambda i: [None if null == f"z{l}" else p(f"z{i}_{l}") for l in range(4)]
        args = (p("x"), rows, k0, h, nl)
        if fn == "e3k_mlp_tile_rows":
            rc = lib.e3k_mlp_tile_rows(rows, o["nets"])
        elif fn == "e3k_mlp_hidden_fwd":
            rc = lib.e3k_mlp_hidden_fwd(*args, _vp(W(0)), al, o.get("act", 2), 1.5, _vp(Z(0)), None if null == "out" else p("out0"), st)
        elif fn == "e3k_mlp_hidden_bwd":
            rc = lib.e3k_mlp_hidden_bwd(*args, _vp(W(0)), al, o.get("act", 2), 1.5, None if null == "z" else _vp(Z(0)), p("g0"),
                                        _vp([p(f"gw0_{l}") for l in range(4)]), p("gx0"), st)
        else:
            arr = (L.MlpNet * nets)()
            for i in range(nets):
                for l in range(4):
                    # (the refused argument sits in the LAST net: the nets before it must not have been launched)
                    arr[i].weights[l], arr[i].z[l] = (W(i)[l], Z(i)[l]) if i == nets - 1 else (p(f"W{i}_{l}"), p(f"z{i}_{l}"))
                    arr[i].g_weights[l] = p(f"gw{i}_{l}")
                arr[i].out = None if null == "out" and i == nets - 1 else p(f"out{i}")
                arr[i].g_out, arr[i].g_x = p(f"g{i}"), p(f"gx{i}")
            f = lib.e3k_mlp_hidden_fwd_multi if fn == "e3k_mlp_hidden_fwd_multi" else lib.e3k_mlp_hidden_bwd_multi
            rc = f(arr, o.get("nets", nets), *args, al, o.get("act", 2), 1.5, st)
    elif fn.startswith("e3k_slope"):
        nets, nh, R, H, k0, null = 2, o.get("nh", 2), o.get("R", 6), o.get("H", 32), o.get("k0", 8), o.get("null")
        one = lambda name, n: ar.alloc(name, n, np.ones(n, f32), align=2)
        one("r", 8), one("w", 64), one("acc", 2 * 2 * (4 * 4 * 8 * 64 + 8 * 64))
        for i in range(nets):
            for l in range(4):
                one(f"W{i}_{l}", 64 * 64), one(f"gw{i}_{l}", 64 * 64)
            one(f"hp{i}", 8 * 64), one(f"g{i}", 8 * 64)
        one("gb", 64)
        ar.upload(dev)
        p, nn = ar.p, max(o.get("nets", nets), nets)
        q = lambda k: None if null == k else p(k)
        Wp = None if null == "W" else _vp([None if null == "W01" and (i, l) == (0, 1) else p(f"W{i % 2}_{l}") for i in range(nn) for l in range(4)])
        io = lambda k: None if null == "io" else _vp([None if null == "io1" and i == 1 else p(f"{k}{i % 2}") for i in range(nn)])
        al = None if null == "alphas" else (C.c_float * 4)(0.5, 0.5, 0.5, 0.5)
        common = (Wp, o.get("nets", nets), nh, al, q("r"), R, q("w"), k0, H, 4.0, o.get("r_min", 0.0), 6.0, 1, o.get("cut", 0), o.get("act", 2), 1.5)
        if fn == "e3k_slope_tangent_fwd":
            rc = lib.e3k_slope_tangent_fwd(*common, io("hp"), st)
        else:
            gh = None if null == "gh" else _vp([p(f"gw{i % 2}_{l}") for i in range(nn) for l in range(4)])
            rc = lib.e3k_slope_tangent_bwd(*common, io("g"), q("acc"), gh, p("gb"), st)
    elif fn == "e3k_sq_error":
        n, null = 40, o.get("null")
        for k in ("pred", "target", "w", "grad"):
            ar.alloc(k, n, np.ones(n, f32))
        ar.alloc("loss", 1, f32(1)).upload(dev)
        q = lambda k: None if null == k else ar.p(k)
        rc = lib.e3k_sq_error(q("pred"), q("target"), ar.p("w"), o.get("w_group", 2), o.get("n", n), 0.5, q("loss"), q("grad"), st)
    else:
        assert fn == "e3k_adam_ema_step"
        cc = dict(c, n=37, ema=True)
        inp = adam_inputs(cc)
        inp["g"] = np.ones(37, f32)
        n = cc["n"]
        for k in ("p", "g", "m", "v", "ema"):
            ar.alloc(k, n, inp[k], align=4, shift=1 if o.get("shift") == k else 0)
        ar.alloc("state", 16, inp["state"]).upload(dev)
        hp = adam_hp(cc, max_norm=_f(1.0), **{k: _f(v) for k, v in o.items() if k in ("b1", "lr", "decay")})
        rc = _adam_call(cc, hp, ar, L, n=o.get("n"), state=o.get("null") != "state")
    assert rc == c["rc"], f"return code {rc}"
    Check(ar, c).finish()


def run_slope(dev, c, L):
    lib, st = L.load(), L.stream_ptr()
    inp, R, H, k0, nh, nets = slope_inputs(c), c["R"], c["H"], c["k0"], c["nh"], c["nets"]
    prm = inp["prm"]
    ar = _arena(c)
    ar.alloc("r", R, inp["r"], align=1).alloc("w", k0, inp["w"], align=1)
    for i in range(nets):
        for l in range(nh):
            ar.alloc(f"W{i}_{l}", inp["W"][i][l].size, inp["W"][i][l], align=1)
            ar.alloc(f"gw{i}_{l}", inp["old"][i][l].size, inp["old"][i][l], align=1)
        ar.alloc(f"hp{i}", R * H, align=1).alloc(f"g{i}", R * H, inp["g_hp"][i], align=1)
    n_acc = lib.e3k_slope_tangent_bwd_scratch(nets, nh, k0, H, R)
    per_net = sum(2 * R * (k0 if l == 0 else H) + 2 * R * H for l in range(nh)) + R * k0
    assert n_acc == nets * per_net
    ar.alloc("acc", 2 * n_acc, align=2).alloc("gb", k0, inp["old_b"], align=1).upload(dev)
    p = ar.p
    al = (C.c_float * nh)(*inp["alphas"])
    Wp = _vp([p(f"W{i}_{l}") if l < nh else None for i in range(nets) for l in range(4)])
    common = (Wp, nets, nh, al, p("r"), R, p("w"), k0, H, prm["r_max"], prm["r_min"], prm["p"], prm["oor"], prm["cut"], c["act"], inp["cst"])
    null = set(c["null_gh"])
    assert lib.e3k_slope_tangent_fwd(*common, _vp([p(f"hp{i}") for i in range(nets)]), st) == E3K_OK
    if c["op"] == "both":
        gh = _vp([p(f"gw{i}_{l}") if l < nh and (i, l) not in null else None for i in range(nets) for l in range(4)])
        assert lib.e3k_slope_tangent_bwd(*common, _vp([p(f"g{i}") for i in range(nets)]), p("acc"), gh, p("gb") if c["gb"] else None, st) == E3K_OK
    ck, ref = Check(ar, c), slope_reference(c, inp)
    for i in range(nets):
        ck.close(f"hp{i}", ref["hp"][i][0], ref["hp"][i][1], "slope_hp")
    if c["op"] == "both":
        ck.free("acc", 2 * n_acc)
        for (i, l), (want, bound, _) in ref["gw"].items():
            if (i, l) not in null:
                ck.close(f"gw{i}_{l}", want, bound, "slope_g_hidden")
        if c["gb"]:
            ck.close("gb", ref["gb"][0], ref["gb"][1], "slope_g_bessel")
    ck.finish()


RUNNERS = dict(slope=run_slope, mlp=run_mlp, sq=run_sq, adam=run_adam, adam_pair=run_adam_pair, refuse=run_refuse)


@pytest.mark.parametrize("c", CASES, ids=[c["id"] for c in CASES])
def test_train_case_against_float64(dev, c):
    from e3_layers_amd.backend import lib as L

    RUNNERS[c["kind"]](dev, c, L)


def test_zz_worst_ratio_per_family(dev):
    """prints what the cases of this run measured (the module's MEASURED is a copy of a full run's)"""
    for family in sorted(WORST):
        print(f"worst error / bound, {family}: {WORST[family]:.3f}")
    assert all(r <= 1.0 for r in WORST.values())
