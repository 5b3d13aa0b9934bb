"""The kernels of csrc/e3k_mlp.hip, csrc/e3k_slope.hip and csrc/e3k_optim.hip that the library ships == the kernels the cases of
tests/test_gpu_train_matrix.py name (no GPU needed); the functions of the three header sections == the functions the cases call; and
the bounds of that file shown on the CPU to hold for models of the kernels' arithmetic and to be sharp.

Models, operation for operation: numpy float32 for adam_ema_kernel, the ticks and sq_error_kernel (an FMA is a float64 product and
sum rounded once); numpy float64 for the slope chain with its fp32 casts and its eight-range partial sums, and the same formulas in
np.longdouble, which every float64 allowance F64 of the slope reference must cover; numpy float32 matrix products for the MLP.

Planted mutants.  Each is a model with one error of the kind the kernels have had or could have; each must leave its case's own bound.
Worst error / bound per mutant (the assertion is > 1; MUTANT_FLOOR holds the values of the current run):
    adam: tail not updated 8.7e4, m written on a skipped step inf (bits moved), bias correction at t - 1 1.3e7, EMA decay off by one
    in k 2.5e6, weight decay before the clip scale 2.8e5, EMA from the old p 9.9e5, eps under the root 2.8e6; sq_error weight
    indexed by i 1e38 (entries of weight 0); mlp weight-gradient rows k >= 32 dropped 8.0e4 (the smallest of all), dgrad without
    alpha 7.2e5; slope: first 32 frequencies only 1.7e6 (k0 = 48) and 1.4e7 (k0 = 64), d2 dropped 1.2e7, last odd row dropped inf
    (NaN in hp) and 5.2e6 (gradients), last row range dropped 3.1e6, alpha once 4.6e7, delta = r_max 8.4e12, cutoffs swapped 2.5e7.
None is below 10.  Three needed a case chosen for them: "eps under the root" moves p by less than an ulp unless v is tiny
(adam_eps_placement plants v = 0, g = 0, m != 0, where the denominator is eps alone); a dropped last row or last row range is silent
when that row sits at r_max, as the last knot rows do (planted on slope_R1 and slope_gb_null, whose last rows are inside).
What the earlier NORMWISE tests would have let through: test_fused_adam_ema_matches_torch and
test_slope_table_is_the_derivative_of_the_radial_mlp (tests/test_gpu_ops.py) are rebuilt below on the CPU -- their sizes, the padded
flat buffer, the lo:hi window, their tolerances and rel_err -- with the kernels replaced by these models, and every Adam and slope
mutant is applied there.  Let through (LET_THROUGH, asserted): the Adam tail (the padded buffer has none), m written on a skipped step
(no skip in the test), weight decay before the clip scale (never both in one configuration), the last odd row (it sits at r_max,
outside the window), delta = r_max (r_min = 0); and k0 = 64 has no counterpart there.  The other nine are caught there too.
"""
import os
import re
import subprocess

import numpy as np

import tests.test_gpu_train_matrix as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "equivariant-nn-zoo_amd", "csrc")
HEADER = os.path.join(ROOT, "include", "e3k.h")
LLVM = "/opt/rocm/llvm/bin"
f32, f64 = np.float32, np.float64
BY_ID = {c["id"]: c for c in T.CASES}

OBJECTS = {"e3k_mlp.o": ("mlp_", 10), "e3k_slope.o": ("slope_", 3), "e3k_optim.o": ("", 7)}
SECTIONS = {r"e3k_mlp_\w+": 5, r"e3k_slope_tangent_\w+": 3, r"e3k_sq_error|e3k_adam_ema_step": 2}


def _tool(name):
    path = os.path.join(LLVM, name)
    return path if os.path.exists(path) else name


def _shipped_kernels(tmp_path, obj):
    """the kernels of the gfx950 bundle of one object, template arguments kept: e3k::mlp_hidden_bwd_kernel<3>"""
    path = os.path.join(CSRC, obj)
    if not os.path.exists(path):
        import __graft_entry__

        __graft_entry__.build()
    work = tmp_path / obj
    work.mkdir()
    # --offloading writes one file per bundle beside the object it reads: a link to it in tmp_path keeps them out of the tree
    os.symlink(path, work / obj)
    subprocess.run([_tool("llvm-objdump"), "--offloading", obj], check=True, cwd=work, capture_output=True)
    bundles = [p for p in os.listdir(work) if p.endswith("gfx950")]
    assert len(bundles) == 1, os.listdir(work)
    syms = subprocess.run([_tool("llvm-readelf"), "-sW", str(work / bundles[0])], check=True, capture_output=True, text=True).stdout
    names = [f[7] for f in (line.split() for line in syms.splitlines()) if len(f) >= 8 and f[3] == "FUNC" and f[4] == "GLOBAL"]
    demangled = subprocess.run(["c++filt"], input="\n".join(names), check=True, capture_output=True, text=True).stdout
    return {m.group(1) for m in re.finditer(r"e3k::(\w+_kernel(?:<[^>]*>)?)\(", demangled)}


def test_every_training_kernel_has_a_float64_checked_case(tmp_path):
    table = T.table_kernels()
    shipped = set()
    for obj, (prefix, count) in OBJECTS.items():
        k = _shipped_kernels(tmp_path, obj) - {"zero_words_kernel"}      # (e3k_common.h's helper, instantiated in every object)
        assert len(k) == count and all(n.startswith(prefix) for n in k), (obj, sorted(k))
        shipped |= k
    assert shipped - table == set(), f"kernels without a case in test_gpu_train_matrix.CASES: {sorted(shipped - table)}"
    assert table - shipped == set(), f"the case table names kernels the library does not ship: {sorted(table - shipped)}"


def test_every_function_of_the_three_header_sections_is_called_by_a_case():
    with open(HEADER) as f:
        text = f.read()
    declared = set()
    for pattern, count in SECTIONS.items():
        found = set(re.findall(r"\b(" + pattern + r")\s*\(", text))
        assert len(found) == count, (pattern, sorted(found))
        declared |= found
    called = T.table_functions()
    assert declared - called == set(), f"declared in include/e3k.h, called by no case: {sorted(declared - called)}"
    assert called - declared == set(), f"cases call functions the header does not declare: {sorted(called - declared)}"


def test_case_ids_are_unique_and_the_issue_values_all_appear():
    ids = [c["id"] for c in T.CASES]
    assert len(ids) == len(set(ids))
    assert all(c["why"] and "kernels" in c and "funcs" in c for c in T.CASES)
    sl = [c for c in T.CASES if c["kind"] == "slope"]
    for key, values in (("R", {1, 2, 3, 17, 37, 129, 641}), ("H", {32, 64}), ("k0", {1, 8, 31, 32, 33, 48, 64}), ("nh", {1, 2, 3, 4}),
                        ("act", {0, 1, 2, 4}), ("nets", {1, 5, 16}), ("r_min", {0.0, 0.5}), ("p", {6.0, 2.5}), ("radii", {"knots", "knots_inside", "random"})):
        assert {c[key] for c in sl} == values, key
    assert {(c["cut"], c["oor"]) for c in sl} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    assert any(c["sat"] for c in sl) and any(c["null_gh"] for c in sl) and any(not c["gb"] for c in sl)
    ml = [c for c in T.CASES if c["kind"] == "mlp"]
    for s in T.MLP_NEW:
        tiles = {T.mlp_tile(c["rows"], min(c["nets"], 8)) for c in ml if (c["k0"], c["h"], c["nl"], c["act"]) == s}
        assert tiles == {16, 64}, s
    assert {c["n"] for c in T.CASES if c["kind"] == "adam"} >= {1, 2, 3, 4, 5, 7, 1027, 524288 + 5, 2097152 + 7}
    assert {c["n"] for c in T.CASES if c["kind"] == "sq"} >= {1, 63, 64, 65, 1023, 1024, 1025, 5000}


# ---------------------------------------------------------------------------------------------------------------------------------
# float32 models
def _fma32(a, b, c):
    return (np.asarray(a, f64) * np.asarray(b, f64) + np.asarray(c, f64)).astype(f32)


def adam_model32(p, g, m, v, ema, sw, hp, n_body=None, mutant=None):
    """adam_ema_kernel in numpy float32 from the state words sw; n_body: elements the update reaches (mutant: the tail is not)"""
    lr, b1, b2, eps, wd = (f32(hp[k]) for k in ("lr", "b1", "b2", "eps", "wd"))
    skip = sw[6] != 0
    step, isb = lr / f32(sw[1]), f32(1.0 / np.sqrt(f64(sw[2])))
    p1, m1, v1 = p.copy(), m.copy(), v.copy()
    if not skip or mutant == "m_on_skipped_step":
        if mutant == "wd_before_clip":
            gv = (_fma32(wd, p, g) if wd != 0 else g) * f32(sw[4])
        else:
            gv = g * f32(sw[4])
            if wd != 0:
                gv = _fma32(wd, p, gv)
        m1 = _fma32(b1, m, (f32(1) - b1) * gv)
    if not skip:
        v1 = _fma32(b2, v, (f32(1) - b2) * gv * gv)
        den = np.sqrt(v1 + eps) * isb if mutant == "eps_under_root" else np.sqrt(v1) * isb + eps
        p1 = p - step * (m1 / den)
    e1 = None
    if ema is not None:
        omd = f32(1) - f32(sw[9])
        e1 = ema - omd * (ema - (p if mutant == "ema_from_old_p" else p1))
    if mutant == "tail_not_updated":
        nb = len(p) & ~3
        p1[nb:], m1[nb:], v1[nb:] = p[nb:], m[nb:], v[nb:]
        if e1 is not None:
            e1[nb:] = ema[nb:]
    return dict(p=p1, m=m1, v=v1, ema=e1)


def tick_model32(sw, g, hp, mutant=None):
    """sumsq_kernel (one float32 chain) + tick_kernel (+ ema_tick_kernel) in numpy float32"""
    s = sw.copy()
    have_norm = hp["max_norm"] > 0 or bool(hp["skip"])
    with np.errstate(over="ignore", invalid="ignore"):
        ssq = f32(np.sum(g.astype(f32) ** 2, dtype=f32)) if have_norm else f32(0)
    bad = have_norm and not np.isfinite(ssq)
    skip = bool(hp["skip"]) and bad
    s[6], s[5] = (1.0 if skip else 0.0), 0.0
    s[0] = s[0] + (0 if skip else 1)
    t = max(float(s[0]), 1.0) - (1.0 if mutant == "bias_t_minus_1" else 0.0)
    s[1], s[2] = f32(1.0 - f64(hp["b1"]) ** t), f32(1.0 - f64(hp["b2"]) ** t)
    with np.errstate(invalid="ignore"):
        norm = np.sqrt(ssq) if have_norm else f32(0)
    s[7], s[4] = norm, 1.0
    if hp["max_norm"] > 0 and have_norm and not bad:
        cq = f32(hp["max_norm"]) / (norm + f32(1e-6))
        s[4] = cq if cq < 1 else 1.0
    if hp["ema"]:
        s[8] = s[8] + 1
        d = f32(hp["decay"])
        if hp["use_num"]:
            k = s[8] - f32(1) if mutant == "ema_k_off_by_one" else s[8]
            alt = (f32(1) + k) / (f32(10) + k)
            d = min(alt, d)
        s[9] = d
    return s


def _state_ratio(got, ref):
    worst = 0.0
    for w, r in ref.items():
        gv = float(got[w])
        if r[0] == "exact":
            worst = max(worst, 0.0 if gv == r[1] else np.inf)
        elif r[0] == "nan":
            worst = max(worst, 0.0 if np.isnan(gv) else np.inf)
        elif r[0] == "ulp":
            worst = max(worst, abs(gv - r[1]) / T._ulp32(r[1]))
        else:
            worst = max(worst, abs(gv - r[1]) / r[2] if r[2] > 0 else (0.0 if gv == r[1] else np.inf))
    return worst


def _ratio(got, want, bound, key=None):
    err = np.abs(np.asarray(got, f64) - want)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err == 0, 0.0, np.inf))
    return float(np.nanmax(np.where(np.isnan(err), np.inf, r))) if r.size else 0.0


def _adam_walk(c, model_mutant=None, ref_mutant=None, tick_mutant=None):
    """three steps of a case through the float32 models: worst error / bound per output against the case's own references.
    ref_mutant / tick_mutant: the model computes the mutated formula (its float64 value, rounded)"""
    inp, hp = T.adam_inputs(c), T.adam_hp(c)
    cur = {k: inp[k].copy() for k in ("p", "m", "v", "ema")}
    if not c["ema"]:
        cur["ema"] = None
    sw = inp["state"].copy()
    worst = {}
    for step in range(3):
        g = T.adam_grad(c, step)
        ref_t = T.tick_reference(sw, g, hp)
        sw1 = tick_model32(sw, g, hp)
        if tick_mutant:
            for w, r in T.tick_reference(sw, g, hp, mutant=tick_mutant).items():
                if r[0] in ("ulp", "close"):
                    sw1[w] = f32(r[1])
        worst["state"] = max(worst.get("state", 0.0), _state_ratio(sw1, ref_t))
        assert all(sw1[w] == T.SENTINEL for w in T.KEEP_WORDS)
        ref = T.adam_reference(cur["p"], g, cur["m"], cur["v"], cur["ema"], sw1, hp)
        if ref_mutant:
            out = {k: w.astype(f32) for k, (w, _) in T.adam_reference(cur["p"], g, cur["m"], cur["v"], cur["ema"], sw1, hp, mutant=ref_mutant).items()}
        else:
            with np.errstate(invalid="ignore", over="ignore"):
                out = adam_model32(cur["p"], g, cur["m"], cur["v"], cur["ema"], sw1, hp, mutant=model_mutant)
        for k in ("p", "m", "v", "ema"):
            if cur[k] is None:
                continue
            if k in ref:
                worst[k] = max(worst.get(k, 0.0), _ratio(out[k], *ref[k], key=k))
            else:      # a skipped step: the bits stay
                worst[k] = max(worst.get(k, 0.0), 0.0 if np.array_equal(out[k], cur[k]) else np.inf)
        # the walk goes on from the unmutated model, as the device would
        good = adam_model32(cur["p"], g, cur["m"], cur["v"], cur["ema"], tick_model32(sw, g, hp), hp) if (model_mutant or ref_mutant or tick_mutant) else out
        cur, sw = {k: good[k] for k in cur}, tick_model32(sw, g, hp)
    return worst


def sq_model32(c, inp, mutant=None):
    n, scale = c["n"], f32(c["scale"])
    d = inp["pred"] - inp["target"]
    if inp["w"] is None:
        wi = np.full(n, f32(1) / f32(n), f32)
    else:
        wi = inp["w"][np.minimum(np.arange(n) if mutant == "weight_by_i" else np.arange(n) // c["w_group"], len(inp["w"]) - 1)]
    grad = f32(2) * scale * wi * d
    acc = np.zeros(1024, f32)
    for lo in range(0, n, 1024):      # thread t strides by 1024
        k = min(1024, n - lo)
        acc[:k] = _fma32(wi[lo:lo + k] * d[lo:lo + k], d[lo:lo + k], acc[:k])
    part = acc.reshape(16, 64)
    for off in (32, 16, 8, 4, 2, 1):
        part = np.concatenate([part[:, :64 - off] + part[:, off:], part[:, 64 - off:]], 1)
    s = f32(0)
    for k in range(16):
        s = s + part[k, 0]
    return dict(grad=grad, loss=np.array([scale * s], f32))


def _act32(a, x):
    with np.errstate(over="ignore"):
        s = f32(1) / (f32(1) + np.exp(-x))
        if a == 1:
            return (np.maximum(x, 0) + np.log(f32(1) + np.exp(-np.abs(x))) - f32(0.6931471805599453)).astype(f32), s
        if a == 2:
            return x * s, s * (f32(1) + x * (f32(1) - s))
        if a == 4:
            return np.tanh(x), f32(1) - np.tanh(x) ** 2
    return (np.abs(x), np.sign(x)) if a == 5 else (x, np.ones_like(x))


def mlp_model32(c, inp, i, mutant=None):
    """the hidden chain in numpy float32 (its matrix products sum in float32 in an order of their own)"""
    x, Ws, al, cst, a = inp["x"], inp["W"][i], [f32(v) for v in inp["alphas"]], f32(inp["cst"]), c["act"]
    prev, zs = x, []
    for W, q in zip(Ws, al):
        zs.append(q * (prev @ W))
        prev = cst * _act32(a, zs[-1])[0]
    g, gws = inp["g"][i], [None] * len(Ws)
    for l in range(len(Ws) - 1, -1, -1):
        gz = g * (cst * _act32(a, zs[l])[1])
        H = cst * _act32(a, zs[l - 1])[0] if l > 0 else x
        gw = al[l] * (H.T @ gz)
        if mutant == "wgrad_rows_32_dropped":
            gw[32:] = 0
        gws[l] = inp["old"][i][l] + gw
        g = (gz @ Ws[l].T) if mutant == "dgrad_without_alpha" else al[l] * (gz @ Ws[l].T)
    return zs, prev, gws, g


def _mlp_walk(c, mutant=None):
    inp = T.mlp_inputs(c)
    zs32, out32, gws32, gx32 = mlp_model32(c, inp, 0, mutant)
    zs, dzs, out, dout = T.mlp_forward(c, inp, 0)
    worst = dict(z=max(_ratio(a, b, d) for a, b, d in zip(zs32, zs, dzs)), out=_ratio(out32, out, dout))
    z_good = mlp_model32(c, inp, 0)[0]
    gws, (gx, dgx) = T.mlp_backward(c, inp, 0, z_good)
    worst["g_w"] = max(_ratio(a, *b, key="g_w") for a, b in zip(gws32, gws))
    worst["g_x"] = _ratio(gx32, gx, dgx, key="g_x")
    return worst


def _slope_walk(c, dt=f64, mutant=None):
    """the slope model at precision dt against the case's reference: float64 + fp32 casts against the bounds; longdouble against F64"""
    inp = T.slope_inputs(c)
    ref = T.slope_reference(c, inp)
    worst, gb_sum = dict(hp=0.0, g_hidden=0.0, g_bessel=0.0), 0
    col = 2 if dt is np.longdouble else 1
    for i in range(c["nets"]):
        lv, bw, dbw = T.slope_plain_forward(inp["r"], inp["w"], inp["W"][i], inp["alphas"], inp["cst"], inp["prm"], c["act"], dt, mutant)
        hp = lv[-1]["da"]
        if mutant == "last_odd_row_dropped" and c["R"] % 2:
            hp = hp.copy()
            hp[-1] = np.nan      # never written
        got = hp.astype(f32).astype(f64) if dt is f64 else (hp - ref["hp"][i][0]).astype(f64) + ref["hp"][i][0]
        worst["hp"] = max(worst["hp"], _ratio(got, ref["hp"][i][0], ref["hp"][i][col], key="hp"))
        if c["op"] != "both":
            continue
        parts, gb = T.slope_plain_backward(lv, bw, dbw, inp["W"][i], inp["cst"], inp["g_hp"][i], dt, mutant)
        gb_sum = gb_sum + gb
        for l in range(c["nh"]):
            want = ref["gw"][(i, l)][0]
            if dt is f64:
                acc = inp["old"][i][l].copy()
                for P in parts[l]:
                    acc = (acc + P.astype(f32)).astype(f32)
                got = acc.astype(f64)
            else:
                got = (inp["old"][i][l].astype(dt) + sum(parts[l]) - want).astype(f64) + want
            worst["g_hidden"] = max(worst["g_hidden"], _ratio(got, want, ref["gw"][(i, l)][col], key="g_hidden"))
    if c["op"] == "both":
        want = ref["gb"][0]
        if mutant == "bessel_first_32":
            gb_sum = np.where(np.arange(c["k0"]) < 32, gb_sum, 0)
        if dt is f64:
            got = (inp["old_b"] + np.asarray(gb_sum, f64).astype(f32)).astype(f32).astype(f64)
        else:
            got = (inp["old_b"].astype(dt) + gb_sum - want).astype(f64) + want
        worst["g_bessel"] = _ratio(got, want, ref["gb"][col], key="g_bessel")
    return worst, T.slope_f64_share(c, ref)


# ---------------------------------------------------------------------------------------------------------------------------------
def test_optimiser_bounds_hold_for_float32_models_and_are_sharp():
    """every Adam and squared-error case through the float32 models: inside the bounds, and the elementwise families come near them:
    measured p 0.994, m 0.955, v 0.989, ema 0.991, sq_error gradient 0.832 (the loss, an order-independent sum, 0.147); the floors
    are set just under those, so a bound loosened by a fifth fails here"""
    FLOOR = dict(p=0.9, m=0.9, v=0.9, ema=0.9, sq_grad=0.8)
    top = {}
    for c in T.CASES:
        if c["kind"] == "adam" and c["n"] <= 1027:
            for k, r in _adam_walk(c).items():
                assert r <= 1.0, (c["id"], k, r)
                top[k] = max(top.get(k, 0.0), r)
        elif c["kind"] == "sq":
            inp = T.sq_inputs(c)
            got, ref = sq_model32(c, inp), T.sq_reference(c, inp)
            for k in ("grad", "loss"):
                r = _ratio(got[k], *ref[k])
                assert r <= 1.0, (c["id"], k, r)
                top["sq_" + k] = max(top.get("sq_" + k, 0.0), r)
    print({k: round(v, 3) for k, v in top.items()})
    for k, floor in FLOOR.items():
        assert top[k] > floor, (k, top[k])


def test_mlp_bounds_hold_for_a_float32_model_at_the_new_shapes():
    """numpy float32 matrix products through the chain: inside the bounds of tests/test_gpu_node_passes.py at the new shapes; measured
    z 0.369, out 0.199, g_w 0.106, g_x 0.036 (bounds over K + 3, R + 4 and h + 3 roundings in any order are not attained by sums of
    random signs); the floor on z, the one nearest its bound, keeps the model and the bound from drifting apart unnoticed"""
    top = {}
    for c in T.CASES:
        if c["kind"] == "mlp" and c["op"] == "both" and not c["exact"] and c["rows"] <= 1984 and c["gw"] == "all" and c["gx"]:
            for k, r in _mlp_walk(c).items():
                assert r <= 1.0, (c["id"], k, r)
                top[k] = max(top.get(k, 0.0), r)
    print({k: round(v, 3) for k, v in top.items()})
    assert top["z"] > 0.3, top


def test_slope_bounds_hold_for_the_float64_model_and_f64_covers_longdouble():
    """float64 model + fp32 casts inside the bounds and near them (hp: one rounding, measured 0.88 .. 1.00 per case; g_hidden 0.25 ..
    0.65); the same formulas in np.longdouble within F64 of the reference values (measured below 0.25 of it); and the condition on F64: below 1 % of the fp32
    term on at least 99 % of the elements of hp, on every case"""
    for c in T.CASES:
        if c["kind"] != "slope":
            continue
        w64, share = _slope_walk(c)
        wl, _ = _slope_walk(c, np.longdouble)
        print(c["id"], {k: round(v, 3) for k, v in w64.items()}, {k: round(v, 4) for k, v in wl.items()}, f"F64 < 1 %: {share:.4f}")
        assert all(r <= 1.0 for r in w64.values()) and all(r <= 1.0 for r in wl.values()), c["id"]
        assert w64["hp"] > 0.8 and (c["op"] == "fwd" or w64["g_hidden"] > 0.2), c["id"]
        assert share >= 0.99, (c["id"], share)


def test_the_explicit_reverse_sweep_is_the_autograd_of_the_tangent():
    """<g_hp, H'> differentiated by torch float64 autograd (H' itself by a Jacobian-vector product of the chain in r) == the explicit
    reverse sweep of the reference, for the weights of every layer and the Bessel frequencies"""
    import torch

    for cid in ("slope_R37_nets5", "slope_R17", "slope_sat_ssp"):
        c = BY_ID[cid]
        inp = T.slope_inputs(c)
        prm = inp["prm"]
        from tests.test_gpu_edge_matrix import rad_formula

        r = torch.from_numpy(inp["r"].astype(f64))
        w = torch.from_numpy(inp["w"].astype(f64)).requires_grad_(True)
        Ws = [torch.from_numpy(W.astype(f64)).requires_grad_(True) for W in inp["W"][0]]
        act = {0: lambda x: x, 1: lambda x: x.clamp(min=0) + torch.log1p(torch.exp(-x.abs())) - np.log(2.0), 2: torch.nn.functional.silu, 4: torch.tanh}[c["act"]]

        def chain(rr):
            a = rad_formula(rr[:, None].expand(len(rr), len(w)), w[None, :].expand(len(rr), len(w)), prm)
            for W, al in zip(Ws, inp["alphas"]):
                a = inp["cst"] * act(al * (a @ W))
            return a

        _, hp = torch.autograd.functional.jvp(chain, r, torch.ones_like(r), create_graph=True)
        grads = torch.autograd.grad((hp * torch.from_numpy(inp["g_hp"][0].astype(f64))).sum(), Ws + [w])
        ref = T.slope_reference(dict(c, nets=1, prefill=False), dict(inp, old=[[np.zeros_like(o) for o in inp["old"][0]]], old_b=np.zeros_like(inp["old_b"])))
        assert np.abs(hp.detach().numpy() - ref["hp"][0][0]).max() <= 1e-11 * np.abs(ref["hp"][0][0]).max()
        for l in range(c["nh"]):
            want = ref["gw"][(0, l)][0]
            assert np.abs(grads[l].numpy() - want).max() <= 1e-10 * np.abs(want).max(), (cid, l)
        want = ref["gb"][0]
        assert np.abs(grads[-1].numpy() - want).max() <= 1e-10 * np.abs(want).max(), cid


MUTANT_FLOOR = {}      # filled by the test below


def test_planted_mutants_leave_their_bounds():
    """every mutant's worst error / bound on its case: all > 1 (the measured values are in the module docstring)"""
    found = {}
    for name, cid, kw, key in (
            ("adam tail not updated", "adam_ema_clip_bites", dict(model_mutant="tail_not_updated"), "p"),
            ("adam m written on a skipped step", "adam_skip_nan_tail", dict(model_mutant="m_on_skipped_step"), "m"),
            ("adam bias correction at t - 1", "adam_ema_clip_bites", dict(tick_mutant="bias_t_minus_1"), "state"),
            ("adam EMA decay off by one in k", "adam_ema", dict(tick_mutant="ema_k_off_by_one"), "state"),
            ("adam weight decay before the clip scale", "adam_ema_clip_bites", dict(ref_mutant="wd_before_clip"), "p"),
            ("adam EMA from the old p", "adam_ema_clip_bites", dict(ref_mutant="ema_from_old_p"), "ema"),
            ("adam eps under the root", "adam_eps_placement", dict(ref_mutant="eps_under_root"), "p")):
        found[name] = _adam_walk(BY_ID[cid], **kw)[key]
    c = BY_ID["sq_weight_group3"]
    inp = T.sq_inputs(c)
    found["sq_error weight indexed by i"] = _ratio(sq_model32(c, inp, "weight_by_i")["grad"], *T.sq_reference(c, inp)["grad"])
    found["mlp weight-gradient rows k >= 32 dropped"] = _mlp_walk(BY_ID["mlp_gw_accumulate"], "wgrad_rows_32_dropped")["g_w"]
    found["mlp dgrad without alpha"] = _mlp_walk(BY_ID["mlp_rows17"], "dgrad_without_alpha")["g_x"]
    for name, cid, mutant, key in (
            ("slope Bessel level sums the first 32 frequencies only", "slope_R129_k48", "bessel_first_32", "g_bessel"),
            ("slope Bessel level sums the first 32 frequencies only (k0 = 64)", "slope_R129_k64", "bessel_first_32", "g_bessel"),
            ("slope d2 term dropped from gz", "slope_R37_nets5", "no_d2", "g_hidden"),
            ("slope last odd row dropped", "slope_R37_nets5", "last_odd_row_dropped", "hp"),
            ("slope last odd row dropped (gradients)", "slope_R1", "last_odd_row_dropped", "g_hidden"),
            ("slope last row range of the split dropped", "slope_gb_null", "last_range_dropped", "g_hidden"),
            ("slope alpha applied once in gz", "slope_sat_ssp", "alpha_once", "g_hidden"),
            ("slope delta = r_max", "slope_R17", "delta_is_r_max", "hp"),
            ("slope cutoff kinds swapped", "slope_R3", "cutoff_swapped", "hp")):
        found[name] = _slope_walk(BY_ID[cid], mutant=mutant)[0][key]
    for name, r in found.items():
        print(f"mutant {name}: error / bound {r:.3g}")
    MUTANT_FLOOR.update(found)
    quiet = {k: v for k, v in found.items() if not v > 1.0}
    assert not quiet, quiet


# ---------------------------------------------------------------------------------------------------------------------------------
# the two earlier NORMWISE tests rebuilt on the CPU: their sizes, windows, tolerances and rel_err formula, the kernels replaced by the
# models above
def _rel_err(a, b):
    a, b = np.asarray(a, f64), np.asarray(b, f64)
    if not np.isfinite(a).all():
        return np.inf
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


OLD_ADAM_CONFIGS = ((None, None, 0.0), (0.999, 0.5, 0.0), (0.99, None, 0.01))      # (ema, clip, wd) of test_fused_adam_ema_matches_torch
OLD_ADAM_SIZES = (64 * 33, 7, 1000, 5 * 5 * 3)


def old_adam_test(ema, clip, wd, model_mutant=None, tick_mutant=None):
    """tests/test_gpu_ops.py::test_fused_adam_ema_matches_torch on the CPU: four parameters in FusedAdamEMA's flat buffer (every slice
    padded to 64 floats, the padding zero: 3328 floats, no tail), lr 1e-2, 12 steps of gradients 0.1 N(0, 1) (3 N(0, 1) every fourth),
    float64 Adam + EMA as the reference; returns the worst rel_err over the parameters and their EMA shadows (the test asks < 1e-5)"""
    rng = np.random.default_rng(13)
    offs, total = [], 0
    for n in OLD_ADAM_SIZES:
        offs.append(total)
        total += -(-n // 64) * 64
    assert total == 3328 and total % 4 == 0
    live = np.zeros(total, bool)
    for o, n in zip(offs, OLD_ADAM_SIZES):
        live[o:o + n] = True
    p = np.where(live, rng.standard_normal(total), 0.0).astype(f32)
    hp = dict(lr=T._f(1e-2), b1=T._f(0.9), b2=T._f(0.999), eps=T._f(1e-8), wd=T._f(wd), decay=T._f(ema or 0.0), use_num=1,
              max_norm=T._f(clip or 0.0), skip=0, ema=ema is not None)
    cur = dict(p=p.copy(), m=np.zeros(total, f32), v=np.zeros(total, f32), ema=p.copy() if ema is not None else None)
    sw = np.zeros(16, f32)
    rp, rm, rv, rs = p.astype(f64), np.zeros(total), np.zeros(total), p.astype(f64)
    for k in range(1, 13):
        g = np.where(live, rng.standard_normal(total) * (3.0 if k % 4 == 0 else 0.1), 0.0).astype(f32)
        gg = g.astype(f64)
        if clip is not None:
            coef = clip / (np.linalg.norm(gg) + 1e-6)
            gg = gg * min(coef, 1.0)
        gg = gg + wd * rp
        rm, rv = 0.9 * rm + 0.1 * gg, 0.999 * rv + 0.001 * gg * gg
        rp = rp - 1e-2 / (1 - 0.9 ** k) * rm / (np.sqrt(rv) / np.sqrt(1 - 0.999 ** k) + 1e-8)
        if ema is not None:
            d = min(ema, (1 + k) / (10 + k))
            rs = rs - (1 - d) * (rs - rp)
        with np.errstate(all="ignore"):
            sw = tick_model32(sw, g, hp, mutant=tick_mutant)
            cur = adam_model32(cur["p"], g, cur["m"], cur["v"], cur["ema"], sw, hp, mutant=model_mutant)
    worst = 0.0
    for o, n in zip(offs, OLD_ADAM_SIZES):
        worst = max(worst, _rel_err(cur["p"][o:o + n], rp[o:o + n]))
        if ema is not None:
            worst = max(worst, _rel_err(cur["ema"][o:o + n], rs[o:o + n]))
    return worst


def old_slope_test(n_basis, mutant=None):
    """tests/test_gpu_ops.py::test_slope_table_is_the_derivative_of_the_radial_mlp on the CPU: the 641 knots of r_max 5 (512 slope knots
    asked for), ssp, H = 64, three hidden layers, the polynomial cutoff with 1 / r, r_min 0, Bessel frequencies n pi; D = H' W_last
    / 8 against float64 on the rows lo:hi = 76:639 through a random combination of its columns (the test asks rel_err < 2e-6), and the
    gradients of <g_D, D> (g_D random on lo:hi, zero elsewhere) for the first hidden layer and the frequencies (< 5e-5).  The last
    layer's width, the plan's d_out in the test, is 192 here; its own gradient is a GEMM's.  Returns the three rel_err"""
    from e3_layers_amd.backend.radial_table import knot_radii, layout

    rng = np.random.default_rng(3 + n_basis)
    r = knot_radii(5.0, 512, "cpu").numpy()
    knots, spacing = layout(5.0, 512)
    assert len(r) == knots + 1 == 641
    lo, hi = int(0.6 / spacing), int(5.0 / spacing) - 1
    prm = dict(r_max=5.0, r_min=0.0, p=6.0, oor=1, cut=0)
    w = (np.arange(1, n_basis + 1) * np.pi).astype(f32)
    Ws = [rng.standard_normal((n_basis if l == 0 else 64, 64)).astype(f32) for l in range(3)]
    alphas, cst = [T._f(1.0 / np.sqrt(n_basis))] + [T._f(0.125)] * 2, T._f(1.679)
    Wl = rng.standard_normal((64, 192)).astype(f32).astype(f64) * 0.125
    cols = rng.standard_normal(192)
    gD = np.zeros((641, 192))
    gD[lo:hi] = rng.standard_normal((hi - lo, 192)).astype(f32)
    g_hp = (gD @ Wl.T).astype(f32)

    def run(mut):
        lv, bw, dbw = T.slope_plain_forward(r, w, Ws, alphas, cst, prm, 1, f64, mut)
        hp = lv[-1]["da"].astype(f32).astype(f64)
        if mut == "last_odd_row_dropped":
            hp[-1] = np.nan
        parts, gb = T.slope_plain_backward(lv, bw, dbw, Ws, cst, g_hp, f64, mut)
        if mut == "bessel_first_32":
            gb = np.where(np.arange(n_basis) < 32, gb, 0.0)
        return ((hp @ Wl) * cols).sum(1)[lo:hi], sum(parts[0]).astype(f32), np.asarray(gb, f64).astype(f32)

    good, got = run(None), run(mutant)
    return tuple(_rel_err(a, b) for a, b in zip(got, good))


# what the two earlier tests let through: (mutant, how it is applied); "identical" = their data cannot express it at all
LET_THROUGH = {
    "adam tail not updated": "identical: FusedAdamEMA pads every slice to 64 floats, n & 3 = 0",
    "adam m written on a skipped step": "identical: the test never sets skip_nonfinite (test_fused_adam_skips_nonfinite_gradient looks at p only)",
    "adam weight decay before the clip scale": "identical: no configuration has a clip and a weight decay together",
    "slope last odd row dropped": "identical on the window: row 640 sits at r_max, outside lo:hi, and carries no gradient",
    "slope delta = r_max": "identical: r_min = 0 in the test",
}
CAUGHT = ("adam bias correction at t - 1", "adam EMA decay off by one in k", "adam EMA from the old p", "adam eps under the root",
          "slope Bessel level sums the first 32 frequencies only", "slope d2 term dropped from gz", "slope last row range of the split dropped",
          "slope alpha applied once in gz", "slope cutoff kinds swapped")


def test_which_mutants_the_earlier_normwise_tests_let_through():
    """every Adam and slope mutant applied to the rebuilt data of the two earlier tests, under their tolerances (1e-5; 2e-6 and 5e-5):
    a mutant is let through when every configuration of the test still passes.  Five of sixteen are, each because the test's data
    cannot express it; a sixth, "first 32 frequencies only" at k0 = 64, has no counterpart there (the test stops at 48 frequencies, where
    it is caught: 0.63).  The sq_error and MLP mutants belong to element-wise tests already and are not part of this."""
    adam = {"adam tail not updated": dict(model_mutant="tail_not_updated"), "adam m written on a skipped step": dict(model_mutant="m_on_skipped_step"),
            "adam bias correction at t - 1": dict(tick_mutant="bias_t_minus_1"), "adam EMA decay off by one in k": dict(tick_mutant="ema_k_off_by_one"),
            "adam weight decay before the clip scale": dict(model_mutant="wd_before_clip"), "adam EMA from the old p": dict(model_mutant="ema_from_old_p"),
            "adam eps under the root": dict(model_mutant="eps_under_root")}
    slope = {"slope Bessel level sums the first 32 frequencies only": "bessel_first_32", "slope d2 term dropped from gz": "no_d2",
             "slope last odd row dropped": "last_odd_row_dropped", "slope last row range of the split dropped": "last_range_dropped",
             "slope alpha applied once in gz": "alpha_once", "slope delta = r_max": "delta_is_r_max", "slope cutoff kinds swapped": "cutoff_swapped"}
    assert all(old_adam_test(*cfg) < 1e-5 for cfg in OLD_ADAM_CONFIGS)      # (the models themselves pass the test: 9e-8 .. 1.3e-7)
    through = set()
    for name, kw in adam.items():
        errs = [old_adam_test(*cfg, **kw) for cfg in OLD_ADAM_CONFIGS]
        print(f"{name}: rel_err {['%.2e' % e for e in errs]} against 1e-5")
        if all(e < 1e-5 for e in errs):
            through.add(name)
    for name, mutant in slope.items():
        errs = [old_slope_test(nb, mutant) for nb in (8, 48)]
        print(f"{name}: rel_err (D, g first hidden, g bessel) {[tuple('%.2e' % x for x in e) for e in errs]} against (2e-6, 5e-5, 5e-5)")
        if all(e[0] < 2e-6 and e[1] < 5e-5 and e[2] < 5e-5 for e in errs):
            through.add(name)
    assert through == set(LET_THROUGH), sorted(through)
    assert through | set(CAUGHT) == set(adam) | set(slope)
