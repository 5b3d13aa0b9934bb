"""The node-side kernels the library ships == the kernels tests/test_gpu_node_matrix.py's cases name plus a short table of kernels
credited to other test files (no GPU needed); every node-side function of include/e3k.h is called by a case or a credited test; the
bounds of the matrix file shown to hold for float32 models of the kernels on the CPU, and shown to be sharp: a wrong term planted in
the float64 reference moves an element by >= 100 bounds on the family's own case inputs.

Reads the gfx950 code object of e3k_node.o: a kernel added without a float64-checked case, or a case naming a kernel that no longer
exists, fails here.

Credited elsewhere.  The Gate forward and backward kernels (scalar and 16-byte forms) are held to float64 element by element in
tests/test_gpu_node_passes.py (the two kernels of e3k_gate_bwd2 are not: they have cases in the matrix).  flag_fetch_clear_kernel
keeps its test in tests/test_gpu_ops.py.

Mutants under the old normwise tolerances (test_mutants_under_the_old_normwise_tolerance): clamping NormActivation on eps instead of
eps^2 is INVISIBLE on the shape of tests/test_gpu_ops.py::test_norm_activation (epsilon 1e-8, random channels and exactly-zero ones: no
channel lies between the two thresholds, rel_err 0), and a normalisation epsilon of 1e-5 gives about 6e-6 on test_layer_norm's shape, below that file's
tolerance of 1e-5: invisible too.  silu'' without its (1 - 2 s) factor is NOT invisible normwise (rel_err about 0.5).
"""
import os
import re
import subprocess

import numpy as np
import pytest

from tests import test_gpu_node_matrix as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NODE_OBJ = os.path.join(ROOT, "equivariant-nn-zoo_amd", "csrc", "e3k_node.o")
NODE_SRC = os.path.join(ROOT, "equivariant-nn-zoo_amd", "csrc", "e3k_node.hip")
HEADER = os.path.join(ROOT, "include", "e3k.h")
LLVM = "/opt/rocm/llvm/bin"
CASES = {c["id"]: c for c in M.CASES}
f32 = np.float32

# kernels and functions other test files hold: file -> (how, kernels, functions)
CREDITED = {
    "tests/test_gpu_node_passes.py": ("float64, element by element",
                                      {"gate_fwd_kernel", "gate_bwd_kernel", "gate_fwd4_kernel<0>", "gate_fwd4_kernel<1>", "gate_bwd4_kernel<0>",
                                       "gate_bwd4_kernel<1>"}, {"e3k_gate_fwd", "e3k_gate_bwd", "e3k_gate_path"}),
    "tests/test_gpu_ops.py": ("value and clearing", {"flag_fetch_clear_kernel"}, {"e3k_flag_fetch_clear"}),
}


def _tool(name):
    path = os.path.join(LLVM, name)
    return path if os.path.exists(path) else name


def _shipped_node_kernels(tmp_path):
    if not os.path.exists(NODE_OBJ):
        import __graft_entry__

        __graft_entry__.build()
    os.symlink(NODE_OBJ, tmp_path / "e3k_node.o")
    subprocess.run([_tool("llvm-objdump"), "--offloading", "e3k_node.o"], check=True, cwd=tmp_path, capture_output=True)
    bundles = [p for p in os.listdir(tmp_path) if p.endswith("gfx950")]
    assert len(bundles) == 1, os.listdir(tmp_path)
    syms = subprocess.run([_tool("llvm-readelf"), "-sW", str(tmp_path / bundles[0])], check=True, capture_output=True, text=True).stdout
    names = [f[7] for f in (line.split() for line in syms.splitlines()) if len(f) >= 8 and f[3] == "FUNC" and f[4] == "GLOBAL"]
    demangled = subprocess.run(["c++filt"], input="\n".join(names), check=True, capture_output=True, text=True).stdout
    return {m.group(1) for m in re.finditer(r"e3k::(\w+_kernel(?:<[^>]*>)?)\(", demangled)}


def test_every_node_kernel_has_a_float64_checked_case_or_a_credit(tmp_path):
    shipped = _shipped_node_kernels(tmp_path)
    # e3k_common.h's static zero_words_kernel is emitted into every object; e3k_node.hip launches it through zero_fill (keyed
    # backward over several key tiles without accumulate_w), so a case has to cover that path
    with open(NODE_SRC) as f:
        assert "zero_fill(" in f.read()
    assert "zero_words_kernel" in shipped and "zero_words_kernel" in M.table_kernels()
    credited = set().union(*(k for _, k, _ in CREDITED.values()))
    table = M.table_kernels()
    assert not (table & credited)
    assert len(shipped) == 31, sorted(shipped)
    assert shipped - table - credited == set(), f"kernels without a case in test_gpu_node_matrix.CASES: {sorted(shipped - table - credited)}"
    assert (table | credited) - shipped == set(), f"named, but not shipped: {sorted((table | credited) - shipped)}"


def test_every_node_function_of_the_header_is_called_by_a_case_or_a_credited_test():
    with open(HEADER) as f:
        text = f.read()
    a, b = text.index("Node-side elementwise kernels."), text.index("Fused hidden chain of the radial MLP.")
    declared = set(re.findall(r"\b(e3k_\w+)\s*\(", text[a:b])) - {"e3k_gemm_grouped", "e3k_keyed_weights_bwd_workspace(...)"}
    declared = {d for d in declared if re.search(r"\b(?:int|int64_t|void)\s+" + d + r"\s*\(", text[a:b])}
    assert len(declared) == 27, sorted(declared)
    credited = set().union(*(fn for _, _, fn in CREDITED.values()))
    called = M.table_functions()
    assert not (called & credited)
    assert declared - called - credited == set(), f"declared in include/e3k.h, called by no case: {sorted(declared - called - credited)}"
    assert (called | credited) - declared == set(), f"cases call functions the header does not declare: {sorted((called | credited) - declared)}"
    for path, (_, _, fns) in CREDITED.items():      # the credited files do call what they are credited with
        with open(os.path.join(ROOT, path)) as f:
            src = f.read()
        for fn in fns:
            assert fn in src, (path, fn)


def test_case_ids_are_unique_and_every_case_says_why():
    ids = [c["id"] for c in M.CASES]
    assert len(ids) == len(set(ids))
    assert all(c["why"] and c["fn"].startswith("e3k_") and c["fn"] in c["funcs"] for c in M.CASES)


def test_dispatch_thresholds_are_reached_by_shape():
    """the key tile (64, or 512 from 1024 column blocks on) and stores / atomics (one tile / several) have no export: both sides by shape"""
    kw = [c for c in M.CASES if c["kind"] == "kw"]
    wide = [c for c in kw if (c["total"] + 255) // 256 >= 1024]
    assert {c["tiles"] for c in wide if c["op"] == "bwd"} == {1, 2} and any(c["K"] > 64 and c["tiles"] == 1 for c in wide)
    narrow = [c for c in kw if (c["total"] + 255) // 256 < 1024 and c["op"] == "bwd"]
    assert {1, 2, 3} <= {c["tiles"] for c in narrow}
    assert {(c["acc"], c["tiles"] > 1) for c in kw if c["op"] == "bwd" and "w" in c["outs"]} >= {(0, False), (0, True), (1, False), (1, True)}
    assert {c["K"] for c in kw} >= {1, 16, 17, 64, 65, 128, 129} and {c["V"] for c in kw} >= {1, 7, 32}
    assert {len(c["layers"]) for c in M.CASES if c["kind"] == "kwm"} >= {1, 2, 8}
    # an instruction boundary inside a 256-column block, different w_out on either side
    (u0, w0), (u1, w1) = M.KW_300
    assert 0 < u0 * w0 < 256 and w0 != w1 and u0 * w0 + u1 * w1 == 300
    # the grid caps
    assert any(c["kind"] == "ln" and (c["rows"] + 3) // 4 > 512 for c in M.CASES)
    assert all(any(c["kind"] == k and n(c) > M.GRID_CAP for c in M.CASES) for k, n in
               (("act", lambda c: c["n"]), ("na", lambda c: c["rows"] * M.TABLES[c["table"]]["row_dim"]), ("oh", lambda c: c["rows"] * c["T"]),
                ("seg", lambda c: len(c["sizes"]) * c["dim"])))


# ---------------------------------------------------------------------------------------------------------------------------------
# float32 models, operation for operation (numpy's float32 exp / log / tanh stand in for the device's)
ONE, TWO, HALF = f32(1), f32(2), f32(0.5)


def sig32(x):
    with np.errstate(over="ignore"):
        return ONE / (ONE + np.exp(-x))


def act32(a, x):
    if a == 1:
        return np.maximum(x, f32(0)) + np.log(ONE + np.exp(-np.abs(x))) - f32(0.6931471805599453)
    return {0: lambda: x, 2: lambda: x * sig32(x), 3: lambda: np.tanh(x) * np.abs(x), 4: lambda: np.tanh(x), 5: lambda: np.abs(x)}[a]()


def dact32(a, x):
    if a == 1:
        return sig32(x)
    if a == 2:
        s = sig32(x)
        return s * (ONE + x * (ONE - s))
    if a == 3:
        th = np.tanh(x)
        return (ONE - th * th) * np.abs(x) + th * np.sign(x)
    if a == 4:
        th = np.tanh(x)
        return ONE - th * th
    return np.sign(x) if a == 5 else np.ones_like(x)


def d2act32(a, x):
    if a == 1:
        s = sig32(x)
        return s * (ONE - s)
    if a == 2:
        s = sig32(x)
        return s * (ONE - s) * (TWO + x * (ONE - TWO * s))
    if a == 3:
        th = np.tanh(x)
        return TWO * (ONE - th * th) * (np.sign(x) - th * np.abs(x))
    if a == 4:
        th = np.tanh(x)
        return -TWO * th * (ONE - th * th)
    return np.zeros_like(x)


def act_model32(c, inp):
    a, cst, x, gy, gh = c["act"], f32(c["cst"]), inp["x"], inp["gy"], inp["gh"]
    with np.errstate(over="ignore", invalid="ignore"):
        if c["op"] == "fwd":
            return dict(y=cst * act32(a, x))
        if c["op"] == "bwd":
            return dict(gx=gy * cst * dact32(a, x))
        if c["op"] == "bwd2":
            h = gh * cst
            return dict(g_gy=h * dact32(a, x), g_x=h * gy * d2act32(a, x))
        inv = ONE / cst
        return dict(gx=gy * cst * (ONE - HALF * np.exp(-inp["y"] * inv)))


def normact_scale32(c, n2, second):
    """normact_scale / normact_scale2"""
    a, eps2 = c["act"], f32(c["eps"]) * f32(c["eps"])
    zero = np.zeros_like(n2)
    if eps2 > 0:
        clamped = n2 < eps2
        n = np.sqrt(np.where(clamped, eps2, n2))
        av, a1 = act32(a, n), dact32(a, n)
        if not second:
            if c["normalize"]:
                return av / n, np.where(clamped, zero, (a1 * n - av) / (n * n * n)), None
            return av, np.where(clamped, zero, a1 / n), None
        a2 = d2act32(a, n)
        if c["normalize"]:
            s, s1, s2 = av / n, (a1 * n - av) / (n * n), (a2 * n * n - TWO * a1 * n + TWO * av) / (n * n * n)
        else:
            s, s1, s2 = av, a1, a2
        return s, np.where(clamped, zero, s1 / n), np.where(clamped, zero, (s2 * n - s1) / (n * n * n))
    return act32(a, n2), TWO * dact32(a, n2), (f32(4) * d2act32(a, n2) if second else None)


def _fma32(a, b, c):
    """fmaf: one rounding (the float64 product of two float32 is exact; the sum's double rounding is below 2^-52)"""
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(f32)


def _dot32(a, b):
    """serial sum over axis 1 of [rows, dim, mul] products"""
    acc = np.zeros((a.shape[0], a.shape[2]), f32)
    for q in range(a.shape[1]):
        acc = a[:, q] * b[:, q] + acc
    return acc


def normact_model32(c, inp):
    tb, rows, op = M.TABLES[c["table"]], c["rows"], c["op"]
    out = {k: np.zeros((rows, tb["row_dim"]), f32) for k in {"fwd": ["y"], "bwd": ["gx"], "bwd2": ["g_gy", "g_x"]}[op]}
    for off, mul, dim in tb["blocks"]:
        sl = slice(off, off + mul * dim)
        X = inp["x"][:, sl].reshape(rows, dim, mul)
        s, d, d2 = normact_scale32(c, _dot32(X, X), op == "bwd2")
        s, d = s[:, None, :], d[:, None, :]
        e3 = lambda v: v.transpose(0, 2, 1).reshape(rows, -1)
        if op == "fwd":
            out["y"][:, sl] = e3(s * X)
            continue
        G = inp["gy"][:, sl].reshape(rows, mul, dim).transpose(0, 2, 1)
        gx_ = _dot32(G, X)[:, None, :]
        if op == "bwd":
            out["gx"][:, sl] = _fma32(s, G, d * gx_ * X).reshape(rows, -1)
            continue
        H = inp["h"][:, sl].reshape(rows, dim, mul)
        hx, hg, d2 = _dot32(H, X)[:, None, :], _dot32(H, G)[:, None, :], d2[:, None, :]
        out["g_gy"][:, sl] = e3(_fma32(s, H, d * hx * X))
        out["g_x"][:, sl] = (d * X * hg + d2 * X * hx * gx_ + d * (H * gx_ + hx * G)).reshape(rows, -1)
    assert all(v.dtype == f32 for v in out.values())
    return out


def _wave_sum32(t):
    """[rows, len] -> [rows]: 64 lanes stride the block, then a butterfly over the lanes"""
    rows, n = t.shape
    pad = np.zeros((rows, -(-n // 64) * 64), f32)
    pad[:, :n] = t
    lanes = np.zeros((rows, 64), f32)
    for j in range(pad.shape[1] // 64):
        lanes = lanes + pad[:, 64 * j:64 * j + 64]
    w = 64
    while w > 1:
        w //= 2
        lanes = lanes[:, :w] + lanes[:, w:2 * w]
    return lanes[:, 0]


def layernorm_model32(c, inp):
    tb, rows, op = M.TABLES[c["table"]], c["rows"], c["op"]
    nb = len(tb["blocks"])
    out = {k: np.full((rows, tb["row_dim"]), np.nan, f32) for k in {"fwd": ["y"], "bwd": ["gx"], "bwd2": ["g_gy", "g_x"]}[op]}
    if op == "fwd":
        out["inv"] = np.zeros((rows, nb), f32)
    else:
        out["g_std"] = inp["old_gstd"].copy()
    for k, (off, mul, dim) in enumerate(tb["blocks"]):
        sl = slice(off, off + mul * dim)
        X, sc, m = inp["x"][:, sl], inp["std"][k], f32(mul)
        if op == "fwd":
            inv = ONE / np.sqrt(_wave_sum32(X * X) / m + f32(1e-6))
            out["inv"][:, k] = inv
            out["y"][:, sl] = X * (inv * sc)[:, None]
            continue
        G, v = inp["gy"][:, sl], inp["inv"][:, k]
        D = _wave_sum32(G * X)
        if op == "bwd":
            coef = D * v * v / m
            out["gx"][:, sl] = (sc * v)[:, None] * (G - X * coef[:, None])
            t = D * v
        else:
            H = inp["h"][:, sl]
            A, B = _wave_sum32(H * G), _wave_sum32(H * X)
            hsk = inp["hs"][k] if c["hs"] else f32(0)
            v3 = v * v * v
            cg_x = -sc * v3 * B / m + hsk * v
            cx_x = -sc * A * v3 / m + f32(3) * sc * v3 * v * v * D * B / (m * m) - hsk * D * v3 / m
            cx_h = -sc * v3 * D / m
            out["g_gy"][:, sl] = _fma32((sc * v)[:, None], H, cg_x[:, None] * X)
            out["g_x"][:, sl] = _fma32(cx_x[:, None], X, _fma32(cg_x[:, None], G, cx_h[:, None] * H))
            t = v * A - v3 * D * B / m
        acc = f32(0)
        for r in range(rows):      # (one of the orders the waves and atomics may take)
            acc = acc + t[r]
        out["g_std"][k] = out["g_std"][k] + acc
    assert all(v.dtype == f32 for v in out.values())
    return out


def segment_model32(c, inp):
    out = np.zeros((len(c["sizes"]), c["dim"]), f32)
    for s, n in enumerate(c["sizes"]):
        acc = np.zeros(c["dim"], f32)
        for r in range(inp["ptr"][s], inp["ptr"][s + 1]):
            acc = acc + inp["x"][r]
        out[s] = acc / f32(max(n, 1)) if c["mean"] else acc
    return dict(out=out)


def _within(got32, want, bound, what):
    got, want, bound = got32.astype(np.float64).ravel(), np.asarray(want).ravel(), np.asarray(bound).ravel()
    nan = np.isnan(want)
    err = np.abs(got - np.where(nan, 0.0, want))
    ok = np.where(nan, np.isnan(got), np.isfinite(got) & (err <= bound))
    assert ok.all(), f"{what}: {int((~ok).sum())} elements of the float32 model outside the bound, worst {float((err[~ok] / np.maximum(bound[~ok], 1e-300)).max())}"
    live = ~nan & (bound > 0)
    return float((err[live] / bound[live]).max()) if live.any() else 0.0


def _model_ratios(kind, inputs, reference, model, skip=()):
    worst = {}
    for c in M.CASES:
        size = c.get("n", c.get("rows", len(c.get("sizes", ()))))
        if c["kind"] != kind or not size or size > 10000:
            continue
        inp = inputs(c)
        ref, got = reference(c, inp), model(c, inp)
        for name, v in got.items():
            fam = f"{kind}_{c['op']}" if "op" in c else kind
            worst[fam] = max(worst.get(fam, 0.0), _within(v, *ref[name], f"{c['id']} {name}"))
    return worst


# the floor: the worst model error over a family's cases is at least this fraction of its bound.  A running error bound is attained
# only when every rounding of a chain of ~10 operations is a full half ulp in the same direction; over the few thousand elements of a
# family's cases the worst element comes within a small factor of it, so a bound loose by an order of magnitude or more fails
FLOOR = 0.1


def test_activation_bounds_hold_for_a_float32_model():
    worst = _model_ratios("act", M.act_inputs, M.act_reference, act_model32)
    print("float32 model, worst error / bound:", worst)
    assert set(worst) == {"act_fwd", "act_bwd", "act_bwd2", "act_out"} and all(FLOOR < r <= 1.0 for r in worst.values()), worst


def test_normact_bounds_hold_for_a_float32_model():
    worst = _model_ratios("na", M.na_inputs, M.na_reference, normact_model32)
    print("float32 model, worst error / bound:", worst)
    assert set(worst) == {"na_fwd", "na_bwd", "na_bwd2"} and all(FLOOR < r <= 1.0 for r in worst.values()), worst


def test_layernorm_bounds_hold_for_a_float32_model():
    worst = _model_ratios("ln", M.ln_inputs, M.ln_reference, layernorm_model32)
    print("float32 model, worst error / bound:", worst)
    assert set(worst) == {"ln_fwd", "ln_bwd", "ln_bwd2"} and all(FLOOR < r <= 1.0 for r in worst.values()), worst


def test_segment_sum_bounds_hold_for_a_float32_model():
    worst = _model_ratios("seg", M.seg_inputs, M.seg_reference, segment_model32)
    print("float32 model, worst error / bound:", worst)
    assert FLOOR < worst["seg"] <= 1.0, worst


def _channel_norms(c, x):
    """per element of a row, the norm of its channel: in the channel-fastest layout and in the e3nn layout (NaN on uncovered columns)"""
    tb, rows = M.TABLES[c["table"]], x.shape[0]
    cf, e3 = np.full(x.shape, np.nan), np.full(x.shape, np.nan)
    for off, mul, dim in tb["blocks"]:
        X = x[:, off:off + mul * dim].astype(np.float64).reshape(rows, dim, mul)
        n = np.broadcast_to(np.sqrt((X * X).sum(1))[:, None, :], X.shape)
        cf[:, off:off + mul * dim] = n.reshape(rows, -1)
        e3[:, off:off + mul * dim] = n.transpose(0, 2, 1).reshape(rows, -1)
    return cf, e3


def test_nothing_is_left_out_of_normact_and_the_bound_is_loose_only_on_small_channels():
    """tests/test_gpu_ops.py::test_norm_activation leaves the clamped channels out.  The matrix leaves NOTHING out (its runner claims
    every word of every output with one comparison: 0 elements excluded, below the cap of the clamped channels' elements).  Where
    act(n) / n and its slopes divide an absolute error by n, n^2, n^3 the bound is large instead: every element bound above 1e-4
    lies in a channel of norm below 0.5 (the planted channels, and random ones that came out small), and the planted channels do
    show such bounds."""
    seen = 0
    for c in M.CASES:
        if c["kind"] == "na" and 0 < c["rows"] < 100:
            inp = M.na_inputs(c)
            ref = M.na_reference(c, inp)
            assert ref["clamped_elems"] <= int(inp["planted"].sum())
            if c["eps"] > 0:
                assert ref["clamped_elems"] > 0
            cf, e3 = _channel_norms(c, inp["x"])
            for name, norms in (("y", e3), ("gx", cf), ("g_gy", e3), ("g_x", cf)):
                if name in ref and c["eps"] > 0:      # (epsilon = 0: the argument is the squared norm, nothing is divided)
                    loose = ref[name][1] > 1e-4
                    assert not (loose & ~(norms < 0.5)).any(), (c["id"], name)
                    seen += int((loose & inp["planted"]).sum()) if name in ("gx", "g_x") else 0
    assert seen > 0


# ---------------------------------------------------------------------------------------------------------------------------------
# the bounds are sharp
MUTANTS = [
    # (mutant, the case whose inputs and bounds it is held against)
    ("silu_d2", "act_bwd2_silu"),
    ("tanhlu_sign", "act_bwd_tanhlu"),
    ("clamp_eps", "na_fwd_norm_silu"),
    ("no_d2", "na_bwd2_norm_silu"),
    ("mean_over_len", "ln_fwd_rows5"),
    ("eps_1e-5", "ln_fwd_rows5"),
    ("v5_factor", "ln_bwd2_rows5"),
    ("empty_div0", "seg_mean_d3"),
    ("uwv", "kw_fwd_V7"),
    ("silu_d2", "gate2_layer_cf"),
]
_REF = dict(act=(M.act_inputs, M.act_reference), gate2=(M.gate2_inputs, M.gate2_reference), na=(M.na_inputs, M.na_reference), ln=(M.ln_inputs, M.ln_reference), seg=(M.seg_inputs, M.seg_reference),
            kw=(M.kw_inputs, M.kw_reference))


def _mutant_move(mutant, cid):
    """the largest |mutated reference - reference| / bound over the case's elements (a non-finite mutated element counts as infinite)"""
    c = CASES[cid]
    inputs, reference = _REF[c["kind"]]
    inp = inputs(c)
    ref, mut = reference(c, inp), reference(c, inp, mutant=mutant)
    move = 0.0
    for name, v in ref.items():
        if not isinstance(v, tuple):
            continue
        want, bound, got = np.asarray(v[0]), np.asarray(v[1]), np.asarray(mut[name][0])
        live = np.isfinite(want) & (bound > 0)
        with np.errstate(invalid="ignore"):
            r = np.where(np.isfinite(got[live]), np.abs(got[live] - want[live]) / bound[live], np.inf)
        move = max(move, float(r.max()) if r.size else 0.0)
    return move


@pytest.mark.parametrize("mutant,cid", MUTANTS, ids=[m[0] + "-" + m[1] for m in MUTANTS])
def test_a_planted_mutant_moves_an_element_by_100_bounds(mutant, cid):
    move = _mutant_move(mutant, cid)
    print(f"mutant {mutant} on {cid}: {move:.3g} bounds")
    assert move >= 100.0, f"{mutant}: the reference moves by {move} bounds only"


def _rel(a, b):
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def test_mutants_under_the_old_normwise_tolerance():
    """rel_err of three mutants on the shapes the module tests use: 150 rows of 8x0e+8x0o+4x1o+6x2e+3x3o with one exactly-zero block
    and epsilon 1e-8 (test_norm_activation, tolerance 1e-5); 64 random rows of 8x0e+8x1o+4x2e (test_layer_norm, 1e-5); random
    arguments of silu'' (the double backward of an activation, 1e-4)"""
    rng = np.random.default_rng(14)
    tb = dict(blocks=M._packed([(8, 1), (8, 1), (4, 3), (6, 5), (3, 7)]), row_dim=79)
    M.TABLES["_old_na"] = tb
    try:
        c = dict(M.na("_old", "x", "fwd", "_old_na", 2, 150, eps=1e-8), id="_old")
        x = rng.standard_normal((150, 79)).astype(f32)
        x[3, 16:28] = 0.0
        inp = dict(x=x, gy=x, h=x)
        want, mut = M.na_reference(c, inp)["y"][0], M.na_reference(c, inp, mutant="clamp_eps")["y"][0]
    finally:
        del M.TABLES["_old_na"]
    clamp = _rel(mut, want)
    M.TABLES["_old_ln"] = dict(blocks=M._packed([(8, 1), (8, 3), (4, 5)]), row_dim=52)      # 8x0e+8x1o+4x2e, 64 rows
    try:
        c = dict(M.ln("_old", "x", "fwd", "_old_ln", 64), id="_old")
        inp = dict(x=rng.standard_normal((64, 52)).astype(f32), std=rng.uniform(0.5, 1.5, 3).astype(f32))
        eps = _rel(M.ln_reference(c, inp, mutant="eps_1e-5")["y"][0], M.ln_reference(c, inp)["y"][0])
    finally:
        del M.TABLES["_old_ln"]
    xs = rng.standard_normal(4000)
    silu = _rel(M.d2act_ev(2, xs, "silu_d2").v, M.d2act_ev(2, xs).v)
    print(f"normwise: clamp_eps {clamp:.3g} (1e-5), eps_1e-5 {eps:.3g} (1e-5), silu_d2 {silu:.3g} (1e-4)")
    assert clamp < 1e-5      # invisible under the old test
    assert eps < 1e-5        # invisible under the old test
    assert silu > 1e-2       # NOT invisible normwise
