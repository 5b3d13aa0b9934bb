"""The edge-geometry kernels the library ships == the kernels tests/test_gpu_edge_matrix.py's cases name (no GPU needed); the bounds of
that file shown to hold for float32 models of the forward and first-order kernels on the CPU, and shown to be sharp: a wrong term planted
in the float64 reference moves an element by >= 100 bounds on the family's own case inputs.

Reads the gfx950 code object of e3k_edge.o: a kernel added without a float64-checked case, or a case naming a kernel that no longer
exists, fails here; so does an edge-geometry function of include/e3k.h that no case calls.

Mutants.  Each is planted in the float64 reference and must move one element of its family's case by >= 100 bounds.  ``s15`` (sqrt(15)
truncated to 3.873) is a relative change of 72 u: it separates only where the bound is below 0.72 u, which a count of roundings never
is.  The forward bound of the components s15 (a b) therefore counts only the products that are inexact in fp32 and the constant's own
representation error (0.474 u): on the vector (1, 1, 0) the mutant moves s15 x y by 152 bounds.
Normwise (rel_err on the shape and under the tolerance of tests/test_gpu_ops.py, test_mutants_under_the_old_normwise_tolerance): s15
gives 3e-6 < 1e-5, invisible there.  The l = 3, m = +-1 swap, marked "norm" in the plan, is NOT invisible normwise (rel_err 0.49), nor
are c1 p for c1 (p + 1) (0.25) and the dropped sin / r^2 term (0.37) on that shape: the claim is dropped for them; what a norm hides
are errors of a few 1e-6 relative, which is s15's size.
"""
import math
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from oracle import e3ref
from tests import test_gpu_edge_matrix as M
from tests.util import rel_err

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EDGE_OBJ = os.path.join(ROOT, "equivariant-nn-zoo_amd", "csrc", "e3k_edge.o")
HEADER = os.path.join(ROOT, "include", "e3k.h")
LLVM = "/opt/rocm/llvm/bin"
CASES = {c["id"]: c for c in M.CASES}
f32 = np.float32


def _tool(name):
    path = os.path.join(LLVM, name)
    return path if os.path.exists(path) else name


def _shipped_edge_kernels(tmp_path):
    if not os.path.exists(EDGE_OBJ):
        import __graft_entry__

        __graft_entry__.build()
    os.symlink(EDGE_OBJ, tmp_path / "e3k_edge.o")
    subprocess.run([_tool("llvm-objdump"), "--offloading", "e3k_edge.o"], check=True, cwd=tmp_path, capture_output=True)
    bundles = [p for p in os.listdir(tmp_path) if p.endswith("gfx950")]
    assert len(bundles) == 1, os.listdir(tmp_path)
    syms = subprocess.run([_tool("llvm-readelf"), "-sW", str(tmp_path / bundles[0])], check=True, capture_output=True, text=True).stdout
    names = [f[7] for f in (line.split() for line in syms.splitlines()) if len(f) >= 8 and f[3] == "FUNC" and f[4] == "GLOBAL"]
    demangled = subprocess.run(["c++filt"], input="\n".join(names), check=True, capture_output=True, text=True).stdout
    found = {m.group(1) for m in re.finditer(r"e3k::(\w+_kernel(?:<[^>]*>)?)\(", demangled)}
    # e3k_common.h's static zero_words_kernel is emitted into every object; e3k_edge.hip never launches it (nor the helper round it)
    with open(os.path.join(os.path.dirname(EDGE_OBJ), "e3k_edge.hip")) as f:
        text = f.read()
    assert "zero_words" not in text and "zero_fill" not in text
    return found - {"zero_words_kernel"}


def test_every_edge_kernel_has_a_float64_checked_case(tmp_path):
    shipped = _shipped_edge_kernels(tmp_path)
    table = M.table_kernels()
    assert len(shipped) == 13, sorted(shipped)
    assert shipped - table == set(), f"kernels without a case in test_gpu_edge_matrix.CASES: {sorted(shipped - table)}"
    assert table - shipped == set(), f"the case table names kernels the library does not ship: {sorted(table - shipped)}"


def test_every_edge_function_of_the_header_is_called_by_a_case():
    with open(HEADER) as f:
        declared = set(re.findall(r"\b(e3k_(?:edge_vector|sph_harm|radial_basis|radius_graph)_\w+)\s*\(", f.read()))
    assert len(declared) == 11, sorted(declared)
    called = M.table_functions()
    assert declared - called == set(), f"declared in include/e3k.h, called by no case: {sorted(declared - called)}"
    assert called - declared == set(), f"cases call functions the header does not declare: {sorted(called - declared)}"


def test_case_ids_are_unique():
    ids = [c["id"] for c in M.CASES]
    assert len(ids) == len(set(ids))
    assert all(c["why"] for c in M.CASES)


@pytest.mark.parametrize("nb,unroll", [(1, 8), (8, 8), (9, 16), (16, 16), (17, 32), (32, 32), (33, 64), (64, 64), (0, -1), (65, -1), (-3, -1)])
def test_radial_bwd_unroll_rule(nb, unroll):
    from e3_layers_amd.backend import lib as L

    assert L.load().e3k_radial_basis_bwd_unroll(nb) == unroll
    if unroll > 0:
        assert M.rad("x", "x", "bwd", nb)["kernels"] == {f"radial_bwd_kernel<{unroll}>"}


# ---------------------------------------------------------------------------------------------------------------------------------
# the restatements the references use, held to the oracle
def test_restatements_agree_with_the_oracle():
    rng = np.random.default_rng(3)
    v = torch.from_numpy(rng.standard_normal((400, 3)))
    v[0] = 0.0
    v[1] = torch.tensor([3e-13, -4e-13, 0.0])
    v[2] *= 1e-14
    assert torch.allclose(M.normalize64(v), torch.nn.functional.normalize(v, dim=-1), rtol=1e-15, atol=0)
    for nn_ in range(3):
        a = M.sh_blocks([0, 1, 2, 3, 2, 1], v[3:], nn_)
        b = e3ref.spherical_harmonics([0, 1, 2, 3, 2, 1], v[3:], False, M.NORMALIZATIONS[nn_])
        assert torch.allclose(a, b, rtol=1e-14, atol=1e-14)
        assert (M.sh_blocks([0, 1, 2, 3], v[3:].abs(), nn_, sgn=+1.0) >= a[:, :16].abs() * (1 - 1e-14)).all()
    # autograd of F.normalize agrees with normalize64 where it is finite
    vv = v[3:].clone().requires_grad_(True)
    g = torch.from_numpy(rng.standard_normal((397, 3)))
    (a,) = torch.autograd.grad(M.normalize64(vv), vv, g)
    (b,) = torch.autograd.grad(torch.nn.functional.normalize(vv, dim=-1), vv, g)
    assert torch.allclose(a, b, rtol=1e-12, atol=1e-12)
    for cut, fn in ((0, e3ref.poly_cutoff), (1, e3ref.symmetric_cutoff)):
        for oor in (0, 1):
            prm = dict(r_max=4.0, r_min=0.5, p=6.0, oor=oor, cut=cut)
            r = torch.from_numpy(rng.uniform(0.2, 4.6, 300))
            w = torch.from_numpy(np.arange(1, 9) * math.pi * (1 + 0.03 * rng.standard_normal(8)))
            got = M.rad_formula(r[:, None], w[None, :], prm)
            bb = e3ref.BesselBasis(4.0, 0.5, 8, one_over_r=bool(oor)).double()
            with torch.no_grad():
                bb.bessel_weights.copy_(w)
                want = bb(r) * fn(r, 1.0 / 4.0, 6.0)[:, None]
            assert torch.allclose(got, want, rtol=1e-12, atol=1e-13)


@pytest.mark.parametrize("cid", ["rad_bwd_nb17", "rad_bwd_cut1_oor0_edge", "rad_bwd_cut0_oor1_edge", "rad_bwd_p2.5", "rad_bwd_rmin"])
def test_explicit_radial_backward_equals_autograd(cid):
    c = CASES[cid]
    inp = M.rad_inputs(c)
    ref = M.rad_reference(c, inp)
    g_r, g_w = M.rad_bwd_explicit(inp, M.rad_params(c))
    assert np.abs(g_r - ref["g_r"][0]).max() <= 1e-3 * ref["g_r"][1][ref["g_r"][1] > 0].min() + 1e-9 * np.abs(g_r).max()
    assert np.allclose(g_w + inp["old_w"], ref["g_w"][0], rtol=1e-10, atol=1e-10)


# ---------------------------------------------------------------------------------------------------------------------------------
# float32 models of the forward and first-order kernels, operation for operation (numpy's float32 sin / cos / power stand in for the
# device library)
class D3:
    """value and gradient, fp32 (the kernel's D3)"""

    def __init__(self, v, dx, dy, dz):
        self.v, self.d = v, (dx, dy, dz)

    def __mul__(self, o):
        return D3(self.v * o.v, *[self.v * b + a * o.v for a, b in zip(self.d, o.d)])

    def __add__(self, o):
        return D3(self.v + o.v, *[a + b for a, b in zip(self.d, o.d)])

    def __sub__(self, o):
        return D3(self.v - o.v, *[a - b for a, b in zip(self.d, o.d)])

    def __rmul__(self, s):
        return D3(s * self.v, *[s * a for a in self.d])


def _sh_eval32(l, x, y, z):
    s3, s5, s15, s7 = f32(1.7320508075688772), f32(2.23606797749979), f32(3.872983346207417), f32(2.6457513110645907)
    one, zero = np.ones_like(x.v), np.zeros_like(x.v)
    if l == 0:
        return [D3(one, zero, zero, zero)]
    if l == 1:
        return [s3 * x, s3 * y, s3 * z]
    x2, y2, z2 = x * x, y * y, z * z
    x2z2 = x2 + z2
    q = [s15 * (x * z), s15 * (x * y), s5 * (y2 - f32(0.5) * x2z2), s15 * (y * z), (f32(0.5) * s15) * (z2 - x2)]
    if l == 2:
        return q
    a, b = f32(1.0801234497346435), f32(1.6201851746019651)
    f = f32(4.0) * y2 - x2z2
    return [a * (q[0] * z + q[4] * x), s7 * (q[0] * y), b * (f * x), (f32(0.5) * s7) * (y * (f32(2.0) * y2 - f32(3.0) * x2z2)), b * (z * f),
            s7 * (q[4] * y), a * (q[4] * z - q[0] * x)]


def sh_model32(c, inp):
    """sph_harm_kernel<false> / <true> in numpy float32: (sh [E, dim], g_vec [E, 3])"""
    vec, g_sh = inp["vec"], inp["g_sh"]
    vx, vy, vz = vec[:, 0], vec[:, 1], vec[:, 2]
    ux, uy, uz, inv = vx, vy, vz, np.ones_like(vx)
    clamped = np.zeros(len(vx), bool)
    if c["normalize"]:
        r = np.sqrt(vx * vx + vy * vy + vz * vz)
        clamped = ~(r > f32(1e-12))
        inv = f32(1.0) / np.maximum(r, f32(1e-12))
        ux, uy, uz = ux * inv, uy * inv, uz * inv
    one, zero = np.ones_like(vx), np.zeros_like(vx)
    x, y, z = D3(ux, one, zero, zero), D3(uy, zero, one, zero), D3(uz, zero, zero, one)
    cols, off = [], 0
    g = [np.zeros_like(vx) for _ in range(3)]
    for l in c["ls"]:
        nf = f32(1.0) if c["normalization"] == 0 else f32(0.28209479177387814) if c["normalization"] == 1 else f32(1.0) / np.sqrt(f32(2 * l + 1))
        for o in _sh_eval32(l, x, y, z):
            cols.append(nf * o.v)
            gm = nf * g_sh[:, off]
            g = [gm * d + a for d, a in zip(o.d, g)]
            off += 1
    if c["normalize"]:
        dot = np.where(clamped, f32(0), g[0] * ux + g[1] * uy + g[2] * uz)
        g = [(a - u * dot) * inv for a, u in zip(g, (ux, uy, uz))]
    out = np.stack(cols, 1), np.stack(g, 1)
    assert out[0].dtype == np.float32 and out[1].dtype == np.float32
    return out


def _cutoff32(r, prm):
    r_max, p = f32(prm["r_max"]), f32(prm["p"])
    x = r / r_max
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        if prm["cut"] == 1:
            q = x * x - f32(1)
            inside = np.abs(x) < f32(1)
            return np.where(inside, q * q, f32(0)), np.where(inside, f32(4) * q * x / r_max, f32(0))
        inside = x < f32(1)
        xs = np.where(inside, x, f32(0.5))
        xp = np.power(xs, p)
        c0, c1, c2 = (p + f32(1)) * (p + f32(2)) * f32(0.5), p * (p + f32(2)), p * (p + f32(1)) * f32(0.5)
        cc = f32(1) - c0 * xp + c1 * xp * xs - c2 * xp * xs * xs
        xpm1 = np.where(xs != 0, xp / xs, f32(0))
        dc = (-c0 * p * xpm1 + c1 * (p + f32(1)) * xp - c2 * (p + f32(2)) * xp * xs) / r_max
    return np.where(inside, cc, f32(0)).astype(f32), np.where(inside, dc, f32(0)).astype(f32)


def rad_model32(c, inp):
    """radial_fwd_kernel and radial_bwd_kernel in numpy float32: out [E, nb], g_r [E], g_w [nb] (old values included)"""
    prm = M.rad_params(c)
    r, w, g = inp["r"][:, None], inp["w"][None, :], inp["g"]
    delta = f32(prm["r_max"]) - f32(prm["r_min"])
    pref = f32(2.0) / delta
    cc, dc = _cutoff32(r, prm)
    with np.errstate(invalid="ignore", divide="ignore"):
        arg = w * r / delta
        sn, cs = np.sin(arg), np.cos(arg)
        scale = pref * cc / r if prm["oor"] else pref * cc
        out = sn * scale
        inv_r = f32(1) / r if prm["oor"] else np.ones_like(r)
        dbasis = pref * cs * (w / delta) * inv_r
        if prm["oor"]:
            dbasis = dbasis - pref * sn * inv_r * inv_r
        g_r = (g * (dbasis * cc + pref * sn * inv_r * dc)).sum(1, dtype=f32)
        g_w = (g * (pref * cs * (r / delta) * inv_r * cc)).sum(0, dtype=f32) + inp["old_w"]
    assert out.dtype == f32 and g_r.dtype == f32 and g_w.dtype == f32
    return out, g_r, g_w


def _fma32(a, b, c):
    return f32(np.float64(a) * np.float64(b) + np.float64(c))


def evb_model32(inp, g_vec=True, g_len=True):
    """edge_vector_bwd_kernel: one serial FMA chain per node, in-edges then out-edges in CSR order"""
    N = inp["N"]
    out = np.zeros((N, 3), f32)
    for n in range(N):
        acc = [f32(0)] * 3
        for name, sign in (("dst", f32(1)), ("src", f32(-1))):
            for t in range(inp[name + "_ptr"][n], inp[name + "_ptr"][n + 1]):
                e = inp[name + "_perm"][t]
                gv = [inp["g_vec"][e, k] if g_vec else f32(0) for k in range(3)]
                if g_len:
                    ln = inp["len"][e]
                    f = inp["g_len"][e] / ln if ln > 0 else f32(0)
                    gv = [_fma32(f, inp["vec"][e, k], gv[k]) for k in range(3)]
                acc = [_fma32(sign, gv[k], acc[k]) for k in range(3)]
        out[n] = acc
    return out


def _within(got32, want, bound, what):
    got = got32.astype(np.float64)
    err = np.abs(got - want)
    ok = np.isfinite(got) & (err <= bound)
    assert ok.all(), f"{what}: {int((~ok).sum())} elements of the float32 model outside the bound, worst {float((err[~ok] / np.maximum(bound[~ok], 1e-300)).max())}"
    live = bound > 0
    return float((err[live] / bound[live]).max()) if live.any() else 0.0


def test_edge_vector_bounds_hold_for_a_float32_model():
    worst = 0.0
    for c in M.CASES:
        if c["kind"] == "evf" and c["E"]:
            inp = M.evf_inputs(c)
            vec, ln, bound = M.evf_reference(inp)
            ln32 = np.sqrt((vec[:, 0] * vec[:, 0] + vec[:, 1] * vec[:, 1]) + vec[:, 2] * vec[:, 2])
            worst = max(worst, _within(ln32, ln, bound, c["id"]))
            assert ln[0] == 0 or c["E"] < 4      # (the self-loop)
        if c["kind"] == "evb" and c["N"] and (c["g_vec"] or c["g_len"]):
            inp = M.evb_inputs(c)
            want, bound = M.evb_reference(inp, c["g_vec"], c["g_len"])
            _within(evb_model32(inp, c["g_vec"], c["g_len"]), want, bound, c["id"])
            if inp["role"]:
                ro = inp["role"]
                deg_in, deg_out = np.bincount(inp["dst"], minlength=c["N"]), np.bincount(inp["src"], minlength=c["N"])
                assert deg_in[ro["lone"]] == deg_out[ro["lone"]] == 0 and deg_out[ro["sink"]] == 0 < deg_in[ro["sink"]]
                assert deg_in[ro["source"]] == 0 < deg_out[ro["source"]] and (inp["len"] == 0).sum() >= 3
                assert "hub" not in ro or deg_in[ro["hub"]] >= 3000 and deg_out[ro["hub"]] >= 2000
    assert 0.1 < worst <= 1.0, worst


def test_sph_harm_bounds_hold_for_a_float32_model():
    worst = {"fwd": 0.0, "bwd": 0.0}
    for c in M.CASES:
        if c["kind"] == "sh" and c["op"] in ("fwd", "bwd") and c["E"]:
            inp = M.sh_inputs(c)
            ref = M.sh_reference(c, inp)
            sh32, g32 = sh_model32(c, inp)
            want, bound = ref["sh" if c["op"] == "fwd" else "g_vec"]
            worst[c["op"]] = max(worst[c["op"]], _within(sh32 if c["op"] == "fwd" else g32, want, bound, c["id"]))
    print("float32 model, worst error / bound:", worst)
    assert 0.02 < worst["fwd"] <= 1.0 and 0.02 < worst["bwd"] <= 1.0, worst


def test_radial_bounds_hold_for_a_float32_model():
    worst = {"fwd": 0.0, "bwd": 0.0}
    for c in M.CASES:
        if c["kind"] == "rad" and c["op"] in ("fwd", "bwd") and c["E"]:
            inp = M.rad_inputs(c)
            ref = M.rad_reference(c, inp)
            out, g_r, g_w = rad_model32(c, inp)
            if c["op"] == "fwd":
                worst["fwd"] = max(worst["fwd"], _within(out, *ref["out"], c["id"]))
            else:
                worst["bwd"] = max(worst["bwd"], _within(g_r, *ref["g_r"], c["id"] + " g_r"), _within(g_w, *ref["g_w"], c["id"] + " g_w"))
    print("float32 model, worst error / bound:", worst)
    assert 0.02 < worst["fwd"] <= 1.0 and 0.02 < worst["bwd"] <= 1.0, worst


# ---------------------------------------------------------------------------------------------------------------------------------
# the bounds are sharp
MUTANTS = [
    # (mutant, the case whose inputs and bounds it is held against, the output)
    ("s15", "sh_fwd_special_n0", "sh"),
    ("swap_m1", "sh_fwd_ls0123", "sh"),
    ("norm_2l1", "sh_fwd_n1_norm2", "sh"),
    ("no_projection", "sh_bwd_ls0123", "g_vec"),
    ("hessian_const_inv", "sh_bwd2_ls0123", "g_vec2"),
    ("no_sin_r2", "rad_bwd_nb8", "g_r"),
    ("c1_p", "rad_bwd_nb8", "g_r"),
    ("delta_is_r_max", "rad_fwd_rmin", "out"),
    ("src_sign", "evb_N257", "g_pos"),
    ("no_inv_len", "evb_N257", "g_pos"),
]


def _mutant_move(mutant, cid, out):
    """the largest |mutated reference - reference| / bound over the case's elements"""
    c = CASES[cid]
    if c["kind"] == "sh":
        inp = M.sh_inputs(c)
        (want, bound), (mut, _) = M.sh_reference(c, inp)[out], M.sh_reference(c, inp, mutant=mutant)[out]
    elif c["kind"] == "rad":
        inp = M.rad_inputs(c)
        want, bound = M.rad_reference(c, inp)[out]
        if mutant == "delta_is_r_max":
            mut = M.rad_reference(c, inp, mutant=mutant)[out][0]
        else:
            assert c["oor"] == 1 and c["cut"] == 0
            mut = M.rad_bwd_explicit(inp, M.rad_params(c), mutant=mutant)[0]
    else:
        inp = M.evb_inputs(c)
        (want, bound), (mut, _) = M.evb_reference(inp), M.evb_reference(inp, mutant=mutant)
        if mutant == "src_sign":      # a self-loop-free part of the graph is enough: nodes the loop does not touch
            keep = np.ones(c["N"], bool)
            keep[inp["role"]["loop"]] = False
            want, bound, mut = want[keep], bound[keep], mut[keep]
    live = bound > 0
    return float((np.abs(mut - want)[live] / bound[live]).max())


@pytest.mark.parametrize("mutant,cid,out", MUTANTS, ids=[m[0] for m in MUTANTS])
def test_a_planted_mutant_moves_an_element_by_100_bounds(mutant, cid, out):
    move = _mutant_move(mutant, cid, out)
    print(f"mutant {mutant} on {cid}: {move:.3g} bounds")
    assert move >= 100.0, f"{mutant}: the reference moves by {move} bounds only"


def test_mutants_under_the_old_normwise_tolerance():
    """rel_err of a mutant on the shape tests/test_gpu_ops.py uses (500 vectors, [0, 1, 2, 3], normalize, component; 777 radii, 8 basis
    functions, one_over_r, polynomial cutoff) against its tolerance there"""
    torch.manual_seed(5)
    v = torch.randn(500, 3, dtype=torch.float64) * 2.0
    ref = M.sh_function([0, 1, 2, 3], 1, 0)(v)
    s15 = rel_err(M.sh_function([0, 1, 2, 3], 1, 0, "s15")(v), ref)
    swap = rel_err(M.sh_function([0, 1, 2, 3], 1, 0, "swap_m1")(v), ref)
    print(f"normwise: s15 {s15:.3g}, swap_m1 {swap:.3g} (tolerance 1e-5)")
    assert s15 < 1e-5      # invisible under the old test, 18 bounds here
    assert swap > 1e-2     # NOT invisible normwise: the plan's "norm" mark is dropped for the swap
    torch.manual_seed(6)
    r = (torch.rand(777, dtype=torch.float64) * 4.6 + 0.4).numpy().astype(np.float32)
    rng = np.random.default_rng(6)
    inp = dict(r=r, w=(np.arange(1, 9) * math.pi).astype(np.float32), g=rng.standard_normal((777, 8)).astype(np.float32))
    prm = dict(r_max=4.0, r_min=0.0, p=6.0, oor=1, cut=0)
    g_r = torch.from_numpy(M.rad_bwd_explicit(inp, prm)[0])
    for mutant, below in (("c1_p", False), ("no_sin_r2", False)):
        e = rel_err(torch.from_numpy(M.rad_bwd_explicit(inp, prm, mutant)[0]), g_r)
        print(f"normwise: {mutant} {e:.3g} (tolerance 5e-5)")
        assert (e < 5e-5) == below


# ---------------------------------------------------------------------------------------------------------------------------------
def test_planted_radius_graph_pairs_split_as_claimed():
    pairs = M.rg_planted_pairs()
    for name, (pi, pj) in pairs.items():
        assert len(pi) >= 6
        ku, kf, ke = M.rg_keep_unfused(pi, pj), M.rg_keep_fused(pi, pj), M.rg_keep_exact(pi, pj)
        d = np.sqrt(((pi.astype(np.float64) - pj.astype(np.float64)) ** 2).sum(-1))
        assert (np.abs(d / M.RG_RMAX - 1) < 4e-7).all()
        if name == "unfused_keeps_fused_drops":
            assert ku.all() and not kf.any()
        elif name == "unfused_drops_fused_keeps":
            assert kf.all() and not ku.any()
        elif name == "unfused_keeps_exact_drops":
            assert ku.all() and not ke.any()
        else:
            assert ke.all() and not ku.any()
    # the case's edge list depends on them: a fused or an exact distance test gives another one
    c = CASES["rg_planted"]
    inp = M.rg_inputs(c)
    counts, ei = M.rg_reference(inp)
    counts_f, _ = M.rg_reference(inp, keep=M.rg_keep_fused)
    assert (counts != counts_f).sum() >= 24
    on = np.flatnonzero((inp["pos"] == np.array([M.RG_RMAX, 0, 0], np.float32)).all(1))[0]
    assert not ((ei[0] == on) & (ei[1] == on - 1)).any()      # the pair exactly on the cutoff is dropped (strict <)
    # the pre-existing edges of rg_old_edges are beyond the cutoff and sit on the ballot seam
    c = CASES["rg_old_edges"]
    inp = M.rg_inputs(c)
    _, with_old = M.rg_reference(inp)
    _, without = M.rg_reference(dict(inp, old_ptr=None, old_dst=None))
    extra = set(map(tuple, with_old.T)) - set(map(tuple, without.T))
    assert {(5, 63), (5, 64)} <= extra and len(extra) >= 20
