"""The knot-table kernels the library ships == the kernels tests/test_gpu_rtable_matrix.py's cases name (no GPU needed), and the
bounds of that file shown to hold for float32 models of the kernels' arithmetic on the CPU.

Reads the gfx950 code object of e3k_rtable.o: a kernel added without a float64-checked case, or a case naming a kernel that no longer
exists, fails here; so does a knot-table function of include/e3k.h that no case calls."""
import os
import re
import subprocess

import numpy as np

from tests.test_gpu_rtable_matrix import CASES, U24, bins_reference, check_record, smooth_table, table_functions, table_kernels, taylor64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RTABLE_OBJ = os.path.join(ROOT, "equivariant-nn-zoo_amd", "csrc", "e3k_rtable.o")
HEADER = os.path.join(ROOT, "include", "e3k.h")
LLVM = "/opt/rocm/llvm/bin"


def _tool(name):
    path = os.path.join(LLVM, name)
    return path if os.path.exists(path) else name


def _shipped_rtable_kernels(tmp_path):
    if not os.path.exists(RTABLE_OBJ):
        import __graft_entry__

        __graft_entry__.build()
    # --offloading writes one file per bundle beside the object it reads: a link to it in tmp_path keeps them out of the tree
    os.symlink(RTABLE_OBJ, tmp_path / "e3k_rtable.o")
    subprocess.run([_tool("llvm-objdump"), "--offloading", "e3k_rtable.o"], check=True, cwd=tmp_path, capture_output=True)
    bundles = [p for p in os.listdir(tmp_path) if p.endswith("gfx950")]
    assert len(bundles) == 1, os.listdir(tmp_path)
    syms = subprocess.run([_tool("llvm-readelf"), "-sW", str(tmp_path / bundles[0])], check=True, capture_output=True,
                          text=True).stdout
    names = [f[7] for f in (line.split() for line in syms.splitlines()) if len(f) >= 8 and f[3] == "FUNC" and f[4] == "GLOBAL"]
    demangled = subprocess.run(["c++filt"], input="\n".join(names), check=True, capture_output=True, text=True).stdout
    return {m.group(1) for m in re.finditer(r"e3k::(rtable_[a-z0-9_]*)", demangled)}


def test_every_rtable_kernel_has_a_float64_checked_case(tmp_path):
    shipped = _shipped_rtable_kernels(tmp_path)
    table = table_kernels()
    assert len(shipped) == 11, sorted(shipped)
    assert shipped - table == set(), f"kernels without a case in test_gpu_rtable_matrix.CASES: {sorted(shipped - table)}"
    assert table - shipped == set(), f"the case table names kernels the library does not ship: {sorted(table - shipped)}"


def test_every_rtable_function_of_the_header_is_called_by_a_case():
    with open(HEADER) as f:
        declared = set(re.findall(r"\b(e3k_rtable_\w+|e3k_edge_records)\s*\(", f.read()))
    assert len(declared) == 12, sorted(declared)
    called = table_functions()
    assert declared - called == set(), f"declared in include/e3k.h, called by no case: {sorted(declared - called)}"
    assert called - declared == set(), f"cases call functions the header does not declare: {sorted(called - declared)}"


def test_case_ids_are_unique():
    ids = [c["id"] for c in CASES]
    assert len(ids) == len(set(ids))
    assert all(c["why"] for c in CASES)


def _coef_model32(r32, h_inv, K):
    """e3k::rtable_bins_rank_kernel's per-edge arithmetic, operation for operation, in numpy float32"""
    f = np.float32
    with np.errstate(over="ignore"):      # (3e38 h_inv = +inf, as on the device)
        x = np.minimum(np.maximum(r32 * f(h_inv), f(0)), f(K))
    i = np.clip(x.astype(np.int32), 1, K - 2)
    t = x - i.astype(f)
    tm1, tm2, tp1 = t - f(1), t - f(2), t + f(1)
    c = np.stack([-t * tm1 * tm2 * f(1.0 / 6.0), tp1 * tm1 * tm2 * f(0.5), -tp1 * t * tm2 * f(0.5), tp1 * t * tm1 * f(1.0 / 6.0)], -1)
    assert c.dtype == np.float32
    return i, c


def test_coef_bound_holds_for_a_float32_model():
    """8 u |c64| (+ 2^-25 |dc/dt| where x - i rounds) against float64 from r itself, over 2 * 10^6 radii and the edge values"""
    rng = np.random.default_rng(5)
    for h_inv, K in ((128.0, 512), (7.3, 64), (1.0, 4)):
        h = 1.0 / h_inv
        r = np.concatenate([rng.uniform(0.0, 1.05 * K * h, 1_000_000), rng.uniform(0.0, 1.5 * h, 500_000), 10.0 ** rng.uniform(-9, 0, 500_000),
                            np.arange(K + 1) * h, [0.0, -1.0, 1e-7, 0.25 * h, 0.5 * h, np.nextafter(np.float32(K * h), np.float32(0)), 2 * K * h,
                                                   np.inf]]).astype(np.float32)
        i32, c32 = _coef_model32(r, h_inv, K)
        i64, c64, bound, nan = bins_reference(r, h_inv, K)
        assert not nan.any() and np.array_equal(i32, i64)
        err = np.abs(c32.astype(np.float64) - c64)
        assert (err <= bound).all(), (h_inv, float((err / np.maximum(bound, 1e-300)).max()))
        assert (c32[c64 == 0] == 0).all()
        exact = bound == 8 * U24 * np.abs(c64)
        ratio = float((err[exact & (c64 != 0)] / bound[exact & (c64 != 0)]).max())
        assert 0.05 < ratio <= 1.0, ratio      # (a bound the model does not come near would catch no one-term error)


def _pack_model(T32, K):
    """e3k::rtable_pack_kernel's arithmetic in numpy: float64 from the fp32 rows, halves through float32, d0 / d1 rounded once"""
    W = T32.shape[1]
    b, c1, c2, c3, e2, _ = taylor64(T32, K)
    hx = (e2 * 1024.0).astype(np.float32).astype(np.float16)
    hy = (c3 * 65536.0).astype(np.float32).astype(np.float16)
    r2, r3 = e2 - hx.astype(np.float64) / 1024.0, c3 - hy.astype(np.float64) / 65536.0
    d0 = (b + c1 / 2 + c2 / 4 + c3 / 8 + r2 / 8).astype(np.float32)
    d1 = (c1 + c2 + 0.75 * c3 + 3.0 * r3 / 16).astype(np.float32)
    P = np.zeros((K + 1, 3 * W), np.uint32)
    P[1:K - 1, 0:2 * W:2] = d0.view(np.uint32)
    P[1:K - 1, 1:2 * W:2] = d1.view(np.uint32)
    P[1:K - 1, 2 * W:] = hx.view(np.uint16).astype(np.uint32) | (hy.view(np.uint16).astype(np.uint32) << 16)
    return P.ravel()


def test_packed_record_bound_holds_for_the_reference_construction():
    """2^-11 (|e2| / 8 + |c3| / 32) + u (|d0| + |d1| / 2) (+ the subnormal terms; the clamped intervals' wider form) on the smooth
    table, for the record built in numpy: the bound holds without a GPU, and is nearly reached (no room for a dropped term)"""
    for K, W, amp in ((256, 64, 1.0), (64, 24, 1e-2), (4, 5, 1.0)):
        T = smooth_table(K, W, amp)
        stored, promise = check_record(_pack_model(T, K), T, K, W)
        assert stored <= 1.0 and promise <= 1.0
        if K == 256:
            assert promise > 0.5, promise
