"""The GEMM-family kernels the library ships == the routes of tests/test_gpu_gemm_matrix.py's cases (no GPU needed).

Reads the gfx950 code object of e3k_gemm.o: a kernel added without a float64-checked case, or a case whose route names a kernel that
no longer exists, fails here.  (zero_words_kernel comes from e3k_common.h and is not a GEMM kernel.)"""
import os
import re
import subprocess

from tests.test_gpu_gemm_matrix import CASES, table_routes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GEMM_OBJ = os.path.join(ROOT, "equivariant-nn-zoo_amd", "csrc", "e3k_gemm.o")
LLVM = "/opt/rocm/llvm/bin"


def _tool(name):
    path = os.path.join(LLVM, name)
    return path if os.path.exists(path) else name


def _shipped_gemm_kernels(tmp_path):
    if not os.path.exists(GEMM_OBJ):
        import __graft_entry__

        __graft_entry__.build()
    # --offloading writes one file per bundle beside the object it reads: a link to it in tmp_path keeps them out of the tree
    os.symlink(GEMM_OBJ, tmp_path / "e3k_gemm.o")
    subprocess.run([_tool("llvm-objdump"), "--offloading", "e3k_gemm.o"], check=True, cwd=tmp_path, capture_output=True)
    bundles = [p for p in os.listdir(tmp_path) if p.endswith("gfx950")]
    assert len(bundles) == 1, os.listdir(tmp_path)
    syms = subprocess.run([_tool("llvm-readelf"), "-sW", str(tmp_path / bundles[0])], check=True, capture_output=True,
                          text=True).stdout
    names = [f[7] for f in (line.split() for line in syms.splitlines()) if len(f) >= 8 and f[3] == "FUNC" and f[4] == "GLOBAL"]
    demangled = subprocess.run(["c++filt"], input="\n".join(names), check=True, capture_output=True, text=True).stdout
    return {m.group(1) for m in re.finditer(r"e3k::((?:gemm_|colsum|wgrad_n1|fctp_reduce)[a-z0-9_]*(?:<[^>]*>)?)", demangled)}


def test_every_gemm_kernel_has_a_float64_checked_case(tmp_path):
    shipped = _shipped_gemm_kernels(tmp_path)
    table = table_routes()
    assert len(shipped) == 17, sorted(shipped)      # 19 before the two 128-row gemm_kernel<4, *> forms went
    assert shipped - table == set(), f"kernels without a case in test_gpu_gemm_matrix.CASES: {sorted(shipped - table)}"
    assert table - shipped == set(), f"case table routes to kernels the library does not ship: {sorted(table - shipped)}"


def test_case_ids_are_unique():
    ids = [c["id"] for c in CASES]
    assert len(ids) == len(set(ids))
