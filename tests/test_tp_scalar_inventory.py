"""The kernels e3k_tp_scalar.o ships == the kernels tests/test_gpu_tp_scalar_matrix.py checks against float64 (no GPU needed).

Reads the gfx950 code object of the object file: a kernel added without a checked case, or a case naming a kernel that no longer
exists, fails here."""
import os
import re
import subprocess

from tests.test_gpu_tp_scalar_matrix import CASES, EXPAND_CASES, KERNELS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OBJ = os.path.join(ROOT, "equivariant-nn-zoo_amd", "csrc", "e3k_tp_scalar.o")
LLVM = "/opt/rocm/llvm/bin"


def _tool(name):
    path = os.path.join(LLVM, name)
    return path if os.path.exists(path) else name


def _shipped_kernels(tmp_path):
    if not os.path.exists(OBJ):
        import __graft_entry__

        __graft_entry__.build()
    # --offloading writes one file per bundle beside the object it reads: a link to it in tmp_path keeps them out of the tree
    os.symlink(OBJ, tmp_path / "e3k_tp_scalar.o")
    subprocess.run([_tool("llvm-objdump"), "--offloading", "e3k_tp_scalar.o"], check=True, cwd=tmp_path, capture_output=True)
    bundles = [p for p in os.listdir(tmp_path) if p.endswith("gfx950")]
    assert len(bundles) == 1, os.listdir(tmp_path)
    syms = subprocess.run([_tool("llvm-readelf"), "-sW", str(tmp_path / bundles[0])], check=True, capture_output=True,
                          text=True).stdout
    names = [f[7] for f in (line.split() for line in syms.splitlines()) if len(f) >= 8 and f[3] == "FUNC" and f[4] in ("GLOBAL", "LOCAL")]
    demangled = subprocess.run(["c++filt"], input="\n".join(names), check=True, capture_output=True, text=True).stdout
    return {m.group(1) for m in re.finditer(r"(?:e3k::)?([a-z_0-9]+_kernel)\b", demangled)}


def test_every_kernel_of_the_object_has_a_checked_case(tmp_path):
    shipped = _shipped_kernels(tmp_path) - {"zero_words_kernel"}      # (e3k_common.h's helper, instantiated where an object fills)
    assert shipped == KERNELS, (sorted(shipped - KERNELS), sorted(KERNELS - shipped))
    assert len(shipped) == 2


def test_case_tables_are_well_formed():
    ids = [c["id"] for c in CASES + EXPAND_CASES]
    assert len(ids) == len(set(ids))
    # both work orders, a two-chunk group, the single-group plans of the lowest and the highest input degree
    assert {c["n"] for c in CASES} == {37, 203}
    assert any("128x" in c["left"] for c in CASES) and {"64x0e", "64x2e"} <= {c["left"] for c in CASES}
