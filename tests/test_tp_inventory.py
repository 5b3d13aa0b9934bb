"""The tensor-product kernels the library ships == the kernels tests/test_gpu_tp_matrix.py checks against float64 (no GPU needed).

Reads the gfx950 code object of e3k_tp.o: a kernel added without a float64-checked case, or a case table row for a kernel that no
longer exists, fails here."""
import os
import re
import subprocess

import pytest

from tests.test_gpu_tp_matrix import CASES, table_routes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TP_OBJ = os.path.join(ROOT, "equivariant-nn-zoo_amd", "csrc", "e3k_tp.o")
LLVM = "/opt/rocm/llvm/bin"


def _tool(name):
    path = os.path.join(LLVM, name)
    return path if os.path.exists(path) else name


def _shipped_tp_kernels(tmp_path):
    if not os.path.exists(TP_OBJ):
        import __graft_entry__

        __graft_entry__.build()
    # --offloading writes one file per bundle beside the object it reads: a link to it in tmp_path keeps them out of the tree
    os.symlink(TP_OBJ, tmp_path / "e3k_tp.o")
    subprocess.run([_tool("llvm-objdump"), "--offloading", "e3k_tp.o"], check=True, cwd=tmp_path, capture_output=True)
    bundles = [p for p in os.listdir(tmp_path) if p.endswith("gfx950")]
    assert len(bundles) == 1, os.listdir(tmp_path)
    syms = subprocess.run([_tool("llvm-readelf"), "-sW", str(tmp_path / bundles[0])], check=True, capture_output=True,
                          text=True).stdout
    names = [f[7] for f in (line.split() for line in syms.splitlines()) if len(f) >= 8 and f[3] == "FUNC" and f[4] == "GLOBAL"]
    demangled = subprocess.run(["c++filt"], input="\n".join(names), check=True, capture_output=True, text=True).stdout
    return {m.group(1) for m in re.finditer(r"e3k::(tp_[a-z_]+_kernel<[^>]*>)", demangled)}


def test_every_tp_kernel_has_a_float64_checked_case(tmp_path):
    shipped = _shipped_tp_kernels(tmp_path)
    table = table_routes()
    assert len(shipped) == 174, len(shipped)      # 231 before the unreachable unsplit channel-complete l3 <= 3 forms went
    assert shipped - table == set(), f"kernels without a case in test_gpu_tp_matrix.CASES: {sorted(shipped - table)}"
    assert table - shipped == set(), f"case table routes to kernels the library does not ship: {sorted(table - shipped)}"


def test_case_table_covers_every_reachable_cell():
    """Every (MAXL, L3MAX, SPLIT, FULL) cell launch_all can reach, once or more; and the ids are unique."""
    cells = {c["cell"] for c in CASES}
    full = {(0, 0, False), (0, 3, False), (1, 1, False), (2, 2, False), (1, 3, True), (2, 3, True), (3, 3, True)}
    partial = {(0, 0, False), (0, 3, False), (1, 1, False), (1, 3, False), (1, 3, True), (2, 2, False), (2, 3, False), (2, 3, True),
               (3, 3, False), (3, 3, True)}
    assert cells == {c + (True,) for c in full} | {c + (False,) for c in partial}
    ids = [c["id"] for c in CASES]
    assert len(ids) == len(set(ids))


@pytest.mark.parametrize("maxl", [1, 2, 3])
def test_channel_complete_plans_with_outputs_to_three_are_split(maxl):
    """Why launch_all has no unsplit channel-complete kernel with outputs up to degree 3 and an input degree >= 1: every slot of
    such a group is enabled, which is more than the 24 accumulators of one wave (e3k_tp_plan_create's kSplitAcc)."""
    from e3_layers_amd.nn.core import tp_slots

    assert sum(2 * l3 + 1 for _, l3 in tp_slots(maxl)) > 24
