"""The kernels csrc/e3k_layer.hip ships == the kernels tests/test_gpu_layer_matrix.py checks, and the route model of
tests/test_gpu_needs_matrix.py on the host (no GPU needed).

Reads the gfx950 code object of e3k_layer.o: a kernel added without a case, or a case table row for a kernel that no longer exists,
fails here.  The route model -- the pure-Python statement of e3k_layer_bwd's decisions the GPU cases are held to -- is run over one
hand-written argument tuple per branch, those no Python caller reaches included, and four deliberately wrong variants of it must
each disagree with it on one tuple or more: a model too coarse to tell them apart would also miss the executor getting it wrong."""
import os
import re
import subprocess

import pytest

from tests.test_gpu_layer_matrix import CASES as LAYER_CASES, table_kernels
from tests.test_gpu_needs_matrix import BRANCHES, CASE_IDS, FORMS, PATTERNS, REACHABLE, ROUTE_KEYS, UNREACHABLE, VARIANTS, route_model, shown_family

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAYER_OBJ = os.path.join(ROOT, "equivariant-nn-zoo_amd", "csrc", "e3k_layer.o")
LLVM = "/opt/rocm/llvm/bin"


def _tool(name):
    path = os.path.join(LLVM, name)
    return path if os.path.exists(path) else name


def _shipped_layer_kernels(tmp_path):
    if not os.path.exists(LAYER_OBJ):
        import __graft_entry__

        __graft_entry__.build()
    # --offloading writes one file per bundle beside the object it reads: a link to it in tmp_path keeps them out of the tree
    os.symlink(LAYER_OBJ, tmp_path / "e3k_layer.o")
    subprocess.run([_tool("llvm-objdump"), "--offloading", "e3k_layer.o"], check=True, cwd=tmp_path, capture_output=True)
    bundles = [p for p in os.listdir(tmp_path) if p.endswith("gfx950")]
    assert len(bundles) == 1, os.listdir(tmp_path)
    syms = subprocess.run([_tool("llvm-readelf"), "-sW", str(tmp_path / bundles[0])], check=True, capture_output=True, text=True).stdout
    names = [f[7] for f in (line.split() for line in syms.splitlines()) if len(f) >= 8 and f[3] == "FUNC" and f[4] == "GLOBAL"]
    demangled = subprocess.run(["c++filt"], input="\n".join(names), check=True, capture_output=True, text=True).stdout
    return {m.group(1) for m in re.finditer(r"e3k::([a-z_]+_kernel)\(", demangled)}


def test_every_layer_kernel_has_a_case(tmp_path):
    shipped = _shipped_layer_kernels(tmp_path)
    assert shipped == {"gather_rows_kernel", "scatter_rows_kernel", "zero_words_kernel"}, sorted(shipped)
    table = table_kernels()
    assert shipped - table == set(), f"kernels without a case in test_gpu_layer_matrix.CASES: {sorted(shipped - table)}"
    assert table - shipped == set(), f"the case table names kernels e3k_layer.o does not ship: {sorted(table - shipped)}"
    for k in shipped:
        assert any(k in c["kernels"] and c["rc"] == 0 for c in LAYER_CASES), f"{k}: only refusals name it"
    ids = [c["id"] for c in LAYER_CASES]
    assert len(ids) == len(set(ids))


def test_form_and_pattern_ids_are_unique():
    assert len(CASE_IDS) == len(set(CASE_IDS))
    pairs = [(c, p) for c in CASE_IDS for p in PATTERNS]
    assert len(pairs) == len(set(pairs)) == len(CASE_IDS) * len(PATTERNS)
    assert len(PATTERNS) == 15 and len(FORMS) == 8
    for form in FORMS:      # every form on one stream and forked
        assert {f"{form}-one_stream-autograd", f"{form}-fork-autograd"} <= set(CASE_IDS)
    for form in ("bench", "in_kernel", "per_edge"):
        assert {f"{form}-one_stream-sink", f"{form}-fork-sink"} <= set(CASE_IDS)
    assert "bench-fork_wgrad_on_main-autograd" in CASE_IDS and "bench-one_stream-autograd-lmax3" in CASE_IDS


def args(**over):
    """the middle layer of the bench form on one stream with everything trainable, one field at a time replaced"""
    a = dict(need_x=1, need_attrs=0, need_radial=0, gb_lin1=1, gb_post=1, gb_sc=0, gb_last=0, gb_hidden=0, have_m=2, gm=1, g_w=1, g_T=1,
             g_T_live=0, table_ws=1, x1=1, fuse_xw=1, side_is_main=1, side3_is_main=1, use_table=1, in_kernel=1, P=1, have_rows=1, w=0,
             E=742, w_live=0, narrow_form=None, has_sc=1, timed=0)
    assert set(over) <= set(a)
    a.update(over)
    assert set(a) == set(ROUTE_KEYS)
    return a


PER_EDGE = dict(use_table=0, in_kernel=0, P=0, w=1, g_T=0, table_ws=0)
FROZEN_RADIAL = dict(g_w=0, g_T=0, table_ws=0)
FORKED = dict(side_is_main=0, side3_is_main=0)
# (name, arguments, branch, the family the route record shows, stream of the weight-gradient pass / its event, transpose, fused launch)
TUPLES = [
    ("bench_one_stream", args(), "xw_ptable", "xw_ptable", "main", "rides", True),
    ("bench_forked", args(**FORKED), "xw_ptable", "xw_ptable", "main", "own", False),
    ("bench_forked_wgrads_on_main", args(side_is_main=0), "xw_ptable", "xw_ptable", "main", "own", False),
    ("bench_profiled", args(timed=1), "xw_ptable", "xw_ptable", "main", "own", False),
    ("scalar_head_layer", args(w_live=192, narrow_form="scalar", g_T_live=1), "scalar", "scalar", "main", "rides", True),
    ("masked_layer_below", args(w_live=704, narrow_form="masked", g_T_live=1), "masked", "masked", "main", "rides", True),
    ("narrow_with_own_radial_gradient", args(w_live=192, narrow_form="scalar", g_T_live=1, gb_last=1), "unsupported", None, None, None, False),
    ("narrow_without_compact_table_gradient", args(w_live=192, narrow_form="scalar"), "unsupported", None, None, None, False),
    ("narrow_with_frozen_radial", args(w_live=192, narrow_form="scalar", g_T_live=1, **FROZEN_RADIAL), "unsupported", None, None, None, False),
    ("frozen_node_side_rides_alone", args(gb_lin1=0, gb_post=0, gm=0), "xw_ptable", "xw_ptable", "main", "rides", False),
    ("per_edge_stack_one_stream", args(**PER_EDGE), "xw_streamed", "xw_streamed", "main", None, False),
    ("per_edge_own_mlp_one_stream", args(**PER_EDGE, have_rows=0, gb_last=1, gb_hidden=1), "xw_streamed", "xw_streamed", "main", None, False),
    ("per_edge_forked", args(**PER_EDGE, **FORKED, have_rows=0, gb_last=1), "x_stream>bwd_w", "bwd_w", "side", None, False),
    ("per_edge_frozen_radial", args(**dict(PER_EDGE, g_w=0), have_rows=0), "x_stream", "x_stream", None, None, False),
    ("packed_frozen_radial", args(**FROZEN_RADIAL), "x_ptable", "x_ptable", None, None, False),
    ("packed_unfused", args(fuse_xw=0), "x_ptable>bwd_w", "bwd_w", "main", "own", False),
    ("packed_unfused_forked", args(fuse_xw=0, **FORKED), "x_ptable>bwd_w", "bwd_w", "side", "own", False),
    ("unpacked_table_frozen_radial", args(P=0, **FROZEN_RADIAL), "x_table", "x_table", None, None, False),
    ("unpacked_table", args(P=0), "x_table>bwd_w", "bwd_w", "main", "own", False),
    ("own_radial_branch_in_kernel", args(have_rows=0, gb_last=1, gb_hidden=1), "xw_ptable", "xw_ptable", "main", "own", False),
    ("first_layer_radial_only", args(need_x=0, gb_lin1=0, gb_post=0, gm=0), "bwd_w", "bwd_w", "main", "own", False),
    ("first_layer_radial_only_forked", args(need_x=0, gb_lin1=0, gb_post=0, gm=0, **FORKED), "bwd_w", "bwd_w", "side", "own", False),
    ("first_layer_post_only", args(need_x=0, gb_lin1=0, gm=0, **FROZEN_RADIAL), "none", None, None, None, False),
    ("first_layer_lin1_only", args(need_x=0, gb_post=0, gm=0, **FROZEN_RADIAL), "x_ptable", "x_ptable", None, None, False),
    ("lin1_wanted_without_input_gradient", args(need_x=0), "xw_ptable", "xw_ptable", "main", "rides", True),
    ("no_edges", args(E=0), "x_ptable", "x_ptable", None, None, False),
    ("table_gradient_buffer_without_a_radial_side", args(have_rows=0), "x_ptable", "x_ptable", None, None, False),
    ("one_radial_stream_with_a_weight_gradient_stream", args(side3_is_main=0), "xw_ptable", "xw_ptable", "main", "own", False),
]


@pytest.mark.parametrize("name,a,branch,shows,wst,transpose,fused", TUPLES, ids=[t[0] for t in TUPLES])
def test_route_model_on_hand_written_arguments(name, a, branch, shows, wst, transpose, fused):
    r = route_model(a)
    assert (r.branch, r.shows, r.wst, r.transpose, r.fused_launch) == (branch, shows, wst, transpose, fused), r
    assert "branch:" + branch in r.labels


def test_the_tuples_reach_every_branch_of_the_model():
    reached = {t[2] for t in TUPLES}
    assert reached == set(BRANCHES), sorted(set(BRANCHES) ^ reached)
    assert set(UNREACHABLE) < set(BRANCHES) and all(UNREACHABLE.values())
    labels = set().union(*[route_model(t[1]).labels for t in TUPLES])
    assert {l for l in REACHABLE if l.startswith("branch:")} <= labels
    assert {"bwd_w@side", "bwd_w@main", "transpose:rides+wgrad", "transpose:rides_alone", "transpose:own", "radial:last", "radial:hidden",
            "wgrads:early", "wgrads:late_lin1", "wgrads:one_call", "kw:gm"} <= labels
    own = route_model(args(have_m=0, gm=0, gb_sc=1, need_attrs=1)).labels
    assert {"kw:own", "attrs:scatter"} <= own and "kw:gm" not in own


@pytest.mark.parametrize("variant", VARIANTS)
def test_a_wrong_model_disagrees_somewhere(variant):
    differ = [t[0] for t in TUPLES if route_model(t[1], variant)[:5] != route_model(t[1])[:5]]
    print(variant, "disagrees on", differ)
    assert differ, f"no hand-written tuple tells the model from its variant {variant}"
    want = {"ride_without_side3": "one_radial_stream_with_a_weight_gradient_stream",
            "fused_xw_without_radial_side": "table_gradient_buffer_without_a_radial_side",
            "wst_ignores_fused_xw": "bench_forked", "need_x1_is_need_x": "lin1_wanted_without_input_gradient"}[variant]
    assert want in differ


def test_route_record_families():
    assert shown_family(None) is None
    assert shown_family("tp_bwd_xw_scalar_kernel") == "scalar" and shown_family("tp_bwd_xw_masked_kernel") == "masked"
    assert shown_family("tp_bwd_w_kernel<false, 2, 2, false, true>") == "bwd_w"
    for mode, fam in ((0, "x_stream"), (1, "x_table"), (4, "x_ptable"), (5, "xw_ptable"), (6, "xw_streamed")):
        assert shown_family(f"tp_bwd_x_kernel<2, 2, false, true, {mode}>") == fam
    assert shown_family("tp_fwd_kernel<2, 2, false, true, 4>") not in BRANCHES
