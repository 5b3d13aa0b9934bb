"""The C ABI: libe3k.so loads (no GPU needed), exports every symbol include/e3k.h declares, and the
ctypes mirror derived from that header (backend/abi.py -> backend/lib.py) has the layout the C compiler gives every struct.  No
compute calls."""
import ctypes as C
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "e3k.h")


def _declared_functions():
    text = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(e3k_[a-z0-9_]+)\s*\(", text)))


def test_library_exports_every_declared_symbol():
    from e3_layers_amd.backend import abi
    from e3_layers_amd.backend import lib as L

    if not os.path.exists(L.LIB_PATH):
        import __graft_entry__

        __graft_entry__.build()
    handle = L.load()
    names = _declared_functions()
    assert len(names) >= 25
    assert sorted(abi.load().functions) == names      # two independent readings of the header
    for name in names:
        assert hasattr(handle, name), f"{name} declared in include/e3k.h but not exported by libe3k.so"
        assert name in L.SIGNATURES, f"{name} has no ctypes signature in backend/lib.py"
    assert handle.e3k_strerror(-3).decode().startswith("degree")
    assert handle.e3k_version() >= 100


def test_every_c_entry_has_one_python_launch_site():
    """Each ``e3k_*`` function is called from ONE place in the package; everything else goes through that function, so an argument
    list is never written twice.  The sources are read as text: nothing of the package is compiled or imported."""
    pkg = os.path.join(ROOT, "equivariant-nn-zoo_amd", "e3_layers_amd")
    sites = {}
    for base, _, files in os.walk(pkg):
        for f in sorted(files):
            if f.endswith(".py"):
                path = os.path.join(base, f)
                for m in re.finditer(r"\.(e3k_[a-z0-9_]+)\(", open(path).read()):
                    sites.setdefault(m.group(1), []).append(os.path.relpath(path, pkg))
    assert len(sites) >= 100 and set(sites) <= set(_declared_functions()), sorted(set(sites) - set(_declared_functions()))
    assert {name: where for name, where in sites.items() if len(where) != 1} == {}


def test_struct_layouts_match_the_c_compiler(tmp_path):
    """sizeof of every struct of the header, offsetof and sizeof of every field: the C compiler against the derived mirror."""
    from e3_layers_amd.backend import abi
    from e3_layers_amd.backend import lib as L

    structs = abi.load().structs
    assert len(structs) >= 17
    want, lines = [], []
    for name, fields in structs.items():
        cls = getattr(L, "".join(w.capitalize() for w in name[len("e3k_"):].split("_")))
        assert [f for f, _ in cls._fields_] == [f for f, _, _ in fields]
        lines.append(f'printf("%zu\\n", sizeof({name}));')
        want.append((name, C.sizeof(cls)))
        for f, _, _ in fields:
            lines.append(f'printf("%zu %zu\\n", offsetof({name}, {f}), sizeof((({name}*)0)->{f}));')
            want += [(f"offsetof({name}, {f})", getattr(cls, f).offset), (f"sizeof({name}.{f})", getattr(cls, f).size)]
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "e3k.h"\nint main(void){\n' + "\n".join(lines) + "\nreturn 0;}\n")
    exe = tmp_path / "sizes"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert len(got) == len(want)
    assert [(what, v) for (what, _), v in zip(want, got)] == want


def test_pinned_signatures_and_fields():
    """A handful of expectations written out by hand, so that a parser bug cannot agree with itself."""
    from e3_layers_amd.backend import lib as L

    P, I32, I64, F = C.c_void_p, C.c_int32, C.c_int64, C.c_float
    assert L.SIGNATURES["e3k_sampler_ode_div"] == (C.c_int, [P, P, P, P, P, I64, P, I64, I32, I32, I32, C.c_double, F, F, P])
    assert L.SIGNATURES["e3k_slope_tangent_bwd"] == (C.c_int, [P, I32, I32, P, P, I64, P, I32, I32, F, F, F, I32, I32, I32, F, P, P, P, P, P])
    assert len(L.SIGNATURES["e3k_slope_tangent_bwd"][1]) == 21
    assert L.SIGNATURES["e3k_layer_create"] == (C.c_int, [C.POINTER(L.LayerDesc), P])
    assert L.SIGNATURES["e3k_strerror"] == (C.c_char_p, [C.c_int])
    assert L.SIGNATURES["e3k_layer_destroy"] == (None, [P])
    assert L.SIGNATURES["e3k_collate_work_ints"] == (I64, [I32])
    assert dict(L.LayerFwdArgs._fields_)["rad"] is L.LayerRadial
    assert dict(L.LayerFwdArgs._fields_)["next_rad"] is C.POINTER(L.LayerRadial)
    assert dict(L.LayerFwdArgs._fields_)["next"] is P
    assert dict(L.LayerDesc._fields_)["live_col"] is I32 * 48 and L.NARROW_MAX_SLOTS == 48
    assert dict(L.TpGroup._fields_)["y_off"] is I32 * 4
    assert dict(L.TpGroup._fields_)["coeff"] is F * 8 and dict(L.TpGroup._fields_)["mask"] is C.c_uint32
    assert L.DEFINES["E3K_ERR_UNSUPPORTED"] == -3 and L.DEFINES["E3K_COLLATE_MAX_FIELDS"] == 16 and "E3K_GEMM_MAX_ROWS" not in L.DEFINES


_SMALL = """
/* a comment with int bogus(unknown_t x); inside */
#ifndef SMALL_H
#define SMALL_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
#define E3K_N 3 /* literal */
#define E3K_NEG (-2)
#define E3K_EXPR ((1LL << 31) - 1)
typedef struct e3k_handle e3k_handle;
typedef struct {
  const float* a;
  float const* b;
  void *main, *side;
  int32_t n_kw, V;
  const float* const* w_hidden;
  float* z[4];
  uint8_t flags[E3K_N];
  int64_t big; uint32_t mask; double acc; int plain;
  const e3k_handle* h;
} e3k_inner;
typedef struct {
  e3k_inner one, two;
  const e3k_inner* ptr;
  e3k_inner arr[2];
} e3k_outer;
const char* e3k_name(int code);
void e3k_free(e3k_handle* h);
int e3k_version(void);
int64_t e3k_run(const e3k_outer* o, e3k_handle** out, const e3k_handle* const* hs, float* const* z,
                uint32_t seed, double scale, void* stream);
#ifdef __cplusplus
}
#endif
#endif
"""


def test_parser_reads_every_construct_of_the_subset():
    from e3_layers_amd.backend import abi

    h = abi.parse(_SMALL)
    assert h.defines == {"E3K_N": 3, "E3K_NEG": -2}
    assert h.opaque == ["e3k_handle"]
    assert list(h.structs) == ["e3k_inner", "e3k_outer"]
    assert h.structs["e3k_inner"] == [
        ("a", ("float", 1), None), ("b", ("float", 1), None), ("main", ("void", 1), None), ("side", ("void", 1), None),
        ("n_kw", ("int32_t", 0), None), ("V", ("int32_t", 0), None), ("w_hidden", ("float", 2), None), ("z", ("float", 1), 4),
        ("flags", ("uint8_t", 0), 3), ("big", ("int64_t", 0), None), ("mask", ("uint32_t", 0), None), ("acc", ("double", 0), None),
        ("plain", ("int", 0), None), ("h", ("e3k_handle", 1), None)]
    assert h.structs["e3k_outer"] == [("one", ("e3k_inner", 0), None), ("two", ("e3k_inner", 0), None), ("ptr", ("e3k_inner", 1), None),
                                      ("arr", ("e3k_inner", 0), 2)]
    assert h.functions == {
        "e3k_name": (("char", 1), [("int", 0)]),
        "e3k_free": (("void", 0), [("e3k_handle", 1)]),
        "e3k_version": (("int", 0), []),
        "e3k_run": (("int64_t", 0), [("e3k_outer", 1), ("e3k_handle", 2), ("e3k_handle", 2), ("float", 2), ("uint32_t", 0), ("double", 0),
                                     ("void", 1)])}


@pytest.mark.parametrize("bad, names", [
    ("int e3k_f(size_t n);", "size_t"),                                                   # unknown type
    ("int e3k_f(int (*cb)(int));", "(*cb)"),                                              # function pointer
    ("typedef struct { void (*cb)(void); } e3k_s;", "(*cb)"),
    ("int e3k_f(int a);\nint e3k_global\n", "e3k_global"),                              # left-over text
    ("int e3k_f(int a); }", "}"),
    ("typedef struct { int32_t a[E3K_MISSING]; } e3k_s;", "E3K_MISSING"),                 # array sized by an undefined name
    ("typedef struct { int32_t a : 3; } e3k_s;", "a : 3"),                                # bit-field
    ("typedef union { int32_t a; float b; } e3k_u;", "union"),
    ("typedef enum { E3K_A, E3K_B } e3k_e;", "enum"),
    ("typedef struct { struct { int a; } in; } e3k_s;", "struct"),                        # nested body
    ("#if 1\nint e3k_f(int a);\n#endif", "#if 1"),
    ("#define E3K_SQ(x) ((x) * (x))", "E3K_SQ"),
    ("typedef struct e3k_h e3k_h;\nint e3k_f(e3k_h h);", "e3k_h"),                       # opaque by value
    ("typedef struct { void v; } e3k_s;", "void"),
    ("typedef struct { e3k_later l; } e3k_s;\ntypedef struct { int a; } e3k_later;", "e3k_later"),
    ("int e3k_f(int a[4]);", "e3k_f"),
])
def test_parser_raises_on_anything_outside_the_subset(bad, names):
    from e3_layers_amd.backend import abi

    good = "#ifndef X_H\n#define X_H\n%s\n#endif\n"
    assert abi.parse(good % "int e3k_f(int a);").functions == {"e3k_f": (("int", 0), [("int", 0)])}
    with pytest.raises(abi.HeaderError) as err:
        abi.parse(good % bad)
    assert names in str(err.value)


def test_a_missing_header_is_named():
    from e3_layers_amd.backend import abi

    with pytest.raises(FileNotFoundError, match="no_such_dir/e3k.h"):
        abi.load("/no_such_dir/e3k.h")


def test_limits_agree_with_generated_header():
    gen = open(os.path.join(ROOT, "equivariant-nn-zoo_amd", "csrc", "e3k_cg_gen.h")).read()
    vals = {k: int(v) for k, v in re.findall(r"#define (E3K_L[123]MAX|E3K_MAXQ) (\d+)", gen)}
    from e3_layers_amd.backend import lib as L
    from e3_layers_amd.nn import core

    assert (vals["E3K_L1MAX"], vals["E3K_L2MAX"], vals["E3K_L3MAX"]) == (core.TP_L1MAX, core.TP_L2MAX, core.TP_L3MAX)
    assert vals["E3K_MAXQ"] == L.TP_MAXQ
    for l1 in range(core.TP_L1MAX + 1):
        m = re.search(r"struct Slots<%d> \{.*?L2\[\d+\] = \{([^}]*)\};.*?L3\[\d+\] = \{([^}]*)\};" % l1, gen, re.S)
        l2s = [int(v) for v in m.group(1).split(",")]
        l3s = [int(v) for v in m.group(2).split(",")]
        assert list(zip(l2s, l3s)) == core.tp_slots(l1)


def test_product_path_has_no_oracle_import():
    """The shipped package must never import the oracle (or the reference)."""
    pkg = os.path.join(ROOT, "equivariant-nn-zoo_amd")
    for base, _, files in os.walk(pkg):
        for f in files:
            if f.endswith(".py"):
                text = open(os.path.join(base, f)).read()
                assert not re.search(r"^\s*(from|import)\s+oracle\b", text, re.M), os.path.join(base, f)
                assert "/root/reference" not in text, os.path.join(base, f)


def test_switches_live_in_one_table_and_the_library_has_no_environment_knobs():
    """the C library's tuning constants are compile-time constants (one build, no environment read, no debug-knob
    switch), and the Python package reads the environment in backend/tuning.py only -- every knob it reads is documented there."""
    import re

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    csrc = os.path.join(root, "equivariant-nn-zoo_amd", "csrc")
    for fn in sorted(os.listdir(csrc)):
        if not fn.endswith((".hip", ".h")):
            continue
        text = open(os.path.join(csrc, fn)).read()
        for word in ("getenv", "E3K_DEBUG_KNOBS", "E3K_KNOB_INT"):
            assert word not in text, (fn, word)
    pkg = os.path.join(root, "equivariant-nn-zoo_amd", "e3_layers_amd")
    used = set()
    for dirpath, _, files in os.walk(pkg):
        for fn in files:
            if not fn.endswith(".py"):
                continue
            text = open(os.path.join(dirpath, fn)).read()
            if fn != "tuning.py":
                assert "os.environ" not in text and "getenv" not in text, os.path.join(dirpath, fn)
            used |= set(re.findall(r'_knob\("(E3K_[A-Z0-9_]+)"\)', text))
    sys.path.insert(0, os.path.join(root, "equivariant-nn-zoo_amd"))
    from e3_layers_amd.backend import tuning

    assert used and used <= set(tuning.KNOBS), used - set(tuning.KNOBS)
    assert set(tuning.KNOBS) - used == set(), set(tuning.KNOBS) - used      # no documented knob that nothing reads
    assert all(len(doc) > 10 and kind in ("path", "threshold", "accuracy", "debug") for _, kind, doc in tuning.KNOBS.values())
