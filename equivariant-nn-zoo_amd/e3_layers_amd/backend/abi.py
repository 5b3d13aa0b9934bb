"""``include/e3k.h`` as data: the one place the C interface is written down.

``backend/lib.py`` builds its ctypes mirror from what ``load()`` returns, and the tests generate their layout program from
it.  Pure Python: no torch, nothing from the package, no ``libe3k.so``.

The parser knows exactly the C subset the header names at its top and is strict about it: a construct outside the subset
raises ``HeaderError`` with the offending text, and whatever is left once comments, preprocessor lines, the ``extern "C"``
braces, typedefs and prototypes are taken out must be whitespace.  A type is ``(base, pointer depth)``; ``const`` is
dropped, it is no part of the binary interface.
"""
from __future__ import annotations

import functools
import os
import re
from typing import Dict, List, NamedTuple, Optional, Tuple

HEADER_PATH = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..", "..", "include", "e3k.h"))
SCALARS = ("int", "int32_t", "uint32_t", "int64_t", "uint8_t", "float", "double")

Type = Tuple[str, int]
Field = Tuple[str, Type, Optional[int]]


class HeaderError(ValueError):
    pass


class Header(NamedTuple):
    defines: Dict[str, int]                            # #define E3K_NAME <integer literal>
    structs: Dict[str, List[Field]]                    # typedef struct { ... } name;  -> [(field, type, array length or None)]
    opaque: List[str]                                  # typedef struct name name;
    functions: Dict[str, Tuple[Type, List[Type]]]      # name -> (return type, argument types)


_EXTERN_C = (r'#ifdef __cplusplus\s*extern "C" \{\s*#endif', r"#ifdef __cplusplus\s*\}\s*#endif")
_DEFINE = re.compile(r"#define\s+(\w+)(\(?)(.*)$")
_INT = re.compile(r"\(\s*(-?\d+)\s*\)$|(-?\d+)$")
_BASE = re.compile(r"(?:const\s+)?(\w+)(?:\s+const\b)?(.*)$", re.S)
_DECLARATOR = re.compile(r"((?:\*\s*(?:const\b\s*)?)*)(\w*)\s*(?:\[\s*(\w+)\s*\])?$")
_OPAQUE = re.compile(r"\btypedef\s+struct\s+(\w+)\s+\1\s*;")
_STRUCT = re.compile(r"\btypedef\s+struct\s*\{([^{}]*)\}\s*(\w+)\s*;")
_PROTOTYPE = re.compile(r"(.*?)\b(\w+)\s*\((.*)\)$", re.S)


def _declaration(text: str, by_value: Dict[str, bool], defines: Dict[str, int]) -> List[Field]:
    """``[const] base [const] declarator {, declarator}``, a declarator being ``{* [const]} [name] [[length]]``.
    ``by_value``: the non-scalar bases known so far, and whether one may stand without a ``*``."""
    text = text.strip()
    m = _BASE.match(text)
    base = m.group(1) if m else ""
    if base not in SCALARS and base not in by_value:
        raise HeaderError(f"unknown type in {text!r}")
    fields = []
    for part in m.group(2).split(","):
        d = _DECLARATOR.match(part.strip())
        if not d:
            raise HeaderError(f"cannot parse the declarator {part.strip()!r} of {text!r}")
        stars, name, length = d.groups()
        if not stars and not by_value.get(base, True):
            raise HeaderError(f"{base} without a * in {text!r}")
        if length is not None and not length.isdigit() and length not in defines:
            raise HeaderError(f"array sized by the undefined name {length} in {text!r}")
        fields.append((name, (base, stars.count("*")), None if length is None else int(defines.get(length, length))))
    return fields


def parse(text: str) -> Header:
    text = re.sub(r"/\*.*?\*/|//[^\n]*", lambda m: " " + "\n" * m.group().count("\n"), text, flags=re.S)
    for idiom in _EXTERN_C:
        text = re.sub(idiom, " ", text, count=1)

    defines: Dict[str, int] = {}
    lines = text.split("\n")
    directives = [i for i, line in enumerate(lines) if line.lstrip().startswith("#")]
    for i in directives:
        line = lines[i].strip()
        m = _DEFINE.match(line)
        if m and not m.group(2):
            value = _INT.match(m.group(3).strip())      # (an expression body, or none: skipped)
            if value:
                defines[m.group(1)] = int(value.group(1) or value.group(2))
        elif not (re.match(r"#include\s*<[\w./]+>$", line) or (i == directives[0] and re.match(r"#ifndef\s+\w+$", line))
                  or (i == directives[-1] and line == "#endif")):
            raise HeaderError(f"preprocessor line outside the parsed subset: {line!r}")
        lines[i] = ""
    text = "\n".join(lines)

    by_value = {"void": False, "char": False}
    opaque = _OPAQUE.findall(text)
    by_value.update(dict.fromkeys(opaque, False))
    text = _OPAQUE.sub(" ", text)

    structs: Dict[str, List[Field]] = {}
    for m in _STRUCT.finditer(text):                    # (header order: a struct by value must be defined above its user)
        fields = [f for line in m.group(1).split(";") if line.strip() for f in _declaration(line, by_value, defines)]
        if not fields or not all(name for name, _, _ in fields):
            raise HeaderError(f"empty struct or unnamed field in {m.group(2)}")
        structs[m.group(2)] = fields
        by_value[m.group(2)] = True
    text = _STRUCT.sub(" ", text)

    functions: Dict[str, Tuple[Type, List[Type]]] = {}
    *statements, tail = text.split(";")
    if tail.strip():
        raise HeaderError(f"left over after the last prototype: {tail.strip()!r}")
    for stmt in statements:
        m = _PROTOTYPE.match(stmt.strip())
        if not m:
            raise HeaderError(f"left over after typedefs and prototypes: {stmt.strip()!r}")
        ret = _declaration(m.group(1), {**by_value, "void": True}, defines)
        args = [] if m.group(3).strip() in ("", "void") else [_declaration(a, by_value, defines) for a in m.group(3).split(",")]
        if any(len(d) != 1 or d[0][2] is not None for d in [ret] + args) or ret[0][0]:
            raise HeaderError(f"cannot parse the prototype {stmt.strip()!r}")
        functions[m.group(2)] = (ret[0][1], [a[0][1] for a in args])
    return Header(defines, structs, opaque, functions)


@functools.lru_cache(maxsize=None)
def load(path: str = HEADER_PATH) -> Header:
    if not os.path.exists(path):
        raise FileNotFoundError(f"the C header {path} is missing: the ctypes binding is derived from it")
    with open(path) as f:
        return parse(f.read())
