"""ctypes binding of ``csrc/libe3k.so`` (the C ABI declared in ``include/e3k.h``).

The library is built in-tree by ``make -C equivariant-nn-zoo_amd/csrc`` (driven by
``__graft_entry__.build()``).  There is **no fallback**: if the shared object is missing or a
call returns a non-zero status a ``RuntimeError`` is raised — the product path never routes
through a CPU or eager-PyTorch implementation.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional, Sequence

import torch

from . import abi
from .tuning import knob as _knob

_HERE = os.path.dirname(os.path.abspath(__file__))
CSRC_DIR = os.path.normpath(os.path.join(_HERE, "..", "..", "csrc"))
LIB_PATH = _knob("E3K_LIB") or os.path.join(CSRC_DIR, "libe3k.so")  # E3K_LIB: another build, for A/B runs

ABI = abi.load()
DEFINES = ABI.defines      # every `#define E3K_NAME <integer>` of the header
TP_MAXQ = DEFINES["E3K_TP_MAXQ"]
NARROW_MAX_SLOTS = DEFINES["E3K_NARROW_MAX_SLOTS"]      # entries of e3k_layer_desc.live_col / live_len

_SCALARS = {"int": C.c_int, "int32_t": C.c_int32, "uint32_t": C.c_uint32, "int64_t": C.c_int64, "uint8_t": C.c_uint8,
            "float": C.c_float, "double": C.c_double}
_MIRRORS = {}      # C struct name -> its ctypes.Structure, in header order


def _ctype(t, ret=False):
    """The typing rule: a scalar is its c_*, a struct by value its mirror, a pointer to a struct the header defines POINTER(mirror),
    every other pointer (opaque handles, device pointers, host scalar arrays) c_void_p; a `const char*` return c_char_p, void None."""
    base, depth = t
    if depth == 0:
        return None if base == "void" else _SCALARS.get(base) or _MIRRORS[base]
    if ret and t == ("char", 1):
        return C.c_char_p
    return C.POINTER(_MIRRORS[base]) if depth == 1 and base in _MIRRORS else C.c_void_p


# the mirrors, exported under the CamelCase of the C name without `e3k_`: e3k_layer_fwd_args -> LayerFwdArgs
for _name, _fields in ABI.structs.items():
    _cls = "".join(w.capitalize() for w in _name[len("e3k_"):].split("_"))
    _MIRRORS[_name] = globals()[_cls] = type(_cls, (C.Structure,), {
        "_fields_": [(f, _ctype(t) if n is None else _ctype(t) * n) for f, t, n in _fields]})

# name -> (restype, argtypes) of every function include/e3k.h declares
SIGNATURES = {name: (_ctype(ret, True), [_ctype(a) for a in args]) for name, (ret, args) in ABI.functions.items()}

_lib: Optional[C.CDLL] = None


def load() -> C.CDLL:
    """Load libe3k.so once; raise loudly if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"libe3k.so not found at {LIB_PATH}: build it with `make -C {CSRC_DIR}` "
            "(or __graft_entry__.build()).  There is no CPU fallback for the HIP path."
        )
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def check(code: int, what: str) -> None:
    if code != 0:
        msg = load().e3k_strerror(code).decode()
        raise RuntimeError(f"{what} failed: {msg} (e3k status {code})")


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)
_cur_device = getattr(torch._C, "_cuda_getDevice", None)


def stream_ptr() -> int:
    """hipStream_t of torch's current stream on the current device (every launch asks: the raw accessor skips the
    Python Stream object that ``torch.cuda.current_stream()`` builds, ~8 us per call)."""
    if _raw_stream is not None and _cur_device is not None:
        return _raw_stream(_cur_device())
    return torch.cuda.current_stream().cuda_stream


def seed_words(seed: int) -> tuple:
    """(low, high) 32-bit words of a 64-bit seed: the first two words of the counter-based draw (``csrc/e3k_draw.h``)."""
    seed = int(seed)
    return seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF


def ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


def require_cuda(*tensors: torch.Tensor) -> None:
    """Operands must live on the CURRENT device: launches go to ``stream_ptr()``, the current stream of the current
    device, and the C ABI never calls hipSetDevice (one process per GPU; use ``torch.cuda.set_device`` / ``device()``)."""
    cur = _cur_device() if _cur_device is not None else torch.cuda.current_device()
    for t in tensors:
        if t is None:
            continue
        if not t.is_cuda:
            raise RuntimeError(
                "e3_layers_amd kernels run on the GPU only (got a CPU tensor); there is no CPU "
                "fallback in the product path — the float64 CPU restatement lives in oracle/ for tests."
            )
        if t.device.index != cur:
            raise RuntimeError(
                f"tensor on cuda:{t.device.index} but the current device is cuda:{cur}: the kernels launch on the current "
                "device's stream — wrap the call in `with torch.cuda.device(tensor.device):`")


def f32c(t: torch.Tensor) -> torch.Tensor:
    """Contiguous fp32 view/copy."""
    if t.dtype != torch.float32:
        t = t.float()
    return t if t.is_contiguous() else t.contiguous()
