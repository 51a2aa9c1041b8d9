"""ctypes binding of the C ABI declared in ``include/spconv_amd.h``.

This is the only place the Python layer touches native code.  It mirrors the
role of ``spconv/pytorch/cppcore.py`` in the reference (raw pointer + stream
hand-off, ``cppcore.py:65-109``) without any tensorview / pybind types.
The header is the one declaration of the ABI: ``signatures()`` reads every
``restype`` / ``argtypes`` out of it, so a new entry point is declared there only.

The library is built in-tree by ``spconv_amd/csrc/build.sh`` (hipcc, gfx950).
There is no CPU fallback: if the shared object is missing the import of any
compute entry point raises.
"""
from __future__ import annotations

import ctypes
import functools
import os
import re
import subprocess
from typing import Optional

_HERE = os.path.dirname(os.path.abspath(__file__))
# SPX_LIB selects another build of the same ABI (the -DSPX_TIMELINE debug build of tools/timeline.py)
LIB_PATH = os.environ.get("SPX_LIB") or os.path.join(_HERE, "lib", "libspconv_amd.so")

c_int_p = ctypes.POINTER(ctypes.c_int)
c_float_p = ctypes.POINTER(ctypes.c_float)
vp = ctypes.c_void_p

HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "spconv_amd.h")
_SCALARS = {"int": ctypes.c_int, "size_t": ctypes.c_size_t, "float": ctypes.c_float, "double": ctypes.c_double,
            "long long": ctypes.c_longlong, "spx_stream_t": vp}


def _ctype(text: str, where: str):
    """ctypes type of one C type of the header.  `int *` is a HOST array (device memory is `int32_t *`) and is bound
    typed; `const char *` is a C string; every other pointer, device or host, travels as void *."""
    words = [w for w in text.replace("*", " * ").split() if w != "const"]
    base, stars = " ".join(w for w in words if w != "*"), words.count("*")
    if stars == 0 and base in _SCALARS:
        return _SCALARS[base]
    if stars and base:
        return {("char", 1): ctypes.c_char_p, ("int", 1): c_int_p}.get((base, stars), vp)
    raise ValueError(f"include/spconv_amd.h: {where}: no ctypes mapping for the type {text.strip()!r}")


def parse_header(text: str) -> dict:
    """{name: (restype, argtypes)} of every `spx_*` declaration of a C header.  ValueError for a type outside the
    mapping of _ctype (never a default) and for an `spx_*(` that is not a complete declaration."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    out = {}
    for m in re.finditer(r"^[ \t]*([\w \t*]+?)\s*\b(spx_\w+)\s*\(([^()]*)\)\s*;", text, flags=re.M):
        ret, name, args = m.groups()
        args = [] if args.strip() == "void" else [re.fullmatch(r"\s*(.*?)\w+\s*", a, flags=re.S) for a in args.split(",")]
        if None in args:
            raise ValueError(f"include/spconv_amd.h: {name}: an argument is empty or has no name")
        out[name] = (_ctype(ret, f"{name}, return type"),
                     [_ctype(a.group(1), f"{name}, argument {i + 1} ({' '.join(a.group(0).split())})")
                      for i, a in enumerate(args)])
    unparsed = sorted(set(re.findall(r"\b(spx_\w+)\s*\(", text)) - set(out))
    if unparsed:
        raise ValueError(f"include/spconv_amd.h: not a declaration this binding can read: {unparsed}")
    return out


@functools.lru_cache(maxsize=None)
def signatures() -> dict:
    """The binding: include/spconv_amd.h is its one declaration (read and parsed once, at the first call)."""
    with open(HEADER_PATH) as f:
        return parse_header(f.read())


DTYPE_F32, DTYPE_F16, DTYPE_BF16, DTYPE_I8, DTYPE_F64 = 0, 1, 2, 3, 4
ACT_NONE, ACT_RELU, ACT_SIGMOID, ACT_LEAKY_RELU = 0, 1, 2, 3
COLLAPSE_SUM, COLLAPSE_MEAN, COLLAPSE_MAX = 0, 1, 2
SCORE_ABSMEAN, SCORE_ABSMAX = 0, 1

_lib: Optional[ctypes.CDLL] = None


def linked_objects() -> list:
    """Object files the library is linked from: csrc/build.sh holds the one list of translation units."""
    script = os.path.join(_HERE, "csrc", "build.sh")
    out = subprocess.check_output(["bash", script, "--list"], text=True)
    return [os.path.join(_HERE, "lib", line.strip()) for line in out.splitlines() if line.strip()]


def build(force: bool = False) -> str:
    """Compile the HIP sources for gfx950 (no GPU needed).  force=True deletes EVERY object the library is linked from
    (and the library) first -- the list is build.sh's own, so a translation unit added there cannot be forgotten here."""
    script = os.path.join(_HERE, "csrc", "build.sh")
    subprocess.check_call(["bash", script] + (["--force"] if force else []))
    return LIB_PATH


def load() -> ctypes.CDLL:
    """Load libspconv_amd.so; raises (never falls back) when it is missing."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"spconv_amd native library not found at {LIB_PATH}. Build it with "
            f"`bash spconv_amd/csrc/build.sh` (hipcc --offload-arch=gfx950). "
            f"There is no CPU fallback.")
    # torch bundles its own libamdhip64 (same SONAME); importing it first makes
    # our library bind to the runtime that owns torch's streams and allocations.
    import torch  # noqa: F401
    lib = ctypes.CDLL(LIB_PATH)
    for name, (restype, argtypes) in signatures().items():
        fn = getattr(lib, name)  # AttributeError if the symbol is not exported
        fn.restype = restype
        fn.argtypes = argtypes
    _lib = lib
    return lib


def check(status: int) -> None:
    if status != 0:
        msg = load().spx_last_error().decode("utf-8", "replace")
        raise RuntimeError(f"spconv_amd native error ({status}): {msg}")


def launch_counts(keys) -> dict:
    """{key: spx_launch_count(key)} for every key; KeyError for a key the library does not know."""
    lib = load()
    out = {k: int(lib.spx_launch_count(k.encode())) for k in keys}
    for k, v in out.items():
        if v < 0:
            raise KeyError(k)
    return out


def ints(values):
    return (ctypes.c_int * len(values))(*[int(v) for v in values])


def ptrs(values):
    """Host array of device pointers (None = NULL) for the C calls that take a list of operands."""
    return (ctypes.c_void_p * len(values))(*[None if v is None else int(v) for v in values])
