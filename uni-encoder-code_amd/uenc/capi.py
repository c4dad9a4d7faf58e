"""ctypes binding of libuenc_hip.so (C ABI: include/uenc.h).

Every entry point takes raw device pointers, sizes / strides and a hipStream_t; it allocates
nothing and never synchronises.  Return convention: 0 ok, <0 invalid argument (nothing launched),
>0 hipError_t.  `check()` turns a non-zero code into a Python exception.

The binding is derived from the header when this module is imported: `parse_header()` reads every declaration and every integer
`#define UENC_*` of include/uenc.h, and `_load()` sets each function's `argtypes` / `restype` from that.  So a new entry point or
constant is declared in include/uenc.h and nowhere else; a type the parser's table does not list is an error, never a guess.

include/uenc.h is the frozen core ABI (`FUNCTIONS`, `CONSTANTS`, `exported_symbols()`).  Entry points added since are declared in
include/uenc_ext.h, defined under csrc/ext/ and bound here on the same `lib` as `EXT_FUNCTIONS` / `EXT_CONSTANTS`.
"""
import ctypes
import os
import re

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libuenc_hip.so")
HEADER_PATH = os.path.normpath(os.path.join(_HERE, "..", "..", "include", "uenc.h"))
EXT_HEADER_PATH = os.path.normpath(os.path.join(_HERE, "..", "..", "include", "uenc_ext.h"))

# the C types of the header's parameters and results; anything with a `*` is a pointer
_CTYPES = {"int": ctypes.c_int, "long": ctypes.c_long, "int64_t": ctypes.c_long, "long long": ctypes.c_longlong, "unsigned": ctypes.c_uint,
           "float": ctypes.c_float, "double": ctypes.c_double, "uenc_stream_t": ctypes.c_void_p}


def _ctype(decl, named, what):
    """ctypes class of one C type; `named`: the last word of `decl` is the parameter's name."""
    if "*" in decl:
        return ctypes.c_void_p
    words = [w for w in decl.split() if w != "const"]
    key = " ".join(words[:-1] if named else words)
    if key not in _CTYPES:
        raise ValueError(f"include/uenc.h: {what} `{decl}`: a type outside the binding's table {sorted(_CTYPES)}")
    return _CTYPES[key]


def parse_header(text):
    """Header text -> (functions, constants): uenc_* name -> (restype, [argtypes]) in order of declaration, and UENC_* macro -> value for
    the macros defined as an integer literal.  Needs neither the library nor torch."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    constants = {m[1]: int(m[2], 0) for m in re.finditer(r"^[ \t]*#[ \t]*define[ \t]+(UENC_\w+)[ \t]+(0[xX][0-9a-fA-F]+|\d+)[ \t]*$", text, re.M)}
    text = re.sub(r"^[ \t]*#.*$", "", text, flags=re.M)
    text = re.sub(r'\bextern\s+"C"\s*\{', " ", text)          # uenc_ext.h has no typedef between the brace and its first declaration
    functions = {}
    for stmt in text.split(";"):
        if "(" not in stmt:             # the typedef, the braces of extern "C"
            continue
        m = re.fullmatch(r"\s*([\w\s*]+?)\s*\b(uenc_\w+)\s*\(([^()]*)\)\s*", stmt)
        if not m:
            raise ValueError(f"include/uenc.h: not a declaration `ret uenc_name(params);`: {' '.join(stmt.split())}")
        ret, name, params = (" ".join(g.split()) for g in m.groups())
        restype = ctypes.c_char_p if ret == "const char*" else _ctype(ret, False, f"{name}: return type")
        argtypes = [] if params == "void" else [_ctype(p.strip(), True, f"{name}: parameter") for p in params.split(",")]
        functions[name] = (restype, argtypes)
    return functions, constants


class UencError(RuntimeError):
    pass


def _bind(lib, functions):
    for name, (restype, argtypes) in functions.items():
        fn = getattr(lib, name)          # AttributeError if the library and the header drift apart
        fn.argtypes = argtypes
        fn.restype = restype


def _load():
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(or `make -C uni-encoder-code_amd/csrc`). The HIP library is mandatory; there is no fallback path.")
    try:
        with open(HEADER_PATH) as f:
            functions, constants = parse_header(f.read())
    except OSError as e:
        raise ImportError(f"{HEADER_PATH} cannot be read ({e}): the binding is derived from it, the package is used in-tree") from e
    lib = ctypes.CDLL(LIB_PATH)
    _bind(lib, functions)
    return lib, functions, constants


def _load_ext(lib):
    """The extension header, after the core one: same parser, same library object.  Its names stay out of FUNCTIONS / CONSTANTS."""
    try:
        with open(EXT_HEADER_PATH) as f:
            functions, constants = parse_header(f.read())
    except OSError as e:
        raise ImportError(f"{EXT_HEADER_PATH} cannot be read ({e}): the binding of the extension entry points is derived from it") from e
    _bind(lib, functions)
    return functions, constants


lib, FUNCTIONS, CONSTANTS = _load()
EXT_FUNCTIONS, EXT_CONSTANTS = _load_ext(lib)

F32, BF16 = CONSTANTS["UENC_F32"], CONSTANTS["UENC_BF16"]
EPI_NONE, EPI_GELU, EPI_RELU, EPI_RESIDUAL, EPI_MUL_DGELU, EPI_MUL_DRELU = (
    CONSTANTS["UENC_EPI_" + n] for n in ("NONE", "GELU", "RELU", "RESIDUAL", "MUL_DGELU", "MUL_DRELU"))


def exported_symbols():
    return sorted(FUNCTIONS)


def check(code: int, what: str = "uenc"):
    if code == 0:
        return
    if code < 0:
        raise UencError(f"{what}: invalid argument (shape / alignment / dtype), nothing was launched")
    raise UencError(f"{what}: hipError_t {code}")


def stream_ptr():
    return torch.cuda.current_stream().cuda_stream


def dt(t: torch.Tensor) -> int:
    if t.dtype == torch.float32:
        return F32
    if t.dtype == torch.bfloat16:
        return BF16
    raise UencError(f"unsupported dtype {t.dtype}")


def ptr(t):
    return 0 if t is None else t.data_ptr()
