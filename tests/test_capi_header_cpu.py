"""uenc/capi.py derives the ctypes binding and the Python constants from include/uenc.h.  Checked here, without a GPU: the binding equals
the one recorded from the last revision that kept it as a hand-written table (tests/golden/capi_signatures_parent.json), nothing the
header declares is dropped, and the parser refuses what its type table does not list.

The golden is written by `python tests/test_capi_header_cpu.py --record <json> --pkg <checkout>/uni-encoder-code_amd --rev <revision>` with
the library of that checkout built."""
import ctypes
import json
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "capi_signatures_parent.json")

# Python name -> where it lives; every one mirrors a UENC_* macro of the header
CONSTANTS = {
    "uenc.capi": ["F32", "BF16", "EPI_NONE", "EPI_GELU", "EPI_RELU", "EPI_RESIDUAL", "EPI_MUL_DGELU", "EPI_MUL_DRELU"],
    "uenc.kernels": ["NT_TILE_256X256", "NT_TILE_256X192", "NT_TILE_128X256", "TARGETS_MAX_SEGMENTS", "EVAL_MAX_CLASSES", "EVAL_PQ_DIM",
                     "AUG_TILE_W", "AUG_TILE_H", "AUG_MAX_TAPS", "AUG_COLOUR_TAB_INTS"],
    "uenc.train_data": ["COLOUR_SAT", "COLOUR_HUE", "COLOUR_CONTRAST_FIRST", "COLOUR_RGB"],
    "uenc.modeling.targets": ["MAX_SEGMENTS"],
    "uenc.evaluation": ["PQ_MAX_SEGMENTS"],
}
# c_long and c_longlong are one class of argument on this ABI: 8 bytes, signed (CPython on LP64 even makes them one type)
_CLASS = {"c_longlong": "c_long"}


def dump():
    """{"functions": name -> {"restype", "argtypes"} as ctypes type names, "constants": "module.NAME" -> int} of the imported package."""
    import importlib
    from uenc import capi
    fns = {}
    for name in capi.exported_symbols():
        fn = getattr(capi.lib, name)
        fns[name] = {"restype": fn.restype.__name__, "argtypes": [t.__name__ for t in fn.argtypes]}
    consts = {}
    for mod, names in CONSTANTS.items():
        m = importlib.import_module(mod)
        for n in names:
            v = getattr(m, n)
            assert type(v) is int, (mod, n, v)
            consts[f"{mod}.{n}"] = v
    return {"functions": fns, "constants": consts}


def _header():
    with open(os.path.join(ROOT, "include", "uenc.h")) as f:
        return f.read()


def test_binding_equals_the_recorded_parent():
    with open(GOLDEN) as f:
        gold = json.load(f)
    assert len(gold["recorded_from"]) == 40
    assert ctypes.sizeof(ctypes.c_long) == ctypes.sizeof(ctypes.c_longlong) == 8
    assert ctypes.c_long(-1).value == ctypes.c_longlong(-1).value == -1          # both signed
    got = dump()
    assert len(gold["functions"]) == 130 and set(got["functions"]) == set(gold["functions"])
    cls = lambda n: _CLASS.get(n, n)
    for name, want in gold["functions"].items():
        g = got["functions"][name]
        assert cls(g["restype"]) == cls(want["restype"]), name
        assert [cls(t) for t in g["argtypes"]] == [cls(t) for t in want["argtypes"]], name
    # the one nominal difference the header makes, `long long ignore_label` bound as written (where ctypes tells the two apart at all)
    differ = [(n, i) for n, w in gold["functions"].items() for i, (a, b) in enumerate(zip(got["functions"][n]["argtypes"], w["argtypes"])) if a != b]
    assert differ in ([], [("uenc_targets_write", 8)])
    assert sum(len(v) for v in CONSTANTS.values()) == len(gold["constants"]) == 24
    assert got["constants"] == gold["constants"]


def test_no_declaration_and_no_integer_macro_is_dropped():
    from test_abi_cpu import _declared         # its own regular expression, independent of the parser
    from uenc import capi
    functions, constants = capi.parse_header(_header())
    assert sorted(functions) == _declared() == capi.exported_symbols() and len(functions) == 130
    macros = dict(re.findall(r"^#define[ \t]+(UENC_\w+)[ \t]+(\d+)\b", _header(), flags=re.M))
    assert len(macros) >= 22 and constants == {k: int(v) for k, v in macros.items()}
    for name, (restype, argtypes) in functions.items():
        fn = getattr(capi.lib, name)
        assert fn.restype is restype and list(fn.argtypes) == argtypes, name


def test_python_constants_are_the_headers():
    """capi and kernels assign theirs from the parse; the three modules that import neither at load time keep literals, held equal here."""
    from uenc import capi, evaluation, kernels as K, train_data
    from uenc.modeling import targets
    C = capi.CONSTANTS
    assert (capi.F32, capi.BF16) == (C["UENC_F32"], C["UENC_BF16"]) == (0, 1)
    for n in CONSTANTS["uenc.capi"][2:]:
        assert getattr(capi, n) == C["UENC_" + n]
    for n in CONSTANTS["uenc.kernels"]:
        assert getattr(K, n) == C["UENC_" + n]
    for n in CONSTANTS["uenc.train_data"]:
        assert getattr(train_data, n) == C["UENC_AUG_" + n]
    assert targets.MAX_SEGMENTS == evaluation.PQ_MAX_SEGMENTS == C["UENC_TARGETS_MAX_SEGMENTS"]
    assert C["UENC_EVAL_PQ_DIM"] == C["UENC_TARGETS_MAX_SEGMENTS"] + 2


def test_missing_header_fails_loudly(tmp_path):
    """A copy of the binding next to a library but two directories away from no include/uenc.h: ImportError naming the path it looked at."""
    import importlib.util
    pkg = tmp_path / "a" / "b"
    pkg.mkdir(parents=True)
    (pkg / "capi_copy.py").write_text(open(os.path.join(ROOT, "uni-encoder-code_amd", "uenc", "capi.py")).read())
    (pkg / "libuenc_hip.so").write_bytes(b"")           # never opened: the header is read first
    spec = importlib.util.spec_from_file_location("capi_copy", pkg / "capi_copy.py")
    with pytest.raises(ImportError) as e:
        spec.loader.exec_module(importlib.util.module_from_spec(spec))
    assert str(tmp_path / "include" / "uenc.h") in str(e.value)


# ---- the parser on small header texts: it needs neither the library nor the real header ---------------------------------------------------

_SMALL = """
/* a header in the style of include/uenc.h */
#ifndef UENC_H
#define UENC_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
#define UENC_F32 0
#define UENC_BIG 0x10      /* sixteen */
#define UENC_STREAM_T void*
typedef UENC_STREAM_T uenc_stream_t;
int uenc_version(void);
const char* uenc_arch(void); // "gfx950"
long uenc_ws_bytes(const int64_t* shapes, int B);   /* a long return */
int uenc_cast_t(const float* src /* [R][C] */, void* dst /* [C][R], ( bf16 ); */,
                int R, int C,     // rows, columns
                uenc_stream_t stream);
int uenc_mix(long n, int64_t m, long long ignore, unsigned seed, float p, double q, const unsigned* seeds, unsigned long long* state);
#ifdef __cplusplus
}
#endif
#endif /* UENC_H */
"""


def test_parser_reads_the_headers_forms():
    from uenc.capi import parse_header
    c = ctypes
    functions, constants = parse_header(_SMALL)
    assert constants == {"UENC_F32": 0, "UENC_BIG": 16}                 # no value (UENC_H) and no integer (UENC_STREAM_T): not constants
    assert list(functions) == ["uenc_version", "uenc_arch", "uenc_ws_bytes", "uenc_cast_t", "uenc_mix"]
    assert functions["uenc_version"] == (c.c_int, [])
    assert functions["uenc_arch"] == (c.c_char_p, [])
    assert functions["uenc_ws_bytes"] == (c.c_long, [c.c_void_p, c.c_int])                  # `const int64_t* shapes` is a pointer
    assert functions["uenc_cast_t"] == (c.c_int, [c.c_void_p, c.c_void_p, c.c_int, c.c_int, c.c_void_p])     # comments inside the list
    assert functions["uenc_mix"] == (c.c_int, [c.c_long, c.c_long, c.c_longlong, c.c_uint, c.c_float, c.c_double, c.c_void_p, c.c_void_p])


@pytest.mark.parametrize("decl,names", [
    ("int uenc_f(int a, short x);", ("uenc_f", "short x")),                    # a type the table does not list
    ("int uenc_f(unsigned char c);", ("uenc_f", "unsigned char c")),
    ("int uenc_f(int);", ("uenc_f", "int")),                                   # no parameter name: nothing to tell the type from
    ("short uenc_f(int a);", ("uenc_f", "short")),                             # the return type alike
    ("int uenc_f(int (*cb)(int), int n);", ("uenc_f",)),                       # a declaration the parser cannot split
])
def test_parser_fails_closed(decl, names):
    from uenc.capi import parse_header
    with pytest.raises(ValueError) as e:
        parse_header("int uenc_ok(int a);\n" + decl)
    for n in names:
        assert n in str(e.value), str(e.value)


if __name__ == "__main__":
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument("--record", required=True)
    ap.add_argument("--pkg", required=True)
    ap.add_argument("--rev", required=True)
    a = ap.parse_args()
    sys.path.insert(0, a.pkg)
    with open(a.record, "w") as f:
        json.dump({"recorded_from": a.rev, **dump()}, f, indent=1, sort_keys=True)
        f.write("\n")
