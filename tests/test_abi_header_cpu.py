"""The C ABI is declared once, in include/haff_hip.h: lib.py derives its ctypes prototypes from the header and every definition in
csrc/ is compiled against it. An ABI lock (tests/golden/abi_signatures.json, recorded from the hand-written table lib.py carried
before) makes an accidental change fail here; the parser is strict; the compiler rejects a definition that disagrees. CPU only."""
import ctypes
import json
import os
import subprocess

import pytest

from haff import lib as hlib
from haff.lib import HaffLibraryError, parse_header

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "2handedafforder_amd", "csrc")
LETTER = {ctypes.c_void_p: "p", ctypes.c_long: "l", ctypes.c_int: "i", ctypes.c_float: "f"}


def _signature(argtypes):
    return "".join(LETTER[t] for t in argtypes)


def _locked():
    with open(os.path.join(ROOT, "tests", "golden", "abi_signatures.json")) as fh:
        return json.load(fh)


def test_derived_prototypes_equal_the_abi_lock():
    locked = _locked()
    assert len(locked) == 143 and set("".join(locked.values())) <= set("plif")
    assert sorted(hlib._PROTOS) == sorted(locked)
    for name, sig in locked.items():
        assert _signature(hlib._PROTOS[name]) == sig, name
    assert hlib.EXPORTED_SYMBOLS == tuple(sorted(locked))
    assert _signature(hlib._PROTOS["haff_gemm_stream_cap"]) == "pi"
    assert hlib.HEADER_PATH == os.path.join(ROOT, "include", "haff_hip.h")


def test_loaded_library_carries_the_abi_lock():
    if not os.path.exists(hlib.LIB_PATH):
        hlib.build_library()
    lib = hlib.load_library()
    for name, sig in _locked().items():
        fn = getattr(lib, name)
        assert _signature(fn.argtypes) == sig, name
        assert fn.restype is ctypes.c_int, name


def test_parser_reads_declarations_as_written():
    got = parse_header("""
        /* int haff_fake(int x); */
        // int haff_fake2(int x);
        #define HAFF_OK 0
        typedef struct haff_chain_layer { const void *wqkv; void *kcache; } haff_chain_layer;
        int haff_three(const void* A, long lda,
                       float scale /* not a parameter: int z, */,
                       int n);
        int haff_ptrs(const haff_chain_layer* t, unsigned char* p, const unsigned* q, const float* f, long* out);
        int haff_none(void);
        int haff_consts(const int n, const long m, float);
    """)
    assert list(got) == ["haff_three", "haff_ptrs", "haff_none", "haff_consts"]
    assert got["haff_three"] == [ctypes.c_void_p, ctypes.c_long, ctypes.c_float, ctypes.c_int]
    assert got["haff_ptrs"] == [ctypes.c_void_p] * 5
    assert got["haff_none"] == []
    assert got["haff_consts"] == [ctypes.c_int, ctypes.c_long, ctypes.c_float]


@pytest.mark.parametrize("decl, names", [
    ("int haff_x(void* p, unsigned n);", ("haff_x", "unsigned n")),
    ("int haff_x(double x);", ("haff_x", "double x")),
    ("int haff_x(int a, size_t n);", ("haff_x", "size_t n")),
    ("int haff_x(haff_chain_layer layer);", ("haff_x", "haff_chain_layer layer")),
    ("int haff_x(unsigned int n);", ("haff_x", "unsigned int n")),
    ("int haff_x(long long n);", ("haff_x", "long long n")),
    ("int haff_x(int a[4]);", ("haff_x", "int a[4]")),
    ("int haff_x(int (*cb)(int));", ("haff_x",)),
    ("int haff_x(int n, ...);", ("haff_x", "...")),
    ("long haff_x(int n);", ("haff_x", "long")),
    ("void haff_x(int n);", ("haff_x", "void")),
    ("const int* haff_x(int n);", ("haff_x",)),
    ("int haff_x(int n);\nint haff_y(void);\nint haff_x(int n);", ("haff_x", "twice")),
])
def test_parser_never_guesses(decl, names):
    with pytest.raises(HaffLibraryError) as e:
        parse_header(decl)
    for word in names:
        assert word in str(e.value), (word, str(e.value))


def test_missing_header_names_its_path(tmp_path, monkeypatch):
    monkeypatch.setattr(hlib, "HEADER_PATH", str(tmp_path / "nowhere.h"))
    with pytest.raises(HaffLibraryError, match="nowhere.h"):
        hlib._read_header()


def _syntax_only(tmp_path, name, cap_type):
    src = tmp_path / name
    src.write_text('#include "haff_common.h"\n'
                   f'extern "C" int haff_gemm_stream_cap(void* stream, {cap_type} cap) {{\n'
                   "  return stream ? (int)cap : HAFF_OK;\n"
                   "}\n")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    return subprocess.run([hipcc, "-std=c++17", "--offload-arch=gfx950", "--cuda-host-only", "-fsyntax-only", "-x", "hip",
                           "-I" + CSRC, "-I" + os.path.join(ROOT, "include"), str(src)], capture_output=True, text=True)


def test_compiler_compares_a_definition_with_its_declaration(tmp_path):
    good = _syntax_only(tmp_path, "agrees.hip", "int")
    assert good.returncode == 0, good.stderr
    bad = _syntax_only(tmp_path, "disagrees.hip", "long")
    assert bad.returncode != 0 and "conflicting types" in bad.stderr, bad.stderr


def test_sources_are_compiled_against_the_header():
    common = open(os.path.join(CSRC, "haff_common.h")).read()
    assert '#include "haff_hip.h"' in common and "#define HAFF_OK" not in common
    header = open(hlib.HEADER_PATH).read()
    for code in ("#define HAFF_OK 0", "#define HAFF_ERR_BAD_ARG (-1)", "#define HAFF_ERR_UNSUPPORTED (-2)", "#define HAFF_ERR_LAUNCH (-3)"):
        assert code in header, code
    makefile = open(os.path.join(CSRC, "Makefile")).read()
    assert "-I../../include" in makefile and "build/%.o: %.hip haff_common.h ../../include/haff_hip.h" in makefile
    for name in os.listdir(CSRC):
        if name.endswith(".hip"):
            src = open(os.path.join(CSRC, name)).read()
            assert '#include "haff_common.h"' in src, name
            assert "struct haff_" not in src, f"{name} redefines a struct of the public header"
    for name, mirror in (("mask_score.hip", "HAFF_SAME_SIZE(ScoreFrame, haff_score_frame)"),
                         ("contour_hausdorff.hip", "HAFF_SAME_SIZE(Plane, haff_contour_plane)"),
                         ("affordance_extract.hip", "HAFF_SAME_SIZE(ExtractItem, haff_extract_item)")):
        assert mirror in open(os.path.join(CSRC, name)).read(), name
