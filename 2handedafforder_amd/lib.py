"""ctypes binding of libhaff_hip.so (the C-ABI declared in include/haff_hip.h).

The product path has NO fallback: if the HIP library is missing or a symbol is absent this module raises.
`build_library()` compiles it in-tree with hipcc for gfx950 (works without a GPU: hipcc cross-compiles).
"""
import ctypes
import os
import re
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("HAFF_LIB_PATH") or os.path.join(_HERE, "lib", "libhaff_hip.so")   # override: A/B builds in tools/
CSRC_DIR = os.path.join(_HERE, "csrc")
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "haff_hip.h")
IO_HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "haff_io.h")   # file-format helpers, beside the frozen hot-path ABI

c_void_p, c_int, c_long, c_float = ctypes.c_void_p, ctypes.c_int, ctypes.c_long, ctypes.c_float


class HaffLibraryError(RuntimeError):
    pass


_SCALARS = {"int": c_int, "long": c_long, "float": c_float}


def _argtype(fn, param):
    if "..." in param or "[" in param or "(" in param:
        raise HaffLibraryError(f"{fn}: parameter `{param}` is varargs, an array or a function pointer")
    if "*" in param:
        return c_void_p
    words = [w for w in param.split() if w != "const"]
    if len(words) not in (1, 2) or words[0] not in _SCALARS:    # [type] or [type, name]
        raise HaffLibraryError(f"{fn}: parameter `{param}` is not a pointer, int, long or float")
    return _SCALARS[words[0]]


def parse_header(text):
    """name -> [ctypes argtypes] of every `int haff_*(...);` declared in the text of a C header. Strict: whatever it cannot map
    exactly (another scalar or return type, an array, a function pointer, varargs, a name declared twice) raises."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    text = re.sub(r"^[ \t]*#.*$", "", text, flags=re.M)
    protos = {}
    for m in re.finditer(r"([^;{}]*?)\b(haff_\w+)\s*\(([^;{}]*)\)\s*;", text):
        ret, fn, params = m.group(1).split(), m.group(2), m.group(3).strip()
        if ret != ["int"]:
            raise HaffLibraryError(f"{fn}: return type `{' '.join(ret)}` is not int")
        if fn in protos:
            raise HaffLibraryError(f"{fn}: declared twice")
        protos[fn] = [] if params == "void" else [_argtype(fn, p.strip()) for p in params.split(",")]
    return protos


def _read_header(path=None):
    path = HEADER_PATH if path is None else path
    try:
        with open(path) as fh:
            return fh.read()
    except OSError as e:
        raise HaffLibraryError(f"{path} not readable: the prototypes of libhaff_hip.so are derived from it") from e


# name -> argtypes ; every entry point returns int (0 ok, <0 error). include/haff_hip.h is the one declaration: this table is read
# from it, and every definition in csrc/ is compiled against it
_PROTOS = parse_header(_read_header())

EXPORTED_SYMBOLS = tuple(sorted(_PROTOS))

# the same for include/haff_io.h, in a table of its own: the hot-path ABI above stays as it is locked
_IO_PROTOS = parse_header(_read_header(IO_HEADER_PATH))
IO_SYMBOLS = tuple(sorted(_IO_PROTOS))

_lib = None


def build_library(verbose=False):
    """Compile every HIP source for gfx950 into lib/libhaff_hip.so (in-tree, so it travels with the repo)."""
    cmd = ["make", "-C", CSRC_DIR, "-j8"]
    res = subprocess.run(cmd, capture_output=True, text=True)
    if verbose or res.returncode != 0:
        print(res.stdout[-4000:])
        print(res.stderr[-8000:])
    if res.returncode != 0:
        raise HaffLibraryError("hipcc build of libhaff_hip.so failed")
    return LIB_PATH


def source_hash():
    """sha256 (16 hex digits) over the HIP sources the library is built from: what profiles/pmc_gemm_traffic.json is stamped with,
    so bench.py never reports PMC traffic collected on another tree as this run's."""
    import hashlib
    h = hashlib.sha256()
    for name in sorted(os.listdir(CSRC_DIR)):
        if name.endswith((".hip", ".h", ".inc")) or name == "Makefile":
            h.update(name.encode())
            with open(os.path.join(CSRC_DIR, name), "rb") as fh:
                h.update(fh.read())
    return h.hexdigest()[:16]


def load_library():
    """dlopen the library and attach prototypes. Raises (never falls back) when it is missing."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise HaffLibraryError(
            f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(there is no CPU or eager fallback for the hot path)")
    lib = ctypes.CDLL(LIB_PATH)
    for name, argtypes in list(_PROTOS.items()) + list(_IO_PROTOS.items()):
        try:
            fn = getattr(lib, name)
        except AttributeError as e:
            raise HaffLibraryError(f"symbol {name} missing from {LIB_PATH}") from e
        fn.argtypes = argtypes
        fn.restype = c_int
    _lib = lib
    return lib


def check(rc, what):
    if rc != 0:
        raise HaffLibraryError(f"{what} failed with code {rc} "
                               "(-1 bad argument, -2 unsupported shape, -3 launch error)")
