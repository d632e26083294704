"""The ctypes signatures of the three shared libraries, derived from the public headers under include/ -- the only place they are written down.

Every `BU_*API <ret> bu_name(<args>);` prototype becomes (restype, argtypes) by one rule: a scalar maps to its exact ctypes type, `const char*` to c_char_p,
every other pointer, array parameter or `*_fn` call-back typedef to c_void_p (which takes byref(), ctypes arrays, data_as(c_void_p), ints, None and CFUNCTYPE
instances). A type the rule does not know raises at import. parse_prototypes takes other marks and names too, and definitions as well as prototypes: the test
checkers (tests/native_libs.py) derive their signatures from their sources with it. The ctypes.Structure mirrors of the headers' structs stay hand-written next to their users."""
import ctypes as C
import functools
import os
import pathlib
import re

PKG_DIR = pathlib.Path(__file__).resolve().parent
LIB_DIR = pathlib.Path(os.environ.get("BU_HIP_LIB_DIR", PKG_DIR / "lib"))  # override: developer experiments with variant builds
INCLUDE_DIR = PKG_DIR.parent / "include"

# library -> (file, the headers it serves, what to do when the file is not there)
LIBRARIES = {
    "hip": ("libbasisu_hip.so", ("basisu_hip.h",), "is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` (there is no CPU fallback)"),
    "frontend": ("libbasisu_frontend.so", ("basisu_hip_frontend.h", "basisu_hip_backend.h", "basisu_hip_etc1s_decode.h", "basisu_hip_image_metrics.h"),
                 "is missing: run __graft_entry__.build()"),
    "rccl": ("libbasisu_rccl.so", ("basisu_hip_comm.h",), "not found: build it (make -C basis_universal_amd/csrc)"),
}

_SCALARS = {"int": C.c_int, "uint8_t": C.c_uint8, "int32_t": C.c_int32, "uint32_t": C.c_uint32, "int64_t": C.c_int64, "uint64_t": C.c_uint64,
            "size_t": C.c_size_t, "float": C.c_float, "double": C.c_double}
_SPELLED_OUT = re.compile(r'\bextern\s+"C"(?!\s*\{)|\b__attribute__\s*\(\((?:[^()]|\([^()]*\))*\)\)')   # what a mark macro expands to, where a declaration writes it out as well


class HipError(RuntimeError):
    pass


def _ctype(decl, function, is_return=False):
    """One return type, or one parameter with or without its name -> ctypes type."""
    words = re.findall(r"\w+|\*|\[", decl)
    base = [w for w in words if w != "const"]
    if "*" in base or "[" in base:
        return C.c_char_p if words[:3] == ["const", "char", "*"] and base.count("*") == 1 and "[" not in base else C.c_void_p
    if is_return and base == ["void"]:
        return None
    if 1 <= len(base) <= (1 if is_return else 2):   # the type and, for a parameter, perhaps a name
        if base[0] in _SCALARS:
            return _SCALARS[base[0]]
        if base[0].endswith("_fn") and not is_return:
            return C.c_void_p
    raise TypeError(f"{function}: no ctypes mapping for `{decl.strip()}`")


def parse_prototypes(text, mark=r"BU_\w*API", name=r"bu_\w+"):
    """The text of a header or a source file -> {function: (restype, [argtypes])} for every `<mark> <ret> <name>(<args>)` in it that ends in `;` or opens a body.
    A function declared twice must be declared the same way both times."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    text = re.sub(r"^[ \t]*#.*$", "", text, flags=re.M)
    text = _SPELLED_OUT.sub(" ", text)
    out, found = {}, re.findall(rf"\b(?:{mark})\s+([^;{{}}()]*?)\b({name})\s*\(([^(){{}};]*)\)\s*[;{{]", text)
    for ret, fn, params in found:
        params = [] if params.strip() in ("", "void") else params.split(",")
        sig = (_ctype(ret, fn, True), [_ctype(p, fn) for p in params])
        if out.setdefault(fn, sig) != sig:
            raise TypeError(f"{fn}: declared twice with different signatures")
    marks = len(re.findall(rf"\b(?:{mark})\b", text))
    if len(found) != marks:
        shown = mark.replace(r"\w*", "*")   # the pattern as prose writes it: BU_\w*API -> BU_*API
        raise TypeError(f"{marks} {shown} marks but {len(found)} prototypes understood: {', '.join(fn for _, fn, _ in found)}")
    return out


PROTOTYPES = {lib: {name: sig for header in headers for name, sig in parse_prototypes((INCLUDE_DIR / header).read_text()).items()}
              for lib, (_, headers, _) in LIBRARIES.items()}


def library_path(lib):
    return LIB_DIR / LIBRARIES[lib][0]


def open_library(lib, path=None):
    """The CDLL of `lib` with restype and argtypes set on every prototype of its headers; a prototype the file does not export is an AttributeError."""
    path = pathlib.Path(path or library_path(lib))
    if not path.exists():
        raise HipError(f"{path} {LIBRARIES[lib][2]}")
    dll = C.CDLL(str(path))
    for name, (res, args) in PROTOTYPES[lib].items():
        fn = getattr(dll, name)  # AttributeError = symbol missing = broken build
        fn.restype, fn.argtypes = res, args
    return dll


load = functools.lru_cache(maxsize=None)(open_library)   # load("frontend"), load("rccl"): one CDLL per library and process; capi.load_library() is the one for "hip"
