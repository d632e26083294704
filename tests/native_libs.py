"""The checker libraries of the tests: which there are, how each is built, and the one place that loads them and sets their ctypes signatures.

A checker's signatures are written once, in its source: every function defined (or declared) behind the library's mark becomes (restype, argtypes) by the rule of
basis_universal_amd/_cabi.py, the one the product's own headers are bound by. Nothing else under tests/ or tools/ calls CDLL on a checker or assigns restype / argtypes."""
import ctypes as C
import fcntl
import functools
import json
import os
import pathlib
import re
import subprocess
import sys

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))   # the tools that put only tests/ on sys.path import the helper modules too
from basis_universal_amd._cabi import parse_prototypes  # noqa: E402

NATIVE, ORACLE = ROOT / "tests" / "native", ROOT / "oracle"
COMPILE = ["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-fvisibility=hidden"]   # the mark carries the visibility

# name -> (library, the source whose marks define its interface, the mark, how it is made):
#   "g++"       COMPILE on the source, whenever the library is older than the source or a file it includes
#   "make"      make -C <the library's directory> <the library>, in every process that loads it: the Makefile knows what it is made from. make writes the library
#               in place, so the call holds a lock on the Makefile: a process that finds it stale waits for the one that is rebuilding it
#   "prebuilt"  never built by a test: oracle/Makefile makes it where the reference is, elsewhere it travels as a binary (and may be of an older revision)
CHECKERS = {name: (NATIVE / f"lib{name}.so", NATIVE / f"{name}.cpp", "HOST_API", "g++")
            for name in ("uastc_host", "fsum_host", "tt_exact_host", "tsvq_node_host", "seam_translate_host", "block_metric_host", "transcode_host", "image_metrics_host",
                         "psnr_hvs_host", "block_unpack_host", "tile_geometry_host")}
CHECKERS["oracle"] = (ORACLE / "liboracle_etc1s.so", ORACLE / "etc1s_oracle.h", "ORC_API", "make")
CHECKERS["ref"] = (ORACLE / "_ref" / "libref_harness.so", ORACLE / "ref_harness.cpp", "REF_API", "prebuilt")


def include_closure(source):
    """the source and every file it includes in quotes, directly or not; each include is looked up next to the file that names it"""
    seen, todo = [], [pathlib.Path(source).resolve()]
    while todo:
        f = todo.pop()
        if f not in seen and f.exists():
            seen.append(f)
            todo += [(f.parent / inc).resolve() for inc in re.findall(r'^[ \t]*#[ \t]*include[ \t]+"([^"]+)"', f.read_text(), re.M)]
    return seen


def is_stale(library, source):
    return not library.exists() or library.stat().st_mtime < max(f.stat().st_mtime for f in include_closure(source))


def build(library, source):
    """COMPILE into a name of this process's own, then moved into place: another process never loads a half-written file, a failed compile leaves the old one"""
    tmp = library.with_name(f"{library.name}.{os.getpid()}.tmp")
    try:
        subprocess.run(COMPILE + ["-o", str(tmp), str(source)], check=True)
        os.replace(tmp, library)
    finally:
        tmp.unlink(missing_ok=True)


@functools.lru_cache(maxsize=None)
def prototypes(name):
    _, source, mark, _ = CHECKERS[name]
    return parse_prototypes(source.read_text(), mark, name=r"\w+")


@functools.lru_cache(maxsize=None)
def load(name):
    """The CDLL of a checker, built first where it is stale, with the signature of every marked function of its source set. A marked function the file does not
    export is an AttributeError, except in the prebuilt harness: there it is left out, and hasattr() / helpers.ref_harness_version() tell."""
    library, source, _, how = CHECKERS[name]
    if how == "g++" and is_stale(library, source):
        build(library, source)
    if how == "make":
        with open(library.parent / "Makefile") as guard:
            fcntl.flock(guard, fcntl.LOCK_EX)   # released when the file closes
            subprocess.check_call(["make", "-C", str(library.parent), library.name], stdout=subprocess.DEVNULL)
    dll = C.CDLL(str(library))
    for fn_name, (res, args) in prototypes(name).items():
        if how == "prebuilt" and not hasattr(dll, fn_name):
            continue
        fn = getattr(dll, fn_name)
        fn.restype, fn.argtypes = res, args
    return dll


def load_npz_golden(path):
    """a golden .npz -> (its arrays, read-only: they are shared; its `meta` member decoded)"""
    z = np.load(path)
    arrays = {k: z[k] for k in z.files}
    for a in arrays.values():
        a.setflags(write=False)
    return arrays, json.loads(arrays["meta"].tobytes().decode())
