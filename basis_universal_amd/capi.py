"""ctypes binding of libbasisu_hip.so (include/basisu_hip.h).

The binding mirrors the C ABI one-to-one (the signatures come from the header, _cabi.py); nothing here computes anything. `HipLibrary` can be constructed
without a GPU (so that CPU-only CI can check that the library loads and exports every declared symbol); creating a context without a GPU raises HipError.
"""
import weakref
import ctypes as C
import functools
import pathlib

import numpy as np

from . import _cabi
from ._cabi import HipError, LIB_DIR, PKG_DIR  # noqa: F401

LIB_PATH = _cabi.library_path("hip")
HEADER_PATH = _cabi.INCLUDE_DIR / "basisu_hip.h"

_vp = C.c_void_p
_u32 = C.c_uint32


def declared_symbols(header=HEADER_PATH):
    """Every BU_HIP_API function name declared in include/basisu_hip.h."""
    return sorted(_cabi.parse_prototypes(pathlib.Path(header).read_text()))


class Tuning(C.Structure):  # = bu_hip_tuning, include/basisu_hip.h
    _fields_ = [(n, C.c_uint32) for n in ("struct_bytes", "tsvq_wide_min", "tsvq_wide6_min", "tsvq_wide_cov_min", "tsvq_windows", "tsvq_dense_min", "tsvq_zero_copy",
                                          "tsvq_chained_only", "tsvq_poll", "refine_unsorted", "debug", "tsvq_deep_levels", "uastc_walk_cus", "codebook_wide_min")]


class HipLibrary:
    def __init__(self, path=LIB_PATH):
        self.path = pathlib.Path(path)
        self.dll = _cabi.open_library("hip", self.path)  # AttributeError = a declared symbol is missing = broken build
        for name in _cabi.PROTOTYPES["hip"]:
            if name != "bu_hip_last_error":
                setattr(self, name[len("bu_hip_"):], getattr(self.dll, name))

    def last_error(self, ctx=None):
        s = self.dll.bu_hip_last_error(ctx)
        return s.decode() if s else ""


load_library = functools.lru_cache(maxsize=None)(HipLibrary)


class Context:
    """One bu_hip_context (= one HIP stream + resident buffers). Raises HipError if no GPU is usable."""

    def __init__(self, device=None, lib=None):
        self.lib = lib or load_library()
        if not self.lib.init(0):
            raise HipError("bu_hip_init failed: " + self.lib.last_error(None))
        self.h = self.lib.create_context() if device is None else self.lib.create_context_on(int(device))
        if not self.h:
            raise HipError("bu_hip_create_context failed: " + self.lib.last_error(None))
        self._dependants = weakref.WeakSet()

    def adopt(self, obj):
        """Registers an object that owns device memory of this context (it must have close()): closing the context closes it first,
        so that a dependant collected later never frees through a dead context."""
        self._dependants.add(obj)

    def check(self, ok, what=""):
        if not ok:
            raise HipError(f"{what} failed: {self.lib.last_error(self.h)}")

    def tuning(self):
        """bu_hip_get_tuning: this context's path-selection knobs as a dict (all paths are bit-identical; see include/basisu_hip.h)."""
        t = Tuning()
        self.lib.get_tuning(self.h, C.byref(t), C.sizeof(t))
        return {n: getattr(t, n) for n, _ in Tuning._fields_ if n != "struct_bytes"}

    def set_tuning(self, **fields):
        """bu_hip_set_tuning: the process defaults with `fields` replaced (no arguments = back to the defaults); codebook builds started on this context afterwards take them."""
        t = Tuning()
        self.lib.get_tuning(None, C.byref(t), C.sizeof(t))
        for k, v in fields.items():
            if k not in dict(Tuning._fields_) or k == "struct_bytes":
                raise KeyError(k)
            setattr(t, k, int(v))
        t.struct_bytes = C.sizeof(t)
        self.check(self.lib.set_tuning(self.h, C.byref(t)), "bu_hip_set_tuning")

    def close(self):
        if getattr(self, "h", None):
            for d in list(getattr(self, "_dependants", ())):
                d.close()
            self.lib.destroy_context(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- raw device memory helpers (used by tests and the host frontend; torch tensors can be passed by data_ptr instead)
    def alloc(self, nbytes):
        p = self.lib.malloc(self.h, int(nbytes))
        if not p:
            raise HipError("bu_hip_malloc failed: " + self.lib.last_error(self.h))
        return p

    def free(self, p):
        self.lib.free(self.h, p)

    def upload(self, arr):
        arr = np.ascontiguousarray(arr)
        p = self.alloc(max(arr.nbytes, 1))
        if arr.nbytes:
            self.memcpy_h2d(p, arr)
        return p

    def memcpy_h2d(self, d, arr):
        """bu_hip_memcpy_h2d: `arr` (C-contiguous) to device pointer `d`; synchronises."""
        if not arr.flags.c_contiguous:
            raise ValueError("memcpy_h2d takes a C-contiguous array")
        self.check(self.lib.memcpy_h2d(self.h, _vp(d), arr.ctypes.data_as(_vp), arr.nbytes), "memcpy_h2d")

    def download(self, p, shape, dtype):
        out = np.empty(shape, dtype)
        self.check(self.lib.memcpy_d2h(self.h, out.ctypes.data_as(_vp), p, out.nbytes), "memcpy_d2h")
        return out

    def memcpy_h2d_async(self, d, arr):
        """bu_hip_memcpy_h2d_async: `arr` (C-contiguous) to device pointer `d`, ordered on the context's stream; `arr` may be overwritten or released on return."""
        if not arr.flags.c_contiguous:
            raise ValueError("memcpy_h2d_async takes a C-contiguous array")
        self.check(self.lib.memcpy_h2d_async(self.h, _vp(d), arr.ctypes.data_as(_vp), arr.nbytes), "memcpy_h2d_async")

    def memcpy_d2d(self, dst, src, nbytes):
        """bu_hip_memcpy_d2d: ordered on the context's stream, no host synchronisation."""
        self.check(self.lib.memcpy_d2d(self.h, _vp(dst), _vp(src), int(nbytes)), "memcpy_d2d")

    def memcpy_d2h(self, arr, src):
        """bu_hip_memcpy_d2h into an existing (C-contiguous, writable) array; synchronises."""
        if not (arr.flags.c_contiguous and arr.flags.writeable):
            raise ValueError("memcpy_d2h takes a writable C-contiguous array")
        self.check(self.lib.memcpy_d2h(self.h, arr.ctypes.data_as(_vp), _vp(src), arr.nbytes), "memcpy_d2h")

    def memset(self, d, value, nbytes):
        """bu_hip_memset: ordered on the context's stream."""
        self.check(self.lib.memset(self.h, _vp(d), int(value), int(nbytes)), "memset")

    def device(self):
        """bu_hip_context_device"""
        return self.lib.context_device(self.h)

    def set_stream(self, stream=None):
        """bu_hip_set_stream: run on an externally owned hipStream_t (its address as an int: torch's cuda_stream, another context's get_stream()); None = back to the context's own."""
        self.check(self.lib.set_stream(self.h, _vp(stream)), "set_stream")

    def get_stream(self):
        """bu_hip_get_stream: the address of the hipStream_t the context enqueues on."""
        return self.lib.get_stream(self.h)

    def set_wait_hook(self, fn=None, user=None):
        """bu_hip_set_wait_hook: fn is a ctypes.CFUNCTYPE(None, c_void_p) instance the caller keeps alive while it is installed; None removes the hook."""
        self.check(self.lib.set_wait_hook(self.h, fn, _vp(user)), "set_wait_hook")

    def profile_enable(self, on=True):
        self.check(self.lib.profile_enable(self.h, int(on)), "profile_enable")

    def profile_read(self):
        """{kernel name: (total ms, launches)} from HIP events on the launch stream since profile_enable(True)."""
        names = (C.c_char_p * 32)(); ms = (C.c_double * 32)(); cnt = (_u32 * 32)()
        n = min(self.lib.profile_read(self.h, names, ms, cnt, 32), 32)
        return {names[i].decode(): (ms[i], cnt[i]) for i in range(n)}

    def sync(self):
        self.check(self.lib.sync(self.h), "sync")
