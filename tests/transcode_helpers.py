"""Test-only helpers of the UASTC transcoder tests: the g++ build of basis_universal_amd/csrc/uastc_transcode.h (tests/native/transcode_host.cpp)."""
import ctypes as C
import pathlib
import subprocess

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parent.parent
u8p = C.POINTER(C.c_uint8)

# transcoder_texture_format values (basis_universal_amd.transcode has the same constants; kept here so the host tests do not need the package's library)
BC1, BC3, BC4, BC5, BC7, ASTC, RGBA32 = 2, 3, 4, 5, 6, 10, 13
BYTES = {BC1: 8, BC3: 16, BC4: 8, BC5: 16, BC7: 16, ASTC: 16, RGBA32: 64}

_lib = None


def transcode_host():
    global _lib
    if _lib is None:
        d, csrc = ROOT / "tests" / "native", ROOT / "basis_universal_amd" / "csrc"
        so = d / "libtranscode_host.so"
        srcs = [d / "transcode_host.cpp"] + [csrc / n for n in ("uastc_transcode.h", "uastc_transcode_tables.inc", "uastc_rdo.h", "uastc_core.h", "uastc_tables.inc")]
        if not so.exists() or so.stat().st_mtime < max(s.stat().st_mtime for s in srcs):
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-o", str(so), str(srcs[0])])
        L = C.CDLL(str(so))
        for n in ("ht_rgba32", "ht_astc", "ht_bc7"):
            getattr(L, n).restype = C.c_uint32
            getattr(L, n).argtypes = [u8p, C.c_uint32, u8p, u8p]
        L.ht_bcn.restype = C.c_uint32
        L.ht_bcn.argtypes = [u8p, C.c_uint32, C.c_uint32, C.c_int, C.c_uint32, C.c_uint32, u8p, u8p]
        L.ht_bc1_hints.restype = C.c_uint32
        L.ht_bc1_hints.argtypes = [u8p]
        L.ht_mode.restype = C.c_uint32
        L.ht_mode.argtypes = [u8p]
        _lib = L
    return _lib


def _p(a):
    return a.ctypes.data_as(u8p)


def host_transcode(blocks, target, high_quality=False, channels=(0, 3)):
    """-> (per-block output (n, bytes) uint8 -- RGBA32 as (n, 4, 4, 4) --, ok flags (n,) uint8). Refused blocks are zero-filled."""
    L = transcode_host()
    blocks = np.ascontiguousarray(blocks, np.uint8).reshape(-1, 16)
    n = blocks.shape[0]
    out, ok = np.zeros((n, BYTES[target]), np.uint8), np.zeros(n, np.uint8)
    if target == RGBA32:
        L.ht_rgba32(_p(blocks), n, _p(out), _p(ok))
        return out.reshape(n, 4, 4, 4), ok
    if target == ASTC:
        L.ht_astc(_p(blocks), n, _p(out), _p(ok))
    elif target == BC7:
        L.ht_bc7(_p(blocks), n, _p(out), _p(ok))
    else:
        L.ht_bcn(_p(blocks), n, target, int(high_quality), channels[0], channels[1], _p(out), _p(ok))
    return out, ok


def block_modes(blocks):
    L = transcode_host()
    blocks = np.ascontiguousarray(blocks, np.uint8).reshape(-1, 16)
    return np.array([L.ht_mode(_p(blocks[i])) for i in range(blocks.shape[0])], np.uint32)


def bc1_routes(blocks):
    """per block: 0 solid / invalid, otherwise 1 | hint0 << 1 | hint1 << 2"""
    L = transcode_host()
    blocks = np.ascontiguousarray(blocks, np.uint8).reshape(-1, 16)
    return np.array([L.ht_bc1_hints(_p(blocks[i])) for i in range(blocks.shape[0])], np.uint32)


def to_raster(tiles, nbx, nby, width, height):
    """(nby * nbx, 4, 4, 4) decoded tiles -> the (height, width, 4) image they cover, cropped"""
    return tiles.reshape(nby, nbx, 4, 4, 4).transpose(0, 2, 1, 3, 4).reshape(nby * 4, nbx * 4, 4)[:height, :width]
