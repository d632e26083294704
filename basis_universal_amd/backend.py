"""ETC1S backend: Python view of bu::etc1s_backend through the C ABI of include/basisu_hip_backend.h.

Mirrors basisu_backend (encoder/basisu_backend.h:278-408): a finished frontend in, the compressed payloads of a .basis / KTX2 file
out. Host code in libbasisu_frontend.so; no GPU is needed when it is driven from plain arrays (`Etc1sBackend.from_arrays`), the
frontend-driven form (`Etc1sBackend.from_frontend`) needs the frontend's device for compression levels above 1.
"""
import ctypes as C

import numpy as np

from .etc1s import load_frontend_library

_vp = C.c_void_p


class BackendParams(C.Structure):
    _fields_ = [("endpoint_rdo_quality_thresh", C.c_float), ("selector_rdo_quality_thresh", C.c_float), ("compression_level", C.c_uint32), ("video", C.c_uint32)]


class SliceDesc(C.Structure):
    _fields_ = [(n, C.c_uint32) for n in ("first_block_index", "orig_width", "orig_height", "width", "height", "num_blocks_x", "num_blocks_y",
                                            "source_file_index", "mip_index")] + [("alpha", C.c_uint8), ("iframe", C.c_uint8), ("reserved", C.c_uint8 * 2)]


class KeyValue(C.Structure):
    _fields_ = [("key", C.c_char_p), ("value", _vp), ("value_size", C.c_uint32)]


class BackendArrays(C.Structure):
    _fields_ = [("total_blocks", C.c_uint32), ("perceptual", C.c_int), ("source_blocks", _vp), ("output_blocks", _vp), ("block_endpoint_index", _vp),
                ("block_selector_index", _vp), ("total_endpoints", C.c_uint32), ("endpoint_color5_inten", _vp), ("total_selectors", C.c_uint32),
                ("selector_blocks", _vp)]


class BackendError(RuntimeError):
    pass


_lib = load_frontend_library


def default_params(quality_level=-1, compression_level=1):
    """basis_compressor's backend thresholds for a quality level -> (endpoint_rdo_thresh, selector_rdo_thresh)."""
    L = _lib()
    p = BackendParams()
    L.bu_backend_default_params(int(quality_level), int(compression_level), C.byref(p))
    return p.endpoint_rdo_quality_thresh, p.selector_rdo_quality_thresh


def slice_descs(slices):
    """[(first_block, num_blocks_x, num_blocks_y[, orig_width, orig_height[, image_index, mip_index, alpha]])] -> SliceDesc array.
    Without the optional fields: unpadded size = padded size, slice i is mip 0 of image i (what the parity harness uses)."""
    arr = (SliceDesc * len(slices))()
    for i, s in enumerate(slices):
        first, nbx, nby = s[:3]
        ow, oh = (s[3], s[4]) if len(s) >= 5 else (nbx * 4, nby * 4)
        image, mip, alpha = (s[5], s[6], s[7]) if len(s) >= 8 else (i, 0, 0)
        iframe = s[8] if len(s) >= 9 else 0
        arr[i] = SliceDesc(first, ow, oh, nbx * 4, nby * 4, nbx, nby, image, mip, int(alpha), int(iframe))
    return arr


def _key_values(key_values):
    kvs = (KeyValue * max(len(key_values), 1))()
    keep = []
    for i, (k, v) in enumerate(key_values):
        vb = np.frombuffer(bytes(v), np.uint8) if len(v) else np.zeros(0, np.uint8)
        keep.append(vb)
        kvs[i] = KeyValue(k.encode(), vb.ctypes.data_as(_vp) if vb.size else None, vb.size)
    return kvs, keep


def uastc_basis_file(blocks16, slices, srgb=True, tex_type=0, userdata0=0, userdata1=0, y_flipped=False, us_per_frame=0, key_values=()):
    """The .basis container around UASTC LDR 4x4 blocks ((n, 16) u8, e.g. uastc.encode_uastc_blocks / uastc.uastc_rdo output)."""
    L = _lib()
    b = np.ascontiguousarray(blocks16, np.uint8).reshape(-1, 16)
    kvs, keep = _key_values(key_values)
    sl = slice_descs(slices)
    args = (b.ctypes.data_as(_vp), b.shape[0], sl, len(slices), int(srgb), tex_type, userdata0, userdata1, int(y_flipped), us_per_frame, kvs, len(key_values))
    need = L.bu_write_basis_file_uastc(*args, None, 0)
    if not need:
        raise BackendError("bu_write_basis_file_uastc failed")
    buf = np.zeros(need, np.uint8)
    L.bu_write_basis_file_uastc(*args, buf.ctypes.data_as(_vp), need)
    return buf


def uastc_ktx2_file(blocks16, slices, srgb=True, tex_type=0, has_alpha=False, key_values=()):
    """The KTX2 container (no supercompression) around UASTC LDR 4x4 blocks."""
    L = _lib()
    b = np.ascontiguousarray(blocks16, np.uint8).reshape(-1, 16)
    kvs, keep = _key_values(key_values)
    sl = slice_descs(slices)
    args = (b.ctypes.data_as(_vp), b.shape[0], sl, len(slices), int(srgb), tex_type, int(has_alpha), kvs, len(key_values))
    need = L.bu_write_ktx2_file_uastc(*args, None, 0)
    if not need:
        raise BackendError("bu_write_ktx2_file_uastc failed")
    buf = np.zeros(need, np.uint8)
    L.bu_write_ktx2_file_uastc(*args, buf.ctypes.data_as(_vp), need)
    return buf


class Etc1sBackend:
    def __init__(self):
        self.L = _lib()
        self.h = self.L.bu_backend_create()
        self._keep = []

    @classmethod
    def from_frontend(cls, frontend, slices, endpoint_rdo_thresh=1.5, selector_rdo_thresh=1.25, compression_level=1, video=False):
        """frontend: a compressed basis_universal_amd.etc1s.Etc1sFrontend (kept alive by this object)."""
        b = cls()
        prm = BackendParams(endpoint_rdo_thresh, selector_rdo_thresh, compression_level, int(video))
        sl = slice_descs(slices)
        b._keep = [frontend]
        if not b.L.bu_backend_init(b.h, frontend.h, C.byref(prm), sl, len(slices)):
            raise BackendError("bu_backend_init failed")
        return b

    @classmethod
    def from_arrays(cls, source_blocks, output_blocks, block_endpoint_index, block_selector_index, endpoint_color5_inten, selector_blocks, slices,
                    perceptual=True, endpoint_rdo_thresh=1.5, selector_rdo_thresh=1.25, compression_level=1, video=False):
        b = cls()
        src = np.ascontiguousarray(source_blocks, np.uint8)
        out = np.ascontiguousarray(output_blocks, np.uint8)
        ei = np.ascontiguousarray(block_endpoint_index, np.uint32)
        si = np.ascontiguousarray(block_selector_index, np.uint32)
        ep = np.ascontiguousarray(endpoint_color5_inten, np.uint8).reshape(-1, 4)
        sb = np.ascontiguousarray(selector_blocks, np.uint8).reshape(-1, 8)
        b._keep = [src, out, ei, si, ep, sb]
        p = lambda a: a.ctypes.data_as(_vp)
        arrays = BackendArrays(ei.size, int(perceptual), p(src), p(out), p(ei), p(si), ep.shape[0], p(ep), sb.shape[0], p(sb))
        prm = BackendParams(endpoint_rdo_thresh, selector_rdo_thresh, compression_level, int(video))
        sl = slice_descs(slices)
        if not b.L.bu_backend_init_arrays(b.h, C.byref(arrays), C.byref(prm), sl, len(slices)):
            raise BackendError("bu_backend_init_arrays failed")
        b._total_endpoints = int(ep.shape[0])   # the length of the old_to_new array the C side hands to the reoptimize call-back
        return b

    REOPTIMIZE_FN = C.CFUNCTYPE(C.c_int, _vp, C.POINTER(C.c_uint32), C.c_uint32, C.POINTER(C.c_int32), C.c_int, C.POINTER(C.c_uint32), C.POINTER(BackendArrays))

    def set_reoptimize(self, fn):
        """fn(new_block_endpoints (u32 array), final_codebook (bool), block_selector_indices (u32 array or None)) -> (old_to_new int32 array,
        dict of the arrays from_arrays takes, describing the frontend afterwards): the frontend call-back of compression levels above 1
        for a backend driven from plain arrays."""
        def thunk(user, nbe, n, o2n, final, bsi, refreshed):
            try:
                new_ep = np.ctypeslib.as_array(nbe, (n,)).copy()
                sel = np.ctypeslib.as_array(bsi, (n,)).copy() if bsi else None
                old_to_new, arrays = fn(new_ep, bool(final), sel)
                old_to_new = np.ascontiguousarray(old_to_new, np.int32)
                have = getattr(self, "_total_endpoints", None)
                if have is not None and old_to_new.size != have:   # the C buffer holds exactly one entry per endpoint of the codebook being replaced
                    raise BackendError(f"reoptimize call-back returned {old_to_new.size} old_to_new entries for a codebook of {have}")
                C.memmove(o2n, old_to_new.ctypes.data, old_to_new.nbytes)
                src = np.ascontiguousarray(arrays["source_blocks"], np.uint8)
                out = np.ascontiguousarray(arrays["output_blocks"], np.uint8)
                ei = np.ascontiguousarray(arrays["block_endpoint_index"], np.uint32)
                si = np.ascontiguousarray(arrays["block_selector_index"], np.uint32)
                ep = np.ascontiguousarray(arrays["endpoint_color5_inten"], np.uint8).reshape(-1, 4)
                sb = np.ascontiguousarray(arrays["selector_blocks"], np.uint8).reshape(-1, 8)
                if src.size != ei.size * 64 or out.size != ei.size * 8 or si.size != ei.size or n != ei.size:
                    raise BackendError("reoptimize call-back returned arrays of inconsistent sizes")
                self._keep_cb = [src, out, ei, si, ep, sb]
                self._total_endpoints = int(ep.shape[0])
                p = lambda a: a.ctypes.data
                r = refreshed.contents
                r.total_blocks, r.perceptual = ei.size, int(arrays.get("perceptual", True))
                r.source_blocks, r.output_blocks, r.block_endpoint_index, r.block_selector_index = p(src), p(out), p(ei), p(si)
                r.total_endpoints, r.endpoint_color5_inten, r.total_selectors, r.selector_blocks = ep.shape[0], p(ep), sb.shape[0], p(sb)
                return 1
            except Exception:
                import traceback
                traceback.print_exc()
                return 0
        self._cb = self.REOPTIMIZE_FN(thunk)
        if not self.L.bu_backend_set_reoptimize_callback(self.h, C.cast(self._cb, _vp), None):
            raise BackendError("bu_backend_set_reoptimize_callback failed")

    def encode(self):
        n = self.L.bu_backend_encode(self.h)
        if not n:
            raise BackendError("bu_backend_encode failed: " + self.L.bu_backend_error(self.h).decode())
        return n

    def get(self, name, slice_index=0, dtype=np.uint8):
        need = self.L.bu_backend_get(self.h, name.encode(), slice_index, None, 0)
        if need == 2 ** 64 - 1:
            raise KeyError(name)
        buf = np.zeros(need, np.uint8)
        self.L.bu_backend_get(self.h, name.encode(), slice_index, buf.ctypes.data_as(_vp), need)
        return buf.view(dtype)

    def basis_file(self, tex_type=0, userdata0=0, userdata1=0, y_flipped=False, us_per_frame=0, key_values=()):
        """The .basis container around the encoded output (basisu_file::init); key_values: [(str, bytes), ...]."""
        kvs = (KeyValue * max(len(key_values), 1))()
        keep = []
        for i, (k, v) in enumerate(key_values):
            vb = np.frombuffer(bytes(v), np.uint8) if len(v) else np.zeros(0, np.uint8)
            keep.append(vb)
            kvs[i] = KeyValue(k.encode(), vb.ctypes.data_as(_vp) if vb.size else None, vb.size)
        args = (self.h, tex_type, userdata0, userdata1, int(y_flipped), us_per_frame, kvs, len(key_values))
        need = self.L.bu_backend_write_basis_file(*args, None, 0)
        if not need:
            raise BackendError("bu_backend_write_basis_file failed")
        buf = np.zeros(need, np.uint8)
        self.L.bu_backend_write_basis_file(*args, buf.ctypes.data_as(_vp), need)
        return buf

    def ktx2_file(self, tex_type=0, has_alpha=False, key_values=()):
        """The KTX2 container (BasisLZ) around the encoded output (basis_compressor::create_ktx2_file); key_values: [(str, bytes), ...]."""
        kvs, keep = _key_values(key_values)
        args = (self.h, tex_type, int(has_alpha), kvs, len(key_values))
        need = self.L.bu_backend_write_ktx2_file(*args, None, 0)
        if not need:
            raise BackendError("bu_backend_write_ktx2_file failed")
        buf = np.zeros(need, np.uint8)
        self.L.bu_backend_write_ktx2_file(*args, buf.ctypes.data_as(_vp), need)
        return buf

    def stage_times(self):
        names = (C.c_char_p * 16)()
        secs = (C.c_double * 16)()
        n = min(self.L.bu_backend_stage_times(self.h, names, secs, 16), 16)
        return [(names[i].decode(), secs[i]) for i in range(n)]

    def close(self):
        if self.h:
            self.L.bu_backend_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
