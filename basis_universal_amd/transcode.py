"""UASTC LDR 4x4 -> GPU texture formats on the GPU: the host-side mirror of basist::basisu_lowlevel_uastc_ldr_4x4_transcoder::transcode_slice
(transcoder/basisu_transcoder.cpp:10078) as a batch op, a reader for the two UASTC containers this package writes, and `transcode_file` on top of both.

Targets are the reference's transcoder_texture_format values; only the ones below exist here. `transcode_uastc_blocks`, `transcode_file` and `transcode_file_images`
take RGBA32, BC1, BC3, BC4, BC5, BC7 and ASTC 4x4 and refuse everything else. `transcode_uastc_texture_blocks`, `transcode_uastc_texture_file`, `transcode_uastc_textures`
and `uastc_texture_layout` are a parallel UASTC family (UASTC_TEXTURE_BYTES_PER_BLOCK / UASTC_TEXTURE_BYTES_PER_PIXEL): those seven targets, byte for byte the same, plus
the consumers of the ETC hints every UASTC block carries -- ETC1_RGB, ETC2_RGBA, ETC2_EAC_R11 / ETC2_EAC_RG11 -- and the RGB565 / BGR565 / RGBA4444 rasters, (height,
width) u16. ETC1 from the alpha channel (cDecodeFlagsTranscodeAlphaDataToOpaqueFormats), ATC / FXT1 / PVRTC2 from UASTC (the reference has no such route), UASTC HDR / ASTC LDR / XUASTC and
Zstandard-supercompressed KTX2 levels are out of scope and are refused with an error. There is no CPU implementation: without the HIP library and a GPU the
transcode functions raise.

ETC1S files have their own three functions at the end of this module (`read_etc1s_file`, `decode_etc1s_file`, `transcode_etc1s_file`) and their own target list
(ETC1S_BYTES_PER_BLOCK / ETC1S_BYTES_PER_PIXEL): the serial half -- containers, Huffman tables, palettes, the per-slice symbol walk -- is host code in
libbasisu_frontend.so (csrc/host/etc1s_decode.cpp, needs no GPU), the texel half is one HIP kernel launch per image (csrc/etc1s_transcode_kernels.hip).

`transcode_etc1s_texture`, `transcode_etc1s_textures` and `etc1s_texture_layout` are a parallel ETC1S family with two more targets, ETC2 RGBA and BC7 RGBA (16 bytes
per block, ETC1S_TEXTURE_BYTES_PER_BLOCK), and BC7's chroma filter as an option; the three functions above keep their six targets and their refusals.
`transcode_etc1s_block_format`, `transcode_etc1s_block_formats` and `etc1s_block_format_layout` are a third ETC1S family with the second one's targets and three
more: ASTC 4x4 RGBA, EAC R11 and EAC RG11 (ETC1S_BLOCK_FORMAT_BYTES_PER_BLOCK); the second family keeps its eight targets and its refusals.
`transcode_etc1s_vendor_format`, `transcode_etc1s_vendor_formats` and `etc1s_vendor_format_layout` are a fourth ETC1S family with the third one's targets and four
more: ATC RGB, FXT1 (16 bytes per 8x4 texels: rows of ceil(num_blocks_x / 2) blocks) and PVRTC2 4bpp RGB / RGBA (ETC1S_VENDOR_FORMAT_BYTES_PER_BLOCK). It refuses, with the
reason, what needs the ETC1S -> BC4 look-up (BC3, BC4, BC5, ATC RGBA).

`transcode_file_images` and `transcode_etc1s_file_images` are the whole-file forms: every image of a file -- levels x layers x faces -- by ONE
launch over a slice table, into one allocation whose layout `image_layout` gives.

PVRTC1 4bpp RGB / RGBA (PVRTC1_4_RGB, PVRTC1_4_RGBA; power-of-two images only) is a family of its own for both codecs, the last section, because a PVRTC1 block
depends on the blocks around it: `transcode_uastc_pvrtc1_blocks`, `transcode_uastc_pvrtc1_file`, `transcode_etc1s_pvrtc1_image`, `transcode_etc1s_pvrtc1`, and for
every image of a file of either codec `transcode_pvrtc1_images` with `pvrtc1_layout`. Every other family keeps refusing those two targets.

Back to pixels: `unpack_blocks` (BC1 / BC3 / BC4 / BC5 / BC7) and, at the end of the module, `unpack_texture` (UNPACK_TEXTURE_BYTES_PER_BLOCK): those five and every other
block target above -- ETC1, ETC2 RGBA, EAC R11 / RG11, ASTC 4x4, PVRTC1 -- as RGBA8, what the reference's gpu_image::unpack makes of them (csrc/texture_unpack_kernels.hip).
"""
import contextlib
import ctypes as C
import struct

import numpy as np

from .etc1s import load_frontend_library

BC1_RGB, BC3_RGBA, BC4_R, BC5_RG, BC7_RGBA, ASTC_4x4_RGBA, RGBA32 = 2, 3, 4, 5, 6, 10, 13
BYTES_PER_BLOCK = {BC1_RGB: 8, BC3_RGBA: 16, BC4_R: 8, BC5_RG: 16, BC7_RGBA: 16, ASTC_4x4_RGBA: 16, RGBA32: 64}
DECODE_FLAGS_HIGH_QUALITY = 32   # cDecodeFlagsHighQuality


class InvalidBlocksError(ValueError):
    """Some blocks did not unpack as UASTC -- or, from unpack_blocks / unpack_texture, as the block format they were given as -- (their output was zero-filled). `count` is how many. From the whole-file calls
    (transcode_file_images, transcode_etc1s_file_images) `per_slice` is the count of every slice in table order and `slice` the lowest slice that has any."""

    def __init__(self, count, total, what="UASTC LDR 4x4", per_slice=None):
        self.count, self.per_slice = count, None if per_slice is None else [int(c) for c in per_slice]
        self.slice = None if per_slice is None else next(s for s, c in enumerate(self.per_slice) if c)
        where = "" if per_slice is None else f", the first in slice {self.slice} (per slice: {self.per_slice})"
        super().__init__(f"{count} of {total} blocks are not valid {what} blocks{where}")


@contextlib.contextmanager
def _output(ctx, out_device, out_row_pitch, out_rows, nbytes):
    """where a transcode writes: the caller's out_device, or a buffer of nbytes() bytes of our own, freed on the way out"""
    if out_device is not None:
        yield out_device
        return
    if out_row_pitch or out_rows:
        raise ValueError("out_row_pitch / out_rows describe a caller-owned raster: give out_device")
    d_out = ctx.alloc(max(nbytes(), 1))
    try:
        yield d_out
    finally:
        ctx.free(d_out)


def _check_uastc_target(target):
    target = int(target)
    if target not in BYTES_PER_BLOCK:
        raise ValueError(f"transcode target {target} is not supported (supported: {sorted(BYTES_PER_BLOCK)})")
    return target


def _channel_pair(channels):
    """channels=(c,) / (c0, c1) / None -> the C ABI's two values, -1 = the reference's default"""
    ch = tuple(channels) if channels is not None else ()
    if len(ch) > 2 or any(not 0 <= int(c) <= 3 for c in ch):
        raise ValueError("channels: up to two values in 0..3")
    return (int(ch[0]) if len(ch) > 0 else -1), (int(ch[1]) if len(ch) > 1 else -1)


def transcode_uastc_blocks(ctx, blocks, nbx, nby, target, *, width=None, height=None, high_quality=False, channels=None, out_device=None,
                           out_row_pitch=0, out_rows=0):
    """blocks: (nby * nbx, 16) uint8 array in raster order (uploaded once) or a device pointer (int) to that many resident blocks.
    Returns (nby * nbx, bytes_per_block) uint8, for RGBA32 the (height, width, 4) raster, or None when out_device (a device pointer with room for
    bu_hip_transcode_output_bytes, or for out_rows x out_row_pitch pixels when those are given) receives the output. width / height default to the padded size;
    channels: BC4's (c,) or BC5's (c0, c1), default (0,) / (0, 3). Raises InvalidBlocksError when a block does not unpack."""
    nbx, nby, target = int(nbx), int(nby), _check_uastc_target(target)
    n = nbx * nby
    width, height = int(width or nbx * 4), int(height or nby * 4)
    if not (0 < width <= nbx * 4 and 0 < height <= nby * 4) and n:
        raise ValueError(f"{width} x {height} pixels do not fit {nbx} x {nby} blocks")
    c0, c1 = _channel_pair(channels)
    own = None
    try:
        if isinstance(blocks, np.ndarray):
            blocks = np.ascontiguousarray(blocks, np.uint8)
            if blocks.size != n * 16:
                raise ValueError(f"{nbx} x {nby} blocks need {n * 16} bytes, got {blocks.size}")
            blocks = own = ctx.upload(blocks) if n else 0
        with _output(ctx, out_device, out_row_pitch, out_rows, lambda: ctx.lib.transcode_output_bytes(nbx, nby, width, height, target)) as d_out:
            invalid = C.c_uint32(0)
            if n:
                ctx.check(ctx.lib.k_transcode_uastc(ctx.h, C.c_void_p(blocks), nbx, nby, width, height, target, DECODE_FLAGS_HIGH_QUALITY if high_quality else 0, c0, c1,
                                                    C.c_void_p(d_out), int(out_row_pitch), int(out_rows), C.byref(invalid)), "transcode_uastc")
            if invalid.value:
                raise InvalidBlocksError(invalid.value, n)
            if out_device is not None:
                return None
            if target == RGBA32:
                return ctx.download(d_out, (height, width, 4), np.uint8) if n else np.zeros((0, 0, 4), np.uint8)
            return ctx.download(d_out, (n, BYTES_PER_BLOCK[target]), np.uint8) if n else np.zeros((0, BYTES_PER_BLOCK[target]), np.uint8)
    finally:
        if own:
            ctx.free(own)


# ---------------------------------------------------------------- block formats back to pixels

UNPACK_BYTES_PER_BLOCK = {BC1_RGB: 8, BC3_RGBA: 16, BC4_R: 8, BC5_RG: 16, BC7_RGBA: 16}


def unpack_blocks(ctx, blocks, nbx, nby, fmt, *, width=None, height=None, out_device=None, out_row_pitch=0, out_rows=0):
    """gpu_image::unpack on the GPU: what a BC1 / BC3 / BC4 / BC5 / BC7 texture (fmt: the transcoder's target value, UNPACK_BYTES_PER_BLOCK) samples as, RGBA8.
    blocks: (nby * nbx, 8 | 16) uint8 array in raster order (uploaded once) or a device pointer (int) to that many resident blocks, as transcode_uastc_blocks writes them.
    Returns the (height, width, 4) raster, or None when out_device (a device pointer with room for out_rows x out_row_pitch pixels, 0 = height / width) receives it;
    width / height default to the padded size. BC1 keeps its punch-through alpha, BC4 fills R and BC5 R, G (the rest (0, 0, 255)). The one invalid block is a BC7
    block whose first byte is 0: zero-filled, and InvalidBlocksError is raised with their count. There is no CPU implementation."""
    nbx, nby, fmt = int(nbx), int(nby), int(fmt)
    if fmt not in UNPACK_BYTES_PER_BLOCK:
        name = _TARGET_NAMES[fmt] if 0 <= fmt < len(_TARGET_NAMES) else "unknown"
        raise ValueError(f"block format {fmt} ({name}) does not unpack here (supported: {sorted(UNPACK_BYTES_PER_BLOCK)})")
    n, unit = nbx * nby, UNPACK_BYTES_PER_BLOCK[fmt]
    width, height = int(width or nbx * 4), int(height or nby * 4)
    if not (0 < width <= nbx * 4 and 0 < height <= nby * 4) and n:
        raise ValueError(f"{width} x {height} pixels do not fit {nbx} x {nby} blocks")
    with _output(ctx, out_device, out_row_pitch, out_rows, lambda: ctx.lib.unpack_output_bytes(nbx, nby, width, height, 0, 0)) as d_out:
        own = None
        try:
            if isinstance(blocks, np.ndarray):
                blocks = np.ascontiguousarray(blocks, np.uint8)
                if blocks.size != n * unit:
                    raise ValueError(f"{nbx} x {nby} blocks need {n * unit} bytes, got {blocks.size}")
                blocks = own = ctx.upload(blocks) if n else 0
            invalid = C.c_uint32(0)
            if n:
                ctx.check(ctx.lib.k_unpack_blocks(ctx.h, C.c_void_p(blocks), nbx, nby, width, height, fmt, C.c_void_p(d_out), int(out_row_pitch), int(out_rows), C.byref(invalid)),
                          "unpack_blocks")
            if invalid.value:
                raise InvalidBlocksError(invalid.value, n, "BC7")
            if out_device is not None:
                return None
            return ctx.download(d_out, (height, width, 4), np.uint8) if n else np.zeros((0, 0, 4), np.uint8)
        finally:
            if own:
                ctx.free(own)


# ---------------------------------------------------------------- containers

_KTX2_MAGIC = bytes([0xAB, 0x4B, 0x54, 0x58, 0x20, 0x32, 0x30, 0xBB, 0x0D, 0x0A, 0x1A, 0x0A])
_BASIS_HEADER, _BASIS_SLICE = 77, 23   # sizeof(basis_file_header), sizeof(basis_slice_desc) (transcoder/basisu_file_headers.h)


def _need(data, ofs, size, what):
    if ofs < 0 or size < 0 or ofs + size > len(data):
        raise ValueError(f"truncated or corrupt file: {what} needs bytes {ofs}..{ofs + size} of {len(data)}")


def _image(level, layer, face, width, height, ofs, what, data):
    nbx, nby = (width + 3) // 4, (height + 3) // 4
    _need(data, ofs, nbx * nby * 16, what)
    return {"level": level, "layer": layer, "face": face, "width": width, "height": height, "num_blocks_x": nbx, "num_blocks_y": nby, "offset": ofs, "length": nbx * nby * 16}


def _read_basis(data):
    _need(data, 0, _BASIS_HEADER, "the .basis header")
    (sig, ver, hsize, _hcrc, dsize, _dcrc), total_slices, total_images = struct.unpack_from("<HHHHIH", data, 0), int.from_bytes(data[14:17], "little"), int.from_bytes(data[17:20], "little")
    tex_format, flags, tex_type = data[20], struct.unpack_from("<H", data, 21)[0], data[23]
    if ver != 0x13 or hsize != _BASIS_HEADER:
        raise ValueError(f"unsupported .basis version {ver:#x} / header size {hsize}")
    if tex_format != 1 or flags & 1:
        raise ValueError("not a UASTC LDR 4x4 .basis file (ETC1S and other texture formats are not transcoded here)")
    if dsize + _BASIS_HEADER > len(data):
        raise ValueError(f"truncated .basis file: the header promises {dsize + _BASIS_HEADER} bytes, {len(data)} are here")
    descs_ofs = struct.unpack_from("<I", data, 65)[0]
    _need(data, descs_ofs, _BASIS_SLICE * total_slices, "the slice descriptors")
    if not total_slices:
        raise ValueError("a .basis file without slices")
    faces = 6 if tex_type == 2 else 1
    if total_images % faces:
        raise ValueError("a cubemap .basis file whose image count is not a multiple of 6")
    images = []
    for i in range(total_slices):
        at = descs_ofs + _BASIS_SLICE * i
        image, level, sflags = int.from_bytes(data[at:at + 3], "little"), data[at + 3], data[at + 4]
        ow, oh, nbx, nby, ofs, size, _crc = struct.unpack_from("<HHHHIIH", data, at + 5)
        if image >= total_images or not ow or not oh or nbx != (ow + 3) // 4 or nby != (oh + 3) // 4 or size != nbx * nby * 16:
            raise ValueError(f"slice {i}: inconsistent descriptor")
        # cSliceDescFlagsHasAlpha (bit 0) on a UASTC slice says that ITS image has alpha (comp.cpp:2928-2933: one face of a cubemap, one frame of a video); the
        # blocks are the same 16 bytes either way. Bit 1 marks an i-frame, which every UASTC video slice is.
        images.append(dict(_image(level, image // faces, image % faces, ow, oh, ofs, f"slice {i}", data), has_alpha=bool(sflags & 1)))
    return {"container": "basis", "format": "UASTC_LDR_4x4", "width": images[0]["width"], "height": images[0]["height"], "has_alpha": bool(flags & 4),
            "levels": sorted({im["level"] for im in images}), "layers": total_images // faces, "faces": faces, "images": images}


def _read_ktx2(data):
    _need(data, 0, 80, "the KTX2 header")
    vk_format, _type_size, width, height, depth, layers, faces, levels, scheme, dfd_ofs, dfd_len, _kvo, _kvl = struct.unpack_from("<13I", data, 12)
    if scheme != 0:
        raise ValueError(f"KTX2 supercompression scheme {scheme} is not supported (only none: BasisLZ is ETC1S, Zstandard levels are out of scope)")
    if vk_format != 0 or depth or not width or not height or faces not in (1, 6) or not 1 <= levels <= 16:
        raise ValueError("not a 2D Basis Universal KTX2 file")
    _need(data, 80, 24 * levels, "the level index")
    _need(data, dfd_ofs, dfd_len, "the data format descriptor")
    if dfd_len < 44 or data[dfd_ofs + 12] != 166:
        raise ValueError("the KTX2 data format descriptor is not UASTC's (colour model 166)")
    has_alpha = data[dfd_ofs + 28 + 3] == 3   # first sample's channel id: KTX2_DF_CHANNEL_UASTC_RGBA
    n_layers = max(layers, 1)
    images = []
    for l in range(levels):
        ofs, length, _ulen = struct.unpack_from("<3Q", data, 80 + 24 * l)
        _need(data, ofs, length, f"level {l}")
        w, h = max(width >> l, 1), max(height >> l, 1)
        per = ((w + 3) // 4) * ((h + 3) // 4) * 16
        if length != per * n_layers * faces:
            raise ValueError(f"level {l}: {length} bytes where {per * n_layers * faces} are expected")
        for layer in range(n_layers):
            for face in range(faces):
                images.append(_image(l, layer, face, w, h, ofs + (layer * faces + face) * per, f"level {l}", data))
    return {"container": "ktx2", "format": "UASTC_LDR_4x4", "width": width, "height": height, "has_alpha": has_alpha, "levels": list(range(levels)), "layers": n_layers,
            "faces": faces, "images": images}


def read_uastc_file(data):
    """Parse a UASTC .basis (cBASISTexFormatUASTC4x4) or .ktx2 (KTX2_SS_NONE, UASTC data format descriptor) file, the two containers this package writes.
    -> {"container", "format", "width", "height", "has_alpha", "levels", "layers", "faces", "images": [{"level", "layer", "face", "width", "height", "num_blocks_x",
    "num_blocks_y", "offset", "length"}]}. Every offset and length is checked against len(data); ETC1S, supercompressed or truncated files raise ValueError."""
    data = bytes(data) if not isinstance(data, (bytes, bytearray, memoryview)) else data
    if len(data) >= 12 and bytes(data[:12]) == _KTX2_MAGIC:
        return _read_ktx2(data)
    if len(data) >= 2 and bytes(data[:2]) == b"sB":
        return _read_basis(data)
    if len(data) < 12:
        raise ValueError(f"truncated file: {len(data)} bytes hold no container signature")
    raise ValueError("neither a .basis nor a .ktx2 file")


def transcode_file(ctx, data, target, *, level=0, layer=0, face=0, high_quality=False, channels=None):
    """One image of a UASTC .basis / .ktx2 file (read_uastc_file) transcoded on the GPU: blocks as transcode_uastc_blocks returns them, RGBA32 as the image."""
    raw = data.tobytes() if isinstance(data, np.ndarray) else bytes(data)
    info = read_uastc_file(raw)
    for im in info["images"]:
        if (im["level"], im["layer"], im["face"]) == (level, layer, face):
            blocks = np.frombuffer(raw, np.uint8, im["length"], im["offset"]).reshape(-1, 16)
            return transcode_uastc_blocks(ctx, blocks, im["num_blocks_x"], im["num_blocks_y"], target, width=im["width"], height=im["height"], high_quality=high_quality,
                                          channels=channels)
    raise ValueError(f"the file has no image at level {level}, layer {layer}, face {face}")


# ---------------------------------------------------------------- ETC1S files

ETC1_RGB, RGB565, BGR565, RGBA4444 = 0, 14, 15, 16   # with BC1_RGB and RGBA32 above: the ETC1S transcoder's targets (transcoder_texture_format values)
ETC1S_BYTES_PER_BLOCK = {ETC1_RGB: 8, BC1_RGB: 8}
ETC1S_BYTES_PER_PIXEL = {RGBA32: 4, RGB565: 2, BGR565: 2, RGBA4444: 2}
ETC2_RGBA = 1
ETC1S_TEXTURE_BYTES_PER_BLOCK = {ETC1_RGB: 8, BC1_RGB: 8, ETC2_RGBA: 16, BC7_RGBA: 16}   # the targets of transcode_etc1s_texture*; the pixel targets are ETC1S_BYTES_PER_PIXEL's
DECODE_FLAGS_NO_ETC1S_CHROMA_FILTERING = 64   # cDecodeFlagsNoETC1SChromaFiltering: the one decode flag of the ETC1S texture entries
# the targets of transcode_etc1s_block_format*: the texture family's and ASTC_4x4_RGBA (10), ETC2_EAC_R11 (20), ETC2_EAC_RG11 (21)
ETC1S_BLOCK_FORMAT_BYTES_PER_BLOCK = {**ETC1S_TEXTURE_BYTES_PER_BLOCK, 10: 16, 20: 8, 21: 16}
# the targets of transcode_etc1s_vendor_format*: the block-format family's and ATC_RGB (11), FXT1_RGB (17), PVRTC2_4_RGB (18), PVRTC2_4_RGBA (19). An FXT1 block is 8x4 texels
ATC_RGB, FXT1_RGB, PVRTC2_4_RGB, PVRTC2_4_RGBA = 11, 17, 18, 19
ETC1S_VENDOR_FORMAT_BYTES_PER_BLOCK = {**ETC1S_BLOCK_FORMAT_BYTES_PER_BLOCK, ATC_RGB: 8, FXT1_RGB: 16, PVRTC2_4_RGB: 8, PVRTC2_4_RGBA: 8}
_TARGET_NAMES = ["ETC1_RGB", "ETC2_RGBA", "BC1_RGB", "BC3_RGBA", "BC4_R", "BC5_RG", "BC7_RGBA", "BC7_ALT", "PVRTC1_4_RGB", "PVRTC1_4_RGBA", "ASTC_4x4_RGBA", "ATC_RGB", "ATC_RGBA",
                 "RGBA32", "RGB565", "BGR565", "RGBA4444", "FXT1_RGB", "PVRTC2_4_RGB", "PVRTC2_4_RGBA", "ETC2_EAC_R11", "ETC2_EAC_RG11"]


class _Etc1sFileInfo(C.Structure):   # = bu_etc1s_file_info, include/basisu_hip_etc1s_decode.h
    _fields_ = [(n, C.c_uint32) for n in ("container", "tex_type", "width", "height", "levels", "layers", "faces", "has_alpha_slices", "srgb", "num_endpoints", "num_selectors",
                                          "num_images")] + [("total_blocks", C.c_uint64)]


class _Etc1sImage(C.Structure):      # = bu_etc1s_image
    _fields_ = [(n, C.c_uint32) for n in ("level", "layer", "face", "width", "height", "num_blocks_x", "num_blocks_y", "reserved")] + [("first_block", C.c_uint64),
                                                                                                                                      ("alpha_first_block", C.c_uint64)]


def _decode_etc1s(data, header_only, whole=False):
    """whole (transcode_etc1s_file_images' private route): also the file's two whole index arrays, as "_endpoint_indices" / "_selector_indices", and per image where
    its slices begin in them, "_first" / "_alpha_first" -- what read_etc1s_file and decode_etc1s_file return does not have them"""
    raw = data.tobytes() if isinstance(data, np.ndarray) else bytes(data)
    L = load_frontend_library()
    err = C.create_string_buffer(512)
    h = L.bu_etc1s_decode_file(raw, len(raw), 1 if header_only else 0, err, len(err))
    if not h:
        raise ValueError(err.value.decode(errors="replace"))
    try:
        fi = _Etc1sFileInfo()
        L.bu_etc1s_file_get_info(h, C.byref(fi))
        ims = (_Etc1sImage * max(fi.num_images, 1))()
        L.bu_etc1s_file_get_images(h, ims, fi.num_images)
        images = []
        for k in range(fi.num_images):
            im = ims[k]
            images.append({"level": im.level, "layer": im.layer, "face": im.face, "width": im.width, "height": im.height, "num_blocks_x": im.num_blocks_x,
                           "num_blocks_y": im.num_blocks_y, "has_alpha": im.alpha_first_block != 2 ** 64 - 1, "_first": im.first_block, "_alpha_first": im.alpha_first_block})
        info = {"container": "ktx2" if fi.container else "basis", "format": "ETC1S", "width": fi.width, "height": fi.height, "has_alpha": bool(fi.has_alpha_slices),
                "has_alpha_slices": bool(fi.has_alpha_slices), "levels": sorted({im["level"] for im in images}), "layers": fi.layers, "faces": fi.faces, "tex_type": fi.tex_type,
                "srgb": bool(fi.srgb), "num_endpoints": fi.num_endpoints, "num_selectors": fi.num_selectors, "images": images}
        if header_only:
            for im in images:
                del im["_first"], im["_alpha_first"]
            return info

        def take(name, count, dtype):
            p = getattr(L, "bu_etc1s_file_" + name)(h)
            return np.frombuffer(C.string_at(p, count * np.dtype(dtype).itemsize), dtype).copy() if count else np.zeros(0, dtype)
        info["endpoint_palette"] = take("endpoint_palette", fi.num_endpoints * 4, np.uint8).reshape(-1, 4)
        info["selector_palette"] = take("selector_palette", fi.num_selectors, np.uint32)
        ep, sel = take("endpoint_indices", fi.total_blocks, np.uint16), take("selector_indices", fi.total_blocks, np.uint16)
        if whole:
            info["_endpoint_indices"], info["_selector_indices"] = ep, sel
        for im in images:
            n, a, b = im["num_blocks_x"] * im["num_blocks_y"], im["_first"], im["_alpha_first"]
            if not whole:
                del im["_first"], im["_alpha_first"]
            shape = (im["num_blocks_y"], im["num_blocks_x"])
            im["endpoint_indices"], im["selector_indices"] = ep[a:a + n].reshape(shape), sel[a:a + n].reshape(shape)
            im["alpha_endpoint_indices"], im["alpha_selector_indices"] = (ep[b:b + n].reshape(shape), sel[b:b + n].reshape(shape)) if im["has_alpha"] else (None, None)
        return info
    finally:
        L.bu_etc1s_file_destroy(h)


def read_etc1s_file(data):
    """Parse an ETC1S .basis (cBASISTexFormatETC1S) or .ktx2 (BasisLZ supercompression, ETC1S data format descriptor) file, the two ETC1S containers this package
    writes: the dictionary read_uastc_file returns ("format": "ETC1S"; an image has "has_alpha" instead of "offset" / "length", because a slice is a bit stream and
    not an array of blocks) plus "has_alpha_slices", "num_endpoints", "num_selectors", "tex_type" and "srgb". Host only. UASTC, video, truncated or corrupt files
    raise ValueError with the reason."""
    return _decode_etc1s(data, True)


def decode_etc1s_file(data):
    """read_etc1s_file plus everything the slices code (host only, no GPU): "endpoint_palette" (n, 4) u8 -- r5, g5, b5, intensity table --, "selector_palette" (n,)
    u32 -- the selector of texel (x, y) at bits 2 * (y * 4 + x) --, and per image "endpoint_indices" / "selector_indices" (num_blocks_y, num_blocks_x) u16 and, for
    images with an alpha slice, "alpha_endpoint_indices" / "alpha_selector_indices" (else None). Every index is checked against its palette."""
    return _decode_etc1s(data, False)


def _check_etc1s_target(target):
    target = int(target)
    if target not in ETC1S_BYTES_PER_BLOCK and target not in ETC1S_BYTES_PER_PIXEL:
        name = _TARGET_NAMES[target] if 0 <= target < len(_TARGET_NAMES) else "unknown"
        raise ValueError(f"ETC1S transcode target {target} ({name}) is not supported (supported: {sorted(list(ETC1S_BYTES_PER_BLOCK) + list(ETC1S_BYTES_PER_PIXEL))})")
    return target


def transcode_etc1s_image(ctx, decoded, image, target, *, out_device=None, out_row_pitch=0, out_rows=0):
    """One image of decode_etc1s_file's result on the GPU. Block targets (ETC1S_BYTES_PER_BLOCK) return (num_blocks, 8) u8, pixel targets (ETC1S_BYTES_PER_PIXEL)
    the (height, width, 4) u8 raster for RGBA32 and the (height, width) u16 raster for the 16-bit formats; with out_device (room for out_rows x out_row_pitch
    pixels when those are given) the output stays there and None is returned."""
    return _transcode_etc1s_image(ctx, decoded, image, _check_etc1s_target(target), None, out_device, out_row_pitch, out_rows)


def _transcode_etc1s_image(ctx, decoded, image, target, decode_flags, out_device, out_row_pitch, out_rows, block_format=False, vendor_format=False):
    """transcode_etc1s_image (decode_flags None: bu_hip_k_transcode_etc1s_counted), transcode_etc1s_texture_image (bu_hip_k_transcode_etc1s_image_counted),
    transcode_etc1s_block_format_image (block_format: bu_hip_k_transcode_etc1s_block_format_counted) and transcode_etc1s_vendor_format_image (vendor_format:
    bu_hip_k_transcode_etc1s_vendor_format_counted)"""
    texture = decode_flags is not None
    nbx, nby, w, h = image["num_blocks_x"], image["num_blocks_y"], image["width"], image["height"]
    ep_pal = np.ascontiguousarray(decoded["endpoint_palette"], np.uint8).reshape(-1, 4)
    sel_pal = np.ascontiguousarray(decoded["selector_palette"], np.uint32).reshape(-1)
    with_alpha = image["alpha_endpoint_indices"] is not None and target in (RGBA32, RGBA4444, ETC2_RGBA, BC7_RGBA, ASTC_4x4_RGBA, ETC2_EAC_RG11, PVRTC2_4_RGBA)
    names = ["endpoint_indices", "selector_indices"] + (["alpha_endpoint_indices", "alpha_selector_indices"] if with_alpha else [])
    if vendor_format:
        output_bytes = ctx.lib.etc1s_vendor_format_output_bytes
    elif block_format:
        output_bytes = ctx.lib.etc1s_block_format_output_bytes
    else:
        output_bytes = ctx.lib.etc1s_image_output_bytes if texture else ctx.lib.etc1s_transcode_output_bytes
    held = []
    with _output(ctx, out_device, out_row_pitch, out_rows, lambda: output_bytes(nbx, nby, w, h, target, 0, 0)) as d_out:
        try:
            for a in [ep_pal, sel_pal] + [np.ascontiguousarray(image[k], np.uint16).reshape(-1) for k in names]:
                held.append(ctx.upload(a))
            d_alpha = (held[4], held[5]) if with_alpha else (None, None)
            invalid = C.c_uint32(0)
            args = (ctx.h, C.c_void_p(held[0]), ep_pal.shape[0], C.c_void_p(held[1]), sel_pal.size, C.c_void_p(held[2]), C.c_void_p(held[3]), C.c_void_p(d_alpha[0]),
                    C.c_void_p(d_alpha[1]), nbx, nby, w, h, target, C.c_void_p(d_out), int(out_row_pitch), int(out_rows))
            if vendor_format:
                ctx.check(ctx.lib.k_transcode_etc1s_vendor_format_counted(*args, int(decode_flags), C.byref(invalid)), "transcode_etc1s_vendor_format")
            elif block_format:
                ctx.check(ctx.lib.k_transcode_etc1s_block_format_counted(*args, int(decode_flags), C.byref(invalid)), "transcode_etc1s_block_format")
            elif texture:
                ctx.check(ctx.lib.k_transcode_etc1s_image_counted(*args, int(decode_flags), C.byref(invalid)), "transcode_etc1s_image")
            else:
                ctx.check(ctx.lib.k_transcode_etc1s_counted(*args, C.byref(invalid)), "transcode_etc1s")
            if invalid.value:
                raise ValueError(f"{invalid.value} of {nbx * nby} blocks have an index past its palette")
            if out_device is not None:
                return None
            if target in ETC1S_VENDOR_FORMAT_BYTES_PER_BLOCK:
                blocks = (nbx + 1) // 2 * nby if target == FXT1_RGB else nbx * nby
                return ctx.download(d_out, (blocks, ETC1S_VENDOR_FORMAT_BYTES_PER_BLOCK[target]), np.uint8)
            return ctx.download(d_out, (h, w, 4), np.uint8) if target == RGBA32 else ctx.download(d_out, (h, w), np.uint16)
        finally:
            for p in held:
                ctx.free(p)


def transcode_etc1s_file(ctx, data, target, *, level=0, layer=0, face=0):
    """One image of an ETC1S .basis / .ktx2 file: decoded on the host (decode_etc1s_file), transcoded on the GPU (transcode_etc1s_image)."""
    target = _check_etc1s_target(target)
    decoded = decode_etc1s_file(data)
    for im in decoded["images"]:
        if (im["level"], im["layer"], im["face"]) == (level, layer, face):
            return transcode_etc1s_image(ctx, decoded, im, target)
    raise ValueError(f"the file has no image at level {level}, layer {layer}, face {face}")


# ---------------------------------------------------------------- the ETC1S texture family: also ETC2 RGBA and BC7 RGBA

def _check_etc1s_texture_target(target):
    target = int(target)
    if target not in ETC1S_TEXTURE_BYTES_PER_BLOCK and target not in ETC1S_BYTES_PER_PIXEL:
        name = _TARGET_NAMES[target] if 0 <= target < len(_TARGET_NAMES) else "unknown"
        raise ValueError(f"ETC1S texture target {target} ({name}) is not supported (supported: {sorted(list(ETC1S_TEXTURE_BYTES_PER_BLOCK) + list(ETC1S_BYTES_PER_PIXEL))})")
    return target


def etc1s_decode_flags(*, chroma_filtering=True, decode_flags=None):
    """the decode_flags word of the ETC1S texture entries: 64 (no chroma filtering) is the only bit there is; an explicit decode_flags with any other bit raises"""
    flags = (0 if chroma_filtering else DECODE_FLAGS_NO_ETC1S_CHROMA_FILTERING) if decode_flags is None else int(decode_flags)
    if flags & ~DECODE_FLAGS_NO_ETC1S_CHROMA_FILTERING:
        raise ValueError(f"ETC1S decode flags 0x{flags:x}: bits 0x{flags & ~DECODE_FLAGS_NO_ETC1S_CHROMA_FILTERING:x} are not supported (supported: 64, "
                         "cDecodeFlagsNoETC1SChromaFiltering)")
    return flags


def transcode_etc1s_texture_image(ctx, decoded, image, target, *, chroma_filtering=True, out_device=None, out_row_pitch=0, out_rows=0):
    """transcode_etc1s_image over the texture family's targets: the six of transcode_etc1s_image, byte for byte the same, plus ETC2_RGBA -- the EAC A8 block of the
    alpha slice, then the ETC1 block of the colour slice -- and BC7_RGBA -- one mode-5 block, by default behind the reference's chroma filter (chroma_filtering=False
    is its -no_etc1s_chroma_filtering). Block targets return (num_blocks, 8 | 16) u8; an image without an alpha slice gets the opaque alpha half."""
    return _transcode_etc1s_image(ctx, decoded, image, _check_etc1s_texture_target(target), etc1s_decode_flags(chroma_filtering=chroma_filtering), out_device, out_row_pitch, out_rows)


def transcode_etc1s_texture(ctx, data, target, *, level=0, layer=0, face=0, chroma_filtering=True):
    """One image of an ETC1S .basis / .ktx2 file as a texture of the family's targets (transcode_etc1s_texture_image): decoded on the host, transcoded on the GPU."""
    target, flags = _check_etc1s_texture_target(target), etc1s_decode_flags(chroma_filtering=chroma_filtering)
    decoded = decode_etc1s_file(data)
    for im in decoded["images"]:
        if (im["level"], im["layer"], im["face"]) == (level, layer, face):
            return _transcode_etc1s_image(ctx, decoded, im, target, flags, None, 0, 0)
    raise ValueError(f"the file has no image at level {level}, layer {layer}, face {face}")


def bc7_mode5_tiles(ctx, tiles):
    """A diagnostic (bu_hip_k_bc7_mode5_tiles): the mode-5 encoder that runs under BC7's chroma filter, on (n, 16, 4) u8 RGBA tiles (pixel y * 4 + x, alpha ignored)
    -> (n, 16) u8 opaque blocks."""
    tiles = np.ascontiguousarray(tiles, np.uint8)
    if tiles.ndim != 3 or tiles.shape[1:] != (16, 4):
        raise ValueError(f"bc7_mode5_tiles wants (n, 16, 4) u8 tiles, not {tiles.shape}")
    n = tiles.shape[0]
    if n == 0:
        return np.zeros((0, 16), np.uint8)
    d_tiles, d_out = ctx.upload(tiles), ctx.alloc(n * 16)
    try:
        ctx.check(ctx.lib.k_bc7_mode5_tiles(ctx.h, C.c_void_p(d_tiles), n, C.c_void_p(d_out)), "bc7_mode5_tiles")
        return ctx.download(d_out, (n, 16), np.uint8)
    finally:
        ctx.free(d_tiles)
        ctx.free(d_out)


# ---------------------------------------------------------------- the ETC1S block-format family: also ASTC 4x4, EAC R11 and EAC RG11

def _check_etc1s_block_format_target(target):
    target = int(target)
    if target not in ETC1S_BLOCK_FORMAT_BYTES_PER_BLOCK and target not in ETC1S_BYTES_PER_PIXEL:
        name = _TARGET_NAMES[target] if 0 <= target < len(_TARGET_NAMES) else "unknown"
        raise ValueError(f"ETC1S block-format target {target} ({name}) is not supported (supported: "
                         f"{sorted(list(ETC1S_BLOCK_FORMAT_BYTES_PER_BLOCK) + list(ETC1S_BYTES_PER_PIXEL))})")
    return target


def transcode_etc1s_block_format_image(ctx, decoded, image, target, *, chroma_filtering=True, out_device=None, out_row_pitch=0, out_rows=0):
    """transcode_etc1s_texture_image over the block-format family's targets: the eight of the texture family, byte for byte the same, plus ASTC_4x4_RGBA (one block of
    whichever ASTC mode the reference picks for the ETC1S block: void extent, block truncation, luminance + alpha, RGB, or RGBA over endpoints of range 0..47),
    ETC2_EAC_R11 (the EAC block of the colour slice's first channel) and ETC2_EAC_RG11 (that block, then the alpha slice's). Block targets return (num_blocks, 8 | 16)
    u8; an image without an alpha slice gets alpha 255 / the opaque second half. chroma_filtering matters to BC7_RGBA alone."""
    return _transcode_etc1s_image(ctx, decoded, image, _check_etc1s_block_format_target(target), etc1s_decode_flags(chroma_filtering=chroma_filtering), out_device, out_row_pitch,
                                  out_rows, True)


def transcode_etc1s_block_format(ctx, data, target, *, level=0, layer=0, face=0, chroma_filtering=True):
    """One image of an ETC1S .basis / .ktx2 file as a texture of the block-format family's targets (transcode_etc1s_block_format_image)."""
    target, flags = _check_etc1s_block_format_target(target), etc1s_decode_flags(chroma_filtering=chroma_filtering)
    decoded = decode_etc1s_file(data)
    for im in decoded["images"]:
        if (im["level"], im["layer"], im["face"]) == (level, layer, face):
            return _transcode_etc1s_image(ctx, decoded, im, target, flags, None, 0, 0, True)
    raise ValueError(f"the file has no image at level {level}, layer {layer}, face {face}")


# ---------------------------------------------------------------- the ETC1S vendor-format family: also ATC RGB, FXT1 and PVRTC2 4bpp RGB / RGBA

_VENDOR_FORMAT_REFUSALS = {3: "it needs the ETC1S -> BC4 look-up, which could not be restated as a search", 12: "its first half is a BC4 block, and the ETC1S -> BC4 look-up could not be "
                           "restated as a search"}
_VENDOR_FORMAT_REFUSALS[4] = _VENDOR_FORMAT_REFUSALS[5] = _VENDOR_FORMAT_REFUSALS[3]


def _check_etc1s_vendor_format_target(target):
    target = int(target)
    if target not in ETC1S_VENDOR_FORMAT_BYTES_PER_BLOCK and target not in ETC1S_BYTES_PER_PIXEL:
        name = _TARGET_NAMES[target] if 0 <= target < len(_TARGET_NAMES) else "unknown"
        why = f": {_VENDOR_FORMAT_REFUSALS[target]}" if target in _VENDOR_FORMAT_REFUSALS else ""
        raise ValueError(f"ETC1S vendor-format target {target} ({name}) is not supported{why} (supported: "
                         f"{sorted(list(ETC1S_VENDOR_FORMAT_BYTES_PER_BLOCK) + list(ETC1S_BYTES_PER_PIXEL))})")
    return target


def transcode_etc1s_vendor_format_image(ctx, decoded, image, target, *, chroma_filtering=True, out_device=None, out_row_pitch=0, out_rows=0):
    """transcode_etc1s_block_format_image over the vendor-format family's targets: the eleven of the block-format family, byte for byte the same, plus ATC_RGB (low colour
    555, high colour 565, 2-bit selectors), PVRTC2_4_RGB (hard opaque blocks: low colour 554, high colour 555) and FXT1_RGB (CC_MIXED blocks of 8x4 texels, each made of
    two source blocks by way of BC1 without three-colour blocks). Block targets return (blocks, 8 | 16) u8 in raster block order; for FXT1 blocks = ceil(num_blocks_x /
    2) * num_blocks_y, and the lone left half at the end of an odd row fills its block alone. None of the three reads the alpha slice. PVRTC2_4_RGBA re-encodes each block per pixel from
    the colour and the alpha slice (hard translucent blocks, colours 4433 / 4443; a constant alpha of 250 or more, or an image without an alpha slice, gives the RGB block)."""
    return _transcode_etc1s_image(ctx, decoded, image, _check_etc1s_vendor_format_target(target), etc1s_decode_flags(chroma_filtering=chroma_filtering), out_device, out_row_pitch,
                                  out_rows, vendor_format=True)


def transcode_etc1s_vendor_format(ctx, data, target, *, level=0, layer=0, face=0, chroma_filtering=True):
    """One image of an ETC1S .basis / .ktx2 file as a texture of the vendor-format family's targets (transcode_etc1s_vendor_format_image)."""
    target, flags = _check_etc1s_vendor_format_target(target), etc1s_decode_flags(chroma_filtering=chroma_filtering)
    decoded = decode_etc1s_file(data)
    for im in decoded["images"]:
        if (im["level"], im["layer"], im["face"]) == (level, layer, face):
            return _transcode_etc1s_image(ctx, decoded, im, target, flags, None, 0, 0, vendor_format=True)
    raise ValueError(f"the file has no image at level {level}, layer {layer}, face {face}")


# ---------------------------------------------------------------- every image of a file in one launch

NO_ALPHA_SLICE = 2 ** 64 - 1   # BU_HIP_NO_ALPHA_SLICE


class TranscodeSlice(C.Structure):   # = bu_hip_transcode_slice, include/basisu_hip.h
    _fields_ = [("first_block", C.c_uint64), ("alpha_first_block", C.c_uint64), ("out_offset", C.c_uint64)] + \
               [(n, C.c_uint32) for n in ("num_blocks_x", "num_blocks_y", "orig_width", "orig_height", "out_row_pitch_pixels", "out_rows_pixels")]


def etc1s_texture_layout(images, target):
    """image_layout for the ETC1S texture family (transcode_etc1s_textures): block targets are (blocks, 8 | 16) u8 by ETC1S_TEXTURE_BYTES_PER_BLOCK. Host only."""
    return _layout(images, _check_etc1s_texture_target(target), ETC1S_TEXTURE_BYTES_PER_BLOCK, True)


def etc1s_block_format_layout(images, target):
    """image_layout for the ETC1S block-format family (transcode_etc1s_block_formats): block targets are (blocks, 8 | 16) u8 by ETC1S_BLOCK_FORMAT_BYTES_PER_BLOCK; for
    the texture family's targets it is etc1s_texture_layout. Host only."""
    return _layout(images, _check_etc1s_block_format_target(target), ETC1S_BLOCK_FORMAT_BYTES_PER_BLOCK, True)


def etc1s_vendor_format_layout(images, target):
    """image_layout for the ETC1S vendor-format family (transcode_etc1s_vendor_formats): block targets are (blocks, 8 | 16) u8 by ETC1S_VENDOR_FORMAT_BYTES_PER_BLOCK,
    FXT1 with ceil(num_blocks_x / 2) * num_blocks_y blocks per image; for the block-format family's targets it is etc1s_block_format_layout. Host only."""
    return _layout(images, _check_etc1s_vendor_format_target(target), ETC1S_VENDOR_FORMAT_BYTES_PER_BLOCK, True)


def image_layout(images, target, *, etc1s):
    """Where the whole-file calls put each image of a file: `images` is the "images" list of read_uastc_file (etc1s=False) or of read_etc1s_file / decode_etc1s_file
    (etc1s=True). -> ([{"offset", "nbytes", "shape", "dtype"} per image, in the list's order], total_bytes): the images packed in order, each rounded up to 16
    bytes. A block target is (blocks, bytes per block) u8; a pixel target the tight raster of the image's own size, (height, width, 4) u8 for RGBA32 and
    (height, width) u16 for ETC1S' 16-bit formats. Host only."""
    target = _check_etc1s_target(target) if etc1s else _check_uastc_target(target)
    return _layout(images, target, ETC1S_BYTES_PER_BLOCK if etc1s else BYTES_PER_BLOCK, etc1s)


def _layout(images, target, bytes_per_block, etc1s):
    layout, at = [], 0
    for im in images:
        n, w, h = im["num_blocks_x"] * im["num_blocks_y"], im["width"], im["height"]
        if etc1s and target in ETC1S_BYTES_PER_PIXEL:
            shape, dtype = ((h, w, 4), np.uint8) if target == RGBA32 else ((h, w), np.uint16)
            nbytes = w * h * ETC1S_BYTES_PER_PIXEL[target]
        elif not etc1s and target == RGBA32:
            shape, dtype, nbytes = (h, w, 4), np.uint8, w * h * 4
        else:
            unit = bytes_per_block[target]
            if etc1s and target == FXT1_RGB:   # a block is two source blocks side by side
                n = (im["num_blocks_x"] + 1) // 2 * im["num_blocks_y"]
            shape, dtype, nbytes = (n, unit), np.uint8, n * unit
        layout.append({"offset": at, "nbytes": nbytes, "shape": shape, "dtype": dtype})
        at += (nbytes + 15) & ~15
    return layout, at


def _slice_table(images, layout, firsts, alpha_firsts=None):
    """the records of one call: image k reads from firsts[k] (alpha_firsts[k], None = no alpha slice) and writes its tight output at layout[k]["offset"]"""
    recs = (TranscodeSlice * len(images))()
    for k, im in enumerate(images):
        alpha = NO_ALPHA_SLICE if alpha_firsts is None or alpha_firsts[k] is None else int(alpha_firsts[k])
        recs[k] = TranscodeSlice(int(firsts[k]), alpha, layout[k]["offset"], im["num_blocks_x"], im["num_blocks_y"], im["width"], im["height"], 0, 0)
    return recs


def _upload_async(ctx, arr):
    """a buffer of our own holding `arr`, the copy ordered on the context's stream: nobody waits for it"""
    p = ctx.alloc(max(arr.nbytes, 1))
    try:
        if arr.nbytes:
            ctx.memcpy_h2d_async(p, np.ascontiguousarray(arr))
    except Exception:
        ctx.free(p)
        raise
    return p


def _run_slices(ctx, call, images, layout, total, out_device, what):
    """the half both whole-file calls share: the output (ours or the caller's), the one call, the per-slice counts, one download"""
    with _output(ctx, out_device, 0, 0, lambda: total) as d_out:
        invalid = (C.c_uint32 * len(images))()
        call(C.c_void_p(d_out), total, invalid)
        if any(invalid):
            raise InvalidBlocksError(sum(invalid), sum(im["num_blocks_x"] * im["num_blocks_y"] for im in images), what, per_slice=list(invalid))
        if out_device is not None:
            return layout, total
        raw = ctx.download(d_out, (total,), np.uint8)
        return [raw[e["offset"]:e["offset"] + e["nbytes"]].view(e["dtype"]).reshape(e["shape"]) for e in layout]


def _uastc_block_span(raw, images):
    """The blocks of a UASTC file's images as ONE host array for one upload -> (u8 array, [each image's first block in it]). Both containers write the images back to
    back, so this is normally the file's own bytes from the first image's to the last one's, not a copy (the table takes inputs in any order; only the device
    buffer needs the 16-byte alignment that a .basis payload does not have in the file). Where an image does not lie a multiple of 16 bytes from the first, or the
    span holds more than twice the images' bytes, the blocks are gathered in image order instead."""
    lo, hi = min(im["offset"] for im in images), max(im["offset"] + im["length"] for im in images)
    if all((im["offset"] - lo) % 16 == 0 for im in images) and hi - lo <= 2 * sum(im["length"] for im in images):
        return np.frombuffer(raw, np.uint8, hi - lo, lo), [(im["offset"] - lo) // 16 for im in images]
    firsts = np.concatenate([[0], np.cumsum([im["length"] // 16 for im in images])])
    return np.concatenate([np.frombuffer(raw, np.uint8, im["length"], im["offset"]) for im in images]), [int(f) for f in firsts[:-1]]


def transcode_file_images(ctx, data, target, *, high_quality=False, channels=None, out_device=None):
    """EVERY image of a UASTC .basis / .ktx2 file (read_uastc_file) transcoded by one launch (bu_hip_k_transcode_uastc_slices): the images' blocks go up
    as one array in one upload (_uastc_block_span: the file's own span of them, or a gather), and one call writes them all. Returns a list of arrays,
    one per image in the order of read_uastc_file's "images", each what transcode_file returns for it (views of one download). With out_device (a device pointer
    with room for image_layout's total_bytes) the output stays there and image_layout(images, target, etc1s=False) is returned. Raises InvalidBlocksError, with
    the per-slice counts and the lowest slice that has any, when a block does not unpack."""
    raw = data.tobytes() if isinstance(data, np.ndarray) else bytes(data)
    images = read_uastc_file(raw)["images"]
    layout, total = image_layout(images, target, etc1s=False)
    target, (c0, c1) = int(target), _channel_pair(channels)
    blocks, firsts = _uastc_block_span(raw, images)
    recs = _slice_table(images, layout, firsts)
    d_blocks = _upload_async(ctx, blocks)
    try:
        def call(d_out, out_bytes, invalid):
            ctx.check(ctx.lib.k_transcode_uastc_slices(ctx.h, C.c_void_p(d_blocks), blocks.size // 16, recs, len(images), target, DECODE_FLAGS_HIGH_QUALITY if high_quality else 0,
                                                       c0, c1, d_out, out_bytes, invalid), "transcode_uastc_slices")
        return _run_slices(ctx, call, images, layout, total, out_device, "UASTC LDR 4x4")
    finally:
        ctx.free(d_blocks)


# ---------------------------------------------------------------- the UASTC texture family: also ETC1, ETC2 RGBA, EAC R11 / RG11 and the 16-bit rasters

ETC2_EAC_R11, ETC2_EAC_RG11 = 20, 21
UASTC_TEXTURE_BYTES_PER_BLOCK = {ETC1_RGB: 8, ETC2_RGBA: 16, BC1_RGB: 8, BC3_RGBA: 16, BC4_R: 8, BC5_RG: 16, BC7_RGBA: 16, ASTC_4x4_RGBA: 16, ETC2_EAC_R11: 8, ETC2_EAC_RG11: 16}
UASTC_TEXTURE_BYTES_PER_PIXEL = {RGBA32: 4, RGB565: 2, BGR565: 2, RGBA4444: 2}


def _check_uastc_texture_target(target):
    target = int(target)
    if target not in UASTC_TEXTURE_BYTES_PER_BLOCK and target not in UASTC_TEXTURE_BYTES_PER_PIXEL:
        name = _TARGET_NAMES[target] if 0 <= target < len(_TARGET_NAMES) else "unknown"
        raise ValueError(f"UASTC texture target {target} ({name}) is not supported (supported: {sorted(list(UASTC_TEXTURE_BYTES_PER_BLOCK) + list(UASTC_TEXTURE_BYTES_PER_PIXEL))})")
    return target


def uastc_decode_flags(*, high_quality=False, decode_flags=None):
    """the decode_flags word of the UASTC texture entries: 32 (high quality) is the only bit there is; an explicit decode_flags with any other bit raises -- bit 4,
    cDecodeFlagsTranscodeAlphaDataToOpaqueFormats (ETC1 from the alpha channel), among them"""
    flags = (DECODE_FLAGS_HIGH_QUALITY if high_quality else 0) if decode_flags is None else int(decode_flags)
    if flags & ~DECODE_FLAGS_HIGH_QUALITY:
        raise ValueError(f"UASTC decode flags 0x{flags:x}: bits 0x{flags & ~DECODE_FLAGS_HIGH_QUALITY:x} are not supported (supported: 32, cDecodeFlagsHighQuality)")
    return flags


def _texture_array(ctx, d_out, target, n, width, height):
    """the download of one image's output as the texture family returns it"""
    if target in UASTC_TEXTURE_BYTES_PER_BLOCK:
        unit = UASTC_TEXTURE_BYTES_PER_BLOCK[target]
        return ctx.download(d_out, (n, unit), np.uint8) if n else np.zeros((0, unit), np.uint8)
    if target == RGBA32:
        return ctx.download(d_out, (height, width, 4), np.uint8) if n else np.zeros((0, 0, 4), np.uint8)
    return ctx.download(d_out, (height, width), np.uint16) if n else np.zeros((0, 0), np.uint16)


def transcode_uastc_texture_blocks(ctx, blocks, nbx, nby, target, *, width=None, height=None, high_quality=False, decode_flags=None, channels=None, out_device=None,
                                   out_row_pitch=0, out_rows=0):
    """transcode_uastc_blocks over the texture family's targets (bu_hip_k_transcode_uastc_texture): the seven of transcode_uastc_blocks, byte for byte the same, plus
    ETC1_RGB, ETC2_RGBA (the EAC A8 block, then the ETC1 block), ETC2_EAC_R11 / ETC2_EAC_RG11 (channels: (c,) / (c0, c1), default (0,) / (0, 3); high_quality
    selects the 16-table packer) and RGB565 / BGR565 / RGBA4444. Block targets return (nby * nbx, 8 | 16) uint8; pixel targets the cropped raster, (height, width, 4)
    uint8 for RGBA32 and (height, width) uint16 for the 16-bit formats. With out_device (room for bu_hip_uastc_texture_output_bytes; out_row_pitch / out_rows, in
    pixels, for a pixel target's padded raster) the output stays on the device and None is returned. Raises InvalidBlocksError when a block does not unpack."""
    nbx, nby, target = int(nbx), int(nby), _check_uastc_texture_target(target)
    flags = uastc_decode_flags(high_quality=high_quality, decode_flags=decode_flags)
    c0, c1 = _channel_pair(channels)
    n = nbx * nby
    width, height = int(width or nbx * 4), int(height or nby * 4)
    if not (0 < width <= nbx * 4 and 0 < height <= nby * 4) and n:
        raise ValueError(f"{width} x {height} pixels do not fit {nbx} x {nby} blocks")
    if target in UASTC_TEXTURE_BYTES_PER_BLOCK and (out_row_pitch or out_rows):
        raise ValueError("out_row_pitch / out_rows describe a pixel raster: the target is a block format")
    own = None
    try:
        if isinstance(blocks, np.ndarray):
            blocks = np.ascontiguousarray(blocks, np.uint8)
            if blocks.size != n * 16:
                raise ValueError(f"{nbx} x {nby} blocks need {n * 16} bytes, got {blocks.size}")
            blocks = own = ctx.upload(blocks) if n else 0
        with _output(ctx, out_device, out_row_pitch, out_rows, lambda: ctx.lib.uastc_texture_output_bytes(nbx, nby, width, height, target, 0, 0)) as d_out:
            invalid = C.c_uint32(0)
            if n:
                ctx.check(ctx.lib.k_transcode_uastc_texture(ctx.h, C.c_void_p(blocks), nbx, nby, width, height, target, flags, c0, c1, C.c_void_p(d_out), int(out_row_pitch),
                                                            int(out_rows), C.byref(invalid)), "transcode_uastc_texture")
            if invalid.value:
                raise InvalidBlocksError(invalid.value, n)
            return None if out_device is not None else _texture_array(ctx, d_out, target, n, width, height)
    finally:
        if own:
            ctx.free(own)


def transcode_uastc_texture_file(ctx, data, target, *, level=0, layer=0, face=0, high_quality=False, decode_flags=None, channels=None):
    """One image of a UASTC .basis / .ktx2 file (read_uastc_file) as a texture of the family's targets: what transcode_uastc_texture_blocks returns for its blocks."""
    target, flags = _check_uastc_texture_target(target), uastc_decode_flags(high_quality=high_quality, decode_flags=decode_flags)
    _channel_pair(channels)
    raw = data.tobytes() if isinstance(data, np.ndarray) else bytes(data)
    for im in read_uastc_file(raw)["images"]:
        if (im["level"], im["layer"], im["face"]) == (level, layer, face):
            blocks = np.frombuffer(raw, np.uint8, im["length"], im["offset"]).reshape(-1, 16)
            return transcode_uastc_texture_blocks(ctx, blocks, im["num_blocks_x"], im["num_blocks_y"], target, width=im["width"], height=im["height"], decode_flags=flags,
                                                  channels=channels)
    raise ValueError(f"the file has no image at level {level}, layer {layer}, face {face}")


def uastc_texture_layout(images, target):
    """image_layout for the UASTC texture family (transcode_uastc_textures): block targets are (blocks, 8 | 16) u8 by UASTC_TEXTURE_BYTES_PER_BLOCK, pixel targets the
    tight raster, (height, width, 4) u8 for RGBA32 and (height, width) u16 for the 16-bit formats. Host only."""
    target = _check_uastc_texture_target(target)
    layout, at = [], 0
    for im in images:
        n, w, h = im["num_blocks_x"] * im["num_blocks_y"], im["width"], im["height"]
        if target in UASTC_TEXTURE_BYTES_PER_PIXEL:
            shape, dtype = ((h, w, 4), np.uint8) if target == RGBA32 else ((h, w), np.uint16)
            nbytes = w * h * UASTC_TEXTURE_BYTES_PER_PIXEL[target]
        else:
            unit = UASTC_TEXTURE_BYTES_PER_BLOCK[target]
            shape, dtype, nbytes = (n, unit), np.uint8, n * unit
        layout.append({"offset": at, "nbytes": nbytes, "shape": shape, "dtype": dtype})
        at += (nbytes + 15) & ~15
    return layout, at


def transcode_uastc_textures(ctx, data, target, *, high_quality=False, decode_flags=None, channels=None, out_device=None):
    """transcode_file_images over the texture family's targets (bu_hip_k_transcode_uastc_textures): EVERY image of a UASTC .basis / .ktx2 file by one launch, each
    what transcode_uastc_texture_file returns for it (views of one download). With out_device (a device pointer with room for uastc_texture_layout's total_bytes) the
    output -- an ETC1 / ETC2 texture for a client that samples those, say -- stays there and uastc_texture_layout(images, target) is returned. Raises
    InvalidBlocksError, with the per-slice counts and the lowest slice that has any, when a block does not unpack."""
    target, flags = _check_uastc_texture_target(target), uastc_decode_flags(high_quality=high_quality, decode_flags=decode_flags)
    c0, c1 = _channel_pair(channels)
    raw = data.tobytes() if isinstance(data, np.ndarray) else bytes(data)
    images = read_uastc_file(raw)["images"]
    layout, total = uastc_texture_layout(images, target)
    blocks, firsts = _uastc_block_span(raw, images)
    recs = _slice_table(images, layout, firsts)
    d_blocks = _upload_async(ctx, blocks)
    try:
        def call(d_out, out_bytes, invalid):
            ctx.check(ctx.lib.k_transcode_uastc_textures(ctx.h, C.c_void_p(d_blocks), blocks.size // 16, recs, len(images), target, flags, c0, c1, d_out, out_bytes, invalid),
                      "transcode_uastc_textures")
        return _run_slices(ctx, call, images, layout, total, out_device, "UASTC LDR 4x4")
    finally:
        ctx.free(d_blocks)


def transcode_etc1s_file_images(ctx, data, target, *, out_device=None):
    """EVERY image of an ETC1S .basis / .ktx2 file transcoded by one launch (bu_hip_k_transcode_etc1s_slices): one host decode, both palettes and the file's two
    whole index arrays uploaded once, one call; an image's alpha slice is a second range of the same arrays. Returns a list of arrays, one per image in the order
    of read_etc1s_file's "images", each what transcode_etc1s_file returns for it (views of one download). With out_device (room for image_layout's total_bytes)
    the output stays there and image_layout(images, target, etc1s=True) is returned. Raises InvalidBlocksError, with the per-slice counts and the lowest slice
    that has any, when a block has an index past its palette."""
    target = _check_etc1s_target(target)
    decoded = _decode_etc1s(data, False, whole=True)
    images = decoded["images"]
    return _transcode_etc1s_slices(ctx, decoded, images, [im["_first"] for im in images], [im["_alpha_first"] if im["has_alpha"] else None for im in images], target, out_device)


def transcode_etc1s_textures(ctx, data, target, *, chroma_filtering=True, out_device=None):
    """transcode_etc1s_file_images over the texture family's targets (bu_hip_k_transcode_etc1s_images): every image of the file in one launch, each what
    transcode_etc1s_texture returns for it. With out_device (room for etc1s_texture_layout's total_bytes) the output stays there -- a block target's part of it goes
    straight into unpack_blocks -- and etc1s_texture_layout(images, target) is returned."""
    target, flags = _check_etc1s_texture_target(target), etc1s_decode_flags(chroma_filtering=chroma_filtering)
    decoded = _decode_etc1s(data, False, whole=True)
    images = decoded["images"]
    return _transcode_etc1s_slices(ctx, decoded, images, [im["_first"] for im in images], [im["_alpha_first"] if im["has_alpha"] else None for im in images], target, out_device,
                                   flags)


def transcode_etc1s_block_formats(ctx, data, target, *, chroma_filtering=True, out_device=None):
    """transcode_etc1s_textures over the block-format family's targets (bu_hip_k_transcode_etc1s_block_formats): every image of the file in one launch, each what
    transcode_etc1s_block_format returns for it. With out_device (room for etc1s_block_format_layout's total_bytes) the output -- an ASTC texture for a client that
    samples it, say -- stays there and etc1s_block_format_layout(images, target) is returned."""
    target, flags = _check_etc1s_block_format_target(target), etc1s_decode_flags(chroma_filtering=chroma_filtering)
    decoded = _decode_etc1s(data, False, whole=True)
    images = decoded["images"]
    return _transcode_etc1s_slices(ctx, decoded, images, [im["_first"] for im in images], [im["_alpha_first"] if im["has_alpha"] else None for im in images], target, out_device,
                                   flags, True)


def transcode_etc1s_vendor_formats(ctx, data, target, *, chroma_filtering=True, out_device=None):
    """transcode_etc1s_block_formats over the vendor-format family's targets (bu_hip_k_transcode_etc1s_vendor_formats): every image of the file in one launch, each what
    transcode_etc1s_vendor_format returns for it. With out_device (room for etc1s_vendor_format_layout's total_bytes) the output stays there and
    etc1s_vendor_format_layout(images, target) is returned."""
    target, flags = _check_etc1s_vendor_format_target(target), etc1s_decode_flags(chroma_filtering=chroma_filtering)
    decoded = _decode_etc1s(data, False, whole=True)
    images = decoded["images"]
    return _transcode_etc1s_slices(ctx, decoded, images, [im["_first"] for im in images], [im["_alpha_first"] if im["has_alpha"] else None for im in images], target, out_device,
                                   flags, vendor_format=True)


def _transcode_etc1s_slices(ctx, decoded, images, firsts, alpha_firsts, target, out_device, decode_flags=None, block_format=False, vendor_format=False):
    """transcode_etc1s_file_images behind the decode (_decode_etc1s with whole=True): `images` (sizes) with where each one's indices begin in the file's whole
    arrays. stats.py decodes an alpha slice as a colour image of its own this way. decode_flags not None: the texture family's entry and layout, or with
    block_format the block-format family's, with vendor_format the vendor-format family's."""
    if vendor_format:
        layout, total = etc1s_vendor_format_layout(images, target)
    elif block_format:
        layout, total = etc1s_block_format_layout(images, target)
    else:
        layout, total = image_layout(images, target, etc1s=True) if decode_flags is None else etc1s_texture_layout(images, target)
    recs = _slice_table(images, layout, firsts, alpha_firsts)
    ep_pal = np.ascontiguousarray(decoded["endpoint_palette"], np.uint8).reshape(-1, 4)
    sel_pal = np.ascontiguousarray(decoded["selector_palette"], np.uint32).reshape(-1)
    ep_idx, sel_idx = decoded["_endpoint_indices"], decoded["_selector_indices"]
    held = []
    try:
        for a in (ep_pal, sel_pal, ep_idx, sel_idx):
            held.append(_upload_async(ctx, a))

        def call(d_out, out_bytes, invalid):
            head = (ctx.h, C.c_void_p(held[0]), ep_pal.shape[0], C.c_void_p(held[1]), sel_pal.size, C.c_void_p(held[2]), C.c_void_p(held[3]), ep_idx.size, recs, len(images), target)
            if vendor_format:
                ctx.check(ctx.lib.k_transcode_etc1s_vendor_formats(*head, int(decode_flags), d_out, out_bytes, invalid), "transcode_etc1s_vendor_formats")
            elif block_format:
                ctx.check(ctx.lib.k_transcode_etc1s_block_formats(*head, int(decode_flags), d_out, out_bytes, invalid), "transcode_etc1s_block_formats")
            elif decode_flags is None:
                ctx.check(ctx.lib.k_transcode_etc1s_slices(*head, d_out, out_bytes, invalid), "transcode_etc1s_slices")
            else:
                ctx.check(ctx.lib.k_transcode_etc1s_images(*head, int(decode_flags), d_out, out_bytes, invalid), "transcode_etc1s_images")
        return _run_slices(ctx, call, images, layout, total, out_device, "ETC1S")
    finally:
        for p in held:
            ctx.free(p)


# ---------------------------------------------------------------- PVRTC1 4bpp, both codecs: the target whose blocks depend on their neighbours

PVRTC1_4_RGB, PVRTC1_4_RGBA = 8, 9
PVRTC1_BYTES_PER_BLOCK = 8


def _check_pvrtc1_target(target):
    target = int(target)
    if target not in (PVRTC1_4_RGB, PVRTC1_4_RGBA):
        name = _TARGET_NAMES[target] if 0 <= target < len(_TARGET_NAMES) else "unknown"
        raise ValueError(f"PVRTC1 target {target} ({name}) is not supported (supported: [{PVRTC1_4_RGB}, {PVRTC1_4_RGBA}])")
    return target


def _check_pvrtc1_size(width, height, what):
    width, height = int(width), int(height)
    if width <= 0 or height <= 0 or width & (width - 1) or height & (height - 1):
        raise ValueError(f"{what}: {width} x {height} pixels: PVRTC1 only supports power of 2 dimensions")


def pvrtc1_layout(images):
    """Where transcode_pvrtc1_images puts each image: `images` is the "images" list of read_uastc_file or read_etc1s_file / decode_etc1s_file. -> ([{"offset",
    "nbytes", "shape", "dtype"} per image, in the list's order], total_bytes): (blocks, 8) u8 each, in PVRTC1's own (Morton) block order, each image rounded up to
    16 bytes; a level of 4x4 pixels or less is its one block, without the padding GL asks of levels under 8x8. An image that is not a power of two each way raises.
    Host only."""
    layout, at = [], 0
    for im in images:
        _check_pvrtc1_size(im["width"], im["height"], f"level {im['level']}, layer {im['layer']}, face {im['face']}")
        n = im["num_blocks_x"] * im["num_blocks_y"]
        layout.append({"offset": at, "nbytes": n * PVRTC1_BYTES_PER_BLOCK, "shape": (n, PVRTC1_BYTES_PER_BLOCK), "dtype": np.uint8})
        at += (n * PVRTC1_BYTES_PER_BLOCK + 15) & ~15
    return layout, at


def transcode_uastc_pvrtc1_blocks(ctx, blocks, nbx, nby, target, *, out_device=None):
    """UASTC blocks -> one PVRTC1 4bpp image (bu_hip_k_transcode_uastc_pvrtc1). blocks: (nby * nbx, 16) uint8 in raster order (uploaded once) or a device pointer to
    that many resident blocks; nbx and nby powers of two. PVRTC1_4_RGBA keeps the pixels' alpha, PVRTC1_4_RGB ignores it (whether a FILE has alpha is its header's
    word: transcode_uastc_pvrtc1_file reads it). Returns (nby * nbx, 8) uint8 in PVRTC1's own (Morton) block order, or None when out_device (room for
    nbx * nby * 8 bytes, 8-byte aligned) receives it. Raises InvalidBlocksError when a block does not unpack (its eight bytes are zero)."""
    nbx, nby, target = int(nbx), int(nby), _check_pvrtc1_target(target)
    _check_pvrtc1_size(nbx * 4, nby * 4, "transcode_uastc_pvrtc1_blocks")
    n = nbx * nby
    own = None
    try:
        if isinstance(blocks, np.ndarray):
            blocks = np.ascontiguousarray(blocks, np.uint8)
            if blocks.size != n * 16:
                raise ValueError(f"{nbx} x {nby} blocks need {n * 16} bytes, got {blocks.size}")
            blocks = own = ctx.upload(blocks)
        with _output(ctx, out_device, 0, 0, lambda: ctx.lib.pvrtc1_output_bytes(nbx, nby)) as d_out:
            invalid = C.c_uint32(0)
            ctx.check(ctx.lib.k_transcode_uastc_pvrtc1(ctx.h, C.c_void_p(blocks), nbx, nby, nbx * 4, nby * 4, target, 0, C.c_void_p(d_out), C.byref(invalid)),
                      "transcode_uastc_pvrtc1")
            if invalid.value:
                raise InvalidBlocksError(invalid.value, n)
            return None if out_device is not None else ctx.download(d_out, (n, PVRTC1_BYTES_PER_BLOCK), np.uint8)
    finally:
        if own:
            ctx.free(own)


def transcode_uastc_pvrtc1_file(ctx, data, target, *, level=0, layer=0, face=0):
    """One image of a UASTC .basis / .ktx2 file (read_uastc_file) as PVRTC1 4bpp: what transcode_uastc_pvrtc1_blocks returns for its blocks. PVRTC1_4_RGBA asked of a
    file whose header has no alpha flag is answered with the RGB route, as the reference does. A file whose level 0 is not a power of two each way raises before the
    device is touched."""
    target = _check_pvrtc1_target(target)
    raw = data.tobytes() if isinstance(data, np.ndarray) else bytes(data)
    info = read_uastc_file(raw)
    _check_pvrtc1_size(info["width"], info["height"], "transcode_uastc_pvrtc1_file")
    for im in info["images"]:
        if (im["level"], im["layer"], im["face"]) == (level, layer, face):
            blocks = np.frombuffer(raw, np.uint8, im["length"], im["offset"]).reshape(-1, 16)
            return transcode_uastc_pvrtc1_blocks(ctx, blocks, im["num_blocks_x"], im["num_blocks_y"], target if info["has_alpha"] else PVRTC1_4_RGB)
    raise ValueError(f"the file has no image at level {level}, layer {layer}, face {face}")


def transcode_etc1s_pvrtc1_image(ctx, decoded, image, target, *, out_device=None):
    """One image of decode_etc1s_file's result as PVRTC1 4bpp (bu_hip_k_transcode_etc1s_pvrtc1_counted): (num_blocks, 8) u8 in PVRTC1's own (Morton) block order, or
    None when out_device receives it. PVRTC1_4_RGBA takes alpha from the image's alpha slice; an image without one gets what PVRTC1_4_RGB writes."""
    target = _check_pvrtc1_target(target)
    nbx, nby, w, h = image["num_blocks_x"], image["num_blocks_y"], image["width"], image["height"]
    _check_pvrtc1_size(w, h, "transcode_etc1s_pvrtc1_image")
    ep_pal = np.ascontiguousarray(decoded["endpoint_palette"], np.uint8).reshape(-1, 4)
    sel_pal = np.ascontiguousarray(decoded["selector_palette"], np.uint32).reshape(-1)
    with_alpha = image["alpha_endpoint_indices"] is not None and target == PVRTC1_4_RGBA
    names = ["endpoint_indices", "selector_indices"] + (["alpha_endpoint_indices", "alpha_selector_indices"] if with_alpha else [])
    held = []
    with _output(ctx, out_device, 0, 0, lambda: ctx.lib.pvrtc1_output_bytes(nbx, nby)) as d_out:
        try:
            for a in [ep_pal, sel_pal] + [np.ascontiguousarray(image[k], np.uint16).reshape(-1) for k in names]:
                held.append(ctx.upload(a))
            d_alpha = (held[4], held[5]) if with_alpha else (None, None)
            invalid = C.c_uint32(0)
            ctx.check(ctx.lib.k_transcode_etc1s_pvrtc1_counted(ctx.h, C.c_void_p(held[0]), ep_pal.shape[0], C.c_void_p(held[1]), sel_pal.size, C.c_void_p(held[2]),
                                                               C.c_void_p(held[3]), C.c_void_p(d_alpha[0]), C.c_void_p(d_alpha[1]), nbx, nby, w, h, target, C.c_void_p(d_out), 0,
                                                               C.byref(invalid)), "transcode_etc1s_pvrtc1")
            if invalid.value:
                raise ValueError(f"{invalid.value} of {nbx * nby} blocks have an index past its palette")
            return None if out_device is not None else ctx.download(d_out, (nbx * nby, PVRTC1_BYTES_PER_BLOCK), np.uint8)
        finally:
            for p in held:
                ctx.free(p)


def transcode_etc1s_pvrtc1(ctx, data, target, *, level=0, layer=0, face=0):
    """One image of an ETC1S .basis / .ktx2 file as PVRTC1 4bpp (transcode_etc1s_pvrtc1_image): decoded on the host, transcoded on the GPU. A file whose level 0 is
    not a power of two each way raises before the device is touched."""
    target = _check_pvrtc1_target(target)
    info = read_etc1s_file(data)
    _check_pvrtc1_size(info["width"], info["height"], "transcode_etc1s_pvrtc1")
    decoded = decode_etc1s_file(data)
    for im in decoded["images"]:
        if (im["level"], im["layer"], im["face"]) == (level, layer, face):
            return transcode_etc1s_pvrtc1_image(ctx, decoded, im, target)
    raise ValueError(f"the file has no image at level {level}, layer {layer}, face {face}")


def _is_etc1s_file(raw):
    """which of the two readers a .basis / .ktx2 file is for: the KTX2 header's supercompression scheme (1 = BasisLZ), the .basis header's texture format byte"""
    if len(raw) >= 12 and raw[:12] == _KTX2_MAGIC:
        return len(raw) >= 48 and struct.unpack_from("<I", raw, 44)[0] == 1
    return len(raw) > 20 and raw[:2] == b"sB" and raw[20] == 0


def transcode_pvrtc1_images(ctx, data, target, *, out_device=None):
    """EVERY image of a UASTC or ETC1S .basis / .ktx2 file as PVRTC1 4bpp by two launches in all (bu_hip_k_transcode_uastc_pvrtc1_images /
    bu_hip_k_transcode_etc1s_pvrtc1_images): a list of arrays, one per image in the order of the reader's "images", each what the one-image call returns for it
    (views of one download). With out_device (room for pvrtc1_layout's total_bytes) the output stays there and pvrtc1_layout(images) is returned. PVRTC1_4_RGBA on
    a file without alpha is answered with the RGB route. A file whose level 0 is not a power of two raises before the device is touched (a power-of-two level 0
    gives a power-of-two chain). Raises InvalidBlocksError, with the per-slice counts, when a block is invalid."""
    target = _check_pvrtc1_target(target)
    raw = data.tobytes() if isinstance(data, np.ndarray) else bytes(data)
    if _is_etc1s_file(raw):
        info = read_etc1s_file(raw)
        _check_pvrtc1_size(info["width"], info["height"], "transcode_pvrtc1_images")
        decoded = _decode_etc1s(raw, False, whole=True)
        images = decoded["images"]
        layout, total = pvrtc1_layout(images)
        alpha = target == PVRTC1_4_RGBA and all(im["has_alpha"] for im in images)
        recs = _slice_table(images, layout, [im["_first"] for im in images], [im["_alpha_first"] if alpha else None for im in images])
        ep_pal = np.ascontiguousarray(decoded["endpoint_palette"], np.uint8).reshape(-1, 4)
        sel_pal = np.ascontiguousarray(decoded["selector_palette"], np.uint32).reshape(-1)
        ep_idx, sel_idx = decoded["_endpoint_indices"], decoded["_selector_indices"]
        held = []
        try:
            for a in (ep_pal, sel_pal, ep_idx, sel_idx):
                held.append(_upload_async(ctx, a))

            def call(d_out, out_bytes, invalid):
                ctx.check(ctx.lib.k_transcode_etc1s_pvrtc1_images(ctx.h, C.c_void_p(held[0]), ep_pal.shape[0], C.c_void_p(held[1]), sel_pal.size, C.c_void_p(held[2]),
                                                                  C.c_void_p(held[3]), ep_idx.size, recs, len(images), target, 0, d_out, out_bytes, invalid),
                          "transcode_etc1s_pvrtc1_images")
            return _run_slices(ctx, call, images, layout, total, out_device, "ETC1S")
        finally:
            for p in held:
                ctx.free(p)
    info = read_uastc_file(raw)
    _check_pvrtc1_size(info["width"], info["height"], "transcode_pvrtc1_images")
    images = info["images"]
    layout, total = pvrtc1_layout(images)
    blocks, firsts = _uastc_block_span(raw, images)
    recs = _slice_table(images, layout, firsts)
    d_blocks = _upload_async(ctx, blocks)
    try:
        def call(d_out, out_bytes, invalid):
            ctx.check(ctx.lib.k_transcode_uastc_pvrtc1_images(ctx.h, C.c_void_p(d_blocks), blocks.size // 16, recs, len(images), target if info["has_alpha"] else PVRTC1_4_RGB,
                                                              0, d_out, out_bytes, invalid), "transcode_uastc_pvrtc1_images")
        return _run_slices(ctx, call, images, layout, total, out_device, "UASTC LDR 4x4")
    finally:
        ctx.free(d_blocks)


# ---------------------------------------------------------------- every block format back to pixels

# the formats of unpack_texture: unpack_blocks' five, byte for byte, and every other block target the transcoders above write
UNPACK_TEXTURE_BYTES_PER_BLOCK = {**UNPACK_BYTES_PER_BLOCK, ETC1_RGB: 8, ETC2_RGBA: 16, PVRTC1_4_RGB: 8, PVRTC1_4_RGBA: 8, ASTC_4x4_RGBA: 16, ETC2_EAC_R11: 8, ETC2_EAC_RG11: 16}


def unpack_texture(ctx, blocks, nbx, nby, fmt, *, width=None, height=None, out_device=None, out_row_pitch=0, out_rows=0):
    """gpu_image::unpack on the GPU for every block format this module's transcoders write (fmt: the transcoder's target value, UNPACK_TEXTURE_BYTES_PER_BLOCK):
    what a GPU samples from the texture, RGBA8 (bu_hip_k_unpack_texture). The five BC formats decode as unpack_blocks decodes them; ETC1 with A = 255; ETC2 RGBA;
    EAC R11 / RG11 into R / R, G with the 11-bit value rounded to 8 bits (the rest (0, 0, 255)); ASTC 4x4, the whole LDR format in the L8 (non-sRGB) decode profile;
    PVRTC1 4bpp with the blocks in their own (Morton) order, as the PVRTC1 transcoders return them, power-of-two images only.
    blocks: (nby * nbx, 8 | 16) uint8 array (uploaded once) or a device pointer (int) to that many resident blocks. Returns the (height, width, 4) raster, or None
    when out_device (a device pointer with room for out_rows x out_row_pitch pixels, 0 = height / width) receives it; width / height default to the padded size.
    Invalid blocks -- BC7's reserved mode, an ETC1 / ETC2 colour half whose differential base overflows (ETC2's T / H / planar encodings), an ASTC block an LDR
    decoder refuses -- are zero-filled, and InvalidBlocksError is raised with their count. There is no CPU implementation."""
    nbx, nby, fmt = int(nbx), int(nby), int(fmt)
    if fmt not in UNPACK_TEXTURE_BYTES_PER_BLOCK:
        name = _TARGET_NAMES[fmt] if 0 <= fmt < len(_TARGET_NAMES) else "unknown"
        raise ValueError(f"texture format {fmt} ({name}) does not unpack here (supported: {sorted(UNPACK_TEXTURE_BYTES_PER_BLOCK)})")
    n, unit = nbx * nby, UNPACK_TEXTURE_BYTES_PER_BLOCK[fmt]
    width, height = int(width or nbx * 4), int(height or nby * 4)
    if not (0 < width <= nbx * 4 and 0 < height <= nby * 4) and n:
        raise ValueError(f"{width} x {height} pixels do not fit {nbx} x {nby} blocks")
    if fmt in (PVRTC1_4_RGB, PVRTC1_4_RGBA) and n:
        _check_pvrtc1_size(width, height, "unpack_texture")
        _check_pvrtc1_size(nbx * 4, nby * 4, "unpack_texture")
    with _output(ctx, out_device, out_row_pitch, out_rows, lambda: ctx.lib.unpack_output_bytes(nbx, nby, width, height, 0, 0)) as d_out:
        own = None
        try:
            if isinstance(blocks, np.ndarray):
                blocks = np.ascontiguousarray(blocks, np.uint8)
                if blocks.size != n * unit:
                    raise ValueError(f"{nbx} x {nby} blocks need {n * unit} bytes, got {blocks.size}")
                blocks = own = ctx.upload(blocks) if n else 0
            invalid = C.c_uint32(0)
            if n:
                ctx.check(ctx.lib.k_unpack_texture(ctx.h, C.c_void_p(blocks), nbx, nby, width, height, fmt, C.c_void_p(d_out), int(out_row_pitch), int(out_rows), C.byref(invalid)),
                          "unpack_texture")
            if invalid.value:
                raise InvalidBlocksError(invalid.value, n, _TARGET_NAMES[fmt])
            if out_device is not None:
                return None
            return ctx.download(d_out, (height, width, 4), np.uint8) if n else np.zeros((0, 0, 4), np.uint8)
        finally:
            if own:
                ctx.free(own)
