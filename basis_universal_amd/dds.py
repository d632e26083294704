"""Source images straight to a DX10 .dds texture -- what the reference tool's `-dds` mode does (dds_mode, basisu_tool.cpp:9243-9371; build_dds,
encoder/basisu_dds_export.cpp) -- with mips, arrays and cubemaps, BC1-BC5 or one of seven uncompressed formats, every stage on the device:

    raster in HBM -> source-image options -> mip levels -> 4x4 tiles of every slice in one launch   (compress()'s own stages and helpers, RGBA kept together)
      -> ONE pack launch over all tiles of the file (dds_pack_kernels.hip) -> the payload, behind a 148-byte header written here

`fmt` is the tool's `-dds_format` token. The block encoders are the reference's (basist::encode_bc1 with cEncodeBC1HighQuality, basist::encode_bc4), restated
for the device in csrc/uastc_core.h / uastc_transcode.h; the raw formats truncate to their bits. BC7 is refused: neither of the reference's two BC7 packers is
implemented here. There is no CPU implementation: without the HIP library and a GPU `export_dds` and `pack_dds_blocks` raise. `dds_header` and `read_dds` are host code.

The other direction, .dds files as SOURCES of the compressor (the tool's `.dds` input files, comp.cpp:2310-2439): `read_dds_source` (host code) reads a 2D texture of
32-bit RGBA or BGRA pixels with its mip chain, and `compress_dds` hands level 0 and the file's own lower levels to compress()'s pipeline -- each file's payload
uploaded once, one launch of mip_levels_kernels.hip for all levels.
"""
import ctypes as C
import struct

import numpy as np

from . import mipmap, source as _source
from .compress import _checked, _resident_level0, _tiles
from .transcode import TranscodeSlice, _output

# token -> (bu_hip's BU_HIP_DDS_* value = the tool's dds_output_format, block format?, bytes per block / per pixel, DXGI UNORM code, DXGI sRGB code or 0)
FORMATS = {
    "bc1": (0, True, 8, 71, 72), "bc2": (1, True, 16, 74, 75), "bc3": (2, True, 16, 77, 78), "bc4": (3, True, 8, 80, 0), "bc5": (4, True, 16, 83, 0),
    "bc7": (5, True, 16, 98, 99),
    "a8r8g8b8": (6, False, 4, 87, 91), "a8b8g8r8": (7, False, 4, 28, 29), "r8": (8, False, 1, 61, 0), "r8g8": (9, False, 2, 49, 0), "r5g6b5": (10, False, 2, 85, 0),
    "a1r5g5b5": (11, False, 2, 86, 0), "a4r4g4b4": (12, False, 2, 115, 0),
}
ALIASES = {"a1r5g6b5": "a1r5g5b5"}   # the tool tolerates this (geometrically impossible) spelling
BC7_REFUSAL = ("dds format 'bc7' is not supported: the reference packs BC7 with bc7f or bc7e_scalar, and neither of the two packers is implemented here "
               "(supported: " + ", ".join(t for t in FORMATS if t != "bc7") + ")")
TEX_TYPE_REFUSAL = "tex_type {!r} is not supported for a .dds file (the header written is a 2D texture's); use '2d', '2darray' or 'cubemap'"
HEADER_BYTES = 148   # "DDS ", DDS_HEADER (124), DDS_HEADER_DXT10 (20)
NO_ALPHA_SLICE = 0xFFFFFFFFFFFFFFFF   # BU_HIP_NO_ALPHA_SLICE

_DDSD_CAPS, _DDSD_HEIGHT, _DDSD_WIDTH, _DDSD_PITCH, _DDSD_PIXELFORMAT, _DDSD_MIPMAPCOUNT, _DDSD_LINEARSIZE = 0x1, 0x2, 0x4, 0x8, 0x1000, 0x20000, 0x80000
_DDSCAPS_COMPLEX, _DDSCAPS_TEXTURE, _DDSCAPS_MIPMAP = 0x8, 0x1000, 0x400000
_DDSCAPS2_CUBEMAP_ALL = 0x200 | 0xFC00
_DDPF_FOURCC, _DX10, _TEXTURE2D, _MISC_TEXTURECUBE = 0x4, 0x30315844, 3, 0x4
_BY_DXGI = {code: (token, srgb) for token, (_, _, _, unorm, s) in FORMATS.items() for code, srgb in ((unorm, False), (s, True)) if code}


def parse_format(fmt):
    """the tool's -dds_format token, case-insensitive -> the canonical token. ValueError for bc7 and for what is no token."""
    token = str(fmt).lower()
    token = ALIASES.get(token, token)
    if token == "bc7":
        raise ValueError(BC7_REFUSAL)
    if token not in FORMATS:
        raise ValueError(f"dds format {fmt!r} is unknown (supported: {', '.join(t for t in FORMATS if t != 'bc7')})")
    return token


def subresource_bytes(token, width, height):
    _, block, unit, _, _ = FORMATS[token]
    return ((width + 3) // 4) * ((height + 3) // 4) * unit if block else width * height * unit


def dds_header(width, height, levels, array_size, cubemap, fmt, srgb=True):
    """build_dx10_header (dds_export.cpp:270-332): the 148 bytes in front of the payload. array_size counts cubes for a cubemap. The sRGB DXGI code is written when
    `srgb` is set and the format has one (bc4, bc5 and the 8 / 16-bit formats have none: UNORM)."""
    token = fmt if fmt in FORMATS else parse_format(fmt)
    _, block, unit, unorm, srgb_code = FORMATS[token]
    flags = _DDSD_CAPS | _DDSD_HEIGHT | _DDSD_WIDTH | _DDSD_PIXELFORMAT | (_DDSD_LINEARSIZE if block else _DDSD_PITCH) | (_DDSD_MIPMAPCOUNT if levels > 1 else 0)
    pitch = subresource_bytes(token, width, height) if block else width * unit
    caps = _DDSCAPS_TEXTURE | (_DDSCAPS_COMPLEX if levels > 1 or cubemap or array_size > 1 else 0) | (_DDSCAPS_MIPMAP if levels > 1 else 0)
    head = struct.pack("<4s7I44x", b"DDS ", 124, flags, height, width, pitch & 0xFFFFFFFF, 0, levels)
    head += struct.pack("<8I", 32, _DDPF_FOURCC, _DX10, 0, 0, 0, 0, 0)
    head += struct.pack("<5I", caps, _DDSCAPS2_CUBEMAP_ALL if cubemap else 0, 0, 0, 0)
    head += struct.pack("<5I", srgb_code if srgb and srgb_code else unorm, _TEXTURE2D, _MISC_TEXTURECUBE if cubemap else 0, array_size, 0)
    assert len(head) == HEADER_BYTES
    return head


def _records(slices, unit, block):
    """slice_table's slices -> (bu_hip_transcode_slice records with the subresources back to back, the payload's bytes)"""
    recs, at = (TranscodeSlice * max(len(slices), 1))(), 0
    for k, s in enumerate(slices):
        recs[k] = TranscodeSlice(int(s[0]), NO_ALPHA_SLICE, at, int(s[1]), int(s[2]), int(s[3]), int(s[4]), 0, 0)
        at += (s[1] * s[2] if block else s[3] * s[4]) * unit
    return recs, at


def export_dds(ctx, image, fmt, *, mipmaps=False, srgb=True, tex_type="2d", renormalize=False, swizzle=None, check_for_alpha=True, force_alpha=False, y_flip=False,
               resample=None, mip_filter="kaiser", mip_scale=1.0, mip_wrapping=True, mip_srgb=None, mip_renormalize=False, mip_fast=True, mip_smallest_dimension=1):
    """image: (h, w, 4) uint8 RGBA, or a sequence of such arrays with tex_type "2darray" (a layer each) or "cubemap" (six consecutive images are the faces of a
    layer). Returns the .dds file the reference tool writes with `-dds -dds_format <fmt>` for the same options, as a uint8 array.
    fmt: bc1, bc2, bc3, bc4, bc5, a8r8g8b8, a8b8g8r8, r8, r8g8, r5g6b5, a1r5g5b5 (alias a1r5g6b5) or a4r4g4b4, in either case.
    mipmaps (`-mipmap`), srgb (False = `-linear`: the UNORM DXGI code, linear mip filtering), and every source and mip option of compress(), with its meaning there:
    renormalize, swizzle, check_for_alpha, force_alpha, y_flip, resample, mip_filter, mip_scale, mip_wrapping, mip_srgb, mip_renormalize, mip_fast,
    mip_smallest_dimension. The stages are compress()'s own (the UASTC path's: a slice keeps its four channels); the payload is one pack launch over all tiles.
    ValueError before ctx is touched: bc7 (neither of the reference's BC7 packers is implemented here) and unknown formats, tex_type "video" and "volume" (the tool
    refuses them for -dds), and everything compress() refuses for its images, options and several images per call."""
    token = parse_format(fmt)
    if tex_type in ("video", "volume"):
        raise ValueError(TEX_TYPE_REFUSAL.format(tex_type))
    bare = not (isinstance(image, (list, tuple)) and (not len(image) or np.ndim(image[0]) == 3) or (isinstance(image, np.ndarray) and image.ndim == 4))
    prepare_options = dict(renormalize=renormalize, swizzle=swizzle, check_for_alpha=check_for_alpha, force_alpha=force_alpha, y_flip=y_flip)
    imgs, level_sizes, _, host_alpha, _ = _checked(
        [image] if bare else list(image), bare, prepare_options, uastc=True, mipmaps=mipmaps, ktx2=False, key_values=(), stats=None, resample=resample, mip_filter=mip_filter,
        mip_scale=mip_scale, mip_smallest_dimension=mip_smallest_dimension, tex_type=tex_type, us_per_frame=0, userdata=(0, 0), ktx2_animdata=(1, 15, 0))
    cubemap = tex_type == "cubemap"
    (width, height), levels = level_sizes[0][0], len(level_sizes[0])
    head = dds_header(width, height, levels, len(imgs) // (6 if cubemap else 1), cubemap, token, srgb)
    owned = []
    try:
        level0, image_alpha, has_alpha = _resident_level0(ctx, owned, imgs, level_sizes, host_alpha, prepare_options, resample=resample, srgb=srgb)
        return _export_resident(ctx, owned, level0, level_sizes, image_alpha, has_alpha, token, head, tex_type=tex_type, mip_srgb=srgb if mip_srgb is None else mip_srgb,
                                mip_filter=mip_filter, mip_scale=mip_scale, mip_wrapping=mip_wrapping, mip_fast=mip_fast, mip_renormalize=mip_renormalize)
    finally:
        for d in owned:
            ctx.free(d)


def _export_resident(ctx, owned, level0, level_sizes, image_alpha, has_alpha, token, head, *, tex_type, mip_srgb, mip_filter, mip_scale, mip_wrapping, mip_fast, mip_renormalize):
    """Resident, prepared level-0 rasters -> the file: the mip chains, the tiles of every slice in one launch, ONE pack launch, one download behind the header. What is
    allocated goes into the caller's `owned`. tools/dds_export_bench.py times this from rasters it keeps resident."""
    code, block, unit, _, _ = FORMATS[token]
    rasters = [mipmap.resident_chain(ctx, owned, d, sizes, srgb=mip_srgb, filter=mip_filter, filter_scale=mip_scale, wrapping=mip_wrapping,
                                     num_comps=4 if has_alpha else 3, fast=mip_fast, renormalize=mip_renormalize) for d, sizes in zip(level0, level_sizes)]
    # slice order -- image outermost, then level -- is DDS subresource order (layer, face, level)
    d_all, slices, _ = _tiles(ctx, owned, rasters, level_sizes, tex_type=tex_type, uastc=True, has_alpha=has_alpha, image_alpha=image_alpha, video=False, with_planes=False)
    n_tiles = sum(s[1] * s[2] for s in slices)
    recs, payload = _records(slices, unit, block)
    d_out = ctx.alloc(max(payload, 1))
    owned.append(d_out)
    if block:
        ctx.check(ctx.lib.k_pack_dds_blocks(ctx.h, C.c_void_p(d_all), n_tiles, code, C.c_void_p(d_out)), "pack_dds_blocks")
    else:
        ctx.check(ctx.lib.k_pack_dds_pixels(ctx.h, C.c_void_p(d_all), n_tiles, recs, len(slices), code, C.c_void_p(d_out), payload), "pack_dds_pixels")
    data = np.empty(HEADER_BYTES + payload, np.uint8)
    data[:HEADER_BYTES] = np.frombuffer(head, np.uint8)
    ctx.memcpy_d2h(data[HEADER_BYTES:], d_out)
    return data


def _resident_tiles(ctx, tiles, n_tiles):
    """tiles as an array (n_tiles x 64 bytes: 16 RGBA texels in rows of four) uploaded, or a device pointer as it is -> (device pointer, ours to free or None)"""
    if isinstance(tiles, np.ndarray):
        tiles = np.ascontiguousarray(tiles, np.uint8)
        if tiles.size != n_tiles * 64:
            raise ValueError(f"{n_tiles} tiles need {n_tiles * 64} bytes, got {tiles.size}")
        d = ctx.upload(tiles)
        return d, d
    return int(tiles), None


def pack_dds_blocks(ctx, tiles, n_tiles, fmt, *, out_device=None):
    """The block kernel on its own (bu_hip_k_pack_dds_blocks). tiles: an array of n_tiles x 64 bytes (16 RGBA texels per tile, rows of four; uploaded once) or a
    device pointer (int) to that many resident tiles. fmt: bc1 .. bc5. Returns (n_tiles, 8 | 16) uint8, or None when out_device (a device pointer with room for
    n_tiles blocks) receives them. ValueError for bc7, unknown formats and raw formats before ctx is touched."""
    token, n_tiles = parse_format(fmt), int(n_tiles)
    code, block, unit, _, _ = FORMATS[token]
    if not block:
        raise ValueError(f"dds format {token!r} is a pixel format: pack_dds_blocks takes bc1, bc2, bc3, bc4 or bc5")
    if n_tiles < 0:
        raise ValueError("n_tiles is negative")
    if not n_tiles:
        return None if out_device is not None else np.zeros((0, unit), np.uint8)
    d_tiles, own = _resident_tiles(ctx, tiles, n_tiles)
    try:
        with _output(ctx, out_device, 0, 0, lambda: n_tiles * unit) as d_out:
            ctx.check(ctx.lib.k_pack_dds_blocks(ctx.h, C.c_void_p(d_tiles), n_tiles, code, C.c_void_p(d_out)), "pack_dds_blocks")
            return None if out_device is not None else ctx.download(d_out, (n_tiles, unit), np.uint8)
    finally:
        if own:
            ctx.free(own)


def pack_dds_pixels(ctx, tiles, sizes, fmt, *, out_device=None):
    """The raw-format kernel on its own (bu_hip_k_pack_dds_pixels). sizes: the (width, height) of every slice, in order; tiles: the slices' tiles back to back (each
    slice ceil(width / 4) x ceil(height / 4) of them in raster order), as an array or a device pointer. fmt: one of the seven raw formats. Returns the subresources
    back to back in tight rows as a uint8 array, or None when out_device (room for that many bytes) receives them."""
    token = parse_format(fmt)
    code, block, unit, _, _ = FORMATS[token]
    if block:
        raise ValueError(f"dds format {token!r} is a block format: pack_dds_pixels takes the raw formats")
    slices, first = [], 0
    for w, h in sizes:
        w, h = int(w), int(h)
        if w <= 0 or h <= 0:
            raise ValueError(f"a slice of {w} x {h} pixels")
        slices.append((first, (w + 3) // 4, (h + 3) // 4, w, h))
        first += slices[-1][1] * slices[-1][2]
    if not slices:
        raise ValueError("no slices")
    recs, payload = _records(slices, unit, False)
    d_tiles, own = _resident_tiles(ctx, tiles, first)
    try:
        with _output(ctx, out_device, 0, 0, lambda: payload) as d_out:
            ctx.check(ctx.lib.k_pack_dds_pixels(ctx.h, C.c_void_p(d_tiles), first, recs, len(slices), code, C.c_void_p(d_out), payload), "pack_dds_pixels")
            return None if out_device is not None else ctx.download(d_out, (payload,), np.uint8)
    finally:
        if own:
            ctx.free(own)


LEGACY_HEADER_BYTES = 128   # "DDS ", DDS_HEADER (124)
_DDPF_ALPHA, _DDPF_RGB, _DDSCAPS2_CUBEMAP, _DDSCAPS2_VOLUME, _TEXTURE3D = 0x2, 0x40, 0x200, 0x200000, 4
_SOURCE_DXGI = {28: ("rgba", False), 29: ("rgba", True), 87: ("bgra", False), 91: ("bgra", True)}   # R8G8B8A8_UNORM / _SRGB, B8G8R8A8_UNORM / _SRGB
_SOURCE_MASKS = {(0x000000FF, 0x0000FF00, 0x00FF0000, 0xFF000000): "rgba",     # D3DFMT_A8B8G8R8
                 (0x00FF0000, 0x0000FF00, 0x000000FF, 0xFF000000): "bgra"}     # D3DFMT_A8R8G8B8
_DXGI_KINDS = [("a block-compressed format", (*range(70, 85), *range(94, 100))), ("a float format", (2, 6, 10, 16, 34, 41, 54)),
               ("a 16-bit format", (*range(11, 15), *range(35, 39), *range(56, 60), 85, 86, 115))]
_FOURCC_KINDS = [("a block-compressed format", tuple(int.from_bytes(t, "little") for t in (b"DXT1", b"DXT2", b"DXT3", b"DXT4", b"DXT5", b"ATI1", b"ATI2", b"BC4U", b"BC4S",
                                                                                           b"BC5U", b"BC5S"))),
                 ("a float format", (111, 112, 113, 114, 115, 116)), ("a 16-bit format", (34, 36, 110))]


def _kind(code, kinds):
    return next((kind for kind, codes in kinds if code in codes), None)


def read_dds_source(data):
    """A .dds file as a SOURCE of compress_dds: what the reference tool reads as one (read_uncompressed_dds_file, encoder/basisu_gpu_texture.cpp:2025-2210, through
    tinydds) for the LDR compressor -- a 2D texture of 32-bit RGBA or BGRA pixels with its mip chain: a DX10 header with DXGI format 28, 29 (R8G8B8A8 UNORM / SRGB),
    87 or 91 (B8G8R8A8 UNORM / SRGB), or a legacy header whose bit masks are those of A8B8G8R8 or A8R8G8B8. The chain may stop early; a mip count of 0 is one level and a
    count past the full chain is cut to it, as the tool's reader does. Bytes behind the last level are ignored.
    -> {"width", "height", "byte_order" ("rgba" | "bgra"), "srgb", "dx10", "levels": per level {"level", "width", "height", "offset" (into "payload"), "nbytes"},
        "payload": the levels' bytes, a uint8 view of `data`}. Every size is checked against the buffer before anything is listed.
    ValueError, naming the reason: a truncated file; texture arrays, cubemaps, volumes and 1D textures (a height of 1 is one to the tool); block-compressed, 16-bit and
    float formats (HDR .dds sources belong to codecs this package does not have) and every other pixel format; a size outside 1..16384."""
    raw = np.frombuffer(data.tobytes() if isinstance(data, np.ndarray) else bytes(data), np.uint8)
    if raw.size < LEGACY_HEADER_BYTES:
        raise ValueError(f"truncated .dds file: the header needs {LEGACY_HEADER_BYTES} bytes, {raw.size} are here")
    magic, size, _flags, height, width, _pitch, depth, levels = struct.unpack_from("<4s7I", raw, 0)
    pf_size, pf_flags, fourcc, bits, *masks = struct.unpack_from("<8I", raw, 76)
    _caps, caps2 = struct.unpack_from("<2I", raw, 108)
    if magic != b"DDS " or size != 124 or pf_size != 32:
        raise ValueError("not a .dds file (magic or header sizes)")
    dx10 = bool(pf_flags & _DDPF_FOURCC) and fourcc == _DX10
    header, dimension, misc, array_size = LEGACY_HEADER_BYTES, _TEXTURE2D, 0, 1
    if dx10:
        header = HEADER_BYTES
        if raw.size < header:
            raise ValueError(f"truncated .dds file: the DX10 header needs {header} bytes, {raw.size} are here")
        dxgi, dimension, misc, array_size, _misc2 = struct.unpack_from("<5I", raw, 128)
    if array_size > 1:
        raise ValueError(f"a texture array of {array_size} layers: the tool reads 2D textures only as sources; compress the layers as several files (tex_type '2darray')")
    if caps2 & _DDSCAPS2_CUBEMAP or misc & _MISC_TEXTURECUBE:
        raise ValueError("a cubemap: the tool reads 2D textures only as sources; compress the faces as six files (tex_type 'cubemap')")
    if depth > 1 or caps2 & _DDSCAPS2_VOLUME or dimension == _TEXTURE3D:
        raise ValueError("a volume texture: the tool reads 2D textures only as sources")
    if dx10:
        if dxgi not in _SOURCE_DXGI:
            raise ValueError(f"DXGI format {dxgi} is {_kind(dxgi, _DXGI_KINDS) or 'another pixel format'}: a .dds source is 32-bit R8G8B8A8 or B8G8R8A8, "
                             "UNORM or SRGB (DXGI 28, 29, 87, 91)")
        byte_order, srgb = _SOURCE_DXGI[dxgi]
    elif pf_flags & _DDPF_FOURCC:
        kind = _kind(fourcc, _FOURCC_KINDS)
        raise ValueError(f"FourCC {fourcc:#x} is {kind or 'another pixel format'}: a .dds source is 32-bit RGBA or BGRA")
    else:
        if bits == 16:
            raise ValueError("a 16-bit format (legacy header, 16 bits per pixel): a .dds source is 32-bit RGBA or BGRA")
        if not pf_flags & (_DDPF_RGB | _DDPF_ALPHA) or bits != 32 or tuple(masks) not in _SOURCE_MASKS:
            raise ValueError(f"a legacy header of {bits} bits per pixel with masks {', '.join(f'{m:#010x}' for m in masks)}: only those of A8B8G8R8 and A8R8G8B8 are read")
        byte_order, srgb = _SOURCE_MASKS[tuple(masks)], False
    if not 1 <= width <= _source.MAX_DIMENSION or not 1 <= height <= _source.MAX_DIMENSION:
        raise ValueError(f"{width} x {height} pixels: 1..{_source.MAX_DIMENSION} each way")
    if height == 1:
        raise ValueError(f"{width} x 1 pixels: a height of 1 is a 1D texture to the tool, which reads 2D textures only as sources")
    levels = min(max(levels, 1), max(width, height).bit_length())
    listed, at = [], 0
    for level in range(levels):
        w, h = max(1, width >> level), max(1, height >> level)
        listed.append({"level": level, "width": w, "height": h, "offset": at, "nbytes": w * h * 4})
        at += w * h * 4
    if header + at > raw.size:
        raise ValueError(f"truncated .dds file: {levels} levels of {width} x {height} 32-bit pixels are {at} bytes behind {header} header bytes, and {raw.size} bytes are here")
    return {"width": width, "height": height, "byte_order": byte_order, "srgb": srgb, "dx10": dx10, "levels": listed, "payload": raw[header:header + at]}


def compress_dds(ctx, data, **options):
    """.dds sources to a .basis / .ktx2 file: what the reference tool does with `.dds` input files (basis_compressor::read_dds_source_images, comp.cpp:2310-2439).
    data: the bytes of one .dds file (bytes or a uint8 array), or a sequence of them with tex_type "2darray", "cubemap", "video" or "volume". options: compress()'s
    keyword arguments, except mip_levels. Level 0 of a file is the source image and goes through every source option; the levels below it are used as they are
    (compress()'s mip_levels: the swizzle alone touches them, they win over `mipmaps`, alpha in any of them gives the file alpha); a file of one level is a plain image.
    Each file's payload is uploaded once, as it is; ONE launch makes RGBA rasters of level 0 (the file's byte order) and of all lower levels (byte order and swizzle);
    the rest is compress()'s pipeline. ValueError before ctx is touched: whatever read_dds_source refuses, files whose level counts or sizes differ, `resample` with a
    file that has lower levels, and everything else compress() refuses."""
    bare = isinstance(data, (bytes, bytearray, memoryview)) or (isinstance(data, np.ndarray) and data.ndim == 1)
    if "mip_levels" in options:
        raise ValueError("mip_levels with .dds sources: the levels below level 0 are the file's")
    from .compress import compress
    return compress(ctx, _source.DdsSources([read_dds_source(d) for d in ([data] if bare else data)], bare), **options)


def read_dds(data):
    """A reader of exactly the files written here (and by the tool's -dds mode): the DX10 header -> {"format" (token), "block" (a block format?), "srgb", "dxgi_format",
    "width", "height", "levels", "layers", "faces", "images": per subresource in file order {"level", "layer", "face", "width", "height", "num_blocks_x",
    "num_blocks_y", "offset", "nbytes"}}. Every size is checked against the buffer before anything is listed: ValueError for a truncated or inconsistent file.
    The bytes of a bc1 / bc3 / bc4 / bc5 subresource go straight into transcode.unpack_blocks."""
    raw = data.tobytes() if isinstance(data, np.ndarray) else bytes(data)
    if len(raw) < HEADER_BYTES:
        raise ValueError(f"truncated .dds file: the DX10 header needs {HEADER_BYTES} bytes, {len(raw)} are here")
    magic, size, flags, height, width, pitch, depth, levels = struct.unpack_from("<4s7I", raw, 0)
    pf_size, pf_flags, fourcc = struct.unpack_from("<3I", raw, 76)
    caps, caps2 = struct.unpack_from("<2I", raw, 108)
    dxgi, dimension, misc, array_size, _misc2 = struct.unpack_from("<5I", raw, 128)
    if magic != b"DDS " or size != 124 or pf_size != 32:
        raise ValueError("not a .dds file (magic or header sizes)")
    if not pf_flags & _DDPF_FOURCC or fourcc != _DX10:
        raise ValueError("not a DX10 .dds file: only the DX10 header extension is read here")
    if dxgi not in _BY_DXGI or _BY_DXGI[dxgi][0] == "bc7":
        raise ValueError(f"DXGI format {dxgi} is not one this package writes")
    token, srgb = _BY_DXGI[dxgi]
    _, block, unit, _, _ = FORMATS[token]
    if dimension != _TEXTURE2D or depth:
        raise ValueError("not a 2D texture")
    if not 1 <= width <= _source.MAX_DIMENSION or not 1 <= height <= _source.MAX_DIMENSION:
        raise ValueError(f"{width} x {height} pixels: 1..{_source.MAX_DIMENSION} each way")
    if not 1 <= levels <= max(width, height).bit_length():
        raise ValueError(f"{levels} levels for {width} x {height} pixels")
    cubemap = bool(misc & _MISC_TEXTURECUBE)
    if cubemap != (caps2 == _DDSCAPS2_CUBEMAP_ALL) or (not cubemap and caps2):
        raise ValueError("the cubemap flags of the two headers disagree (a cubemap here has all six faces)")
    expect = dds_header(width, height, levels, array_size, cubemap, token, srgb)
    if (flags, pitch, caps) != (struct.unpack_from("<I", expect, 8)[0], struct.unpack_from("<I", expect, 20)[0], struct.unpack_from("<I", expect, 108)[0]):
        raise ValueError("flags, pitch / linear size or caps are not what this format and size are written with")
    if raw[:HEADER_BYTES] != expect:
        raise ValueError("a header field this package writes as 0 (reserved words, bit masks, further flags) is set")
    faces = 6 if cubemap else 1
    sizes = [(max(1, width >> level), max(1, height >> level)) for level in range(levels)]
    chain = sum(subresource_bytes(token, w, h) for w, h in sizes)
    if array_size < 1 or HEADER_BYTES + array_size * faces * chain != len(raw):
        raise ValueError(f"truncated or corrupt .dds file: {array_size} x {faces} x {levels} subresources of {chain} bytes per chain behind {HEADER_BYTES} header bytes "
                         f"are not the {len(raw)} bytes here")
    images, at = [], HEADER_BYTES
    for layer in range(array_size):
        for face in range(faces):
            for level, (w, h) in enumerate(sizes):
                n = subresource_bytes(token, w, h)
                images.append({"level": level, "layer": layer, "face": face, "width": w, "height": h, "num_blocks_x": (w + 3) // 4, "num_blocks_y": (h + 3) // 4,
                               "offset": at, "nbytes": n})
                at += n
    assert at == len(raw)
    return {"format": token, "block": block, "srgb": srgb, "dxgi_format": dxgi, "width": width, "height": height, "levels": levels, "layers": array_size, "faces": faces,
            "images": images}
