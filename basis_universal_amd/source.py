"""The compressor's source-image options on the device: what basis_compressor::read_source_images (encoder/basisu_comp.cpp:2569-2697) does to a source image before the
first block is cut -- `basisu -renorm`, `-swizzle` / `-separate_rg_to_color_alpha`, `-force_alpha` / `-no_alpha`, `-y_flip` in one pass of source_prep_kernels.hip
(the per-pixel rules: csrc/source_prep.h), then `-resample` / `-resample_factor` through the mip generator's resampler -- and the argument checks compress() shares.
For several source images per call (texture arrays, cubemaps, video, volumes): the texture-type rules of basis_compressor::validate_texture_type_constraints, the
slice table of read_source_images (both pure functions), and the one-launch tiling of every slice (bu_hip_k_extract_slices).
For mip levels the caller made (m_source_mipmap_images; the levels of a .dds source): the selector word of a level, and every level of a call from one resident payload
into tight rasters by one launch (bu_hip_k_prepare_mip_levels).
Nothing here has a CPU implementation."""
import ctypes
import math

import numpy as np

MIP_FILTERS = ("box", "tent", "bell", "mitchell", "blackman", "lanczos3", "lanczos4", "lanczos6", "lanczos12", "kaiser", "catmullrom")   # csrc/host/mipmap.h
IDENTITY_SWIZZLE = 0x03020100
MAX_DIMENSION = 16384          # basist::BASISU_MAX_SUPPORTED_TEXTURE_DIMENSION
_LETTERS = {"r": 0, "g": 1, "b": 2, "a": 3, "0": 0, "1": 1, "2": 2, "3": 3}
TEX_TYPES = {"2d": 0, "2darray": 1, "cubemap": 2, "video": 3, "volume": 4}   # basist::basis_texture_type; the tool's -tex_type 2d|2darray|cubemap|video|3d
MAX_SLICES = 0xFFFFFF          # BASISU_MAX_SLICES (comp.h:67)
SLICE_AS_IS, SLICE_RGB, SLICE_ALPHA = 0, 1, 2   # BU_HIP_SLICE_*: the pixels as they are, (r, g, b, 255), (a, a, a, 255)


def normal_map_options():
    """The keyword arguments of compress() that `basisu -normal_map` (= `-texture`, basisu_tool.cpp:1765-1779) sets, for ETC1S and UASTC LDR 4x4:
    set_srgb_options(false) -- linear metrics, linear mip filtering, no sRGB transfer function in the file -- and both backend RDO stages off. What else the preset
    touches (channel weights, sharpening, deblocking) belongs to codecs this package does not have. It does NOT renormalise: add renormalize / mip_renormalize."""
    return {"srgb": False, "mip_srgb": False, "no_selector_rdo": True, "no_endpoint_rdo": True}


def parse_swizzle(swizzle):
    """None, four of "rgba" / "0123" (either case, as `-swizzle` takes them) or four ints 0..3 -> s0 | s1 << 8 | s2 << 16 | s3 << 24. "rrrg" is the tool's
    -separate_rg_to_color_alpha."""
    if swizzle is None:
        return IDENTITY_SWIZZLE
    if isinstance(swizzle, str):
        if len(swizzle) != 4 or any(c.lower() not in _LETTERS for c in swizzle):
            raise ValueError(f"swizzle {swizzle!r}: exactly 4 characters, each one of [rgba] or [0123]")
        entries = [_LETTERS[c.lower()] for c in swizzle]
    else:
        entries = list(swizzle)
        if len(entries) != 4 or any(isinstance(e, bool) or not isinstance(e, (int, np.integer)) or not 0 <= e <= 3 for e in entries):
            raise ValueError(f"swizzle {swizzle!r}: four channel indices 0..3")
    return sum(int(e) << (8 * i) for i, e in enumerate(entries))


def resampled_size(w, h, resample):
    """None -> None; (w, h) -> itself; a factor -> (max(1, ceilf(w * f)), max(1, ceilf(h * f))) in binary32, both capped at 16384 (comp.cpp:2649-2697)."""
    if resample is None:
        return None
    if isinstance(resample, (int, float, np.floating, np.integer)) and not isinstance(resample, bool):
        f = np.float32(resample)
        if not f > 0 or not np.isfinite(f):
            raise ValueError(f"resample factor {resample!r} must be positive")
        size = [max(1, int(math.ceil(np.float32(np.float32(v) * f)))) for v in (w, h)]
    else:
        size = list(resample)
        if len(size) != 2 or any(isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v <= 0 for v in size):
            raise ValueError(f"resample {resample!r}: (width, height), both positive, or a factor")
    return tuple(min(int(v), MAX_DIMENSION) for v in size)


def check_mip_options(mip_filter, mip_scale, mip_smallest_dimension):
    if mip_filter not in MIP_FILTERS:
        raise ValueError(f"mip_filter {mip_filter!r} is not one of {', '.join(MIP_FILTERS)}")
    if not float(mip_scale) > 0 or not math.isfinite(float(mip_scale)):
        raise ValueError(f"mip_scale {mip_scale!r} must be positive")
    if isinstance(mip_smallest_dimension, bool) or not isinstance(mip_smallest_dimension, (int, np.integer)) or mip_smallest_dimension < 1:
        raise ValueError(f"mip_smallest_dimension {mip_smallest_dimension!r} must be an integer >= 1")


def is_identity(renormalize, swizzle, check_for_alpha, force_alpha, y_flip):
    """True where the options leave every pixel alone and has_alpha is image::has_alpha of the image as it is: the prepare kernel has nothing to do"""
    return not renormalize and parse_swizzle(swizzle) == IDENTITY_SWIZZLE and bool(check_for_alpha) and not force_alpha and not y_flip


def prepare_resident(ctx, d_src, w, h, d_dst, *, renormalize=False, swizzle=None, check_for_alpha=True, force_alpha=False, y_flip=False, src_pitch=None, dst_pitch=None):
    """bu_hip_k_prepare_source on resident rasters -> (has_alpha, any prepared alpha below 255). With only `renormalize` set and d_dst == d_src it is the in-place
    renormalisation plus the flag. force_alpha wins over check_for_alpha=False, as in the reference (comp.cpp:2616-2621)."""
    has_alpha, below = ctypes.c_uint32(0), ctypes.c_uint32(0)
    ctx.check(ctx.lib.k_prepare_source(ctx.h, ctypes.c_void_p(d_src), w, h, src_pitch or w * 4, ctypes.c_void_p(d_dst), dst_pitch or w * 4, int(bool(renormalize)), parse_swizzle(swizzle),
                                       int(bool(check_for_alpha)), int(bool(force_alpha)), int(bool(y_flip)), ctypes.byref(has_alpha), ctypes.byref(below)), "k_prepare_source")
    return bool(has_alpha.value), bool(below.value)


def renormalize_resident(ctx, d_raster, w, h, pitch=None):
    """image::renormalize_normal_map in place on a resident raster (the mip levels of mip_renormalize); no synchronisation"""
    ctx.check(ctx.lib.k_renormalize_normal_map(ctx.h, ctypes.c_void_p(d_raster), w, h, pitch or w * 4), "k_renormalize_normal_map")


def split_alpha_resident(ctx, d_raster, w, h, d_rgb, d_alpha, pitch=None, rgb_pitch=None, alpha_pitch=None):
    """(r, g, b, 255) -> d_rgb (may be d_raster) and (a, a, a, 255) -> d_alpha: the two ETC1S slices of a level with alpha; no synchronisation"""
    ctx.check(ctx.lib.k_split_alpha(ctx.h, ctypes.c_void_p(d_raster), w, h, pitch or w * 4, ctypes.c_void_p(d_rgb), rgb_pitch or w * 4, ctypes.c_void_p(d_alpha), alpha_pitch or w * 4), "k_split_alpha")


def resample_resident(ctx, d_src, w, h, new_w, new_h, srgb):
    """image_resample(src, dst, srgb, "box") with that function's declared defaults for the rest (scale 1, no wrapping, all four components) -> a new resident raster"""
    from . import mipmap
    d = ctx.alloc(new_w * new_h * 4)
    try:
        ctx.check(mipmap._lib().bu_generate_mipmap_level(ctx.h, d_src, w, h, d, new_w, new_h, int(bool(srgb)), b"box", 1.0, 0, 4), "bu_generate_mipmap_level")
    except Exception:
        ctx.free(d)
        raise
    return d


def prepare_source(ctx, image_or_device, width=None, height=None, *, renormalize=False, swizzle=None, check_for_alpha=True, force_alpha=False, y_flip=False,
                   resample=None, srgb=True):
    """image_or_device: an (h, w, 4) uint8 RGBA array, or a resident tightly packed RGBA8 raster (a device address) with width and height; a resident source is left
    as it is. Returns (d_raster, (width, height), has_alpha): a NEW resident raster the caller frees with ctx.free, prepared in the reference's order -- renormalise,
    swizzle, alpha policy, flip, then resample (`srgb` = the compressor's perceptual flag, which picks the resampler's transfer function) --, its size, and the
    reference's has_alpha of the source image, decided BEFORE the resample as the reference decides it.
    swizzle: four of "rgba" or four ints. force_alpha wins over check_for_alpha=False. Bad arguments raise ValueError before ctx is touched."""
    packed = parse_swizzle(swizzle)
    if isinstance(image_or_device, (int, np.integer)) and not isinstance(image_or_device, bool):
        if width is None or height is None or int(width) <= 0 or int(height) <= 0:
            raise ValueError("a resident source needs its width and height, both positive")
        img, w, h = None, int(width), int(height)
    else:
        img = np.ascontiguousarray(image_or_device, np.uint8)
        if img.ndim != 3 or img.shape[2] != 4 or not img.shape[0] or not img.shape[1]:
            raise ValueError("image must be (h, w, 4) uint8, not empty")
        h, w = img.shape[:2]
    if w > MAX_DIMENSION or h > MAX_DIMENSION:
        raise ValueError(f"{w} x {h} pixels is too large ({MAX_DIMENSION} each way at the most)")
    new_size = resampled_size(w, h, resample)
    owned = []
    try:
        d_src = int(image_or_device) if img is None else ctx.upload(img)
        if img is not None:
            owned.append(d_src)
        if img is not None and not y_flip:
            d_out = d_src            # our own upload: prepared in place
        else:
            d_out = ctx.alloc(w * h * 4)
            owned.append(d_out)
        has_alpha, _ = prepare_resident(ctx, d_src, w, h, d_out, renormalize=renormalize, swizzle=packed_entries(packed), check_for_alpha=check_for_alpha,
                                        force_alpha=force_alpha, y_flip=y_flip)
        if new_size is not None:
            d_new = resample_resident(ctx, d_out, w, h, new_size[0], new_size[1], srgb)
            owned.append(d_new)
            d_out, (w, h) = d_new, new_size
        owned.remove(d_out)
        return d_out, (w, h), has_alpha
    finally:
        for d in owned:
            ctx.free(d)


def packed_entries(packed):
    return [(packed >> (8 * i)) & 255 for i in range(4)]


# ---- several source images per call

def check_texture_type(tex_type, sizes):
    """validate_texture_type_constraints (comp.cpp:3143-3200) and what comes before it, on the images' (width, height) alone. -> the basis_texture_type number."""
    if tex_type not in TEX_TYPES:
        raise ValueError(f"tex_type {tex_type!r} is not one of {', '.join(TEX_TYPES)}")
    if not sizes:
        raise ValueError("no source images: the sequence is empty")
    if tex_type == "2d":
        if len(sizes) > 1:
            raise ValueError(f"{len(sizes)} source images with tex_type '2d': the reference tool compresses those as separate files, one call each; for one file of "
                             "several images pass tex_type '2darray', 'cubemap', 'video' or 'volume'")
        return 0
    if tex_type == "cubemap" and len(sizes) % 6:
        raise ValueError(f"a cubemap of {len(sizes)} images: for cubemaps the total number of input images must be a multiple of 6")
    if any(size != sizes[0] for size in sizes):
        k = next(i for i, size in enumerate(sizes) if size != sizes[0])
        raise ValueError(f"the source image resolutions are not all equal (image 0 is {sizes[0][0]} x {sizes[0][1]}, image {k} is {sizes[k][0]} x {sizes[k][1]}): "
                         f"the images of a {tex_type} must all have one size")
    return TEX_TYPES[tex_type]


def check_slice_count(n_images, n_levels, split_alpha):
    n = n_images * n_levels * (2 if split_alpha else 1)
    if n > MAX_SLICES:
        raise ValueError(f"{n} slices ({n_images} images x {n_levels} levels{' x colour and alpha' if split_alpha else ''}): too many slices, "
                         f"BASISU_MAX_SLICES is {MAX_SLICES}")
    return n


def image_layer_face(tex_type, image):
    """where a source image lies in the file: cubemap faces are six consecutive images of a layer, everything else is a layer per image"""
    return (image // 6, image % 6) if tex_type in ("cubemap", 2) else (image, 0)


def slice_table(level_sizes, *, uastc, any_alpha, image_alpha=None, video=False):
    """The slices basis_compressor::read_source_images makes (comp.cpp:2773-3044), in its order: source image outermost, then level, then -- ETC1S with
    m_any_source_image_has_alpha -- the colour and the alpha slice.
    level_sizes: per source image the (width, height) of its levels; any_alpha: m_any_source_image_has_alpha; image_alpha: per image whether its raster has an alpha
    value below 255 (UASTC: the slice's own flag, image::has_alpha of the slice; without any_alpha no slice has one), or per image a list with a flag per level.
    -> (slices, sources): slices[i] = (first_block, num_blocks_x, num_blocks_y, width, height, image, level, alpha, iframe) as backend.slice_descs takes them;
    sources[i] = (image, level, mode) with mode one of SLICE_AS_IS / SLICE_RGB / SLICE_ALPHA: what the slice's tiles are cut from.
    video: ETC1S -- the slices of image 0 are i-frames; UASTC -- every slice is (comp.cpp:3016-3030)."""
    slices, sources, first = [], [], 0
    for image, levels in enumerate(level_sizes):
        for level, (w, h) in enumerate(levels):
            nbx, nby = (w + 3) // 4, (h + 3) // 4
            if uastc:
                own = image_alpha[image] if image_alpha is not None else False
                if isinstance(own, (list, tuple)):       # a flag per level: caller-supplied levels, each image::has_alpha of its own pixels
                    own = own[level]
                parts = [(SLICE_AS_IS, int(bool(any_alpha and own)))]
            else:
                parts = [(SLICE_RGB, 0), (SLICE_ALPHA, 1)] if any_alpha else [(SLICE_AS_IS, 0)]
            for mode, alpha in parts:
                iframe = int(bool(video) and (bool(uastc) or image == 0))
                slices.append((first, nbx, nby, w, h, image, level, alpha, iframe))
                sources.append((image, level, mode))
                first += nbx * nby
    return slices, sources


class SliceSource(ctypes.Structure):   # = bu_hip_slice_source, include/basisu_hip.h
    _fields_ = [("d_raster", ctypes.c_void_p), ("width", ctypes.c_uint32), ("height", ctypes.c_uint32), ("pitch_bytes", ctypes.c_uint32), ("mode", ctypes.c_uint32),
                ("first_block", ctypes.c_uint64)]


def extract_slices_resident(ctx, entries, d_out_blocks):
    """bu_hip_k_extract_slices: entries = [(d_raster, width, height, pitch_bytes or 0, mode, first_block)], every slice of the call tiled in ONE launch; no synchronisation"""
    arr = (SliceSource * max(len(entries), 1))()
    for i, (d, w, h, pitch, mode, first) in enumerate(entries):
        arr[i] = SliceSource(d, w, h, pitch or w * 4, mode, first)
    ctx.check(ctx.lib.k_extract_slices(ctx.h, arr, len(entries), ctypes.c_void_p(d_out_blocks)), "k_extract_slices")


# ---- mip levels the caller made (basis_compressor_params::m_source_mipmap_images; the levels of a .dds source)

BYTE_ORDERS = {"rgba": (0, 1, 2, 3), "bgra": (2, 1, 0, 3)}   # where a pixel's r, g, b, a lie in memory: DXGI R8G8B8A8 and B8G8R8A8


class MipLevelRecord(ctypes.Structure):   # = bu_hip_mip_level_record, include/basisu_hip.h
    _fields_ = [("src_offset", ctypes.c_uint64), ("dst_offset", ctypes.c_uint64), ("width", ctypes.c_uint32), ("height", ctypes.c_uint32), ("selector", ctypes.c_uint32),
                ("reserved", ctypes.c_uint32)]


def level_selector(byte_order="rgba", swizzle=None):
    """The selector word of a level's record: the source's byte order composed with the compressor's swizzle -- output channel i is the reader's channel swizzle[i],
    which lies at byte byte_order[swizzle[i]] of the source pixel. That is all the reference applies to a supplied level (comp.cpp:2796-2817)."""
    order = BYTE_ORDERS[byte_order]
    return sum(order[s] << (8 * i) for i, s in enumerate(packed_entries(parse_swizzle(swizzle))))


def full_chain_levels(w, h):
    """how many levels lie below level 0 of a full chain (down to 1 x 1)"""
    return max(int(w), int(h)).bit_length() - 1


def check_supplied_levels(name, w, h, sizes):
    """sizes: the (width, height) of the levels supplied below a w x h level 0; each must be the next halving, and the chain may stop early"""
    if len(sizes) > full_chain_levels(w, h):
        raise ValueError(f"{name}: {len(sizes)} mip levels below {w} x {h} pixels, whose full chain has {full_chain_levels(w, h)}")
    for k, size in enumerate(sizes, 1):
        want = (max(1, w >> k), max(1, h >> k))
        if tuple(size) != want:
            raise ValueError(f"{name}: mip level {k} is {size[0]} x {size[1]} pixels; level {k} of {w} x {h} is {want[0]} x {want[1]} (max(1, size >> level))")


def prepare_mip_levels_resident(ctx, d_payload, payload_bytes, records, d_out, out_bytes, d_flags):
    """bu_hip_k_prepare_mip_levels: records = [(src_offset, dst_offset, width, height, selector)], every level of the call in ONE launch; no synchronisation"""
    arr = (MipLevelRecord * max(len(records), 1))()
    for i, (src, dst, w, h, selector) in enumerate(records):
        arr[i] = MipLevelRecord(src, dst, w, h, selector, 0)
    ctx.check(ctx.lib.k_prepare_mip_levels(ctx.h, ctypes.c_void_p(d_payload), payload_bytes, arr, len(records), ctypes.c_void_p(d_out), out_bytes, ctypes.c_void_p(d_flags)),
              "k_prepare_mip_levels")


def resident_levels(ctx, owned, parts, levels):
    """parts: host uint8 arrays (C-contiguous, sizes multiples of 4), uploaded once each, back to back, into ONE resident payload; levels = [(part, byte offset within
    the part, width, height, selector)]. ONE prepare_mip_levels launch writes every level as a tight RGBA8 raster (each begins on a 16-byte line, so that the tiler
    reads whole rows) -> ([device address per level], [per level: is any written alpha not 255]). The call waits once, for the flags. What is allocated goes into the
    caller's `owned`."""
    starts, payload_bytes = [], 0
    for part in parts:
        starts.append(payload_bytes)
        payload_bytes += part.nbytes
    records, out_bytes = [], 0
    for part, offset, w, h, selector in levels:
        records.append((starts[part] + offset, out_bytes, w, h, selector))
        out_bytes += (w * h * 4 + 15) & ~15
    d_payload, d_out, d_flags = ctx.alloc(max(payload_bytes, 4)), ctx.alloc(max(out_bytes, 4)), ctx.alloc(4 * max(len(levels), 1))
    owned.extend((d_payload, d_out, d_flags))
    for part, at in zip(parts, starts):
        if part.nbytes:
            ctx.memcpy_h2d_async(d_payload + at, part)
    prepare_mip_levels_resident(ctx, d_payload, payload_bytes, records, d_out, out_bytes, d_flags)
    flags = ctx.download(d_flags, (max(len(levels), 1),), np.uint32)
    return [d_out + r[1] for r in records], [bool(f) for f in flags[:len(levels)]]


class DdsSources:
    """The source images of compress() as parsed .dds files (dds.read_dds_source): what dds.compress_dds hands to compress() in place of arrays. Level 0 and the lower
    levels stay in the file's bytes; `arrays` gives views of them for the argument checks, `resident` brings every level of every file to the device."""

    def __init__(self, files, bare):
        self.files, self.bare = list(files), bool(bare)

    def arrays(self):
        """-> (level-0 views, per file the views of its lower levels or None where no file has any): the file's bytes as they are, whatever the byte order"""
        views = [[f["payload"][lv["offset"]:lv["offset"] + lv["nbytes"]].reshape(lv["height"], lv["width"], 4) for lv in f["levels"]] for f in self.files]
        lower = [v[1:] for v in views]
        return [v[0] for v in views], (lower if any(lower) else None)

    def resident(self, ctx, owned, swizzle):
        """every file's payload uploaded once, ONE launch for level 0's byte order and the lower levels' byte order and swizzle
        -> per file ([level rasters], [the flag of each])"""
        levels = [(k, lv["offset"], lv["width"], lv["height"], level_selector(f["byte_order"], swizzle if i else None))
                  for k, f in enumerate(self.files) for i, lv in enumerate(f["levels"])]
        rasters, flags = resident_levels(ctx, owned, [f["payload"] for f in self.files], levels)
        out, at = [], 0
        for f in self.files:
            n = len(f["levels"])
            out.append((rasters[at:at + n], flags[at:at + n]))
            at += n
        return out
