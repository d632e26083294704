"""The compressor's source-image options on the device: what basis_compressor::read_source_images (encoder/basisu_comp.cpp:2569-2697) does to a source image before the
first block is cut -- `basisu -renorm`, `-swizzle` / `-separate_rg_to_color_alpha`, `-force_alpha` / `-no_alpha`, `-y_flip` in one pass of source_prep_kernels.hip
(the per-pixel rules: csrc/source_prep.h), then `-resample` / `-resample_factor` through the mip generator's resampler -- and the argument checks compress() shares.
Nothing here has a CPU implementation."""
import math

import numpy as np

MIP_FILTERS = ("box", "tent", "bell", "mitchell", "blackman", "lanczos3", "lanczos4", "lanczos6", "lanczos12", "kaiser", "catmullrom")   # csrc/host/mipmap.h
IDENTITY_SWIZZLE = 0x03020100
MAX_DIMENSION = 16384          # basist::BASISU_MAX_SUPPORTED_TEXTURE_DIMENSION
_LETTERS = {"r": 0, "g": 1, "b": 2, "a": 3, "0": 0, "1": 1, "2": 2, "3": 3}


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
    import ctypes as C
    has_alpha, below = C.c_uint32(0), C.c_uint32(0)
    ctx.check(ctx.lib.k_prepare_source(ctx.h, C.c_void_p(d_src), w, h, src_pitch or w * 4, C.c_void_p(d_dst), dst_pitch or w * 4, int(bool(renormalize)), parse_swizzle(swizzle),
                                       int(bool(check_for_alpha)), int(bool(force_alpha)), int(bool(y_flip)), C.byref(has_alpha), C.byref(below)), "k_prepare_source")
    return bool(has_alpha.value), bool(below.value)


def renormalize_resident(ctx, d_raster, w, h, pitch=None):
    """image::renormalize_normal_map in place on a resident raster (the mip levels of mip_renormalize); no synchronisation"""
    import ctypes as C
    ctx.check(ctx.lib.k_renormalize_normal_map(ctx.h, C.c_void_p(d_raster), w, h, pitch or w * 4), "k_renormalize_normal_map")


def split_alpha_resident(ctx, d_raster, w, h, d_rgb, d_alpha, pitch=None, rgb_pitch=None, alpha_pitch=None):
    """(r, g, b, 255) -> d_rgb (may be d_raster) and (a, a, a, 255) -> d_alpha: the two ETC1S slices of a level with alpha; no synchronisation"""
    import ctypes as C
    ctx.check(ctx.lib.k_split_alpha(ctx.h, C.c_void_p(d_raster), w, h, pitch or w * 4, C.c_void_p(d_rgb), rgb_pitch or w * 4, C.c_void_p(d_alpha), alpha_pitch or w * 4), "k_split_alpha")


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
