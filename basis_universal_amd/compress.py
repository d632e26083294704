"""One call from an image to a file: the C-style entry of the reference (`basis_compress`, encoder/basisu_comp.cpp:5561-5900 ->
basis_compressor::process, comp.cpp:619-1040) for the two hot paths of this package, every stage in its MI355X-native form:

    raster in HBM -> source-image options (source_prep_kernels.hip; source.py) -> mip levels (mipmap_kernels.hip; the caller's own or a .dds file's: mip_levels_kernels.hip) -> 4x4 tiles of every slice in one launch (bu_hip_k_extract_slices)
      ETC1S : resident frontend (etc1s.Etc1sFrontend) -> host backend (backend.Etc1sBackend) -> .basis / .ktx2
      UASTC : encode_uastc kernels (-> uastc_rdo kernels) -> .basis / .ktx2 (KTX2_SS_NONE: what the reference's library default,
              comp.h:323, and `basisu -ktx2_no_zstandard` write; Zstandard supercompression of the levels is not part of this package)

There is one pipeline: a single image is a sequence of one. Several source images per call -- texture arrays, cubemaps, video, volumes (`-tex_type`) -- take the source and
mip stages per image; all their slices are tiled into one tile array and go through one frontend / backend run.
The result is the file the reference command line tool writes for the same options (tests/test_gpu_backend.py, test_gpu_mipmap.py,
test_gpu_compress_multi_image.py), given the same key-values. No stage has a CPU implementation here: without the HIP libraries and a GPU the context cannot be created."""
import struct

import numpy as np

from . import mipmap, source as _source, uastc as _uastc
from .backend import Etc1sBackend, default_params, uastc_basis_file, uastc_ktx2_file
from .etc1s import Etc1sFrontend, quality_to_clusters


def unified_quality_effort(uastc, quality=-1, effort=-1):
    """basis_compressor_params::set_format_mode_and_quality_effort (comp.cpp:76-92, 158-205; `basisu -quality Q -effort E`) for the two LDR formats here.
    quality in [1, 100] (-1: leave the default), effort in [0, 10] (-1: default). Returns the low-level settings as keyword arguments of compress():
      ETC1S : quality = round(255 q / 100), comp_level = round(6 e / 10)                       (std::round: halves away from zero)
      UASTC : uastc_level = round(4 e / 10); quality < 100 switches the RDO post-pass on with lambda = 20 (1 - q/100)^1.3 in binary32
              (uastc_ldr_4x4_lambda_from_quality, comp.cpp:54-63), quality 100 switches it off."""
    def rnd(x):
        return int(np.floor(np.float32(x) + np.float32(0.5)))
    if quality > 0:
        quality = min(max(int(quality), 0), 100)
    if effort > 0:
        effort = min(max(int(effort), 0), 10)
    fq = np.float32(min(max(np.float32(quality) / np.float32(100.0), np.float32(0)), np.float32(1))) if quality >= 0 else np.float32(0)
    fe = np.float32(min(max(np.float32(effort) / np.float32(10.0), np.float32(0)), np.float32(1))) if effort >= 0 else np.float32(0)
    lerp = lambda a, b, c: np.float32(a) + (np.float32(b) - np.float32(a)) * np.float32(c)       # basisu::lerp, enc.h
    if not uastc:
        out = {}
        if quality >= 0:
            out["quality"] = rnd(lerp(0, 255.0, fq))
        out["comp_level"] = rnd(lerp(0, 6.0, fe)) if effort >= 0 else 2      # BASISU_DEFAULT_ETC1S_COMPRESSION_LEVEL (the library default; the CLI's is 1)
        return out
    out = {"uastc": True, "uastc_level": rnd(lerp(0, 4.0, fe)) if effort >= 0 else _uastc.LEVEL_DEFAULT, "uastc_rdo_lambda": None}
    if 0 <= quality < 100:
        # `pow(1.0f - q, 1.3f)` is the binary32 overload; the correctly rounded double power rounded once more agrees with glibc's powf for every
        # quality 0..99 (tests/test_host_logic.py holds all hundred to the reference's own values)
        out["uastc_rdo_lambda"] = float(np.float32(20.0) * np.float32(float(np.float32(1.0) - fq) ** float(np.float32(1.3)))) if fq < 1 else 0.0
    return out


def compress(ctx, image, *, uastc=False, quality=128, comp_level=1, uastc_level=_uastc.LEVEL_DEFAULT, uastc_rdo_lambda=None, uastc_rdo_jobs=1, mipmaps=False,
             ktx2=False, srgb=True, key_values=(), max_threads=0, stats=None, stats_hvs=False, stats_bc7=False, stats_ssim=False,
             renormalize=False, swizzle=None, check_for_alpha=True, force_alpha=False, y_flip=False, resample=None,
             mip_filter="kaiser", mip_scale=1.0, mip_wrapping=True, mip_srgb=None, mip_renormalize=False, mip_fast=True, mip_smallest_dimension=1,
             no_selector_rdo=False, no_endpoint_rdo=False, tex_type="2d", us_per_frame=0, userdata=(0, 0), ktx2_animdata=(1, 15, 0), mip_levels=None):
    """image: (h, w, 4) uint8 RGBA, or a sequence of such arrays (below). Returns the file as a uint8 array.
    ETC1S: quality 1-255 (`-q`), comp_level 0-6 (`-comp_level`). UASTC: uastc_level 0-4, uastc_rdo_lambda (`-uastc_rdo_l`; None = no post-pass, any float
    incl. 0.0 = post-pass on, as m_rdo_uastc_ldr_4x4 + its scalar), uastc_rdo_jobs = the strips of the post-pass (the reference: min(4, pool threads) when
    multithreaded, else 1; comp.cpp:2078). The post-pass works per slice, as the reference's does, and is ONE uastc.uastc_rdo_slices call for all slices of the file:
    the strips of every image and level walk side by side. `**unified_quality_effort(...)` gives the settings of `-quality` / `-effort`.
    max_threads: the reference's codebook-thread configuration (0 / 1 = `-no_multithreading`; T > 1 = the T-way partitioned codebook build its
    multi-threaded default takes from 262,144 distinct training vectors up, enc.h:2086-2215: etc1s.reference_max_threads() gives the T a host would use).
    mipmaps: the compressor's defaults (Kaiser, sRGB-aware, wrapping, down to 1x1). srgb: perceptual metrics + sRGB transfer function flag.
    stats: a list to be filled with the reference's per-slice quality stats of the file (m_compute_stats; stats.file_stats) against the level rasters and split
    planes that are resident here anyway; None = the stage does not run: the call's launches and bytes are what they are without it.
    stats_hvs: with stats, every slice dict gains "hvs" (PSNR-HVS / PSNR-HVS-M, stats.psnr_hvs: the reference's m_psnr_hvs_m_stats).
    stats_bc7: with stats and uastc, every slice dict gains "bc7", the same stats against the slice's BC7 transcode (stats.file_stats's bc7); without uastc it raises
    ValueError before any work: the ETC1S transcoder here has no BC7 target.
    stats_ssim: with stats, every slice dict (and with stats_bc7 its "bc7" dict) gains "ssim", the seven figures of `basisu -compare_ssim` (stats.ssim).
    The source-image options of basis_compressor::read_source_images (comp.cpp:2569-2697), applied on the device in the reference's order before anything else; every
    default is today's behaviour, and with all of them at their defaults the prepare kernel is not launched (source.normal_map_options() gives `-normal_map`):
      renormalize (`-renorm`): image::renormalize_normal_map.  swizzle (`-swizzle`): four of "rgba" or four ints 0..3; "rrrg" is `-separate_rg_to_color_alpha`.
      check_for_alpha=False (`-no_alpha`): alpha becomes 255.  force_alpha (`-force_alpha`): the file has alpha whatever the pixels say; it wins over
      check_for_alpha=False, as in the reference. A swizzle that moves another channel into alpha forces alpha too.
      y_flip (`-y_flip`): rows reversed, and the .basis header's Y-flipped flag set (basisu_file::init); a .ktx2 records nothing about it, as the reference's does not.
      resample (`-resample W H` / `-resample_factor F`): (w, h), or a float factor (ceilf(w * F), at least 1); box filter, `srgb` picks its transfer function.
    has_alpha is decided on the prepared raster, on the device, before the resample. The mip levels are made from the prepared image:
      mip_filter (`-mip_filter`: box, tent, bell, mitchell, blackman, lanczos3/4/6/12, kaiser, catmullrom), mip_scale (`-mip_scale`), mip_wrapping=False (`-mip_clamp`),
      mip_srgb (None = follows srgb; False = `-mip_linear`), mip_renormalize (`-mip_renorm`: every level renormalised after it is made), mip_fast=False (`-mip_slow`:
      every level from level 0 instead of the level above), mip_smallest_dimension (`-mip_smallest`).
    no_selector_rdo / no_endpoint_rdo (ETC1S): the backend's threshold stays 0 (comp.cpp:3536-3540).
    A bad swizzle, filter name, scale or size raises ValueError before ctx is touched.
    Several images in one file (basis_compressor::read_source_images with more than one source, comp.cpp:2773-3044): `image` is a sequence of (h, w, 4) arrays and
      tex_type (`-tex_type`) says what they are: "2darray" (a layer each), "cubemap" (six consecutive images are the faces of a layer), "video" (frames) or "volume"
      (`-tex_type 3d`); "2d" takes exactly one image -- the tool compresses several 2D images as separate files, which here is a call each.
      Every source option above applies to every image and each image gets its own mip chain. The slices go source image outermost, then level, then (ETC1S with
      alpha) colour and alpha, into one tile array: one codebook pair for the whole file. The file has alpha when ANY prepared image has (or force_alpha): an ETC1S
      file then carries an alpha slice for every image; a UASTC slice carries its own image's flag. Video: ETC1S runs the frontend and the backend in video mode with
      the slices of image 0 as i-frames; every UASTC slice is an i-frame.
      us_per_frame (`-framerate`, as microseconds; .basis header, at most 0xFFFFFF as basisu_file::init clamps it), userdata (`-userdata0`, `-userdata1`; .basis header).
      ktx2_animdata = (duration, timescale, loop count) (`-ktx2_animdata_*`): a video .ktx2 gains the KTXanimData key/value the tool adds (basisu_tool.cpp:2382-2401),
      unless key_values already holds that key.
      stats: one dict per slice in slice order; ETC1S video with stats raises ValueError before any work (the ETC1S reader does not read video files).
      ValueError before ctx is touched: several images with tex_type "2d", a cubemap whose image count is not a multiple of 6, images of different sizes (after
      `resample`) in anything but "2d", more slices than BASISU_MAX_SLICES, an empty sequence.
    A single array is a sequence of one: the same stages, the same launches, the same bytes.
    mip_levels: the levels below level 0 as the caller made them (basis_compressor_params::m_source_mipmap_images, comp.cpp:2737-2818) -- for a bare image a sequence
      of (h, w, 4) uint8 arrays, levels 1..n; for a sequence of images one such sequence per image. Level k is max(1, w >> k) x max(1, h >> k) pixels; a chain may stop
      early. None, an empty sequence or empty sequences throughout: the call is what it is without the argument, and nothing new is launched. Supplied levels win over
      `mipmaps` (the reference generates only where none are given, comp.cpp:2849), and of the source options only `swizzle` touches them (comp.cpp:2796-2817):
      renormalize, y_flip and the alpha policy are level 0's. All levels of all images go up as one payload and become rasters in ONE launch (source.resident_levels).
      has_alpha is level 0's answer OR any supplied level with an alpha value that is not 255 after the swizzle (comp.cpp:2746-2766) -- so with check_for_alpha=False,
      which clears level 0 only, alpha in a lower level still gives an ETC1S file alpha slices for every level; a UASTC slice carries its own level's flag. `stats`
      compares level k with the supplied level k.
      ValueError before ctx is touched: a level of another size, more levels than the full chain, chains of unequal length, a flat sequence where one per image is
      needed or the reverse, a level that is not an (h, w, 4) uint8 array, `resample` together with mip_levels, too many slices.
    dds.compress_dds gives the same for .dds sources (image is then a source.DdsSources and mip_levels must stay None)."""
    if stats_bc7 and not uastc:
        from .stats import BC7_REFUSAL
        raise ValueError(BC7_REFUSAL)
    dds = image if isinstance(image, _source.DdsSources) else None
    if dds is not None:
        if mip_levels is not None:
            raise ValueError("mip_levels with .dds sources: the levels below level 0 are the file's")
        bare, (images, levels) = dds.bare, dds.arrays()
    else:
        bare = not (isinstance(image, (list, tuple)) and (not len(image) or np.ndim(image[0]) == 3) or (isinstance(image, np.ndarray) and image.ndim == 4))
        images = [image] if bare else list(image)
        levels = _mip_level_arrays(mip_levels, len(images), bare)
    prepare_options = dict(renormalize=renormalize, swizzle=swizzle, check_for_alpha=check_for_alpha, force_alpha=force_alpha, y_flip=y_flip)
    imgs, level_sizes, type_index, host_alpha, key_values = _checked(
        images, bare, prepare_options, uastc=uastc, mipmaps=mipmaps, ktx2=ktx2, key_values=key_values, stats=stats, resample=resample,
        mip_filter=mip_filter, mip_scale=mip_scale, mip_smallest_dimension=mip_smallest_dimension, tex_type=tex_type, us_per_frame=us_per_frame, userdata=userdata,
        ktx2_animdata=ktx2_animdata, mip_levels=levels, host_alpha=dds is None)
    owned = []
    try:
        if dds is not None:
            level0, image_alpha, has_alpha, lower, level_alpha = _resident_dds(ctx, owned, dds, level_sizes, prepare_options, resample=resample, srgb=srgb)
        else:
            level0, image_alpha, has_alpha = _resident_level0(ctx, owned, imgs, level_sizes, host_alpha, prepare_options, resample=resample, srgb=srgb)
            lower, level_alpha = _resident_supplied_levels(ctx, owned, levels, swizzle) if levels is not None else (None, None)
        if lower is not None:   # comp.cpp:2746-2766: any supplied level with alpha gives the file alpha; a UASTC slice is marked by its own pixels (comp.cpp:2932)
            has_alpha = has_alpha or any(any(flags) for flags in level_alpha)
            image_alpha = [[own, *flags] for own, flags in zip(image_alpha, level_alpha)]
        _source.check_slice_count(len(imgs), len(level_sizes[0]), has_alpha and not uastc)
        if lower is not None:
            rasters = [[d, *below] for d, below in zip(level0, lower)]
        else:
            # each image's own chain (generate_mipmaps with m_any_source_image_has_alpha: four components for every image when any has alpha)
            rasters = [mipmap.resident_chain(ctx, owned, d, sizes, srgb=srgb if mip_srgb is None else mip_srgb, filter=mip_filter, filter_scale=mip_scale, wrapping=mip_wrapping,
                                             num_comps=4 if has_alpha else 3, fast=mip_fast, renormalize=mip_renormalize) for d, sizes in zip(level0, level_sizes)]
        d_all, slices, planes = _tiles(ctx, owned, rasters, level_sizes, tex_type=tex_type, uastc=uastc, has_alpha=has_alpha, image_alpha=image_alpha,
                                       video=tex_type == "video", with_planes=stats is not None)
        data = _encode(ctx, owned, d_all, slices, has_alpha, uastc=uastc, quality=quality, comp_level=comp_level, uastc_level=uastc_level, uastc_rdo_lambda=uastc_rdo_lambda,
                       uastc_rdo_jobs=uastc_rdo_jobs, ktx2=ktx2, srgb=srgb, key_values=key_values, max_threads=max_threads, y_flip=y_flip, no_selector_rdo=no_selector_rdo,
                       no_endpoint_rdo=no_endpoint_rdo, tex_type=type_index, us_per_frame=us_per_frame, userdata=userdata)
        if stats is not None:   # m_compute_stats (comp.cpp:4195-4253) while the sources are still resident
            from . import stats as _stats
            stats.extend(_stats._stats_from_slices(ctx, bytes(data), lambda level, layer, face, n_slices: planes[(level, layer, face)], hvs=stats_hvs, bc7=stats_bc7,
                                                   ssim=stats_ssim))
        return data
    finally:
        for d in owned:
            ctx.free(d)


VIDEO_STATS_REFUSAL = ("stats of an ETC1S video file: video files are not supported: a P-frame's blocks may repeat the previous frame's indices, which this reader "
                       "does not keep (csrc/host/etc1s_decode.cpp)")


def _mip_level_arrays(mip_levels, n_images, bare):
    """compress()'s mip_levels -> per image the list of its levels as (h, w, 4) uint8 arrays, or None where there are none (None, empty, or empty for every image).
    ValueError for a flat sequence where one per image is needed or the reverse, a count that is not the images', and for what is no (h, w, 4) uint8 array."""
    if mip_levels is None or not len(mip_levels):
        return None

    def is_level(x):
        return isinstance(x, np.ndarray) and x.ndim <= 3

    if bare:
        if not all(is_level(x) for x in mip_levels):
            raise ValueError("mip_levels of a single image is a flat sequence of (h, w, 4) uint8 arrays, levels 1..n; a sequence per image goes with a sequence of images")
        chains = [list(mip_levels)]
    else:
        if any(is_level(x) for x in mip_levels):
            raise ValueError("mip_levels of a sequence of images is one sequence of levels per image (nested), not a flat sequence of arrays")
        if len(mip_levels) != n_images:
            raise ValueError(f"mip_levels holds the levels of {len(mip_levels)} images, and there are {n_images} images")
        chains = [list(chain) for chain in mip_levels]
    for k, chain in enumerate(chains):
        for i, level in enumerate(chain, 1):
            if not isinstance(level, np.ndarray) or level.dtype != np.uint8 or level.ndim != 3 or level.shape[2] != 4:
                what = f"{level.dtype} {level.shape}" if isinstance(level, np.ndarray) else type(level).__name__
                raise ValueError(f"mip level {i}{'' if bare else f' of image {k}'} must be an (h, w, 4) uint8 array, not {what}")
    if not any(chains):
        return None
    return [[np.ascontiguousarray(level) for level in chain] for chain in chains]


def _checked(images, bare, prepare_options, *, uastc, mipmaps, ktx2, key_values, stats, resample, mip_filter, mip_scale, mip_smallest_dimension, tex_type, us_per_frame,
             userdata, ktx2_animdata, mip_levels=None, host_alpha=True):
    """Everything that can be refused, before ctx is touched. -> the images as uint8 arrays, per image the (width, height) of its levels (level 0: after `resample`), the
    basis_texture_type number, per image image::has_alpha decided on the host (None where the prepare kernel decides it, or without `host_alpha`), and key_values with a
    video .ktx2's KTXanimData. mip_levels: None, or per image its supplied levels as arrays (_mip_level_arrays): their sizes are then the levels' sizes."""
    imgs = []
    for k, image in enumerate(images):
        name = "image" if bare else f"image {k}"
        img = np.ascontiguousarray(image, np.uint8)
        if img.ndim != 3 or img.shape[2] != 4:
            raise ValueError(f"{name} must be (h, w, 4) uint8")
        h, w = img.shape[:2]
        if not w or not h or w > _source.MAX_DIMENSION or h > _source.MAX_DIMENSION:
            raise ValueError(f"{name} of {w} x {h} pixels: 1..{_source.MAX_DIMENSION} each way")
        imgs.append(img)
    prepare = not _source.is_identity(**prepare_options)   # parses the swizzle: ValueError
    _source.check_mip_options(mip_filter, mip_scale, mip_smallest_dimension)
    sizes = [_source.resampled_size(img.shape[1], img.shape[0], resample) or (img.shape[1], img.shape[0]) for img in imgs]
    type_index = _source.check_texture_type(tex_type, sizes)
    video = tex_type == "video"
    if video and not uastc and stats is not None:
        raise ValueError(VIDEO_STATS_REFUSAL)
    if len(tuple(userdata)) != 2 or len(tuple(ktx2_animdata)) != 3 or any(not 0 <= int(v) < 2 ** 32 for v in (*userdata, *ktx2_animdata, us_per_frame)):
        raise ValueError("userdata is two, ktx2_animdata three and us_per_frame one unsigned 32-bit value")
    if mip_levels is not None:
        if resample is not None:
            raise ValueError("resample together with mip_levels: the supplied levels are halvings of the source's size and the reference resamples level 0 only "
                             "(its file would hold levels that do not follow from level 0); resample the levels yourself, or let compress() generate them")
        if any(len(chain) != len(mip_levels[0]) for chain in mip_levels):
            raise ValueError(f"the images' mip chains are of unequal length ({', '.join(str(len(chain)) for chain in mip_levels)} levels): every image of a file "
                             "has the same levels")
        for k, (size, chain) in enumerate(zip(sizes, mip_levels)):
            _source.check_supplied_levels("image" if bare else f"image {k}", size[0], size[1], [(level.shape[1], level.shape[0]) for level in chain])
        level_sizes = [[size] + [(level.shape[1], level.shape[0]) for level in chain] for size, chain in zip(sizes, mip_levels)]
    else:
        level_sizes = [[size] + (mipmap.level_sizes(size[0], size[1], int(mip_smallest_dimension)) if mipmaps else []) for size in sizes]
    host_alpha = [bool((img[..., 3] != 255).any()) for img in imgs] if not prepare and host_alpha else None      # image::has_alpha of an image that is not prepared
    # the alpha slices double the count; where only the device can say whether there are any (the prepare kernel's flag), the count is checked again once it has
    alpha_known = bool(prepare_options["force_alpha"]) or (host_alpha is not None and any(host_alpha))
    _source.check_slice_count(len(imgs), len(level_sizes[0]), not uastc and alpha_known)
    if video and ktx2 and not any(k == "KTXanimData" for k, _ in key_values):   # basisu_tool.cpp:2382-2401: three little-endian 32-bit words
        key_values = list(key_values) + [("KTXanimData", struct.pack("<III", *(int(v) for v in ktx2_animdata)))]
    return imgs, level_sizes, type_index, host_alpha, key_values


def _resident_level0(ctx, owned, imgs, level_sizes, host_alpha, prepare_options, *, resample, srgb):
    """Every source image resident, prepared and resampled -> (level-0 rasters, per image image::has_alpha of the prepared raster, m_any_source_image_has_alpha)."""
    level0, image_alpha, has_alpha = [], [], False
    for k, img in enumerate(imgs):
        h, w = img.shape[:2]
        d_src = ctx.upload(img)
        owned.append(d_src)
        d_level0, one_has, one_any = _prepared(ctx, owned, d_src, w, h, None if host_alpha is None else host_alpha[k], prepare_options, resample=resample,
                                               new_size=level_sizes[k][0], srgb=srgb)
        level0.append(d_level0)
        image_alpha.append(one_any)
        has_alpha = has_alpha or one_has
    return level0, image_alpha, has_alpha


def _prepared(ctx, owned, d_src, w, h, alpha, prepare_options, *, resample, new_size, srgb):
    """One resident source image (ours: prepared in place) -> (its level-0 raster, has_alpha, any prepared alpha below 255). alpha: image::has_alpha of an image that
    needs no preparing, None where the prepare kernel runs and decides it."""
    d_level0 = d_src
    if alpha is None:
        if prepare_options["y_flip"]:                                 # the flip reads another row than it writes: not in place
            d_level0 = ctx.alloc(w * h * 4)
            owned.append(d_level0)
        one_has, one_any = _source.prepare_resident(ctx, d_src, w, h, d_level0, **prepare_options)
    else:
        one_has = one_any = alpha
    if resample is not None:   # has_alpha is decided before the resample, as the reference decides it
        d_level0 = _source.resample_resident(ctx, d_level0, w, h, *new_size, srgb)
        owned.append(d_level0)
    return d_level0, one_has, one_any


def _resident_supplied_levels(ctx, owned, levels, swizzle):
    """The supplied levels of every image as one payload, one launch -> (per image its level rasters, per image the levels' alpha flags)"""
    parts = [level.reshape(-1) for chain in levels for level in chain]
    selector = _source.level_selector("rgba", swizzle)
    rasters, flags = _source.resident_levels(ctx, owned, parts, [(i, 0, level.shape[1], level.shape[0], selector) for i, level in enumerate(lv for chain in levels for lv in chain)])
    n = len(levels[0])
    return [rasters[k * n:(k + 1) * n] for k in range(len(levels))], [flags[k * n:(k + 1) * n] for k in range(len(levels))]


def _resident_dds(ctx, owned, dds, level_sizes, prepare_options, *, resample, srgb):
    """.dds sources: every file's payload uploaded once and ONE launch for level 0's byte order and the lower levels; level 0 then goes through the source options as an
    image does. -> (level-0 rasters, per image any alpha below 255, has_alpha, per image the lower levels' rasters or None, their flags or None)"""
    identity = _source.is_identity(**prepare_options)
    level0, image_alpha, has_alpha, lower, level_alpha = [], [], False, [], []
    for k, ((rasters, flags), f) in enumerate(zip(dds.resident(ctx, owned, prepare_options["swizzle"]), dds.files)):
        d_level0, one_has, one_any = _prepared(ctx, owned, rasters[0], f["width"], f["height"], flags[0] if identity else None, prepare_options, resample=resample,
                                               new_size=level_sizes[k][0], srgb=srgb)
        level0.append(d_level0)
        image_alpha.append(one_any)
        has_alpha = has_alpha or one_has
        lower.append(rasters[1:])
        level_alpha.append(flags[1:])
    if not any(lower):
        lower = level_alpha = None
    return level0, image_alpha, has_alpha, lower, level_alpha


def _tiles(ctx, owned, rasters, level_sizes, *, tex_type, uastc, has_alpha, image_alpha, video, with_planes):
    """The slice table and the tiles of every slice by ONE launch -> (resident tile array, slices, {(level, layer, face): the resident source of each of its slices}; the
    last only with_planes, for the stats stage, which reads planes: ETC1S alpha is then split into planes and the tiles are cut from those)."""
    slices, sources = _source.slice_table(level_sizes, uastc=uastc, any_alpha=has_alpha, image_alpha=image_alpha, video=video)
    d_all = ctx.alloc(sum(s[1] * s[2] for s in slices) * 64)   # one contiguous tile array: every image, level and alpha slice shares the codebooks
    owned.append(d_all)
    split_alpha = has_alpha and not uastc
    planes = {}
    if with_planes:
        for k, (chain, levels) in enumerate(zip(rasters, level_sizes)):
            for level, (d_raster, (lw, lh)) in enumerate(zip(chain, levels)):
                one = [d_raster]
                if split_alpha:            # (r, g, b, 255) in the level's own buffer -- every level is made already -- and (a, a, a, 255) beside it
                    one.append(ctx.alloc(lw * lh * 4))
                    owned.append(one[1])
                    _source.split_alpha_resident(ctx, d_raster, lw, lh, one[0], one[1])
                planes[(level, *_source.image_layer_face(tex_type, k))] = [(d, lw, lh, lw) for d in one]
    entries = []
    for s, (k, level, mode) in zip(slices, sources):
        if with_planes and split_alpha:
            d_raster, mode = planes[(level, *_source.image_layer_face(tex_type, k))][mode == _source.SLICE_ALPHA][0], _source.SLICE_AS_IS
        else:
            d_raster = rasters[k][level]
        entries.append((d_raster, s[3], s[4], 0, mode, s[0]))
    _source.extract_slices_resident(ctx, entries, d_all)
    return d_all, slices, planes


def _encode(ctx, owned, d_all, slices, has_alpha, *, uastc, quality, comp_level, uastc_level, uastc_rdo_lambda, uastc_rdo_jobs, ktx2, srgb, key_values, max_threads, y_flip,
            no_selector_rdo, no_endpoint_rdo, tex_type, us_per_frame, userdata):
    """resident tiles of every slice -> the file"""
    video = tex_type == 3
    header = dict(tex_type=tex_type, userdata0=int(userdata[0]), userdata1=int(userdata[1]), y_flipped=bool(y_flip), us_per_frame=int(us_per_frame), key_values=key_values)
    slice_blocks = [s[1] * s[2] for s in slices]
    total_blocks = sum(slice_blocks)
    if uastc:
        rdo = uastc_rdo_lambda is not None and uastc_rdo_lambda is not False
        flags = int(uastc_level) | (_uastc.FAVOR_SIMPLER_MODES if rdo else 0)       # comp.cpp:2016-2018
        d_out = ctx.alloc(total_blocks * 16)
        owned.append(d_out)
        _uastc.encode_uastc_blocks(ctx, d_all, flags, n_blocks=total_blocks, out_device=d_out)
        if rdo:
            # the post-pass works per slice (comp.cpp:2066-2082): one call, every slice's strips side by side
            _uastc.uastc_rdo_slices(ctx, d_out, d_all, slice_blocks, _uastc.RdoParams(m_lambda=float(uastc_rdo_lambda)), int(uastc_level), uastc_rdo_jobs)
        packed = ctx.download(d_out, (total_blocks, 16), np.uint8)
        if ktx2:
            return uastc_ktx2_file(packed, slices, srgb=srgb, tex_type=tex_type, has_alpha=has_alpha, key_values=key_values)
        # encode_slices_to_uastc_4x4_ldr (comp.cpp:1973-1985) never sets basisu_backend_output::m_srgb, which basisu_backend_output::clear() leaves true
        # (backend.h:243): the reference's UASTC .basis files carry the sRGB header flag whatever -linear says (the .ktx2 DFD does follow the option)
        return uastc_basis_file(packed, slices, srgb=True, **header)
    max_ep, max_sel = quality_to_clusters(quality, total_blocks)
    fe = Etc1sFrontend(ctx, max_threads=max_threads, video=video)
    try:
        fe.init(d_all, max_ep, max_sel, comp_level, srgb, n_blocks=total_blocks)
        fe.compress()
        ept, selt = default_params(quality, comp_level)
        ept, selt = (0.0 if no_endpoint_rdo else ept), (0.0 if no_selector_rdo else selt)   # comp.cpp:3536-3540
        be = Etc1sBackend.from_frontend(fe, slices, ept, selt, comp_level, video=video)
        try:
            be.encode()
            if ktx2:
                return be.ktx2_file(tex_type=tex_type, has_alpha=has_alpha, key_values=key_values)
            return be.basis_file(**header)
        finally:
            be.close()
    finally:
        fe.close()
