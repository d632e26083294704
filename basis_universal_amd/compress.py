"""One call from an image to a file: the C-style entry of the reference (`basis_compress`, encoder/basisu_comp.cpp:5561-5900 ->
basis_compressor::process, comp.cpp:619-1040) for the two hot paths of this package, every stage in its MI355X-native form:

    raster in HBM -> source-image options (source_prep_kernels.hip; source.py) -> mip levels (mipmap_kernels.hip) -> 4x4 tiles (k_extract_blocks)
      ETC1S : resident frontend (etc1s.Etc1sFrontend) -> host backend (backend.Etc1sBackend) -> .basis / .ktx2
      UASTC : encode_uastc kernels (-> uastc_rdo kernels) -> .basis / .ktx2 (KTX2_SS_NONE: what the reference's library default,
              comp.h:323, and `basisu -ktx2_no_zstandard` write; Zstandard supercompression of the levels is not part of this package)

The result is the file the reference command line tool writes for the same options (tests/test_gpu_backend.py, test_gpu_mipmap.py), given the
same key-values. No stage has a CPU implementation here: without the HIP libraries and a GPU the context cannot be created."""
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
             no_selector_rdo=False, no_endpoint_rdo=False):
    """image: (h, w, 4) uint8 RGBA. Returns the file as a uint8 array.
    ETC1S: quality 1-255 (`-q`), comp_level 0-6 (`-comp_level`). UASTC: uastc_level 0-4, uastc_rdo_lambda (`-uastc_rdo_l`; None = no post-pass, any float
    incl. 0.0 = post-pass on, as m_rdo_uastc_ldr_4x4 + its scalar), uastc_rdo_jobs = the strips of the post-pass (the reference: min(4, pool threads) when
    multithreaded, else 1; comp.cpp:2078). `**unified_quality_effort(...)` gives the settings of `-quality` / `-effort`.
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
    A bad swizzle, filter name, scale or size raises ValueError before ctx is touched."""
    if stats_bc7 and not uastc:
        from .stats import BC7_REFUSAL
        raise ValueError(BC7_REFUSAL)
    img = np.ascontiguousarray(image, np.uint8)
    if img.ndim != 3 or img.shape[2] != 4:
        raise ValueError("image must be (h, w, 4) uint8")
    h, w = img.shape[:2]
    if not w or not h or w > _source.MAX_DIMENSION or h > _source.MAX_DIMENSION:
        raise ValueError(f"image of {w} x {h} pixels: 1..{_source.MAX_DIMENSION} each way")
    prepare = not _source.is_identity(renormalize, swizzle, check_for_alpha, force_alpha, y_flip)   # parses the swizzle: ValueError
    _source.check_mip_options(mip_filter, mip_scale, mip_smallest_dimension)
    new_size = _source.resampled_size(w, h, resample)
    mip_srgb = srgb if mip_srgb is None else mip_srgb
    owned = []
    try:
        # ---- the source image, resident and prepared
        d_src = ctx.upload(img)
        owned.append(d_src)
        if prepare:
            d_level0 = d_src
            if y_flip:                                                    # the flip reads another row than it writes: not in place
                d_level0 = ctx.alloc(w * h * 4)
                owned.append(d_level0)
            # has_alpha -> m_any_source_image_has_alpha; any_alpha = image::has_alpha of the prepared raster
            has_alpha, any_alpha = _source.prepare_resident(ctx, d_src, w, h, d_level0, renormalize=renormalize, swizzle=swizzle, check_for_alpha=check_for_alpha,
                                                            force_alpha=force_alpha, y_flip=y_flip)
        else:
            d_level0 = d_src
            has_alpha = any_alpha = bool((img[..., 3] != 255).any())      # image::has_alpha -> m_any_source_image_has_alpha
        if new_size is not None:
            d_level0 = _source.resample_resident(ctx, d_level0, w, h, new_size[0], new_size[1], srgb)
            owned.append(d_level0)
            w, h = new_size
        # ---- the levels, resident
        sizes = [(w, h)] + (mipmap.level_sizes(w, h, int(mip_smallest_dimension)) if mipmaps else [])
        rasters = [d_level0]
        for lw, lh in sizes[1:]:
            d = ctx.alloc(lw * lh * 4)
            owned.append(d)
            at = len(rasters) - 1 if mip_fast else 0                      # m_mip_fast: from the level above; else every level from level 0
            sw, sh = sizes[at]
            ctx.check(mipmap._lib().bu_generate_mipmap_level(ctx.h, rasters[at], sw, sh, d, lw, lh, int(bool(mip_srgb)), mip_filter.encode(), float(mip_scale),
                                                             int(bool(mip_wrapping)), 4 if has_alpha else 3), "bu_generate_mipmap_level")
            if mip_renormalize:
                _source.renormalize_resident(ctx, d, lw, lh)
            rasters.append(d)
        # ---- the slices: one per level, for ETC1S with alpha a colour slice and an (a, a, a) slice per level (comp.cpp:2880-2910)
        split_alpha = has_alpha and not uastc
        per_level = [((lw + 3) // 4) * ((lh + 3) // 4) for lw, lh in sizes]
        total_blocks = sum(per_level) * (2 if split_alpha else 1)
        d_all = ctx.alloc(total_blocks * 64)   # one contiguous tile array: the levels (and the alpha slices) share the codebooks
        owned.append(d_all)
        slices, slice_blocks, first, level_planes = [], [], 0, []
        for mip, ((lw, lh), d_raster) in enumerate(zip(sizes, rasters)):
            nbx, nby = (lw + 3) // 4, (lh + 3) // 4
            if split_alpha:   # (r, g, b, 255) in the level's own buffer -- every level below it is made already -- and (a, a, a, 255) beside it
                planes = [d_raster, ctx.alloc(lw * lh * 4)]
                owned.append(planes[1])
                _source.split_alpha_resident(ctx, d_raster, lw, lh, planes[0], planes[1])
            else:
                planes = [d_raster]
            level_planes.append([(d_plane, lw, lh, lw) for d_plane in planes])
            for k, d_plane in enumerate(planes):   # basis_compressor::extract_source_blocks on the resident plane, straight into its place
                ctx.check(ctx.lib.k_extract_blocks(ctx.h, d_plane, lw, lh, lw * 4, d_all + first * 64), "k_extract_blocks")
                # the slice's alpha flag: ETC1S the alpha plane; UASTC image::has_alpha of the slice (comp.cpp:2928-2937), known for the prepared raster
                slices.append((first, nbx, nby, lw, lh, 0, mip, k if split_alpha else int(has_alpha and any_alpha)))
                slice_blocks.append(nbx * nby)
                first += nbx * nby

        def finish(data):   # m_compute_stats (comp.cpp:4195-4253) while the sources are still resident
            if stats is not None:
                from . import stats as _stats
                stats.extend(_stats._stats_from_slices(ctx, bytes(data), lambda level, layer, face, n_slices: level_planes[level], hvs=stats_hvs, bc7=stats_bc7, ssim=stats_ssim))
            return data
        # ---- encode
        if uastc:
            rdo = uastc_rdo_lambda is not None and uastc_rdo_lambda is not False
            flags = int(uastc_level) | (_uastc.FAVOR_SIMPLER_MODES if rdo else 0)       # comp.cpp:2016-2018
            d_out = ctx.alloc(total_blocks * 16)
            owned.append(d_out)
            _uastc.encode_uastc_blocks(ctx, d_all, flags, n_blocks=total_blocks, out_device=d_out)
            if rdo:
                at = 0
                for n in slice_blocks:   # the post-pass runs per slice (comp.cpp:2066-2082)
                    _uastc.uastc_rdo(ctx, d_out + at * 16, d_all + at * 64, _uastc.RdoParams(m_lambda=float(uastc_rdo_lambda)), int(uastc_level), uastc_rdo_jobs, n_blocks=n)
                    at += n
            packed = ctx.download(d_out, (total_blocks, 16), np.uint8)
            if ktx2:
                return finish(uastc_ktx2_file(packed, slices, srgb=srgb, has_alpha=has_alpha, key_values=key_values))
            # encode_slices_to_uastc_4x4_ldr (comp.cpp:1973-1985) never sets basisu_backend_output::m_srgb, which basisu_backend_output::clear() leaves true
            # (backend.h:243): the reference's UASTC .basis files carry the sRGB header flag whatever -linear says (the .ktx2 DFD does follow the option)
            return finish(uastc_basis_file(packed, slices, srgb=True, y_flipped=bool(y_flip), key_values=key_values))
        max_ep, max_sel = quality_to_clusters(quality, total_blocks)
        fe = Etc1sFrontend(ctx, max_threads=max_threads)
        try:
            fe.init(d_all, max_ep, max_sel, comp_level, srgb, n_blocks=total_blocks)
            fe.compress()
            ept, selt = default_params(quality, comp_level)
            ept, selt = (0.0 if no_endpoint_rdo else ept), (0.0 if no_selector_rdo else selt)   # comp.cpp:3536-3540
            be = Etc1sBackend.from_frontend(fe, slices, ept, selt, comp_level)
            try:
                be.encode()
                return finish(be.ktx2_file(has_alpha=has_alpha, key_values=key_values) if ktx2 else be.basis_file(y_flipped=bool(y_flip), key_values=key_values))
            finally:
                be.close()
        finally:
            fe.close()
    finally:
        for d in owned:
            ctx.free(d)
