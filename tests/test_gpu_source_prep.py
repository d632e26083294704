"""-m gpu: the compressor's source-image options on the device (csrc/source_prep_kernels.hip through bu_hip_k_prepare_source / _renormalize_normal_map / _split_alpha,
basis_universal_amd.source and compress()) against what the reference tool wrote for the same flags (tests/golden/source_prep_vectors.npz, source_prep_digests.json)
and against the g++ build of the same header. Every comparison is equality of bytes."""
import ctypes as C

import numpy as np
import pytest

import helpers
import image_metrics_helpers as M
import source_prep_helpers as H
from basis_universal_amd import source
from basis_universal_amd.compress import compress

pytestmark = pytest.mark.gpu
CASES = H.golden_cases()
IDS = [c["name"] for c in CASES]
GUARD = 0xA5
vp = C.c_void_p


def case_kwargs(case):
    return H.kwargs_from_flags(case["flags"], source.normal_map_options)


# ---------------------------------------------------------------- 1. prepare_source against the tool's prepared level-0 raster

def tool_level0(case):
    slices = H.slices_of(case)
    w, h = case["sizes"][0]
    level0 = np.array(slices[0][:h, :w])
    if not case["uastc"] and case["has_alpha"]:
        level0[..., 3] = slices[1][:h, :w, 0]     # ETC1S: the alpha slice is its own (a, a, a, 255) image
    return level0


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_prepare_source_equals_the_tools_prepared_raster(hip_ctx, case):
    kw = case_kwargs(case)
    options = H.prepare_kwargs(kw)
    if "resample" in kw:
        options.update(resample=kw["resample"], srgb=kw.get("srgb", True))
    d, (w, h), has_alpha = source.prepare_source(hip_ctx, H.source_image(case), **options)
    try:
        got = hip_ctx.download(d, (h, w, 4), np.uint8)
    finally:
        hip_ctx.free(d)
    assert [w, h] == case["sizes"][0] and has_alpha == case["has_alpha"]
    assert (got == tool_level0(case)).all()


def test_prepare_source_leaves_a_resident_source_alone(hip_ctx):
    (case,) = [c for c in CASES if c["name"] == "combo_renorm_flip_rrrg"]
    img = H.source_image(case)
    d_src = hip_ctx.upload(img)
    try:
        d, size, has_alpha = source.prepare_source(hip_ctx, d_src, case["w"], case["h"], **H.prepare_kwargs(case_kwargs(case)))
        try:
            assert size == (case["w"], case["h"]) and has_alpha
            assert (hip_ctx.download(d, img.shape, np.uint8) == tool_level0(case)).all()
        finally:
            hip_ctx.free(d)
        assert (hip_ctx.download(d_src, img.shape, np.uint8) == img).all()
    finally:
        hip_ctx.free(d_src)


def _prepare(ctx, d_src, w, h, src_pitch, d_dst, dst_pitch, renormalize=0, swizzle=0x03020100, check=1, force=0, flip=0):
    has_alpha, below = C.c_uint32(77), C.c_uint32(77)
    r = ctx.lib.k_prepare_source(ctx.h, vp(d_src), w, h, src_pitch, vp(d_dst), dst_pitch, renormalize, swizzle, check, force, flip, C.byref(has_alpha), C.byref(below))
    return r, has_alpha.value, below.value


# 1030 x 37: 258 quads a row (five workgroups across, the last ragged: 1030 = 4 * 257 + 2) and ten workgroups down (37 = 4 * 9 + 1); 21 x 13 and 4 x 1: less than one
GEOMETRY = [(1030, 37), (21, 13), (4, 1), (1, 5)]


@pytest.mark.parametrize("w,h", GEOMETRY)
def test_all_options_with_padded_pitches_equal_the_host_build(hip_ctx, w, h):
    """pitch = width (rows off the 16-byte lines unless the width is a multiple of 4), source and destination pitches padded differently, and a raster that starts 4 bytes
    into a line: the prepared pixels are the host build's, and every byte outside width x height keeps the guard"""
    rng = np.random.default_rng(w * 100 + h)
    img = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    img[rng.random((h, w)) < 0.1, :3] = 128
    img[rng.random((h, w)) < 0.1, :3] = rng.integers(124, 133, 3, dtype=np.uint8)
    for options in (dict(renormalize=True, swizzle="bgra", check_for_alpha=True, y_flip=True), dict(renormalize=True, swizzle="rrrg", y_flip=True),
                    dict(check_for_alpha=False), dict(swizzle="gbra"), dict(renormalize=True)):
        want, want_alpha, want_below = H.host_prepare(img, **options)
        for src_pad, dst_pad, lead in ((0, 0, 0), (3, 1, 0), (1, 2, 1)):
            sp, dp = w + src_pad, w + dst_pad
            src = np.full((lead + h * sp + 5, 4), 0x5A, np.uint8)
            src[lead:lead + h * sp].reshape(h, sp, 4)[:, :w] = img
            fill = np.full((lead + h * dp + 5, 4), GUARD, np.uint8)
            d_src, d_dst = hip_ctx.upload(src), hip_ctx.upload(fill)
            try:
                r = _prepare(hip_ctx, d_src + 4 * lead, w, h, sp * 4, d_dst + 4 * lead, dp * 4, int(options.get("renormalize", False)), H.pack_swizzle(options.get("swizzle")),
                             int(options.get("check_for_alpha", True)), int(options.get("force_alpha", False)), int(options.get("y_flip", False)))
                out = hip_ctx.download(d_dst, fill.shape, np.uint8)
            finally:
                hip_ctx.free(d_src)
                hip_ctx.free(d_dst)
            what = (w, h, options, src_pad, dst_pad, lead)
            assert r == (1, int(want_alpha), int(want_below)), what
            raster = out[lead:lead + h * dp].reshape(h, dp, 4)
            assert (raster[:, :w] == want).all(), what
            assert (raster[:, w:] == GUARD).all() and (out[:lead] == GUARD).all() and (out[lead + h * dp:] == GUARD).all(), what


def test_the_alpha_flag_sees_one_pixel_anywhere(hip_ctx):
    """one alpha value of 254 in the last pixel of a ragged row, in the last row, in the first pixel: each is found; none: not"""
    w, h = 1030, 37
    d = hip_ctx.alloc(w * h * 4)
    try:
        for at in (None, (0, 0), (h - 1, w - 1), (17, w - 1), (h - 1, 0), (20, 515)):
            img = np.full((h, w, 4), 255, np.uint8)
            if at is not None:
                img[at[0], at[1], 3] = 254
            d_src = hip_ctx.upload(img)
            try:
                assert _prepare(hip_ctx, d_src, w, h, w * 4, d, w * 4) == (1, int(at is not None), int(at is not None)), at
                assert _prepare(hip_ctx, d_src, w, h, w * 4, d, w * 4, check=0) == (1, 0, 0), at            # -no_alpha: overwritten, so nothing is below 255
                assert _prepare(hip_ctx, d_src, w, h, w * 4, d, w * 4, check=0, force=1) == (1, 1, int(at is not None)), at
                assert _prepare(hip_ctx, d_src, w, h, w * 4, d, w * 4, swizzle=0x00020100) == (1, 1, 0), at   # alpha := r = 255: swizzled alpha counts as alpha
            finally:
                hip_ctx.free(d_src)
    finally:
        hip_ctx.free(d)


# ---------------------------------------------------------------- 2. all 2^24 colours

def test_device_renormalisation_of_all_2_24_colours_matches_the_tool(hip_ctx):
    """one upload, one launch (in place), hashing on the host: the 64 band digests of the tool's own prepared raster"""
    img = H.all_colours_image()
    d = hip_ctx.upload(img)
    try:
        assert hip_ctx.lib.k_renormalize_normal_map(hip_ctx.h, vp(d), H.ALL_SIDE, H.ALL_SIDE, H.ALL_SIDE * 4) == 1, hip_ctx.lib.last_error(hip_ctx.h)
        got = hip_ctx.download(d, img.shape, np.uint8)
    finally:
        hip_ctx.free(d)
    want = H.digests()["sha256"]
    bad = [k for k, (a, b) in enumerate(zip(H.band_digests(got), want)) if a != b]
    assert not bad, f"bands {bad} of 64 differ from the tool's"


# ---------------------------------------------------------------- 3. compress() with each case's options: the tool's file

def tool_key_values(case, data):
    return (helpers.ktx2_file_key_values if case["ext"] == "ktx2" else helpers.basis_file_key_values)(data)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_compress_returns_the_reference_tools_file(hip_ctx, case):
    want = H.golden()[0]["file_" + case["name"]]
    got = compress(hip_ctx, H.source_image(case), key_values=tool_key_values(case, want), **H.codec_kwargs(case), **case_kwargs(case))
    assert got.tobytes() == want.tobytes()


# ---------------------------------------------------------------- 4. the defaults are today's call

DEFAULTS = dict(renormalize=False, swizzle=None, check_for_alpha=True, force_alpha=False, y_flip=False, resample=None, mip_filter="kaiser", mip_scale=1.0, mip_wrapping=True,
                mip_srgb=None, mip_renormalize=False, mip_fast=True, mip_smallest_dimension=1, no_selector_rdo=False, no_endpoint_rdo=False)


def profile_regions(ctx, cap=256):
    """{region: (ms, launches)} of everything timed since profile_enable: ETC1S has more regions than Context.profile_read's 32"""
    names, ms, count = (C.c_char_p * cap)(), (C.c_double * cap)(), (C.c_uint32 * cap)()
    n = ctx.lib.profile_read(ctx.h, names, ms, count, cap)
    assert n <= cap
    return {names[i].decode(): (ms[i], count[i]) for i in range(n)}


@pytest.mark.parametrize("codec", [dict(quality=128, mipmaps=True), dict(uastc=True, ktx2=True, mipmaps=True)], ids=["etc1s_alpha", "uastc"])
def test_defaults_change_nothing_and_do_not_launch_the_prepare_kernel(hip_ctx, codec):
    img = H.alpha_image(20, 28, 5)
    plain = compress(hip_ctx, img, **codec)
    hip_ctx.profile_enable(True)
    try:
        named = compress(hip_ctx, img, **codec, **DEFAULTS)
        regions = profile_regions(hip_ctx)
    finally:
        hip_ctx.profile_enable(False)
    assert named.tobytes() == plain.tobytes()
    assert "prepare_source" not in regions and "renormalize_normal_map" not in regions
    # every slice of the call is tiled by one launch, straight from the level rasters: no plane is split off and nothing is tiled slice by slice
    assert "split_alpha" not in regions and "extract_blocks" not in regions
    assert regions["extract_slices"][1] == 1


def test_with_stats_the_etc1s_alpha_planes_are_split_and_the_file_is_the_same(hip_ctx):
    """the stats stage reads planes: one split per level (the five levels of 20x28), the tiles cut from those planes by the one launch, the same bytes"""
    img, codec = H.alpha_image(20, 28, 5), dict(quality=128, mipmaps=True)
    plain = compress(hip_ctx, img, **codec)
    hip_ctx.profile_enable(True)
    try:
        named = compress(hip_ctx, img, **codec, **DEFAULTS, stats=[])
        regions = profile_regions(hip_ctx)
    finally:
        hip_ctx.profile_enable(False)
    assert named.tobytes() == plain.tobytes()
    assert "prepare_source" not in regions and "renormalize_normal_map" not in regions and "extract_blocks" not in regions
    assert regions["split_alpha"][1] == 5
    assert regions["extract_slices"][1] == 1


def test_etc1s_alpha_golden_survives_the_device_split(hip_ctx):
    """the ETC1S file with alpha slices that tests/golden/image_stats_vectors.npz holds, through the split kernel"""
    arrays, _ = M.golden()
    want = arrays["file_etc1s_alpha_basis"]
    got = compress(hip_ctx, np.array(arrays["src_etc1s_alpha_basis"]), quality=128, key_values=helpers.basis_file_key_values(want))
    assert got.tobytes() == want.tobytes()


# ---------------------------------------------------------------- 5. split_alpha

@pytest.mark.parametrize("w,h", [(21, 13), (4, 1), (1030, 37)])
def test_split_alpha_equals_numpy(hip_ctx, w, h):
    img = np.random.default_rng(w + h).integers(0, 256, (h, w, 4), dtype=np.uint8)
    want_rgb = img.copy(); want_rgb[..., 3] = 255
    want_a = np.repeat(img[..., 3:4], 4, axis=2); want_a[..., 3] = 255
    host_rgb, host_a = H.host_split_alpha(img)
    assert (host_rgb == want_rgb).all() and (host_a == want_a).all()
    for pads in ((0, 0, 0), (2, 3, 1)):
        sp, cp, ap = (w + p for p in pads)
        src = np.full((h, sp, 4), 0x5A, np.uint8); src[:, :w] = img
        d_src, d_rgb, d_a = hip_ctx.upload(src), hip_ctx.upload(np.full((h, cp, 4), GUARD, np.uint8)), hip_ctx.upload(np.full((h, ap, 4), GUARD, np.uint8))
        try:
            assert hip_ctx.lib.k_split_alpha(hip_ctx.h, vp(d_src), w, h, sp * 4, vp(d_rgb), cp * 4, vp(d_a), ap * 4) == 1, hip_ctx.lib.last_error(hip_ctx.h)
            rgb, a = hip_ctx.download(d_rgb, (h, cp, 4), np.uint8), hip_ctx.download(d_a, (h, ap, 4), np.uint8)
            assert (rgb[:, :w] == want_rgb).all() and (a[:, :w] == want_a).all(), pads
            assert (rgb[:, w:] == GUARD).all() and (a[:, w:] == GUARD).all(), pads
            # the colour plane in place, as compress() runs it
            assert hip_ctx.lib.k_split_alpha(hip_ctx.h, vp(d_src), w, h, sp * 4, vp(d_src), sp * 4, vp(d_a), ap * 4) == 1
            back = hip_ctx.download(d_src, (h, sp, 4), np.uint8)
            assert (back[:, :w] == want_rgb).all() and (back[:, w:] == 0x5A).all() and (hip_ctx.download(d_a, (h, ap, 4), np.uint8)[:, :w] == want_a).all()
        finally:
            for d in (d_src, d_rgb, d_a):
                hip_ctx.free(d)


# ---------------------------------------------------------------- 6. the C ABI's refusals

def test_bad_arguments_are_refused_by_name_and_nothing_is_written(hip_ctx):
    w, h = 8, 8
    img = np.random.default_rng(3).integers(0, 256, (h, w, 4), dtype=np.uint8)
    fill = np.full((h, w, 4), GUARD, np.uint8)
    d_src, d_dst, d_dst2 = hip_ctx.upload(img), hip_ctx.upload(fill), hip_ctx.upload(fill)
    lib, ctx = hip_ctx.lib, hip_ctx.h
    P = w * 4
    ident = 0x03020100
    try:
        prepare = [((0, w, h, P, d_dst, P, 0, ident, 1, 0, 0), "null device pointer"), ((d_src, w, h, P, 0, P, 0, ident, 1, 0, 0), "null device pointer"),
                   ((d_src, 0, h, P, d_dst, P, 0, ident, 1, 0, 0), "zero dimension"), ((d_src, w, 0, P, d_dst, P, 0, ident, 1, 0, 0), "zero dimension"),
                   ((d_src, w, h, P - 4, d_dst, P, 0, ident, 1, 0, 0), "source row pitch 28 bytes is less than 4 * width = 32"),
                   ((d_src, w, h, P, d_dst, P - 1, 0, ident, 1, 0, 0), "destination row pitch 31 bytes is less than 4 * width = 32"),
                   ((d_src, w, h, P, d_dst, P + 2, 0, ident, 1, 0, 0), "4-byte aligned"), ((d_src + 2, w, h, P, d_dst, P, 0, ident, 1, 0, 0), "4-byte aligned"),
                   ((d_src, 16385, 1, 16385 * 4, d_dst, 16385 * 4, 0, ident, 1, 0, 0), "too large"),
                   ((d_src, w, h, P, d_dst, P, 0, 0x03020400, 1, 0, 0), "swizzle entry above 3"), ((d_src, w, h, P, d_dst, P, 0, 0xFF020100, 1, 0, 0), "swizzle entry above 3"),
                   ((d_dst, w, h, P, d_dst, P, 1, ident, 1, 0, 1), "source equals destination with y_flip")]
        for args, text in prepare:
            has_alpha, below = C.c_uint32(77), C.c_uint32(77)
            call = [vp(a) if k in (0, 4) else a for k, a in enumerate(args)]
            assert lib.k_prepare_source(ctx, *call, C.byref(has_alpha), C.byref(below)) == 0, args
            assert text in lib.last_error(ctx), (args, lib.last_error(ctx))
            assert (has_alpha.value, below.value) == (77, 77)
        renorm = [((0, w, h, P), "null device pointer"), ((d_dst, 0, h, P), "zero dimension"), ((d_dst, w, h, P - 4), "less than 4 * width"), ((d_dst, w, 16385, P), "too large")]
        for args, text in renorm:
            assert lib.k_renormalize_normal_map(ctx, vp(args[0]), *args[1:]) == 0, args
            assert "renormalize_normal_map" in lib.last_error(ctx) and text in lib.last_error(ctx), (args, lib.last_error(ctx))
        split = [((0, w, h, P, d_dst, P, d_dst2, P), "null device pointer"), ((d_src, w, h, P, 0, P, d_dst2, P), "null device pointer"),
                 ((d_src, w, h, P, d_dst, P, 0, P), "null device pointer"), ((d_src, w, 0, P, d_dst, P, d_dst2, P), "zero dimension"),
                 ((d_src, w, h, P, d_dst, P - 4, d_dst2, P), "colour row pitch 28"), ((d_src, w, h, P, d_dst, P, d_dst2, P - 4), "alpha row pitch 28"),
                 ((d_src, w, h, P - 4, d_dst, P, d_dst2, P), "source row pitch 28"), ((d_src, w, h, P, d_dst, P, d_dst, P), "a buffer of its own")]
        for args, text in split:
            call = [vp(a) if k in (0, 4, 6) else a for k, a in enumerate(args)]
            assert lib.k_split_alpha(ctx, *call) == 0, args
            assert "split_alpha" in lib.last_error(ctx) and text in lib.last_error(ctx), (args, lib.last_error(ctx))
        assert lib.k_prepare_source(None, vp(d_src), w, h, P, vp(d_dst), P, 0, ident, 1, 0, 0, None, None) == 0
        assert (hip_ctx.download(d_dst, fill.shape, np.uint8) == fill).all() and (hip_ctx.download(d_dst2, fill.shape, np.uint8) == fill).all(), "a refused call wrote something"
        assert (hip_ctx.download(d_src, img.shape, np.uint8) == img).all()
        # and the same buffers are fine when the arguments are; the two flags are optional
        assert lib.k_prepare_source(ctx, vp(d_src), w, h, P, vp(d_dst), P, 0, ident, 1, 0, 1, None, None) == 1
        assert (hip_ctx.download(d_dst, fill.shape, np.uint8) == img[::-1]).all()
    finally:
        for d in (d_src, d_dst, d_dst2):
            hip_ctx.free(d)
    with pytest.raises(ValueError, match="swizzle"):
        source.prepare_source(hip_ctx, img, swizzle="rgbq")
