"""-m gpu: compress(mip_levels=) and dds.compress_dds against the files the reference tool wrote from .dds sources whose mip chains it used as they are
(tests/golden/mip_levels_vectors.npz, tools/gen_golden_mip_levels.py). Every comparison of files is equality of bytes."""
import numpy as np
import pytest

import helpers
import image_metrics_helpers as IM
import mip_levels_helpers as L
import multi_image_helpers as M
from basis_universal_amd import dds, source, stats as stats_mod
from basis_universal_amd.compress import compress

pytestmark = pytest.mark.gpu
G, META = L.load()
CASES = L.cases()
FILES = [(name, ext) for name, case in CASES.items() for ext in case["exts"]]


def key_values(data, ext):
    return (helpers.ktx2_file_key_values if ext == "ktx2" else helpers.basis_file_key_values)(data)


def arrays_of(name):
    """the golden sources of a case as compress() takes them: (level-0 images, their lower levels), bare where the case is one file"""
    chains = [L.rgba_levels(dds.read_dds_source(data)) for data in L.golden_sources(G, name)]
    if len(chains) == 1:
        return chains[0][0], chains[0][1:]
    return [c[0] for c in chains], [c[1:] for c in chains]


def sources_of(name):
    files = L.golden_sources(G, name)
    return files[0] if len(files) == 1 else files


@pytest.fixture(scope="module")
def written(hip_ctx):
    """every case compressed once each way into each of its containers, shared by the tests below and left unchanged"""
    out = {}
    for name, ext in FILES:
        tool = G[f"file_{name}_{ext}"]
        kw = dict(CASES[name]["kw"], ktx2=ext == "ktx2", key_values=key_values(tool, ext))
        image, levels = arrays_of(name)
        out[name, ext, "arrays"] = compress(hip_ctx, image, mip_levels=levels, **kw)
        out[name, ext, "dds"] = dds.compress_dds(hip_ctx, sources_of(name), **kw)
    return out


@pytest.mark.parametrize("how", ["arrays", "dds"])
@pytest.mark.parametrize("name,ext", FILES)
def test_file_equals_the_tools(written, name, ext, how):
    mine, tool = written[name, ext, how], G[f"file_{name}_{ext}"]
    n = min(mine.size, tool.size)
    assert mine.shape == tool.shape and (mine == tool).all(), (name, ext, how, mine.shape, tool.shape, np.argwhere(mine[:n] != tool[:n])[:8].ravel())


def test_the_golden_cases_are_the_issues(written):
    """what the generator asserted of the tool, as far as the fixture shows it: slice counts and alpha flags per case"""
    col = M.SLICE_FIELDS.index
    for name, case in CASES.items():
        rows = G[f"slices_{name}"]
        assert rows.shape[0] == case["slices"] == META["cases"][name]["slices"]
        assert rows[:, col("alpha")].tolist() == case["alpha"]


def supplied_sources(name):
    """{(level, layer, face): source image} for stats.file_stats: level 0 as the options leave it is not needed here -- the stats cases have no level-0 options --
    and level k is the supplied level k"""
    image, levels = arrays_of(name)
    assert not {k for k in CASES[name]["kw"] if k not in ("uastc", "tex_type")}
    chains = [[image, *levels]] if isinstance(image, np.ndarray) else [[im, *lv] for im, lv in zip(image, levels)]
    return {(level, layer, 0): raster for layer, chain in enumerate(chains) for level, raster in enumerate(chain)}


@pytest.mark.parametrize("how", ["arrays", "dds"])
@pytest.mark.parametrize("name", [n for n, c in CASES.items() if c.get("stats")] + ["k_etc1s_array_alpha_in_one_level"])
def test_stats_are_those_of_the_supplied_levels(hip_ctx, written, name, how):
    ext = CASES[name]["exts"][0]
    tool = G[f"file_{name}_{ext}"]
    kw = dict(CASES[name]["kw"], ktx2=ext == "ktx2", key_values=key_values(tool, ext))
    got = []
    if how == "arrays":
        image, levels = arrays_of(name)
        mine = compress(hip_ctx, image, mip_levels=levels, stats=got, **kw)
    else:
        mine = dds.compress_dds(hip_ctx, sources_of(name), stats=got, **kw)
    assert (mine == written[name, ext, how]).all()                   # the stats stage changes no byte of the file
    assert len(got) == CASES[name]["slices"]
    assert got == stats_mod.file_stats(hip_ctx, mine, supplied_sources(name))
    if f"stats_{name}" in G.files:                                   # the tool's printed figures
        printed = G[f"stats_{name}"]
        assert printed.shape[0] == len(got)
        for k, one in enumerate(got):
            IM.assert_close_to_printed(one, printed[k], (name, how, k))


@pytest.mark.parametrize("kw", [dict(), dict(uastc=True, mipmaps=True), dict(mipmaps=True, ktx2=True, swizzle="rrrg")], ids=["etc1s", "uastc_mips", "etc1s_mips_ktx2_swizzle"])
def test_no_levels_is_the_plain_call(hip_ctx, kw):
    """mip_levels=None, [] and (several images) empty chains give the bytes of a call without the argument, and launch nothing new"""
    img = M.alpha_ramp(L.level_image(20, 28, 77))
    plain = compress(hip_ctx, img, **kw)
    for levels in (None, [], ()):
        hip_ctx.profile_enable(True)
        mine = compress(hip_ctx, img, mip_levels=levels, **kw)
        regions = hip_ctx.profile_read()
        hip_ctx.profile_enable(False)
        assert mine.shape == plain.shape and (mine == plain).all()
        assert "prepare_mip_levels" not in regions
    pair = [img, L.level_image(20, 28, 78)]
    plain = compress(hip_ctx, pair, tex_type="2darray", **kw)
    for levels in (None, [], [[], []]):
        mine = compress(hip_ctx, pair, tex_type="2darray", mip_levels=levels, **kw)
        assert mine.shape == plain.shape and (mine == plain).all()


def test_one_launch_for_all_levels_of_all_images(hip_ctx):
    """two files of three levels: ONE prepare_mip_levels launch either way; the .dds way it covers level 0 as well, and no generated level is made"""
    name = "k_etc1s_array_alpha_in_one_level"
    image, levels = arrays_of(name)
    for run in (lambda: compress(hip_ctx, image, mip_levels=levels, mipmaps=True, **CASES[name]["kw"]),
                lambda: dds.compress_dds(hip_ctx, sources_of(name), mipmaps=True, **CASES[name]["kw"])):
        hip_ctx.profile_enable(True)
        run()
        regions = hip_ctx.profile_read()
        hip_ctx.profile_enable(False)
        assert regions["prepare_mip_levels"][1] == 1 and regions["extract_slices"][1] == 1
        assert not [r for r in regions if "mipmap" in r or "resample" in r], regions


def test_a_dds_file_of_one_level_is_a_plain_image(hip_ctx):
    """no lower levels: `mipmaps` generates them and `resample` is allowed, exactly as for the image"""
    img = L.level_image(20, 28, 91)
    for order, legacy in (("rgba", False), ("bgra", False), ("bgra", True)):
        data = L.dds_file([img], order=order, legacy=legacy)
        for kw in (dict(mipmaps=True), dict(resample=(8, 8), uastc=True), dict(y_flip=True, swizzle="bgra")):
            mine, plain = dds.compress_dds(hip_ctx, data, **kw), compress(hip_ctx, img, **kw)
            assert mine.shape == plain.shape and (mine == plain).all(), (order, legacy, kw)


def test_swizzle_reaches_the_supplied_levels_and_nothing_else_does(hip_ctx):
    """against compress() itself: level 0 prepared with every option, the lower levels swizzled by numpy and handed over with the identity -- the same file"""
    image, levels = arrays_of("f_etc1s_swizzle_rrrg")
    mine = compress(hip_ctx, image, mip_levels=levels, swizzle="rrrg", y_flip=True, renormalize=True, force_alpha=True)
    d_raster, _, _ = source.prepare_source(hip_ctx, image, swizzle="rrrg", y_flip=True, renormalize=True, force_alpha=True)
    try:
        level0 = hip_ctx.download(d_raster, image.shape, np.uint8)
    finally:
        hip_ctx.free(d_raster)
    # y_flip is also a header flag of the file: keep the option and undo its effect on the pixels
    other = compress(hip_ctx, np.ascontiguousarray(level0[::-1]), mip_levels=[L.swizzled(lv, "rrrg") for lv in levels], y_flip=True, force_alpha=True)
    assert mine.shape == other.shape and (mine == other).all()
