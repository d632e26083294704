"""-m gpu: compress() with several source images -- texture arrays, cubemaps, video, a volume -- against the files the reference tool wrote for the same images and
options (tests/golden/multi_image_vectors.npz, tools/gen_golden_multi_image.py). Every comparison of files is equality of bytes."""
import struct

import numpy as np
import pytest

import helpers
import multi_image_helpers as M
from basis_universal_amd import source, stats as stats_mod, transcode
from basis_universal_amd.compress import compress

pytestmark = pytest.mark.gpu
G, META = M.load()
CASES = M.cases()
CONTAINERS = ("basis", "ktx2")


def golden(name, ext):
    return G[f"file_{name}_{ext}"]


def key_values(data, ext):
    return (helpers.ktx2_file_key_values if ext == "ktx2" else helpers.basis_file_key_values)(data)


@pytest.fixture(scope="module")
def written(hip_ctx):
    """every case compressed once into both containers, shared by the tests below and left unchanged"""
    out = {}
    for name, case in CASES.items():
        images = M.golden_images(G, name)
        for ext in CONTAINERS:
            tool = golden(name, ext)
            out[name, ext] = compress(hip_ctx, images, ktx2=ext == "ktx2", key_values=key_values(tool, ext), **case["kw"])
    return out


@pytest.mark.parametrize("ext", CONTAINERS)
@pytest.mark.parametrize("name", list(CASES))
def test_file_equals_the_tools(written, name, ext):
    mine, tool = written[name, ext], golden(name, ext)
    assert mine.shape == tool.shape and (mine == tool).all(), (name, ext, mine.shape, tool.shape, np.argwhere(mine[:min(mine.size, tool.size)] != tool[:min(mine.size, tool.size)])[:8].ravel())


@pytest.mark.parametrize("name", ["d_etc1s_video_alpha", "e_uastc_video"])
def test_video_ktx2_gains_the_animation_key_on_its_own(hip_ctx, name):
    """without KTXanimData among the key-values compress() adds it as the tool does; the tool's file shows the bytes: duration 1, timescale 15, loop count 0"""
    tool = golden(name, "ktx2")
    kvs = key_values(tool, "ktx2")
    assert dict(kvs)["KTXanimData"] == struct.pack("<III", 1, 15, 0)
    rest = [(k, v) for k, v in kvs if k != "KTXanimData"]
    images = M.golden_images(G, name)
    mine = compress(hip_ctx, images, ktx2=True, key_values=rest, **CASES[name]["kw"])
    assert mine.shape == tool.shape and (mine == tool).all()
    other = compress(hip_ctx, images, ktx2=True, key_values=rest, ktx2_animdata=(2, 30, 5), **CASES[name]["kw"])
    assert dict(key_values(other, "ktx2"))["KTXanimData"] == struct.pack("<III", 2, 30, 5)
    # a key the caller gives wins over ktx2_animdata
    kept = compress(hip_ctx, images, ktx2=True, key_values=kvs, ktx2_animdata=(2, 30, 5), **CASES[name]["kw"])
    assert (kept == tool).all()


@pytest.mark.parametrize("uastc", [False, True])
def test_header_fields_of_a_basis_file(hip_ctx, uastc):
    """us_per_frame (clamped to 24 bits as basisu_file::init clamps it), userdata and the texture type arrive in the .basis header; nothing else changes"""
    name = "e_uastc_video" if uastc else "d_etc1s_video_alpha"
    images, tool = M.golden_images(G, name), golden(name, "basis")
    kw = dict(CASES[name]["kw"], key_values=key_values(tool, "basis"))
    mine = compress(hip_ctx, images, us_per_frame=33333, userdata=(0xDEADBEEF, 7), **kw)
    # basis_file_header: m_tex_type at 23, m_us_per_frame (24 bits) at 24, m_userdata0 / 1 at 31 / 35; the header's CRC16 at 6 covers them, the data CRC at 12 does not
    assert mine[23] == 3 and int.from_bytes(mine[24:27].tobytes(), "little") == 33333
    assert struct.unpack_from("<II", mine.tobytes(), 31) == (0xDEADBEEF, 7)
    same = np.ones(mine.size, bool)
    same[[6, 7, 24, 25, 26, *range(31, 39)]] = False
    assert mine.shape == tool.shape and (mine[same] == tool[same]).all()
    clamped = compress(hip_ctx, images, us_per_frame=0x1000000, **kw)
    assert int.from_bytes(clamped[24:27].tobytes(), "little") == 0xFFFFFF


def test_refusals_come_before_the_context_is_used():
    ctx = M.Untouchable()
    for name, (images, args) in M.refusals().items():
        tex_type = args[args.index("-tex_type") + 1]
        for uastc in (False, True):
            with pytest.raises(ValueError):
                compress(ctx, images, tex_type=tex_type, uastc=uastc)
    with pytest.raises(ValueError, match="empty"):
        compress(ctx, [], tex_type="2darray")
    with pytest.raises(ValueError, match="video files are not supported"):
        compress(ctx, M.golden_images(G, "d_etc1s_video_alpha"), tex_type="video", stats=[])


@pytest.mark.parametrize("kw", [dict(), dict(uastc=True, mipmaps=True), dict(mipmaps=True, ktx2=True)], ids=["etc1s", "uastc_mips", "etc1s_mips_ktx2"])
def test_a_list_of_one_image_is_the_bare_image(hip_ctx, kw):
    img = M.alpha_ramp(np.ascontiguousarray(helpers.synth(20, 28, 77)))
    bare = compress(hip_ctx, img, **kw)
    listed = compress(hip_ctx, [img], tex_type="2d", **kw)
    assert bare.shape == listed.shape and (bare == listed).all()


def sources_by_key(hip_ctx, name, written_file):
    """{(level, layer, face): source image} for stats.file_stats: every level of every image as compress() makes it -- the mip generator on the device"""
    from basis_universal_amd import mipmap
    kw = CASES[name]["kw"]
    images = M.golden_images(G, name)
    any_alpha = any(bool((img[..., 3] != 255).any()) for img in images)
    out = {}
    for k, img in enumerate(images):
        layer, face = source.image_layer_face(kw["tex_type"], k)
        levels = [img] + (mipmap.generate_mipmaps(hip_ctx, img, has_alpha=any_alpha) if kw.get("mipmaps") else [])
        for level, raster in enumerate(levels):
            out[(level, layer, face)] = np.ascontiguousarray(raster)
    return out


@pytest.mark.parametrize("name", ["a_etc1s_array_mips", "c_uastc_cubemap_alpha"])
def test_stats_come_per_slice_in_slice_order(hip_ctx, written, name):
    images, tool = M.golden_images(G, name), golden(name, "basis")
    got = []
    mine = compress(hip_ctx, images, key_values=key_values(tool, "basis"), stats=got, **CASES[name]["kw"])
    assert (mine == written[name, "basis"]).all()                    # the stats stage changes no byte of the file
    assert len(got) == G[f"slices_{name}"].shape[0]
    expected = stats_mod.file_stats(hip_ctx, mine, sources_by_key(hip_ctx, name, mine))
    assert got == expected


def test_uastc_video_stats_work_and_etc1s_video_stats_raise(hip_ctx, written):
    images = M.golden_images(G, "e_uastc_video")
    got = []
    mine = compress(hip_ctx, images, key_values=key_values(golden("e_uastc_video", "basis"), "basis"), stats=got, **CASES["e_uastc_video"]["kw"])
    assert (mine == written["e_uastc_video", "basis"]).all() and len(got) == 4
    assert got == stats_mod.file_stats(hip_ctx, mine, {(0, k, 0): img for k, img in enumerate(images)})
    with pytest.raises(ValueError, match="video files are not supported: a P-frame's blocks may repeat the previous frame's indices"):
        compress(hip_ctx, M.golden_images(G, "d_etc1s_video_alpha"), stats=[], **CASES["d_etc1s_video_alpha"]["kw"])


@pytest.mark.parametrize("ext", CONTAINERS)
@pytest.mark.parametrize("name", list(CASES))
def test_files_read_back_with_their_layers_faces_and_levels(written, name, ext):
    data, kw, rows = written[name, ext], CASES[name]["kw"], G[f"slices_{name}"]
    n_images = len(CASES[name]["images"])
    col = M.SLICE_FIELDS.index
    levels = int(rows[:, col("level")].max()) + 1
    faces = 6 if kw["tex_type"] == "cubemap" else 1
    want = sorted((level, *source.image_layer_face(kw["tex_type"], k)) for k in range(n_images) for level in range(levels))
    if kw.get("uastc"):
        info = transcode.read_uastc_file(data)
    elif kw["tex_type"] == "video":
        with pytest.raises(Exception, match="video files are not supported"):       # the ETC1S reader keeps no previous frame: it refuses them, and says so
            transcode.read_etc1s_file(data)
        return
    else:
        info = transcode.read_etc1s_file(data)
    assert sorted((im["level"], im["layer"], im["face"]) for im in info["images"]) == want
    assert info["faces"] == faces and info["layers"] == n_images // faces and len(info["levels"]) == levels
    w0, h0 = CASES[name]["images"][0].shape[1], CASES[name]["images"][0].shape[0]
    for im in info["images"]:
        assert (im["width"], im["height"]) == (max(1, w0 >> im["level"]), max(1, h0 >> im["level"]))
