"""compress() with several source images, the part that needs no device: the argument checks (each raised before the context is used) and the slice table --
order, first_block, alpha and i-frame flags -- against the `Slice:` lines the reference tool printed for the cases of tests/golden/multi_image_vectors.npz."""
import numpy as np
import pytest

import helpers
import multi_image_helpers as M
from basis_universal_amd import mipmap, source
from basis_universal_amd.compress import compress

G, META = M.load()
CASES = M.cases()
CTX = M.Untouchable()


def small(seed=1, w=16, h=16):
    return np.ascontiguousarray(helpers.synth(w, h, seed))


@pytest.mark.parametrize("name", list(CASES))
def test_slice_table_equals_the_tools_slice_lines(name):
    case, rows = CASES[name], G[f"slices_{name}"]
    kw = case["kw"]
    images = M.golden_images(G, name)
    assert len(images) == len(case["images"]) and all((a == b).all() for a, b in zip(images, case["images"]))   # the table above still makes the committed images
    image_alpha = [bool((img[..., 3] != 255).any()) for img in images]
    levels = [[(img.shape[1], img.shape[0])] + (mipmap.level_sizes(img.shape[1], img.shape[0], 1) if kw.get("mipmaps") else []) for img in images]
    slices, sources = source.slice_table(levels, uastc=bool(kw.get("uastc")), any_alpha=any(image_alpha), image_alpha=image_alpha, video=kw["tex_type"] == "video")
    mine = np.array([[i, s[7], s[3], s[4], s[1] * 4, s[2] * 4, s[0], s[5], s[6], s[8]] for i, s in enumerate(slices)], np.int64)
    assert mine.shape == rows.shape and (mine == rows).all(), (mine, rows)
    # what each slice is cut from: ETC1S with alpha a colour and an alpha slice of the same raster, everything else the raster as it is
    if any(image_alpha) and not kw.get("uastc"):
        assert [m for _, _, m in sources] == [source.SLICE_RGB, source.SLICE_ALPHA] * (len(slices) // 2)
    else:
        assert all(m == source.SLICE_AS_IS for _, _, m in sources)
    assert [(k, level) for k, level, _ in sources] == [(s[5], s[6]) for s in slices]


def test_the_cases_cover_what_they_are_there_for():
    rows = {name: G[f"slices_{name}"] for name in CASES}
    col = M.SLICE_FIELDS.index
    assert rows["c_uastc_cubemap_alpha"][:, col("alpha")].tolist() == [0, 0, 0, 1, 0, 0]           # UASTC: the alpha face alone carries the flag
    assert rows["b_etc1s_cubemap_alpha"][:, col("alpha")].tolist() == [0, 1] * 6                   # ETC1S: every face gets an alpha slice
    assert rows["d_etc1s_video_alpha"][:, col("iframe")].tolist() == [1, 1, 0, 0, 0, 0, 0, 0]      # the slices of frame 0
    assert rows["e_uastc_video"][:, col("iframe")].tolist() == [1, 1, 1, 1]
    f = rows["f_uastc_array_ragged_mips_rdo"]
    assert (f[:, col("orig_width")] != f[:, col("width")]).any() and ((f[:, col("width")] // 4) * (f[:, col("height")] // 4) == 1).any()   # ragged blocks, levels of one block
    assert set(META["refusals"]) == set(M.refusals()) and all(r["exit_status"] != 0 for r in META["refusals"].values())


@pytest.mark.parametrize("name,match", [("array_of_two_sizes", "resolutions are not all equal"), ("cubemap_of_five", "multiple of 6"), ("two_files_as_2d", "separate files")])
def test_what_the_tool_refuses_is_refused_before_the_context_is_used(name, match):
    images, args = M.refusals()[name]
    tex_type = {"3d": "volume"}.get(args[args.index("-tex_type") + 1], args[args.index("-tex_type") + 1])
    for uastc in (False, True):
        with pytest.raises(ValueError, match=match):
            compress(CTX, images, tex_type=tex_type, uastc=uastc)


@pytest.mark.parametrize("tex_type", ["2darray", "cubemap", "video", "volume"])
def test_images_of_different_sizes_are_refused_for_every_type_but_2d(tex_type):
    images = [small(i) for i in range(6)]
    images[4] = small(9, 20, 16)
    with pytest.raises(ValueError, match="resolutions are not all equal.*image 4 is 20 x 16"):
        compress(CTX, images, tex_type=tex_type)
    with pytest.raises(ValueError, match="resolutions are not all equal"):
        compress(CTX, images, tex_type=tex_type, resample=0.5)          # 8 x 8 and 10 x 8
    # a resample to one size makes them equal: the sizes compared are the prepared ones, and the refusal that remains is not about sizes
    source.check_texture_type(tex_type, [source.resampled_size(img.shape[1], img.shape[0], (8, 8)) for img in images])


def test_other_bad_arguments_are_refused_before_the_context_is_used():
    with pytest.raises(ValueError, match="empty"):
        compress(CTX, [])
    with pytest.raises(ValueError, match="empty"):
        compress(CTX, [], tex_type="video", uastc=True)
    with pytest.raises(ValueError, match="tex_type 'cube' is not one of 2d, 2darray, cubemap, video, volume"):
        compress(CTX, [small()], tex_type="cube")
    with pytest.raises(ValueError, match="tex_type '3d'"):
        compress(CTX, small(), tex_type="3d")
    with pytest.raises(ValueError, match="multiple of 6"):
        compress(CTX, [small(i) for i in range(7)], tex_type="cubemap", uastc=True)
    with pytest.raises(ValueError, match=r"image 1 must be \(h, w, 4\) uint8"):
        compress(CTX, [small(), small()[..., :3]], tex_type="2darray")
    with pytest.raises(ValueError, match="image 1 of 0 x 16"):
        compress(CTX, [small(), small()[:, :0]], tex_type="2darray")
    with pytest.raises(ValueError, match="swizzle"):
        compress(CTX, [small(), small()], tex_type="2darray", swizzle="rgbx")
    with pytest.raises(ValueError, match="mip_filter"):
        compress(CTX, [small(), small()], tex_type="video", mip_filter="nearest")
    with pytest.raises(ValueError, match="userdata"):
        compress(CTX, small(), userdata=(1, 2, 3))
    with pytest.raises(ValueError, match="us_per_frame"):
        compress(CTX, [small(), small()], tex_type="video", us_per_frame=-1)
    with pytest.raises(ValueError, match="video files are not supported"):
        compress(CTX, [small(), small()], tex_type="video", stats=[])
    with pytest.raises(ValueError, match="BC7"):
        compress(CTX, [small(), small()], tex_type="2darray", stats=[], stats_bc7=True)


def test_too_many_slices_are_refused_by_the_references_limit():
    assert source.MAX_SLICES == 0xFFFFFF
    assert source.check_slice_count(0xFFFFFF, 1, False) == 0xFFFFFF
    for images, levels, alpha in [(0x1000000, 1, False), (0x800000, 1, True), (0x200000, 5, True), (3, 0x555556, False)]:
        with pytest.raises(ValueError, match="too many slices.*BASISU_MAX_SLICES is 16777215"):
            source.check_slice_count(images, levels, alpha)


def test_layers_and_faces_of_the_source_images():
    assert [source.image_layer_face("cubemap", k) for k in (0, 5, 6, 13)] == [(0, 0), (0, 5), (1, 0), (2, 1)]
    assert [source.image_layer_face(t, 7) for t in ("2d", "2darray", "video", "volume")] == [(7, 0)] * 4
    assert source.TEX_TYPES == {"2d": 0, "2darray": 1, "cubemap": 2, "video": 3, "volume": 4}
