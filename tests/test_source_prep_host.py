"""No GPU: csrc/source_prep.h built by g++ (tests/native/source_prep_host.cpp) against what the reference tool wrote (tests/golden/source_prep_vectors.npz,
source_prep_digests.json; tools/gen_golden_source_prep.py), the flag table of the cases, and compress()'s argument checks, which come before the context is touched."""
import numpy as np
import pytest

import source_prep_helpers as H
from basis_universal_amd import source
from basis_universal_amd.compress import compress


def test_renormalisation_of_all_2_24_colours_matches_the_tool():
    """every RGB value once: the 64 band digests of the tool's own prepared raster"""
    img = H.all_colours_image()
    want = H.digests()
    assert want["band_rows"] == H.BAND_ROWS and len(want["sha256"]) == H.ALL_SIDE // H.BAND_ROWS == 64
    got = H.host_renormalize(img)
    assert (got[..., 3] == img[..., 3]).all()
    assert int((got[..., :3] != img[..., :3]).any(axis=2).sum()) == want["pixels_changed"]
    bad = [k for k, (a, b) in enumerate(zip(H.band_digests(got), want["sha256"])) if a != b]
    assert not bad, f"bands {bad} of 64 differ from the tool's"


def test_the_synthetic_normal_map_has_its_known_shares():
    for w, h in ((21, 13), (20, 28)):
        img, counts = H.normal_map_image(w, h, 1)
        assert all(v >= w * h // 10 for v in counts.values()), counts
        assert int((img[..., :3] == 128).all(axis=2).sum()) >= counts["grey"]
        changed = (H.host_renormalize(img) != img).any(axis=2).sum()
        assert changed >= counts["off_unit"] // 2, "the off-unit pixels are inside the band renormalisation leaves alone"


def tool_level0(case):
    """the tool's prepared level-0 image of a case, cropped to its size, reassembled from the two ETC1S slices where the image has alpha; and the padded slices"""
    slices = H.slices_of(case)
    w, h = case["sizes"][0]
    level0 = np.array(slices[0][:h, :w])
    if not case["uastc"] and case["has_alpha"]:
        assert (level0[..., 3] == 255).all() and (slices[1][..., 3] == 255).all()
        assert (slices[1][..., 0] == slices[1][..., 1]).all() and (slices[1][..., 0] == slices[1][..., 2]).all()
        level0[..., 3] = slices[1][:h, :w, 0]
    return level0, slices


CASES = H.golden_cases()


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_host_preparation_equals_the_tools_prepared_raster(case):
    kw = H.kwargs_from_flags(case["flags"], source.normal_map_options)
    got, has_alpha, below = H.host_prepare(H.source_image(case), **H.prepare_kwargs(kw))
    assert has_alpha == case["has_alpha"]
    assert source.is_identity(**{**dict(renormalize=False, swizzle=None, check_for_alpha=True, force_alpha=False, y_flip=False), **H.prepare_kwargs(kw)}) == (not H.prepare_kwargs(kw))
    level0, slices = tool_level0(case)
    if "resample" in kw:
        assert level0.shape[:2] == source.resampled_size(case["w"], case["h"], kw["resample"])[::-1]
        return   # the level-0 raster is the resampled one: the resampler is the device's (tests/test_gpu_source_prep.py)
    assert level0.shape == got.shape and (got == level0).all()
    assert below == bool((level0[..., 3] < 255).any())
    # the tool pads every slice to whole blocks by repeating the last column and row
    ys, xs = np.minimum(np.arange(slices[0].shape[0]), level0.shape[0] - 1), np.minimum(np.arange(slices[0].shape[1]), level0.shape[1] - 1)
    if not case["uastc"] and case["has_alpha"]:
        rgb, alpha = H.host_split_alpha(got)
        assert (rgb[ys][:, xs] == slices[0]).all() and (alpha[ys][:, xs] == slices[1]).all()
    else:
        assert (got[ys][:, xs] == slices[0]).all()


def test_every_listed_case_is_in_the_golden_file_with_its_flags():
    listed = H.case_list()
    assert [{k: c[k] for k in listed[0]} for c in CASES] == listed, "tests/source_prep_helpers.py's cases changed: run tools/gen_golden_source_prep.py"
    flags = {f for c in listed for f in c["flags"] if f.startswith("-") and not f[1:2].isdigit()}
    assert flags == set(H._FLAGS) | {"-normal_map"}, "a flag of the table has no case, or a case a flag outside it"
    assert {c["has_alpha"] for c in CASES} == {True, False}


def test_the_preset_and_the_swizzle_parser():
    assert source.normal_map_options() == {"srgb": False, "mip_srgb": False, "no_selector_rdo": True, "no_endpoint_rdo": True}
    assert source.parse_swizzle(None) == source.parse_swizzle("rgba") == source.parse_swizzle("0123") == source.parse_swizzle((0, 1, 2, 3)) == 0x03020100
    assert source.parse_swizzle("rrrg") == source.parse_swizzle("RRRG") == 0x01000000 and source.parse_swizzle([2, 1, 0, 3]) == H.pack_swizzle("bgra") == 0x03000102
    assert source.resampled_size(21, 13, 0.6) == (13, 8) and source.resampled_size(20, 28, 0.6) == (12, 17) and source.resampled_size(5, 5, 0.01) == (1, 1)
    assert source.resampled_size(5, 5, (12, 9)) == (12, 9) and source.resampled_size(5, 5, None) is None and source.resampled_size(5, 5, (99999, 2)) == (16384, 2)


IMG = np.zeros((4, 4, 4), np.uint8)
BAD = [({"swizzle": "rgbx"}, "swizzle"), ({"swizzle": "rgb"}, "swizzle"), ({"swizzle": (0, 1, 2, 4)}, "swizzle"), ({"swizzle": (0, 1, 2)}, "swizzle"),
       ({"swizzle": (0, 1, 2, -1)}, "swizzle"), ({"mip_filter": "gaussian"}, "mip_filter"), ({"mip_filter": ""}, "mip_filter"), ({"mip_scale": 0.0}, "mip_scale"),
       ({"mip_scale": -1.0}, "mip_scale"), ({"mip_smallest_dimension": 0}, "mip_smallest_dimension"), ({"mip_smallest_dimension": 1.5}, "mip_smallest_dimension"),
       ({"resample": (0, 5)}, "resample"), ({"resample": (5, -1)}, "resample"), ({"resample": (5,)}, "resample"), ({"resample": 0.0}, "resample"),
       ({"resample": -0.5}, "resample"), ({"resample": (4.0, 4.0)}, "resample")]


@pytest.mark.parametrize("kw,text", BAD, ids=[f"{list(k)[0]}={list(k.values())[0]!r}" for k, _ in BAD])
def test_compress_refuses_bad_arguments_before_it_touches_the_context(kw, text):
    """ctx is None: anything but the ValueError would be an AttributeError"""
    for codec in ({}, {"uastc": True}):
        with pytest.raises(ValueError, match=text):
            compress(None, IMG, **codec, **kw)
    if "swizzle" in kw or "resample" in kw:
        with pytest.raises(ValueError, match=text):
            source.prepare_source(None, IMG, **kw)


def test_bad_images_are_refused_before_the_context():
    for image in (np.zeros((4, 4, 3), np.uint8), np.zeros((0, 4, 4), np.uint8), np.zeros((4, 0, 4), np.uint8)):
        with pytest.raises(ValueError):
            compress(None, image, y_flip=True)
        with pytest.raises(ValueError):
            source.prepare_source(None, image)
    with pytest.raises(ValueError, match="width and height"):
        source.prepare_source(None, 0x1000, renormalize=True)


def test_force_alpha_wins_over_no_alpha_as_in_the_reference():
    """comp.cpp:2616-2621: m_force_alpha is looked at first; the tool's own file for `-no_alpha -force_alpha` has alpha slices and the alpha kept"""
    (case,) = [c for c in CASES if c["name"] == "combo_force_and_no_alpha"]
    assert case["has_alpha"] and case["slices"] == 2
    got, has_alpha, _ = H.host_prepare(H.source_image(case), check_for_alpha=False, force_alpha=True)
    assert has_alpha and (got == H.source_image(case)).all()
