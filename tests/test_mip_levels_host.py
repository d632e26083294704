"""No GPU: the host half of caller-supplied mip chains -- dds.read_dds_source on the golden sources, on truncated files and on every kind of file it refuses; the
selector word; the slice table's per-level flags; and every ValueError of compress(mip_levels=) and dds.compress_dds, raised before the context is touched."""
import struct

import numpy as np
import pytest

import mip_levels_helpers as L
import multi_image_helpers as M
from basis_universal_amd import dds, source
from basis_universal_amd.compress import compress

G, META = L.load()
CASES = L.cases()


@pytest.mark.parametrize("name", list(CASES))
def test_read_dds_source_on_every_golden_source(name):
    files = L.golden_sources(G, name)
    assert len(files) == len(CASES[name]["files"]) == META["cases"][name]["files"]
    for data, f in zip(files, CASES[name]["files"]):
        assert (data == L.dds_file(f["levels"], f["order"], f["srgb"], f["legacy"])).all()     # the fixture's sources are the table's
        got = dds.read_dds_source(data)
        h, w = f["levels"][0].shape[:2]
        assert (got["width"], got["height"], got["byte_order"], got["dx10"]) == (w, h, f["order"], not f["legacy"])
        assert got["srgb"] == (f["srgb"] and not f["legacy"])
        assert [(lv["level"], lv["width"], lv["height"]) for lv in got["levels"]] == [(k, lv.shape[1], lv.shape[0]) for k, lv in enumerate(f["levels"])]
        at = 0
        for lv in got["levels"]:
            assert lv["offset"] == at and lv["nbytes"] == lv["width"] * lv["height"] * 4
            at += lv["nbytes"]
        assert got["payload"].size == at == data.size - (128 if f["legacy"] else 148)
        for mine, theirs in zip(L.rgba_levels(got), f["levels"]):
            assert (mine == theirs).all()
        assert dds.read_dds_source(data.tobytes())["payload"].tobytes() == got["payload"].tobytes()      # bytes and arrays alike


def test_read_dds_stays_the_reader_of_the_files_written_here():
    data = L.golden_sources(G, "a_etc1s_full_chain")[0]
    info = dds.read_dds(data)
    assert (info["format"], info["levels"], info["width"], info["height"]) == ("a8b8g8r8", 5, 20, 28)
    with pytest.raises(ValueError, match="only the DX10 header extension is read here"):
        dds.read_dds(L.golden_sources(G, "i_etc1s_legacy_bgra")[0])


@pytest.mark.parametrize("legacy", [False, True])
def test_truncations_at_every_header_boundary(legacy):
    levels = L.chain(20, 28, 3, 900)
    data = L.dds_file(levels, "bgra", legacy=legacy)
    header = 128 if legacy else 148
    cuts = [0, 3, 4, 127] + ([] if legacy else [128, 147]) + [header, header + 20 * 28 * 4 - 1, header + 20 * 28 * 4, header + 20 * 28 * 4 + 10 * 14 * 4, data.size - 1]
    for cut in cuts:
        with pytest.raises(ValueError, match="truncated .dds file"):
            dds.read_dds_source(data[:cut])
    assert len(dds.read_dds_source(data)["levels"]) == 3
    assert len(dds.read_dds_source(np.concatenate([data, np.zeros(7, np.uint8)]))["levels"]) == 3      # bytes behind the last level are not read


def patched(data, **fields):
    """a copy of a .dds file with 32-bit header fields replaced: name -> value, by byte offset"""
    offsets = dict(height=12, width=16, depth=24, mips=28, pf_flags=80, fourcc=84, bits=88, rmask=92, gmask=96, bmask=100, amask=104, caps2=112, dxgi=128, dimension=132,
                   misc=136, array=140)
    out = data.copy()
    for k, v in fields.items():
        out[offsets[k]:offsets[k] + 4] = np.frombuffer(struct.pack("<I", v), np.uint8)
    return out


def fourcc(text):
    return int.from_bytes(text, "little")


def test_each_refused_kind_of_file_is_named():
    levels = L.chain(20, 28, 3, 910)
    dx10, legacy = L.dds_file(levels), L.dds_file(levels, legacy=True)
    refused = [
        (patched(dx10, array=2), "a texture array of 2 layers"),
        (patched(dx10, misc=4), "a cubemap"), (patched(dx10, caps2=0xFE00), "a cubemap"), (patched(legacy, caps2=0xFE00), "a cubemap"),
        (patched(dx10, depth=4), "a volume texture"), (patched(dx10, dimension=4), "a volume texture"), (patched(legacy, caps2=0x200000, depth=2), "a volume texture"),
        (patched(dx10, dxgi=71), "DXGI format 71 is a block-compressed format"), (patched(dx10, dxgi=98), "DXGI format 98 is a block-compressed format"),
        (patched(legacy, pf_flags=0x4, fourcc=fourcc(b"DXT1")), "is a block-compressed format"), (patched(legacy, pf_flags=0x4, fourcc=fourcc(b"ATI2")), "is a block-compressed format"),
        (patched(dx10, dxgi=85), "DXGI format 85 is a 16-bit format"), (patched(dx10, dxgi=11), "DXGI format 11 is a 16-bit format"),
        (patched(legacy, bits=16, rmask=0xF800, gmask=0x07E0, bmask=0x001F, amask=0), "a 16-bit format"), (patched(legacy, pf_flags=0x4, fourcc=36), "is a 16-bit format"),
        (patched(dx10, dxgi=10), "DXGI format 10 is a float format"), (patched(dx10, dxgi=2), "DXGI format 2 is a float format"),
        (patched(legacy, pf_flags=0x4, fourcc=113), "is a float format"), (patched(legacy, pf_flags=0x4, fourcc=116), "is a float format"),
        (patched(dx10, dxgi=24), "DXGI format 24 is another pixel format"),
        (patched(legacy, amask=0), "only those of A8B8G8R8 and A8R8G8B8 are read"), (patched(legacy, bits=24), "only those of A8B8G8R8 and A8R8G8B8 are read"),
        (patched(dx10, width=16385), "16385 x 28 pixels"), (patched(dx10, height=0), "20 x 0 pixels"), (patched(dx10, height=1, mips=1), "a height of 1 is a 1D texture"),
        (np.frombuffer(b"DDSx" + dx10.tobytes()[4:], np.uint8), "not a .dds file"),
    ]
    for data, match in refused:
        with pytest.raises(ValueError, match=match):
            dds.read_dds_source(data)
    # what the tool's reader tolerates: a mip count of 0 is one level, a count past the full chain is cut to it
    assert len(dds.read_dds_source(patched(dx10, mips=0))["levels"]) == 1
    full = L.dds_file(L.chain(20, 28, 5, 920))
    assert len(dds.read_dds_source(patched(full, mips=9))["levels"]) == 5


def test_the_selector_is_byte_order_composed_with_the_swizzle():
    px = np.array([10, 20, 30, 40], np.uint8)                        # r, g, b, a
    for order, at in L.ORDERS.items():
        stored = px[at]
        for swizzle in (None, "rrrg", "abgr", "bgra", (3, 3, 0, 1)):
            word = source.level_selector(order, swizzle)
            got = np.array([stored[(word >> (8 * i)) & 255] for i in range(4)], np.uint8)
            want = px[[(source.parse_swizzle(swizzle) >> (8 * i)) & 255 for i in range(4)]]
            assert (got == want).all(), (order, swizzle, hex(word))
    assert source.level_selector() == source.IDENTITY_SWIZZLE and source.level_selector("bgra") == 0x03000102


def test_slice_table_takes_a_flag_per_level():
    sizes = [[(20, 28), (10, 14), (5, 7)]] * 2
    slices, _ = source.slice_table(sizes, uastc=True, any_alpha=True, image_alpha=[[False, False, True], [False, True, False]])
    assert [s[7] for s in slices] == [0, 0, 1, 0, 1, 0]
    slices, _ = source.slice_table(sizes, uastc=True, any_alpha=False, image_alpha=[[True] * 3] * 2)
    assert [s[7] for s in slices] == [0] * 6
    same, _ = source.slice_table(sizes, uastc=True, any_alpha=True, image_alpha=[True, False])       # a flag per image, as before
    assert [s[7] for s in same] == [1, 1, 1, 0, 0, 0]
    etc1s, _ = source.slice_table(sizes, uastc=False, any_alpha=True, image_alpha=[[False] * 3] * 2)
    assert [s[7] for s in etc1s] == [0, 1] * 6


def test_compress_refuses_bad_mip_levels_before_the_context_is_used():
    ctx = M.Untouchable()
    img, other = L.level_image(20, 28, 930), L.level_image(20, 28, 931)
    lv = L.chain(20, 28, 5, 940)[1:]
    refused = [
        (dict(image=img, mip_levels=[lv[0], L.level_image(5, 6, 1)]), "mip level 2 is 5 x 6 pixels; level 2 of 20 x 28 is 5 x 7"),
        (dict(image=img, mip_levels=[lv[1]]), "mip level 1 is 5 x 7 pixels; level 1 of 20 x 28 is 10 x 14"),
        (dict(image=img, mip_levels=[*lv, L.level_image(1, 1, 2)]), "5 mip levels below 20 x 28 pixels, whose full chain has 4"),
        (dict(image=[img, other], tex_type="2darray", mip_levels=[lv[:2], lv[:1]]), "unequal length"),
        (dict(image=[img, other], tex_type="2darray", mip_levels=[lv[:2], []]), "unequal length"),
        (dict(image=[img, other], tex_type="2darray", mip_levels=lv[:2]), "one sequence of levels per image"),
        (dict(image=[img], mip_levels=lv[:2]), "one sequence of levels per image"),
        (dict(image=[img, other], tex_type="2darray", mip_levels=[lv[:2]]), "the levels of 1 images, and there are 2"),
        (dict(image=img, mip_levels=[lv[:2]]), "a flat sequence"),
        (dict(image=img, mip_levels=[lv[0].astype(np.float32)]), "must be an \\(h, w, 4\\) uint8 array, not float32"),
        (dict(image=img, mip_levels=[lv[0].astype(np.uint16)]), "must be an \\(h, w, 4\\) uint8 array, not uint16"),
        (dict(image=img, mip_levels=[lv[0][..., :3]]), "must be an \\(h, w, 4\\) uint8 array"),
        (dict(image=img, mip_levels=[lv[0][..., 0]]), "must be an \\(h, w, 4\\) uint8 array"),
        (dict(image=[img, other], tex_type="2darray", mip_levels=[lv[:1], [lv[0].tolist()]]), "mip level 1 of image 1 must be"),
        (dict(image=img, mip_levels=lv[:2], resample=(8, 8)), "resample together with mip_levels: .*the reference resamples level 0 only"),
        (dict(image=img, mip_levels=lv[:2], resample=0.5), "resample together with mip_levels"),
        (dict(image=[img, other], tex_type="2d", mip_levels=[lv[:1], lv[:1]]), "tex_type '2d'"),
    ]
    for kw, match in refused:
        for uastc in (False, True):
            with pytest.raises(ValueError, match=match):
                compress(ctx, kw["image"], uastc=uastc, **{k: v for k, v in kw.items() if k != "image"})


def test_the_slice_limit_counts_the_supplied_levels(monkeypatch):
    """BASISU_MAX_SLICES is 2^24 - 1: lowered here, so that the refusal is reached with a handful of arrays"""
    ctx = M.Untouchable()
    monkeypatch.setattr(source, "MAX_SLICES", 11)
    imgs = [L.level_image(16, 16, 950 + i) for i in range(3)]
    chains = [L.chain(16, 16, 4, 960 + 10 * i)[1:] for i in range(3)]          # 3 images x 4 levels = 12 slices
    with pytest.raises(ValueError, match="12 slices \\(3 images x 4 levels\\): too many slices"):
        compress(ctx, imgs, tex_type="2darray", mip_levels=chains)
    with pytest.raises(ValueError, match="too many slices"):
        compress(ctx, imgs[:2], tex_type="2darray", mip_levels=chains[:2], force_alpha=True)      # 2 x 4 x colour and alpha = 16


def test_compress_dds_refuses_before_the_context_is_used():
    ctx = M.Untouchable()
    three, two = L.dds_file(L.chain(16, 16, 3, 970)), L.dds_file(L.chain(16, 16, 2, 980), "bgra")
    one, big = L.dds_file(L.chain(16, 16, 1, 990)), L.dds_file(L.chain(20, 28, 3, 995))
    with pytest.raises(ValueError, match="unequal length \\(2, 1 levels\\)"):          # the levels below level 0
        dds.compress_dds(ctx, [three, two], tex_type="2darray")
    with pytest.raises(ValueError, match="unequal length \\(2, 0 levels\\)"):
        dds.compress_dds(ctx, [three, one], tex_type="2darray")
    with pytest.raises(ValueError, match="resolutions are not all equal"):
        dds.compress_dds(ctx, [three, big], tex_type="2darray")
    with pytest.raises(ValueError, match="resample together with mip_levels"):
        dds.compress_dds(ctx, three, resample=(8, 8))
    with pytest.raises(ValueError, match="the levels below level 0 are the file's"):
        dds.compress_dds(ctx, three, mip_levels=[])
    with pytest.raises(ValueError, match="tex_type '2d'"):
        dds.compress_dds(ctx, [three, three])
    with pytest.raises(ValueError, match="truncated .dds file"):
        dds.compress_dds(ctx, three[:-1])
    with pytest.raises(ValueError, match="a cubemap"):
        dds.compress_dds(ctx, [three, patched(three, misc=4)], tex_type="2darray")
    with pytest.raises(ValueError, match="swizzle"):
        dds.compress_dds(ctx, three, swizzle="rgbx")
