"""The host half of the .dds export (basis_universal_amd/dds.py) and the g++ build of the device packers (csrc/dds_pack.h through tests/native/dds_pack_host.cpp)
against the reference tool's files (tests/golden/dds_export_vectors.npz, tools/gen_golden_dds_export.py). Nothing here needs a GPU."""
import pathlib
import re
import struct

import numpy as np
import pytest

import dds_export_helpers as D
import helpers
from multi_image_helpers import Untouchable
from basis_universal_amd import dds, mipmap

CASES = D.cases()
ROOT = pathlib.Path(__file__).resolve().parent.parent


def _golden_file(name):
    arrays, _ = D.golden()
    return arrays[f"file_{name}"].tobytes()


def test_the_golden_holds_every_case_and_nothing_else():
    arrays, meta = D.golden()
    assert sorted(meta["cases"]) == sorted(CASES)
    for name, case in CASES.items():
        assert meta["cases"][name]["fmt"] == case["fmt"] and meta["cases"][name]["tool"] == case["tool"]
        got = D.golden_images(arrays, name)
        assert len(got) == len(case["images"]) and all((a == b).all() for a, b in zip(got, case["images"])), name


@pytest.mark.parametrize("name", sorted(CASES))
def test_header_writer_equals_the_tools_first_148_bytes(name):
    case = CASES[name]
    kw = case["kw"]
    h, w = case["images"][0].shape[:2]
    w, h = kw.get("resample", (w, h))
    levels = 1 + (len(mipmap.level_sizes(w, h, 1)) if kw.get("mipmaps") else 0)
    cubemap = kw.get("tex_type") == "cubemap"
    head = dds.dds_header(w, h, levels, len(case["images"]) // (6 if cubemap else 1), cubemap, case["fmt"], kw.get("srgb", True))
    assert len(head) == dds.HEADER_BYTES == 148
    assert head == _golden_file(name)[:148]


@pytest.mark.parametrize("name", sorted(CASES))
def test_read_dds_lists_every_subresource_of_the_tools_file(name):
    case, raw = CASES[name], _golden_file(name)
    info = dds.read_dds(raw)
    kw = case["kw"]
    cubemap = kw.get("tex_type") == "cubemap"
    h, w = case["images"][0].shape[:2]
    w, h = kw.get("resample", (w, h))
    assert (info["format"], info["width"], info["height"]) == (case["fmt"], w, h)
    assert info["faces"] == (6 if cubemap else 1) and info["layers"] * info["faces"] == len(case["images"])
    assert info["block"] == (case["fmt"] in D.BLOCK_FORMATS)
    assert info["srgb"] == (kw.get("srgb", True) and dds.FORMATS[case["fmt"]][4] != 0)
    sizes = [(w, h)] + (mipmap.level_sizes(w, h, 1) if kw.get("mipmaps") else [])
    assert info["levels"] == len(sizes) and len(info["images"]) == len(case["images"]) * len(sizes)
    at = 148
    for k, im in enumerate(info["images"]):    # file order: layer, face, level; back to back; the whole file
        image, level = divmod(k, len(sizes))
        assert (im["layer"], im["face"], im["level"]) == (image // info["faces"], image % info["faces"], level)
        assert (im["width"], im["height"]) == sizes[level] and im["offset"] == at and im["nbytes"] == dds.subresource_bytes(case["fmt"], *sizes[level])
        at += im["nbytes"]
    assert at == len(raw)
    assert (dds.read_dds(np.frombuffer(raw, np.uint8))["images"] == info["images"])


def _patched(raw, at, value):
    return raw[:at] + struct.pack("<I", value) + raw[at + 4:]


def test_read_dds_refuses_truncated_and_corrupt_files():
    for name in ("o20_bc1", "o20_r8", "cube_bc3", "array_bc1"):
        raw = _golden_file(name)
        for n in (0, 3, 4, 127, 147, 148, 149, len(raw) - 1):
            with pytest.raises(ValueError):
                dds.read_dds(raw[:n])
        with pytest.raises(ValueError):
            dds.read_dds(raw + b"\0")
        # field offsets: 0 magic, 4 dwSize, 8 flags, 12 height, 16 width, 20 pitch, 24 depth, 28 mips, 76 pf size, 80 pf flags, 84 fourcc, 108 caps, 112 caps2,
        # 128 dxgi, 132 dimension, 136 misc, 140 array size
        for at, values in {0: (0, 0x20534443), 4: (0, 123, 0xFFFFFFFF), 8: (0, 0xFFFFFFFF), 12: (0, 1, 16385, 0xFFFFFFFF), 16: (0, 1, 16385, 0xFFFFFFFF),
                           20: (0, 0xFFFFFFFF), 24: (1,), 28: (0, 1, 6, 33, 0xFFFFFFFF), 76: (0, 31), 80: (0,), 84: (0, 0x31545844), 108: (0, 0xFFFFFFFF),
                           112: (0x200, 0xFFFFFFFF, 0xFC00), 128: (0, 2, 98, 99, 0xFFFFFFFF), 132: (0, 2, 4), 136: (1, 0xFFFFFFFF), 140: (0, 7, 0x7FFFFFFF, 0xFFFFFFFF)}.items():
            for v in values:
                bad = _patched(raw, at, v)
                if bad == raw:
                    continue
                with pytest.raises(ValueError):
                    dds.read_dds(bad)
    # a cubemap's flag pair taken away or added on one side only
    cube = _golden_file("cube_bc3")
    for bad in (_patched(cube, 136, 0), _patched(cube, 112, 0), _patched(_golden_file("o20_bc1"), 136, 4), _patched(_golden_file("o20_bc1"), 112, 0xFE00)):
        with pytest.raises(ValueError):
            dds.read_dds(bad)


def test_format_table_and_alias():
    header = (ROOT / "include" / "basisu_hip.h").read_text()
    declared = {m.group(1).lower(): int(m.group(2)) for m in re.finditer(r"BU_HIP_DDS_(\w+) = (\d+)", header)}
    assert declared == {token: entry[0] for token, entry in dds.FORMATS.items()} and len(declared) == 13
    host = D.host()
    for token, (code, block, unit, unorm, srgb) in dds.FORMATS.items():
        if token == "bc7":
            assert host.hd_unit_bytes(code) == 0 and not host.hd_pack_blocks(None, 0, code, None) and not host.hd_pack_pixels(None, 0, code, None)
            continue
        assert host.hd_unit_bytes(code) == unit and bool(host.hd_is_block_format(code)) == block
        assert dds.parse_format(token) == dds.parse_format(token.upper()) == token
        assert (token in D.BLOCK_FORMATS) == block and (token in D.RAW_FORMATS) == (not block)
        assert bool(srgb) == (token in ("bc1", "bc2", "bc3", "a8r8g8b8", "a8b8g8r8"))
    assert host.hd_unit_bytes(13) == 0 and host.hd_unit_bytes(0xFFFFFFFF) == 0
    assert dds.parse_format("a1r5g6b5") == dds.parse_format("A1R5G6B5") == "a1r5g5b5"
    assert dds.dds_header(8, 8, 1, 1, False, "a1r5g6b5") == dds.dds_header(8, 8, 1, 1, False, "a1r5g5b5")
    # the sRGB code only where the format has one
    assert struct.unpack_from("<I", dds.dds_header(8, 8, 1, 1, False, "bc1", True), 128)[0] == 72
    assert struct.unpack_from("<I", dds.dds_header(8, 8, 1, 1, False, "bc1", False), 128)[0] == 71
    assert struct.unpack_from("<I", dds.dds_header(8, 8, 1, 1, False, "bc4", True), 128)[0] == 80
    assert struct.unpack_from("<I", dds.dds_header(8, 8, 1, 1, False, "r5g6b5", True), 128)[0] == 85


def test_refusals_come_before_the_context_is_touched():
    ctx, img = Untouchable(), helpers.synth(16, 16, 1)
    other = np.ascontiguousarray(helpers.synth(20, 28, 2))
    with pytest.raises(ValueError, match="neither of the two packers is implemented"):
        dds.export_dds(ctx, img, "bc7")
    with pytest.raises(ValueError, match="neither of the two packers is implemented"):
        dds.export_dds(ctx, img, "BC7")
    for fmt in ("bc6h", "", "rgba32", "bc1 ", None, 0):
        with pytest.raises(ValueError, match="unknown"):
            dds.export_dds(ctx, img, fmt)
    for tex_type in ("video", "volume"):
        with pytest.raises(ValueError, match="not supported for a .dds file"):
            dds.export_dds(ctx, [img, img], "bc1", tex_type=tex_type)
    with pytest.raises(ValueError, match="not one of"):
        dds.export_dds(ctx, img, "bc1", tex_type="3d")
    with pytest.raises(ValueError, match="separate files"):
        dds.export_dds(ctx, [img, img], "bc1")
    with pytest.raises(ValueError, match="multiple of 6"):
        dds.export_dds(ctx, [img] * 5, "bc3", tex_type="cubemap")
    with pytest.raises(ValueError, match="not all equal"):
        dds.export_dds(ctx, [img, other], "bc1", tex_type="2darray")
    with pytest.raises(ValueError, match="empty"):
        dds.export_dds(ctx, [], "bc1", tex_type="2darray")
    with pytest.raises(ValueError, match="uint8"):
        dds.export_dds(ctx, img[..., :3], "bc1")
    with pytest.raises(ValueError, match="swizzle"):
        dds.export_dds(ctx, img, "bc5", swizzle="rgbx")
    with pytest.raises(ValueError, match="mip_filter"):
        dds.export_dds(ctx, img, "bc1", mipmaps=True, mip_filter="cubic")
    with pytest.raises(ValueError, match="resample"):
        dds.export_dds(ctx, img, "bc1", resample=(0, 4))
    # the kernel on its own
    tiles = np.zeros((4, 64), np.uint8)
    with pytest.raises(ValueError, match="neither of the two packers is implemented"):
        dds.pack_dds_blocks(ctx, tiles, 4, "bc7")
    with pytest.raises(ValueError, match="unknown"):
        dds.pack_dds_blocks(ctx, tiles, 4, "etc1")
    with pytest.raises(ValueError, match="pixel format"):
        dds.pack_dds_blocks(ctx, tiles, 4, "r8")
    with pytest.raises(ValueError, match="block format"):
        dds.pack_dds_pixels(ctx, tiles, [(4, 4)], "bc1")
    with pytest.raises(ValueError, match="neither of the two packers is implemented"):
        dds.pack_dds_pixels(ctx, tiles, [(4, 4)], "bc7")


@pytest.mark.parametrize("name", sorted(n for n, c in CASES.items() if c["fmt"] != "a8b8g8r8"))
def test_host_build_reproduces_every_golden_payload_from_the_prepared_pixels(name):
    """the g++ build of dds_pack.h on the golden's own a8b8g8r8 pixels (the prepared slices themselves): every block, or every pixel, of the tool's payload"""
    arrays, _ = D.golden()
    fmt, raw = CASES[name]["fmt"], _golden_file(name)
    info, twin = dds.read_dds(raw), D.a8b8g8r8_twin(arrays, name)
    assert twin is not None and len(twin) == len(info["images"])
    for im in info["images"]:
        pixels = twin[(im["level"], im["layer"], im["face"])]
        assert pixels.shape == (im["height"], im["width"], 4)
        want = np.frombuffer(raw, np.uint8, im["nbytes"], im["offset"])
        if info["block"]:
            got = D.host_pack_blocks(helpers.to_pixel_blocks(pixels), fmt)
            want = want.reshape(got.shape)
            bad = np.flatnonzero((got != want).any(axis=1))
            assert not bad.size, f"{name} level {im['level']} layer {im['layer']} face {im['face']}: {bad.size} of {got.shape[0]} blocks differ, the first at {bad[:8]}"
        else:
            assert (D.host_pack_pixels(pixels, fmt) == want).all(), f"{name} level {im['level']}"


def test_raw_packings_truncate():
    """r >> 3, g >> 2, a >= 128, a >> 4: never rounded, for every value of a channel"""
    v = np.arange(256, dtype=np.uint32)
    px = np.zeros((256, 4), np.uint8)
    px[:, 0], px[:, 1], px[:, 2], px[:, 3] = v, v[::-1], (v * 7) & 255, (v * 13 + 5) & 255
    r, g, b, a = (px[:, k].astype(np.uint32) for k in range(4))
    u16 = lambda fmt: D.host_pack_pixels(px, fmt).view("<u2").astype(np.uint32)
    assert (u16("r5g6b5") == ((r >> 3) << 11 | (g >> 2) << 5 | (b >> 3))).all()
    assert (u16("a1r5g5b5") == ((a >= 128).astype(np.uint32) << 15 | (r >> 3) << 10 | (g >> 3) << 5 | (b >> 3))).all()
    assert (u16("a4r4g4b4") == ((a >> 4) << 12 | (r >> 4) << 8 | (g >> 4) << 4 | (b >> 4))).all()
    assert (D.host_pack_pixels(px, "a8r8g8b8").reshape(-1, 4) == px[:, [2, 1, 0, 3]]).all()
    assert (D.host_pack_pixels(px, "a8b8g8r8").reshape(-1, 4) == px).all()
    assert (D.host_pack_pixels(px, "r8") == px[:, 0]).all() and (D.host_pack_pixels(px, "r8g8").reshape(-1, 2) == px[:, :2]).all()
