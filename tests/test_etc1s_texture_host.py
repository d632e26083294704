"""Host half of the ETC1S texture targets (ETC2 RGBA, BC7 RGBA): the look-up searches of tools/gen_etc1s_transcode_tables.py and the CPU restatement of
tests/etc1s_texture_helpers.py against the reference tool's bytes (tests/golden/etc1s_texture_vectors.npz), and the Python layer's layout and refusals. No GPU."""
import numpy as np
import pytest

import etc1s_texture_helpers as X
import etc1s_transcode_helpers as E
from basis_universal_amd import transcode as T


def _files():
    _, meta = X.golden()
    return [f["name"] for f in meta["files"]]


@pytest.fixture(scope="module")
def coverage():
    arrays, _ = X.golden()
    dec = T.decode_etc1s_file(arrays["file_coverage_basis"])
    return arrays, dec, dec["images"][0], X.selectors16(dec["selector_palette"])


def test_generated_tables_are_what_the_tool_generates():
    import pathlib
    import sys
    sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent.parent / "tools"))
    import gen_etc1s_transcode_tables as G
    assert G.OUT.read_text() == G.generate()


def test_eac_a8_search_reproduces_every_entry_the_tool_shows(coverage):
    """Every block of the coverage file that goes through the EAC A8 look-up shows its entry in the tool's ETC2 bytes: base, table | multiplier, and the code of each
    selector the block uses. 1,023 of the 1,024 entries occur (meta says which one the writer cannot reach and why)."""
    arrays, dec, im, sel16 = coverage
    want = arrays[E.image_key("coverage_basis", 0, 0, 0) + "_etc2"]
    table, seen = X.tables()["eac_a8"], set()
    for k, (e, s) in enumerate(zip(im["alpha_endpoint_indices"].reshape(-1), im["alpha_selector_indices"].reshape(-1))):
        ep, sel = dec["endpoint_palette"][e], sel16[s]
        lo, hi = int(sel.min()), int(sel.max())
        if lo == hi:
            continue
        r = X.ALPHA_RANGES.index((lo, hi)) if (lo, hi) in X.ALPHA_RANGES else 0
        v = int(table[int(ep[3]), int(ep[0]), r])
        blk = want[k]
        assert (int(blk[0]), int(blk[1])) == (v & 255, (v >> 8) & 255), (k, ep, r)
        bits = int.from_bytes(blk[2:8].tobytes(), "big")
        for y in range(4):
            for x in range(4):
                assert (bits >> (45 - 3 * (x * 4 + y))) & 7 == (v >> (16 + 3 * int(sel[y * 4 + x]))) & 7, (k, x, y)
        seen.add((int(ep[3]), int(ep[0]), r))
    _, meta = X.golden()
    assert len(seen) == meta["coverage"]["eac_a8_entries"] == 1023


def test_bc7_searches_reproduce_every_entry_the_tool_shows(coverage):
    """The same for BC7 without the filter: a block of three or four selectors shows, per channel, the endpoints of the colour look-up's entry for the mapping with
    the least summed error, and in its alpha fields the endpoints and indices of the alpha look-up's entry -- either way round, depending on texel 0."""
    arrays, dec, im, sel16 = coverage
    want = arrays[E.image_key("coverage_basis", 0, 0, 0) + "_bc7nf"]
    t = X.tables()
    colour_seen, alpha_seen = set(), set()
    for k, (e, s) in enumerate(zip(im["endpoint_indices"].reshape(-1), im["selector_indices"].reshape(-1))):
        ep, sel = [int(v) for v in dec["endpoint_palette"][e]], sel16[s]
        used = sorted(set(int(v) for v in sel))
        if len(used) < 3:
            continue
        r = X.RANGES.index((used[0], used[-1]))
        lo, hi = int.from_bytes(want[k, :8].tobytes(), "little"), int.from_bytes(want[k, 8:].tobytes(), "little")
        rows = [t["bc7_color"][ep[3], ep[c], r] for c in range(3)]
        m = int(sum((row >> 16).astype(np.int64) for row in rows).argmin())
        swapped = bool(X.MAPPINGS[m][int(sel[0])] & 2)
        for c, shift in enumerate((8, 22, 36)):
            got = ((lo >> shift) & 127, (lo >> (shift + 7)) & 127)
            entry = (int(rows[c][m]) & 127, (int(rows[c][m]) >> 8) & 127)
            assert got == (entry[::-1] if swapped else entry), (k, ep, r, m, c)
        assert (hi >> 2) & 0x7FFFFFFF == X._index_bits([X.MAPPINGS[m][int(v)] ^ (3 if swapped else 0) for v in sel]), (k, m)
        colour_seen.add((ep[3], r, m))
        v = int(t["bc7_alpha"][ep[3], ep[0], r])   # the alpha slice is the same state
        a, trans = (v & 255, (v >> 8) & 255), v >> 16
        if (trans >> (2 * int(sel[0]))) & 2:
            a, trans = a[::-1], trans ^ 0xFF
        assert ((lo >> 50) & 255, ((lo >> 58) & 63) | ((hi & 3) << 6)) == a, (k, ep, r)
        assert hi >> 33 == X._index_bits([(trans >> (2 * int(v))) & 3 for v in sel]), (k, ep, r)
        alpha_seen.add((ep[3], ep[0], r))
    _, meta = X.golden()
    assert len(colour_seen) == meta["coverage"]["bc7_color_reachable"] and len(alpha_seen) == 8 * 32 * 3


@pytest.mark.parametrize("name", _files())
def test_restatement_reproduces_every_golden_block(name):
    """ETC2 RGBA, BC7 without and with the chroma filter, every image of every golden file: solid, two-selector and look-up routes, the filter's gate, its clamped taps
    on 1-wide images, the encoder's simple and principal-axis routes -- bit for bit in numpy float32"""
    arrays, meta = X.golden()
    dec = T.decode_etc1s_file(arrays["file_" + name])
    entry = next(f for f in meta["files"] if f["name"] == name)
    assert [[im["level"], im["layer"], im["face"], im["width"], im["height"]] for im in dec["images"]] == entry["images"]
    for im in dec["images"]:
        key = E.image_key(name, im["level"], im["layer"], im["face"])
        for suffix, got in (("_etc2", X.etc2_rgba_blocks(dec, im)), ("_bc7nf", X.bc7_blocks(dec, im, False)), ("_bc7", X.bc7_blocks(dec, im, True))):
            bad = np.flatnonzero((got != arrays[key + suffix]).any(1))
            assert bad.size == 0, (key, suffix, bad[:8])


def test_golden_meets_the_route_counts():
    _, meta = X.golden()
    c = meta["chroma_routes"]
    assert c["differ"] >= 32 and c["simple"] >= 8 and c["pca"] >= 8 and c["smooth"] >= 4, c
    cov = meta["coverage"]
    assert cov["two_selector_arms"] == 12 and cov["bc7_alpha_entries"] == 768 and cov["bc7_color_table_range_mapping"] == cov["bc7_color_reachable"] > 100, cov
    assert cov["bc7_alpha_entries_swapped"] > 0 and cov["bc7_color_swapped"] > 0, cov


def test_an_opaque_file_restates_to_the_opaque_alpha_halves():
    arrays, _ = X.golden()
    assert not T.read_etc1s_file(arrays["file_opaque_basis"])["has_alpha_slices"]
    key = E.image_key("opaque_basis", 0, 0, 0)
    assert (arrays[key + "_etc2"][:, :8] == np.array(X.OPAQUE_EAC_A8, np.uint8)).all()
    bc7 = arrays[key + "_bc7nf"]
    a0, a1 = (bc7[:, 6] >> 2) | ((bc7[:, 7] & 3) << 6), (bc7[:, 7] >> 2) | ((bc7[:, 8] & 3) << 6)
    assert (a0 == 255).all() and (a1 == 255).all()


def test_layout_sizes_offsets_and_rounding():
    images = [{"num_blocks_x": 5, "num_blocks_y": 7, "width": 20, "height": 28}, {"num_blocks_x": 3, "num_blocks_y": 1, "width": 9, "height": 3},
              {"num_blocks_x": 1, "num_blocks_y": 1, "width": 1, "height": 1}]
    for target, unit in T.ETC1S_TEXTURE_BYTES_PER_BLOCK.items():
        layout, total = T.etc1s_texture_layout(images, target)
        assert [e["shape"] for e in layout] == [(35, unit), (3, unit), (1, unit)] and all(e["dtype"] is np.uint8 for e in layout)
        assert [e["nbytes"] for e in layout] == [35 * unit, 3 * unit, unit]
        offsets = [0, (35 * unit + 15) & ~15, ((35 * unit + 15) & ~15) + ((3 * unit + 15) & ~15)]   # 8-byte targets: 280 -> 288, 24 -> 32
        assert [e["offset"] for e in layout] == offsets and total == offsets[2] + 16
    assert T.ETC1S_TEXTURE_BYTES_PER_BLOCK == {T.ETC1_RGB: 8, T.BC1_RGB: 8, T.ETC2_RGBA: 16, T.BC7_RGBA: 16}
    # the old targets lay out as image_layout does; a pixel target's raster is tight
    for target in (T.ETC1_RGB, T.BC1_RGB, T.RGBA32, T.RGB565):
        assert T.etc1s_texture_layout(images, target) == T.image_layout(images, target, etc1s=True)


def test_unknown_targets_and_flag_bits_raise_by_name():
    images = [{"num_blocks_x": 1, "num_blocks_y": 1, "width": 4, "height": 4}]
    for target, name in ((3, "BC3_RGBA"), (4, "BC4_R"), (5, "BC5_RG"), (10, "ASTC_4x4_RGBA"), (20, "ETC2_EAC_R11")):
        with pytest.raises(ValueError, match=rf"ETC1S texture target {target} \({name}\) is not supported"):
            T.etc1s_texture_layout(images, target)
        with pytest.raises(ValueError, match=rf"target {target} \({name}\)"):
            T.transcode_etc1s_texture(None, b"", target)
        with pytest.raises(ValueError, match=rf"target {target} \({name}\)"):
            T.transcode_etc1s_textures(None, b"", target)
    assert T.etc1s_decode_flags() == 0 and T.etc1s_decode_flags(chroma_filtering=False) == 64 == T.DECODE_FLAGS_NO_ETC1S_CHROMA_FILTERING
    with pytest.raises(ValueError, match=r"decode flags 0x60: bits 0x20 are not supported \(supported: 64, cDecodeFlagsNoETC1SChromaFiltering\)"):
        T.etc1s_decode_flags(decode_flags=64 | 32)


def test_the_first_family_still_refuses_the_new_targets():
    images = [{"num_blocks_x": 1, "num_blocks_y": 1, "width": 4, "height": 4}]
    for target, name in ((1, "ETC2_RGBA"), (3, "BC3_RGBA"), (6, "BC7_RGBA")):
        text = rf"ETC1S transcode target {target} \({name}\) is not supported \(supported: \[0, 2, 13, 14, 15, 16\]\)"
        with pytest.raises(ValueError, match=text):
            T.image_layout(images, target, etc1s=True)
        with pytest.raises(ValueError, match=text):
            T.transcode_etc1s_file(None, b"", target)
        with pytest.raises(ValueError, match=text):
            T.transcode_etc1s_file_images(None, b"", target)
        with pytest.raises(ValueError, match=text):
            T.transcode_etc1s_image(None, {}, {}, target)
