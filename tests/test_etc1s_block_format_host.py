"""Host half of the ETC1S block-format targets (ASTC 4x4, EAC R11, EAC RG11): the look-up searches of tools/gen_etc1s_transcode_tables.py and the CPU restatement of
tests/etc1s_block_format_helpers.py against the reference tool's bytes (tests/golden/etc1s_block_format_vectors.npz), the Python layer's layout and refusals, and
the packing of the two lossless ASTC layouts against the format. No GPU."""
import functools
import os
import pathlib
import shutil
import subprocess

import numpy as np
import pytest

import etc1s_block_format_helpers as B
import etc1s_texture_helpers as X
import etc1s_transcode_helpers as E
from basis_universal_amd import transcode as T

ROOT = pathlib.Path(__file__).resolve().parent.parent
IMAGES = [{"num_blocks_x": 5, "num_blocks_y": 7, "width": 20, "height": 28}, {"num_blocks_x": 3, "num_blocks_y": 1, "width": 9, "height": 3},
          {"num_blocks_x": 1, "num_blocks_y": 1, "width": 1, "height": 1}]


def _files():
    _, meta = B.golden()
    return [f["name"] for f in meta["files"]]


@pytest.mark.parametrize("name", _files())
def test_restatement_reproduces_every_golden_block(name):
    """ASTC 4x4, EAC R11 and EAC RG11, every image of every golden file, byte for byte"""
    arrays, meta = B.golden()
    dec = T.decode_etc1s_file(arrays["file_" + name])
    entry = next(f for f in meta["files"] if f["name"] == name)
    assert [[im["level"], im["layer"], im["face"], im["width"], im["height"]] for im in dec["images"]] == entry["images"]
    for im in dec["images"]:
        key = E.image_key(name, im["level"], im["layer"], im["face"])
        for short, target in B.TARGETS.items():
            got, want = B.blocks(dec, im, target), arrays[key + "_" + short]
            bad = np.flatnonzero((got != want).any(1))
            assert got.shape == want.shape and bad.size == 0, (key, short, bad[:8])


def test_golden_meets_the_coverage_conditions():
    _, meta = B.golden()
    cov = meta["coverage"]
    # every grey entry of the 0..255 look-up for three and four selectors, in the colour plane and in the alpha plane of the luminance + alpha route
    assert cov["grey_0_255_entries"] == cov["alpha_0_255_entries"] == 8 * 32 * 3 and cov["grey_0_255_unreached"] == []
    # every reachable (table, range, mapping) of the RGB route and of the RGBA route's colour part. Neither look-up holds a colour whose high endpoints sum to less
    # than its low ones, so the endpoints never trade places there (the generator asserts that of the enumeration); they do in the single-colour route
    assert cov["rgb_covered"] == cov["rgb_reachable"] > 100 and cov["rgba_covered"] == cov["rgba_reachable"] > 100
    assert cov["rgb_swapped"] == cov["rgba_swapped"] == 0 and cov["solid_colour_swapped_and_not"] == [False, True]
    # all alpha entries of the 0..47 look-up but one: table 0 over base 0 under selectors (0, 1), whose two colours both clamp to 0 -- the writer folds such a
    # block onto one selector, so no file of this backend holds it and the entry rests on the search's rule alone
    assert cov["alpha_0_47_entries"] == 8 * 32 * 6 - 1 and cov["alpha_0_47_unreached"] == [[0, 0, 5]]
    assert cov["outlier_routes"] == ["alpha", "color"]
    # the single-colour route and void extent for every value a block colour can take; a constant alpha of 255 takes the RGB route, never the single-colour one
    assert cov["block_colour_values"] == cov["solid_colour_values"] == cov["void_extent_values"] == 256 and cov["solid_alpha_values"] == 255
    # block truncation for every set of one or two selectors in colour against every such set in alpha (all but one-against-one, which is void extent); colours
    # ascend with the selector, so its endpoints never trade places
    assert cov["btc_selector_pairs"] == 10 * 10 - 4 * 4 and cov["btc_swapped"] == 0
    assert cov["r11_entries"] == 8 * 32 * 4 and cov["r11_unreached"] == []
    assert min(cov["scaled_error_rule_blocks"].values()) >= 8
    routes = meta["all_routes"]
    assert all(routes["coverage"][r] >= 200 for r in B.ROUTES) and routes["grey"] == {"grey": 30} and routes["greya"] == {"grey": 30}
    assert routes["opaque"].get("rgb", 0) > 0 and routes["alpha"].get("rgba", 0) > 0


def test_layout_sizes_offsets_and_rounding():
    assert T.ETC1S_BLOCK_FORMAT_BYTES_PER_BLOCK == {T.ETC1_RGB: 8, T.ETC2_RGBA: 16, T.BC1_RGB: 8, T.BC7_RGBA: 16, T.ASTC_4x4_RGBA: 16, T.ETC2_EAC_R11: 8, T.ETC2_EAC_RG11: 16}
    for target, unit in T.ETC1S_BLOCK_FORMAT_BYTES_PER_BLOCK.items():
        layout, total = T.etc1s_block_format_layout(IMAGES, target)
        assert [e["shape"] for e in layout] == [(35, unit), (3, unit), (1, unit)] and all(e["dtype"] is np.uint8 for e in layout)
        assert [e["nbytes"] for e in layout] == [35 * unit, 3 * unit, unit]
        offsets = [0, (35 * unit + 15) & ~15, ((35 * unit + 15) & ~15) + ((3 * unit + 15) & ~15)]   # 8-byte targets: 280 -> 288, 24 -> 32
        assert [e["offset"] for e in layout] == offsets and total == offsets[2] + 16
    for target in list(T.ETC1S_TEXTURE_BYTES_PER_BLOCK) + list(T.ETC1S_BYTES_PER_PIXEL):
        assert T.etc1s_block_format_layout(IMAGES, target) == T.etc1s_texture_layout(IMAGES, target)


def test_unsupported_targets_and_flag_bits_raise_by_name():
    refused = ((3, "BC3_RGBA"), (4, "BC4_R"), (5, "BC5_RG"), (8, "PVRTC1_4_RGB"), (9, "PVRTC1_4_RGBA"), (11, "ATC_RGB"), (12, "ATC_RGBA"), (17, "FXT1_RGB"), (18, "PVRTC2_4_RGB"),
               (19, "PVRTC2_4_RGBA"), (22, "unknown"), (-1, "unknown"))
    for target, name in refused:
        text = rf"ETC1S block-format target {target} \({name}\) is not supported \(supported: \[0, 1, 2, 6, 10, 13, 14, 15, 16, 20, 21\]\)"
        with pytest.raises(ValueError, match=text):
            T.etc1s_block_format_layout(IMAGES, target)
        with pytest.raises(ValueError, match=text):
            T.transcode_etc1s_block_format(None, b"", target)
        with pytest.raises(ValueError, match=text):
            T.transcode_etc1s_block_formats(None, b"", target)
        with pytest.raises(ValueError, match=text):
            T.transcode_etc1s_block_format_image(None, {}, {}, target)
    # the second family still refuses the three new targets, by its own text
    for target, name in ((10, "ASTC_4x4_RGBA"), (20, "ETC2_EAC_R11"), (21, "ETC2_EAC_RG11")):
        with pytest.raises(ValueError, match=rf"ETC1S texture target {target} \({name}\) is not supported"):
            T.etc1s_texture_layout(IMAGES, target)


def test_generated_tables_are_what_the_tool_generates():
    G = B.tables().G
    assert G.OUT.read_text() == G.generate()


@functools.lru_cache(maxsize=None)
def _pair_colours(values):
    """(n * n, 4): the four interpolated values of every endpoint pair, in search order: hi outermost, lo innermost -- plain integer arithmetic, pair by pair"""
    out = []
    for hi in values:
        for lo in values:
            c0, c1 = lo * 257, hi * 257
            out.append([((c0 * (64 - w) + c1 * w + 32) // 64) >> 8 for w in B.WEIGHTS])
    return np.array(out, np.int64)


def _search(values, block, s0, s1, mapping, ends_weight):
    """one entry by the plainest statement of the search: the error of every pair, the first least of them; -> (lo, hi, raw error)"""
    colours = _pair_colours(tuple(values))
    err = sum((block[s] - colours[:, mapping[s]]) ** 2 * (ends_weight if s in (0, 3) else 1) for s in range(s0, s1 + 1))
    k = int(err.argmin())
    return k % len(values), k // len(values), int(err[k])


def _entries(values, t, base5, r):
    """the ten stored entries of (table, base, range): the searches, then the rule for errors past 16 bits"""
    block = [int(v) for v in X.block_colors((base5, base5, base5, t))[:, 0]]
    s0, s1 = B.RANGES[r]
    found = [_search(values, block, s0, s1, m, 8 if t == 7 and (s0, s1) == (0, 3) else 1) for m in B.MAPPINGS]
    top = max(f[2] for f in found)
    return [lo | (hi << 8) | ((err if top <= 0xFFFF else (2 * err * 0xFFFF + top) // (2 * top)) << 16) for lo, hi, err in found]


def test_astc_0_47_table_in_full_against_a_plain_search():
    t = B.tables()
    for tab in range(8):
        for base5 in range(32):
            for r in range(6):
                assert [int(v) for v in t.table47[tab, base5, r]] == _entries(t.unquant, tab, base5, r), (tab, base5, r)
    # the best grey mapping of both look-ups is the first least error of the ten
    for table in (t.table47, t.whole255):
        best = t.G.astc_best_grey_mapping(table.reshape(-1))
        assert best.shape == (8, 32, 6)
        for tab, base5, r in ((0, 0, 0), (7, 3, 0), (7, 31, 0), (3, 17, 4), (5, 9, 2)):
            errs = [int(v) >> 16 for v in table[tab, base5, r]]
            assert int(best[tab, base5, r]) == errs.index(min(errs))


def test_astc_0_255_table_on_a_seeded_sample_and_the_rows_whose_errors_are_scaled():
    """Every one of the 768 rows of ranges 0-2 is read by the goldens (meta: table_0_255_rows_read), and the restatement over them reproduces the tool. Against the plain
    search: the 32 rows of the widest table over selectors 0..3 -- the only ones whose errors are scaled, in either look-up -- and 40 seeded others, 720 entries."""
    t = B.tables()
    _, meta = B.golden()
    assert meta["coverage"]["table_0_255_rows_read"] == 768
    rng = np.random.default_rng(255)
    rows = [(7, b, 0) for b in range(32)] + [(int(rng.integers(8)), int(rng.integers(32)), int(rng.integers(6))) for _ in range(40)]
    values = list(range(256))
    scaled = 0
    for tab, base5, r in rows:
        want = _entries(values, tab, base5, r)
        assert [int(v) for v in t.whole255[tab, base5, r]] == want, (tab, base5, r)
        assert [int(v) for v in t.G.astc_table_0_255_entries(tab, base5, r)] == want
        scaled += max(v >> 16 for v in want) == 0xFFFF
    assert scaled >= 32


def test_small_astc_tables_against_their_definitions():
    t = B.tables()
    # the 48 values are those of ASTC's endpoint range 0..47: distinct, symmetric about 127.5, and the 8-bit expansions of 48 evenly spaced levels to within rounding
    assert len(set(t.unquant)) == 48 and t.unquant[0] == 0 and t.unquant[1] == 255
    assert sorted(t.unquant) == sorted(255 - v for v in t.unquant)
    assert max(abs(v - round(k * 255 / 47)) for k, v in enumerate(sorted(t.unquant))) <= 1
    pairs = [(lo, hi) for lo in range(48) for hi in range(48)]   # lo outermost
    at_weight_1 = [(((t.unquant[lo] * 257) * 43 + (t.unquant[hi] * 257) * 21 + 32) // 64) >> 8 for lo, hi in pairs]
    for i in range(256):
        errs = [abs(v - i) for v in at_weight_1]
        assert tuple(int(v) for v in t.solid[i]) == pairs[errs.index(min(errs))], i
        errs = [abs(v - i) for v in t.unquant]
        assert int(t.nearest[i]) == errs.index(min(errs)), i


def test_eac_r11_table_in_full_against_a_plain_search():
    """per entry: every (base, multiplier, table) in order, each in-range colour on its nearest of the eight 11-bit values"""
    t = B.tables()
    G = t.G
    base, mul, table = np.meshgrid(np.arange(256), np.arange(16), np.arange(16), indexing="ij")
    values = np.clip(base.reshape(-1, 1) * 8 + 4 + np.where(mul == 0, 1, mul * 8).reshape(-1, 1) * G.EAC_MODIFIERS[table.reshape(-1)], 0, 2047)   # (65536, 8), search order
    nearest = {}
    for tab in range(8):
        for base5 in range(32):
            block = [int(v) for v in X.block_colors((base5, base5, base5, tab))[:, 0]]
            for r, (s0, s1) in enumerate(B.ALPHA_RANGES):
                total = 0
                for s in range(s0, s1 + 1):
                    if block[s] not in nearest:
                        d = np.abs(values - (block[s] * 2047 + 128) // 255)
                        nearest[block[s]] = (d.min(1).astype(np.int64) ** 2, d.argmin(1))
                    total = total + nearest[block[s]][0]
                k = int(np.argmin(total))
                trans = sum(int(nearest[block[s]][1][k]) << (3 * s) for s in range(s0, s1 + 1))
                want = (k // 256) | (((k % 16) | (((k // 16) % 16) << 4)) << 8) | (trans << 16)
                assert int(t.r11[tab, base5, r]) == want, (tab, base5, r)


def test_solid_and_block_truncation_blocks_decode_to_the_etc1s_pixels():
    """The packing against the format, not against the restatement: a small decoder of exactly the void-extent layout and the CEM 12 / 1-bit-weight layout shows
    that every golden block of those two routes decodes, texel for texel, to what the ETC1S blocks themselves decode to."""
    arrays, _ = B.golden()
    seen = {"void": 0, "btc": 0}
    for name in ("coverage_basis", "opaque_basis", "mip_ktx2", "cube_basis"):
        dec = T.decode_etc1s_file(arrays["file_" + name])
        ep, sel16 = np.asarray(dec["endpoint_palette"]), X.selectors16(dec["selector_palette"])
        for im in dec["images"]:
            astc = arrays[E.image_key(name, im["level"], im["layer"], im["face"]) + "_astc"]
            details = []
            B.blocks(dec, im, B.ASTC_4x4_RGBA, details=details)
            alpha = im["alpha_endpoint_indices"] is not None
            for k, (route, _) in enumerate(details):
                if route not in seen:
                    continue
                texels = B.decode_astc_lossless(astc[k])
                assert texels is not None, (name, k, route)
                colours = X.block_colors(ep[im["endpoint_indices"].reshape(-1)[k]])[sel16[im["selector_indices"].reshape(-1)[k]]]
                assert (texels[:, :3] == colours).all(), (name, k, route)
                if alpha:
                    values = X.block_colors(ep[im["alpha_endpoint_indices"].reshape(-1)[k]])[:, 1][sel16[im["alpha_selector_indices"].reshape(-1)[k]]]
                    assert (texels[:, 3] == values).all(), (name, k, route)
                else:
                    assert (texels[:, 3] == 255).all(), (name, k, route)
                seen[route] += 1
    assert seen["void"] >= 256 and seen["btc"] >= 84, seen


def test_device_block_code_under_host_sanitizers_equals_the_restatement(tmp_path):
    """The per-block code the kernels run (etc1s_block_format_targets.h), built by g++ with AddressSanitizer and UndefinedBehaviorSanitizer into a stand-alone program
    (tools/etc1s_block_format_sanitize.cpp: host code, CPU only, a child process, nothing preloaded), over every block of the coverage file and 8,000 random blocks
    of random palette entries and selector words, with and without alpha: no sanitizer speaks, and every ASTC, R11 and RG11 block is the restatement's."""
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed to build the sanitizer program"
    exe = tmp_path / "etc1s_block_format_sanitize"
    r = subprocess.run([cxx, "-std=c++17", "-O2", "-g", "-fsanitize=address,undefined", "-static-libasan", "-static-libubsan", "-fno-sanitize-recover", "-fno-omit-frame-pointer",
                        "-ffp-contract=off", "-o", str(exe), str(ROOT / "tools" / "etc1s_block_format_sanitize.cpp")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    t = B.tables()
    arrays, _ = B.golden()
    dec = T.decode_etc1s_file(arrays["file_coverage_basis"])
    im = dec["images"][0]
    pal = np.ascontiguousarray(dec["endpoint_palette"], np.uint8).view(np.uint32).reshape(-1)
    flat = [im[k].reshape(-1) for k in ("endpoint_indices", "selector_indices", "alpha_endpoint_indices", "alpha_selector_indices")]
    n_cov = flat[0].size
    cov = np.stack([pal[flat[0]], dec["selector_palette"][flat[1]], np.ones(n_cov, np.uint32), pal[flat[2]], dec["selector_palette"][flat[3]]], 1)
    rng = np.random.default_rng(404)
    n_rnd = 8000
    entries = rng.integers(0, 32, (2, n_rnd, 4)).astype(np.uint8)
    entries[..., 3] = rng.integers(0, 8, (2, n_rnd))
    grey = rng.random((2, n_rnd)) < 0.3
    entries[grey, 1] = entries[grey, 0]
    entries[grey, 2] = entries[grey, 0]
    few = rng.integers(0, 4, (2, n_rnd, 4))   # selector words that use a handful of values: each texel picks one of four draws, which often coincide
    sels = E.selector_palette_u32(np.take_along_axis(few, rng.integers(0, 4, (2, n_rnd, 16)), 2).reshape(-1, 16)).reshape(2, n_rnd)
    rnd = np.stack([entries[0].view(np.uint32).reshape(-1), sels[0], (rng.random(n_rnd) < 0.7).astype(np.uint32), entries[1].view(np.uint32).reshape(-1), sels[1]], 1)
    records = np.ascontiguousarray(np.concatenate([cov, rnd]), np.uint32)
    np.concatenate([t.table47.reshape(-1), t.whole255.reshape(-1)]).astype(np.uint32).tofile(tmp_path / "tables.bin")
    records.tofile(tmp_path / "in.bin")
    env = dict(os.environ)
    env["ASAN_OPTIONS"] = "detect_leaks=1:abort_on_error=0"
    r = subprocess.run([str(exe), str(tmp_path / "tables.bin"), str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True, env=env)
    assert r.returncode == 0 and not r.stderr.strip() and r.stdout.split() == ["blocks", str(len(records))], (r.returncode, r.stdout[-500:], r.stderr[-3000:])
    got = np.fromfile(tmp_path / "out.bin", np.uint8).reshape(-1, 40)
    key = E.image_key("coverage_basis", 0, 0, 0)
    for name, at, width in (("astc", 0, 16), ("r11", 16, 8), ("rg11", 24, 16)):
        assert (got[:n_cov, at:at + width] == arrays[key + "_" + name]).all(), name
    routes = {}
    for k, rec in enumerate(rnd):
        e, ae = rec[0:1].view(np.uint8), rec[3:4].view(np.uint8)
        sel, asel = X.selectors16(rec[1:2])[0], X.selectors16(rec[4:5])[0]
        block, route, _ = B.astc_block(t, e, sel, ae if rec[2] else None, asel if rec[2] else None)
        routes[route] = routes.get(route, 0) + 1
        want = list(block.to_bytes(16, "little")) + B.eac_r11_block(t, e, sel) * 2 + (B.eac_r11_block(t, ae, asel) if rec[2] else B.OPAQUE_EAC)
        assert (got[n_cov + k] == np.array(want, np.uint8)).all(), (k, route, rec)
    assert all(routes.get(k, 0) >= 20 for k in B.ROUTES), routes   # every route is there; void extent, both words on one value, is the rarest
