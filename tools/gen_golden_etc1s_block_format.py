#!/usr/bin/env python3
"""Known answers of the ETC1S transcoder's ASTC 4x4, EAC R11 and EAC RG11 targets from the real reference tool (oracle/_ref/basisu, build machine only;
`make -C oracle ref`) -> tests/golden/etc1s_block_format_vectors.npz.

Member 1, files compressed by the reference tool at -q 128, each as .basis and as .ktx2: gen_golden_etc1s_texture.py's alpha, opaque, mip, array and cube (the same
    images), and
    grey       24x20 grey without alpha
    greya      24x20 grey with an alpha ramp: ASTC's luminance + alpha route on natural content
Member 2, coverage: a synthetic ETC1S state whose palettes serve the colour AND the alpha slice of one image, each slice with its own indices, written by this
    package's own backend writer. What a block can reach is enumerated from the host tables (tools/gen_etc1s_transcode_tables.py); what the file holds is counted on
    what it decodes to, by the CPU restatement that has just reproduced every block; the counts go into `meta`. Parts (colour block / alpha block):
    A  grey base of every (table, base) under patterns of the ranges (0,3) (1,3) (0,2) (1,2) / the same block: the luminance + alpha route, every grey entry of the
       0..255 look-up for three and four selectors in both planes, the two-selector plane, and the EAC R11 look-up in both halves of RG11
    B  per reachable (table, range, mapping, swapped) of the 0..255 colour look-up two colours / constant alpha 255: the RGB route
    C  colours cycling through the reachable (table, range, mapping, swapped) of the 0..47 colour look-up / a grey base of every (table, base) under a pattern of each
       of the six ranges: the RGBA route's two look-ups
    S  colours of the widest table over selectors 0..3 for which clamping the ten errors at 65535 and scaling them to 65535 choose different mappings: what the
       look-ups store
    E  the widest table's two extremes in colour / in alpha against three-selector blocks: both outlier routes
    F  a solid colour / a solid alpha for every value a block colour can take against four-selector blocks: the single-colour routes; and both solid: void extent
    H  every set of one or two selectors in colour against every such set in alpha: block truncation
Per image the npz holds the raw blocks of `basisu -unpack -ktx_only`'s _transcoded_{ASTC_LDR_4X4_RGBA,ETC2_EAC_R11,ETC2_EAC_RG11}_*.ktx (key suffixes _astc, _r11, _rg11).
The file is accepted only after tests/etc1s_block_format_helpers.py's CPU restatement has reproduced every block of it.
usage: gen_golden_etc1s_block_format.py"""
import json
import pathlib
import sys
import tempfile

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests"))
sys.path.insert(0, str(ROOT / "tools"))
sys.path.insert(0, str(ROOT))
import helpers  # noqa: E402
import etc1s_transcode_helpers as E  # noqa: E402
import etc1s_texture_helpers as X  # noqa: E402
import etc1s_block_format_helpers as B  # noqa: E402
import gen_etc1s_transcode_tables as G  # noqa: E402
import gen_golden_etc1s_transcode as GG  # noqa: E402  (the tool runner and the npz writer)
import gen_golden_etc1s_texture as GT  # noqa: E402  (the images and the KTX1 reader)
from basis_universal_amd.transcode import decode_etc1s_file  # noqa: E402

UNIT = {"astc": 16, "r11": 8, "rg11": 16}


def unpack_with_tool(name, data, ext, arrays):
    dec = decode_etc1s_file(data)
    with tempfile.TemporaryDirectory() as d:
        (pathlib.Path(d) / f"x.{ext}").write_bytes(bytes(data))
        GG.tool(["-unpack", "-ktx_only", f"x.{ext}"], d)
        by_image = {}
        for im in dec["images"]:
            by_image.setdefault((im["layer"], im["face"]), []).append(im)
        for (layer, face), ims in by_image.items():
            ims.sort(key=lambda im: im["level"])
            sizes = [im["num_blocks_x"] * im["num_blocks_y"] for im in ims]
            for short, tag in B.TAGS.items():
                if ext == "basis" and dec["faces"] == 6:
                    levels = GT.ktx1_levels(pathlib.Path(d) / f"x_transcoded_cubemap_{tag}_{layer}.ktx", sizes, 6, UNIT[short])[face]
                elif ext == "basis":
                    levels = GT.ktx1_levels(pathlib.Path(d) / f"x_transcoded_{tag}_{layer:04d}.ktx", sizes, 1, UNIT[short])[0]
                elif dec["faces"] == 6:
                    levels = GT.ktx1_levels(pathlib.Path(d) / f"x_transcoded_{tag}_face_{face}_layer_{layer:04d}.ktx", sizes, 1, UNIT[short])[0]
                else:
                    levels = GT.ktx1_levels(pathlib.Path(d) / f"x_transcoded_{tag}_layer_{layer:04d}.ktx", sizes, 1, UNIT[short])[0]
                for im, blocks in zip(ims, levels):
                    arrays[E.image_key(name, im["level"], layer, face) + "_" + short] = blocks
    return dec


def check_restatement(name, dec, arrays, routes, details=None):
    """the CPU restatement must reproduce every block of the file before it is accepted"""
    for im in dec["images"]:
        key = E.image_key(name, im["level"], im["layer"], im["face"])
        for short, target in B.TARGETS.items():
            got = B.blocks(dec, im, target, routes if short == "astc" else None, details if short == "astc" else None)
            want = arrays[key + "_" + short]
            bad = np.flatnonzero((got != want).any(1))
            assert got.shape == want.shape and bad.size == 0, (key, short, bad[:8], got[bad[:2]], want[bad[:2]])


def grey_image(w, h, seed, alpha):
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    v = np.clip(128 + 90 * np.sin(x * 0.7) * np.cos(y * 0.5) + rng.integers(-25, 25, (h, w)), 0, 255).astype(np.uint8)
    img = np.full((h, w, 4), 255, np.uint8)
    img[..., 0] = img[..., 1] = img[..., 2] = v
    return GT.with_alpha(img, seed + 1) if alpha else img


def reference_files(arrays, meta, routes):
    alpha_img = helpers.synth(32, 24, 13)
    alpha_img[..., 3] = np.clip(np.mgrid[0:24, 0:32][1] * 8 + np.mgrid[0:24, 0:32][0] * 3, 0, 255).astype(np.uint8)
    o20 = helpers.synth(20, 28, 12)
    cube = [helpers.synth(16, 16, 30 + i) for i in range(6)]
    cube[2] = GT.with_alpha(cube[2], 41)
    jobs = [("alpha", [alpha_img], []), ("opaque", [o20], []), ("mip", [GT.with_alpha(o20, 40)], ["-mipmap"]),
            ("array", [helpers.synth(16, 16, 20), GT.with_alpha(helpers.synth(16, 16, 21), 42)], ["-tex_type", "2darray"]), ("cube", cube, ["-tex_type", "cubemap"]),
            ("grey", [grey_image(24, 20, 50, False)], []), ("greya", [grey_image(24, 20, 50, True)], [])]
    for name, imgs, args in jobs:
        counts = []
        for ext in ("basis", "ktx2"):
            with tempfile.TemporaryDirectory() as d:
                pngs = []
                for i, img in enumerate(imgs):
                    helpers.save_png(pathlib.Path(d) / f"in{i}.png", img)
                    pngs.append(f"in{i}.png")
                GG.tool([f"-{ext}", "-q", "128", *args, *pngs, "-output_file", f"out.{ext}"], d)
                data = (pathlib.Path(d) / f"out.{ext}").read_bytes()
            full = f"{name}_{ext}"
            arrays["file_" + full] = np.frombuffer(data, np.uint8).copy()
            dec = unpack_with_tool(full, data, ext, arrays)
            meta["files"].append({"name": full, "container": ext, "has_alpha": bool(dec["has_alpha_slices"]),
                                  "images": [[im["level"], im["layer"], im["face"], im["width"], im["height"]] for im in dec["images"]]})
            check_restatement(full, dec, arrays, routes.setdefault(name, {}) if ext == "basis" else {})
            counts.append(len(dec["images"]))
        print(name, counts, "images", routes.get(name), flush=True)


def pattern(used):
    return tuple(used[k % len(used)] for k in range(16))


SETS = [(s,) for s in range(4)] + [(a, b) for a in range(4) for b in range(a + 1, 4)] + [(0, 1, 2), (1, 2, 3), (0, 1, 3), (0, 2, 3), (0, 1, 2, 3)]
PATTERNS = [pattern(u) for u in SETS]
OF_RANGE = {(0, 3): SETS.index((0, 1, 2, 3)), (1, 3): SETS.index((1, 2, 3)), (0, 2): SETS.index((0, 1, 2)), (1, 2): SETS.index((1, 2)), (2, 3): SETS.index((2, 3)),
            (0, 1): SETS.index((0, 1))}


def colour_choices(table, unquant):
    """per (intensity table, range of three or four selectors): for every non-grey (r5, g5, b5) the mapping the colour route picks and whether the endpoints trade
    places -> {(table, range, mapping, swapped): [(r5, g5, b5), ...]}"""
    t4 = table.reshape(8, 32, 6, 10)
    errs = (t4 >> 16).astype(np.int64)
    lo, hi = unquant[(t4 & 255).astype(np.int64)], unquant[((t4 >> 8) & 255).astype(np.int64)]
    out = {}
    grey = np.eye(32, dtype=bool)[:, :, None] & np.eye(32, dtype=bool)[None, :, :]   # r == g and g == b
    for tab in range(8):
        for r in range(3):
            e = errs[tab, :, r, :]
            best = (e[:, None, None, :] + e[None, :, None, :] + e[None, None, :, :]).argmin(3)
            i, j, k = np.indices(best.shape)
            s0 = lo[tab, i, r, best] + lo[tab, j, r, best] + lo[tab, k, r, best]
            s1 = hi[tab, i, r, best] + hi[tab, j, r, best] + hi[tab, k, r, best]
            swapped = s1 < s0
            for m in range(10):
                for sw in (False, True):
                    hits = np.argwhere((best == m) & (swapped == sw) & ~grey)
                    if hits.size:
                        out[tab, r, m, sw] = hits
    return out


def coverage_member(arrays, meta, routes):
    t = B.tables()
    rng = np.random.default_rng(2026)
    unq = np.array(t.unquant)
    reach47 = colour_choices(t.table47.reshape(-1), unq)
    reach255 = colour_choices(t.whole255.reshape(-1), np.arange(256))
    endpoints, pairs = {}, []   # pairs: ((endpoint, pattern) of the colour block, (endpoint, pattern) of the alpha block)

    def ep(e):
        return endpoints.setdefault(tuple(int(v) for v in e), len(endpoints))

    def grey(tab, base):
        return ep((base, base, base, tab))
    four, three = SETS.index((0, 1, 2, 3)), SETS.index((0, 1, 2))
    busy_alpha, busy_colour = (grey(3, 14), four), (ep((9, 20, 27, 3)), four)
    opaque = (grey(0, 31), SETS.index((3,)))   # 255 in every texel
    for tab in range(8):                                                  # A
        for base in range(32):
            for r in ((0, 3), (1, 3), (0, 2), (1, 2)):
                pairs.append(((grey(tab, base), OF_RANGE[r]),) * 2)
    for (tab, r, m, sw), hits in sorted(reach255.items()):               # B
        for pick in hits[rng.choice(hits.shape[0], min(2, hits.shape[0]), replace=False)]:
            pairs.append(((ep((*pick, tab)), OF_RANGE[X.RANGES[r]]), opaque))
    picks47 = []
    for (tab, r, m, sw), hits in sorted(reach47.items()):
        for pick in hits[rng.choice(hits.shape[0], min(2, hits.shape[0]), replace=False)]:
            picks47.append((ep((*pick, tab)), OF_RANGE[X.RANGES[r]]))
    k = 0
    for tab in range(8):                                                  # C
        for base in range(32):
            for r in X.RANGES:
                pairs.append((picks47[k % len(picks47)], (grey(tab, base), OF_RANGE[r])))
                k += 1
    assert k >= len(picks47)
    scaled_rule = {}
    for name, whole, clamp_table, alpha_block in (("rgb", t.whole255, G.astc_endpoint_table(np.arange(256), scaled=False), opaque),      # S
                                                  ("rgba", t.table47, G.astc_endpoint_table(G.astc_unquant48(), scaled=False), busy_alpha)):
        a, b = (whole[7, :, 0, :] >> 16).astype(np.int64), (clamp_table.reshape(8, 32, 6, 10)[7, :, 0, :] >> 16).astype(np.int64)
        differ = np.argwhere((a[:, None, None, :] + a[None, :, None, :] + a[None, None, :, :]).argmin(3) != (b[:, None, None, :] + b[None, :, None, :] + b[None, None, :, :]).argmin(3))
        differ = differ[~((differ[:, 0] == differ[:, 1]) & (differ[:, 1] == differ[:, 2]))]
        chosen = differ[rng.choice(differ.shape[0], 16, replace=False)]
        scaled_rule[name] = {tuple(int(v) for v in c) for c in chosen}
        for c in chosen:
            pairs.append(((ep((*c, 7)), four), alpha_block))
    outer = SETS.index((0, 3))
    for base in range(32):                                                # E
        pairs.append(((ep((base, base ^ 1, base, 7)), outer), (grey(2, (base * 5) % 32), three)))
        pairs.append((busy_colour, (grey(7, base), outer)))
    values = sorted({int(v) for tab in range(8) for base in range(32) for v in X.block_colors((base, base, base, tab))[:, 0]})
    seen_c, seen_a = set(), set()
    for tab in range(8):                                                  # F
        for base in range(32):
            for s in range(4):
                v = int(X.block_colors((base, base, base, tab))[s, 0])
                if v not in seen_c:
                    seen_c.add(v)
                    solid = (ep((base, base ^ 1, base, tab)), SETS.index((s,)))
                    pairs.append((solid, busy_alpha))
                    pairs.append((solid, (grey(tab, base), SETS.index((s,)))))
                if v not in seen_a:
                    seen_a.add(v)
                    pairs.append((busy_colour, (grey(tab, base), SETS.index((s,)))))
    few = [k for k, u in enumerate(SETS) if len(u) <= 2]
    for n, (pc, pa) in enumerate((pc, pa) for pc in few for pa in few):   # H
        tab = n % 8
        pairs.append(((ep(((n * 7) % 32, (n * 11 + 3) % 32, (n * 13 + 5) % 32, tab)), pc), (grey((tab + 3) % 8, (n * 3) % 32), pa)))
    nbx = 32
    while len(pairs) % nbx:
        pairs.append(pairs[-1])
    n, nby = len(pairs), len(pairs) // nbx
    ep_pal, sel_pal = np.array(list(endpoints.keys()), np.uint8), np.array(PATTERNS, np.uint8)
    ei = np.array([p[0][0] for p in pairs] + [p[1][0] for p in pairs])
    si = np.array([p[0][1] for p in pairs] + [p[1][1] for p in pairs])
    be = E.backend_from_state(ep_pal, sel_pal, ei, si, [(0, nbx, nby, nbx * 4, nby * 4, 0, 0, 0), (n, nbx, nby, nbx * 4, nby * 4, 0, 0, 1)])
    be.encode()
    data = be.basis_file()
    be.close()
    arrays["file_coverage_basis"] = np.asarray(data, np.uint8).copy()
    dec = unpack_with_tool("coverage_basis", bytes(data), "basis", arrays)
    im = dec["images"][0]
    assert im["has_alpha"]
    details = []
    t.reached255.clear()
    check_restatement("coverage_basis", dec, arrays, routes.setdefault("coverage", {}), details)
    # what the file holds, from what it decodes to
    sel16 = X.selectors16(dec["selector_palette"])
    grey255, alpha255, alpha47, rgb, rgba, void_values, solid_values, solid_alpha, btc, outliers, r11 = set(), set(), set(), set(), set(), set(), set(), set(), set(), set(), set()
    scaled_seen, solid_swaps = {"rgb": set(), "rgba": set()}, set()
    flat = [im[k].reshape(-1) for k in ("endpoint_indices", "selector_indices", "alpha_endpoint_indices", "alpha_selector_indices")]
    for k, (route, d) in enumerate(details):
        e, ae = [int(v) for v in dec["endpoint_palette"][flat[0][k]]], [int(v) for v in dec["endpoint_palette"][flat[2][k]]]
        for pe, ps in ((e, sel16[flat[1][k]]), (ae, sel16[flat[3][k]])):
            lo, hi = int(ps.min()), int(ps.max())
            if lo != hi:
                r11.add((pe[3], pe[0], X.ALPHA_RANGES.index((lo, hi)) if (lo, hi) in X.ALPHA_RANGES else 0))
        if route == "void":
            void_values.update(d["color"] + (d["alpha"],))
        elif route == "btc":
            btc.add((d["pair"], d["alpha_pair"], d["swapped"]))
        elif route == "grey":
            grey255.update([d["grey255"]] if "grey255" in d else [])
            alpha255.update([d["alpha255"]] if "alpha255" in d else [])
        elif route == "rgb":
            rgb.add(d["color"] + (d["swapped"],))
            if d["color"][:2] == (7, 0) and tuple(e[:3]) in scaled_rule["rgb"]:
                scaled_seen["rgb"].add(tuple(e[:3]))
        else:
            if d["alpha"] == "lookup":
                alpha47.add(d["alpha47"])
            if d["alpha"] == "solid":
                solid_alpha.add(int(X.block_colors(ae)[int(sel16[flat[3][k]][0]), 1]))
            if d["color"] == "lookup":
                rgba.add(d["color47"] + (d["swapped"],))
                if d["color47"][:2] == (7, 0) and tuple(e[:3]) in scaled_rule["rgba"]:
                    scaled_seen["rgba"].add(tuple(e[:3]))
            if d["color"] == "solid":
                solid_values.update(d["solid_values"])
                solid_swaps.add(d["swapped"])
            outliers.update(w for w in ("color", "alpha") if d[w] == "outlier")
    all_r11 = {(a, b, c) for a in range(8) for b in range(32) for c in range(4)}
    all47 = {(a, b, c) for a in range(8) for b in range(32) for c in range(6)}
    all255 = {(a, b, c) for a in range(8) for b in range(32) for c in range(3)}
    cov = {"blocks": n, "grey_0_255_entries": len(grey255 & all255), "alpha_0_255_entries": len(alpha255 & all255), "alpha_0_47_entries": len(alpha47),
           "alpha_0_47_unreached": [list(v) for v in sorted(all47 - alpha47)], "grey_0_255_unreached": [list(v) for v in sorted(all255 - grey255)],
           "rgb_reachable": len(reach255), "rgb_covered": len(rgb & set(reach255)), "rgb_swapped": len({v for v in rgb if v[3]}), "rgb_not_swapped": len({v for v in rgb if not v[3]}),
           "rgba_reachable": len(reach47), "rgba_covered": len(rgba & set(reach47)), "rgba_swapped": len({v for v in rgba if v[3]}),
           "outlier_routes": sorted(outliers), "block_colour_values": len(values), "solid_colour_values": len(solid_values & set(values)),
           "solid_alpha_values": len(solid_alpha & set(values)), "void_extent_values": len(void_values & set(values)),
           "btc_selector_pairs": len({(a, b) for a, b, _ in btc}), "btc_swapped": len({v for v in btc if v[2]}),
           "r11_entries": len(r11), "r11_unreached": [list(v) for v in sorted(all_r11 - r11)],
           "solid_colour_swapped_and_not": sorted(solid_swaps), "scaled_error_rule_blocks": {w: len(v) for w, v in scaled_seen.items()},
           "table_0_255_rows_read": len(t.reached255)}
    # The writer moves a selector whose colour clamps onto its neighbour's to that neighbour, which changes the range: an entry may stay unreached only where that happens
    for tab, base, r in [tuple(v) for v in cov["r11_unreached"] + cov["alpha_0_47_unreached"] + cov["grey_0_255_unreached"]]:
        c = X.block_colors((base, base, base, tab))[:, 0]
        assert c[0] == c[1] or c[2] == c[3], (tab, base, r)
    assert cov["rgb_covered"] == cov["rgb_reachable"] and cov["rgba_covered"] == cov["rgba_reachable"], cov
    assert cov["outlier_routes"] == ["alpha", "color"] and cov["solid_colour_values"] == cov["void_extent_values"] == cov["block_colour_values"], cov
    assert cov["solid_alpha_values"] == cov["block_colour_values"] - 1 and 255 not in solid_alpha, cov   # a constant alpha of 255 takes the RGB route instead
    assert cov["solid_colour_swapped_and_not"] == [False, True], cov
    # no colour of either look-up has a high endpoint darker than its low one: the trade of endpoints is reachable through the single-colour table alone
    assert cov["rgb_swapped"] == cov["rgba_swapped"] == 0 and not any(k[3] for k in list(reach47) + list(reach255)), cov
    assert cov["grey_0_255_entries"] == cov["alpha_0_255_entries"] == 768 == cov["table_0_255_rows_read"] and cov["alpha_0_47_entries"] >= 8 * 32 * 6 - 1, cov
    assert cov["r11_entries"] >= 8 * 32 * 4 - 1, cov
    assert cov["btc_selector_pairs"] == 10 * 10 - 16 and cov["btc_swapped"] == 0, cov   # colours ascend with the selector: block truncation never trades its endpoints
    assert min(cov["scaled_error_rule_blocks"].values()) >= 8, cov
    meta["files"].append({"name": "coverage_basis", "container": "basis", "has_alpha": True, "images": [[0, 0, 0, nbx * 4, nby * 4]]})
    meta["coverage"] = cov
    print("coverage:", cov, routes["coverage"], flush=True)


if __name__ == "__main__":
    assert GG.BASISU.exists(), "oracle/_ref/basisu is missing: build it on the build machine (make -C oracle ref)"
    arrays, meta, routes = {}, {"files": [], "targets": B.TAGS}, {}
    reference_files(arrays, meta, routes)
    coverage_member(arrays, meta, routes)
    meta["all_routes"] = {n: {str(k): v for k, v in r.items()} for n, r in routes.items()}
    arrays["meta"] = np.frombuffer(json.dumps(meta, sort_keys=True).encode(), np.uint8)
    GG.save(B.GOLDEN, arrays)
    assert B.GOLDEN.stat().st_size <= 1 << 20, B.GOLDEN.stat().st_size
    print("wrote", B.GOLDEN, B.GOLDEN.stat().st_size, "bytes,", len(arrays), "members")
