#!/usr/bin/env python3
"""Known answers of the ETC1S transcoder's ETC2 RGBA and BC7 targets from the real reference tool (oracle/_ref/basisu, build machine only; `make -C oracle ref`)
-> tests/golden/etc1s_texture_vectors.npz.

Member 1, files compressed by the reference tool at -q 128, each as .basis and as .ktx2:
    alpha      32x24 with an alpha ramp
    opaque     20x28 without alpha: every two-half target takes the opaque alpha half
    mip        20x28 with alpha and a mip chain down to 1x1 (5x7, 3x4, 2x2, 1x1 and 1x1 blocks: single-block images and 1-wide edges for the filter's clamped taps)
    array      two 16x16 layers, the second with alpha
    cube       six 16x16 faces, one with alpha
    chroma64   64x64, saturated patches of different hue, some edges on block boundaries and some not, luma texture of varying strength inside: made for the BC7
               chroma filter. 16 blocks wide: a wave's 64 lanes span four block rows.
    chroma36   the same content at 36x20 (9x5 blocks): a row is no power of two and lanes of one wave sit on the left and the right image edge
Member 2, coverage: a synthetic ETC1S state, used as the colour AND as the alpha slice of one image, written by this package's own backend writer: every
    (intensity table, base, selector range) of the EAC A8 and BC7 alpha look-ups that a block can reach, every reachable (table, range, mapping) of the BC7 colour
    look-up, solid blocks of every selector over every grey base, two-selector blocks of every selector pair with texel 0 on the low and on the high selector, and the
    same two arms for the blocks of three and four selectors. Counted on what the file decodes to; the counts go into `meta`.
Per image the npz holds the raw blocks of `basisu -unpack -ktx_only`'s _transcoded_{ETC2_RGBA,BC7_RGBA}_*.ktx (key suffixes _etc2, _bc7) and, from a second run with
-no_etc1s_chroma_filtering, BC7 again (_bc7nf). The file is accepted only after tests/etc1s_texture_helpers.py's CPU restatement has reproduced every block of it.

BC3, BC4 and BC5 are not here: their look-up could not be restated as a search.
usage: gen_golden_etc1s_texture.py"""
import json
import pathlib
import struct
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
import gen_golden_etc1s_transcode as GG  # noqa: E402  (the tool runner, the file naming and the npz writer are that generator's)
from basis_universal_amd.transcode import decode_etc1s_file  # noqa: E402


def ktx1_levels(path, sizes, faces=1, unit=16):
    """gen_golden_etc1s_transcode.ktx1_levels for blocks of `unit` bytes"""
    raw = pathlib.Path(path).read_bytes()
    n_faces, levels, kv = struct.unpack_from("<III", raw, 52)
    assert n_faces == faces and levels == len(sizes) and kv == 0, (n_faces, levels, kv)
    at, out = 64, [[] for _ in range(faces)]
    for n in sizes:
        assert struct.unpack_from("<I", raw, at)[0] == n * unit
        at += 4
        for f in range(faces):
            out[f].append(np.frombuffer(raw, np.uint8, n * unit, at).reshape(n, unit).copy())
            at += n * unit
    assert at == len(raw)
    return out


def unpack_with_tool(name, data, ext, arrays):
    dec = decode_etc1s_file(data)
    for suffix, extra in (("", []), ("nf", ["-no_etc1s_chroma_filtering"])):
        with tempfile.TemporaryDirectory() as d:
            (pathlib.Path(d) / f"x.{ext}").write_bytes(bytes(data))
            GG.tool(["-unpack", "-ktx_only", *extra, f"x.{ext}"], d)
            by_image = {}
            for im in dec["images"]:
                by_image.setdefault((im["layer"], im["face"]), []).append(im)
            for (layer, face), ims in by_image.items():
                ims.sort(key=lambda im: im["level"])
                sizes = [im["num_blocks_x"] * im["num_blocks_y"] for im in ims]
                for short, tag in X.TAGS.items():
                    if suffix and short != "bc7":
                        continue
                    if ext == "basis" and dec["faces"] == 6:
                        levels = ktx1_levels(pathlib.Path(d) / f"x_transcoded_cubemap_{tag}_{layer}.ktx", sizes, 6)[face]
                    elif ext == "basis":
                        levels = ktx1_levels(pathlib.Path(d) / f"x_transcoded_{tag}_{layer:04d}.ktx", sizes)[0]
                    elif dec["faces"] == 6:
                        levels = ktx1_levels(pathlib.Path(d) / f"x_transcoded_{tag}_face_{face}_layer_{layer:04d}.ktx", sizes)[0]
                    else:
                        levels = ktx1_levels(pathlib.Path(d) / f"x_transcoded_{tag}_layer_{layer:04d}.ktx", sizes)[0]
                    for im, blocks in zip(ims, levels):
                        arrays[E.image_key(name, im["level"], layer, face) + "_" + short + suffix] = blocks
    return dec


def check_restatement(name, dec, arrays, routes):
    """the CPU restatement must reproduce every block of the file before it is accepted"""
    for im in dec["images"]:
        key = E.image_key(name, im["level"], im["layer"], im["face"])
        for suffix, got in (("_etc2", X.etc2_rgba_blocks(dec, im)), ("_bc7nf", X.bc7_blocks(dec, im, False)), ("_bc7", X.bc7_blocks(dec, im, True, routes))):
            bad = np.flatnonzero((got != arrays[key + suffix]).any(1))
            assert bad.size == 0, (key, suffix, bad[:8], got[bad[:2]], arrays[key + suffix][bad[:2]])


def chroma_image(w, h, seed):
    """Upper half: saturated patches of 12x12 pixels laid out from (-2, -2): every third patch edge is a block boundary, the others are not; inside a patch a luma
    texture whose strength differs from patch to patch (strong, weak, none), so that the filter's variance gate passes some blocks and stops others. Lower half: a
    slow chroma ramp (12 units of Co per block, a triangle wave) under a faint luma texture: neighbours differ by just more than the filter's threshold, and the
    rebuilt pixels vary so little that the encoder takes its simple-block route."""
    rng = np.random.default_rng(seed)
    hues = np.array([[230, 30, 30], [30, 210, 40], [40, 50, 230], [225, 215, 30], [215, 40, 215], [30, 210, 215], [235, 130, 20], [128, 128, 128]], np.float64)
    y, x = np.mgrid[0:h, 0:w]
    py, px = (y + 2) // 12, (x + 2) // 12
    patch = (py * 5 + px * 3 + (py * px) % 3) % len(hues)
    strength = np.array([0.55, 0.06, 0.0, 0.3])[(py + 2 * px) % 4]
    tex = np.sin(x * 1.3 + py) * np.cos(y * 0.9 + px) + rng.uniform(-0.3, 0.3, (h, w))
    rgb = hues[patch] * (0.62 + (strength * tex)[..., None] * 0.6)
    co = (np.abs(((x / 4.0 + y / 8.0) % 8) - 4) - 2) * 12
    luma = 120 + tex * 4
    rgb = np.where((y >= h // 2)[..., None], np.stack([luma + co, luma, luma - co], -1), rgb)
    img = np.full((h, w, 4), 255, np.uint8)
    img[..., :3] = np.clip(rgb, 0, 255).astype(np.uint8)
    return img


def with_alpha(img, seed):
    out = img.copy()
    h, w = img.shape[:2]
    out[..., 3] = np.clip(np.mgrid[0:h, 0:w][1] * (255 // max(w - 1, 1)) + np.random.default_rng(seed).integers(-20, 20, (h, w)), 0, 255).astype(np.uint8)
    return out


def reference_files(arrays, meta, routes):
    alpha_img = helpers.synth(32, 24, 13)
    alpha_img[..., 3] = np.clip(np.mgrid[0:24, 0:32][1] * 8 + np.mgrid[0:24, 0:32][0] * 3, 0, 255).astype(np.uint8)
    o20 = helpers.synth(20, 28, 12)
    cube = [helpers.synth(16, 16, 30 + i) for i in range(6)]
    cube[2] = with_alpha(cube[2], 41)
    jobs = [("alpha", [alpha_img], []), ("opaque", [o20], []), ("mip", [with_alpha(o20, 40)], ["-mipmap"]),
            ("array", [helpers.synth(16, 16, 20), with_alpha(helpers.synth(16, 16, 21), 42)], ["-tex_type", "2darray"]), ("cube", cube, ["-tex_type", "cubemap"]),
            ("chroma64", [chroma_image(64, 64, 5)], []), ("chroma36", [chroma_image(36, 20, 5)], [])]
    for name, imgs, args in jobs:
        decs = {}
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
            decs[ext] = unpack_with_tool(full, data, ext, arrays)
            meta["files"].append({"name": full, "container": ext, "has_alpha": bool(decs[ext]["has_alpha_slices"]),
                                  "images": [[im["level"], im["layer"], im["face"], im["width"], im["height"]] for im in decs[ext]["images"]]})
            check_restatement(full, decs[ext], arrays, routes.setdefault(name, {}) if ext == "basis" else {})
        print(name, [len(d["images"]) for d in decs.values()], "images", routes.get(name), flush=True)


def pattern(used, start_high):
    """16 selectors cycling through `used`, texel 0 on the lowest or the highest of them"""
    off = len(used) - 1 if start_high else 0
    return tuple(used[(k + off) % len(used)] for k in range(16))


def coverage_member(arrays, meta, routes):
    t = X.tables()
    errs = (t["bc7_color"] >> 16).astype(np.int64)
    rng = np.random.default_rng(91)
    sets = [(s,) for s in range(4)] + [(a, b) for a in range(4) for b in range(a + 1, 4)] + [(0, 1, 2), (1, 2, 3), (0, 1, 3), (0, 2, 3), (0, 1, 2, 3)]
    patterns = []
    for u in sets:
        patterns.append(pattern(u, False))
        if len(u) > 1:
            patterns.append(pattern(u, True))
    endpoints, blocks = {}, []

    def ep_index(e):
        return endpoints.setdefault(tuple(int(v) for v in e), len(endpoints))
    for tab in range(8):       # every table and base (grey: the alpha look-ups read the first channel) under every pattern
        for base in range(32):
            for p in range(len(patterns)):
                blocks.append((ep_index((base, base, base, tab)), p))
    reachable = 0
    for tab in range(8):       # every mapping the colour look-up can choose, per table and range; ranges 3..5 hold two selectors and never get to the look-up
        for r in range(3):
            e = errs[tab, :, r, :]
            best = (e[:, None, None, :] + e[None, :, None, :] + e[None, None, :, :]).argmin(3)
            for m in range(10):
                hits = np.argwhere(best == m)
                if not hits.size:
                    continue
                reachable += 1
                for pick in hits[rng.choice(hits.shape[0], min(2, hits.shape[0]), replace=False)]:
                    for p, pat in enumerate(patterns):
                        if len(set(pat)) >= 3 and (min(pat), max(pat)) == X.RANGES[r]:
                            blocks.append((ep_index((pick[0], pick[1], pick[2], tab)), p))
    nbx = 32
    while len(blocks) % nbx:
        blocks.append(blocks[-1])
    nby, n = len(blocks) // nbx, len(blocks)
    ep_pal, sel_pal = np.array(list(endpoints.keys()), np.uint8), np.array(patterns, np.uint8)
    ei, si = np.array([b[0] for b in blocks] * 2), np.array([b[1] for b in blocks] * 2)
    be = E.backend_from_state(ep_pal, sel_pal, ei, si, [(0, nbx, nby, nbx * 4, nby * 4, 0, 0, 0), (n, nbx, nby, nbx * 4, nby * 4, 0, 0, 1)])
    be.encode()
    data = be.basis_file()
    be.close()
    arrays["file_coverage_basis"] = np.asarray(data, np.uint8).copy()
    dec = unpack_with_tool("coverage_basis", bytes(data), "basis", arrays)
    im = dec["images"][0]
    assert im["has_alpha"] and (im["endpoint_indices"] == im["alpha_endpoint_indices"]).all() and (im["selector_indices"] == im["alpha_selector_indices"]).all()
    check_restatement("coverage_basis", dec, arrays, routes.setdefault("coverage", {}))
    sel16 = X.selectors16(dec["selector_palette"])
    eac, m5a, m5c, solid_values, two = set(), set(), set(), set(), set()
    for e, s in zip(im["endpoint_indices"].reshape(-1), im["selector_indices"].reshape(-1)):
        ep, sel = [int(v) for v in dec["endpoint_palette"][e]], sel16[s]
        used = sorted(set(int(v) for v in sel))
        lo, hi = used[0], used[-1]
        if len(used) == 1:
            solid_values.update((lo, int(v)) for v in X.block_colors(ep)[lo])
            continue
        eac.add((ep[3], ep[0], X.ALPHA_RANGES.index((lo, hi)) if (lo, hi) in X.ALPHA_RANGES else 0))
        if len(used) == 2:
            two.add((lo, hi, int(sel[0]) == hi))
            continue
        r = X.RANGES.index((lo, hi))
        m5a.add((ep[3], ep[0], r, bool((int(t["bc7_alpha"][ep[3], ep[0], r]) >> (16 + 2 * int(sel[0]))) & 2)))
        m = int(sum(errs[ep[3], ep[c], r] for c in range(3)).argmin())
        m5c.add((ep[3], r, m, bool(X.MAPPINGS[m][int(sel[0])] & 2)))
    grey_solid = {(s, int(v)) for tab in range(8) for b in range(32) for s in range(4) for v in X.block_colors((b, b, b, tab))[s][:1]}
    cov = {"blocks": n, "eac_a8_entries": len(eac), "bc7_alpha_entries": len({k[:3] for k in m5a}), "bc7_alpha_entries_swapped": len({k[:3] for k in m5a if k[3]}),
           "bc7_color_table_range_mapping": len({k[:3] for k in m5c}), "bc7_color_reachable": reachable, "bc7_color_swapped": len({k[:3] for k in m5c if k[3]}),
           "solid_selector_values": len(solid_values), "two_selector_arms": len(two)}
    # the writer moves a selector whose colour clamps onto its neighbour's (0 and 1 of table 0 over base 0 are both 0) to that neighbour, which changes the range:
    # an entry may stay unreached only where that happens
    unreached = sorted({(a, b, c) for a in range(8) for b in range(32) for c in range(4)} - eac)
    cov["eac_a8_unreached"] = [list(k) for k in unreached]
    for tab, base, r in unreached:
        c = X.block_colors((base, base, base, tab))[:, 0]
        assert c[0] == c[1] or c[2] == c[3], (tab, base, r)
    assert cov["eac_a8_entries"] >= 8 * 32 * 4 - 1 and cov["bc7_alpha_entries"] == 8 * 32 * 3 and cov["bc7_color_table_range_mapping"] == reachable, cov
    assert cov["bc7_alpha_entries_swapped"] > 0 and cov["bc7_color_swapped"] > 0 and grey_solid <= solid_values and cov["two_selector_arms"] == 12, cov
    meta["files"].append({"name": "coverage_basis", "container": "basis", "has_alpha": True, "images": [[0, 0, 0, nbx * 4, nby * 4]]})
    meta["coverage"] = cov
    print("coverage:", cov, routes["coverage"], flush=True)


if __name__ == "__main__":
    assert GG.BASISU.exists(), "oracle/_ref/basisu is missing: build it on the build machine (make -C oracle ref)"
    arrays, meta, routes = {}, {"files": [], "targets": X.TAGS}, {}
    reference_files(arrays, meta, routes)
    coverage_member(arrays, meta, routes)
    # the filter's routes on the two chroma images, from the restatement that has just reproduced every block; `differ` from the tool's two outputs alone
    chroma = {}
    for name in ("chroma64", "chroma36"):
        for k, v in routes[name].items():
            chroma[str(k)] = chroma.get(str(k), 0) + v
        key = E.image_key(name + "_basis", 0, 0, 0)
        chroma["differ"] = chroma.get("differ", 0) + int((arrays[key + "_bc7"] != arrays[key + "_bc7nf"]).any(1).sum())
    assert chroma["differ"] >= 32 and chroma.get("simple", 0) >= 8 and chroma.get("pca", 0) >= 8 and chroma.get("smooth", 0) >= 4, chroma
    meta["chroma_routes"] = chroma
    meta["all_routes"] = {n: {str(k): v for k, v in r.items()} for n, r in routes.items()}
    print("chroma:", chroma)
    arrays["meta"] = np.frombuffer(json.dumps(meta, sort_keys=True).encode(), np.uint8)
    GG.save(X.GOLDEN, arrays)
    assert X.GOLDEN.stat().st_size <= 1 << 20, X.GOLDEN.stat().st_size
    print("wrote", X.GOLDEN, X.GOLDEN.stat().st_size, "bytes,", len(arrays), "members")
