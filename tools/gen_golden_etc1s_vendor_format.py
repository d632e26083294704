#!/usr/bin/env python3
"""Known answers of the ETC1S transcoder's ATC RGB, FXT1 and PVRTC2 4bpp RGB / RGBA targets from the real reference tool (oracle/_ref/basisu, build machine only;
`make -C oracle ref`) -> tests/golden/etc1s_vendor_format_vectors.npz.

Member 1, files compressed by the reference tool at -q 128, each as .basis and as .ktx2: gen_golden_etc1s_block_format.py's alpha, opaque, mip (20x28 down to 1x1:
    FXT1 rows of 5, 3, 2 and 1 source blocks), array, cube, grey and greya (the same images), and
    narrow     4x12, one block wide: every FXT1 block is a lone left half
Member 2, coverage: a synthetic ETC1S state whose palettes serve the colour AND the alpha slice of one image, written by this package's own backend writer. What a block can reach is enumerated from the host
    tables (tools/gen_etc1s_transcode_tables.py); what the file holds is counted on what it decodes to, by the CPU restatement that has just reproduced every block;
    the counts go into `meta`. Parts:
    A  per reachable (table, range, mapping) of the colour choice of each target -- ATC over the look-ups 55 / 56 / 55, PVRTC2 over 55 / 55 / 45, FXT1 over BC1's
       5 / 6 / 5 -- one colour, preferred among those whose four block colours do not clamp
    G  colours whose BC1 endpoints come out equal from the look-ups, zero and positive: FXT1's second punch-through guard
    F  a solid block for every value a block colour can take (grey, so that the value goes through every channel's table), among them 0 and 255: FXT1's first
       guard with both outcomes
    E  the widest table's two extremes alone, for every base: the outlier route
    The green-lsb swap of FXT1 falls both ways all over A. The alpha blocks of A-E are a constant 255, so that PVRTC2 RGBA takes its RGB route there.
    P  PVRTC2 RGBA: a busy colour block against a constant alpha of 249 and of 250; constant colours against constant alphas until the early exit (by err0 == 0 and
       by alpha < 3) and each of the modes 1, 0 and 3 has its blocks; constant colours against varying alpha; near-equal colours against varying alpha (the
       alpha-only modulation); and seeded pairs of colour and alpha blocks under patterns that run with and against each other: the 4D route with and without the
       alpha swap, the 2D route with and without the flip; and blocks whose first texel is the mean of the sixteen in all four channels, which take the 4D route's
       `< .5f` axis fallback. The generator also tries every grey block colour against every alpha value for the err0 == err3 tie.
Per image the npz holds the raw blocks of `basisu -unpack -ktx_only`'s _transcoded_{ATC_RGB,FXT1_RGB,PVRTC2_4_RGB,PVRTC2_4_RGBA}_*.ktx (key suffixes _atc, _fxt1, _pvrtc2, _pvrtc2a).
The file is accepted only after tests/etc1s_vendor_format_helpers.py's CPU restatement has reproduced every block of it.
usage: gen_golden_etc1s_vendor_format.py"""
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
import etc1s_vendor_format_helpers as V  # noqa: E402
import gen_golden_etc1s_transcode as GG  # noqa: E402  (the tool runner and the npz writer)
import gen_golden_etc1s_texture as GT  # noqa: E402  (the images and the KTX1 reader)
import gen_golden_etc1s_block_format as GB  # noqa: E402  (the grey images, the selector patterns)
from basis_universal_amd.transcode import decode_etc1s_file  # noqa: E402

LOOKUPS = {"atc": ("55", "56", "55"), "pvrtc2": ("55", "55", "45")}


def out_blocks(im, short):
    return (im["num_blocks_x"] + 1) // 2 * im["num_blocks_y"] if short == "fxt1" else im["num_blocks_x"] * im["num_blocks_y"]


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
            for short, tag in V.TAGS.items():
                sizes = [out_blocks(im, short) for im in ims]
                if ext == "basis" and dec["faces"] == 6:
                    levels = GT.ktx1_levels(pathlib.Path(d) / f"x_transcoded_cubemap_{tag}_{layer}.ktx", sizes, 6, V.UNIT[short])[face]
                elif ext == "basis":
                    levels = GT.ktx1_levels(pathlib.Path(d) / f"x_transcoded_{tag}_{layer:04d}.ktx", sizes, 1, V.UNIT[short])[0]
                elif dec["faces"] == 6:
                    levels = GT.ktx1_levels(pathlib.Path(d) / f"x_transcoded_{tag}_face_{face}_layer_{layer:04d}.ktx", sizes, 1, V.UNIT[short])[0]
                else:
                    levels = GT.ktx1_levels(pathlib.Path(d) / f"x_transcoded_{tag}_layer_{layer:04d}.ktx", sizes, 1, V.UNIT[short])[0]
                for im, blocks in zip(ims, levels):
                    arrays[E.image_key(name, im["level"], layer, face) + "_" + short] = blocks
    return dec


def check_restatement(name, dec, arrays, details=None):
    """the CPU restatement must reproduce every block of the file before it is accepted"""
    for im in dec["images"]:
        key = E.image_key(name, im["level"], im["layer"], im["face"])
        for short, target in V.TARGETS.items():
            got = V.blocks(dec, im, target, None if details is None else details.setdefault(short, []))
            want = arrays[key + "_" + short]
            bad = np.flatnonzero((got != want).any(1)) if got.shape == want.shape else []
            assert got.shape == want.shape and len(bad) == 0, (key, short, got.shape, want.shape, bad[:8], got[bad[:2]], want[bad[:2]])


def reference_files(arrays, meta):
    alpha_img = helpers.synth(32, 24, 13)
    alpha_img[..., 3] = np.clip(np.mgrid[0:24, 0:32][1] * 8 + np.mgrid[0:24, 0:32][0] * 3, 0, 255).astype(np.uint8)
    o20 = helpers.synth(20, 28, 12)
    cube = [helpers.synth(16, 16, 30 + i) for i in range(6)]
    cube[2] = GT.with_alpha(cube[2], 41)
    jobs = [("alpha", [alpha_img], []), ("opaque", [o20], []), ("mip", [GT.with_alpha(o20, 40)], ["-mipmap"]),
            ("array", [helpers.synth(16, 16, 20), GT.with_alpha(helpers.synth(16, 16, 21), 42)], ["-tex_type", "2darray"]), ("cube", cube, ["-tex_type", "cubemap"]),
            ("grey", [GB.grey_image(24, 20, 50, False)], []), ("greya", [GB.grey_image(24, 20, 50, True)], []), ("narrow", [helpers.synth(4, 12, 14)], [])]
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
            check_restatement(full, dec, arrays)
            counts.append(len(dec["images"]))
        print(name, counts, "images", flush=True)


def colour_choices(tr, tg, tb):
    """the mapping the colour route picks for every (r5, g5, b5) -> {(table, range, mapping): [(r5, g5, b5), ...]}, and (32, 32, 32) bool per (table, range): whether
    the chosen entries' low and high endpoints are equal in all three channels"""
    out, equal = {}, {}
    for tab in range(8):
        for r in range(6):
            er, eg, eb = [(t[tab, :, r, :] >> 16).astype(np.int64) for t in (tr, tg, tb)]
            best = (er[:, None, None, :] + eg[None, :, None, :] + eb[None, None, :, :]).argmin(3)
            i, j, k = np.indices(best.shape)
            vr, vg, vb = tr[tab, i, r, best], tg[tab, j, r, best], tb[tab, k, r, best]
            equal[tab, r] = ((vr & 255) == ((vr >> 8) & 255)) & ((vg & 255) == ((vg >> 8) & 255)) & ((vb & 255) == ((vb >> 8) & 255)), vr, vg, vb
            for m in range(10):
                hits = np.argwhere(best == m)
                if hits.size:
                    out[tab, r, m] = hits
    return out, equal


def mean_patterns(rng, inten):
    """{intensity table: [pattern, ...]}: selector patterns of sixteen whose FIRST texel has the mean of the sixteen values wherever nothing clamps. With the table's
    modifiers (-b, -a, a, b) and n_s texels on selector s that is b (n3 - n0) + a (n2 - n1) = 16 x the first texel's modifier. Up to three per table and first selector,
    of at least three selectors, the other fifteen texels in seeded order."""
    out = {}
    for tab in range(8):
        mods = [int(v) for v in inten[tab]]
        for s0 in range(4):
            found = []
            for n0 in range(17):
                for n1 in range(17 - n0):
                    for n2 in range(17 - n0 - n1):
                        n = [n0, n1, n2, 16 - n0 - n1 - n2]
                        if n[s0] >= 1 and sum(c > 0 for c in n) >= 3 and sum(c * m for c, m in zip(n, mods)) == 16 * mods[s0]:
                            found.append(n)
            for k in rng.permutation(len(found))[:3]:
                n = list(found[k])
                n[s0] -= 1
                rest = [sv for sv in range(4) for _ in range(n[sv])]
                out.setdefault(tab, []).append((s0,) + tuple(int(rest[j]) for j in rng.permutation(15)))
    return out


def unclamped(e):
    c = X.block_colors(e).astype(np.int64)
    return all(len(set(c[:, k])) == 4 for k in range(3))


def coverage_member(arrays, meta):
    t = V.tables()
    rng = np.random.default_rng(2027)
    reach = {"atc": colour_choices(*[t.atc[w] for w in LOOKUPS["atc"]])[0], "pvrtc2": colour_choices(*[t.atc[w] for w in LOOKUPS["pvrtc2"]])[0]}
    reach["fxt1"], bc1_equal = colour_choices(t.bc1[5], t.bc1[6], t.bc1[5])
    endpoints, blocks = {}, []   # blocks: (endpoint, pattern) of the colour slice; the alpha slice's are in `alphas`, a constant 255 where none is given

    def ep(e):
        return endpoints.setdefault(tuple(int(v) for v in e), len(endpoints))
    for short in ("atc", "pvrtc2", "fxt1"):                                # A
        for (tab, r, m), hits in sorted(reach[short].items()):
            order = hits[rng.permutation(hits.shape[0])]
            pick = next((h for h in order[:64] if unclamped((*h, tab))), order[0])
            blocks.append((ep((*pick, tab)), GB.OF_RANGE[X.RANGES[r]]))
    guard_candidates = {"zero": 0, "positive": 0}
    for (tab, r), (eq, vr, vg, vb) in sorted(bc1_equal.items()):          # G
        zero = eq & ((vr & 255) == 0) & ((vg & 255) == 0) & ((vb & 255) == 0)
        for what, mask in (("zero", zero), ("positive", eq & ~zero)):
            hits = np.argwhere(mask)
            guard_candidates[what] += int(hits.shape[0])
            for pick in hits[rng.permutation(hits.shape[0])[:3]]:
                blocks.append((ep((*pick, tab)), GB.OF_RANGE[X.RANGES[r]]))
    values = sorted({int(v) for tab in range(8) for base in range(32) for v in X.block_colors((base, base, base, tab))[:, 0]})
    seen = set()
    for tab in range(8):                                                   # F
        for base in range(32):
            for s in range(4):
                v = int(X.block_colors((base, base, base, tab))[s, 0])
                if v not in seen:
                    seen.add(v)
                    blocks.append((ep((base, base, base, tab)), GB.SETS.index((s,))))
    outer = GB.SETS.index((0, 3))
    for base in range(32):                                                 # E
        blocks.append((ep((base, base ^ 1, (base * 7) % 32, 7)), outer))
    patterns = list(GB.PATTERNS) + [p[::-1] for p in GB.PATTERNS] + [tuple(int(v) for v in rng.integers(0, 4, 16)) for _ in range(40)]
    mean_first = mean_patterns(rng, t.G.INTEN)   # for the 4D route's axis fallback, below
    pattern_at = {}
    for tab, pts in sorted(mean_first.items()):
        for pt in pts:
            pattern_at[pt] = len(patterns)
            patterns.append(pt)
    n_cyclic = len(GB.PATTERNS)
    one = {s: GB.SETS.index((s,)) for s in range(4)}
    opaque = (ep((31, 31, 31, 0)), one[3])   # 255 in every texel
    alphas = [opaque] * len(blocks)
    alpha_of = {}   # value -> a grey block and the selector that gives it
    for tab in range(8):
        for base in range(32):
            for sv in range(4):
                alpha_of.setdefault(int(X.block_colors((base, base, base, tab))[sv, 0]), (ep((base, base, base, tab)), one[sv]))
    busy = (ep((9, 20, 27, 3)), GB.SETS.index((0, 1, 2, 3)))

    def add(colour, alpha):
        blocks.append(colour)
        alphas.append(alpha)
    for v in (249, 250, 248, 251, 255, 0):                                 # P: the opaque gate on both sides
        add(busy, alpha_of[v])
    for k in range(24):                                                    # varying colour, constant alpha
        add((ep(((k * 7 + 2) % 32, (k * 5 + 9) % 32, (k * 11 + 4) % 32, k % 8)), GB.SETS.index((0, 1, 2, 3)) if k % 2 else GB.SETS.index((1, 2, 3))), alpha_of[values[(k * 41 + 7) % 250]])
    # constant colour against constant alpha: seeded combinations until every way out has its blocks, and the tie of err0 and err3 over every grey colour x alpha
    sel16 = {k: np.array(pt) for k, pt in enumerate(patterns)}
    pal = list(endpoints.keys())
    want, tie_search = {"early_err0": 12, "early_alpha": 12, "mode1": 12, "mode0": 12, "mode3": 12}, {"combinations": 0, "ties": 0}
    combos = [(v, a) for v in values for a in sorted(alpha_of) if a < 250]
    for k in rng.permutation(len(combos)):
        v, a = combos[k]
        (ce, cs), (aep, asl) = alpha_of[v], alpha_of[a]
        _, _, d = V.pvrtc2_rgba_block(t, pal[ce], sel16[cs], pal[aep], sel16[asl])
        if want.get(d["gate"], 0) > 0:
            want[d["gate"]] -= 1
            add(alpha_of[v], alpha_of[a])
        if not any(want.values()):
            break
    assert not any(want.values()), want
    for v, a in combos:
        (ce, cs), (aep, asl) = alpha_of[v], alpha_of[a]
        _, _, d = V.pvrtc2_rgba_block(t, pal[ce], sel16[cs], pal[aep], sel16[asl])
        tie_search["combinations"] += 1
        tie_search["ties"] += bool(d.get("tie03"))
    four, rev = GB.SETS.index((0, 1, 2, 3)), n_cyclic + GB.SETS.index((0, 1, 2, 3))
    for k in range(24):                                                    # constant colour, varying alpha; near-equal colours (table 0, selectors 1 and 2), varying alpha
        add(alpha_of[values[(k * 37) % len(values)]], (ep(((k * 5) % 32,) * 3 + (k % 8,)), four if k % 2 else rev))
        add((ep(((k * 7 + 3) % 32, (k * 11) % 32, (k * 13 + 5) % 32, 0)), GB.SETS.index((1, 2))), (ep(((k * 3 + 1) % 32,) * 3 + (2 + k % 6,)), four if k % 2 else rev))
    many = [k for k, pt in enumerate(patterns) if len(set(pt)) >= 2]
    for k in range(700):                                                   # seeded pairs: the 4D and the 2D route, both outcomes of each
        tab = int(rng.integers(0, 8))
        c = rng.integers(8, 24, 3) if k % 2 else rng.integers(0, 32, 3)   # the middle of the range seldom clamps
        a_base = int(rng.integers(8, 24)) if k % 2 else int(rng.integers(0, 32))
        add((ep((*c, min(tab, 3) if k % 2 else tab)), int(rng.choice(many))), (ep((a_base,) * 3 + (int(rng.integers(0, 4)) if k % 2 else int(rng.integers(0, 8)),)), int(rng.choice(many))))
    # The 4D route's `< .5f` fallback: the incremental estimate starts from the first texel's offset from the mean. Where that is zero in all four channels the axis stays
    # zero through every step, the normalised axis has length 0, and the fallback axis (.5, .5, .5, .5) is taken. So: colour and alpha blocks under patterns whose first
    # texel is the mean, nothing clamped away from it, and an end of a range at exactly 0 or 255 so that the block takes the 4D route at all. Seeded tries, kept where the
    # restatement says the fallback was taken.
    fallbacks, tries = 0, 0
    while fallbacks < 16 and tries < 20000:
        tries += 1
        tc, ta = (int(v) for v in rng.choice(sorted(mean_first), 2))
        ce, ae = (*(int(v) for v in rng.integers(0, 32, 3)), tc), (int(rng.integers(0, 32)),) * 3 + (ta,)
        cp, ap = mean_first[tc][int(rng.integers(len(mean_first[tc])))], mean_first[ta][int(rng.integers(len(mean_first[ta])))]
        _, _, d = V.pvrtc2_rgba_block(t, ce, np.array(cp), ae, np.array(ap))
        if d.get("axis_fallback"):
            fallbacks += 1
            add((ep(ce), pattern_at[cp]), (ep(ae), pattern_at[ap]))
    assert fallbacks >= 16, (fallbacks, tries)
    nbx = 31   # odd: every row of the coverage image ends in a lone left half
    while len(blocks) % nbx:
        add(blocks[-1], alphas[-1])
    n, nby = len(blocks), len(blocks) // nbx
    ep_pal, sel_pal = np.array(list(endpoints.keys()), np.uint8), np.array(patterns, np.uint8)
    be = E.backend_from_state(ep_pal, sel_pal, np.array([b[0] for b in blocks] + [b[0] for b in alphas]), np.array([b[1] for b in blocks] + [b[1] for b in alphas]),
                              [(0, nbx, nby, nbx * 4, nby * 4, 0, 0, 0), (n, nbx, nby, nbx * 4, nby * 4, 0, 0, 1)])
    be.encode()
    data = be.basis_file()
    be.close()
    arrays["file_coverage_basis"] = np.asarray(data, np.uint8).copy()
    dec = unpack_with_tool("coverage_basis", bytes(data), "basis", arrays)
    details = {}
    check_restatement("coverage_basis", dec, arrays, details)
    # what the file holds, from what it decodes to
    cov = {"blocks": n, "block_colour_values": len(values)}
    for short in ("atc", "fxt1", "pvrtc2"):
        entries = {d["entry"] for route, d in details[short] if route == "lookup"}
        solid = set()
        for route, d in details[short]:
            if route == "solid" and len(set(d["values"])) == 1:
                solid.add(d["values"][0])
        cov[short] = {"reachable": len(reach[short]), "covered": len(entries & set(reach[short])), "unreached": [list(v) for v in sorted(set(reach[short]) - entries)],
                      "solid_values": len(solid & set(values)), "outlier_blocks": sum(route == "outlier" for route, _ in details[short]),
                      "routes": {r: sum(route == r for route, _ in details[short]) for r in V.ROUTES}}
    guards, swaps = {}, {"swapped": 0, "kept": 0}
    for route, d in details["fxt1"]:
        swaps["swapped" if d["swapped"] else "kept"] += 1
        if d["guard"]:
            guards["_".join(d["guard"])] = guards.get("_".join(d["guard"]), 0) + 1
    cov["fxt1_green_lsb"], cov["fxt1_guards"], cov["fxt1_guard_candidates"] = swaps, guards, guard_candidates
    im = dec["images"][0]
    cov["fxt1_lone_left_halves"] = im["num_blocks_y"] if im["num_blocks_x"] % 2 else 0
    gates, constant_alphas = {}, set()
    for route, d in details["pvrtc2a"]:
        gates[d["gate"]] = gates.get(d["gate"], 0) + 1
        if d["gate"] in ("opaque", "constant_alpha"):
            constant_alphas.add(d.get("alpha", -1))
    pixels = [d for route, d in details["pvrtc2a"] if route == "pixels"]
    cov["pvrtc2a"] = {"gates": gates, "alpha_only_modulation": sum(d["alpha_only"] for d in pixels), "general_modulation": sum(not d["alpha_only"] for d in pixels),
                      "axis_fallback": sum(bool(d.get("axis_fallback")) for d in pixels), "err0_equals_err3": sum(bool(d.get("tie03")) for _, d in details["pvrtc2a"]),
                      "opaque_gate_alphas": sorted(a for a in constant_alphas if a >= 240), "tie_search": tie_search}
    # The writer moves a selector whose colour clamps onto its neighbour's to that neighbour, which changes the range: an entry may stay unreached only where every
    # colour that picks it has such a clamp
    for short in ("atc", "fxt1", "pvrtc2"):
        for tab, r, m in [tuple(v) for v in cov[short]["unreached"]]:
            assert not any(unclamped((*h, tab)) for h in reach[short][tab, r, m]), (short, tab, r, m)
    meta["files"].append({"name": "coverage_basis", "container": "basis", "has_alpha": True, "images": [[0, 0, 0, nbx * 4, nby * 4]]})
    meta["coverage"] = cov
    print("coverage:", json.dumps(cov), flush=True)
    for short in ("atc", "fxt1", "pvrtc2"):
        assert cov[short]["solid_values"] == len(values) and cov[short]["outlier_blocks"] >= 32, cov[short]
    assert min(swaps.values()) >= 100, swaps
    assert all(guards.get(k, 0) >= 1 for k in ("solid_zero", "solid_positive", "lookup_positive")), guards
    assert guards.get("lookup_zero", 0) >= 1 or guard_candidates["zero"] == 0, (guards, guard_candidates)
    pa = cov["pvrtc2a"]
    assert all(pa["gates"].get(g, 0) >= 8 for g in ("opaque", "early_err0", "early_alpha", "mode1", "mode0", "mode3", "solid_colour", "constant_alpha", "pca4d", "pca4d_swapped", "pca2d",
                                                     "pca2d_flipped")), pa
    assert pa["alpha_only_modulation"] >= 8 and pa["general_modulation"] >= 100 and {249, 250} <= set(pa["opaque_gate_alphas"]), pa
    assert pa["axis_fallback"] >= 12, pa
    assert pa["err0_equals_err3"] == 0 and tie_search["ties"] == 0, pa   # the gate listed as unreachable


if __name__ == "__main__":
    assert GG.BASISU.exists(), "oracle/_ref/basisu is missing: build it on the build machine (make -C oracle ref)"
    arrays, meta = {}, {"files": [], "targets": V.TAGS}
    reference_files(arrays, meta)
    coverage_member(arrays, meta)
    meta["table_digest"] = V.tables().digest()
    meta["unreachable"] = V.UNREACHABLE
    arrays["meta"] = np.frombuffer(json.dumps(meta, sort_keys=True).encode(), np.uint8)
    GG.save(V.GOLDEN, arrays)
    assert V.GOLDEN.stat().st_size <= 1 << 20, V.GOLDEN.stat().st_size
    print("wrote", V.GOLDEN, V.GOLDEN.stat().st_size, "bytes,", len(arrays), "members")
