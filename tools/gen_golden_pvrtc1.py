#!/usr/bin/env python3
"""Known answers of the PVRTC1 4bpp RGB / RGBA targets of both codecs from the real reference tool (oracle/_ref/basisu, build machine only; `make -C oracle ref`)
-> tests/golden/pvrtc1_vectors.npz.

Member 1, files compressed by the reference tool, each as ETC1S (-q 128) and as UASTC, each as .basis and as .ktx2 (UASTC .ktx2 without Zstandard):
    alpha    32x32 with an alpha ramp
    opaque   32x32 without alpha: PVRTC1_4_RGBA is answered with the RGB route
    wide     64x16 with mips down to 1x1, opaque      (non-square both ways; 4x1 and 1x4 pixels; the single block that is its own eight neighbours)
    tall     16x64 with mips down to 1x1, with alpha
    array    two layers of 16x16, the second with alpha
    cube     a 16x16 cubemap with alpha in one face
Member 2, `etc1s_coverage`: one image of 16x16 blocks whose palettes serve the colour AND the alpha slice, each slice with its own indices, written by this
    package's own backend writer. Rows 0-3 are solid black / white blocks with solid alpha 0 / 255 (colours every endpoint format holds exactly: dl == 0 with p > 0 and
    with p <= 0); the rest draws endpoints and selector patterns at random from palettes that hold every intensity table at base colours 0 and 31 (where the unclamped
    colour term leaves 0..48*255), single-selector patterns beside full ones, and alpha entries on both sides of 238 / 255. The seed is the first of 0..4095 under which
    the restatement counts the most of the three equalities p == 3 dl, 8 dl, 13 dl (dl > 0) in both ETC1S routes.
Member 3, `uastc_coverage`: 16x16 blocks: up to six of every one of the 19 modes from the encoder sets of uastc_transcode_vectors.npz, the rest random-bit blocks that
    unpack (uastc_transcode_fuzz.npz), in this package's own .ktx2 container (has_alpha set).
Per image the npz holds the raw blocks of `basisu -unpack -ktx_only`'s _transcoded_PVRTC1_4_RGB_* / _transcoded_PVRTC1_4_RGBA_* KTX files (key suffixes _rgb, _rgba);
every level's byte count is taken from the file and is blocks * 8. A file is accepted only after tests/pvrtc1_helpers.py's CPU restatement has reproduced every
block of it; what the restatement counted on the way goes into `meta`.
usage: gen_golden_pvrtc1.py"""
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
import pvrtc1_helpers as P  # noqa: E402
import transcode_helpers as T  # noqa: E402
import uastc_texture_helpers as U  # noqa: E402
import gen_golden_etc1s_transcode as GG  # noqa: E402  (the tool runner and the npz writer)
from basis_universal_amd.backend import uastc_ktx2_file  # noqa: E402
from basis_universal_amd.transcode import decode_etc1s_file, read_uastc_file  # noqa: E402


def ktx1_levels(path, faces):
    """the raw bytes of a KTX1 file, [face][level], each level as long as the file says (imageSize is one face's)"""
    raw = pathlib.Path(path).read_bytes()
    assert raw[:12] == bytes([0xAB, 0x4B, 0x54, 0x58, 0x20, 0x31, 0x31, 0xBB, 0x0D, 0x0A, 0x1A, 0x0A])
    n_faces, levels, kv = struct.unpack_from("<III", raw, 52)
    assert n_faces == faces and kv == 0, (n_faces, kv)
    at, out = 64, [[] for _ in range(faces)]
    for _ in range(levels):
        n = struct.unpack_from("<I", raw, at)[0]
        at += 4
        for f in range(faces):
            out[f].append(np.frombuffer(raw, np.uint8, n, at).copy())
            at += n
    assert at == len(raw)
    return out


def unpack_with_tool(name, data, ext, info, arrays):
    """runs the tool on one file and stores every image's PVRTC1 blocks as it wrote them"""
    with tempfile.TemporaryDirectory() as d:
        (pathlib.Path(d) / f"x.{ext}").write_bytes(bytes(data))
        GG.tool(["-unpack", "-ktx_only", f"x.{ext}"], d)
        by_image = {}
        for im in info["images"]:
            by_image.setdefault((im["layer"], im["face"]), []).append(im)
        for (layer, face), ims in by_image.items():
            ims.sort(key=lambda im: im["level"])
            for short, tag in P.TAGS.items():
                if ext == "basis" and info["faces"] == 6:
                    levels = ktx1_levels(pathlib.Path(d) / f"x_transcoded_cubemap_{tag}_{layer}.ktx", 6)[face]
                elif ext == "basis":
                    levels = ktx1_levels(pathlib.Path(d) / f"x_transcoded_{tag}_{layer:04d}.ktx", 1)[0]
                elif info["faces"] == 6:
                    levels = ktx1_levels(pathlib.Path(d) / f"x_transcoded_{tag}_face_{face}_layer_{layer:04d}.ktx", 1)[0]
                else:
                    levels = ktx1_levels(pathlib.Path(d) / f"x_transcoded_{tag}_layer_{layer:04d}.ktx", 1)[0]
                assert len(levels) == len(ims), (name, short, len(levels))
                for im, blocks in zip(ims, levels):
                    n = im["num_blocks_x"] * im["num_blocks_y"]
                    assert blocks.size == n * 8, (name, short, im["level"], blocks.size, n)   # no padding of tiny levels in what the tool writes
                    arrays[P.image_key(name, im["level"], layer, face) + "_" + short] = blocks.reshape(n, 8)


def restate(name, codec, data, arrays, stats):
    """every image of the file through the restatement, for both targets -> must equal what the tool wrote"""
    if codec == "etc1s":
        dec = decode_etc1s_file(data)
        for im in dec["images"]:
            for short, target in P.TARGETS.items():
                route = "etc1s_rgba" if target == P.RGBA and im["has_alpha"] else "etc1s_rgb"
                got = P.etc1s_image_blocks(dec, im, target, stats[route])
                want = arrays[P.image_key(name, im["level"], im["layer"], im["face"]) + "_" + short]
                bad = np.flatnonzero((got != want).any(1))
                assert bad.size == 0, (name, short, im["level"], bad[:8], got[bad[:2]], want[bad[:2]])
        return dec
    raw = bytes(data)
    info = read_uastc_file(raw)
    for im in info["images"]:
        blocks = np.frombuffer(raw, np.uint8, im["length"], im["offset"]).reshape(-1, 16)
        for short, target in P.TARGETS.items():
            eff = P.RGBA if target == P.RGBA and info["has_alpha"] else P.RGB
            got, invalid = P.uastc_blocks(blocks, im["num_blocks_x"], im["num_blocks_y"], eff, stats["uastc_rgba" if eff == P.RGBA else "uastc_rgb"])
            want = arrays[P.image_key(name, im["level"], im["layer"], im["face"]) + "_" + short]
            bad = np.flatnonzero((got != want).any(1))
            assert invalid == 0 and bad.size == 0, (name, short, im["level"], bad[:8], got[bad[:2]], want[bad[:2]])
    return info


def add_file(name, codec, ext, data, arrays, meta, stats):
    arrays["file_" + name] = np.frombuffer(bytes(data), np.uint8).copy()
    info = decode_etc1s_file(data) if codec == "etc1s" else read_uastc_file(bytes(data))
    unpack_with_tool(name, data, ext, info, arrays)
    restate(name, codec, data, arrays, stats)
    meta["files"].append({"name": name, "codec": codec, "container": ext, "has_alpha": bool(info["has_alpha"]),
                          "images": [[im["level"], im["layer"], im["face"], im["width"], im["height"]] for im in info["images"]]})
    return info


def ramp(img, seed):
    h, w = img.shape[:2]
    rng = np.random.default_rng(seed)
    out = img.copy()
    y, x = np.mgrid[0:h, 0:w]
    out[..., 3] = np.clip((x * 255) // max(w - 1, 1) + (y * 40) // max(h - 1, 1) - 20 + rng.integers(-6, 7, (h, w)), 0, 255).astype(np.uint8)
    return out


def reference_files(arrays, meta, stats):
    cube = [helpers.synth(16, 16, 130 + i) for i in range(6)]
    cube[2] = ramp(cube[2], 141)
    jobs = [("alpha", [ramp(helpers.synth(32, 32, 113), 7)], []), ("opaque", [helpers.synth(32, 32, 112)], []), ("wide", [helpers.synth(64, 16, 114)], ["-mipmap"]),
            ("tall", [ramp(helpers.synth(16, 64, 115), 8)], ["-mipmap"]),
            ("array", [helpers.synth(16, 16, 120), ramp(helpers.synth(16, 16, 121), 9)], ["-tex_type", "2darray"]), ("cube", cube, ["-tex_type", "cubemap"])]
    for name, imgs, args in jobs:
        for codec, cargs in (("etc1s", ["-q", "128"]), ("uastc", ["-uastc", "-ktx2_no_zstandard"])):
            counts = []
            for ext in ("basis", "ktx2"):
                with tempfile.TemporaryDirectory() as d:
                    pngs = []
                    for i, img in enumerate(imgs):
                        helpers.save_png(pathlib.Path(d) / f"in{i}.png", img)
                        pngs.append(f"in{i}.png")
                    GG.tool([f"-{ext}", *cargs, *args, *pngs, "-output_file", f"out.{ext}"], d)
                    data = (pathlib.Path(d) / f"out.{ext}").read_bytes()
                info = add_file(f"{codec}_{name}_{ext}", codec, ext, data, arrays, meta, stats)
                counts.append(len(info["images"]))
            print(name, codec, counts, "images", flush=True)


SEEDS = 4096   # how far the search for the three equalities goes
PATTERNS = [(s,) * 16 for s in range(4)] + [tuple((a, b)[k % 2] for k in range(16)) for a in range(4) for b in range(a + 1, 4)] + \
           [tuple(k % 4 for k in range(16)), tuple(3 - k % 4 for k in range(16)), tuple((k // 4) % 4 for k in range(16)), tuple((0, 1, 2)[k % 3] for k in range(16)),
            tuple((1, 2, 3)[k % 3] for k in range(16)), tuple((0, 3, 3, 0)[k % 4] for k in range(16))]


def coverage_state(seed):
    """-> (endpoint palette (n, 4), selector palette (n, 16), colour (endpoint idx, selector idx), alpha (endpoint idx, selector idx)) of a 16x16-block image"""
    rng = np.random.default_rng(1000 + seed)
    eps = []
    for tab in range(8):
        eps += [(0, 0, 0, tab), (31, 31, 31, tab), (1, 0, 2, tab), (30, 31, 29, tab), (29, 30, 31, tab)]
        eps += [tuple(int(v) for v in rng.integers(0, 32, 3)) + (tab,) for _ in range(3)]
    eps = np.array(eps, np.uint8)
    sels = np.array(PATTERNS + [tuple(int(v) for v in rng.integers(0, 4, 16)) for _ in range(10)], np.uint8)
    n = 256
    ei, si = rng.integers(0, eps.shape[0], n), rng.integers(0, sels.shape[0], n)
    aei, asi = rng.integers(0, eps.shape[0], n), rng.integers(0, sels.shape[0], n)
    # a third of the alpha blocks near the top of the range, where the two endpoints choose their formats on their own
    top = np.flatnonzero(eps[:, 1] >= 29)
    near = rng.random(n) < 0.35
    aei[near] = top[rng.integers(0, top.size, int(near.sum()))]
    # rows 0-3: solid black / white in 2x2-block tiles, alpha solid 0 / 255 in 4x2-block tiles
    black, white = 0, 1            # (0, 0, 0, 0) under selector 0 is 0; (31, 31, 31, 0) under selector 3 is 255
    for by in range(4):
        for bx in range(16):
            k = by * 16 + bx
            w, a = ((bx >> 1) + (by >> 1)) & 1, ((bx >> 2) + (by >> 1)) & 1
            ei[k], si[k] = (white, 3) if w else (black, 0)
            aei[k], asi[k] = (white, 3) if a else (black, 0)
    return eps, sels, (ei, si), (aei, asi)


def etc1s_coverage(arrays, meta, stats):
    best = None
    for seed in range(SEEDS):
        eps, sels, (ei, si), (aei, asi) = coverage_state(seed)
        words = (sels.astype(np.uint32) << (2 * np.arange(16, dtype=np.uint32))[None, :]).sum(1).astype(np.uint32)
        hits = 0
        for target in (P.RGB, P.RGBA):
            s = P.new_stats()
            P.etc1s_state_blocks(eps, words, ei, si, aei, asi, 16, 16, target, s)
            hits += sum(1 for k in (3, 8, 13) if s[f"p_equals_{k}dl"])
        if best is None or hits > best[0]:
            best = (hits, seed)
        if hits == 6:
            break
    hits, seed = best
    eps, sels, (ei, si), (aei, asi) = coverage_state(seed)
    n = 256
    be = E.backend_from_state(eps, sels, np.concatenate([ei, aei]), np.concatenate([si, asi]), [(0, 16, 16, 64, 64, 0, 0, 0), (n, 16, 16, 64, 64, 0, 0, 1)])
    be.encode()
    data = be.basis_file()
    be.close()
    own = {"etc1s_rgb": P.new_stats(), "etc1s_rgba": P.new_stats()}
    info = add_file("etc1s_coverage_basis", "etc1s", "basis", np.asarray(data, np.uint8).tobytes(), arrays, meta, own)
    assert info["images"][0]["has_alpha"]
    tables = {int(t) for t in info["endpoint_palette"][np.concatenate([info["images"][0]["endpoint_indices"].reshape(-1), info["images"][0]["alpha_endpoint_indices"].reshape(-1)]), 3]}
    assert tables == set(range(8)), tables
    meta["etc1s_coverage"] = {"seed": seed, "equalities_in_the_state": hits, "seeds_tried": seed + 1, "stats": own}
    for route, s in own.items():
        merge(stats[route], s)
    print("etc1s coverage: seed", seed, {r: {k: s[k] for k in ("p_equals_3dl", "p_equals_8dl", "p_equals_13dl", "dl_zero_p_positive", "dl_zero_p_not_positive", "ca_above_cb")}
                                         for r, s in own.items()}, flush=True)


def merge(into, s):
    for k, v in s.items():
        if isinstance(v, dict):
            for kk, vv in v.items():
                into[k][kk] += vv
        elif isinstance(v, list):
            into[k] = [a + b for a, b in zip(into[k], v)]
        else:
            into[k] += v


def uastc_coverage(arrays, meta, stats):
    sets = np.concatenate([U.encoder_grid(name)[0] for name in U.ENCODER_SETS])
    modes = T.code_modes(sets)
    picked = []
    for m in range(19):
        idx = np.flatnonzero(modes == m)
        assert idx.size >= 1, m
        picked.append(sets[idx[np.unique(np.linspace(0, idx.size - 1, 6).astype(int))]])
    grid, _, _, n_valid, _ = U.fuzz_valid_grid()
    fuzz = grid[:n_valid]
    fill = 256 - sum(p.shape[0] for p in picked)
    assert n_valid >= fill
    blocks = np.concatenate(picked + [fuzz[np.linspace(0, n_valid - 1, fill).astype(int)]])
    rng = np.random.default_rng(77)
    blocks = np.ascontiguousarray(blocks[rng.permutation(256)])
    data = uastc_ktx2_file(blocks, [(0, 16, 16, 64, 64, 0, 0, 1)], srgb=False, has_alpha=True)
    add_file("uastc_coverage_ktx2", "uastc", "ktx2", data.tobytes(), arrays, meta, stats)
    meta["uastc_coverage"] = {"blocks_per_mode": [int(p.shape[0]) for p in picked], "random_bit_blocks": int(fill)}
    print("uastc coverage: 256 blocks", flush=True)


if __name__ == "__main__":
    assert GG.BASISU.exists(), "oracle/_ref/basisu is missing: build it on the build machine (make -C oracle ref)"
    arrays, meta = {}, {"files": [], "targets": P.TAGS}
    stats = {r: P.new_stats() for r in ("etc1s_rgb", "etc1s_rgba", "uastc_rgb", "uastc_rgba")}
    reference_files(arrays, meta, stats)
    etc1s_coverage(arrays, meta, stats)
    uastc_coverage(arrays, meta, stats)
    meta["stats"] = stats
    for route, s in stats.items():
        print(route, s, flush=True)
    arrays["meta"] = np.frombuffer(json.dumps(meta, sort_keys=True).encode(), np.uint8)
    GG.save(P.GOLDEN, arrays)
    assert P.GOLDEN.stat().st_size <= 256 << 10, P.GOLDEN.stat().st_size
    print("wrote", P.GOLDEN, P.GOLDEN.stat().st_size, "bytes,", len(arrays), "members")
