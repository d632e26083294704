#!/usr/bin/env python3
"""Known answers of the ETC1S transcoder from the real reference tool (oracle/_ref/basisu, build machine only) -> tests/golden/etc1s_transcode_vectors.npz.

Member 1, files: tiny images compressed by the reference tool, each as .basis and as .ktx2 --
    64x64 and 20x28 opaque at quality 1 / 128 / 255, 32x24 with alpha, 20x28 with a mip chain down to 1x1 (its levels are 5x7, 3x4, 2x2, 1x1 and 1x1 blocks; level 2 is
    5x7 pixels), a 2-layer array and a cubemap of 16x16 images.
Member 2, coverage: a synthetic ETC1S state (palettes + indices) in which every intensity table x selector range x selector mapping combination of the ETC1S -> BC1
    conversion that any colour can reach occurs, plus solid blocks and the two-colour blocks of the widest table; wrapped into a .basis file by this package's own
    backend writer (host code). The combinations are counted on what the file decodes to and the counts go into `meta`.
Per image the npz holds what `basisu -unpack -ktx_only` makes of it: the raw blocks out of the _transcoded_{ETC1_RGB,BC1_RGB}_*.ktx files (a 64-byte KTX1 header, then
per mip level a 4-byte size and the blocks in raster order). -ktx_only writes no pixel formats: their expected value is the ETC1 output decoded by the format definition
(tests/etc1s_transcode_helpers.py); the alpha plane of the alpha file is taken from the RGBA32 .png a second, plain -unpack run writes, whose colour is checked against
that decode here.
usage: gen_golden_etc1s_transcode.py"""
import io
import json
import pathlib
import struct
import subprocess
import sys
import tempfile
import zipfile
import zlib

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests"))
sys.path.insert(0, str(ROOT / "tools"))
sys.path.insert(0, str(ROOT))
import helpers  # noqa: E402
import etc1s_transcode_helpers as E  # noqa: E402
import gen_etc1s_transcode_tables as G  # noqa: E402
from basis_universal_amd.transcode import decode_etc1s_file  # noqa: E402

BASISU = ROOT / "oracle" / "_ref" / "basisu"
TAGS = {"etc1": "ETC1_RGB", "bc1": "BC1_RGB"}


def tool(args, cwd):
    r = subprocess.run([str(BASISU), "-no_multithreading", *args], cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-2000:]


def read_png(path):
    """8-bit RGB / RGBA, non-interlaced -> (h, w, channels) u8"""
    raw = pathlib.Path(path).read_bytes()
    assert raw[:8] == b"\x89PNG\r\n\x1a\n"
    at, idat, w = 8, b"", 0
    while at < len(raw):
        n, tag = struct.unpack_from(">I4s", raw, at)
        body = raw[at + 8:at + 8 + n]
        if tag == b"IHDR":
            w, h, depth, ctype, _, _, interlace = struct.unpack(">IIBBBBB", body)
            assert depth == 8 and ctype in (2, 6) and not interlace
            ch = 3 if ctype == 2 else 4
        elif tag == b"IDAT":
            idat += body
        at += 12 + n
    data = zlib.decompress(idat)
    stride = w * ch
    out = np.zeros((h, stride), np.int64)
    for y in range(h):
        f = data[y * (stride + 1)]
        line = np.frombuffer(data, np.uint8, stride, y * (stride + 1) + 1).astype(np.int64)
        up = out[y - 1] if y else np.zeros(stride, np.int64)
        cur = np.zeros(stride, np.int64)
        for x in range(stride):
            a = cur[x - ch] if x >= ch else 0
            c = up[x - ch] if x >= ch else 0
            b = up[x]
            if f == 0: p = 0
            elif f == 1: p = a
            elif f == 2: p = b
            elif f == 3: p = (a + b) // 2
            else:
                pa, pb, pc = abs(b - c), abs(a - c), abs(a + b - 2 * c)
                p = a if (pa <= pb and pa <= pc) else (b if pb <= pc else c)
            cur[x] = (line[x] + p) & 255
        out[y] = cur
    return out.astype(np.uint8).reshape(h, w, ch)


def ktx1_levels(path, sizes, faces=1):
    """the raw blocks of a KTX1 file, [face][level]; sizes: blocks per level. A level is a 4-byte size (of one face) and then the faces' blocks in raster order."""
    raw = pathlib.Path(path).read_bytes()
    assert raw[:12] == bytes([0xAB, 0x4B, 0x54, 0x58, 0x20, 0x31, 0x31, 0xBB, 0x0D, 0x0A, 0x1A, 0x0A])
    n_faces, levels, kv = struct.unpack_from("<III", raw, 52)
    assert n_faces == faces and levels == len(sizes) and kv == 0, (n_faces, levels, kv)
    at, out = 64, [[] for _ in range(faces)]
    for n in sizes:
        assert struct.unpack_from("<I", raw, at)[0] == n * 8
        at += 4
        for f in range(faces):
            out[f].append(np.frombuffer(raw, np.uint8, n * 8, at).reshape(n, 8).copy())
            at += n * 8
    assert at == len(raw)
    return out


def unpack_with_tool(name, data, ext, arrays):
    """runs the tool on one file and stores every image's ETC1 and BC1 blocks; returns the decoded file (this package's host decoder)"""
    dec = decode_etc1s_file(data)
    with tempfile.TemporaryDirectory() as d:
        (pathlib.Path(d) / f"x.{ext}").write_bytes(bytes(data))
        tool(["-unpack", "-ktx_only", f"x.{ext}"], d)
        by_image = {}
        for im in dec["images"]:
            by_image.setdefault((im["layer"], im["face"]), []).append(im)
        for (layer, face), ims in by_image.items():
            ims.sort(key=lambda im: im["level"])
            sizes = [im["num_blocks_x"] * im["num_blocks_y"] for im in ims]
            for short, tag in TAGS.items():
                if ext == "basis" and dec["faces"] == 6:   # a .basis cubemap is unpacked into one KTX1 cubemap per layer
                    levels = ktx1_levels(pathlib.Path(d) / f"x_transcoded_cubemap_{tag}_{layer}.ktx", sizes, 6)[face]
                elif ext == "basis":
                    levels = ktx1_levels(pathlib.Path(d) / f"x_transcoded_{tag}_{layer:04d}.ktx", sizes)[0]
                elif dec["faces"] == 6:
                    levels = ktx1_levels(pathlib.Path(d) / f"x_transcoded_{tag}_face_{face}_layer_{layer:04d}.ktx", sizes)[0]
                else:
                    levels = ktx1_levels(pathlib.Path(d) / f"x_transcoded_{tag}_layer_{layer:04d}.ktx", sizes)[0]
                for im, blocks in zip(ims, levels):
                    arrays[E.image_key(name, im["level"], layer, face) + "_" + short] = blocks
    return dec


def reference_files(arrays, meta):
    rng_img = {"o64": helpers.synth(64, 64, 11), "o20": helpers.synth(20, 28, 12)}
    alpha_img = helpers.synth(32, 24, 13)
    alpha_img[..., 3] = np.clip(np.mgrid[0:24, 0:32][1] * 8 + np.mgrid[0:24, 0:32][0] * 3, 0, 255).astype(np.uint8)
    jobs = []   # (name, [images], tool args)
    for k, img in rng_img.items():
        for q in (1, 128, 255):
            jobs.append((f"{k}_q{q}", [img], ["-q", str(q)]))
    jobs.append(("alpha", [alpha_img], ["-q", "128"]))
    jobs.append(("mip", [rng_img["o20"]], ["-q", "128", "-mipmap"]))
    jobs.append(("array", [helpers.synth(16, 16, 20), helpers.synth(16, 16, 21)], ["-q", "128", "-tex_type", "2darray"]))
    jobs.append(("cube", [helpers.synth(16, 16, 30 + i) for i in range(6)], ["-q", "128", "-tex_type", "cubemap"]))
    for name, imgs, args in jobs:
        decs = {}
        for ext in ("basis", "ktx2"):
            with tempfile.TemporaryDirectory() as d:
                pngs = []
                for i, img in enumerate(imgs):
                    helpers.save_png(pathlib.Path(d) / f"in{i}.png", img)
                    pngs.append(f"in{i}.png")
                tool([f"-{ext}", *args, *pngs, "-output_file", f"out.{ext}"], d)
                data = (pathlib.Path(d) / f"out.{ext}").read_bytes()
                if name == "alpha" and ext == "ktx2":
                    tool(["-unpack", f"out.{ext}"], d)
                    png = read_png(pathlib.Path(d) / "out_unpacked_rgba_RGBA32_level_0_face_0_layer0000.png")
            full = f"{name}_{ext}"
            arrays["file_" + full] = np.frombuffer(data, np.uint8).copy()
            decs[ext] = unpack_with_tool(full, data, ext, arrays)
            meta["files"].append({"name": full, "container": ext, "images": [[im["level"], im["layer"], im["face"], im["width"], im["height"]] for im in decs[ext]["images"]]})
        # both containers hold the same slices
        for a, b in zip(decs["basis"]["images"], decs["ktx2"]["images"]):
            ka, kb = E.image_key(f"{name}_basis", a["level"], a["layer"], a["face"]), E.image_key(f"{name}_ktx2", b["level"], b["layer"], b["face"])
            assert (arrays[ka + "_etc1"] == arrays[kb + "_etc1"]).all() and (arrays[ka + "_bc1"] == arrays[kb + "_bc1"]).all(), name
        if name == "alpha":
            rgb = E.decode_etc1_blocks(arrays[E.image_key("alpha_ktx2", 0, 0, 0) + "_etc1"], 8, 6)
            assert png.shape == (24, 32, 4) and (png[..., :3] == rgb).all(), "the tool's RGBA32 colour is not its ETC1 output decoded"
            for ext in ("basis", "ktx2"):
                arrays[E.image_key(f"alpha_{ext}", 0, 0, 0) + "_alpha"] = png[..., 3].copy()
        print(name, [len(d["images"]) for d in decs.values()], "images", flush=True)


def bc1_route(tab5, tab6, ep, sel16):
    """which path of the ETC1S -> BC1 conversion a block takes: ("solid",) / ("two",) / (table, range, mapping)"""
    used = sorted(set(int(s) for s in sel16))
    lo, hi = used[0], used[-1]
    if lo == hi:
        return ("solid",)
    if ep[3] >= 7 and len(used) == 2 and lo == 0 and hi == 3:
        return ("two",)
    r = E.BC1_RANGES.index((lo, hi))
    err = sum((t[int(ep[3]), int(c), r, :] >> 16).astype(np.int64) for t, c in ((tab5, ep[0]), (tab6, ep[1]), (tab5, ep[2])))
    return (int(ep[3]), r, int(err.argmin()))


def coverage_member(arrays, meta):
    tab5, tab6 = G.endpoint_table(5).reshape(8, 32, 6, 10), G.endpoint_table(6).reshape(8, 32, 6, 10)
    e5, e6 = (tab5 >> 16).astype(np.int64), (tab6 >> 16).astype(np.int64)
    c = np.arange(32)
    rng = np.random.default_rng(77)
    endpoints, blocks, reachable = {}, [], 0
    sel_patterns = [tuple((lo + (k % (hi - lo + 1))) for k in range(16)) for lo, hi in E.BC1_RANGES] + [(s,) * 16 for s in range(4)] + [tuple(3 * ((k * 7 // 3) & 1) for k in range(16))]

    def ep_index(e):
        return endpoints.setdefault(tuple(int(v) for v in e), len(endpoints))
    for t in range(8):
        for r in range(6):
            total = e5[t, :, r, :][:, None, None, :] + e6[t, :, r, :][None, :, None, :] + e5[t, :, r, :][None, None, :, :]   # [r5][g5][b5][mapping]
            best = total.argmin(3)
            for m in range(10):
                hits = np.argwhere(best == m)
                if not hits.size:
                    continue
                reachable += 1
                for pick in hits[rng.choice(hits.shape[0], min(2, hits.shape[0]), replace=False)]:
                    blocks.append((ep_index((pick[0], pick[1], pick[2], t)), r))
    for t in range(8):          # solid blocks of every selector, two-colour blocks (only table 7 takes that path; the others go through the tables)
        for k in range(6):
            e = ep_index((*rng.integers(0, 32, 3), t)) if k else ep_index((31 * (t & 1), 31 * (t & 1), 31 * (t & 1), t))
            for s in range(4):
                blocks.append((e, 6 + s))
            blocks.append((e, 10))
    ep_pal = np.array(list(endpoints.keys()), np.uint8)
    sel_pal = np.array(sel_patterns, np.uint8)
    nbx = 32
    while len(blocks) % nbx:
        blocks.append(blocks[-1])
    nby = len(blocks) // nbx
    ei, si = np.array([b[0] for b in blocks]), np.array([b[1] for b in blocks])
    be = E.backend_from_state(ep_pal, sel_pal, ei, si, [(0, nbx, nby, nbx * 4, nby * 4, 0, 0, 0)])
    be.encode()
    data = be.basis_file()
    be.close()
    arrays["file_coverage_basis"] = np.asarray(data, np.uint8).copy()
    dec = unpack_with_tool("coverage_basis", bytes(data), "basis", arrays)
    im = dec["images"][0]
    sel16 = (dec["selector_palette"][:, None] >> (2 * np.arange(16))[None, :]) & 3
    routes = {}
    for e, s in zip(im["endpoint_indices"].reshape(-1), im["selector_indices"].reshape(-1)):
        k = bc1_route(tab5, tab6, dec["endpoint_palette"][e], sel16[s])
        routes[k] = routes.get(k, 0) + 1
    covered = sum(1 for k in routes if len(k) == 3)
    tables_seen = sorted({k[0] for k in routes if len(k) == 3})
    pairs_seen = sorted({(k[1], k[2]) for k in routes if len(k) == 3})
    assert covered == reachable, (covered, reachable)
    assert tables_seen == list(range(8)) and routes.get(("solid",), 0) >= 100 and routes.get(("two",), 0) >= 4
    meta["files"].append({"name": "coverage_basis", "container": "basis", "images": [[0, 0, 0, nbx * 4, nby * 4]]})
    meta["coverage"] = {"blocks": len(blocks), "table_range_mapping_reachable": reachable, "table_range_mapping_covered": covered, "table_range_mapping_total": 8 * 6 * 10,
                        "range_mapping_pairs_covered": len(pairs_seen), "solid_blocks": routes.get(("solid",), 0), "two_colour_blocks": routes.get(("two",), 0)}
    print("coverage:", meta["coverage"], flush=True)


def save(path, arrays):
    """np.savez_compressed with fixed member timestamps, so that a rerun rewrites the file byte for byte"""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for k in sorted(arrays):
            buf = io.BytesIO()
            np.save(buf, arrays[k])
            z.writestr(zipfile.ZipInfo(k + ".npy", (1980, 1, 1, 0, 0, 0)), buf.getvalue(), zipfile.ZIP_DEFLATED, 9)


if __name__ == "__main__":
    assert BASISU.exists(), "oracle/_ref/basisu is missing: build it on the build machine (make -C oracle ref)"
    arrays, meta = {}, {"files": [], "targets": TAGS}
    reference_files(arrays, meta)
    coverage_member(arrays, meta)
    arrays["meta"] = np.frombuffer(json.dumps(meta, sort_keys=True).encode(), np.uint8)
    save(E.GOLDEN, arrays)
    assert E.GOLDEN.stat().st_size <= 1 << 20, E.GOLDEN.stat().st_size
    print("wrote", E.GOLDEN, E.GOLDEN.stat().st_size, "bytes,", len(arrays), "members")
