#!/usr/bin/env python3
"""Known answers of the UASTC LDR 4x4 transcoder from the real reference (oracle/_ref, build machine only):
  tests/golden/uastc_transcode_vectors.npz      committed UASTC block sets (uastc_reference_vectors.npz level3 / level2, uastc_rdo_vectors.npz default_l2) laid out as
                                                64-block-wide grids (tail padded with a solid block), and per set what the reference makes of them for every target
  tests/golden/uastc_transcode_big_digests.json the 4096x4096 synthetic image's level-2 blocks (pinned by uastc_big_digests.json): one sha256 per 65,536-block chunk
                                                of every target's output
How: the blocks are wrapped into a .ktx2 with this package's own writer (backend.uastc_ktx2_file, host code), `basisu -unpack -ktx_only` (and again with
-higher_quality_transcoding) transcodes it, and the raw blocks are read back out of the .ktx files it writes (68 bytes of KTX1 header + imageSize, then the
blocks in raster order). RGBA32 is not written under -ktx_only: it comes from the harness's unpack_uastc. The tool's BC4 is channel 0 and its BC5 channels 0 and 3.
  tests/golden/uastc_transcode_fuzz.npz         blocks no encoder writes (transcode_helpers.fuzz_families: random bits stratified by mode, every BC1 hint setting,
                                                trit / quint groups past their radix, degenerate endpoints, solid blocks with junk after the colour, invalid blocks)
                                                with the reference's validity flag and output for every target, from the harness's ref_transcode_uastc (version 3)
usage: gen_golden_uastc_transcode.py [vectors] [big] [fuzz]   (default: vectors and big; `big` spends about a minute encoding with the reference)"""
import hashlib
import json
import pathlib
import subprocess
import sys
import tempfile

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests"))
sys.path.insert(0, str(ROOT))
import helpers  # noqa: E402
import transcode_helpers as T  # noqa: E402
from basis_universal_amd.backend import uastc_ktx2_file  # noqa: E402

GOLDEN = ROOT / "tests" / "golden"
BASISU = ROOT / "oracle" / "_ref" / "basisu"
GRID_W = 64
CHUNK = 65536
# output name -> (the tool's file tag, bytes per block, high quality run)
TOOL = {"astc": ("ASTC_LDR_4X4_RGBA", 16, False), "bc7": ("BC7_RGBA", 16, False), "bc1": ("BC1_RGB", 8, False), "bc1_hq": ("BC1_RGB", 8, True),
        "bc3": ("BC3_RGBA", 16, False), "bc3_hq": ("BC3_RGBA", 16, True), "bc4_r": ("BC4_R", 8, False), "bc5_ra": ("BC5_RG", 16, False)}


def reference_transcode(blocks, nbx, nby):
    """{output name: (n, bytes) u8} for an nbx x nby grid of UASTC blocks"""
    n = nbx * nby
    assert blocks.shape == (n, 16)
    data = uastc_ktx2_file(blocks, [(0, nbx, nby, nbx * 4, nby * 4, 0, 0, 1)], srgb=False, has_alpha=True)
    out = {}
    for hq in (False, True):
        with tempfile.TemporaryDirectory() as d:
            (pathlib.Path(d) / "x.ktx2").write_bytes(data.tobytes())
            cmd = [str(BASISU), "-unpack", "-ktx_only", "-no_multithreading"] + (["-higher_quality_transcoding"] if hq else []) + ["x.ktx2"]
            r = subprocess.run(cmd, cwd=d, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
            assert r.returncode == 0, r.stdout[-2000:]
            for name, (tag, bpb, want_hq) in TOOL.items():
                if want_hq != hq:
                    continue
                raw = (pathlib.Path(d) / f"x_transcoded_{tag}_layer_0000.ktx").read_bytes()
                assert len(raw) == 68 + n * bpb, (name, len(raw))
                assert int.from_bytes(raw[64:68], "little") == n * bpb
                out[name] = np.frombuffer(raw[68:], np.uint8).reshape(n, bpb).copy()
    out["rgba32"] = helpers.ref_decode_uastc(blocks).reshape(n, 64)
    return out


def gen_vectors():
    ref = np.load(GOLDEN / "uastc_reference_vectors.npz")
    rdo = np.load(GOLDEN / "uastc_rdo_vectors.npz")
    sets = {"level3": ref["level3"], "level2": ref["level2"], "default_l2": rdo["default_l2"]}
    arrays, modes_seen, routes = {}, np.zeros(19, np.int64), {}
    for name, blocks in sets.items():
        blocks = np.ascontiguousarray(blocks, np.uint8).reshape(-1, 16)
        modes = T.block_modes(blocks)
        solid = blocks[np.flatnonzero(modes == 8)[0]]
        nby = -(-blocks.shape[0] // GRID_W)
        grid = np.concatenate([blocks, np.repeat(solid[None], GRID_W * nby - blocks.shape[0], 0)])
        modes_seen += np.bincount(modes, minlength=19)[:19]
        r = T.bc1_routes(blocks)
        r = r[r != 0]
        routes[name] = (int(((r & 2) != 0).sum()), int(((r & 6) == 4).sum()), int(((r & 6) == 0).sum()))
        arrays[f"{name}_blocks"] = grid
        arrays[f"{name}_grid"] = np.array([GRID_W, nby, blocks.shape[0]], np.uint32)
        for k, v in reference_transcode(grid, GRID_W, nby).items():
            arrays[f"{name}_{k}"] = v
        print(name, blocks.shape[0], "blocks, BC1 routes hint0 / hint1 / neither:", routes[name], flush=True)
    assert (modes_seen > 0).all(), modes_seen
    assert all(min(v) >= 100 for v in routes.values()), routes
    p = GOLDEN / "uastc_transcode_vectors.npz"
    helpers_save(p, arrays)
    print("wrote", p, p.stat().st_size, "bytes; blocks per mode", modes_seen.tolist())


def helpers_save(path, arrays):
    """np.savez_compressed with fixed member timestamps, so that a rerun rewrites the file byte for byte"""
    import io
    import zipfile
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for k in sorted(arrays):
            buf = io.BytesIO()
            np.save(buf, arrays[k])
            z.writestr(zipfile.ZipInfo(k + ".npy", (1980, 1, 1, 0, 0, 0)), buf.getvalue(), zipfile.ZIP_DEFLATED, 9)


def gen_big():
    pinned = json.loads((GOLDEN / "uastc_big_digests.json").read_text())["synth4096_l2"]
    packed = helpers.ref_encode_uastc(helpers.to_pixel_blocks(helpers.synth(4096, 4096, 1234)), 2)
    assert hashlib.sha256(packed.tobytes()).hexdigest() == pinned["sha256"]
    out = {"width": 4096, "height": 4096, "seed": 1234, "flags": 2, "n_blocks": int(packed.shape[0]), "chunk_blocks": CHUNK, "source_sha256": pinned["sha256"], "targets": {}}
    for k, v in reference_transcode(packed, 1024, 1024).items():
        out["targets"][k] = {"bytes_per_block": int(v.shape[1]), "chunk_sha256": [hashlib.sha256(v[i:i + CHUNK].tobytes()).hexdigest() for i in range(0, v.shape[0], CHUNK)]}
        print(k, out["targets"][k]["chunk_sha256"][0], flush=True)
    p = GOLDEN / "uastc_transcode_big_digests.json"
    p.write_text(json.dumps({"synth4096_l2": out}, indent=1, sort_keys=True) + "\n")
    print("wrote", p)


def gen_fuzz():
    assert helpers.ref_harness_version() >= 3, "oracle/_ref/libref_harness.so has no ref_transcode_uastc: rebuild it (make -C oracle ref)"
    fam, cause, drawn = T.fuzz_families()
    blocks = np.concatenate([fam[k] for k in T.FAMILIES])
    family = np.concatenate([np.full(fam[k].shape[0], i, np.uint8) for i, k in enumerate(T.FAMILIES)])
    arrays = {"blocks": blocks, "family": family, "invalid_cause": cause}
    for name, (target, hq, ch) in T.FUZZ_CASES.items():
        out, ok = helpers.ref_transcode_uastc(blocks, target, hq, ch)
        if "valid" in arrays:
            assert (ok == arrays["valid"]).all(), f"the reference's {name} transcoder refuses other blocks than its unpack_uastc"
        else:
            arrays["valid"] = ok
        assert (out[ok == 0] == 0).all()
        arrays[name] = out
    valid = arrays["valid"]
    per_mode, routes = T.check_fuzz_coverage(blocks, family, valid, cause, T.FUZZ_QUOTA)
    # the reference's own view of the uniformly random draw the `random` families come from
    drawn_blocks = T.random_bit_blocks(((drawn + 1023) // 1024) * 1024, T.FUZZ_SEED)[:drawn]
    drawn_ok = helpers.ref_transcode_uastc(drawn_blocks, T.RGBA32)[1] != 0
    drawn_modes = np.bincount(T.code_modes(drawn_blocks)[drawn_ok], minlength=19)[:19]
    assert int((~drawn_ok).sum()) == fam["random_invalid"].shape[0]
    meta = {"seed": T.FUZZ_SEED, "quota": T.FUZZ_QUOTA, "families": list(T.FAMILIES), "invalid_causes": list(T.INVALID_CAUSES), "blocks": int(blocks.shape[0]),
            "valid_by_reference": int(valid.sum()), "valid_per_mode": per_mode.tolist(), "bc1_routes_hint0_hint1_neither": list(routes),
            "random_drawn": int(drawn), "random_drawn_valid_by_reference": int(drawn_ok.sum()), "random_drawn_valid_per_mode": drawn_modes.tolist()}
    arrays["meta"] = np.frombuffer(json.dumps(meta, sort_keys=True).encode(), np.uint8)
    p = GOLDEN / "uastc_transcode_fuzz.npz"
    helpers_save(p, arrays)
    assert p.stat().st_size <= 1 << 20, p.stat().st_size
    print("wrote", p, p.stat().st_size, "bytes")
    print(json.dumps(meta, indent=1, sort_keys=True))
    print(f"uniformly random draw: {drawn} blocks, {100.0 * drawn_ok.mean():.2f} % valid according to the reference")


if __name__ == "__main__":
    what = sys.argv[1:] or ["vectors", "big"]
    if "vectors" in what:
        gen_vectors()
    if "big" in what:
        gen_big()
    if "fuzz" in what:
        gen_fuzz()
