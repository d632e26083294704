#!/usr/bin/env python3
"""Known answers of the texture unpacker from the real reference (oracle/_ref/libref_harness.so and oracle/_ref/basisu, build machine only; `make -C oracle ref`)
-> tests/golden/texture_unpack_vectors.npz.

Block by block, as tools/gen_golden_block_unpack.py does it: basisu::unpack_block(texture_format, const void*, color_rgba*, bool astc_srgb = false) through ctypes,
one block at a time into 16 texels pre-filled with (0, 0, 0, 255); the texture_format values are read from transcoder/basisu.h. Per member `<name>_blocks`
(n, 8 | 16) u8, `<name>_texels` (n, 16, 4) u8 as the reference left them (for a block it refuses: whatever it left; only `ok` and the zero fill are compared there)
and `<name>_ok` (n,) u8, its return value. Everything from one fixed seed through PCG64's raw stream.

  etc1           256 random-bit blocks without the overflow cases, then 64 differential blocks whose deltas are -4 or +3 in every channel without overflow
  etc1_overflow  64 differential blocks whose second base leaves 0..31: 16 each with red, green, blue below 0 and with any channel above 31. All refused
  etc2           256 random-bit blocks whose colour half is valid (the first 16: multiplier 0, multiplier 15, base 0, base 255, four each), then 32 whose colour
                 half overflows (refused)
  r11, rg11      256 random-bit blocks each; the first 24 (rg11: in both halves): base 0 and base 255 under multiplier 15 (both clamps), multiplier 0
  astc           every block accepted: block mode, partition count, endpoint mode(s) and dual-plane fields forced into random bits over the whole parameter space
                 of a 4x4 footprint (grid 2x2..4x4, the twelve weight ranges, 1-4 partitions, two planes, one CEM or one per partition), the first 1024 the reference
                 accepts and then those of a class that still lacks blocks; then 32 void-extent blocks (16 with all-ones extents, 16 with ordered ones)
  astc_refused   256 blocks the reference refuses: 216 raw random-bit blocks; 8 each of the forced-mode candidates it refuses for an HDR endpoint mode, for too
                 few bits for the endpoint values, for weight bits out of range and for four partitions with two planes; 8 HDR void extents
  uastc_*, etc1s_*   the first 512 blocks of what this package's transcoders write (texture_unpack_helpers.ENCODER_MADE)
  pvrtc1_<image>_<rgb|rgba>_texels   the `_unpacked_rgb*_PVRTC1_4_RGB*_*.png` rasters `basisu -unpack` writes for files of tests/golden/pvrtc1_vectors.npz, whose
                 blocks are the inputs (not stored again): (h, w, 3) where the tool writes no alpha, else (h, w, 4)
  pvrtc1_random_<nbx>x<nby>_blocks / _texels   random-bit PVRTC1 images (Morton order) of BOTH modulation modes. Their texels are NOT a run of the reference:
                 they come from the Python restatement of get_pixel in tests/texture_unpack_helpers.py, which first has to reproduce every tool-made raster above
`meta` records the counts (texture_unpack_helpers.check_coverage, asserted here before writing and by tests/test_texture_unpack_host.py on the committed file) and
whether the reference's unpack of the UASTC-made ASTC blocks equals its RGBA32 transcode of the same UASTC blocks.
usage: gen_golden_texture_unpack.py"""
import ctypes as C
import json
import pathlib
import re
import subprocess
import sys
import tempfile

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests"))
sys.path.insert(0, str(ROOT / "tools"))
import helpers  # noqa: E402
import texture_unpack_helpers as X  # noqa: E402
import gen_golden_block_unpack as GB  # noqa: E402  (Bits, put)
import gen_golden_etc1s_transcode as GG  # noqa: E402  (the tool runner and the PNG reader)
import gen_golden_image_stats as S  # noqa: E402  (the npz writer)

HARNESS = ROOT / "oracle" / "_ref" / "libref_harness.so"
SEED = 20261021
MAX_BYTES = 731308   # the largest transcode fixture already committed (uastc_transcode_vectors.npz)
REF_NAMES = {X.ETC1: "cETC1", X.ETC2: "cETC2_RGBA", X.R11: "cETC2_R11_EAC", X.RG11: "cETC2_RG11_EAC", X.ASTC: "cASTC_LDR_4x4"}
ASTC_ACCEPTED = 1024   # accepted ASTC candidates kept whatever their class; more are kept while a class of check_coverage lacks blocks
put = GB.put


def reference_formats():
    """basisu::texture_format's values, counted from the enum in the reference's header"""
    text = (helpers.REF_DIR / "transcoder" / "basisu.h").read_text()
    body = re.search(r"enum class texture_format\s*\{(.*?)\}", text, re.S).group(1)
    body = re.sub(r"//[^\n]*", "", body)
    values, nxt = {}, 0
    for item in body.split(","):
        item = item.strip()
        if not item:
            continue
        name, _, val = (s.strip() for s in item.partition("="))
        nxt = int(val, 0) if val else nxt
        values[name] = nxt
        nxt += 1
    return {fmt: values[name] for fmt, name in REF_NAMES.items()}


def reference_unpack(formats):
    assert HARNESS.exists(), "oracle/_ref/libref_harness.so is missing: build it on the build machine (make -C oracle ref)"
    names = subprocess.run(["nm", "-DC", str(HARNESS)], check=True, stdout=subprocess.PIPE, text=True).stdout.splitlines()
    want = "basisu::unpack_block(basisu::texture_format, void const*, basisu::color_rgba*, bool)"
    at = [k for k, line in enumerate(names) if line.endswith(" T " + want)]
    assert len(at) == 1, f"the harness does not export {want}"
    mangled = subprocess.run(["nm", "-D", str(HARNESS)], check=True, stdout=subprocess.PIPE, text=True).stdout.splitlines()[at[0]].split()[-1]
    fn = getattr(C.CDLL(str(HARNESS)), mangled)
    fn.restype = C.c_bool
    fn.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_bool]

    def unpack(blocks, fmt):
        blocks = np.ascontiguousarray(blocks, np.uint8)
        n = blocks.shape[0]
        texels, ok = np.zeros((n, 16, 4), np.uint8), np.zeros(n, np.uint8)
        texels[..., 3] = 255
        for i in range(n):
            ok[i] = 1 if fn(formats[fmt], blocks[i].ctypes.data, texels[i].ctypes.data, False) else 0
        return texels, ok
    return unpack


class Draw:
    """small integers from the same raw stream as the blocks"""

    def __init__(self, bits):
        self.bits = bits

    def below(self, n, count=1):
        v = self.bits.g.random_raw(count) % np.uint64(n)
        return [int(x) for x in v]


# ---------------------------------------------------------------- ETC1 / ETC2 / EAC

def etc1_diff_channel(draw, way):
    """one colour byte base5 << 3 | delta3 of a differential block: way "in" (stays in 0..31), "low" (below 0), "high" (above 31), "ends" (delta -4 or +3, in range)"""
    if way == "low":
        base = draw.below(4)[0]
        d = -4 + draw.below(4 - base)[0]          # base + d < 0
    elif way == "high":
        base = 29 + draw.below(3)[0]
        d = 32 - base + draw.below(base - 28)[0]  # base + d > 31, d <= 3
    elif way == "ends":
        d = (-4, 3)[draw.below(2)[0]]
        base = 4 + draw.below(24)[0]
    else:
        base, d = 4 + draw.below(24)[0], -4 + draw.below(8)[0]
    return (base << 3) | (d & 7)


def etc1_forced(rng, draw, n, ways):
    """n random-bit differential blocks whose colour bytes go the given ways (r, g, b)"""
    blk = rng.blocks(n, 8)
    for b in blk:
        b[3] |= 2
        for c in range(3):
            b[c] = etc1_diff_channel(draw, ways[c])
    return blk


def etc1_valid_random(rng, n):
    out = []
    while len(out) < n:
        out += [b for b in rng.blocks(n, 8) if X.etc1_fields(b)["overflow"] is None]
    return np.array(out[:n])


def etc1_overflowing(rng, draw, per_way):
    high = []
    for k in range(per_way):
        ways = ["in", "in", "in"]
        ways[k % 3] = "high"
        high.append(etc1_forced(rng, draw, 1, ways))
    return np.concatenate([etc1_forced(rng, draw, per_way, ("low", "in", "in")), etc1_forced(rng, draw, per_way, ("in", "low", "in")),
                           etc1_forced(rng, draw, per_way, ("in", "in", "low"))] + high)


def eac_forced(blocks8):
    """in place, the first 24 blocks: base 0 and base 255 under multiplier 15 with every selector used, multiplier 0"""
    for k in range(8):
        blocks8[k, 0], blocks8[k, 1] = 0, 0xF0 | (blocks8[k, 1] & 15)
        blocks8[8 + k, 0], blocks8[8 + k, 1] = 255, 0xF0 | (blocks8[8 + k, 1] & 15)
        blocks8[16 + k, 1] &= 15


# ---------------------------------------------------------------- ASTC

def astc_candidate(rng, draw):
    """one random-bit block with a block mode of the 4x4 footprint's parameter space forced in"""
    b = rng.blocks(1, 16)
    w, h, r, high, dual, parts, cem, selector = (v + o for v, o in zip(draw.below(3) + draw.below(3) + draw.below(6) + draw.below(2) + draw.below(2) + draw.below(4) +
                                                                       draw.below(16) + draw.below(4), (2, 2, 2, 0, 0, 1, 0, 0)))
    if w == 4:
        put(b, 2, 2, 0); put(b, 7, 2, 0)
    else:
        put(b, 2, 2, 3); put(b, 8, 1, 1); put(b, 7, 1, w - 2)
    put(b, 5, 2, h - 2)
    put(b, 4, 1, r & 1); put(b, 0, 2, r >> 1)
    put(b, 9, 1, high); put(b, 10, 1, dual); put(b, 11, 2, parts - 1)
    if parts == 1:
        put(b, 13, 4, cem)
    else:
        put(b, 23, 2, selector)
        if selector == 0:
            put(b, 25, 4, cem)
    return b[0]


def astc_classes(f):
    """the classes of check_coverage a normal block counts for"""
    out = [("class", f"{f['parts']}_{'dual' if f['dual'] else 'single'}"), ("range", "%d_%d" % f["range"]), ("grid", "%dx%d" % f["grid"])]
    out += [("mode", str(m)) for m in f["used"]]
    if f["selector"] != 0 and len(set(f["cems"])) > 1:
        out.append(("multi_cem", ""))
    return out


def astc_accepted(rng, draw, unpack, tries=60000):
    need = {}
    for p in (1, 2, 3, 4):
        for d in ("single", "dual"):
            if (p, d) != (4, "dual"):
                need[("class", f"{p}_{d}")] = X.ASTC_MIN["class"]
    need.update({("mode", str(m)): X.ASTC_MIN["mode"] for m in X.ASTC_LDR_MODES})
    need.update({("range", "%d_%d" % k): X.ASTC_MIN["range"] for k in X.ASTC_WEIGHT_RANGES})
    need.update({("grid", f"{w}x{h}"): X.ASTC_MIN["grid"] for w in (2, 3, 4) for h in (2, 3, 4)})
    need[("multi_cem", "")] = X.ASTC_MIN["multi_cem"]
    kept, refused = [], {why: [] for why in X.ASTC_REFUSED_WELL_FORMED}
    for _ in range(tries):
        if not any(v > 0 for v in need.values()) and all(len(r) >= X.ASTC_MIN["refused_hdr_mode"] for r in refused.values()) and len(kept) >= ASTC_ACCEPTED:
            break
        b = astc_candidate(rng, draw)
        f = X.astc_fields(b)
        ok = unpack(b[None], X.ASTC)[1][0]
        assert bool(ok) == (f["kind"] == "normal"), (b.tolist(), f, ok)   # the header parser of the helpers and the reference agree on every candidate
        if f["why"] in refused and len(refused[f["why"]]) < X.ASTC_MIN["refused_hdr_mode"]:
            refused[f["why"]].append(b)
        if not ok:
            continue
        mine = astc_classes(f)
        if any(need[c] > 0 for c in mine) or len(kept) < ASTC_ACCEPTED:
            kept.append(b)
            for c in mine:
                need[c] -= 1
    assert not any(v > 0 for v in need.values()), {k: v for k, v in need.items() if v > 0}
    assert all(len(r) == X.ASTC_MIN["refused_hdr_mode"] for r in refused.values()), {k: len(r) for k, r in refused.items()}
    return np.array(kept), np.concatenate([np.array(refused[why]) for why in X.ASTC_REFUSED_WELL_FORMED])


def astc_void(rng, n, hdr):
    b = rng.blocks(n, 16)
    put(b, 0, 9, 0x1FC); put(b, 9, 1, 1 if hdr else 0); put(b, 10, 2, 3)
    for k, x in enumerate(b):
        if k < n // 2:
            put(x[None], 12, 52, (1 << 52) - 1)
        else:
            for at in (12, 38):
                lo, hi = sorted((X.field(x, at, 13), X.field(x, at + 13, 13)))
                hi += 1 if lo == hi else 0
                lo -= 1 if hi > 0x1FFF else 0
                put(x[None], at, 13, lo); put(x[None], at + 13, 13, min(hi, 0x1FFF))
    return b


def astc_raw_refused(rng, unpack, n):
    out = []
    while len(out) < n:
        b = rng.blocks(n, 16)
        ok = unpack(b, X.ASTC)[1]
        for x, o in zip(b, ok):
            f = X.astc_fields(x)
            assert bool(o) == (f["kind"] != "refused"), (x.tolist(), f, o)
            if not o:
                out.append(x)
    return np.array(out[:n])


# ---------------------------------------------------------------- PVRTC1

def pvrtc1_rasters(arrays, meta):
    """every image of the chosen files through `basisu -unpack`; the restatement has to reproduce each raster before it is stored"""
    pv, pv_meta = X.golden_pvrtc1()
    files = {f["name"]: f for f in pv_meta["files"]}
    for name in X.PVRTC1_FILES:
        f, ext = files[name], files[name]["container"]
        with tempfile.TemporaryDirectory() as d:
            (pathlib.Path(d) / f"x.{ext}").write_bytes(pv["file_" + name].tobytes())
            GG.tool(["-unpack", f"x.{ext}"], d)
            mips = len(f["images"]) > 1
            for level, layer, face, w, h in f["images"]:
                key = f"{name}_L{level}_A{layer}_F{face}"
                if ext == "ktx2":   # the tool's names: a level is named only where the file has more than one
                    where = f"level_{level}_face_{face}_layer_{layer:04d}" if mips else f"face_{face}_layer_{layer:04d}"
                else:
                    where = f"{level}_{layer:04d}" if mips else f"{layer:04d}"
                for short, tag in (("rgb", "PVRTC1_4_RGB"), ("rgba", "PVRTC1_4_RGBA")):
                    png = pathlib.Path(d) / f"x_unpacked_rgba_{tag}_{where}.png"
                    if not png.exists():
                        png = pathlib.Path(d) / f"x_unpacked_rgb_{tag}_{where}.png"
                    want = GG.read_png(png)
                    assert want.shape[:2] == (h, w), (key, want.shape)
                    nbx, nby = (w + 3) // 4, (h + 3) // 4
                    got = X.pvrtc1_restate(pv[f"{key}_{short}"], nbx, nby, w, h)
                    assert (got[..., :want.shape[2]] == want).all(), (key, short)
                    if want.shape[2] == 3:
                        assert (got[..., 3] == 255).all(), (key, short)
                    arrays[f"pvrtc1_{key}_{short}_texels"] = want
                    meta["pvrtc1_images"].append([key, short, w, h, int(want.shape[2])])
        print("pvrtc1", name, len(f["images"]), "images", flush=True)


if __name__ == "__main__":
    formats = reference_formats()
    unpack = reference_unpack(formats)
    rng = GB.Bits(SEED)
    draw = Draw(rng)
    sets = {}
    sets["etc1"] = np.concatenate([etc1_valid_random(rng, 256), etc1_forced(rng, draw, 64, ("ends", "ends", "ends"))])
    sets["etc1_overflow"] = etc1_overflowing(rng, draw, 16)
    etc2 = np.concatenate([rng.blocks(256, 8), etc1_valid_random(rng, 256)], 1)
    for k in range(4):
        etc2[k, 1] &= 15; etc2[4 + k, 1] |= 0xF0; etc2[8 + k, 0] = 0; etc2[12 + k, 0] = 255
    sets["etc2"] = np.concatenate([etc2, np.concatenate([rng.blocks(32, 8), etc1_overflowing(rng, draw, 8)], 1)])
    r11 = rng.blocks(256, 8)
    eac_forced(r11)
    rg11 = rng.blocks(256, 16)
    eac_forced(rg11[:, :8]); eac_forced(rg11[:, 8:])
    sets["r11"], sets["rg11"] = r11, rg11
    accepted, hdr_mode = astc_accepted(rng, draw, unpack)
    sets["astc"] = np.concatenate([accepted, astc_void(rng, X.ASTC_MIN["void"], False)])
    sets["astc_refused"] = np.concatenate([astc_raw_refused(rng, unpack, X.ASTC_MIN["refused"] - 8 - hdr_mode.shape[0]), hdr_mode, astc_void(rng, 8, True)])
    for name, (file, array, _) in X.ENCODER_MADE.items():
        sets[name] = np.array(np.load(ROOT / "tests" / "golden" / file)[array][:X.ENCODER_MADE_BLOCKS])
    arrays = {}
    meta = {"seed": SEED, "reference_texture_formats": {str(k): v for k, v in formats.items()}, "members": {}, "pvrtc1_images": [],
            "pvrtc1_random": [list(s) for s in X.PVRTC1_RANDOM],
            "pvrtc1_modulation_mode_1": "the texels of the pvrtc1_random_* members come from the Python restatement of pvrtc4_image::get_pixel in "
                                        "tests/texture_unpack_helpers.py, not from a run of the reference; the restatement reproduced every tool-made raster listed in "
                                        "pvrtc1_images (all of modulation mode 0) before they were written"}
    for name, blocks in sets.items():
        fmt = X.BLOCK_MEMBERS[name]
        texels, ok = unpack(blocks, fmt)
        arrays[name + "_blocks"], arrays[name + "_texels"], arrays[name + "_ok"] = blocks, texels, ok
        meta["members"][name] = {"format": fmt, "blocks": int(blocks.shape[0]), "refused": int((ok == 0).sum())}
        print(name, blocks.shape, "refused", int((ok == 0).sum()), flush=True)
    rgba32 = np.load(ROOT / "tests" / "golden" / "uastc_transcode_vectors.npz")["level2_rgba32"][:X.ENCODER_MADE_BLOCKS].reshape(-1, 16, 4)
    meta["uastc_astc_unpack_equals_rgba32"] = bool((arrays["uastc_astc_texels"] == rgba32).all())
    pvrtc1_rasters(arrays, meta)
    for nbx, nby in X.PVRTC1_RANDOM:
        blocks = rng.blocks(nbx * nby, 8)
        arrays[f"pvrtc1_random_{nbx}x{nby}_blocks"] = blocks
        arrays[f"pvrtc1_random_{nbx}x{nby}_texels"] = X.pvrtc1_restate(blocks, nbx, nby)
    meta["counts"] = X.check_coverage(arrays, None)
    arrays["meta"] = np.frombuffer(json.dumps(meta, sort_keys=True).encode(), np.uint8)
    S.save(X.GOLDEN, arrays)
    size = X.GOLDEN.stat().st_size
    assert size <= MAX_BYTES, size
    print("wrote", X.GOLDEN, size, "bytes,", len(arrays), "members; uastc astc == rgba32:", meta["uastc_astc_unpack_equals_rgba32"])
