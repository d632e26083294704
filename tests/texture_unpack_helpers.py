"""Test-only helpers of the texture unpacker's tests: the g++ build of basis_universal_amd/csrc/texture_unpack.h (tests/native/texture_unpack_host.cpp), the golden
file (tests/golden/texture_unpack_vectors.npz), what the generator and the tests both need to know about the leading fields of an ETC1, EAC and ASTC block, and a
Python restatement of PVRTC1's texel (pvrtc4_image::get_pixel, encoder/basisu_pvrtc1_4.cpp:338-379, with get_endpoint_5554 :238 and interpolate, basisu_pvrtc1_4.h:341).

The restatement is there for ONE reason: modulation mode M = 1 is the one thing the reference cannot be run on from here (every transcoder writes M = 0, unpack_block
has no PVRTC1 case). It first has to reproduce every raster the reference tool wrote (M = 0); the M = 1 texels of the fixture's random-bit images are its word alone."""
import ctypes as C
import functools
import pathlib

import numpy as np

import native_libs

ROOT = pathlib.Path(__file__).resolve().parent.parent
NATIVE = native_libs.NATIVE
native_libs.CHECKERS.setdefault("texture_unpack_host", (NATIVE / "libtexture_unpack_host.so", NATIVE / "texture_unpack_host.cpp", "HOST_API", "g++"))

GOLDEN = ROOT / "tests" / "golden" / "texture_unpack_vectors.npz"
GOLDEN_PVRTC1 = ROOT / "tests" / "golden" / "pvrtc1_vectors.npz"
u8p = C.POINTER(C.c_uint8)

# transcoder_texture_format values (basis_universal_amd.transcode has the same constants; kept here so the host tests do not need the package's library)
ETC1, ETC2, BC1, BC3, BC4, BC5, BC7, PVRTC1_RGB, PVRTC1_RGBA, ASTC, R11, RG11 = 0, 1, 2, 3, 4, 5, 6, 8, 9, 10, 20, 21
BYTES = {ETC1: 8, ETC2: 16, BC1: 8, BC3: 16, BC4: 8, BC5: 16, BC7: 16, PVRTC1_RGB: 8, PVRTC1_RGBA: 8, ASTC: 16, R11: 8, RG11: 16}
NEW_FORMATS = (ETC1, ETC2, PVRTC1_RGB, PVRTC1_RGBA, ASTC, R11, RG11)
BC_FORMATS = (BC1, BC3, BC4, BC5, BC7)
REFUSED_FORMATS = {13: "RGBA32", 11: "ATC_RGB", 12: "ATC_RGBA", 99: "unknown"}

# the block-wise members of the fixture: name -> format. `<name>_blocks`, `<name>_texels`, `<name>_ok`
CONSTRUCTED = {"etc1": ETC1, "etc1_overflow": ETC1, "etc2": ETC2, "r11": R11, "rg11": RG11, "astc": ASTC, "astc_refused": ASTC}
# what this package's transcoders write: member -> (golden file, array, format); the first ENCODER_MADE_BLOCKS blocks of each
ENCODER_MADE_BLOCKS = 512
ENCODER_MADE = {"uastc_etc1": ("uastc_texture_vectors.npz", "level2_etc1", ETC1), "uastc_etc2": ("uastc_texture_vectors.npz", "level2_etc2", ETC2),
                "uastc_r11": ("uastc_texture_vectors.npz", "level2_r11", R11), "uastc_rg11": ("uastc_texture_vectors.npz", "level2_rg11", RG11),
                "uastc_astc": ("uastc_transcode_vectors.npz", "level2_astc", ASTC),
                "etc1s_astc": ("etc1s_block_format_vectors.npz", "coverage_basis_L0_A0_F0_astc", ASTC),
                "etc1s_r11": ("etc1s_block_format_vectors.npz", "coverage_basis_L0_A0_F0_r11", R11),
                "etc1s_rg11": ("etc1s_block_format_vectors.npz", "coverage_basis_L0_A0_F0_rg11", RG11)}
BLOCK_MEMBERS = {**CONSTRUCTED, **{k: v[2] for k, v in ENCODER_MADE.items()}}
# the PVRTC1 images whose rasters the reference tool wrote: files of pvrtc1_vectors.npz (its blocks are the inputs) -> `pvrtc1_<image key>_<rgb|rgba>_texels`
PVRTC1_FILES = ("etc1s_alpha_basis", "etc1s_opaque_basis", "etc1s_wide_basis", "etc1s_tall_basis", "etc1s_coverage_basis",
                "uastc_alpha_ktx2", "uastc_opaque_ktx2", "uastc_wide_ktx2", "uastc_tall_ktx2", "uastc_coverage_ktx2")
PVRTC1_TARGETS = {"rgb": PVRTC1_RGB, "rgba": PVRTC1_RGBA}
# the random-bit PVRTC1 images (both modulation modes): (nbx, nby) -> `pvrtc1_random_<nbx>x<nby>_blocks` (Morton order), `_texels` (the restatement's raster)
PVRTC1_RANDOM = ((1, 1), (2, 1), (1, 2), (2, 2), (8, 2))


def host():
    return native_libs.load("texture_unpack_host")


def _p(a):
    return a.ctypes.data_as(u8p)


def host_unpack(blocks, fmt):
    """-> (texels (n, 16, 4) uint8 in raster order, ok flags (n,) uint8). An invalid block is zero-filled. Every format but PVRTC1."""
    blocks = np.ascontiguousarray(blocks, np.uint8).reshape(-1, BYTES[fmt])
    n = blocks.shape[0]
    out, ok = np.zeros((n, 16, 4), np.uint8), np.zeros(n, np.uint8)
    assert host().th_unpack(_p(blocks), n, fmt, _p(out), _p(ok))
    return out, ok


def to_raster(texels, nbx, nby, width, height):
    """(nby * nbx, 16, 4) texels -> the (height, width, 4) image they cover, cropped"""
    return np.ascontiguousarray(texels.reshape(nby, nbx, 4, 4, 4).transpose(0, 2, 1, 3, 4).reshape(nby * 4, nbx * 4, 4)[:height, :width])


def host_unpack_pvrtc1(blocks, nbx, nby, width=None, height=None):
    """blocks (nbx * nby, 8) in Morton order -> the (height, width, 4) raster"""
    blocks = np.ascontiguousarray(blocks, np.uint8).reshape(nbx * nby, 8)
    out = np.zeros((nbx * nby, 16, 4), np.uint8)
    assert host().th_unpack_pvrtc1(_p(blocks), nbx, nby, _p(out))
    return to_raster(out, nbx, nby, width or nbx * 4, height or nby * 4)


def ise_value(bits16, kind, n, values, k):
    """value k of a BISE sequence (kind 0 bits, 1 trits, 2 quints; n plain bits) packed from bit 0 of 16 bytes -> (plain bits, trit or quint)"""
    v = host().th_ise_value(_p(np.ascontiguousarray(bits16, np.uint8)), kind, n, values, k)
    return v & 255, v >> 8


@functools.lru_cache(maxsize=None)
def golden():
    """-> (arrays, meta) of texture_unpack_vectors.npz: loaded once and shared; nobody writes into the arrays"""
    return native_libs.load_npz_golden(GOLDEN)


@functools.lru_cache(maxsize=None)
def golden_pvrtc1():
    return native_libs.load_npz_golden(GOLDEN_PVRTC1)


def field(block, ofs, width):
    """bits ofs .. ofs + width of a block, little-endian bit order"""
    return (int.from_bytes(np.asarray(block, np.uint8).tobytes(), "little") >> ofs) & ((1 << width) - 1)


# ---------------------------------------------------------------- PVRTC1

def morton_address(x, y, nbx, nby):
    """where block (x, y) lies: y in the even bits, x in the odd ones over the shorter axis' bits, the longer axis' other bits above"""
    low = min(nbx.bit_length(), nby.bit_length()) - 1
    at = 0
    for k in range(low):
        at |= ((y >> k) & 1) << (2 * k) | ((x >> k) & 1) << (2 * k + 1)
    return at | ((x if nbx > nby else y) >> low) << (2 * low)


def pvrtc1_images(files=PVRTC1_FILES):
    """the tool-made PVRTC1 images the fixture holds rasters of -> [(key in pvrtc1_vectors.npz without the target suffix, width, height)]"""
    _, meta = golden_pvrtc1()
    out = []
    for f in meta["files"]:
        if f["name"] in files:
            out += [(f"{f['name']}_L{level}_A{layer}_F{face}", w, h) for level, layer, face, w, h in f["images"]]
    return out


def _endpoint_5554(word, high):
    """(n,) endpoint words -> (n, 4) int: r5 g5 b5 a4"""
    p = (word >> 16) if high else (word & 0xFFFF)
    opaque = (p & 0x8000) != 0
    rep = lambda v, bits: (v << (5 - bits)) | (v >> (2 * bits - 5))
    if high:
        ob, tb = p & 31, rep(p & 15, 4)
    else:
        ob, tb = rep((p >> 1) & 15, 4), rep((p >> 1) & 7, 3)
    o = np.stack([(p >> 10) & 31, (p >> 5) & 31, ob, np.full_like(p, 15)], -1)
    t = np.stack([rep((p >> 8) & 15, 4), rep((p >> 4) & 15, 4), tb, ((p >> 12) & 7) << 1], -1)
    return np.where(opaque[..., None], o, t).astype(np.int64)


def pvrtc1_restate(blocks, nbx, nby, width=None, height=None):
    """get_pixel over a whole image: blocks (nbx * nby, 8) in Morton order -> (height, width, 4) uint8. Both modulation modes."""
    blocks = np.ascontiguousarray(blocks, np.uint8).reshape(nbx * nby, 8)
    words = blocks.view("<u4").astype(np.int64)   # [:, 0] modulation, [:, 1] endpoints
    order = np.array([[morton_address(x, y, nbx, nby) for x in range(nbx)] for y in range(nby)])
    mod, ends = words[order, 0], words[order, 1]   # (nby, nbx), raster order
    ys, xs = np.mgrid[0:nby * 4, 0:nbx * 4]
    bx0, by0 = ((xs - 2) >> 2) % nbx, ((ys - 2) >> 2) % nby
    bx1, by1 = (bx0 + 1) % nbx, (by0 + 1) % nby
    u, v = ((xs + 2) & 3)[..., None], ((ys + 2) & 3)[..., None]
    both = []
    for high in (0, 1):
        p, q, r, s = (_endpoint_5554(ends[yy, xx], high) for yy, xx in ((by0, bx0), (by0, bx1), (by1, bx0), (by1, bx1)))
        t, b = p * 4 + u * (q - p), r * 4 + u * (s - r)
        val = t * 4 + v * (b - t)
        rgb = val[..., :3] >> 1
        rgb = rgb + (rgb >> 5)
        a = val[..., 3:] + (val[..., 3:] >> 4)
        both.append(np.concatenate([rgb, a], -1))
    l, h = both
    m = ((mod[ys >> 2, xs >> 2] >> (2 * ((ys & 3) * 4 + (xs & 3)))) & 3)[..., None]
    punch = ((ends[ys >> 2, xs >> 2] & 1) != 0)[..., None]
    mean = (l + h) // 2
    mean_punch = mean.copy()
    mean_punch[..., 3:] = np.where(m == 2, 0, mean[..., 3:])
    mid = np.where(punch, mean_punch, np.where(m == 1, (l * 5 + h * 3) // 8, (l * 3 + h * 5) // 8))
    out = np.where(m == 0, l, np.where(m == 3, h, mid))
    assert out.min() >= 0 and out.max() <= 255
    return np.ascontiguousarray(out.astype(np.uint8)[:height or nby * 4, :width or nbx * 4])


# ---------------------------------------------------------------- ETC1 / EAC fields, from the formats

def etc1_fields(block):
    """-> {"diff", "flip", "tables": (t0, t1), "deltas": (dr, dg, db) or None, "overflow": None | "r_low" | "g_low" | "b_low" | "high"}"""
    b = np.asarray(block, np.uint8)
    diff, flip = bool(b[3] & 2), bool(b[3] & 1)
    out = {"diff": diff, "flip": flip, "tables": (int(b[3] >> 5), int((b[3] >> 2) & 7)), "deltas": None, "overflow": None}
    if diff:
        deltas, sums = [], []
        for c in range(3):
            d = int(b[c] & 7)
            d -= 8 if d >= 4 else 0
            deltas.append(d)
            sums.append(int(b[c] >> 3) + d)
        out["deltas"] = tuple(deltas)
        if any(s > 31 for s in sums):
            out["overflow"] = "high"
        else:
            low = [n for n, s in zip("rgb", sums) if s < 0]
            out["overflow"] = low[0] + "_low" if low else None
    return out


def eac_values(block8):
    """the 16 unclamped 11-bit values of an EAC R11 block, for the clamp counts"""
    b = np.asarray(block8, np.uint8)
    base, mul, table = int(b[0]) * 8 + 4, int(b[1] >> 4), int(b[1] & 15)
    sels = int.from_bytes(b[2:8].tobytes(), "big")
    return [base + EAC_TABLES[table][(sels >> (45 - 3 * k)) & 7] * (mul * 8 if mul else 1) for k in range(16)]


EAC_TABLES = [[-3, -6, -9, -15, 2, 5, 8, 14], [-3, -7, -10, -13, 2, 6, 9, 12], [-2, -5, -8, -13, 1, 4, 7, 12], [-2, -4, -6, -13, 1, 3, 5, 12],
              [-3, -6, -8, -12, 2, 5, 7, 11], [-3, -7, -9, -11, 2, 6, 8, 10], [-4, -7, -8, -11, 3, 6, 7, 10], [-3, -5, -8, -11, 2, 4, 7, 10],
              [-2, -6, -8, -10, 1, 5, 7, 9], [-2, -5, -8, -10, 1, 4, 7, 9], [-2, -4, -8, -10, 1, 3, 7, 9], [-2, -5, -7, -10, 1, 4, 6, 9],
              [-3, -4, -7, -10, 2, 3, 6, 9], [-1, -2, -3, -10, 0, 1, 2, 9], [-4, -6, -8, -9, 3, 5, 7, 8], [-3, -5, -7, -9, 2, 4, 6, 8]]


# ---------------------------------------------------------------- ASTC 4x4 header fields, from the format (Khronos data format specification, ASTC chapter)

ASTC_HDR_MODES = (2, 3, 7, 11, 14, 15)
ASTC_LDR_MODES = (0, 1, 4, 5, 6, 8, 9, 10, 12, 13)
# weight range by (r, high-precision bit): (kind 0 bits / 1 trits / 2 quints, plain bits)
ASTC_WEIGHT_RANGES = {(2, 0): (0, 1), (3, 0): (1, 0), (4, 0): (0, 2), (5, 0): (2, 0), (6, 0): (1, 1), (7, 0): (0, 3),
                      (2, 1): (2, 1), (3, 1): (1, 2), (4, 1): (0, 4), (5, 1): (2, 2), (6, 1): (1, 3), (7, 1): (0, 5)}


def ise_bits(kind, n, values):
    return values * n + ((values * 8 + 4) // 5 if kind == 1 else ((values * 7 + 2) // 3 if kind == 2 else 0))


def astc_partition(seed10, parts, x, y):
    """the partition of texel (x, y) of a 4x4 block (a "small block": coordinates doubled)"""
    M = 0xFFFFFFFF
    seed = seed10 + 1024 * (parts - 1)
    p = seed
    p ^= p >> 15; p = (p - (p << 17)) & M; p = (p + (p << 7)) & M; p = (p + (p << 4)) & M
    p ^= p >> 5; p = (p + (p << 16)) & M; p ^= p >> 7; p ^= p >> 3
    p = (p ^ (p << 6)) & M; p ^= p >> 17
    s = [(p >> (4 * k)) & 15 for k in range(8)]
    s = [(v * v) & 255 for v in s]
    sha, shb = (4 if seed & 2 else 5), (6 if parts == 3 else 5)
    sh1, sh2 = (sha, shb) if seed & 1 else (shb, sha)
    s = [v >> (sh1 if k % 2 == 0 else sh2) for k, v in enumerate(s)]
    x, y = x * 2, y * 2
    a = 63 & (s[0] * x + s[1] * y + (p >> 14))
    b = 63 & (s[2] * x + s[3] * y + (p >> 10))
    c = 63 & (s[4] * x + s[5] * y + (p >> 6)) if parts >= 3 else 0
    d = 63 & (s[6] * x + s[7] * y + (p >> 2)) if parts >= 4 else 0
    return 0 if (a >= b and a >= c and a >= d) else (1 if (b >= c and b >= d) else (2 if c >= d else 3))


def astc_fields(block):
    """The leading fields of an ASTC 4x4 block. -> {"kind": "void" | "normal" | "refused", "why": the first rule an LDR 4x4 decoder refuses it by (or None), and
    for a normal or an HDR-refused block: "grid" (w, h), "range" (r, high), "dual", "parts", "selector" (the CEM selector bits; 0 for one partition), "cems"
    (per partition), "used" (the modes of the partitions that hold a texel)}"""
    v = int.from_bytes(np.asarray(block, np.uint8).tobytes(), "little")
    bits = lambda ofs, n: (v >> ofs) & ((1 << n) - 1)
    bm = bits(0, 11)
    if (bm & 0x1FF) == 0x1FC:
        ext = [bits(12 + 13 * k, 13) for k in range(4)]
        if bits(10, 2) != 3:
            return {"kind": "refused", "why": "void extent reserved bits"}
        if bits(9, 1):
            return {"kind": "refused", "why": "hdr void extent"}
        if not all(e == 0x1FFF for e in ext) and (ext[0] >= ext[1] or ext[2] >= ext[3]):
            return {"kind": "refused", "why": "void extent coordinates"}
        return {"kind": "void", "why": None}
    if (bm & 3) == 0:
        return {"kind": "refused", "why": "reserved block mode or grid past 4x4"}
    layout, a, b = (bm >> 2) & 3, (bm >> 5) & 3, (bm >> 7) & 3
    if layout == 0:
        w, h = b + 4, a + 2
    elif layout == 3 and b & 2:
        w, h = (b & 1) + 2, a + 2
    else:
        return {"kind": "refused", "why": "grid past 4x4"}
    if w > 4 or h > 4:
        return {"kind": "refused", "why": "grid past 4x4"}
    r, high, dual, parts = ((bm >> 4) & 1) | ((bm & 3) << 1), (bm >> 9) & 1, (bm >> 10) & 1, bits(11, 2) + 1
    kind, n = ASTC_WEIGHT_RANGES[(r, high)]
    wbits = ise_bits(kind, n, w * h * (dual + 1))
    if wbits > 96 or wbits < 24:
        return {"kind": "refused", "why": "weight bits"}
    if parts == 4 and dual:
        return {"kind": "refused", "why": "four partitions and two planes"}
    selector = bits(23, 2) if parts > 1 else 0
    under = 128 - wbits - (0 if selector == 0 else 3 * parts - 4)
    if parts == 1:
        cems = [bits(13, 4)]
    elif selector == 0:
        cems = [bits(25, 4)] * parts
    else:
        cems = []
        for p in range(parts):
            cls = selector - (0 if bits(25 + p, 1) else 1)
            low = [bits(25 + q, 1) if q < 4 else bits(under + q - 4, 1) for q in (parts + 2 * p, parts + 2 * p + 1)]
            cems.append(cls << 2 | low[1] << 1 | low[0])
    values = sum((m // 4 + 1) * 2 for m in cems)
    config = (17 if parts == 1 else (29 if selector == 0 else 25 + 3 * parts)) + 2 * dual
    if values > 18 or 128 - wbits - config < (13 * values + 4) // 5:
        return {"kind": "refused", "why": "endpoint bits"}
    used = sorted({cems[astc_partition(bits(13, 10), parts, t & 3, t >> 2) if parts > 1 else 0] for t in range(16)})
    out = {"kind": "normal", "why": None, "grid": (w, h), "range": (r, high), "dual": dual, "parts": parts, "selector": selector, "cems": cems, "used": used}
    if any(m in ASTC_HDR_MODES for m in used):
        out.update(kind="refused", why="hdr endpoint mode")
    return out


# ---------------------------------------------------------------- the conditions the fixture is written under

ASTC_REFUSED_WELL_FORMED = ("hdr endpoint mode", "endpoint bits", "weight bits", "four partitions and two planes")   # refusals past the block mode's layout bits
ASTC_MIN = {"class": 16, "mode": 16, "range": 8, "grid": 8, "multi_cem": 16, "void": 32, "refused": 256, "refused_hdr_mode": 8, "refused_hdr_void": 8}


def check_coverage(arrays, meta):
    """Counted from the blocks themselves; asserted by tools/gen_golden_texture_unpack.py before it writes and by tests/test_texture_unpack_host.py on the
    committed file. -> the counts, which are the fixture's meta["counts"]."""
    counts = {}
    # ETC1: every block of `etc1` valid; mode x flip, every table in both sub-blocks, deltas at both ends; 16 blocks per way of overflowing
    f = [etc1_fields(b) for b in arrays["etc1_blocks"]]
    assert arrays["etc1_ok"].all() and all(x["overflow"] is None for x in f) and len(f) >= 256
    counts["etc1_mode_flip"] = [sum(1 for x in f if x["diff"] == d and x["flip"] == fl) for d in (False, True) for fl in (False, True)]
    assert min(counts["etc1_mode_flip"]) >= 32, counts["etc1_mode_flip"]
    counts["etc1_tables"] = [[sum(1 for x in f if x["tables"][s] == t) for t in range(8)] for s in (0, 1)]
    assert min(min(row) for row in counts["etc1_tables"]) >= 1
    counts["etc1_delta_ends"] = [sum(1 for x in f if x["deltas"] and e in x["deltas"]) for e in (-4, 3)]
    assert min(counts["etc1_delta_ends"]) >= 8, counts["etc1_delta_ends"]
    f = [etc1_fields(b) for b in arrays["etc1_overflow_blocks"]]
    counts["etc1_overflow"] = {w: sum(1 for x in f if x["overflow"] == w) for w in ("r_low", "g_low", "b_low", "high")}
    assert not arrays["etc1_overflow_ok"].any() and all(c == 16 for c in counts["etc1_overflow"].values()), counts["etc1_overflow"]
    # ETC2 RGBA: the alpha half's tables, multipliers 0 and 15, bases 0 and 255; 32 blocks whose colour half overflows, refused
    b = arrays["etc2_blocks"]
    over = np.array([etc1_fields(x[8:])["overflow"] is not None for x in b])
    assert (over == (arrays["etc2_ok"] == 0)).all() and int(over.sum()) == 32 and int((~over).sum()) >= 256
    counts["etc2_tables"] = np.bincount(b[:, 1] & 15, minlength=16).tolist()
    counts["etc2_multiplier_0_15"] = [int(((b[:, 1] >> 4) == m).sum()) for m in (0, 15)]
    counts["etc2_base_0_255"] = [int((b[:, 0] == v).sum()) for v in (0, 255)]
    assert min(counts["etc2_tables"]) >= 1 and min(counts["etc2_multiplier_0_15"]) >= 1 and min(counts["etc2_base_0_255"]) >= 1
    # R11 / RG11: every table, multiplier 0, both clamps reached
    for name, halves in (("r11", 1), ("rg11", 2)):
        b = arrays[name + "_blocks"].reshape(-1, 8)
        assert arrays[name + "_ok"].all() and b.shape[0] >= 256 * halves
        vals = np.array([eac_values(x) for x in b])
        counts[name] = {"tables": np.bincount(b[:, 1] & 15, minlength=16).tolist(), "multiplier_0": int(((b[:, 1] >> 4) == 0).sum()),
                        "clamped_low": int((vals < 0).sum()), "clamped_high": int((vals > 2047).sum())}
        assert min(counts[name]["tables"]) >= 1 and counts[name]["multiplier_0"] >= 1 and counts[name]["clamped_low"] >= 1 and counts[name]["clamped_high"] >= 1
    # ASTC, accepted
    f = [astc_fields(x) for x in arrays["astc_blocks"]]
    assert arrays["astc_ok"].all() and all(x["kind"] in ("void", "normal") for x in f)
    normal = [x for x in f if x["kind"] == "normal"]
    counts["astc_void"] = sum(1 for x in f if x["kind"] == "void")
    counts["astc_class"] = {f"{p}_{'dual' if d else 'single'}": sum(1 for x in normal if x["parts"] == p and x["dual"] == d) for p in (1, 2, 3, 4) for d in (0, 1) if (p, d) != (4, 1)}
    counts["astc_mode"] = {str(m): sum(1 for x in normal if m in x["used"]) for m in ASTC_LDR_MODES}
    counts["astc_range"] = {f"{r}_{h}": sum(1 for x in normal if x["range"] == (r, h)) for (r, h) in ASTC_WEIGHT_RANGES}
    counts["astc_grid"] = {f"{w}x{h}": sum(1 for x in normal if x["grid"] == (w, h)) for w in (2, 3, 4) for h in (2, 3, 4)}
    counts["astc_multi_cem"] = sum(1 for x in normal if x["selector"] != 0 and len(set(x["cems"])) > 1)
    assert counts["astc_void"] >= ASTC_MIN["void"] and counts["astc_multi_cem"] >= ASTC_MIN["multi_cem"], counts
    for key, least in (("astc_class", "class"), ("astc_mode", "mode"), ("astc_range", "range"), ("astc_grid", "grid")):
        assert min(counts[key].values()) >= ASTC_MIN[least], (key, counts[key])
    # ASTC, refused
    f = [astc_fields(x) for x in arrays["astc_refused_blocks"]]
    assert not arrays["astc_refused_ok"].any() and all(x["kind"] == "refused" for x in f) and len(f) == ASTC_MIN["refused"]
    why = sorted({x["why"] for x in f})
    counts["astc_refused"] = {w: sum(1 for x in f if x["why"] == w) for w in why}
    assert all(counts["astc_refused"].get(w, 0) >= ASTC_MIN["refused_hdr_mode"] for w in ASTC_REFUSED_WELL_FORMED), counts["astc_refused"]
    assert counts["astc_refused"].get("hdr void extent", 0) >= ASTC_MIN["refused_hdr_void"]
    # what the transcoders write: all accepted
    for name, (_, _, fmt) in ENCODER_MADE.items():
        assert arrays[name + "_blocks"].shape == (ENCODER_MADE_BLOCKS, BYTES[fmt]) and arrays[name + "_ok"].all(), name
    # PVRTC1: both modulation modes and every modulation value among the random-bit images
    mode = np.concatenate([arrays[f"pvrtc1_random_{x}x{y}_blocks"][:, 4] & 1 for x, y in PVRTC1_RANDOM])
    counts["pvrtc1_random_mode"] = np.bincount(mode, minlength=2).tolist()
    assert min(counts["pvrtc1_random_mode"]) >= 4
    if meta is not None:
        assert meta["counts"] == counts, "meta's counts are not what the blocks give"
    return counts
