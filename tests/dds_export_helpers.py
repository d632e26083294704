"""The cases of tests/golden/dds_export_vectors.npz: source images turned into DX10 .dds files by the reference tool's `-dds` mode (tools/gen_golden_dds_export.py)
and by dds.export_dds. One table for the generator and the tests: per case the images, the tool's arguments and the keyword arguments of export_dds() that say the
same. Also the host build of the packers (tests/native/dds_pack_host.cpp) and the tile helpers the tests share."""
import functools
import pathlib

import numpy as np

import helpers
import native_libs

ROOT = pathlib.Path(__file__).resolve().parent.parent
NATIVE = native_libs.NATIVE
native_libs.CHECKERS.setdefault("dds_pack_host", (NATIVE / "libdds_pack_host.so", NATIVE / "dds_pack_host.cpp", "HOST_API", "g++"))

GOLDEN = ROOT / "tests" / "golden" / "dds_export_vectors.npz"
BLOCK_FORMATS = ("bc1", "bc2", "bc3", "bc4", "bc5")
RAW_FORMATS = ("a8r8g8b8", "a8b8g8r8", "r8", "r8g8", "r5g6b5", "a1r5g5b5", "a4r4g4b4")
UNPACK_TARGET = {"bc1": 2, "bc3": 3, "bc4": 4, "bc5": 5}   # transcode.unpack_blocks' format values


def alpha_image():
    """32x24 with the alpha ramp of tools/gen_golden_etc1s_transcode.py"""
    img = helpers.synth(32, 24, 13)
    yy, xx = np.mgrid[0:24, 0:32]
    img[..., 3] = np.clip(xx * 8 + yy * 3, 0, 255).astype(np.uint8)
    return img


def photo_image():
    """a 64x64 crop of kodim03 (tests/golden/kodim03.npz): real content for the least-squares passes of the BC1 encoder"""
    rgba = np.load(ROOT / "tests" / "golden" / "kodim03.npz")["rgba"]
    return np.ascontiguousarray(rgba[200:264, 330:394])


COVER_SOLID = 40   # the first COVER_SOLID tiles of cover_tiles() are solid


def cover_tiles():
    """256 crafted tiles, (256, 4, 4, 4) u8: solid colours (0 and 255 among them), two-colour tiles, tiles whose R or G or A is constant (bc4's mx == mn), a full
    0..255 ramp in one channel, tiles where min and max differ by 1, random tiles."""
    rng = np.random.default_rng(2024)
    tiles = []
    solid = [(0, 0, 0, 0), (255, 255, 255, 255), (0, 0, 0, 255), (255, 255, 255, 0), (255, 0, 0, 255), (0, 255, 0, 128), (0, 0, 255, 1), (1, 1, 1, 254), (128, 128, 128, 127)]
    solid += [tuple(int(v) for v in rng.integers(0, 256, 4)) for _ in range(COVER_SOLID - len(solid))]
    for c in solid:
        tiles.append(np.broadcast_to(np.array(c, np.uint8), (4, 4, 4)).copy())
    for _ in range(40):   # two colours, in a random pattern
        a, b = rng.integers(0, 256, 4), rng.integers(0, 256, 4)
        pick = rng.integers(0, 2, (4, 4, 1))
        tiles.append(np.where(pick, a, b).astype(np.uint8))
    for ch in (0, 1, 3, 0, 1, 3, 0, 1, 3, 2, 2, 2):   # one channel constant, the others random
        t = rng.integers(0, 256, (4, 4, 4)).astype(np.uint8)
        t[..., ch] = rng.integers(0, 256)
        tiles.append(t)
    for ch in range(4):   # 0, 17, ..., 255 in one channel, forwards and shuffled; the others random / constant
        ramp = (np.arange(16) * 17).astype(np.uint8)
        for order in (np.arange(16), rng.permutation(16)):
            t = rng.integers(0, 256, (4, 4, 4)).astype(np.uint8)
            t[..., ch] = ramp[order].reshape(4, 4)
            tiles.append(t)
            t = np.full((4, 4, 4), 77, np.uint8)
            t[..., ch] = ramp[order].reshape(4, 4)
            tiles.append(t)
    for _ in range(40):   # min and max differ by 1, in every channel
        base = rng.integers(0, 255, 4)
        tiles.append((base + rng.integers(0, 2, (4, 4, 4))).astype(np.uint8))
    for _ in range(20):   # smooth gradients
        a, b = rng.integers(0, 256, 4).astype(np.float64), rng.integers(0, 256, 4).astype(np.float64)
        w = (np.arange(16).reshape(4, 4, 1) / 15.0)
        tiles.append(np.clip(a + (b - a) * w + rng.normal(0, 3, (4, 4, 4)), 0, 255).astype(np.uint8))
    while len(tiles) < 256:
        tiles.append(rng.integers(0, 256, (4, 4, 4)).astype(np.uint8))
    return np.ascontiguousarray(np.stack(tiles[:256]))


def tiles_to_image(tiles, nbx):
    """(n, 4, 4, 4) tiles in raster order -> the (4 n / nbx, 4 nbx, 4) image they tile"""
    n = tiles.shape[0]
    return np.ascontiguousarray(tiles.reshape(n // nbx, nbx, 4, 4, 4).transpose(0, 2, 1, 3, 4).reshape(n // nbx * 4, nbx * 4, 4))


def cover_image():
    return tiles_to_image(cover_tiles(), 16)


def _faces():
    faces = [helpers.synth(16, 16, 500 + i) for i in range(6)]
    yy, xx = np.mgrid[0:16, 0:16]
    faces[3][..., 3] = np.clip(40 + xx * 9 + yy * 4, 0, 255).astype(np.uint8)
    return faces


def cases():
    """name -> {"images", "fmt", "tool": the tool's arguments behind `-dds -dds_format <fmt>`, "kw": export_dds()'s}. Every group also has its a8b8g8r8 file: the
    prepared pixels themselves, from which the host build reproduces the group's block payloads, and which tells a source-stage difference from an encoder's."""
    o20 = np.ascontiguousarray(helpers.synth(20, 28, 12))
    out = {}

    def add(group, images, formats, tool, kw):
        for fmt in dict.fromkeys((*formats, "a8b8g8r8")):
            out[f"{group}_{fmt}"] = dict(images=images, fmt=fmt, tool=list(tool), kw=dict(kw))
    add("o20", [o20], BLOCK_FORMATS + RAW_FORMATS, ["-mipmap"], dict(mipmaps=True))
    add("alpha", [alpha_image()], ("bc2", "bc3", "a8r8g8b8", "a1r5g5b5", "a4r4g4b4"), ["-mipmap"], dict(mipmaps=True))
    add("photo", [photo_image()], ("bc1", "bc3"), [], {})
    add("cover", [cover_image()], ("bc1", "bc3", "bc5"), [], {})
    add("array", [helpers.synth(16, 16, 520), helpers.synth(16, 16, 521)], ("bc1",), ["-tex_type", "2darray", "-mipmap"], dict(tex_type="2darray", mipmaps=True))
    add("cube", _faces(), ("bc3",), ["-tex_type", "cubemap", "-mipmap"], dict(tex_type="cubemap", mipmaps=True))
    add("linear", [o20], ("bc1", "bc4"), ["-linear"], dict(srgb=False))
    add("yflip", [o20], ("bc1",), ["-y_flip"], dict(y_flip=True))
    add("rg", [o20], ("bc5",), ["-separate_rg_to_color_alpha"], dict(swizzle="rrrg"))
    add("normal", [o20], ("bc5",), ["-normal_map"], dict(srgb=False, mip_srgb=False))
    add("resample", [o20], ("a8b8g8r8",), ["-resample", "12", "20"], dict(resample=(12, 20)))
    return out


@functools.lru_cache(maxsize=None)
def golden():
    """-> (arrays, meta) of dds_export_vectors.npz, loaded once and shared, read-only: file_<case> (the tool's .dds bytes), image_<group>_<i> (the source pixels)"""
    return native_libs.load_npz_golden(GOLDEN)


def group_of(name):
    """"o20_bc1" -> "o20": the cases of a group differ only in their format"""
    return name.rsplit("_", 1)[0]


def golden_images(arrays, name):
    """the source images of a case (stored once per group)"""
    out, i = [], 0
    while f"image_{group_of(name)}_{i}" in arrays:
        out.append(arrays[f"image_{group_of(name)}_{i}"])
        i += 1
    return out


# ---- the host build of dds_pack.h

def host():
    return native_libs.load("dds_pack_host")


def host_pack_blocks(tiles, fmt):
    """(n, 64 bytes) tiles -> (n, 8 | 16) blocks by the g++ build of the per-tile packers"""
    from basis_universal_amd import dds
    code, _, unit, _, _ = dds.FORMATS[fmt]
    tiles = np.ascontiguousarray(tiles, np.uint8).reshape(-1, 64)
    out = np.zeros((tiles.shape[0], unit), np.uint8)
    assert host().hd_pack_blocks(tiles.ctypes.data, tiles.shape[0], code, out.ctypes.data) == 1
    return out


def host_pack_pixels(rgba, fmt):
    """(..., 4) texels -> the tight bytes of a raw format by the g++ build of the per-pixel packer"""
    from basis_universal_amd import dds
    code, _, unit, _, _ = dds.FORMATS[fmt]
    rgba = np.ascontiguousarray(rgba, np.uint8).reshape(-1, 4)
    out = np.zeros(rgba.shape[0] * unit, np.uint8)
    assert host().hd_pack_pixels(rgba.ctypes.data, rgba.shape[0], code, out.ctypes.data) == 1
    return out


def a8b8g8r8_twin(arrays, name):
    """the prepared pixels of a case: the a8b8g8r8 file of its group, as {(level, layer, face): (h, w, 4) raster}; None where the group has no such file"""
    from basis_universal_amd import dds
    key = f"file_{group_of(name)}_a8b8g8r8"
    if key not in arrays:
        return None
    raw = arrays[key].tobytes()
    info = dds.read_dds(raw)
    return {(im["level"], im["layer"], im["face"]): np.frombuffer(raw, np.uint8, im["nbytes"], im["offset"]).reshape(im["height"], im["width"], 4) for im in info["images"]}

