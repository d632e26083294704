"""Test-only helpers of the block unpacker tests: the g++ build of basis_universal_amd/csrc/block_unpack.h (tests/native/block_unpack_host.cpp), the golden files
(tests/golden/block_unpack_vectors.npz, bc7_stats_vectors.npz) and what the generator and the tests both need to know about a BC7 block's leading fields."""
import ctypes as C
import functools
import pathlib

import numpy as np

import native_libs

ROOT = pathlib.Path(__file__).resolve().parent.parent
GOLDEN = ROOT / "tests" / "golden" / "block_unpack_vectors.npz"
GOLDEN_STATS = ROOT / "tests" / "golden" / "bc7_stats_vectors.npz"
u8p = C.POINTER(C.c_uint8)

# transcoder_texture_format values (basis_universal_amd.transcode has the same constants; kept here so the host tests do not need the package's library)
BC1, BC3, BC4, BC5, BC7 = 2, 3, 4, 5, 6
BYTES = {BC1: 8, BC3: 16, BC4: 8, BC5: 16, BC7: 16}
NAMES = {BC1: "bc1", BC3: "bc3", BC4: "bc4", BC5: "bc5", BC7: "bc7"}
# the encoder-made members: array of uastc_transcode_vectors.npz -> format
ENCODER_MADE = {"level2_bc1": BC1, "level2_bc1_hq": BC1, "level2_bc3": BC3, "level2_bc4_r": BC4, "level2_bc5_ra": BC5, "level2_bc7": BC7}


def host():
    return native_libs.load("block_unpack_host")


def host_unpack(blocks, fmt):
    """-> (texels (n, 16, 4) uint8 in raster order, ok flags (n,) uint8). An invalid block (BC7, byte 0 == 0) is zero-filled."""
    blocks = np.ascontiguousarray(blocks, np.uint8).reshape(-1, BYTES[fmt])
    n = blocks.shape[0]
    out, ok = np.zeros((n, 16, 4), np.uint8), np.zeros(n, np.uint8)
    assert host().bh_unpack(blocks.ctypes.data_as(u8p), n, fmt, out.ctypes.data_as(u8p), ok.ctypes.data_as(u8p))
    return out, ok


def host_bc1_four_colour(blocks):
    blocks = np.ascontiguousarray(blocks, np.uint8).reshape(-1, 8)
    out = np.zeros((blocks.shape[0], 16, 4), np.uint8)
    host().bh_bc1_four(blocks.ctypes.data_as(u8p), blocks.shape[0], out.ctypes.data_as(u8p))
    return out


def to_raster(texels, nbx, nby, width, height):
    """(nby * nbx, 16, 4) texels -> the (height, width, 4) image they cover, cropped"""
    return texels.reshape(nby, nbx, 4, 4, 4).transpose(0, 2, 1, 3, 4).reshape(nby * 4, nbx * 4, 4)[:height, :width]


@functools.lru_cache(maxsize=None)
def golden():
    """-> (arrays, meta) of block_unpack_vectors.npz: loaded once and shared; nobody writes into the arrays"""
    return native_libs.load_npz_golden(GOLDEN)


@functools.lru_cache(maxsize=None)
def golden_stats():
    return native_libs.load_npz_golden(GOLDEN_STATS)


def format_set(fmt):
    """every golden block of a format, the constructed ones and the encoder-made ones -> (blocks (n, bytes), texels (n, 16, 4), ok (n,))"""
    arrays, _ = golden()
    name = NAMES[fmt]
    keys = [name] + [k for k, f in ENCODER_MADE.items() if f == fmt]
    blocks = np.concatenate([arrays[k + "_blocks"] for k in keys])
    texels = np.concatenate([arrays[k + "_texels"] for k in keys])
    ok = np.concatenate([arrays[k + "_ok"] for k in keys])
    return blocks, texels, ok


# ---------------------------------------------------------------- BC7's leading fields, from the format: mode = lowest set bit of byte 0

BC7_PARTITION_BITS = {0: 4, 1: 6, 2: 6, 3: 6, 7: 6}


def bc7_modes(blocks):
    """per block: 0..7, or -1 for the reserved mode (byte 0 == 0)"""
    b0 = np.ascontiguousarray(blocks, np.uint8).reshape(-1, 16)[:, 0].astype(np.int64)
    return np.where(b0 == 0, -1, np.log2(np.maximum(b0 & -b0, 1)).astype(np.int64))


def field(block, ofs, width):
    """bits ofs .. ofs + width of a block, little-endian bit order"""
    return (int.from_bytes(np.asarray(block, np.uint8).tobytes(), "little") >> ofs) & ((1 << width) - 1)


def bc7_setting(block, mode):
    """the field that follows the mode bits: the partition (modes 0-3, 7), (rotation, index selection) as rotation | selection << 2 (mode 4), the rotation (mode 5)"""
    if mode in BC7_PARTITION_BITS:
        return field(block, mode + 1, BC7_PARTITION_BITS[mode])
    if mode == 4:
        return field(block, 5, 3)
    if mode == 5:
        return field(block, 6, 2)
    return 0


# endpoint field extents per mode: (first bit, number of bits) of the endpoint values and p-bits together
BC7_ENDPOINT_FIELDS = {0: (5, 78), 1: (8, 74), 2: (9, 90), 3: (10, 88), 4: (8, 42), 5: (8, 58), 6: (7, 58), 7: (14, 84)}


def endpoint_orders(blocks, lo_at, width):
    """per block: +1 low > high, -1 low < high, 0 equal, for two `width`-bit endpoints at bit lo_at and lo_at + width"""
    return np.array([np.sign(field(b, lo_at, width) - field(b, lo_at + width, width)) for b in blocks], np.int64)


def check_coverage(arrays, meta):
    """The conditions block_unpack_vectors.npz is written under, counted from the blocks themselves (asserted by tools/gen_golden_block_unpack.py before it writes,
    and by tests/test_block_unpack_host.py on the committed file). -> {what: count} for the record."""
    seen = {}
    blocks, ok = arrays["bc7_blocks"], arrays["bc7_ok"]
    modes = bc7_modes(blocks)
    assert ((modes == -1) == (ok == 0)).all(), "the reference refuses exactly the blocks whose first byte is 0"
    assert int((modes == -1).sum()) == 16 == meta["bc7_counts"]["reserved"]
    for mode in range(8):
        mine = blocks[modes == mode]
        assert mine.shape[0] == meta["bc7_counts"][str(mode)], (mode, mine.shape[0])
        settings = np.bincount([bc7_setting(b, mode) for b in mine])
        want_settings, per = {4: (8, 32), 5: (4, 32), 6: (1, 256)}.get(mode, (1 << BC7_PARTITION_BITS.get(mode, 0), 8))
        assert settings.shape[0] == want_settings and (settings >= per).all(), (mode, settings.tolist())
        first, length = BC7_ENDPOINT_FIELDS[mode]
        ends = [field(b, first, length) for b in mine]
        assert sum(e == 0 for e in ends) >= 4 and sum(e == (1 << length) - 1 for e in ends) >= 4, mode
        seen[f"bc7 mode {mode}"] = int(mine.shape[0])
    for name, lo_at, width in (("bc1", 0, 16), ("bc4", 0, 8)):
        b = arrays[name + "_blocks"]
        orders = endpoint_orders(b, lo_at, width)
        for o in (1, -1, 0):
            assert (orders == o).sum() >= 64, (name, o)
        seen[name] = int(b.shape[0])
    b = arrays["bc1_blocks"]
    orders = endpoint_orders(b, 0, 16)
    index3 = np.array([any(field(x, 32 + 2 * t, 2) == 3 for t in range(16)) for x in b])
    for o in (1, -1, 0):
        assert (index3 & (orders == o)).any(), f"no BC1 block of endpoint order {o} uses index 3"
    ends = {(int(x[0]), int(x[1])) for x in arrays["bc4_blocks"]}
    assert (0, 255) in ends and (255, 0) in ends
    assert (endpoint_orders(arrays["bc3_blocks"], 64, 16) <= 0).sum() >= 64
    seen["bc3"], seen["bc5"] = int(arrays["bc3_blocks"].shape[0]), int(arrays["bc5_blocks"].shape[0])
    assert arrays["bc3_blocks"].shape[0] >= 256 + 64 and arrays["bc5_blocks"].shape[0] >= 256
    for name, fmt in ENCODER_MADE.items():
        assert arrays[name + "_blocks"].shape == (512, BYTES[fmt]) and arrays[name + "_ok"].all(), name
    return seen
