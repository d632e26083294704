"""Test-only helpers of the UASTC texture family's tests (ETC1, ETC2 RGBA, EAC R11 / RG11, the 16-bit rasters): the g++ build of the second half of
basis_universal_amd/csrc/uastc_transcode.h (tests/native/uastc_texture_host.cpp), the cases of tests/golden/uastc_texture_vectors.npz (one table for
tools/gen_golden_uastc_texture.py and the tests), and the conditions that fixture is written under."""
import ctypes as C
import functools
import pathlib

import numpy as np

import native_libs
import transcode_helpers as T

ROOT = pathlib.Path(__file__).resolve().parent.parent
NATIVE = native_libs.NATIVE
native_libs.CHECKERS.setdefault("uastc_texture_host", (NATIVE / "libuastc_texture_host.so", NATIVE / "uastc_texture_host.cpp", "HOST_API", "g++"))

GOLDEN = ROOT / "tests" / "golden" / "uastc_texture_vectors.npz"
GRID_W = 64

# transcoder_texture_format values (basis_universal_amd.transcode has the same constants; kept here so the host tests do not need the package's library)
ETC1, ETC2, RGB565, BGR565, RGBA4444, R11, RG11 = 0, 1, 14, 15, 16, 20, 21
NEW_BLOCK_TARGETS = {ETC1: 8, ETC2: 16, R11: 8, RG11: 16}
REFUSED_TARGETS = (7, 8, 9, 11, 12, 17, 18, 19, 22, 23, 255, 2 ** 31)
# fixture array suffix -> (target, high quality, the reference tool's file tag): what `basisu -unpack -ktx_only` writes; its R11 is channel 0, its RG11 channels 0 and 3
BLOCK_CASES = {"etc1": (ETC1, False, "ETC1_RGB"), "etc2": (ETC2, False, "ETC2_RGBA"), "r11": (R11, False, "ETC2_EAC_R11"), "rg11": (RG11, False, "ETC2_EAC_RG11"),
               "r11_hq": (R11, True, "ETC2_EAC_R11"), "rg11_hq": (RG11, True, "ETC2_EAC_RG11")}
ENCODER_SETS = ("level3", "level2", "default_l2")
PIXEL_SET = "level2"        # the set whose 16-bit rasters are stored, whole and cropped
CROP_W = 254                # the cropped declaration: 254 x (4 * nby - 3) pixels of the same blocks

u8p = C.POINTER(C.c_uint8)


def texture_host():
    return native_libs.load("uastc_texture_host")


def _p(a):
    return a.ctypes.data_as(u8p)


def host_texture(blocks, target, high_quality=False, channels=(0, 3)):
    """-> (per-block output (n, bytes) uint8 -- pixel targets: the 16 texels in raster order, 64 or 32 bytes --, ok flags (n,) uint8). Refused blocks are zero-filled."""
    L = texture_host()
    blocks = np.ascontiguousarray(blocks, np.uint8).reshape(-1, 16)
    n, unit = blocks.shape[0], L.ht_texture_block_bytes(int(target))
    assert unit, f"target {target} is not one of the family's"
    out, ok = np.zeros((n, unit), np.uint8), np.zeros(n, np.uint8)
    L.ht_texture(_p(blocks), n, int(target), int(high_quality), channels[0], channels[1], _p(out), _p(ok))
    return out, ok


def host_pack_eac(values, high_quality=False):
    """pack_eac / pack_eac_high_quality of (n, 16) raw values in raster order -> (n, 8) uint8"""
    values = np.ascontiguousarray(values, np.uint8).reshape(-1, 16)
    out = np.zeros((values.shape[0], 8), np.uint8)
    texture_host().ht_pack_eac(_p(values), values.shape[0], int(high_quality), _p(out))
    return out


def etc_hints(blocks):
    """per block (n, 8) uint8: [0] 0 refused / 1 solid / 2 other, [1] flip, [2] diff, [3] inten0, [4] inten1, [5] bias, [6] EAC byte, [7] 1 = bias-carrying mode | 2 = alpha mode"""
    blocks = np.ascontiguousarray(blocks, np.uint8).reshape(-1, 16)
    out = np.zeros((blocks.shape[0], 8), np.uint8)
    texture_host().ht_etc_hints(_p(blocks), blocks.shape[0], _p(out))
    return out


def tiles16_to_raster(tiles, nbx, nby, width, height):
    """(nby * nbx, 32) bytes of 16-bit tiles -> the (height, width) u16 image they cover, cropped"""
    t = np.ascontiguousarray(tiles, np.uint8).reshape(-1, 32).view("<u2").reshape(nby, nbx, 4, 4)
    return np.ascontiguousarray(t.transpose(0, 2, 1, 3).reshape(nby * 4, nbx * 4)[:height, :width])


def swap_565(img):
    """RGB565 <-> BGR565: the two 5-bit fields exchanged"""
    img = np.asarray(img, np.uint16)
    return ((img & 0x1F) << 11) | (img & 0x07E0) | (img >> 11)


def eac_multiplier(blocks8):
    return np.asarray(blocks8, np.uint8).reshape(-1, 8)[:, 1] >> 4


@functools.lru_cache(maxsize=None)
def golden():
    """(arrays, meta) of the committed fixture, read-only"""
    return native_libs.load_npz_golden(GOLDEN)


def encoder_grid(name):
    """the (blocks, nbx, nby) of one of the three encoder sets, exactly as uastc_transcode_vectors.npz lays them out"""
    g = np.load(ROOT / "tests" / "golden" / "uastc_transcode_vectors.npz")
    nbx, nby, _ = (int(v) for v in g[f"{name}_grid"])
    return np.ascontiguousarray(g[f"{name}_blocks"]), nbx, nby


def fuzz_valid_grid():
    """the valid blocks of uastc_transcode_fuzz.npz as a 64-wide grid (tail padded with the first solid block among them) -> (grid, nbx, nby, n valid, their
    indices in the fuzz file)"""
    z = np.load(ROOT / "tests" / "golden" / "uastc_transcode_fuzz.npz")
    idx = np.flatnonzero(z["valid"] != 0)
    blocks = np.ascontiguousarray(z["blocks"][idx])
    solid = blocks[np.flatnonzero(T.code_modes(blocks) == 8)[0]]
    nby = -(-blocks.shape[0] // GRID_W)
    return np.concatenate([blocks, np.repeat(solid[None], GRID_W * nby - blocks.shape[0], 0)]), GRID_W, nby, blocks.shape[0], idx


def check_hint_coverage(blocks):
    """The conditions the fuzz part of the fixture is written under, on blocks the core accepts (asserted by tools/gen_golden_uastc_texture.py before it writes, and
    by tests/test_uastc_texture_host.py on the committed inputs) -> the counts, for the fixture's meta."""
    h = etc_hints(blocks)
    assert (h[:, 0] != 0).all(), "a refused block among the valid ones"
    ns = h[h[:, 0] == 2]
    flip_diff = np.bincount(ns[:, 1] | (ns[:, 2] << 1), minlength=4)
    tables = np.bincount(np.concatenate([ns[:, 3], ns[:, 4]]), minlength=8)
    alpha = ns[(ns[:, 7] & 2) != 0]
    eac_tables = np.bincount(alpha[:, 6] & 15, minlength=16)
    bias = (int(((ns[:, 7] & 1) != 0).sum()), int(((ns[:, 7] & 1) == 0).sum()))
    mul0 = int(((alpha[:, 6] >> 4) == 0).sum())
    assert (flip_diff >= 100).all(), flip_diff
    assert (tables >= 100).all(), tables
    assert (eac_tables >= 100).all(), eac_tables
    assert min(bias) >= 100, bias
    assert mul0 >= 20, mul0
    return {"flip_diff": flip_diff.tolist(), "inten_tables": tables.tolist(), "eac_tables": eac_tables.tolist(), "bias_modes_with_without": list(bias), "eac_multiplier_0": mul0}
