"""The host half of the tile / raster layer (basis_universal_amd/csrc/tile_geometry_check.h through tests/native/tile_geometry_host.cpp): the refusal texts the
entries of the C ABI give for a bad geometry or slice table -- the ones test_gpu_transcode_slices, test_gpu_dds_export, test_gpu_extract_slices, test_gpu_block_unpack
and the one-image transcoders' tests assert on a GPU -- and the normalised records and prefix tables the kernels read. Nothing here needs a GPU."""
import ctypes as C

import numpy as np
import pytest

import native_libs
from basis_universal_amd.source import SliceSource
from basis_universal_amd.transcode import NO_ALPHA_SLICE, TranscodeSlice

UASTC, ETC1S, DDS = 0, 1, 2
OUT = 0x7000_0000_0000      # a device address: never read
FIRST, ALPHA, OFF, NBX, NBY, W, H, PITCH, ROWS = range(9)


def host():
    return native_libs.load("tile_geometry_host")


def resolve(who, uastc, *six):
    out, err = (C.c_uint32 * 6)(), C.create_string_buffer(512)
    ok = host().tg_resolve(who.encode(), int(uastc), *six, out, err, len(err))
    return (tuple(out), "") if ok else (None, err.value.decode())


def records(specs):
    return (TranscodeSlice * max(len(specs), 1))(*[TranscodeSlice(f, NO_ALPHA_SLICE if a is None else a, *rest) for f, a, *rest in specs])


def transcode_table(policy, fn, specs, n_inputs, unit, pixels, out_bytes, target_name="BC1_RGB", d_out=OUT, n_slices=None, null_slices=False):
    """-> (records as uploaded, prefix, layout) or the refusal's text"""
    pack, layout, err = np.zeros(1 << 16, np.uint8), (C.c_uint64 * 4)(), C.create_string_buffer(512)
    n = len(specs) if n_slices is None else n_slices
    ok = host().tg_transcode_table(policy, fn.encode(), None if null_slices else records(specs), n, n_inputs, unit, int(pixels), target_name.encode(), d_out, out_bytes,
                                   pack.ctypes.data_as(C.c_void_p), pack.size, layout, err, len(err))
    if ok != 1:
        assert ok == 0, "the wrapper's own check of the pack failed"
        return err.value.decode()
    size, prefix_at, counters_at, total = layout
    recs = np.frombuffer(pack[:prefix_at].tobytes(), np.dtype([("u64", "<u8", 3), ("u32", "<u4", 6)]))
    prefix = np.frombuffer(pack[prefix_at:counters_at].tobytes(), "<u4")
    return recs, prefix, (size, prefix_at, counters_at, total)


# ---------------------------------------------------------------- one image: transcode_uastc, transcode_etc1s, unpack_blocks

@pytest.mark.parametrize("who,uastc", [("transcode_uastc", True), ("transcode_etc1s", False), ("unpack_blocks", False)])
def test_one_image_defaults_and_refusals(who, uastc):
    assert resolve(who, uastc, 2, 2, 0, 0, 0, 0) == ((2, 2, 8, 8, 8, 8), "")
    assert resolve(who, uastc, 1, 1, 0, 0, 0, 0) == ((1, 1, 4, 4, 4, 4), "")
    assert resolve(who, uastc, 2, 2, 5, 7, 0, 0) == ((2, 2, 5, 7, 5, 7), "")
    assert resolve(who, uastc, 2, 2, 5, 7, 10, 5) == ((2, 2, 5, 7, 10, 5), "")     # pitch w + 5, rows h - 2
    assert resolve(who, uastc, 17, 16, 0, 0, 0, 0) == ((17, 16, 68, 64, 68, 64), "")
    assert resolve(who, uastc, 2, 2, 8, 8, 7, 0) == (None, f"{who}: row pitch 7 is less than the width 8")
    assert resolve(who, uastc, 2, 2, 9, 8, 0, 0) == (None, f"{who}: 9 x 8 pixels do not fit 2 x 2 blocks")
    assert resolve(who, uastc, 2, 2, 8, 9, 0, 0) == (None, f"{who}: 8 x 9 pixels do not fit 2 x 2 blocks")
    if uastc:    # any grid of up to 2^31 - 1 blocks
        assert resolve(who, uastc, 16385, 1, 0, 0, 0, 0)[0] == (16385, 1, 65540, 4, 65540, 4)
        assert resolve(who, uastc, 65536, 32768, 0, 0, 0, 0) == (None, "transcode_uastc: 65536 x 32768 blocks is too many")
        assert resolve(who, uastc, 65536, 32767, 0, 0, 0, 0)[0] is not None
    else:
        assert resolve(who, uastc, 16384, 1, 0, 0, 0, 0)[0] is not None
        assert resolve(who, uastc, 16385, 1, 0, 0, 0, 0) == (None, f"{who}: 16385 x 1 blocks is too many (16384 each way at the most)")
        assert resolve(who, uastc, 1, 16385, 0, 0, 0, 0) == (None, f"{who}: 1 x 16385 blocks is too many (16384 each way at the most)")


def test_output_bytes():
    b = host().tg_output_bytes
    assert b(2, 2, 0, 0, 0, 0, 4, 1) == 256 and b(2, 2, 5, 7, 0, 0, 4, 1) == 5 * 7 * 4 and b(2, 2, 5, 7, 9, 3, 4, 1) == 9 * 3 * 4    # unpack_output_bytes' cases
    assert b(2, 2, 5, 7, 9, 3, 2, 1) == 9 * 3 * 2 and b(17, 16, 0, 0, 0, 0, 1, 1) == 68 * 64
    assert b(2, 2, 5, 7, 9, 3, 8, 0) == 32 and b(17, 16, 0, 0, 0, 0, 16, 0) == 272 * 16         # a block target: blocks x unit whatever the pixels are
    assert b(2, 2, 0, 0, 0, 0, 0, 0) == 0 and b(2, 2, 0, 0, 0, 0, 0, 1) == 0                   # a target the codec does not have
    assert b(16384, 16384, 0, 0, 0, 0, 4, 1) == 65536 * 65536 * 4                               # in size_t


# ---------------------------------------------------------------- the whole-file transcoders' table

def _table(**change):
    specs = [[4 * k, None, 512 * k, 2, 2, 0, 0, 0, 0] for k in range(4)]
    for k, fields in change.items():
        for i, v in fields.items():
            specs[int(k[1:])][i] = v
    return [tuple(s) for s in specs]


@pytest.mark.parametrize("etc1s", [False, True])
def test_transcoder_table_refusals(etc1s):
    """test_gpu_transcode_slices.py's cases: a 4-slice table of 2 x 2 blocks, 64 inputs, 2048 bytes of output"""
    fn, inputs = ("transcode_etc1s_slices", "indices") if etc1s else ("transcode_uastc_slices", "blocks")
    policy = ETC1S if etc1s else UASTC
    pixel, block = (4, True, "RGBA32"), (8, False, "BC1_RGB")
    size = 256

    def refused(specs, target, n_inputs=64, **kw):
        got = transcode_table(policy, fn, specs, n_inputs, target[0], target[1], 2048, target[2], **kw)
        assert isinstance(got, str), "accepted"
        return got
    assert refused([], pixel) == f"{fn}: no slices (n_slices == 0)"
    assert refused(_table(s1={NBX: 0}), pixel) == f"{fn}: slice 1: zero blocks (0 x 2)"
    assert refused(_table(s3={NBY: 0}), block) == f"{fn}: slice 3: zero blocks (2 x 0)"
    assert refused(_table(s0={NBX: 16385}), block) == f"{fn}: slice 0: 16385 x 2 blocks is too many (16384 each way at the most)"
    assert refused(_table(s2={NBY: 16385}), pixel) == f"{fn}: slice 2: 2 x 16385 blocks is too many (16384 each way at the most)"
    assert refused(_table(s1={W: 9}), pixel) == f"{fn}: slice 1: 9 x 8 pixels do not fit 2 x 2 blocks"
    assert refused(_table(s1={H: 9}), block) == f"{fn}: slice 1: 8 x 9 pixels do not fit 2 x 2 blocks"
    assert refused(_table(s2={W: 7, PITCH: 6}), pixel) == f"{fn}: slice 2: row pitch 6 is less than the width 7"
    assert refused(_table(s1={PITCH: 8}), block) == f"{fn}: slice 1: row pitch 8 / rows 0 given for a block target (BC1_RGB): they describe a pixel raster"
    assert refused(_table(s1={ROWS: 8}), block) == f"{fn}: slice 1: row pitch 0 / rows 8 given for a block target (BC1_RGB): they describe a pixel raster"
    assert refused(_table(s1={PITCH: 1}), block).startswith(f"{fn}: slice 1: row pitch 1 / rows 0 given for a block target")     # never "less than the width"
    assert refused(_table(s3={FIRST: 61}), pixel) == f"{fn}: slice 3: {inputs} 61..65 are past the 64 given"
    assert refused(_table(), block, n_inputs=15) == f"{fn}: slice 3: {inputs} 12..16 are past the 15 given"
    assert refused(_table(s0={FIRST: 2 ** 63}), block).startswith(f"{fn}: slice 0: {inputs} {2 ** 63}..")
    assert refused(_table(s1={OFF: 520}), pixel) == f"{fn}: slice 1: out_offset 520 is not 16-byte aligned"
    assert refused(_table(s3={OFF: 2048 - size + 16}), pixel) == f"{fn}: slice 3: its output, bytes 1808..2064, ends past out_bytes = 2048"
    assert refused(_table(s3={OFF: 4096}), block) == f"{fn}: slice 3: its output, bytes 4096..4128, ends past out_bytes = 2048"
    assert refused(_table(s2={OFF: 512 + size - 16}), pixel) == (f"{fn}: slice 2: out_offset 752 lies before the end of slice 1's output (768): "
                                                                 "outputs must ascend without overlap")
    assert refused(_table(s1={OFF: 1024}, s2={OFF: 512}), block) == (f"{fn}: slice 2: out_offset 512 lies before the end of slice 1's output (1056): "
                                                                     "outputs must ascend without overlap")
    if etc1s:
        assert refused(_table(s1={ALPHA: 62}), pixel) == f"{fn}: slice 1: alpha indices 62..66 are past the 64 given"
    else:
        assert refused(_table(s2={ALPHA: 0}), pixel) == f"{fn}: slice 2: alpha_first_block is set, and a UASTC image has no alpha slice"
    assert refused(_table(), pixel, null_slices=True) == f"{fn}: null pointer"
    assert refused(_table(), pixel, d_out=0) == f"{fn}: null pointer"
    assert refused(_table(), pixel, d_out=OUT + 8) == f"{fn}: the output is not 16-byte aligned"
    big = [(0, None, k * 2 ** 31, 16384, 16384, 0, 0, 0, 0) for k in range(5)]    # 5 x 2^28 blocks reading the same range: refused on the count alone
    got = transcode_table(policy, fn, big, 2 ** 28, 8, False, 2 ** 40)
    assert got == f"{fn}: more than 2^30 blocks in one call (at slice 4)"
    assert not isinstance(transcode_table(policy, fn, big[:4], 2 ** 28, 8, False, 2 ** 40), str)    # 2^30 itself is taken


@pytest.mark.parametrize("etc1s", [False, True])
def test_transcoder_table_as_the_kernels_read_it(etc1s):
    fn, policy = "t", ETC1S if etc1s else UASTC
    alpha = 300 if etc1s else None
    # a single block; 5 x 7 pixels at pitch w + 5 with rows h - 2; 17 x 16 blocks; 1 x 5 pixels
    specs = [(0, None, 0, 1, 1, 0, 0, 0, 0), (1, alpha, 64, 2, 2, 5, 7, 10, 5), (5, None, 64 + 10 * 5 * 4 + 8, 17, 16, 0, 0, 0, 0), (277, None, 17680, 1, 2, 1, 5, 0, 0)]
    recs, prefix, (size, prefix_at, counters_at, total) = transcode_table(policy, fn, specs, 600, 4, True, 17680 + 5 * 4, "RGBA32")
    assert (prefix_at, counters_at, size) == (4 * 48, 4 * 48 + 5 * 4, 4 * 48 + 5 * 4 + 4 * 4)     # records, prefix[n + 1], a counter per slice
    assert prefix.tolist() == [0, 1, 5, 277, 279] and total == 279
    assert recs["u64"].tolist() == [[0, NO_ALPHA_SLICE, 0], [1, NO_ALPHA_SLICE if alpha is None else alpha, 64], [5, NO_ALPHA_SLICE, 272], [277, NO_ALPHA_SLICE, 17680]]
    assert recs["u32"].tolist() == [[1, 1, 4, 4, 4, 4], [2, 2, 5, 7, 10, 5], [17, 16, 68, 64, 68, 64], [1, 2, 1, 5, 1, 5]]
    # a block target: the zeros of pitch / rows are filled in all the same, and a slice takes blocks x unit bytes
    specs = [(0, None, 0, 2, 2, 5, 7, 0, 0), (4, None, 32, 17, 16, 0, 0, 0, 0)]
    recs, prefix, layout = transcode_table(policy, fn, specs, 276, 8, False, 32 + 272 * 8)
    assert prefix.tolist() == [0, 4, 276] and recs["u32"].tolist() == [[2, 2, 5, 7, 5, 7], [17, 16, 68, 64, 68, 64]]
    assert transcode_table(policy, fn, specs, 276, 8, False, 32 + 272 * 8 - 1) == "t: slice 1: its output, bytes 32..2208, ends past out_bytes = 2207"


# ---------------------------------------------------------------- the DDS pixel packer's table

def _dds(first, nbx, nby, w=0, h=0, at=0, alpha=None, pitch=0, rows=0):
    return (first, alpha, at, nbx, nby, w, h, pitch, rows)


def test_dds_pixel_table_refusals_and_pack():
    """test_gpu_dds_export.py's cases: 8 tiles, 4096 bytes of output"""
    fn = "pack_dds_pixels"

    def table(specs, unit=4, n_tiles=8, out_bytes=4096, **kw):
        return transcode_table(DDS, fn, specs, n_tiles, unit, True, out_bytes, "", **kw)
    one = [_dds(0, 2, 2)]
    assert table(one, n_slices=0) == f"{fn}: no slices (n_slices == 0)"
    assert table(one, null_slices=True) == f"{fn}: null pointer"
    assert table([_dds(0, 0, 2)]) == f"{fn}: slice 0: zero blocks (0 x 2)"
    assert table([_dds(0, 16385, 1)], n_tiles=1 << 20) == f"{fn}: slice 0: 16385 x 1 blocks is too many (16384 each way at the most)"
    assert table([_dds(0, 2, 2, w=9, h=8)]) == f"{fn}: slice 0: 9 x 8 pixels do not fit 2 x 2 blocks"
    assert table([_dds(0, 2, 2, pitch=8)]) == f"{fn}: slice 0: row pitch 8 / rows 0 given: the rows of a DDS subresource are tight"
    assert table([_dds(0, 2, 2, rows=8)]) == f"{fn}: slice 0: row pitch 0 / rows 8 given: the rows of a DDS subresource are tight"
    assert table([_dds(0, 2, 2, alpha=0)]) == f"{fn}: slice 0: alpha_first_block is set, and a tile carries its own alpha"
    assert table([_dds(5, 2, 2)]) == f"{fn}: slice 0: tiles 5..9 are past the 8 given"
    assert table([_dds(9, 1, 1)]) == f"{fn}: slice 0: tiles 9..10 are past the 8 given"
    assert table([_dds(0, 1, 1, w=3, h=3, at=2)]) == f"{fn}: slice 0: out_offset 2 is not a multiple of the pixel size 4"
    assert table([_dds(0, 1, 1, w=3, h=3, at=1)], unit=2) == f"{fn}: slice 0: out_offset 1 is not a multiple of the pixel size 2"
    assert table([_dds(0, 1, 1), _dds(1, 1, 1, at=32)]) == f"{fn}: slice 1: out_offset 32 lies before the end of slice 0's output (64): outputs must ascend without overlap"
    assert table([_dds(0, 2, 2)], out_bytes=255) == f"{fn}: slice 0: its output, bytes 0..256, ends past out_bytes = 255"
    assert table([_dds(0, 1, 1), _dds(1, 1, 1, at=4064)]) == f"{fn}: slice 1: its output, bytes 4064..4128, ends past out_bytes = 4096"
    big = [_dds(0, 16384, 16384, at=k * 2 ** 34) for k in range(5)]
    assert table(big, n_tiles=2 ** 28, out_bytes=2 ** 40) == f"{fn}: more than 2^30 tiles in one call (at slice 4)"
    # the table the GPU test has taken: tight rows at offsets that are multiples of the pixel size only, no counters behind the prefix
    ok = [_dds(0, 1, 1, w=3, h=3), _dds(4, 2, 2, w=5, h=6, at=36)]
    recs, prefix, (size, prefix_at, counters_at, total) = table(ok, out_bytes=156)
    assert (prefix_at, counters_at, size, total) == (96, 108, 108, 5) and prefix.tolist() == [0, 1, 5]
    assert recs["u64"].tolist() == [[0, NO_ALPHA_SLICE, 0], [4, NO_ALPHA_SLICE, 36]] and recs["u32"].tolist() == [[1, 1, 3, 3, 3, 3], [2, 2, 5, 6, 5, 6]]
    assert table(ok, out_bytes=155) == f"{fn}: slice 1: its output, bytes 36..156, ends past out_bytes = 155"
    recs, prefix, _ = table([_dds(0, 1, 1, w=3, h=3), _dds(4, 2, 2, w=5, h=6, at=9)], unit=1, out_bytes=39)     # r8: one byte per pixel, odd offsets
    assert prefix.tolist() == [0, 1, 5] and recs["u64"][1].tolist() == [4, NO_ALPHA_SLICE, 9]


# ---------------------------------------------------------------- extract_slices' table

def source_table(entries, d_out=OUT, null_slices=False, n=None):
    arr = (SliceSource * max(len(entries), 1))(*[SliceSource(*e) for e in entries])
    pack, layout, err = np.zeros(4096, np.uint8), (C.c_uint64 * 4)(), C.create_string_buffer(512)
    ok = host().tg_source_table(b"extract_slices", None if null_slices else arr, len(entries) if n is None else n, d_out, pack.ctypes.data_as(C.c_void_p), pack.size, layout, err,
                                len(err))
    if ok != 1:
        assert ok == 0
        return err.value.decode()
    size, prefix_at, counters_at, total = layout
    assert size == counters_at and pack[:prefix_at].tobytes() == bytes(arr)[:prefix_at]    # the records go up as they are, no counters
    return np.frombuffer(pack[prefix_at:counters_at].tobytes(), "<u4").tolist(), total


def test_extract_slices_table_refusals_and_pack():
    """test_gpu_extract_slices.py's cases: two 8 x 8 rasters"""
    d0, d1, w, h, pitch, AS_IS, RGB, A = 0x1000, 0x2000, 8, 8, 32, 0, 1, 2
    good = [(d0, w, h, pitch, AS_IS, 0), (d1, w, h, pitch, RGB, 4)]
    fn = "extract_slices"
    assert source_table([]) == f"{fn}: no slices (n == 0)"
    assert source_table([good[0], (d1, 0, h, pitch, RGB, 4)]) == f"{fn}: slice 1: zero size (0 x 8)"
    assert source_table([good[0], (d1, w, 0, pitch, RGB, 4)]) == f"{fn}: slice 1: zero size (8 x 0)"
    assert source_table([good[0], (d1, w, h, 28, RGB, 4)]) == f"{fn}: slice 1: row pitch 28 bytes is less than 4 * width = 32"
    assert source_table([good[0], (d1, w, h, pitch, RGB, 3)]) == f"{fn}: slice 1: first_block 3 lies before the end of slice 0's blocks (4): ranges must ascend without overlap"
    assert source_table([(d0, w, h, pitch, AS_IS, 4), (d1, w, h, pitch, RGB, 0)]) == (f"{fn}: slice 1: first_block 0 lies before the end of slice 0's blocks (8): "
                                                                                  "ranges must ascend without overlap")
    assert source_table([good[0], (d1, w, h, pitch, 3, 4)]) == f"{fn}: slice 1: unknown mode 3"
    assert source_table([good[0], (None, w, h, pitch, RGB, 4)]) == f"{fn}: slice 1: null raster"
    assert source_table([good[0], (d1, 2 ** 31, h, 2 ** 32 - 4, RGB, 4)]) == f"{fn}: slice 1: {2 ** 31} x 8 pixels is too large"
    assert source_table(good, d_out=0) == f"{fn}: null pointer" and source_table(good, null_slices=True) == f"{fn}: null pointer"
    assert source_table(good, d_out=OUT + 8) == f"{fn}: the output is not 16-byte aligned"
    big = [(d0, 65536, 65536, 4 * 65536, AS_IS, k * 2 ** 28) for k in range(4)]       # 2^30 tiles: taken
    assert source_table(big)[1] == 2 ** 30
    assert source_table(big + [(d1, 4, 4, 16, AS_IS, 2 ** 30)]) == f"{fn}: more than 2^30 tiles in one call (at slice 4)"
    assert source_table([(d0, 2 ** 30 - 1, 2 ** 31 - 1, 2 ** 32 - 4, AS_IS, 0)]) == f"{fn}: more than 2^30 tiles in one call (at slice 0)"
    assert source_table(good) == ([0, 4, 8], 8)
    # 5 x 7 and 1 x 5 pixels, 17 x 16 tiles, gaps between the ranges
    assert source_table([(d0, 5, 7, 20, AS_IS, 0), (d1, 1, 5, 4, A, 10), (d0, 68, 64, 272, RGB, 12)]) == ([0, 4, 6, 278], 278)


# ---------------------------------------------------------------- the two rasters of a quality metric

@pytest.mark.parametrize("fn", ["image_metrics", "psnr_hvs", "ssim", "ssim_map"])
def test_raster_pair_region(fn):
    def region(d_a, wa, ha, pa, d_b, wb, hb, pb, max_dim=16384):
        out, err = (C.c_uint32 * 4)(), C.create_string_buffer(512)
        ok = host().tg_pair_region(fn.encode(), d_a, wa, ha, pa, d_b, wb, hb, pb, max_dim, out, err, len(err))
        return tuple(out) if ok else err.value.decode()
    a, b = 0x1000, 0x2004
    assert region(a, 17, 16, 0, b, 20, 9, 0) == (17, 20, 17, 9)               # pitches default to the widths; the region is what both have
    assert region(a, 17, 16, 22, b, 20, 9, 20) == (22, 20, 17, 9)
    assert region(a, 0, 16, 0, b, 20, 9, 0) == (0, 20, 0, 9)                  # an empty region is the caller's to refuse
    assert region(a + 2, 8, 8, 0, b, 8, 8, 0) == f"{fn}: a raster is not 4-byte aligned" == region(a, 8, 8, 0, b + 1, 8, 8, 0)
    assert region(a, 8, 8, 7, b, 8, 8, 0) == f"{fn}: row pitch 7 of the first raster is less than its width 8"
    assert region(a, 8, 8, 0, b, 9, 8, 8) == f"{fn}: row pitch 8 of the second raster is less than its width 9"
    assert region(a, 16385, 8, 0, b, 16385, 8, 0) == f"{fn}: a region of 16385 x 8 pixels is too large (16384 each way at the most)"
    assert region(a, 8, 16385, 0, b, 8, 20000, 0) == f"{fn}: a region of 8 x 16385 pixels is too large (16384 each way at the most)"
    assert region(a, 16385, 8, 0, b, 16384, 8, 0) == (16385, 16384, 16384, 8)
    assert region(a, 70000, 8, 0, b, 70000, 8, 0, max_dim=2 ** 32 - 1) == (70000, 70000, 70000, 8)     # SSIM's call: its size limit is its own sentence
