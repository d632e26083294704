"""-m gpu: the block unpacker (csrc/block_unpack_kernels.hip through bu_hip_k_unpack_blocks and basis_universal_amd.transcode.unpack_blocks) against the host build of
the same core and the reference's known answers (tests/golden/block_unpack_vectors.npz), its raster geometry against a guard pattern, the resident transcode ->
unpack chain, its refusals, and the BC7 half of the quality stats against what the reference tool printed (tests/golden/bc7_stats_vectors.npz)."""
import ctypes as C

import numpy as np
import pytest

import block_unpack_helpers as B
import image_metrics_helpers as M
import psnr_hvs_helpers as P
from basis_universal_amd import mipmap, stats
from basis_universal_amd import transcode as T
from basis_universal_amd.compress import compress

pytestmark = pytest.mark.gpu
FORMATS = [B.BC1, B.BC3, B.BC4, B.BC5, B.BC7]
GUARD = 0xA5


@pytest.mark.parametrize("fmt", FORMATS, ids=[B.NAMES[f] for f in FORMATS])
def test_kernel_equals_host_core_equals_reference_block_for_block(hip_ctx, fmt):
    """Every golden block of the format as one row of blocks: the widest ragged-free texture for the 4-blocks-per-wave mapping, and several hundred workgroups."""
    blocks, want, want_ok = B.format_set(fmt)
    n = blocks.shape[0]
    host, host_ok = B.host_unpack(blocks, fmt)
    refused = want_ok == 0
    assert (host_ok == want_ok).all() and (host[~refused] == want[~refused]).all() and (host[refused] == 0).all()
    if refused.any():
        with pytest.raises(T.InvalidBlocksError) as e:
            T.unpack_blocks(hip_ctx, blocks, n, 1, fmt)
        assert e.value.count == int(refused.sum()) == 16
        # the raster itself, through a caller-owned buffer: the refused blocks zero-filled, their valid neighbours what they are without them
        d_blk, d_out, invalid = hip_ctx.upload(blocks), hip_ctx.upload(np.full((4, n * 4, 4), GUARD, np.uint8)), C.c_uint32(0)
        try:
            assert hip_ctx.lib.k_unpack_blocks(hip_ctx.h, C.c_void_p(d_blk), n, 1, 0, 0, fmt, C.c_void_p(d_out), 0, 0, C.byref(invalid)) == 1
            got = hip_ctx.download(d_out, (4, n * 4, 4), np.uint8)
        finally:
            hip_ctx.free(d_blk)
            hip_ctx.free(d_out)
        assert invalid.value == 16
    else:
        got = T.unpack_blocks(hip_ctx, blocks, n, 1, fmt)
    assert got.shape == (4, n * 4, 4)
    tiles = got.reshape(4, n, 4, 4).transpose(1, 0, 2, 3).reshape(n, 16, 4)
    bad = np.flatnonzero((tiles != host).any(axis=(1, 2)))
    assert bad.size == 0, f"{B.NAMES[fmt]}: {bad.size} of {n} blocks differ from the host core; first: block {bad[0]} {blocks[bad[0]].tobytes().hex()}"
    assert (tiles[refused] == 0).all()
    near = np.flatnonzero(refused)
    for k in (near - 1, near + 1):
        k = k[(k >= 0) & (k < n)]
        k = k[~refused[k]]
        assert (tiles[k] == want[k]).all()


GEOMETRY = [(1, 1), (5, 7), (20, 28), (268, 12)]   # 1 block; 2x2 ragged both ways; 35 blocks, no multiple of the 4 per wave; 201 blocks, more than one workgroup of 16


@pytest.mark.parametrize("fmt", [B.BC7, B.BC4], ids=["bc7", "bc4"])
@pytest.mark.parametrize("w,h", GEOMETRY)
def test_only_the_image_is_written(hip_ctx, fmt, w, h):
    """pitch = width, pitch = width + 3, rows < height, and a raster that starts 4 bytes into a 16-byte line: every byte outside width x height (rows) keeps the guard"""
    nbx, nby = (w + 3) // 4, (h + 3) // 4
    blocks, _, ok = B.format_set(fmt)
    blocks = blocks[ok != 0][:nbx * nby]
    assert blocks.shape[0] == nbx * nby
    want = B.to_raster(B.host_unpack(blocks, fmt)[0], nbx, nby, w, h)
    assert (T.unpack_blocks(hip_ctx, blocks, nbx, nby, fmt, width=w, height=h) == want).all()
    d_blk = hip_ctx.upload(blocks)
    try:
        for pitch, rows, lead in ((w, h, 0), (w + 3, h, 0), (w + 3, max(h - 2, 1), 0), (w + 1, h, 1), (w, h, 3)):
            total = lead + rows * pitch + 5   # pixels: `lead` before the raster, 5 after it
            fill = np.full((total, 4), GUARD, np.uint8)
            d_buf = hip_ctx.upload(fill)
            try:
                assert T.unpack_blocks(hip_ctx, d_blk, nbx, nby, fmt, width=w, height=h, out_device=d_buf + 4 * lead, out_row_pitch=pitch, out_rows=rows) is None
                out = hip_ctx.download(d_buf, (total, 4), np.uint8)
            finally:
                hip_ctx.free(d_buf)
            what = (B.NAMES[fmt], w, h, pitch, rows, lead)
            assert (out[:lead] == GUARD).all() and (out[lead + rows * pitch:] == GUARD).all(), what
            raster = out[lead:lead + rows * pitch].reshape(rows, pitch, 4)
            assert (raster[:min(rows, h), :w] == want[:rows]).all(), what
            assert (raster[:, w:] == GUARD).all() and (raster[h:] == GUARD).all(), what
            assert hip_ctx.lib.unpack_output_bytes(nbx, nby, w, h, pitch, rows) == rows * pitch * 4
    finally:
        hip_ctx.free(d_blk)


RESIDENT = [("level2_bc7", T.BC7_RGBA, {}), ("level2_bc1", T.BC1_RGB, {}), ("level2_bc1_hq", T.BC1_RGB, {"high_quality": True}), ("level2_bc3", T.BC3_RGBA, {}),
            ("level2_bc4_r", T.BC4_R, {}), ("level2_bc5_ra", T.BC5_RG, {})]


def test_resident_transcode_then_unpack(hip_ctx):
    """UASTC blocks go up once; device transcode to each block format and device unpack of its output, nothing downloaded in between: the host unpack of the
    reference's own transcoded blocks."""
    z = np.load(B.ROOT / "tests" / "golden" / "uastc_transcode_vectors.npz")
    uastc = z["level2_blocks"]
    n = uastc.shape[0]
    nbx, nby = 64, n // 64
    assert nbx * nby == n
    d_uastc, d_mid, d_out = hip_ctx.upload(uastc), hip_ctx.alloc(n * 16), hip_ctx.alloc(n * 64)
    try:
        for name, target, options in RESIDENT:
            assert T.transcode_uastc_blocks(hip_ctx, d_uastc, nbx, nby, target, out_device=d_mid, **options) is None
            assert T.unpack_blocks(hip_ctx, d_mid, nbx, nby, target, out_device=d_out) is None
            got = hip_ctx.download(d_out, (nby * 4, nbx * 4, 4), np.uint8)
            texels, ok = B.host_unpack(z[name], target)
            assert ok.all() and (got == B.to_raster(texels, nbx, nby, nbx * 4, nby * 4)).all(), name
    finally:
        for d in (d_uastc, d_mid, d_out):
            hip_ctx.free(d)


def _unpack(ctx, d_blk, nbx, nby, w, h, fmt, d_out, pitch=0, rows=0):
    invalid = C.c_uint32(77)
    r = ctx.lib.k_unpack_blocks(ctx.h, C.c_void_p(d_blk), nbx, nby, w, h, fmt, C.c_void_p(d_out), pitch, rows, C.byref(invalid))
    return r, invalid.value


@pytest.mark.parametrize("fmt,name", [(0, "ETC1_RGB"), (1, "ETC2_RGBA"), (10, "ASTC_4x4_RGBA"), (13, "RGBA32"), (99, "unknown")])
def test_other_formats_are_refused_by_name(hip_ctx, fmt, name):
    fill = np.full((8, 8, 4), GUARD, np.uint8)
    d_blk, d_out = hip_ctx.upload(np.zeros((4, 16), np.uint8)), hip_ctx.upload(fill)
    try:
        assert _unpack(hip_ctx, d_blk, 2, 2, 0, 0, fmt, d_out) == (0, 0)
        err = hip_ctx.lib.last_error(hip_ctx.h)
        assert "not supported" in err and name in err and str(fmt) in err
        assert (hip_ctx.download(d_out, fill.shape, np.uint8) == fill).all()
    finally:
        hip_ctx.free(d_blk)
        hip_ctx.free(d_out)
    with pytest.raises(ValueError, match=f"{name}.*does not unpack"):
        T.unpack_blocks(hip_ctx, np.zeros((4, 16), np.uint8), 2, 2, fmt)
    assert hip_ctx.lib.unpack_output_bytes(2, 2, 0, 0, 0, 0) == 8 * 8 * 4   # the raster's size does not depend on the format


def test_bad_arguments_are_refused(hip_ctx):
    blocks, _, ok = B.format_set(B.BC7)
    blocks = blocks[ok != 0][:4]
    fill = np.full((8, 8, 4), GUARD, np.uint8)
    d_blk, d_out = hip_ctx.upload(blocks), hip_ctx.upload(fill)
    try:
        for args, text in (((0, 2, 2, 0, 0, B.BC7, d_out), "null"), ((d_blk, 2, 2, 0, 0, B.BC7, 0), "null"),
                           ((d_blk, 2, 2, 8, 8, B.BC7, d_out, 7), "row pitch 7 is less than the width 8"),
                           ((d_blk, 2, 2, 9, 8, B.BC7, d_out), "9 x 8 pixels do not fit 2 x 2 blocks"), ((d_blk, 2, 2, 8, 9, B.BC7, d_out), "do not fit"),
                           ((d_blk, 16385, 1, 0, 0, B.BC7, d_out), "too many"), ((d_blk + 8, 1, 1, 0, 0, B.BC7, d_out), "aligned"), ((d_blk, 1, 1, 0, 0, B.BC7, d_out + 2), "aligned")):
            assert _unpack(hip_ctx, *args) == (0, 0), args
            assert text in hip_ctx.lib.last_error(hip_ctx.h), (args, hip_ctx.lib.last_error(hip_ctx.h))
        assert hip_ctx.lib.k_unpack_blocks(None, C.c_void_p(d_blk), 2, 2, 0, 0, B.BC7, C.c_void_p(d_out), 0, 0, None) == 0
        assert (hip_ctx.download(d_out, fill.shape, np.uint8) == fill).all(), "a refused call wrote something"
        assert _unpack(hip_ctx, d_blk, 2, 2, 0, 0, B.BC7, d_out) == (1, 0)     # and the same buffers are fine when the arguments are
        assert hip_ctx.lib.k_unpack_blocks(hip_ctx.h, C.c_void_p(d_blk), 2, 2, 0, 0, B.BC7, C.c_void_p(d_out), 0, 0, None) == 1   # the count is optional
        assert (hip_ctx.download(d_out, fill.shape, np.uint8) == B.to_raster(B.host_unpack(blocks, B.BC7)[0], 2, 2, 8, 8)).all()
        assert hip_ctx.lib.unpack_output_bytes(2, 2, 0, 0, 0, 0) == 256 and hip_ctx.lib.unpack_output_bytes(2, 2, 5, 7, 0, 0) == 5 * 7 * 4
        assert hip_ctx.lib.unpack_output_bytes(2, 2, 5, 7, 9, 3) == 9 * 3 * 4
    finally:
        hip_ctx.free(d_blk)
        hip_ctx.free(d_out)
    for kw, text in (({"width": 9}, "do not fit"), ({"out_row_pitch": 8}, "give out_device")):
        with pytest.raises(ValueError, match=text):
            T.unpack_blocks(hip_ctx, blocks, 2, 2, B.BC7, **kw)
    with pytest.raises(ValueError, match="need 64 bytes"):
        T.unpack_blocks(hip_ctx, blocks[:3], 2, 2, B.BC7)


def test_invalid_blocks_error_carries_the_count(hip_ctx):
    blocks, _, ok = B.format_set(B.BC7)
    blocks = np.array(blocks[ok != 0][:35])
    blocks[[0, 17, 34], 0] = 0
    with pytest.raises(T.InvalidBlocksError, match="3 of 35 blocks are not valid BC7") as e:
        T.unpack_blocks(hip_ctx, blocks, 5, 7, B.BC7, width=20, height=28)
    assert e.value.count == 3 and isinstance(e.value, ValueError)


# ---------------------------------------------------------------- the BC7 half of the quality stats

def stats_cases():
    return B.golden_stats()[1]["cases"]


def _case_data(case):
    arrays, _ = B.golden_stats()
    holder = M.golden()[0] if case["in_image_stats_vectors"] else arrays
    return holder["file_" + case["name"]], np.array(holder["src_" + case["name"]])


@pytest.fixture(scope="module")
def mip_sources(hip_ctx):
    """the source of every level of the 20x28 mip case, made on the device as compress() makes them"""
    src = np.array(B.golden_stats()[0]["src_uastc_mip_basis"])
    return [src] + mipmap.generate_mipmaps(hip_ctx, src, has_alpha=False)


def without_bc7(slices):
    return [{k: v for k, v in s.items() if k != "bc7"} for s in slices]


@pytest.mark.parametrize("case", stats_cases(), ids=[c["name"] for c in stats_cases()])
def test_file_stats_bc7_match_what_the_reference_tool_printed(hip_ctx, case, mip_sources):
    arrays, _ = B.golden_stats()
    data, src = _case_data(case)
    sources = mip_sources if "-mipmap" in case["args"] else [src]
    printed, printed_hvs = arrays["stats_" + case["name"]], arrays["hvs_" + case["name"]]
    got = stats.file_stats(hip_ctx, data, sources, hvs=True, bc7=True)
    assert len(got) == case["slices"] == printed.shape[0] == printed_hvs.shape[0]
    for k, s in enumerate(got):
        M.assert_close_to_printed(s["bc7"], printed[k], f"{case['name']} slice {k} (BC7)")
        P.assert_close_to_printed(s["bc7"]["hvs"], printed_hvs[k], f"{case['name']} slice {k} (BC7 HVS)")
        assert (s["bc7"]["width"], s["bc7"]["height"]) == (s["width"], s["height"]) and "bc7" not in s["bc7"]
    # the flag off: today's dicts, with and without naming it; and without hvs the BC7 dict has none either
    plain = stats.file_stats(hip_ctx, data, sources, hvs=True)
    assert plain == stats.file_stats(hip_ctx, data, sources, hvs=True, bc7=False) == without_bc7(got) and all("bc7" not in s for s in plain)
    no_hvs = stats.file_stats(hip_ctx, data, sources, bc7=True)
    assert all("hvs" not in s and "hvs" not in s["bc7"] for s in no_hvs)
    assert [{k: v for k, v in s["bc7"].items() if k != "hvs"} for s in got] == [s["bc7"] for s in no_hvs]


def test_compress_fills_bc7_stats(hip_ctx):
    src = np.array(M.golden()[0]["src_uastc_alpha_ktx2"])
    assert src.shape == (24, 32, 4)
    filled, plain = [], []
    data = compress(hip_ctx, src, uastc=True, ktx2=True, stats=filled, stats_bc7=True)
    assert compress(hip_ctx, src, uastc=True, ktx2=True, stats=plain).tobytes() == data.tobytes() == compress(hip_ctx, src, uastc=True, ktx2=True, stats_bc7=True).tobytes()
    assert filled == stats.file_stats(hip_ctx, data, [src], bc7=True) and plain == without_bc7(filled)
    M.assert_close_to_printed(filled[0]["bc7"], B.golden_stats()[0]["stats_uastc_alpha_ktx2"][0], "compress (BC7)")


def test_etc1s_refuses_the_bc7_flag(hip_ctx):
    arrays, _ = M.golden()
    src = np.array(arrays["src_etc1s_o20_basis"])
    with pytest.raises(ValueError, match="the ETC1S transcoder here has no BC7 target"):
        stats.file_stats(hip_ctx, arrays["file_etc1s_o20_basis"], [src], bc7=True)
    filled = []
    with pytest.raises(ValueError, match="the ETC1S transcoder here has no BC7 target"):
        compress(hip_ctx, src, quality=128, stats=filled, stats_bc7=True)
    assert filled == []
