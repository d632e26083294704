"""-m gpu: the texture unpacker (csrc/texture_unpack_kernels.hip through bu_hip_k_unpack_texture and basis_universal_amd.transcode.unpack_texture) against the host
build of the same core and the reference's known answers (tests/golden/texture_unpack_vectors.npz), the five BC formats against bu_hip_k_unpack_blocks, its raster
geometry against a guard pattern, PVRTC1's Morton order and wrapped neighbours at the smallest sizes, the resident transcode -> unpack chains, and its refusals."""
import ctypes as C

import numpy as np
import pytest

import block_unpack_helpers as B
import texture_unpack_helpers as X
from basis_universal_amd import transcode as T

pytestmark = pytest.mark.gpu
GUARD = 0xA5
NAMES = {X.ETC1: "etc1", X.ETC2: "etc2", X.R11: "r11", X.RG11: "rg11", X.ASTC: "astc", X.PVRTC1_RGB: "pvrtc1_rgb", X.PVRTC1_RGBA: "pvrtc1_rgba", **B.NAMES}


def _call(ctx, d_blk, nbx, nby, w, h, fmt, d_out, pitch=0, rows=0):
    invalid = C.c_uint32(77)
    r = ctx.lib.k_unpack_texture(ctx.h, C.c_void_p(d_blk), nbx, nby, w, h, fmt, C.c_void_p(d_out), pitch, rows, C.byref(invalid))
    return r, invalid.value


def _raster(ctx, blocks, nbx, nby, fmt, w=None, h=None):
    """through the C entry into a caller-owned, guard-filled buffer -> (raster (h, w, 4), invalid count)"""
    w, h = w or nbx * 4, h or nby * 4
    d_blk, d_out = ctx.upload(np.ascontiguousarray(blocks)), ctx.upload(np.full((h, w, 4), GUARD, np.uint8))
    try:
        r, invalid = _call(ctx, d_blk, nbx, nby, w, h, fmt, d_out)
        assert r == 1, ctx.lib.last_error(ctx.h)
        return ctx.download(d_out, (h, w, 4), np.uint8), invalid
    finally:
        ctx.free(d_blk)
        ctx.free(d_out)


def _tiles(raster, nbx, nby):
    return raster.reshape(nby, 4, nbx, 4, 4).transpose(0, 2, 1, 3, 4).reshape(nbx * nby, 16, 4)


@pytest.mark.parametrize("name", sorted(X.BLOCK_MEMBERS))
def test_kernel_equals_host_core_equals_reference_on_every_member(hip_ctx, name):
    """Every block of the member as one row of blocks (several workgroups, a count that is no multiple of the 16 per workgroup where the member has one): texel for
    texel the host core, which is the reference wherever it accepts; refused blocks zero, alpha included, and counted."""
    arrays, _ = X.golden()
    fmt = X.BLOCK_MEMBERS[name]
    blocks, want, want_ok = arrays[name + "_blocks"], arrays[name + "_texels"], arrays[name + "_ok"]
    n, refused = blocks.shape[0], want_ok == 0
    host, host_ok = X.host_unpack(blocks, fmt)
    assert (host_ok == want_ok).all() and (host[~refused] == want[~refused]).all()
    got, invalid = _raster(hip_ctx, blocks, n, 1, fmt)
    tiles = _tiles(got, n, 1)
    assert invalid == int(refused.sum())
    bad = np.flatnonzero((tiles != host).any(axis=(1, 2)))
    assert bad.size == 0, f"{name}: {bad.size} of {n} blocks differ from the host core; first: block {bad[0]} {blocks[bad[0]].tobytes().hex()}"
    assert (tiles[refused] == 0).all() and (tiles[~refused] == want[~refused]).all()
    if refused.any():
        with pytest.raises(T.InvalidBlocksError) as e:
            T.unpack_texture(hip_ctx, blocks, n, 1, fmt)
        assert e.value.count == int(refused.sum())
    else:
        assert (T.unpack_texture(hip_ctx, blocks, n, 1, fmt) == got).all()


@pytest.mark.parametrize("fmt", X.BC_FORMATS, ids=[B.NAMES[f] for f in X.BC_FORMATS])
def test_bc_formats_equal_the_block_unpacker(hip_ctx, fmt):
    """the five existing formats through the new entry: the raster and the count bu_hip_k_unpack_blocks gives for the same resident blocks, BC7's refusals included"""
    blocks, _, ok = B.format_set(fmt)
    n = blocks.shape[0]
    d_blk, d_a, d_b = hip_ctx.upload(blocks), hip_ctx.upload(np.full((4, n * 4, 4), GUARD, np.uint8)), hip_ctx.upload(np.full((4, n * 4, 4), GUARD, np.uint8))
    try:
        old = C.c_uint32(0)
        assert hip_ctx.lib.k_unpack_blocks(hip_ctx.h, C.c_void_p(d_blk), n, 1, 0, 0, fmt, C.c_void_p(d_a), 0, 0, C.byref(old)) == 1
        assert _call(hip_ctx, d_blk, n, 1, 0, 0, fmt, d_b) == (1, old.value) and old.value == int((ok == 0).sum())
        assert (hip_ctx.download(d_a, (4, n * 4, 4), np.uint8) == hip_ctx.download(d_b, (4, n * 4, 4), np.uint8)).all()
    finally:
        for d in (d_blk, d_a, d_b):
            hip_ctx.free(d)
    assert hip_ctx.lib.unpack_texture_bytes_per_block(fmt) == B.BYTES[fmt]


def _accepted(fmt, count):
    arrays, _ = X.golden()
    name = {X.ETC1: "etc1", X.ETC2: "etc2", X.R11: "r11", X.RG11: "rg11", X.ASTC: "astc"}[fmt]
    blocks = arrays[name + "_blocks"][arrays[name + "_ok"] != 0]
    reps = -(-count // blocks.shape[0])
    return np.ascontiguousarray(np.concatenate([blocks] * reps)[:count])


GEOMETRY = [(1, 1), (5, 7), (22, 27), (269, 14)]   # 1 block, one texel of it; 4n + 1 x 4n + 3; 4n + 2 x 4n + 3, 42 blocks; 4n + 1 x 4n + 2, 272 blocks: 17 workgroups


@pytest.mark.parametrize("fmt", [X.ASTC, X.ETC2, X.R11, X.ETC1, X.RG11], ids=["astc", "etc2", "r11", "etc1", "rg11"])
@pytest.mark.parametrize("w,h", GEOMETRY)
def test_only_the_image_is_written(hip_ctx, fmt, w, h):
    """pitch = width, pitch = width + 3, rows < height, and a raster that starts 4 bytes into a 16-byte line: every byte outside width x height (rows) keeps the guard"""
    nbx, nby = (w + 3) // 4, (h + 3) // 4
    blocks = _accepted(fmt, nbx * nby)
    want = X.to_raster(X.host_unpack(blocks, fmt)[0], nbx, nby, w, h)
    assert (T.unpack_texture(hip_ctx, blocks, nbx, nby, fmt, width=w, height=h) == want).all()
    d_blk = hip_ctx.upload(blocks)
    try:
        for pitch, rows, lead in ((w, h, 0), (w + 3, h, 0), (w + 3, max(h - 2, 1), 0), (w + 1, h, 1), (w, h, 3)):
            total = lead + rows * pitch + 5   # pixels: `lead` before the raster, 5 after it
            d_buf = hip_ctx.upload(np.full((total, 4), GUARD, np.uint8))
            try:
                assert T.unpack_texture(hip_ctx, d_blk, nbx, nby, fmt, width=w, height=h, out_device=d_buf + 4 * lead, out_row_pitch=pitch, out_rows=rows) is None
                out = hip_ctx.download(d_buf, (total, 4), np.uint8)
            finally:
                hip_ctx.free(d_buf)
            what = (NAMES[fmt], w, h, pitch, rows, lead)
            assert (out[:lead] == GUARD).all() and (out[lead + rows * pitch:] == GUARD).all(), what
            raster = out[lead:lead + rows * pitch].reshape(rows, pitch, 4)
            assert (raster[:min(rows, h), :w] == want[:rows]).all(), what
            assert (raster[:, w:] == GUARD).all() and (raster[h:] == GUARD).all(), what
    finally:
        hip_ctx.free(d_blk)


# ---------------------------------------------------------------- PVRTC1

@pytest.mark.parametrize("nbx,nby", X.PVRTC1_RANDOM)
@pytest.mark.parametrize("fmt", [X.PVRTC1_RGB, X.PVRTC1_RGBA], ids=["rgb", "rgba"])
def test_pvrtc1_smallest_images_of_both_modulation_modes(hip_ctx, nbx, nby, fmt):
    """1x1 (the block that is its own neighbour all round), 2x1, 1x2, 2x2 and 8x2 blocks (non-square Morton order) of random bits: the fixture's raster, which is
    the restatement's, and the host core's; the two format values decode alike"""
    arrays, _ = X.golden()
    blocks, want = arrays[f"pvrtc1_random_{nbx}x{nby}_blocks"], arrays[f"pvrtc1_random_{nbx}x{nby}_texels"]
    got, invalid = _raster(hip_ctx, blocks, nbx, nby, fmt)
    assert invalid == 0 and (got == want).all() and (got == X.host_unpack_pvrtc1(blocks, nbx, nby)).all()
    assert (T.unpack_texture(hip_ctx, blocks, nbx, nby, fmt) == want).all()


def test_pvrtc1_equals_every_raster_the_reference_tool_wrote(hip_ctx):
    """alpha and opaque 32x32, the 64x16 and 16x64 chains down to 1x1 pixels (a cropped single block), both 64x64 coverage files, of both codecs and both targets"""
    arrays, meta = X.golden()
    pv, _ = X.golden_pvrtc1()
    assert len(meta["pvrtc1_images"]) >= 36
    for key, short, w, h, channels in meta["pvrtc1_images"]:
        nbx, nby = (w + 3) // 4, (h + 3) // 4
        got = T.unpack_texture(hip_ctx, pv[f"{key}_{short}"], nbx, nby, X.PVRTC1_TARGETS[short], width=w, height=h)
        assert got.shape == (h, w, 4) and (got[..., :channels] == arrays[f"pvrtc1_{key}_{short}_texels"]).all(), (key, short)


def test_pvrtc1_only_the_image_is_written(hip_ctx):
    arrays, _ = X.golden()
    blocks = arrays["pvrtc1_random_8x2_blocks"]
    want = arrays["pvrtc1_random_8x2_texels"]
    d_blk = hip_ctx.upload(blocks)
    try:
        for w, h, pitch, rows, lead in ((32, 8, 35, 8, 0), (32, 8, 33, 5, 1), (32, 4, 32, 4, 3), (16, 8, 19, 8, 0)):
            total = lead + rows * pitch + 5
            d_buf = hip_ctx.upload(np.full((total, 4), GUARD, np.uint8))
            try:
                assert T.unpack_texture(hip_ctx, d_blk, 8, 2, X.PVRTC1_RGBA, width=w, height=h, out_device=d_buf + 4 * lead, out_row_pitch=pitch, out_rows=rows) is None
                out = hip_ctx.download(d_buf, (total, 4), np.uint8)
            finally:
                hip_ctx.free(d_buf)
            assert (out[:lead] == GUARD).all() and (out[lead + rows * pitch:] == GUARD).all(), (w, h, pitch, rows)
            raster = out[lead:lead + rows * pitch].reshape(rows, pitch, 4)
            assert (raster[:min(rows, h), :w] == want[:min(rows, h), :w]).all() and (raster[:, w:] == GUARD).all() and (raster[h:] == GUARD).all(), (w, h, pitch, rows)
    finally:
        hip_ctx.free(d_blk)


# ---------------------------------------------------------------- resident chains

def _uastc_grid(nby):
    z = np.load(X.ROOT / "tests" / "golden" / "uastc_transcode_vectors.npz")
    return np.ascontiguousarray(z["level2_blocks"][:64 * nby]), 64, nby


def test_resident_uastc_transcode_then_unpack(hip_ctx):
    """UASTC blocks go up once; device transcode to ETC1 / ETC2 RGBA / RG11 / ASTC and device unpack of that pointer, nothing downloaded in between: the host
    unpack of the blocks downloaded afterwards"""
    uastc, nbx, nby = _uastc_grid(23)
    n = nbx * nby
    d_uastc, d_mid, d_out = hip_ctx.upload(uastc), hip_ctx.alloc(n * 16), hip_ctx.alloc(n * 64)
    try:
        for target in (T.ETC1_RGB, T.ETC2_RGBA, T.ETC2_EAC_RG11, T.ASTC_4x4_RGBA):
            assert T.transcode_uastc_texture_blocks(hip_ctx, d_uastc, nbx, nby, target, out_device=d_mid) is None
            assert T.unpack_texture(hip_ctx, d_mid, nbx, nby, target, out_device=d_out) is None
            got = hip_ctx.download(d_out, (nby * 4, nbx * 4, 4), np.uint8)
            texels, ok = X.host_unpack(hip_ctx.download(d_mid, (n, T.UNPACK_TEXTURE_BYTES_PER_BLOCK[target]), np.uint8), target)
            assert ok.all() and (got == X.to_raster(texels, nbx, nby, nbx * 4, nby * 4)).all(), target
    finally:
        for d in (d_uastc, d_mid, d_out):
            hip_ctx.free(d)


@pytest.mark.parametrize("target", [T.PVRTC1_4_RGB, T.PVRTC1_4_RGBA], ids=["rgb", "rgba"])
def test_resident_uastc_pvrtc1_transcode_then_unpack(hip_ctx, target):
    uastc, nbx, nby = _uastc_grid(16)
    n = nbx * nby
    d_uastc, d_mid, d_out = hip_ctx.upload(uastc), hip_ctx.alloc(n * 8), hip_ctx.alloc(n * 64)
    try:
        assert T.transcode_uastc_pvrtc1_blocks(hip_ctx, d_uastc, nbx, nby, target, out_device=d_mid) is None
        assert T.unpack_texture(hip_ctx, d_mid, nbx, nby, target, out_device=d_out) is None
        got = hip_ctx.download(d_out, (nby * 4, nbx * 4, 4), np.uint8)
        assert (got == X.host_unpack_pvrtc1(hip_ctx.download(d_mid, (n, 8), np.uint8), nbx, nby)).all()
        if target == T.PVRTC1_4_RGB:
            assert (got[..., 3] == 255).all()
    finally:
        for d in (d_uastc, d_mid, d_out):
            hip_ctx.free(d)


def test_uastc_made_astc_unpacks_to_the_rgba32_transcode(hip_ctx):
    """asserted because, and only because, the fixture's meta records that the reference's own unpack of these ASTC blocks equals its RGBA32 transcode"""
    _, meta = X.golden()
    if not meta["uastc_astc_unpack_equals_rgba32"]:
        return
    uastc, nbx, nby = _uastc_grid(23)
    n = nbx * nby
    d_uastc, d_mid = hip_ctx.upload(uastc), hip_ctx.alloc(n * 16)
    try:
        assert T.transcode_uastc_texture_blocks(hip_ctx, d_uastc, nbx, nby, T.ASTC_4x4_RGBA, out_device=d_mid) is None
        assert (T.unpack_texture(hip_ctx, d_mid, nbx, nby, T.ASTC_4x4_RGBA) == T.transcode_uastc_blocks(hip_ctx, d_uastc, nbx, nby, T.RGBA32)).all()
    finally:
        hip_ctx.free(d_uastc)
        hip_ctx.free(d_mid)


@pytest.mark.parametrize("name,level", [("opaque_basis", 0), ("mip_ktx2", 0), ("mip_ktx2", 1), ("mip_ktx2", 3), ("alpha_basis", 0)])
def test_etc1s_file_as_etc1_unpacks_to_the_rgb_of_its_rgba32_transcode(hip_ctx, name, level):
    """ETC1S is an ETC1 subset, so this needs no reference: the file's ETC1 transcode, unpacked, is the colour of its RGBA32 transcode, ragged levels cropped"""
    data = np.load(X.ROOT / "tests" / "golden" / "etc1s_block_format_vectors.npz")["file_" + name]
    im = next(i for i in T.read_etc1s_file(data)["images"] if i["level"] == level and i["layer"] == 0 and i["face"] == 0)
    etc1 = T.transcode_etc1s_file(hip_ctx, data, T.ETC1_RGB, level=level)
    rgba = T.transcode_etc1s_file(hip_ctx, data, T.RGBA32, level=level)
    got = T.unpack_texture(hip_ctx, etc1, im["num_blocks_x"], im["num_blocks_y"], T.ETC1_RGB, width=im["width"], height=im["height"])
    assert got.shape == rgba.shape == (im["height"], im["width"], 4)
    assert (got[..., :3] == rgba[..., :3]).all() and (got[..., 3] == 255).all()


# ---------------------------------------------------------------- refusals

@pytest.mark.parametrize("fmt,name", [(13, "RGBA32"), (11, "ATC_RGB"), (12, "ATC_RGBA"), (99, "unknown")])
def test_other_formats_are_refused_by_name(hip_ctx, fmt, name):
    fill = np.full((8, 8, 4), GUARD, np.uint8)
    d_blk, d_out = hip_ctx.upload(np.zeros((4, 16), np.uint8)), hip_ctx.upload(fill)
    try:
        assert _call(hip_ctx, d_blk, 2, 2, 0, 0, fmt, d_out) == (0, 0)
        err = hip_ctx.lib.last_error(hip_ctx.h)
        assert "not supported" in err and name in err and str(fmt) in err and "ASTC_4x4_RGBA (10)" in err and "PVRTC1_4_RGB (8)" in err
        assert (hip_ctx.download(d_out, fill.shape, np.uint8) == fill).all()
    finally:
        hip_ctx.free(d_blk)
        hip_ctx.free(d_out)
    with pytest.raises(ValueError, match=f"{name}.*does not unpack"):
        T.unpack_texture(hip_ctx, np.zeros((4, 16), np.uint8), 2, 2, fmt)
    assert hip_ctx.lib.unpack_texture_bytes_per_block(fmt) == 0


def test_bytes_per_block_of_every_format(hip_ctx):
    assert T.UNPACK_TEXTURE_BYTES_PER_BLOCK == X.BYTES
    for fmt, unit in X.BYTES.items():
        assert hip_ctx.lib.unpack_texture_bytes_per_block(fmt) == unit


def test_bad_arguments_are_refused(hip_ctx):
    blocks = _accepted(X.ASTC, 4)
    fill = np.full((8, 8, 4), GUARD, np.uint8)
    d_blk, d_out = hip_ctx.upload(blocks), hip_ctx.upload(fill)
    try:
        for args, text in (((0, 2, 2, 0, 0, X.ASTC, d_out), "null"), ((d_blk, 2, 2, 0, 0, X.ASTC, 0), "null"),
                           ((d_blk, 2, 2, 8, 8, X.ASTC, d_out, 7), "row pitch 7 is less than the width 8"),
                           ((d_blk, 2, 2, 9, 8, X.ASTC, d_out), "9 x 8 pixels do not fit 2 x 2 blocks"), ((d_blk, 16385, 1, 0, 0, X.ASTC, d_out), "too many"),
                           ((d_blk + 8, 1, 1, 0, 0, X.ASTC, d_out), "16-byte aligned"), ((d_blk + 4, 1, 1, 0, 0, X.ETC1, d_out), "8-byte aligned"),
                           ((d_blk + 4, 1, 1, 0, 0, X.PVRTC1_RGB, d_out), "8-byte aligned"), ((d_blk, 1, 1, 0, 0, X.R11, d_out + 2), "aligned"),
                           ((d_blk, 3, 1, 0, 0, X.PVRTC1_RGB, d_out), "PVRTC1 only supports power of 2 dimensions"),
                           ((d_blk, 2, 2, 8, 6, X.PVRTC1_RGBA, d_out), "PVRTC1 only supports power of 2 dimensions"),
                           ((d_blk, 2, 2, 7, 8, X.PVRTC1_RGBA, d_out), "PVRTC1 only supports power of 2 dimensions")):
            assert _call(hip_ctx, *args) == (0, 0), args
            assert text in hip_ctx.lib.last_error(hip_ctx.h), (args, hip_ctx.lib.last_error(hip_ctx.h))
        assert hip_ctx.lib.k_unpack_texture(None, C.c_void_p(d_blk), 2, 2, 0, 0, X.ASTC, C.c_void_p(d_out), 0, 0, None) == 0
        assert (hip_ctx.download(d_out, fill.shape, np.uint8) == fill).all(), "a refused call wrote something"
        assert _call(hip_ctx, d_blk, 2, 2, 0, 0, X.ASTC, d_out) == (1, 0)     # and the same buffers are fine when the arguments are
        assert hip_ctx.lib.k_unpack_texture(hip_ctx.h, C.c_void_p(d_blk), 2, 2, 0, 0, X.ASTC, C.c_void_p(d_out), 0, 0, None) == 1   # the count is optional
        assert (hip_ctx.download(d_out, fill.shape, np.uint8) == X.to_raster(X.host_unpack(blocks, X.ASTC)[0], 2, 2, 8, 8)).all()
    finally:
        hip_ctx.free(d_blk)
        hip_ctx.free(d_out)
    for kw, text in (({"width": 9}, "do not fit"), ({"out_row_pitch": 8}, "give out_device")):
        with pytest.raises(ValueError, match=text):
            T.unpack_texture(hip_ctx, blocks, 2, 2, X.ASTC, **kw)
    with pytest.raises(ValueError, match="need 64 bytes"):
        T.unpack_texture(hip_ctx, blocks[:3], 2, 2, X.ASTC)
    with pytest.raises(ValueError, match="PVRTC1 only supports power of 2 dimensions"):
        T.unpack_texture(hip_ctx, np.zeros((3, 8), np.uint8), 3, 1, X.PVRTC1_RGB)
    with pytest.raises(ValueError, match="PVRTC1 only supports power of 2 dimensions"):
        T.unpack_texture(hip_ctx, np.zeros((4, 8), np.uint8), 2, 2, X.PVRTC1_RGBA, width=6)


def test_the_block_unpacker_keeps_its_refusals(hip_ctx):
    """the old entry is as it was: it still refuses by name what only the new one takes"""
    d_blk, d_out = hip_ctx.upload(np.zeros((4, 16), np.uint8)), hip_ctx.upload(np.zeros((8, 8, 4), np.uint8))
    try:
        for fmt in X.NEW_FORMATS:
            invalid = C.c_uint32(0)
            assert hip_ctx.lib.k_unpack_blocks(hip_ctx.h, C.c_void_p(d_blk), 2, 2, 0, 0, fmt, C.c_void_p(d_out), 0, 0, C.byref(invalid)) == 0
            assert "not supported" in hip_ctx.lib.last_error(hip_ctx.h)
    finally:
        hip_ctx.free(d_blk)
        hip_ctx.free(d_out)
    assert sorted(T.UNPACK_BYTES_PER_BLOCK) == [2, 3, 4, 5, 6]


def test_invalid_blocks_error_carries_the_count(hip_ctx):
    arrays, _ = X.golden()
    blocks = np.array(_accepted(X.ASTC, 35))
    blocks[[0, 17, 34]] = arrays["astc_refused_blocks"][[0, 100, 250]]
    with pytest.raises(T.InvalidBlocksError, match="3 of 35 blocks are not valid ASTC_4x4_RGBA") as e:
        T.unpack_texture(hip_ctx, blocks, 5, 7, X.ASTC, width=20, height=28)
    assert e.value.count == 3 and isinstance(e.value, ValueError)
    etc2 = np.array(_accepted(X.ETC2, 16))
    etc2[5] = arrays["etc2_blocks"][arrays["etc2_ok"] == 0][0]
    with pytest.raises(T.InvalidBlocksError, match="1 of 16 blocks are not valid ETC2_RGBA") as e:
        T.unpack_texture(hip_ctx, etc2, 4, 4, X.ETC2)
    assert e.value.count == 1
