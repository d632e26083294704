"""-m gpu tests of the device-side UASTC LDR 4x4 transcoder (include/basisu_hip.h: bu_hip_k_transcode_uastc; basis_universal_amd/transcode.py) against the reference's
known answers: tests/golden/uastc_transcode_vectors.npz and uastc_transcode_big_digests.json (tools/gen_golden_uastc_transcode.py ran oracle/_ref on the build
machine). Where no golden exists (odd sizes, spliced invalid blocks) the expected values come from the g++ build of the same core, which
tests/test_uastc_transcode_host.py holds to the reference."""
import hashlib
import json
import pathlib

import numpy as np
import pytest

import helpers
import transcode_helpers as T
from basis_universal_amd import transcode, uastc
from basis_universal_amd.compress import compress

pytestmark = pytest.mark.gpu
HERE = pathlib.Path(__file__).resolve().parent
SETS = ("level3", "level2", "default_l2")
CASES = {"rgba32": (transcode.RGBA32, False), "astc": (transcode.ASTC_4x4_RGBA, False), "bc7": (transcode.BC7_RGBA, False), "bc1": (transcode.BC1_RGB, False),
         "bc1_hq": (transcode.BC1_RGB, True), "bc3": (transcode.BC3_RGBA, False), "bc3_hq": (transcode.BC3_RGBA, True), "bc4_r": (transcode.BC4_R, False),
         "bc5_ra": (transcode.BC5_RG, False)}


@pytest.fixture(scope="module")
def golden():
    return np.load(HERE / "golden" / "uastc_transcode_vectors.npz")


def _as_blocks(out, target, nbx, nby):
    """what transcode_uastc_blocks returned, per block (RGBA32: the raster cut back into tiles)"""
    if target != transcode.RGBA32:
        return out
    return out.reshape(nby, 4, nbx, 4, 4).transpose(0, 2, 1, 3, 4).reshape(nbx * nby, 64)


@pytest.mark.parametrize("name", sorted(CASES))
@pytest.mark.parametrize("which", SETS)
def test_device_equals_reference(hip_ctx, golden, which, name):
    target, hq = CASES[name]
    nbx, nby, _n = (int(v) for v in golden[f"{which}_grid"])
    got = _as_blocks(transcode.transcode_uastc_blocks(hip_ctx, golden[f"{which}_blocks"], nbx, nby, target, high_quality=hq), target, nbx, nby)
    exp = golden[f"{which}_{name}"]
    bad = np.flatnonzero((got != exp).any(axis=1))
    assert bad.size == 0, f"{bad.size} of {exp.shape[0]} blocks differ, first {bad[:8].tolist()}"


def test_device_channel_selection(hip_ctx, golden):
    blocks = golden["level3_blocks"]
    nbx, nby, _n = (int(v) for v in golden["level3_grid"])
    for ch in ((1,), (2,), (3,)):
        assert (transcode.transcode_uastc_blocks(hip_ctx, blocks, nbx, nby, transcode.BC4_R, channels=ch) == T.host_transcode(blocks, T.BC4, channels=(ch[0], 3))[0]).all()
    assert (transcode.transcode_uastc_blocks(hip_ctx, blocks, nbx, nby, transcode.BC5_RG, channels=(1, 2)) == T.host_transcode(blocks, T.BC5, channels=(1, 2))[0]).all()


@pytest.mark.parametrize("w,h", [(4, 4), (5, 7), (255, 257), (1845, 894)])
def test_rgba32_raster_is_cropped_and_respects_the_pitch(hip_ctx, w, h):
    nbx, nby = (w + 3) // 4, (h + 3) // 4
    img = helpers.synth(nbx * 4, nby * 4, 99 + w)
    blocks = uastc.encode_uastc_blocks(hip_ctx, helpers.to_pixel_blocks(img), uastc.LEVEL_FASTEST)
    tiles, ok = T.host_transcode(blocks, T.RGBA32)
    assert ok.all()
    exp = T.to_raster(tiles, nbx, nby, w, h)
    got = transcode.transcode_uastc_blocks(hip_ctx, blocks, nbx, nby, transcode.RGBA32, width=w, height=h)
    assert got.shape == (h, w, 4) and (got == exp).all()
    # a caller-owned raster with a padded pitch and spare rows, pre-filled with a sentinel: only the image's pixels change
    for pitch in (w + 3, ((w + 7) // 4) * 4 + 4):
        rows = h + 2
        raster = np.full((rows, pitch, 4), 0xA5, np.uint8)
        d = hip_ctx.upload(raster)
        try:
            assert transcode.transcode_uastc_blocks(hip_ctx, blocks, nbx, nby, transcode.RGBA32, width=w, height=h, out_device=d, out_row_pitch=pitch, out_rows=rows) is None
            back = hip_ctx.download(d, raster.shape, np.uint8)
        finally:
            hip_ctx.free(d)
        assert (back[:h, :w] == exp).all()
        assert (back[:h, w:] == 0xA5).all() and (back[h:] == 0xA5).all()


def test_invalid_blocks_are_counted_zero_filled_and_do_not_stop_the_rest(hip_ctx, golden):
    blocks = golden["level3_blocks"].copy()
    nbx, nby, _n = (int(v) for v in golden["level3_grid"])
    modes = T.block_modes(blocks)
    two_subset = np.flatnonzero(np.isin(modes, (2, 4, 9, 16)))
    assert two_subset.size >= 8
    # a pattern index out of range: all ones written over the block's 5-bit pattern field (found as the first 5-bit window past the 7 bits that can hold the mode code
    # which makes the block invalid when filled with ones; nothing but the pattern check can fail there)
    victims = []
    for i in two_subset[:: max(1, two_subset.size // 8)][:8]:
        v = int.from_bytes(blocks[i].tobytes(), "little")
        for ofs in range(7, 48):
            cand = np.frombuffer((v | (31 << ofs)).to_bytes(16, "little"), np.uint8)
            if T.block_modes(cand[None])[0] == 255:
                blocks[i] = cand
                victims.append(int(i))
                break
    assert len(victims) == 8
    keep = np.ones(blocks.shape[0], bool)
    keep[victims] = False
    for name, (target, hq) in CASES.items():
        with pytest.raises(transcode.InvalidBlocksError) as e:
            transcode.transcode_uastc_blocks(hip_ctx, blocks, nbx, nby, target, high_quality=hq)
        assert e.value.count == len(victims), name
        # the same call through the C ABI, to look at what it wrote
        import ctypes as C
        d_in, nbytes = hip_ctx.upload(blocks), hip_ctx.lib.transcode_output_bytes(nbx, nby, 0, 0, target)
        d_out = hip_ctx.alloc(nbytes)
        try:
            invalid = C.c_uint32(0)
            hip_ctx.check(hip_ctx.lib.k_transcode_uastc(hip_ctx.h, C.c_void_p(d_in), nbx, nby, 0, 0, target, 32 if hq else 0, -1, -1, C.c_void_p(d_out), 0, 0, C.byref(invalid)))
            raw = hip_ctx.download(d_out, (nbytes,), np.uint8)
        finally:
            hip_ctx.free(d_in)
            hip_ctx.free(d_out)
        assert invalid.value == len(victims)
        got = _as_blocks(raw.reshape(nby * 4, nbx * 4, 4) if target == transcode.RGBA32 else raw.reshape(nbx * nby, -1), target, nbx, nby)
        assert (got[victims] == 0).all(), name
        assert (got[keep] == golden[f"level3_{name}"][keep]).all(), name


def test_unsupported_target_is_an_error(hip_ctx):
    import ctypes as C
    d = hip_ctx.alloc(64)
    try:
        invalid = C.c_uint32(0)
        for target in (0, 1, 8, 14, 16, 22):
            assert hip_ctx.lib.k_transcode_uastc(hip_ctx.h, C.c_void_p(d), 1, 1, 0, 0, target, 0, -1, -1, C.c_void_p(d), 0, 0, C.byref(invalid)) == 0
            assert hip_ctx.lib.transcode_output_bytes(1, 1, 0, 0, target) == 0
    finally:
        hip_ctx.free(d)


def test_big_4096_resident_blocks_every_target(hip_ctx):
    """BASELINE's 4096x4096 synthetic image: encoded at level 2 into HBM, transcoded from there to every target, chunk digests against the reference tool's."""
    g = json.loads((HERE / "golden" / "uastc_transcode_big_digests.json").read_text())["synth4096_l2"]
    px = helpers.to_pixel_blocks(helpers.synth(g["width"], g["height"], g["seed"]))
    n, c = g["n_blocks"], g["chunk_blocks"]
    assert px.shape[0] == n
    d_blocks = hip_ctx.alloc(n * 16)
    try:
        uastc.encode_uastc_blocks(hip_ctx, px, g["flags"], out_device=d_blocks)
        assert hashlib.sha256(hip_ctx.download(d_blocks, (n, 16), np.uint8).tobytes()).hexdigest() == g["source_sha256"]
        for name, (target, hq) in CASES.items():
            got = _as_blocks(transcode.transcode_uastc_blocks(hip_ctx, d_blocks, 1024, 1024, target, high_quality=hq), target, 1024, 1024)
            want = g["targets"][name]["chunk_sha256"]
            bad = [i for i in range(len(want)) if hashlib.sha256(np.ascontiguousarray(got[i * c:(i + 1) * c]).tobytes()).hexdigest() != want[i]]
            assert not bad, f"{name}: chunks {bad} of {len(want)} differ from the reference"
    finally:
        hip_ctx.free(d_blocks)


@pytest.mark.parametrize("name", ["k03", "k20"])
def test_transcode_file_of_compress_output(hip_ctx, name):
    """compress(uastc, ktx2, mipmaps) -> transcode_file: every level to every target without an invalid block; level 0 as RGBA32 has the PSNR the reference's decode of
    the reference's blocks has (tests/golden/kodak24_digests.json), the gate tests/test_gpu_kodak24.py computes through the CPU checker."""
    digests = json.loads((HERE / "golden" / "kodak24_digests.json").read_text())["images"][name]
    rgb = np.load(HERE / "golden" / "kodak24.npz")[name]
    img = np.concatenate([rgb, np.full(rgb.shape[:2] + (1,), 255, np.uint8)], axis=2)
    data = compress(hip_ctx, img, uastc=True, ktx2=True, mipmaps=True)
    info = transcode.read_uastc_file(data.tobytes())
    h, w = img.shape[:2]
    assert (info["width"], info["height"]) == (w, h) and len(info["levels"]) > 1
    for level in info["levels"]:
        for target, hq in CASES.values():
            out = transcode.transcode_file(hip_ctx, data, target, level=level, high_quality=hq)
            lw, lh = max(w >> level, 1), max(h >> level, 1)
            assert out.shape == ((lh, lw, 4) if target == transcode.RGBA32 else (((lw + 3) // 4) * ((lh + 3) // 4), transcode.BYTES_PER_BLOCK[target]))
    p = helpers.psnr(transcode.transcode_file(hip_ctx, data, transcode.RGBA32), img)
    assert abs(p - digests["uastc_psnr_rgba"]) < 1e-3, p
