"""-m gpu tests of the device-side UASTC LDR 4x4 transcoder (include/basisu_hip.h: bu_hip_k_transcode_uastc; basis_universal_amd/transcode.py) against the reference's
known answers: on encoder output tests/golden/uastc_transcode_vectors.npz and uastc_transcode_big_digests.json, on arbitrary valid and invalid blocks no encoder
writes tests/golden/uastc_transcode_fuzz.npz (tools/gen_golden_uastc_transcode.py ran oracle/_ref on the build machine for all three). Where no golden exists (odd
sizes, spliced invalid blocks, a million random-bit blocks) the expected values come from the g++ build of the same core, which tests/test_uastc_transcode_host.py
holds to the reference on encoder output, on the fuzz fixture and on fresh random blocks."""
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


# ---------------------------------------------------------------- blocks no encoder writes

@pytest.fixture(scope="module")
def fuzz():
    return np.load(HERE / "golden" / "uastc_transcode_fuzz.npz")


def _channels(target, ch):
    """FUZZ_CASES' channel pair as transcode_uastc_blocks takes it"""
    return (ch[0],) if target == transcode.BC4_R else (ch if target == transcode.BC5_RG else None)


def _c_abi(hip_ctx, blocks, nbx, nby, target, hq, ch, width=0, height=0):
    """bu_hip_k_transcode_uastc on (nby * nbx, 16) host blocks or a device pointer -> (what it wrote, its `invalid` out-parameter). The call succeeds whatever the blocks are."""
    import ctypes as C
    own = hip_ctx.upload(np.ascontiguousarray(blocks, np.uint8)) if isinstance(blocks, np.ndarray) else None
    nbytes = hip_ctx.lib.transcode_output_bytes(nbx, nby, width, height, target)
    assert nbytes == ((width or nbx * 4) * (height or nby * 4) * 4 if target == transcode.RGBA32 else nbx * nby * transcode.BYTES_PER_BLOCK[target])
    d_out = hip_ctx.alloc(nbytes)
    try:
        invalid = C.c_uint32(0xFFFFFFFF)
        c0, c1 = (ch[0], -1) if target == transcode.BC4_R else (ch if target == transcode.BC5_RG else (-1, -1))
        hip_ctx.check(hip_ctx.lib.k_transcode_uastc(hip_ctx.h, C.c_void_p(own if own is not None else blocks), nbx, nby, width, height, target, 32 if hq else 0, c0, c1,
                                                    C.c_void_p(d_out), 0, 0, C.byref(invalid)))
        raw = hip_ctx.download(d_out, (nbytes,), np.uint8)
    finally:
        if own is not None:
            hip_ctx.free(own)
        hip_ctx.free(d_out)
    if target == transcode.RGBA32:
        return raw.reshape(height or nby * 4, width or nbx * 4, 4), invalid.value
    return raw.reshape(nbx * nby, -1), invalid.value


@pytest.mark.parametrize("name", sorted(T.FUZZ_CASES))
def test_device_equals_reference_on_fuzz_families(hip_ctx, fuzz, name):
    """Every family of the fuzz fixture, one launch each through the C ABI and one through transcode_uastc_blocks: blocks the reference accepts byte-equal, blocks it
    refuses zero-filled, and both ways of reporting the invalid count equal to the fixture's."""
    target, hq, ch = T.FUZZ_CASES[name]
    for f, family in enumerate(T.FAMILIES):
        pick = fuzz["family"] == f
        blocks, exp, valid = np.ascontiguousarray(fuzz["blocks"][pick]), fuzz[name][pick], fuzz["valid"][pick]
        n, bad = blocks.shape[0], int((valid == 0).sum())
        assert n > 0
        got, invalid = _c_abi(hip_ctx, blocks, n, 1, target, hq, ch)
        T.assert_equals_reference(blocks, exp, valid, _as_blocks(got, target, n, 1), None, f"device, {name}, family {family}", fuzz["family"][pick])
        assert invalid == bad, (name, family)
        if bad:
            with pytest.raises(transcode.InvalidBlocksError) as e:
                transcode.transcode_uastc_blocks(hip_ctx, blocks, n, 1, target, high_quality=hq, channels=_channels(target, ch))
            assert e.value.count == bad, (name, family)
        else:
            out = _as_blocks(transcode.transcode_uastc_blocks(hip_ctx, blocks, n, 1, target, high_quality=hq, channels=_channels(target, ch)), target, n, 1)
            assert (out == exp).all(), (name, family)


@pytest.mark.parametrize("name", sorted(T.FUZZ_CASES))
def test_device_fuzz_blocks_on_ragged_grids(hip_ctx, fuzz, name):
    """The whole fixture (valid and invalid blocks mixed) as grids whose block count is not a multiple of the 256-lane workgroup: one row, one column, a width that leaves a
    ragged last workgroup, fewer blocks than one workgroup; RGBA32 also cropped so that the last column and row of tiles are cut."""
    target, hq, ch = T.FUZZ_CASES[name]
    total = fuzz["blocks"].shape[0]
    assert total % 256 != 0
    for nbx, nby in ((total, 1), (1, total), (37, total // 37), (9, 11), (1, 1)):
        n = nbx * nby
        assert n == 1 or n % 256 != 0
        blocks, exp, valid = np.ascontiguousarray(fuzz["blocks"][:n]), fuzz[name][:n], fuzz["valid"][:n]
        got, invalid = _c_abi(hip_ctx, blocks, nbx, nby, target, hq, ch)
        T.assert_equals_reference(blocks, exp, valid, _as_blocks(got, target, nbx, nby), None, f"device, {name}, {nbx} x {nby} blocks", fuzz["family"][:n])
        assert invalid == int((valid == 0).sum()), (name, nbx, nby)
        if target == transcode.RGBA32:
            for cut_w, cut_h in ((1, 3), (3, 1), (2, 0), (0, 2)):
                w, h = nbx * 4 - cut_w, nby * 4 - cut_h
                got, invalid = _c_abi(hip_ctx, blocks, nbx, nby, target, hq, ch, width=w, height=h)
                assert got.shape == (h, w, 4) and (got == T.to_raster(exp.reshape(n, 4, 4, 4), nbx, nby, w, h)).all(), (nbx, nby, w, h)
                assert invalid == int((valid == 0).sum())


def test_device_equals_host_core_on_a_million_random_blocks(hip_ctx):
    """1,048,576 random-bit blocks uploaded once and transcoded to every target from the resident buffer: the one full-size launch of blocks no encoder wrote. Output, zero
    fill and invalid count against the g++ build of the core; a strided sample of 65,536 blocks also against the reference itself where oracle/_ref is there."""
    n = 1 << 20
    blocks = T.random_bit_blocks(n, 20261019)
    sample = np.arange(0, n, 16)
    with_ref = helpers.ref_harness_version() >= 3
    d_blocks = hip_ctx.upload(blocks)
    try:
        for name, (target, hq, ch) in T.FUZZ_CASES.items():
            got, invalid = _c_abi(hip_ctx, d_blocks, 1024, 1024, target, hq, ch)
            got = _as_blocks(got, target, 1024, 1024)
            exp, ok = T.host_transcode(blocks, target, hq, ch)
            assert ok.mean() > 0.9
            T.assert_equals_reference(blocks, exp, ok, got, None, f"device against the host core, {name}")
            assert invalid == int((ok == 0).sum()), name
            if with_ref:
                ref_out, ref_ok = helpers.ref_transcode_uastc(blocks[sample], target, hq, ch)
                T.assert_equals_reference(blocks[sample], ref_out, ref_ok, got[sample], None, f"device against the reference, {name}")
            with pytest.raises(transcode.InvalidBlocksError) as e:
                transcode.transcode_uastc_blocks(hip_ctx, d_blocks, 1024, 1024, target, high_quality=hq, channels=_channels(target, ch))
            assert e.value.count == invalid, name
    finally:
        hip_ctx.free(d_blocks)
