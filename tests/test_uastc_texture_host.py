"""The UASTC texture family's further targets (ETC1, ETC2 RGBA, EAC R11 / RG11, RGB565 / BGR565 / RGBA4444) on the CPU: the g++ build of the core
(tests/native/uastc_texture_host.cpp) against the reference tool's known answers (tests/golden/uastc_texture_vectors.npz, tools/gen_golden_uastc_texture.py),
the plumbing between channels and targets, the refusals of the Python entry points, and the core under the host sanitizers."""
import os
import pathlib
import shutil
import subprocess

import numpy as np
import pytest

import multi_image_helpers as M
import transcode_helpers as T
import uastc_texture_helpers as U
from basis_universal_amd import transcode

ROOT = pathlib.Path(__file__).resolve().parent.parent
SETS = U.ENCODER_SETS + ("fuzz",)


def _grid(name):
    if name == "fuzz":
        grid, nbx, nby, _, _ = U.fuzz_valid_grid()
        return grid, nbx, nby
    return U.encoder_grid(name)


@pytest.fixture(scope="module")
def golden():
    return U.golden()[0]


@pytest.fixture(scope="module")
def old_golden():
    return np.load(ROOT / "tests" / "golden" / "uastc_transcode_vectors.npz")


def test_fixture_inputs_cover_every_hint_value(golden):
    """the conditions the generator asserts before it writes, on the committed inputs: each flip x diff, each intensity table, each EAC table at least 100 times
    among the non-solid valid blocks, bias-carrying and bias-free modes at least 100 each, at least 20 blocks with EAC multiplier 0; and all 19 modes"""
    grid, nbx, nby, n_valid, idx = U.fuzz_valid_grid()
    assert golden["fuzz_grid"].tolist() == [nbx, nby, n_valid]
    meta = U.golden()[1]
    assert U.check_hint_coverage(grid[:n_valid]) == meta["fuzz_hint_coverage"]
    fuzz = np.load(ROOT / "tests" / "golden" / "uastc_transcode_fuzz.npz")
    assert (fuzz["valid"][idx] != 0).all() and idx.size == int((fuzz["valid"] != 0).sum())
    modes = np.concatenate([T.block_modes(U.encoder_grid(s)[0]) for s in U.ENCODER_SETS])
    assert (np.bincount(modes, minlength=19)[:19] > 0).all()


@pytest.mark.parametrize("case", sorted(U.BLOCK_CASES))
@pytest.mark.parametrize("which", SETS)
def test_host_core_equals_reference(golden, which, case):
    target, hq, _ = U.BLOCK_CASES[case]
    blocks, _, _ = _grid(which)
    got, ok = U.host_texture(blocks, target, hq)
    exp = golden[f"{which}_{case}"]
    T.assert_equals_reference(blocks, exp, np.ones(blocks.shape[0], np.uint8), got, ok, f"{which} {case}")


@pytest.mark.parametrize("crop", (False, True))
def test_host_pixels_equal_reference(golden, crop):
    """RGB565 and RGBA4444 as the tool's PNGs have them, whole and as the 254 x (4 nby - 3) image; BGR565, which the tool never writes, is checked as RGB565 with R
    and B exchanged"""
    blocks, nbx, nby = U.encoder_grid(U.PIXEL_SET)
    w, h = (U.CROP_W, 4 * nby - 3) if crop else (4 * nbx, 4 * nby)
    tag = f"{U.PIXEL_SET}_crop" if crop else U.PIXEL_SET
    for name, target in (("rgb565", U.RGB565), ("rgba4444", U.RGBA4444)):
        got = U.tiles16_to_raster(U.host_texture(blocks, target)[0], nbx, nby, w, h)
        assert golden[f"{tag}_{name}"].shape == (h, w) and (got == golden[f"{tag}_{name}"]).all(), (tag, name)
    bgr = U.tiles16_to_raster(U.host_texture(blocks, U.BGR565)[0], nbx, nby, w, h)
    assert (bgr == U.swap_565(golden[f"{tag}_rgb565"])).all()


def test_channel_plumbing(golden, old_golden):
    """R11 of channel c = pack_eac of channel c of the decoded texels (c = 0 is what the tool shows; 1 and 2 it does not), with high quality pack_eac_high_quality;
    R11 of channel 3 = the EAC half of ETC2 RGBA (the hint's route); RG11 = two R11 side by side; on solid blocks R11 carries multiplier 0 and ETC2's alpha half
    multiplier 1."""
    for s in U.ENCODER_SETS:
        blocks, _, _ = U.encoder_grid(s)
        texels = old_golden[f"{s}_rgba32"].reshape(-1, 16, 4)
        solid = T.block_modes(blocks) == 8
        assert solid.any() and (~solid).any()
        for hq, tag in ((False, ""), (True, "_hq")):
            r11 = [U.host_texture(blocks, U.R11, hq, (c, 3))[0] for c in range(4)]
            assert (r11[0] == golden[f"{s}_r11{tag}"]).all()
            for c in range(3):
                assert (r11[c][~solid] == U.host_pack_eac(texels[~solid][:, :, c], hq)).all(), (s, c, hq)
            assert (r11[3][~solid] == golden[f"{s}_etc2"][~solid][:, :8]).all(), (s, hq)
            for c0, c1 in ((0, 3), (1, 2), (3, 0), (2, 2)):
                rg = U.host_texture(blocks, U.RG11, hq, (c0, c1))[0]
                assert (rg[:, :8] == r11[c0]).all() and (rg[:, 8:] == r11[c1]).all(), (s, c0, c1, hq)
            assert (golden[f"{s}_rg11{tag}"][:, :8] == r11[0]).all() and (golden[f"{s}_rg11{tag}"][:, 8:] == r11[3]).all()
            for c in range(4):
                assert (U.eac_multiplier(r11[c][solid]) == 0).all() and (r11[c][solid][:, 0] == texels[solid][:, 0, c]).all()
        assert (U.eac_multiplier(golden[f"{s}_etc2"][solid][:, :8]) == 1).all()
        assert (golden[f"{s}_etc2"][:, 8:] == golden[f"{s}_etc1"]).all()


def test_pack_eac_branches():
    """pack_eac on values chosen for each branch: constant (multiplier 0), a range of 5 or less (table 13, multiplier 1, lossless), and wide ranges that touch
    0 and 255 (the clamped selector search: multiplier 1..15, and without high quality one of the four tables)"""
    tables = np.array([[-3, -6, -9, -15, 2, 5, 8, 14], [-3, -7, -10, -13, 2, 6, 9, 12], [-2, -5, -8, -13, 1, 4, 7, 12], [-2, -4, -6, -13, 1, 3, 5, 12],
                       [-3, -6, -8, -12, 2, 5, 7, 11], [-3, -7, -9, -11, 2, 6, 8, 10], [-4, -7, -8, -11, 3, 6, 7, 10], [-3, -5, -8, -11, 2, 4, 7, 10],
                       [-2, -6, -8, -10, 1, 5, 7, 9], [-2, -5, -8, -10, 1, 4, 7, 9], [-2, -4, -8, -10, 1, 3, 7, 9], [-2, -5, -7, -10, 1, 4, 6, 9],
                       [-3, -4, -7, -10, 2, 3, 6, 9], [-1, -2, -3, -10, 0, 1, 2, 9], [-4, -6, -8, -9, 3, 5, 7, 8], [-3, -5, -7, -9, 2, 4, 6, 8]])
    rng = np.random.default_rng(7)
    const = np.repeat(np.array([0, 1, 128, 254, 255], np.uint8)[:, None], 16, 1)
    narrow = (rng.integers(0, 6, (64, 16)) + rng.integers(0, 246, (64, 1))).astype(np.uint8)
    narrow[:, 0], narrow[:, 1] = narrow.min(1), narrow.min(1) + 5
    wide = rng.integers(0, 256, (256, 16)).astype(np.uint8)
    wide[:64, :2] = (0, 255)
    for hq in (False, True):
        c = U.host_pack_eac(const, hq)
        assert (c[:, 0] == const[:, 0]).all() and (c[:, 1] == 13).all()
        for vals in (narrow, wide):
            blk = U.host_pack_eac(vals, hq)
            base, table, mul = blk[:, 0].astype(np.int64), blk[:, 1] & 15, (blk[:, 1] >> 4).astype(np.int64)
            bits = np.zeros(vals.shape[0], np.uint64)
            for k in range(6):
                bits |= blk[:, 2 + k].astype(np.uint64) << np.uint64(8 * (5 - k))
            dec = np.zeros(vals.shape, np.int64)
            for i in range(16):
                sel = (bits >> np.uint64(45 - 3 * ((i & 3) * 4 + (i >> 2)))) & np.uint64(7)
                dec[:, i] = np.clip(base + tables[table, sel.astype(np.int64)] * mul, 0, 255)
            if vals is narrow:
                assert (dec == vals).all() and (table == 13).all() and (mul == 1).all(), hq
            else:
                assert (mul >= 1).all() and (hq or np.isin(table, (2, 8, 11, 13)).all())


def test_first_family_targets_through_the_texture_entry(old_golden):
    """the seven targets the two families share: the texture family's host entry writes what the first family's does"""
    for s in U.ENCODER_SETS:
        blocks = old_golden[f"{s}_blocks"]
        for name, (target, hq, ch) in T.FUZZ_CASES.items():
            got, ok = U.host_texture(blocks, target, hq, ch)
            exp, exp_ok = T.host_transcode(blocks, target, hq, ch)
            assert (got == exp.reshape(got.shape)).all() and (ok == exp_ok).all(), (s, name)


def test_refusals_come_before_the_context():
    ctx, one = M.Untouchable(), np.zeros((1, 16), np.uint8)
    file = np.zeros(64, np.uint8)
    for target in U.REFUSED_TARGETS:
        for call in (lambda: transcode.transcode_uastc_texture_blocks(ctx, one, 1, 1, target), lambda: transcode.transcode_uastc_texture_file(ctx, file, target),
                     lambda: transcode.transcode_uastc_textures(ctx, file, target), lambda: transcode.uastc_texture_layout([], target)):
            with pytest.raises(ValueError, match=f"UASTC texture target {target} .*is not supported"):
                call()
    for flags in (1, 2, 4, 8, 16, 64, 128, 256, 512, 1024, 32 | 4, 2 ** 31):
        for call in (lambda: transcode.transcode_uastc_texture_blocks(ctx, one, 1, 1, U.ETC1, decode_flags=flags),
                     lambda: transcode.transcode_uastc_texture_file(ctx, file, U.ETC1, decode_flags=flags), lambda: transcode.transcode_uastc_textures(ctx, file, U.R11, decode_flags=flags)):
            with pytest.raises(ValueError, match="decode flags .*are not supported"):
                call()
    for channels in ((4,), (0, 4), (-1,), (0, 1, 2)):
        for call in (lambda: transcode.transcode_uastc_texture_blocks(ctx, one, 1, 1, U.RG11, channels=channels),
                     lambda: transcode.transcode_uastc_texture_file(ctx, file, U.RG11, channels=channels), lambda: transcode.transcode_uastc_textures(ctx, file, U.RG11, channels=channels)):
            with pytest.raises(ValueError, match="channels"):
                call()
    with pytest.raises(ValueError, match="pixel raster"):
        transcode.transcode_uastc_texture_blocks(ctx, one, 1, 1, U.ETC2, out_device=16, out_row_pitch=8)
    with pytest.raises(ValueError, match="do not fit"):
        transcode.transcode_uastc_texture_blocks(ctx, one, 1, 1, U.RGB565, width=5)
    assert transcode.uastc_decode_flags(high_quality=True) == 32 and transcode.uastc_decode_flags() == 0


def test_first_family_still_refuses_the_new_targets():
    ctx, one = M.Untouchable(), np.zeros((1, 16), np.uint8)
    for target in (0, 1, 14, 15, 16, 20, 21):
        with pytest.raises(ValueError, match="not supported"):
            transcode.transcode_uastc_blocks(ctx, one, 1, 1, target)
        with pytest.raises(ValueError, match="not supported"):
            transcode.image_layout([], target, etc1s=False)
    assert sorted(transcode.BYTES_PER_BLOCK) == [2, 3, 4, 5, 6, 10, 13]


def test_texture_layout():
    images = [{"num_blocks_x": 2, "num_blocks_y": 2, "width": 7, "height": 5}, {"num_blocks_x": 1, "num_blocks_y": 1, "width": 3, "height": 2}]
    lay, total = transcode.uastc_texture_layout(images, U.RGB565)
    assert [(e["offset"], e["nbytes"], e["shape"], e["dtype"]) for e in lay] == [(0, 70, (5, 7), np.uint16), (80, 12, (2, 3), np.uint16)] and total == 96
    lay, total = transcode.uastc_texture_layout(images, U.ETC2)
    assert [(e["offset"], e["nbytes"], e["shape"]) for e in lay] == [(0, 64, (4, 16)), (64, 16, (1, 16))] and total == 80
    lay, total = transcode.uastc_texture_layout(images, U.R11)
    assert [(e["offset"], e["nbytes"], e["shape"]) for e in lay] == [(0, 32, (4, 8)), (32, 8, (1, 8))] and total == 48
    for target in T.BYTES:   # the shared targets lay out as image_layout lays them out
        assert transcode.uastc_texture_layout(images, target) == transcode.image_layout(images, target, etc1s=False)
    assert set(transcode.UASTC_TEXTURE_BYTES_PER_BLOCK) | set(transcode.UASTC_TEXTURE_BYTES_PER_PIXEL) == {0, 1, 2, 3, 4, 5, 6, 10, 13, 14, 15, 16, 20, 21}


def test_core_under_host_sanitizers(tmp_path):
    """the core built with AddressSanitizer and UndefinedBehaviorSanitizer into a stand-alone program (tools/uastc_texture_sanitize.cpp: host code, CPU only,
    a child process, nothing preloaded): 1,000,000 random-bit blocks from a fixed generator through every new target and both qualities, and no sanitizer speaks"""
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed to build the sanitizer program"
    exe = tmp_path / "uastc_texture_sanitize"
    r = subprocess.run([cxx, "-std=c++17", "-O2", "-g", "-fsanitize=address,undefined", "-static-libasan", "-static-libubsan", "-fno-sanitize-recover",
                        "-fno-omit-frame-pointer", "-ffp-contract=off", "-pthread", "-o", str(exe), str(ROOT / "tools" / "uastc_texture_sanitize.cpp")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ)
    env["ASAN_OPTIONS"] = "detect_leaks=1:abort_on_error=0"
    r = subprocess.run([str(exe), "1000000"], capture_output=True, text=True, env=env)
    assert r.returncode == 0 and not r.stderr.strip(), (r.returncode, r.stdout[-500:], r.stderr[-3000:])
    words = r.stdout.split()
    assert int(words[1]) == 1000000 and 0 < int(words[3]) < 100000, r.stdout   # about 3.7 % of random blocks do not unpack
