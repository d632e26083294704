"""-m gpu: bu_hip_k_extract_slices (k_extract_slices, csrc/etc1s_misc_kernels.hip) -- every slice of a call tiled by one launch -- against numpy and against the
per-slice kernels it stands in for (k_extract_blocks after k_split_alpha). Every comparison is equality of bytes; the output lies between guard tiles."""
import ctypes as C
import re

import numpy as np
import pytest

from basis_universal_amd import source

pytestmark = pytest.mark.gpu
GUARD = 0xA5
AS_IS, RGB, ALPHA = source.SLICE_AS_IS, source.SLICE_RGB, source.SLICE_ALPHA


def picture(w, h, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 4), dtype=np.uint8)


def expected_tiles(img, mode):
    """image::extract_block_clamped per 4x4 block, block-raster order -> (blocks, 64) u8; mode 1: (r, g, b, 255), mode 2: (a, a, a, 255)"""
    h, w = img.shape[:2]
    px = img.copy()
    if mode == RGB:
        px[..., 3] = 255
    elif mode == ALPHA:
        px = np.concatenate([np.repeat(img[..., 3:4], 3, axis=2), np.full((h, w, 1), 255, np.uint8)], axis=2)
    nbx, nby = (w + 3) // 4, (h + 3) // 4
    px = np.pad(px, ((0, nby * 4 - h), (0, nbx * 4 - w), (0, 0)), mode="edge")
    return np.ascontiguousarray(px.reshape(nby, 4, nbx, 4, 4).transpose(0, 2, 1, 3, 4)).reshape(nby * nbx, 64)


class Call:
    """one bu_hip_k_extract_slices call: specs = [(image, pitch in bytes or 0, mode, tiles skipped before the slice)]; the output has `lead` guard tiles in
    front (the pointer the call gets lies behind them) and 64 behind"""

    def __init__(self, ctx, specs, lead=3):
        self.ctx, self.specs, self.lead, self.owned, self.entries, self.ranges = ctx, specs, lead, [], [], []
        at = 0
        for img, pitch, mode, gap in specs:
            h, w = img.shape[:2]
            pitch = pitch or w * 4
            rows = np.full((h, pitch), 0x3C, np.uint8)       # what lies in a row's padding must never reach a tile
            rows[:, :w * 4] = img.reshape(h, w * 4)
            d = ctx.upload(rows)
            self.owned.append(d)
            at += gap
            n = ((w + 3) // 4) * ((h + 3) // 4)
            self.entries.append((d, w, h, pitch, mode, at))
            self.ranges.append((at, n))
            at += n
        self.total = at
        self.d_buf = ctx.upload(np.full((lead + at + 64, 64), GUARD, np.uint8))
        self.owned.append(self.d_buf)
        self.d_out = self.d_buf + lead * 64

    def run(self):
        source.extract_slices_resident(self.ctx, self.entries, self.d_out)
        return self.download()

    def download(self):
        return self.ctx.download(self.d_buf, (self.lead + self.total + 64, 64), np.uint8)

    def check(self, got):
        written = np.zeros(got.shape[0], bool)
        for (img, _, mode, _), (first, n) in zip(self.specs, self.ranges):
            exp = expected_tiles(img, mode)
            assert exp.shape[0] == n
            mine = got[self.lead + first:self.lead + first + n]
            assert (mine == exp).all(), (img.shape, mode, first, np.argwhere((mine != exp).any(axis=1))[:4].ravel())
            written[self.lead + first:self.lead + first + n] = True
        assert (got[~written] == GUARD).all(), "something outside the slices' ranges was written"

    def close(self):
        for d in self.owned:
            self.ctx.free(d)


def run_and_check(ctx, specs, lead=3):
    call = Call(ctx, specs, lead)
    try:
        got = call.run()
        call.check(got)
        return got
    finally:
        call.close()


SHAPES = {
    "one_pixel": [(picture(1, 1, 1), 0, AS_IS, 0)],
    "five_by_seven": [(picture(5, 7, 2), 0, AS_IS, 0)],
    # 1, 35 and 64 blocks: the first wave holds slice 0, and 15 tiles of slice 1; a later one the end of slice 1 and the start of slice 2
    "waves_straddle_slices": [(picture(4, 4, 3), 0, AS_IS, 0), (picture(20, 28, 4), 0, AS_IS, 0), (picture(32, 32, 5), 0, AS_IS, 0)],
    "ragged_35_blocks": [(picture(3, 2, 6), 0, AS_IS, 0), (picture(18, 27, 7), 0, AS_IS, 0), (picture(29, 30, 8), 0, AS_IS, 0)],
    # a wave of three slices: 1 + 2 + 70 blocks
    "three_slices_in_a_wave": [(picture(2, 3, 9), 0, RGB, 0), (picture(8, 4, 10), 0, ALPHA, 0), (picture(40, 28, 11), 0, AS_IS, 0)],
    "first_block_off_the_wave_grid": [(picture(12, 8, 12), 0, AS_IS, 5), (picture(16, 16, 13), 0, RGB, 7), (picture(9, 9, 14), 0, ALPHA, 66)],
    # a row pitch beyond the row: 48 bytes keeps the rows 16-byte aligned (whole-row loads), 44 and 36 do not; 80 for a 5-pixel row
    "padded_pitch": [(picture(8, 8, 15), 48, AS_IS, 0), (picture(8, 8, 16), 44, RGB, 0), (picture(8, 5, 17), 36, ALPHA, 0), (picture(5, 8, 18), 80, ALPHA, 0), (picture(16, 12, 19), 128, RGB, 0)],
    "modes_mixed": [(picture(16, 16, 20), 0, RGB, 0), (picture(16, 16, 20), 0, ALPHA, 0), (picture(7, 5, 21), 0, AS_IS, 0), (picture(7, 5, 22), 0, ALPHA, 0), (picture(7, 5, 22), 0, RGB, 0),
                    (picture(64, 36, 23), 0, ALPHA, 0)],
    # past one wave's (64) and one workgroup's (256) worth of table entries
    "65_slices_of_one_block": [(picture(1 + k % 4, 1 + (k // 4) % 4, 100 + k), 0, k % 3, 0) for k in range(65)],
    "300_slices_of_one_block": [(picture(1 + k % 4, 1 + (k // 4) % 4, 200 + k), 0, k % 3, k % 2) for k in range(300)],
}


@pytest.mark.parametrize("name", list(SHAPES))
def test_tiles_equal_numpy_and_nothing_else_is_written(hip_ctx, name):
    run_and_check(hip_ctx, SHAPES[name])


def test_misaligned_lead_keeps_every_range_in_place(hip_ctx):
    """the same call behind 1 and behind 64 guard tiles: the output pointer itself is no multiple of a wave's or a workgroup's tiles"""
    a = run_and_check(hip_ctx, SHAPES["modes_mixed"], lead=1)
    b = run_and_check(hip_ctx, SHAPES["modes_mixed"], lead=64)
    assert (a[1:-64] == b[64:-64]).all()


def test_equals_the_per_slice_kernels(hip_ctx):
    """what compress() did before per level with alpha: k_split_alpha into two planes, then k_extract_blocks of each -- here one launch over the RGBA rasters"""
    ctx = hip_ctx
    images = [picture(20, 28, 30), picture(10, 14, 31), picture(5, 7, 32), picture(3, 4, 33), picture(2, 2, 34), picture(1, 1, 35)]
    specs = [(img, 0, mode, 0) for img in images for mode in (RGB, ALPHA)] + [(images[0], 0, AS_IS, 0)]
    call = Call(ctx, specs, lead=0)
    owned = []
    try:
        got = call.run()
        call.check(got)
        d_ref = ctx.upload(np.full((call.total, 64), GUARD, np.uint8))
        owned.append(d_ref)
        for (img, _, mode, _), (d_raster, w, h, pitch, _, first) in zip(specs, call.entries):
            d_plane = d_raster
            if mode != AS_IS:
                d_rgb, d_a = ctx.alloc(w * h * 4), ctx.alloc(w * h * 4)
                owned += [d_rgb, d_a]
                source.split_alpha_resident(ctx, d_raster, w, h, d_rgb, d_a)
                d_plane = d_rgb if mode == RGB else d_a
            ctx.check(ctx.lib.k_extract_blocks(ctx.h, d_plane, w, h, w * 4, d_ref + first * 64), "k_extract_blocks")
        ref = ctx.download(d_ref, (call.total, 64), np.uint8)
        assert (got[:call.total] == ref).all()
    finally:
        call.close()
        for d in owned:
            ctx.free(d)


def test_refusals_name_their_cause_and_write_nothing(hip_ctx):
    ctx = hip_ctx
    call = Call(ctx, [(picture(8, 8, 40), 0, AS_IS, 0), (picture(8, 8, 41), 0, RGB, 0)], lead=2)
    try:
        (d0, w, h, pitch, _, _), (d1, *_rest) = call.entries
        good = [(d0, w, h, pitch, AS_IS, 0), (d1, w, h, pitch, RGB, 4)]
        bad = {
            "no slices": [],
            "zero size": [good[0], (d1, 0, h, pitch, RGB, 4)],
            "zero size (8 x 0)": [good[0], (d1, w, 0, pitch, RGB, 4)],
            "row pitch 28 bytes is less than 4 * width = 32": [good[0], (d1, w, h, 28, RGB, 4)],
            "slice 1: first_block 3 lies before the end of slice 0's blocks (4)": [good[0], (d1, w, h, pitch, RGB, 3)],          # overlapping
            "slice 1: first_block 0 lies before the end": [(d0, w, h, pitch, AS_IS, 4), (d1, w, h, pitch, RGB, 0)],                    # not ascending
            "unknown mode 3": [good[0], (d1, w, h, pitch, 3, 4)],
            "slice 1: null raster": [good[0], (None, w, h, pitch, RGB, 4)],
        }
        for match, entries in bad.items():
            with pytest.raises(Exception, match="k_extract_slices failed: extract_slices: .*" + re.escape(match)):
                source.extract_slices_resident(ctx, entries, call.d_out)
            assert (call.download() == GUARD).all(), match
        arr = (source.SliceSource * 1)(source.SliceSource(d0, w, h, pitch, AS_IS, 0))
        assert not ctx.lib.k_extract_slices(ctx.h, arr, 1, None) and "null pointer" in ctx.lib.last_error(ctx.h)
        assert not ctx.lib.k_extract_slices(ctx.h, None, 1, C.c_void_p(call.d_out)) and "null pointer" in ctx.lib.last_error(ctx.h)
        assert not ctx.lib.k_extract_slices(ctx.h, arr, 1, C.c_void_p(call.d_out + 8)) and "16-byte aligned" in ctx.lib.last_error(ctx.h)
        assert (call.download() == GUARD).all()
        # and the same arguments put right are accepted: the refusals above were about what they name
        source.extract_slices_resident(ctx, good, call.d_out)
        call.check(call.download())
    finally:
        call.close()
