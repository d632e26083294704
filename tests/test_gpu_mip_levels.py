"""-m gpu: bu_hip_k_prepare_mip_levels (k_prepare_mip_levels, csrc/mip_levels_kernels.hip) -- every supplied mip level of a call into a tight RGBA8 raster by one
launch -- against numpy. Every comparison is equality of bytes; every destination lies between guard bytes, and the flags are exact per level."""
import ctypes as C
import re

import numpy as np
import pytest

from basis_universal_amd import source

pytestmark = pytest.mark.gpu
GUARD, GAP = 0xA5, 20          # guard bytes between, before and behind the rasters: a multiple of 4, not of 16
SIZES = [(1, 1), (2, 3), (5, 7), (10, 14), (65, 3)]   # width x height: one-pixel and sub-wave levels (a wave covers several records), and rows of 65
ORDERS = {"rgba": [0, 1, 2, 3], "bgra": [2, 1, 0, 3]}
SWIZZLES = {"identity": None, "rrrg": "rrrg", "abgr": "abgr"}
LETTERS = {"r": 0, "g": 1, "b": 2, "a": 3}


def opaque_picture(w, h, seed):
    img = np.random.default_rng(seed).integers(0, 256, (h, w, 4), dtype=np.uint8)
    img[..., 3] = 255
    return img


def expected(level, swizzle):
    return level if swizzle is None else np.ascontiguousarray(level[..., [LETTERS[c] for c in swizzle]])


class Call:
    """one bu_hip_k_prepare_mip_levels call over `levels` (RGBA arrays) stored in `order` with GAP bytes of junk between them in the payload; the rasters are laid
    out with GAP guard bytes before, between and behind them"""

    def __init__(self, ctx, levels, order, swizzle):
        self.ctx, self.levels, self.swizzle = ctx, levels, swizzle
        selector = source.level_selector(order, swizzle)
        payload, self.records, at = [], [], GAP
        src = 0
        for lv in levels:
            h, w = lv.shape[:2]
            payload.append(np.full(GAP, 0x3C, np.uint8))
            payload.append(np.ascontiguousarray(lv[..., ORDERS[order]]).reshape(-1))
            src += GAP
            self.records.append((src, at, w, h, selector))
            src += w * h * 4
            at += w * h * 4 + GAP
        self.payload = np.concatenate(payload) if payload else np.zeros(4, np.uint8)
        self.out_bytes = at
        self.d_payload = ctx.upload(self.payload)
        self.d_out = ctx.upload(np.full(self.out_bytes, GUARD, np.uint8))
        self.d_flags = ctx.upload(np.full(max(len(levels), 1) + 1, 0xDEADBEEF, np.uint32))   # one word more than the call may touch

    def run(self, records=None):
        source.prepare_mip_levels_resident(self.ctx, self.d_payload, self.payload.size, self.records if records is None else records, self.d_out, self.out_bytes, self.d_flags)
        return self.download()

    def download(self):
        return self.ctx.download(self.d_out, (self.out_bytes,), np.uint8), self.ctx.download(self.d_flags, (max(len(self.levels), 1) + 1,), np.uint32)

    def check(self, got, flags):
        written = np.zeros(got.size, bool)
        for k, (lv, (_, at, w, h, _)) in enumerate(zip(self.levels, self.records)):
            exp = expected(lv, self.swizzle)
            mine = got[at:at + w * h * 4].reshape(h, w, 4)
            assert (mine == exp).all(), (k, w, h, np.argwhere((mine != exp).any(axis=2))[:4].tolist())
            written[at:at + w * h * 4] = True
            assert flags[k] == int((exp[..., 3] != 255).any()), (k, flags[:len(self.levels)].tolist())
        assert (got[~written] == GUARD).all(), "bytes outside the levels' rasters were written"
        assert flags[len(self.levels)] == 0xDEADBEEF, "a flag word past the records was written"

    def untouched(self):
        got, flags = self.download()
        assert (got == GUARD).all() and (flags == 0xDEADBEEF).all(), "a refused call wrote something"

    def close(self):
        for d in (self.d_payload, self.d_out, self.d_flags):
            self.ctx.free(d)


def levels_of(seed, alpha_at=None):
    """SIZES as opaque pictures; alpha_at = (level, y, x): that one pixel of that one level gets alpha 254"""
    levels = [opaque_picture(w, h, seed + i) for i, (w, h) in enumerate(SIZES)]
    if alpha_at is not None:
        k, y, x = alpha_at
        levels[k][y, x, 3] = 254
    return levels


@pytest.mark.parametrize("swizzle", list(SWIZZLES))
@pytest.mark.parametrize("order", list(ORDERS))
def test_levels_of_every_size_in_one_call(hip_ctx, order, swizzle):
    """1x1, 2x3, 5x7, 10x14 and 65x3 in ONE launch; the levels carry random colour and are opaque, so with `rrrg` and `abgr` every level's alpha comes from a colour
    channel and its flag is set, and with the identity none is"""
    call = Call(hip_ctx, levels_of(100), order, SWIZZLES[swizzle])
    try:
        hip_ctx.profile_enable(True)
        got, flags = call.run()
        regions = hip_ctx.profile_read()
        hip_ctx.profile_enable(False)
        call.check(got, flags)
        assert regions["prepare_mip_levels"][1] == 1          # one region, which is one launch
    finally:
        call.close()


@pytest.mark.parametrize("order", list(ORDERS))
@pytest.mark.parametrize("at", [(0, 0, 0), (1, 2, 1), (2, 6, 4), (3, 13, 9), (4, 2, 64)], ids=[f"{w}x{h}" for w, h in SIZES])
def test_alpha_in_one_pixel_of_one_level_sets_that_levels_flag_alone(hip_ctx, order, at):
    call = Call(hip_ctx, levels_of(200, alpha_at=at), order, None)
    try:
        got, flags = call.run()
        call.check(got, flags)
        assert flags[:len(SIZES)].tolist() == [int(k == at[0]) for k in range(len(SIZES))]
    finally:
        call.close()


def test_many_one_pixel_levels_share_a_wave(hip_ctx):
    """70 levels of 1x1: a wave's lanes are 64 different records, alpha in every third of them; then a level that begins in the middle of a wave"""
    levels = [opaque_picture(1, 1, 300 + i) for i in range(70)] + [opaque_picture(9, 9, 399)]
    for lv in levels[::3]:
        lv[0, 0, 3] = 7
    call = Call(hip_ctx, levels, "bgra", "abgr")
    try:
        call.check(*call.run())
    finally:
        call.close()


def test_flags_are_cleared_by_the_call(hip_ctx):
    """a second call on the same flag words with opaque levels leaves none of the first call's flags behind"""
    call = Call(hip_ctx, levels_of(400, alpha_at=(3, 0, 0)), "rgba", None)
    try:
        call.check(*call.run())
        call.levels[3][0, 0, 3] = 255
        hip_ctx.memcpy_h2d(call.d_payload, np.concatenate([np.concatenate([np.full(GAP, 0x3C, np.uint8), lv.reshape(-1)]) for lv in call.levels]))
        got, flags = call.run()
        call.check(got, flags)
        assert not flags[:len(SIZES)].any()
    finally:
        call.close()


def test_zero_records_is_a_no_op(hip_ctx):
    call = Call(hip_ctx, [], "rgba", None)
    try:
        call.run()
        call.untouched()
    finally:
        call.close()


def test_refusals_name_themselves_and_write_nothing(hip_ctx):
    ctx = hip_ctx
    call = Call(ctx, levels_of(500), "rgba", None)
    try:
        good = call.records
        src, dst, w, h, sel = good[2]
        bad = [
            ([(src + 2, dst, w, h, sel)], "level 0: src_offset"),
            ([good[0], (src, dst + 1, w, h, sel)], "level 1: src_offset"),                 # one sentence for both offsets; it names the level
            ([(call.payload.size - 4 * w * h + 4, dst, w, h, sel)], "ends past payload_bytes"),
            ([(call.payload.size + 4, dst, 1, 1, sel)], "ends past payload_bytes"),
            ([(src, call.out_bytes - 4 * w * h + 4, w, h, sel)], "ends past out_bytes"),
            ([(src, dst, 0, h, sel)], "0 x 7 pixels (1..16384 each way)"),
            ([(src, dst, w, 0, sel)], "5 x 0 pixels (1..16384 each way)"),
            ([(src, dst, 16385, 1, sel)], "16385 x 1 pixels (1..16384 each way)"),
            ([(src, dst, 1, 16385, sel)], "1 x 16385 pixels (1..16384 each way)"),
            ([(src, dst, w, h, 0x04020100)], "selector entry above 3"),
        ]
        for records, match in bad:
            with pytest.raises(Exception, match="k_prepare_mip_levels failed: prepare_mip_levels: .*" + re.escape(match)):
                call.run(records)
            call.untouched()
        lib, arr = ctx.lib, (source.MipLevelRecord * 1)(source.MipLevelRecord(*good[0], 0))
        vp = C.c_void_p
        args = dict(payload=vp(call.d_payload), records=arr, out=vp(call.d_out), flags=vp(call.d_flags))
        for null in args:
            a = dict(args, **{null: None})
            assert not lib.k_prepare_mip_levels(ctx.h, a["payload"], call.payload.size, a["records"], 1, a["out"], call.out_bytes, a["flags"])
            assert "null pointer" in lib.last_error(ctx.h), null
        for odd in ("payload", "out", "flags"):
            a = dict(args, **{odd: vp(args[odd].value + 2)})
            assert not lib.k_prepare_mip_levels(ctx.h, a["payload"], call.payload.size, a["records"], 1, a["out"], call.out_bytes, a["flags"])
            assert "4-byte aligned" in lib.last_error(ctx.h), odd
        # more records than a file has slices: the count alone is refused, before any record is read
        assert not lib.k_prepare_mip_levels(ctx.h, args["payload"], call.payload.size, arr, source.MAX_SLICES + 1, args["out"], call.out_bytes, args["flags"])
        assert "more than the 16777215 slices of one file" in lib.last_error(ctx.h)
        call.untouched()
        call.check(*call.run())       # and the context still works
    finally:
        call.close()
