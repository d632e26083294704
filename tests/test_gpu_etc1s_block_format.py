"""-m gpu: the ETC1S block-format targets -- ASTC 4x4, EAC R11, EAC RG11 -- through bu_hip_k_transcode_etc1s_block_format* / bu_hip_k_transcode_etc1s_block_formats
and transcode.transcode_etc1s_block_format*, against the reference tool's bytes (tests/golden/etc1s_block_format_vectors.npz) and the CPU restatement
(tests/etc1s_block_format_helpers.py). Shapes: the fixtures' (1x1 to 8x6 blocks, the coverage image of 32x118), 1x1, 5x7, 9x5 and 16x4 blocks of a synthetic
state, and 3,000 random blocks."""
import ctypes as C

import numpy as np
import pytest

import etc1s_block_format_helpers as B
import etc1s_transcode_helpers as E
from basis_universal_amd import transcode as T

pytestmark = pytest.mark.gpu

NEW_TARGETS = [("astc", T.ASTC_4x4_RGBA, 16), ("r11", T.ETC2_EAC_R11, 8), ("rg11", T.ETC2_EAC_RG11, 16)]
OLD_TARGETS = [T.ETC1_RGB, T.ETC2_RGBA, T.BC1_RGB, T.BC7_RGBA, T.RGBA32, T.RGB565, T.BGR565, T.RGBA4444]
FILL = 0x5A


@pytest.fixture(scope="module")
def ctx():
    from basis_universal_amd import capi
    c = capi.Context(0)
    yield c
    c.close()


def _files():
    _, meta = B.golden()
    return [f["name"] for f in meta["files"]]


def _same(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.flatnonzero((got != want).any(1))
    assert bad.size == 0, (what, bad[:8], got[bad[:2]], want[bad[:2]])


@pytest.mark.parametrize("name", _files())
def test_every_target_and_golden_image_matches_the_reference_tool(ctx, name):
    """the one-image entry per image (host and resident output), the one-launch entry per file (host and resident output), and the file-level wrapper"""
    arrays, _ = B.golden()
    data = arrays["file_" + name]
    decoded = T.decode_etc1s_file(data)
    for suffix, target, unit in NEW_TARGETS:
        whole = T.transcode_etc1s_block_formats(ctx, data, target)
        layout, total = T.etc1s_block_format_layout(decoded["images"], target)
        d_all = ctx.alloc(total)
        try:
            assert T.transcode_etc1s_block_formats(ctx, data, target, out_device=d_all) == (layout, total)
            resident = ctx.download(d_all, (total,), np.uint8)
        finally:
            ctx.free(d_all)
        assert len(whole) == len(decoded["images"])
        for im, got_whole, place in zip(decoded["images"], whole, layout):
            what = (name, suffix, im["level"], im["layer"], im["face"])
            want = arrays[E.image_key(name, im["level"], im["layer"], im["face"]) + "_" + suffix]
            _same(T.transcode_etc1s_block_format_image(ctx, decoded, im, target), want, what + ("one image",))
            _same(got_whole, want, what + ("whole file",))
            _same(resident[place["offset"]:place["offset"] + place["nbytes"]].reshape(-1, unit), want, what + ("whole file, resident",))
            d_one = ctx.alloc(want.size)
            try:
                assert T.transcode_etc1s_block_format_image(ctx, decoded, im, target, out_device=d_one) is None
                _same(ctx.download(d_one, want.shape, np.uint8), want, what + ("one image, resident",))
            finally:
                ctx.free(d_one)
        im = decoded["images"][-1]
        _same(T.transcode_etc1s_block_format(ctx, data, target, level=im["level"], layer=im["layer"], face=im["face"]),
              arrays[E.image_key(name, im["level"], im["layer"], im["face"]) + "_" + suffix], (name, suffix, "file wrapper"))


@pytest.mark.parametrize("name", ["mip_basis", "cube_ktx2"])
def test_the_second_familys_targets_are_what_the_second_family_writes(ctx, name):
    arrays, _ = B.golden()
    data = arrays["file_" + name]
    decoded = T.decode_etc1s_file(data)
    for target in OLD_TARGETS:
        for filtering in ((True, False) if target == T.BC7_RGBA else (True,)):
            old_whole = T.transcode_etc1s_textures(ctx, data, target, chroma_filtering=filtering)
            new_whole = T.transcode_etc1s_block_formats(ctx, data, target, chroma_filtering=filtering)
            for im, a, b in zip(decoded["images"], old_whole, new_whole):
                assert a.shape == b.shape and a.dtype == b.dtype and (a == b).all(), (name, target, im["level"], "whole file")
                c = T.transcode_etc1s_block_format_image(ctx, decoded, im, target, chroma_filtering=filtering)
                assert c.shape == a.shape and (c == a).all(), (name, target, im["level"], "one image")


def test_device_built_astc_tables_equal_the_host_statement(ctx):
    t47, t255, unq = np.zeros(15360, np.uint32), np.zeros(15360, np.uint32), np.zeros(48, np.uint32)
    ctx.check(ctx.lib.etc1s_astc_tables(ctx.h, t47.ctypes.data_as(C.c_void_p), t255.ctypes.data_as(C.c_void_p), unq.ctypes.data_as(C.c_void_p)), "etc1s_astc_tables")
    t = B.tables()
    for got, want, what in ((t47, t.table47.reshape(-1), "0..47"), (t255, t.whole255.reshape(-1), "0..255"), (unq, np.array(t.unquant, np.uint32), "unquantised")):
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, (what, bad[:8], got[bad[:4]], want[bad[:4]])
    assert (t255.reshape(8, 32, 6, 10)[7, :, 0].max(1) >> 16 == 0xFFFF).all()   # the rows whose errors are scaled


# ---------------------------------------------------------------- a synthetic state: every route at every shape

def _state(seed, n_endpoints, n_selectors):
    """palettes in which every route of the ASTC conversion is common: a third of the endpoints grey, an eighth of the widest table; selectors of one to four values"""
    rng = np.random.default_rng(seed)
    ep = rng.integers(0, 32, (n_endpoints, 4)).astype(np.uint8)
    ep[:, 3] = rng.integers(0, 8, n_endpoints)
    grey = rng.random(n_endpoints) < 1 / 3
    ep[grey, 1] = ep[grey, 0]
    ep[grey, 2] = ep[grey, 0]
    ep[rng.random(n_endpoints) < 1 / 8, 3] = 7
    ep[0] = (31, 31, 31, 0)
    sets = [(s,) for s in range(4)] + [(a, b) for a in range(4) for b in range(a + 1, 4)] + [(0, 1, 2), (1, 2, 3), (0, 1, 3), (0, 2, 3), (0, 1, 2, 3)]
    sel = np.zeros((n_selectors, 16), np.uint32)
    for k in range(n_selectors):
        u = sets[k % len(sets)]
        sel[k] = rng.permutation(np.resize(np.array(u), 16)) if k >= len(sets) else np.resize(np.array(u), 16)
    return ep, E.selector_palette_u32(sel)


class _Resident:
    """palettes and index arrays on the device, and calls of the three entries over them with a filled, sentinel-guarded output"""
    GUARD = 64

    def __init__(self, ctx, ep, sel, ei, si):
        self.ctx, self.ep, self.sel, self.ei, self.si = ctx, np.ascontiguousarray(ep, np.uint8), np.ascontiguousarray(sel, np.uint32), ei.astype(np.uint16), si.astype(np.uint16)
        self.held = [ctx.upload(a) for a in (self.ep, self.sel, self.ei, self.si)]
        self.decoded = {"endpoint_palette": self.ep, "selector_palette": self.sel}

    def close(self):
        for p in self.held:
            self.ctx.free(p)

    def image(self, first, alpha_first, nbx, nby):
        n = nbx * nby
        take = lambda a, at: a[at:at + n].reshape(nby, nbx)   # noqa: E731
        return {"num_blocks_x": nbx, "num_blocks_y": nby, "width": nbx * 4, "height": nby * 4, "endpoint_indices": take(self.ei, first), "selector_indices": take(self.si, first),
                "alpha_endpoint_indices": None if alpha_first is None else take(self.ei, alpha_first),
                "alpha_selector_indices": None if alpha_first is None else take(self.si, alpha_first)}

    def one(self, fn, target, unit, first, alpha_first, bx, by, flags=0, **kw):
        """an image of bx x by blocks; kw replaces arguments of the call by name -> (return value, invalid count, the n x unit output, the guard bytes behind it)"""
        ctx, n = self.ctx, bx * by
        fill = np.full(n * unit + self.GUARD, FILL, np.uint8)
        d_out = ctx.upload(fill)
        try:
            at = lambda base, k: None if k is None else C.c_void_p(base + 2 * k)   # noqa: E731
            args = dict(ep=C.c_void_p(self.held[0]), n_ep=self.ep.shape[0], sel=C.c_void_p(self.held[1]), n_sel=self.sel.size, ei=at(self.held[2], first), si=at(self.held[3], first),
                        aei=at(self.held[2], alpha_first), asi=at(self.held[3], alpha_first), nbx=bx, nby=by, w=bx * 4, h=by * 4, target=target, out=C.c_void_p(d_out), pitch=0, rows=0,
                        flags=flags)
            args.update(kw)
            invalid = C.c_uint32(0xFFFF)
            tail = (C.byref(invalid),) if fn.endswith("_counted") else ()
            ok = getattr(ctx.lib, fn)(ctx.h, *[args[k] for k in ("ep", "n_ep", "sel", "n_sel", "ei", "si", "aei", "asi", "nbx", "nby", "w", "h", "target", "out", "pitch", "rows", "flags")],
                                      *tail)
            out = ctx.download(d_out, fill.shape, np.uint8)
            return ok, invalid.value, out[:n * unit].reshape(n, unit), out[n * unit:]
        finally:
            ctx.free(d_out)

    def many(self, target, unit, images, flags=0):
        """images: [(first, alpha_first, nbx, nby)] -> (return value, per-slice counts, [output per image], guard bytes)"""
        ctx = self.ctx
        recs, at = (T.TranscodeSlice * len(images))(), 0
        for k, (first, alpha_first, nbx, nby) in enumerate(images):
            recs[k] = T.TranscodeSlice(first, T.NO_ALPHA_SLICE if alpha_first is None else alpha_first, at, nbx, nby, nbx * 4, nby * 4, 0, 0)
            at += (nbx * nby * unit + 15) & ~15
        fill = np.full(at + self.GUARD, FILL, np.uint8)
        d_out = ctx.upload(fill)
        try:
            counts = (C.c_uint32 * len(images))(*([0xFFFF] * len(images)))
            ok = ctx.lib.k_transcode_etc1s_block_formats(ctx.h, C.c_void_p(self.held[0]), self.ep.shape[0], C.c_void_p(self.held[1]), self.sel.size, C.c_void_p(self.held[2]),
                                                         C.c_void_p(self.held[3]), self.ei.size, recs, len(images), target, flags, C.c_void_p(d_out), at, counts)
            out = ctx.download(d_out, fill.shape, np.uint8)
            return ok, list(counts), [out[r.out_offset:r.out_offset + r.num_blocks_x * r.num_blocks_y * unit].reshape(-1, unit) for r in recs], out[at:]
        finally:
            ctx.free(d_out)


SHAPES = [(1, 1), (5, 7), (9, 5), (16, 4)]   # one block; ragged against a 64-lane wave; lanes of one wave on both image edges; one wave spans four block rows


@pytest.fixture(scope="module")
def shapes_state(ctx):
    ep, sel = _state(7, 300, 150)
    rng = np.random.default_rng(8)
    total = 2 * sum(x * y for x, y in SHAPES)
    r = _Resident(ctx, ep, sel, rng.integers(0, ep.shape[0], total), rng.integers(0, sel.size, total))
    yield r
    r.close()


def test_small_shapes_through_the_one_image_entries(ctx, shapes_state):
    r, at = shapes_state, 0
    for nbx, nby in SHAPES:
        n = nbx * nby
        for alpha_first in (at + n, None):
            im = r.image(at, alpha_first, nbx, nby)
            for suffix, target, unit in NEW_TARGETS:
                want = B.blocks(r.decoded, im, target)
                for fn in ("k_transcode_etc1s_block_format_counted", "k_transcode_etc1s_block_format"):
                    ok, invalid, out, guard = r.one(fn, target, unit, at, alpha_first, nbx, nby)
                    assert ok == 1 and invalid in (0, 0xFFFF) and (guard == FILL).all(), (fn, suffix, nbx, nby, ctx.lib.last_error(ctx.h))
                    _same(out, want, (fn, suffix, nbx, nby, alpha_first is not None))
        at += 2 * n


def test_a_slice_table_of_images_of_different_sizes_with_and_without_alpha(ctx, shapes_state):
    r, at, images = shapes_state, 0, []
    for k, (nbx, nby) in enumerate(SHAPES):
        images.append((at, at + nbx * nby if k % 2 == 0 else None, nbx, nby))
        at += 2 * nbx * nby
    images.append((0, None, 1, 1))   # the first image's colour slice again, opaque this time
    for suffix, target, unit in NEW_TARGETS:
        ok, counts, outs, guard = r.many(target, unit, images)
        assert ok == 1 and counts == [0] * len(images) and (guard == FILL).all(), (suffix, ctx.lib.last_error(ctx.h))
        for (first, alpha_first, nbx, nby), out in zip(images, outs):
            _same(out, B.blocks(r.decoded, r.image(first, alpha_first, nbx, nby), target), (suffix, nbx, nby, alpha_first is not None))
        assert ctx.lib.etc1s_block_format_slice_extent(C.byref(T.TranscodeSlice(0, T.NO_ALPHA_SLICE, 0, 5, 7, 20, 28, 0, 0)), target) == 35 * unit
        assert ctx.lib.etc1s_block_format_output_bytes(5, 7, 20, 28, target, 0, 0) == 35 * unit


def test_random_state_over_large_palettes_takes_every_route(ctx):
    """3,000 blocks (60 x 50) over 6,000 endpoints and 4,000 selectors, colour and alpha slice, against the restatement; every route and sub-route often enough"""
    ep, sel = _state(21, 6000, 4000)
    rng = np.random.default_rng(22)
    nbx, nby = 60, 50
    n = nbx * nby
    ei, si = rng.integers(0, ep.shape[0], 2 * n), rng.integers(0, sel.size, 2 * n)
    white = rng.random(n) < 0.15
    ei[n:][white] = 0
    si[n:][white] = 3   # a constant alpha of 255 for the RGB route: endpoint 0 is white under table 0, selector 3 its highest selector alone
    r = _Resident(ctx, ep, sel, ei, si)
    try:
        im = r.image(0, n, nbx, nby)
        routes, details = {}, []
        want = B.blocks(r.decoded, im, B.ASTC_4x4_RGBA, routes, details)
        assert all(routes.get(k, 0) >= 30 for k in B.ROUTES), routes
        sub = {}
        for route, d in details:
            if route == "rgba":
                for k in ("color", "alpha"):
                    sub[k, d[k]] = sub.get((k, d[k]), 0) + 1
                sub["swapped", d["swapped"]] = sub.get(("swapped", d["swapped"]), 0) + 1
        assert all(sub.get((k, v), 0) >= 5 for k in ("color", "alpha") for v in ("solid", "outlier", "lookup")) and sub.get(("swapped", True), 0) >= 5, sub
        ok, invalid, out, guard = r.one("k_transcode_etc1s_block_format_counted", T.ASTC_4x4_RGBA, 16, 0, n, nbx, nby)
        assert ok == 1 and invalid == 0 and (guard == FILL).all()
        _same(out, want, "astc")
        for suffix, target, unit in NEW_TARGETS[1:]:
            ok, invalid, out, guard = r.one("k_transcode_etc1s_block_format_counted", target, unit, 0, n, nbx, nby)
            assert ok == 1 and invalid == 0 and (guard == FILL).all()
            _same(out, B.blocks(r.decoded, im, target), suffix)
        ok, counts, outs, guard = r.many(T.ASTC_4x4_RGBA, 16, [(0, n, nbx, nby), (n, None, nbx, nby)])
        assert ok == 1 and counts == [0, 0] and (guard == FILL).all()
        _same(outs[0], want, "astc, slice table")
        _same(outs[1], B.blocks(r.decoded, r.image(n, None, nbx, nby), B.ASTC_4x4_RGBA), "astc, the alpha slice as an opaque image")
    finally:
        r.close()


def test_indices_past_a_palette_are_zero_blocks_and_counted(ctx, shapes_state):
    """One index planted at n_endpoints in the colour slice and one at n_selectors in the alpha slice, the smallest values that are wrong. The block is zero and counted,
    every other block is what it was, the bytes behind the output keep their fill; the checked entry refuses before it launches. EAC R11 does not read the alpha slice."""
    r = shapes_state
    nbx, nby = SHAPES[1]
    first = 2 * SHAPES[0][0] * SHAPES[0][1]
    n = nbx * nby
    clean_ei, clean_si = r.ei.copy(), r.si.copy()
    try:
        for suffix, target, unit in NEW_TARGETS:
            _, _, clean, _ = r.one("k_transcode_etc1s_block_format_counted", target, unit, first, first + n, nbx, nby)
            for plant, where in (("colour", first + 7), ("alpha", first + n + n - 1)):
                ei, si = clean_ei.copy(), clean_si.copy()
                if plant == "colour":
                    ei[where] = r.ep.shape[0]
                else:
                    si[where] = r.sel.size
                planted = _Resident(ctx, r.ep, r.sel, ei, si)
                try:
                    block = where - first if plant == "colour" else where - first - n
                    reads = plant == "colour" or target != T.ETC2_EAC_R11
                    ok, invalid, out, guard = planted.one("k_transcode_etc1s_block_format_counted", target, unit, first, first + n, nbx, nby)
                    assert ok == 1 and invalid == (1 if reads else 0) and (guard == FILL).all(), (suffix, plant, invalid)
                    keep = np.setdiff1d(np.arange(n), [block] if reads else [])
                    _same(out[keep], clean[keep], (suffix, plant))
                    if reads:
                        assert (out[block] == 0).all(), (suffix, plant)
                    ok, _, out, guard = planted.one("k_transcode_etc1s_block_format", target, unit, first, first + n, nbx, nby)
                    if reads:
                        assert ok == 0 and "past their palette" in ctx.lib.last_error(ctx.h) and (out == FILL).all() and (guard == FILL).all(), (suffix, plant)
                    else:
                        assert ok == 1
                    ok, counts, outs, guard = planted.many(target, unit, [(0, 1, 1, 1), (first, first + n, nbx, nby)])
                    assert ok == 1 and counts == [0, 1 if reads else 0] and (guard == FILL).all(), (suffix, plant, counts)
                    _same(outs[1][keep], clean[keep], (suffix, plant, "slice table"))
                finally:
                    planted.close()
    finally:
        assert (r.ei == clean_ei).all() and (r.si == clean_si).all()


def test_refusals_come_before_any_launch(ctx, shapes_state):
    r, lib = shapes_state, ctx.lib
    nbx, nby = SHAPES[1]
    first = 2
    n = nbx * nby

    def refused(text, target=T.ASTC_4x4_RGBA, **kw):
        for fn in ("k_transcode_etc1s_block_format", "k_transcode_etc1s_block_format_counted"):
            ok, _, out, guard = r.one(fn, target, 16, first, first + n, nbx, nby, **kw)
            assert ok == 0 and text in lib.last_error(ctx.h), (text, lib.last_error(ctx.h))
            assert (out == FILL).all() and (guard == FILL).all(), text

    refused("null device pointer", ep=None)
    refused("null device pointer", out=None)
    refused("an alpha slice needs both of its index arrays", asi=None)
    refused("palettes of 0 endpoints", n_ep=0)
    refused("transcode_etc1s_block_format: 20 x 28 pixels do not fit 0 x 7 blocks", nbx=0)
    refused("bits 0x20 are not supported (supported: 64, cDecodeFlagsNoETC1SChromaFiltering)", flags=32)
    refused("bits 0x4 are not supported", flags=64 | 4)   # cDecodeFlagsTranscodeAlphaDataToOpaqueFormats
    supported = "(supported: ETC1_RGB (0), ETC2_RGBA (1), BC1_RGB (2), BC7_RGBA (6), ASTC_4x4_RGBA (10), RGBA32 (13), RGB565 (14), BGR565 (15), RGBA4444 (16), ETC2_EAC_R11 (20), ETC2_EAC_RG11 (21))"
    for target, name in ((3, "BC3_RGBA"), (4, "BC4_R"), (5, "BC5_RG"), (8, "PVRTC1_4_RGB"), (9, "PVRTC1_4_RGBA"), (11, "ATC_RGB"), (12, "ATC_RGBA"), (17, "FXT1_RGB"),
                         (18, "PVRTC2_4_RGB"), (19, "PVRTC2_4_RGBA")):
        refused(f"transcode_etc1s_block_format: target {target} ({name}) is not supported {supported}", target=target)
        assert lib.etc1s_block_format_output_bytes(2, 2, 0, 0, target, 0, 0) == 0
    refused("target 22 (", target=22)
    # the first two families still refuse the new targets, by their own lists
    for target, name in ((10, "ASTC_4x4_RGBA"), (20, "ETC2_EAC_R11"), (21, "ETC2_EAC_RG11")):
        ok, _, out, _ = r.one("k_transcode_etc1s_image_counted", target, 16, first, first + n, nbx, nby)
        assert ok == 0 and f"transcode_etc1s_image: target {target} ({name}) is not supported (supported: ETC1_RGB (0), ETC2_RGBA (1), BC1_RGB (2), BC7_RGBA (6), RGBA32" in \
            lib.last_error(ctx.h) and (out == FILL).all()
        assert lib.etc1s_image_output_bytes(2, 2, 0, 0, target, 0, 0) == 0 and lib.etc1s_transcode_output_bytes(2, 2, 0, 0, target, 0, 0) == 0
    # a 16-byte target wants a 16-byte aligned output
    d_out = ctx.upload(np.full(n * 16 + 16, FILL, np.uint8))
    try:
        for fn in ("k_transcode_etc1s_block_format", "k_transcode_etc1s_block_format_counted"):
            ok, _, _, _ = r.one(fn, T.ASTC_4x4_RGBA, 16, first, first + n, nbx, nby, out=C.c_void_p(d_out + 8))
            assert ok == 0 and "16-byte aligned" in lib.last_error(ctx.h)
        assert (ctx.download(d_out, (n * 16 + 16,), np.uint8) == FILL).all()
    finally:
        ctx.free(d_out)
    # the one-launch entry: the same target list and flags
    rec = (T.TranscodeSlice * 1)(T.TranscodeSlice(first, first + n, 0, nbx, nby, nbx * 4, nby * 4, 0, 0))
    counts = (C.c_uint32 * 1)()
    d_out = ctx.upload(np.full(n * 16, FILL, np.uint8))
    try:
        def formats(target, flags, records=rec):
            return lib.k_transcode_etc1s_block_formats(ctx.h, C.c_void_p(r.held[0]), r.ep.shape[0], C.c_void_p(r.held[1]), r.sel.size, C.c_void_p(r.held[2]), C.c_void_p(r.held[3]),
                                                       r.ei.size, records, 1, target, flags, C.c_void_p(d_out), n * 16, counts)
        assert formats(3, 0) == 0 and "transcode_etc1s_block_format: target 3 (BC3_RGBA)" in lib.last_error(ctx.h)
        assert formats(11, 0) == 0 and "ATC_RGB" in lib.last_error(ctx.h)
        assert formats(T.ASTC_4x4_RGBA, 2) == 0 and "bits 0x2 are not supported" in lib.last_error(ctx.h)
        pitched = (T.TranscodeSlice * 1)(T.TranscodeSlice(first, first + n, 0, nbx, nby, nbx * 4, nby * 4, 64, 0))
        assert formats(T.ASTC_4x4_RGBA, 0, pitched) == 0 and "block target (ASTC_4x4_RGBA)" in lib.last_error(ctx.h)
        assert lib.etc1s_block_format_slice_extent(rec, T.ASTC_4x4_RGBA) == n * 16 and lib.etc1s_block_format_slice_extent(rec, 3) == 0
        assert lib.etc1s_image_slice_extent(rec, T.ASTC_4x4_RGBA) == 0
        assert (ctx.download(d_out, (n * 16,), np.uint8) == FILL).all()
        assert formats(T.ASTC_4x4_RGBA, 0) == 1 and counts[0] == 0   # and a good call goes through
    finally:
        ctx.free(d_out)
