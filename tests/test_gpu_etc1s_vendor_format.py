"""-m gpu: the ETC1S vendor-format targets -- ATC RGB, FXT1, PVRTC2 4bpp RGB / RGBA -- through bu_hip_k_transcode_etc1s_vendor_format* / bu_hip_k_transcode_etc1s_vendor_formats
and transcode.transcode_etc1s_vendor_format*, against the reference tool's bytes (tests/golden/etc1s_vendor_format_vectors.npz) and the CPU restatement
(tests/etc1s_vendor_format_helpers.py). Shapes: the fixtures' (1x1 to 8x6 blocks, the coverage image of 31x58 with its alpha slice, an image one block wide), and 1x1, 5x7, 9x5, 16x4
and 30x20 blocks of a synthetic state: odd and even rows of FXT1, one block, lanes of one wave on both image edges, more than one workgroup."""
import ctypes as C

import numpy as np
import pytest

import etc1s_transcode_helpers as E
import etc1s_vendor_format_helpers as V
from basis_universal_amd import transcode as T

pytestmark = pytest.mark.gpu

NEW_TARGETS = [("atc", T.ATC_RGB, 8), ("fxt1", T.FXT1_RGB, 16), ("pvrtc2", T.PVRTC2_4_RGB, 8), ("pvrtc2a", T.PVRTC2_4_RGBA, 8)]
OLD_TARGETS = [T.ETC1_RGB, T.ETC2_RGBA, T.BC1_RGB, T.BC7_RGBA, T.ASTC_4x4_RGBA, T.RGBA32, T.RGB565, T.BGR565, T.RGBA4444, T.ETC2_EAC_R11, T.ETC2_EAC_RG11]
FILL = 0x5A
SUPPORTED = ("(supported: ETC1_RGB (0), ETC2_RGBA (1), BC1_RGB (2), BC7_RGBA (6), ASTC_4x4_RGBA (10), ATC_RGB (11), RGBA32 (13), RGB565 (14), BGR565 (15), RGBA4444 (16), "
             "FXT1_RGB (17), PVRTC2_4_RGB (18), PVRTC2_4_RGBA (19), ETC2_EAC_R11 (20), ETC2_EAC_RG11 (21))")


@pytest.fixture(scope="module")
def ctx():
    from basis_universal_amd import capi
    c = capi.Context(0)
    yield c
    c.close()


def _files():
    _, meta = V.golden()
    return [f["name"] for f in meta["files"]]


def _same(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.flatnonzero((got != want).any(1))
    assert bad.size == 0, (what, bad[:8], got[bad[:2]], want[bad[:2]])


def _out_blocks(target, nbx, nby):
    return (nbx + 1) // 2 * nby if target == T.FXT1_RGB else nbx * nby


@pytest.mark.parametrize("name", _files())
def test_every_target_and_golden_image_matches_the_reference_tool(ctx, name):
    """the one-image entry per image (host and resident output), the one-launch entry per file (host and resident output), and the file-level wrapper"""
    arrays, _ = V.golden()
    data = arrays["file_" + name]
    decoded = T.decode_etc1s_file(data)
    for suffix, target, unit in NEW_TARGETS:
        whole = T.transcode_etc1s_vendor_formats(ctx, data, target)
        layout, total = T.etc1s_vendor_format_layout(decoded["images"], target)
        d_all = ctx.alloc(total)
        try:
            assert T.transcode_etc1s_vendor_formats(ctx, data, target, out_device=d_all) == (layout, total)
            resident = ctx.download(d_all, (total,), np.uint8)
        finally:
            ctx.free(d_all)
        assert len(whole) == len(decoded["images"])
        for im, got_whole, place in zip(decoded["images"], whole, layout):
            what = (name, suffix, im["level"], im["layer"], im["face"])
            want = arrays[E.image_key(name, im["level"], im["layer"], im["face"]) + "_" + suffix]
            _same(T.transcode_etc1s_vendor_format_image(ctx, decoded, im, target), want, what + ("one image",))
            _same(got_whole, want, what + ("whole file",))
            _same(resident[place["offset"]:place["offset"] + place["nbytes"]].reshape(-1, unit), want, what + ("whole file, resident",))
        im = decoded["images"][-1]
        _same(T.transcode_etc1s_vendor_format(ctx, data, target, level=im["level"], layer=im["layer"], face=im["face"]),
              arrays[E.image_key(name, im["level"], im["layer"], im["face"]) + "_" + suffix], (name, suffix, "file wrapper"))


def test_the_third_familys_targets_are_what_the_third_family_writes(ctx):
    arrays, _ = V.golden()
    data = arrays["file_mip_basis"]
    decoded = T.decode_etc1s_file(data)
    for target in OLD_TARGETS:
        old_whole = T.transcode_etc1s_block_formats(ctx, data, target)
        new_whole = T.transcode_etc1s_vendor_formats(ctx, data, target)
        for im, a, b in zip(decoded["images"], old_whole, new_whole):
            assert a.shape == b.shape and a.dtype == b.dtype and (a == b).all(), (target, im["level"], "whole file")
        im = decoded["images"][1]
        c = T.transcode_etc1s_vendor_format_image(ctx, decoded, im, target)
        assert c.shape == old_whole[1].shape and (c == old_whole[1]).all(), (target, "one image")


def test_device_built_atc_tables_equal_the_host_statement(ctx):
    got = [np.zeros(15360, np.uint32) for _ in range(3)]
    ctx.check(ctx.lib.etc1s_atc_tables(ctx.h, *[g.ctypes.data_as(C.c_void_p) for g in got]), "etc1s_atc_tables")
    t = V.tables()
    for g, which in zip(got, ("55", "56", "45")):
        bad = np.flatnonzero(g != t.atc[which].reshape(-1))
        assert bad.size == 0, (which, bad[:8], g[bad[:4]], t.atc[which].reshape(-1)[bad[:4]])
    assert ctx.lib.etc1s_atc_tables(ctx.h, got[0].ctypes.data_as(C.c_void_p), None, got[2].ctypes.data_as(C.c_void_p)) == 0 and "null pointer" in ctx.lib.last_error(ctx.h)


# ---------------------------------------------------------------- a synthetic state: every route at every shape

def _state(seed, n_endpoints, n_selectors):
    """palettes in which every route is common: an eighth of the endpoints of the widest table, some black and white; selectors of one to four values"""
    rng = np.random.default_rng(seed)
    ep = rng.integers(0, 32, (n_endpoints, 4)).astype(np.uint8)
    ep[:, 3] = rng.integers(0, 8, n_endpoints)
    ep[rng.random(n_endpoints) < 1 / 8, 3] = 7
    mid = rng.random(n_endpoints) < 0.35   # mid-range bases under narrow tables: nothing clamps, which is what PVRTC2 RGBA's 2D route wants
    ep[mid, :3] = rng.integers(10, 22, (int(mid.sum()), 3))
    ep[mid, 3] = rng.integers(0, 3, int(mid.sum()))
    ep[rng.random(n_endpoints) < 1 / 6, 3] = 7   # the outlier route needs the widest table
    grey = rng.random(n_endpoints) < 0.4   # alpha reads green alone: grey entries make a constant colour meet a constant alpha
    ep[grey, 0] = ep[grey, 2] = ep[grey, 1]
    ep[0], ep[1] = (31, 31, 31, 0), (0, 0, 0, 0)
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

    def image(self, first, nbx, nby, alpha_first=None):
        n = nbx * nby
        take = lambda a, at: None if at is None else a[at:at + n].reshape(nby, nbx)   # noqa: E731
        return {"num_blocks_x": nbx, "num_blocks_y": nby, "width": nbx * 4, "height": nby * 4, "endpoint_indices": take(self.ei, first), "selector_indices": take(self.si, first),
                "alpha_endpoint_indices": take(self.ei, alpha_first), "alpha_selector_indices": take(self.si, alpha_first)}

    def one(self, fn, target, unit, first, bx, by, flags=0, alpha_first=None, **kw):
        """an image of bx x by blocks; kw replaces arguments of the call by name -> (return value, invalid count, the output blocks, the guard bytes behind them)"""
        ctx, n = self.ctx, _out_blocks(target, bx, by)
        fill = np.full(n * unit + self.GUARD, FILL, np.uint8)
        d_out = ctx.upload(fill)
        try:
            args = dict(ep=C.c_void_p(self.held[0]), n_ep=self.ep.shape[0], sel=C.c_void_p(self.held[1]), n_sel=self.sel.size, ei=C.c_void_p(self.held[2] + 2 * first),
                        si=C.c_void_p(self.held[3] + 2 * first), aei=None if alpha_first is None else C.c_void_p(self.held[2] + 2 * alpha_first),
                        asi=None if alpha_first is None else C.c_void_p(self.held[3] + 2 * alpha_first), nbx=bx, nby=by, w=bx * 4, h=by * 4, target=target, out=C.c_void_p(d_out), pitch=0, rows=0, flags=flags)
            args.update(kw)
            invalid = C.c_uint32(0xFFFF)
            tail = (C.byref(invalid),) if fn.endswith("_counted") else ()
            ok = getattr(ctx.lib, fn)(ctx.h, *[args[k] for k in ("ep", "n_ep", "sel", "n_sel", "ei", "si", "aei", "asi", "nbx", "nby", "w", "h", "target", "out", "pitch", "rows", "flags")],
                                      *tail)
            out = ctx.download(d_out, fill.shape, np.uint8)
            return ok, invalid.value, out[:n * unit].reshape(n, unit), out[n * unit:]
        finally:
            ctx.free(d_out)

    def many(self, target, unit, images, flags=0, short_by=0):
        """images: [(first, nbx, nby) or (first, nbx, nby, alpha_first)] -> (return value, per-slice counts, [output per image], guard bytes); short_by: out_bytes is that much less than the table needs"""
        ctx = self.ctx
        recs, at = (T.TranscodeSlice * len(images))(), 0
        for k, (first, nbx, nby, *alpha) in enumerate(images):
            recs[k] = T.TranscodeSlice(first, alpha[0] if alpha and alpha[0] is not None else T.NO_ALPHA_SLICE, at, nbx, nby, nbx * 4, nby * 4, 0, 0)
            at += (_out_blocks(target, nbx, nby) * unit + 15) & ~15
        fill = np.full(at + self.GUARD, FILL, np.uint8)
        d_out = ctx.upload(fill)
        try:
            counts = (C.c_uint32 * len(images))(*([0xFFFF] * len(images)))
            ok = ctx.lib.k_transcode_etc1s_vendor_formats(ctx.h, C.c_void_p(self.held[0]), self.ep.shape[0], C.c_void_p(self.held[1]), self.sel.size, C.c_void_p(self.held[2]),
                                                          C.c_void_p(self.held[3]), self.ei.size, recs, len(images), target, flags, C.c_void_p(d_out), at - short_by, counts)
            out = ctx.download(d_out, fill.shape, np.uint8)
            return ok, list(counts), [out[r.out_offset:r.out_offset + _out_blocks(target, r.num_blocks_x, r.num_blocks_y) * unit].reshape(-1, unit) for r in recs], out[at:]
        finally:
            ctx.free(d_out)


SHAPES = [(1, 1), (5, 7), (9, 5), (16, 4), (30, 20)]   # one block; odd rows ragged against a wave; both image edges in one wave; even rows; three workgroups


@pytest.fixture(scope="module")
def shapes_state(ctx):
    ep, sel = _state(7, 300, 150)
    rng = np.random.default_rng(8)
    total = 2 * sum(x * y for x, y in SHAPES)   # every image's colour slice, then as many indices for its alpha slice
    r = _Resident(ctx, ep, sel, rng.integers(0, ep.shape[0], total), rng.integers(0, sel.size, total))
    yield r
    r.close()


def test_small_shapes_through_all_three_entries_equal_the_restatement(ctx, shapes_state):
    r, at, images = shapes_state, 0, []
    routes = {}
    for nbx, nby in SHAPES:
        n = nbx * nby
        for alpha_first in (at + n, None):
            im = r.image(at, nbx, nby, alpha_first)
            for suffix, target, unit in NEW_TARGETS:
                details = []
                want = V.blocks(r.decoded, im, target, details)
                for route, d in details:
                    key = (suffix, d["gate"] if suffix == "pvrtc2a" and alpha_first is not None else route)
                    routes[key] = routes.get(key, 0) + 1
                for fn in ("k_transcode_etc1s_vendor_format_counted", "k_transcode_etc1s_vendor_format"):
                    ok, invalid, out, guard = r.one(fn, target, unit, at, nbx, nby, alpha_first=alpha_first)
                    assert ok == 1 and invalid in (0, 0xFFFF) and (guard == FILL).all(), (fn, suffix, nbx, nby, ctx.lib.last_error(ctx.h))
                    _same(out, want, (fn, suffix, nbx, nby, alpha_first is not None))
                assert ctx.lib.etc1s_vendor_format_output_bytes(nbx, nby, 0, 0, target, 0, 0) == want.size
                assert ctx.lib.etc1s_vendor_format_slice_extent(C.byref(T.TranscodeSlice(0, T.NO_ALPHA_SLICE, 0, nbx, nby, 0, 0, 0, 0)), target) == want.size
        images.append((at, nbx, nby, at + n if len(images) % 2 == 0 else None))
        at += 2 * n
    assert all(routes.get((s, k), 0) >= 10 for s, _, _ in NEW_TARGETS[:3] for k in V.ROUTES), routes
    assert all(routes.get(("pvrtc2a", g), 0) >= 5 for g in ("solid_colour", "constant_alpha", "pca4d", "pca4d_swapped", "pca2d", "pca2d_flipped")), routes
    images.append((0, 1, 1))   # the first image again, opaque this time
    for suffix, target, unit in NEW_TARGETS:
        ok, counts, outs, guard = r.many(target, unit, images)
        assert ok == 1 and counts == [0] * len(images) and (guard == FILL).all(), (suffix, ctx.lib.last_error(ctx.h))
        for (first, nbx, nby, *alpha), out in zip(images, outs):
            _same(out, V.blocks(r.decoded, r.image(first, nbx, nby, alpha[0] if alpha else None), target), (suffix, nbx, nby, "slice table"))
        # out_bytes ends where the table's last record begins (each record is rounded up to 16 bytes): refused, nothing written
        ok, _, outs, guard = r.many(target, unit, images, short_by=16)
        assert ok == 0 and "ends past out_bytes" in ctx.lib.last_error(ctx.h) and all((o == FILL).all() for o in outs) and (guard == FILL).all(), suffix


def _alpha_planted(ctx, r, where):
    ei, si = r.ei.copy(), r.si.copy()
    for at, kind in where:
        if kind == "e":
            ei[at] = r.ep.shape[0]
        else:
            si[at] = r.sel.size
    return _Resident(ctx, r.ep, r.sel, ei, si)


def test_indices_past_a_palette_are_zero_blocks_and_counted(ctx, shapes_state):
    """One endpoint index planted at n_endpoints in a left half and one selector index at n_selectors in the last block of an odd row (a lone left half); for a third
    state, both halves of one FXT1 block; and in the alpha arrays an endpoint and a selector index in two more blocks: the smallest values that are wrong. The output
    block is zero and the source blocks counted, every other block is what it was, the bytes behind the output keep their fill; the checked entry refuses before it
    launches. Only PVRTC2 RGBA reads the alpha arrays: for the other three a bad alpha index changes nothing."""
    r = shapes_state
    nbx, nby = SHAPES[1]
    first = 2 * SHAPES[0][0] * SHAPES[0][1]
    n = nbx * nby
    plants = {"endpoint": [(first + 7, "e")], "selector, lone half": [(first + 2 * nbx - 1, "s")], "both halves": [(first + 10, "e"), (first + 11, "s")],
              "alpha": [(first + n + 20, "e"), (first + n + 33, "s")]}
    for suffix, target, unit in NEW_TARGETS:
        _, _, clean, _ = r.one("k_transcode_etc1s_vendor_format_counted", target, unit, first, nbx, nby, alpha_first=first + n)
        for plant, where in plants.items():
            if plant == "alpha" and target != T.PVRTC2_4_RGBA:
                planted = _alpha_planted(ctx, r, where)
                try:
                    ok, invalid, out, guard = planted.one("k_transcode_etc1s_vendor_format_counted", target, unit, first, nbx, nby, alpha_first=first + n)
                    assert ok == 1 and invalid == 0 and (guard == FILL).all() and (out == clean).all(), (suffix, plant)
                    assert planted.one("k_transcode_etc1s_vendor_format", target, unit, first, nbx, nby, alpha_first=first + n)[0] == 1
                finally:
                    planted.close()
                continue
            ei, si = r.ei.copy(), r.si.copy()
            for at, kind in where:
                if kind == "e":
                    ei[at] = r.ep.shape[0]
                else:
                    si[at] = r.sel.size
            local = [(at - first) % n for at, _ in where]
            zero = sorted({(k // nbx) * ((nbx + 1) // 2) + (k % nbx) // 2 for k in local} if target == T.FXT1_RGB else set(local))
            planted = _Resident(ctx, r.ep, r.sel, ei, si)
            try:
                ok, invalid, out, guard = planted.one("k_transcode_etc1s_vendor_format_counted", target, unit, first, nbx, nby, alpha_first=first + n)
                assert ok == 1 and invalid == len(where) and (guard == FILL).all(), (suffix, plant, invalid)
                keep = np.setdiff1d(np.arange(out.shape[0]), zero)
                _same(out[keep], clean[keep], (suffix, plant))
                assert (out[zero] == 0).all() and not (clean[zero] == 0).all(1).any(), (suffix, plant)
                ok, _, out, guard = planted.one("k_transcode_etc1s_vendor_format", target, unit, first, nbx, nby, alpha_first=first + n)
                assert ok == 0 and "past their palette" in ctx.lib.last_error(ctx.h) and (out == FILL).all() and (guard == FILL).all(), (suffix, plant)
                ok, counts, outs, guard = planted.many(target, unit, [(0, 1, 1), (first, nbx, nby, first + n)])
                assert ok == 1 and counts == [0, len(where)] and (guard == FILL).all(), (suffix, plant, counts)
                _same(outs[1][keep], clean[keep], (suffix, plant, "slice table"))
                assert (outs[1][zero] == 0).all()
            finally:
                planted.close()


def test_refusals_name_the_target_and_come_before_any_launch(ctx, shapes_state):
    r, lib = shapes_state, ctx.lib
    nbx, nby = SHAPES[1]
    first, n = 1, nbx * nby

    def refused(text, target=T.ATC_RGB, unit=8, **kw):
        for fn in ("k_transcode_etc1s_vendor_format", "k_transcode_etc1s_vendor_format_counted"):
            ok, _, out, guard = r.one(fn, target, unit, first, nbx, nby, **kw)
            assert ok == 0 and text in lib.last_error(ctx.h), (text, lib.last_error(ctx.h))
            assert (out == FILL).all() and (guard == FILL).all(), text

    for suffix, target, unit in NEW_TARGETS:
        refused("null device pointer", target, unit, ep=None)
        refused("null device pointer", target, unit, out=None)
        refused("palettes of 0 endpoints", target, unit, n_ep=0)
        refused("transcode_etc1s_vendor_format: 20 x 28 pixels do not fit 0 x 7 blocks", target, unit, nbx=0)
        refused("bits 0x20 are not supported (supported: 64, cDecodeFlagsNoETC1SChromaFiltering)", target, unit, flags=32)
    refused("an alpha slice needs both of its index arrays", T.PVRTC2_4_RGBA, 8, aei=C.c_void_p(r.held[2]))
    refused("an alpha slice needs both of its index arrays", T.PVRTC2_4_RGBA, 8, asi=C.c_void_p(r.held[3]))
    refused("transcode_etc1s_vendor_format: row pitch 8 is less than the width 20", T.RGBA32, 8, pitch=8)
    bc4 = ": it needs the ETC1S -> BC4 look-up, which could not be restated as a search "
    for target, name, why in ((3, "BC3_RGBA", bc4), (4, "BC4_R", bc4), (5, "BC5_RG", bc4),
                              (12, "ATC_RGBA", ": its first half is a BC4 block, and the ETC1S -> BC4 look-up could not be restated as a search "),
                              (8, "PVRTC1_4_RGB", " "), (9, "PVRTC1_4_RGBA", " ")):
        refused(f"transcode_etc1s_vendor_format: target {target} ({name}) is not supported{why}{SUPPORTED}", target=target)
        assert lib.etc1s_vendor_format_output_bytes(2, 2, 0, 0, target, 0, 0) == 0
    refused("target 22 (", target=22)
    # FXT1 is a 16-byte target: a 16-byte aligned output
    d_out = ctx.upload(np.full(n * 16 + 16, FILL, np.uint8))
    try:
        for fn in ("k_transcode_etc1s_vendor_format", "k_transcode_etc1s_vendor_format_counted"):
            ok, _, _, _ = r.one(fn, T.FXT1_RGB, 16, first, nbx, nby, out=C.c_void_p(d_out + 8))
            assert ok == 0 and "16-byte aligned" in lib.last_error(ctx.h)
        assert (ctx.download(d_out, (n * 16 + 16,), np.uint8) == FILL).all()
    finally:
        ctx.free(d_out)
    # the one-launch entry: the same target list and flags
    rec = (T.TranscodeSlice * 1)(T.TranscodeSlice(first, T.NO_ALPHA_SLICE, 0, nbx, nby, nbx * 4, nby * 4, 0, 0))
    counts = (C.c_uint32 * 1)()
    d_out = ctx.upload(np.full(n * 16, FILL, np.uint8))
    try:
        def formats(target, flags, records=rec, n_records=1):
            return lib.k_transcode_etc1s_vendor_formats(ctx.h, C.c_void_p(r.held[0]), r.ep.shape[0], C.c_void_p(r.held[1]), r.sel.size, C.c_void_p(r.held[2]), C.c_void_p(r.held[3]),
                                                        r.ei.size, records, n_records, target, flags, C.c_void_p(d_out), n * 16, counts)
        assert formats(12, 0) == 0 and "transcode_etc1s_vendor_format: target 12 (ATC_RGBA) is not supported: its first half is a BC4 block" in lib.last_error(ctx.h)
        assert formats(T.FXT1_RGB, 2) == 0 and "bits 0x2 are not supported" in lib.last_error(ctx.h)
        assert formats(T.FXT1_RGB, 0, rec, 0) == 0 and "no slices" in lib.last_error(ctx.h)
        assert formats(T.FXT1_RGB, 0, None) == 0 and "null pointer" in lib.last_error(ctx.h)
        pitched = (T.TranscodeSlice * 1)(T.TranscodeSlice(first, T.NO_ALPHA_SLICE, 0, nbx, nby, nbx * 4, nby * 4, 64, 0))
        assert formats(T.FXT1_RGB, 0, pitched) == 0 and "block target (FXT1_RGB)" in lib.last_error(ctx.h)
        assert lib.etc1s_vendor_format_slice_extent(rec, T.FXT1_RGB) == 21 * 16 and lib.etc1s_vendor_format_slice_extent(rec, 12) == 0
        assert lib.etc1s_block_format_slice_extent(rec, T.FXT1_RGB) == 0
        assert (ctx.download(d_out, (n * 16,), np.uint8) == FILL).all()
        assert formats(T.FXT1_RGB, 0) == 1 and counts[0] == 0   # and a good call goes through
    finally:
        ctx.free(d_out)
    # the three earlier families still refuse the new targets, by their own lists
    for target, name in ((11, "ATC_RGB"), (17, "FXT1_RGB"), (18, "PVRTC2_4_RGB"), (19, "PVRTC2_4_RGBA")):
        for fn, who in (("k_transcode_etc1s_counted", "transcode_etc1s"), ("k_transcode_etc1s_image_counted", "transcode_etc1s_image"),
                        ("k_transcode_etc1s_block_format_counted", "transcode_etc1s_block_format")):
            fill = np.full(n * 16, FILL, np.uint8)
            d = ctx.upload(fill)
            try:
                invalid = C.c_uint32(0)
                head = (ctx.h, C.c_void_p(r.held[0]), r.ep.shape[0], C.c_void_p(r.held[1]), r.sel.size, C.c_void_p(r.held[2]), C.c_void_p(r.held[3]), None, None, nbx, nby, 0, 0, target,
                        C.c_void_p(d), 0, 0)
                ok = getattr(lib, fn)(*head, *(() if who == "transcode_etc1s" else (0,)), C.byref(invalid))
                assert ok == 0 and f"{who}: target {target} ({name}) is not supported (supported: ETC1_RGB (0)," in lib.last_error(ctx.h), lib.last_error(ctx.h)
                assert (ctx.download(d, fill.shape, np.uint8) == FILL).all()
            finally:
                ctx.free(d)
