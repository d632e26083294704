"""-m gpu: the ETC1S texture targets -- ETC2 RGBA and BC7 RGBA with the reference's chroma filter -- through bu_hip_k_transcode_etc1s_image* /
bu_hip_k_transcode_etc1s_images and transcode.transcode_etc1s_texture*, against the reference tool's bytes (tests/golden/etc1s_texture_vectors.npz). Every shape is a
fixture shape: 1x1 to 16x16 blocks, and the coverage image of 32x234."""
import ctypes as C

import numpy as np
import pytest

import etc1s_texture_helpers as X
import etc1s_transcode_helpers as E
from basis_universal_amd import transcode as T

pytestmark = pytest.mark.gpu

CONFIGS = [("etc2", T.ETC2_RGBA, True), ("bc7", T.BC7_RGBA, True), ("bc7nf", T.BC7_RGBA, False)]   # npz suffix, target, chroma filtering
OLD_TARGETS = [T.ETC1_RGB, T.BC1_RGB, T.RGBA32, T.RGB565, T.BGR565, T.RGBA4444]


@pytest.fixture(scope="module")
def ctx():
    from basis_universal_amd import capi
    c = capi.Context(0)
    yield c
    c.close()


def _files():
    _, meta = X.golden()
    return [f["name"] for f in meta["files"]]


def _same(got, want, what):
    bad = np.flatnonzero((got != want).any(1))
    assert got.shape == want.shape and bad.size == 0, (what, bad[:8], got[bad[:2]], want[bad[:2]])


@pytest.mark.parametrize("name", _files())
def test_every_target_and_golden_image_matches_the_reference_tool(ctx, name):
    """the one-image entry per image, the one-launch entry per file, and the file-level wrapper on the first image: all three the tool's bytes"""
    arrays, _ = X.golden()
    data = arrays["file_" + name]
    decoded = T.decode_etc1s_file(data)
    for suffix, target, filtering in CONFIGS:
        whole = T.transcode_etc1s_textures(ctx, data, target, chroma_filtering=filtering)
        assert len(whole) == len(decoded["images"])
        for im, got_whole in zip(decoded["images"], whole):
            want = arrays[E.image_key(name, im["level"], im["layer"], im["face"]) + "_" + suffix]
            _same(T.transcode_etc1s_texture_image(ctx, decoded, im, target, chroma_filtering=filtering), want, (name, suffix, im["level"], "one image"))
            _same(got_whole, want, (name, suffix, im["level"], "whole file"))
        im = decoded["images"][0]
        _same(T.transcode_etc1s_texture(ctx, data, target, level=im["level"], layer=im["layer"], face=im["face"], chroma_filtering=filtering),
              arrays[E.image_key(name, im["level"], im["layer"], im["face"]) + "_" + suffix], (name, suffix, "file wrapper"))


@pytest.mark.parametrize("name", ["mip_basis", "cube_ktx2"])
def test_the_six_first_targets_are_what_the_first_family_writes(ctx, name):
    arrays, _ = X.golden()
    data = arrays["file_" + name]
    decoded = T.decode_etc1s_file(data)
    for target in OLD_TARGETS:
        old_whole, new_whole = T.transcode_etc1s_file_images(ctx, data, target), T.transcode_etc1s_textures(ctx, data, target)
        for im, a, b in zip(decoded["images"], old_whole, new_whole):
            assert a.shape == b.shape and a.dtype == b.dtype and (a == b).all(), (name, target, im["level"], "whole file")
            c = T.transcode_etc1s_texture_image(ctx, decoded, im, target)
            assert c.shape == a.shape and (c == T.transcode_etc1s_image(ctx, decoded, im, target)).all() and (c == a).all(), (name, target, im["level"], "one image")


def test_device_built_bc7_tables_equal_the_host_statement(ctx):
    table, mid = np.zeros(15360, np.uint32), np.zeros(128, np.uint32)
    ctx.check(ctx.lib.etc1s_bc7_color_table(ctx.h, table.ctypes.data_as(C.c_void_p), mid.ctypes.data_as(C.c_void_p)), "etc1s_bc7_color_table")
    want = X.tables()["bc7_color"].reshape(-1)
    bad = np.flatnonzero(table != want)
    assert bad.size == 0, (bad[:8], table[bad[:4]], want[bad[:4]])
    assert (mid.view(np.float32) == np.array(X.MIDPOINTS, np.float32)).all()


def test_an_opaque_file_gets_the_opaque_alpha_halves(ctx):
    arrays, _ = X.golden()
    data = arrays["file_opaque_ktx2"]
    etc2 = T.transcode_etc1s_texture(ctx, data, T.ETC2_RGBA)
    assert (etc2[:, :8] == np.array(X.OPAQUE_EAC_A8, np.uint8)).all()
    assert (etc2[:, 8:] == T.transcode_etc1s_file(ctx, data, T.ETC1_RGB)).all()
    for filtering in (True, False):
        texels = X.decode_bc7_mode5(T.transcode_etc1s_texture(ctx, data, T.BC7_RGBA, chroma_filtering=filtering))
        assert (texels[..., 3] == 255).all()


class _Counted:
    """bu_hip_k_transcode_etc1s_image_counted over one golden image with indices of the caller's choosing"""

    def __init__(self, ctx, name):
        arrays, _ = X.golden()
        self.ctx, self.arrays, self.name = ctx, arrays, name
        self.dec = T.decode_etc1s_file(arrays["file_" + name])
        self.im = self.dec["images"][0]
        self.nbx, self.nby = self.im["num_blocks_x"], self.im["num_blocks_y"]
        self.ep = np.ascontiguousarray(self.dec["endpoint_palette"], np.uint8)
        self.sel = np.ascontiguousarray(self.dec["selector_palette"], np.uint32)

    def golden(self, suffix):
        return self.arrays[E.image_key(self.name, 0, 0, 0) + "_" + suffix]

    def indices(self):
        im = self.im
        alpha = [im[k].reshape(-1).copy() for k in ("alpha_endpoint_indices", "alpha_selector_indices")] if im["alpha_endpoint_indices"] is not None else [None, None]
        return [im["endpoint_indices"].reshape(-1).copy(), im["selector_indices"].reshape(-1).copy()] + alpha

    def run(self, target, flags, idx, fn="k_transcode_etc1s_image_counted"):
        ctx, n = self.ctx, self.nbx * self.nby
        held = [ctx.upload(a) for a in [self.ep, self.sel] + [np.ascontiguousarray(a, np.uint16) for a in idx if a is not None]]
        fill = np.full((n, 16), 0x5A, np.uint8)
        d_out = ctx.upload(fill)
        try:
            alpha = (C.c_void_p(held[4]), C.c_void_p(held[5])) if idx[2] is not None else (None, None)
            invalid = C.c_uint32(0xFFFF)
            tail = (flags, C.byref(invalid)) if fn.endswith("_counted") else (flags,)
            ok = getattr(ctx.lib, fn)(ctx.h, C.c_void_p(held[0]), self.ep.shape[0], C.c_void_p(held[1]), self.sel.size, C.c_void_p(held[2]), C.c_void_p(held[3]), *alpha,
                                      self.nbx, self.nby, self.im["width"], self.im["height"], target, C.c_void_p(d_out), 0, 0, *tail)
            return ok, invalid.value, ctx.download(d_out, fill.shape, np.uint8)
        finally:
            for p in held + [d_out]:
                ctx.free(p)


def test_planted_colour_selector_and_alpha_indices_are_zero_blocks_and_counted(ctx):
    """Indices planted at n_endpoints / n_selectors, the smallest values that are wrong. A planted block is zero and counted; every other block is the golden -- for
    the colour slice shown where no block reads a neighbour (ETC2, BC7 without the filter), for the alpha slice also under the filter, which never reads it."""
    c = _Counted(ctx, "alpha_basis")
    n = c.nbx * c.nby
    for suffix, target, flags, plant in (("etc2", T.ETC2_RGBA, 0, "colour"), ("bc7nf", T.BC7_RGBA, 64, "colour"), ("etc2", T.ETC2_RGBA, 0, "alpha"), ("bc7", T.BC7_RGBA, 0, "alpha")):
        idx = c.indices()
        base = 0 if plant == "colour" else 2
        idx[base][7] = c.ep.shape[0]
        idx[base + 1][n - 1] = c.sel.size
        ok, invalid, out = c.run(target, flags, idx)
        assert ok == 1 and invalid == 2, (suffix, plant, invalid)
        assert (out[[7, n - 1]] == 0).all(), (suffix, plant)
        keep = np.setdiff1d(np.arange(n), [7, n - 1])
        _same(out[keep], c.golden(suffix)[keep], (suffix, plant))
        # the checked entry refuses the same indices before it launches: the output keeps its fill
        ok, _, out = c.run(target, flags, idx, "k_transcode_etc1s_image")
        assert ok == 0 and "past their palette" in ctx.lib.last_error(ctx.h) and (out == 0x5A).all(), (suffix, plant)
    ok, invalid, out = c.run(T.BC7_RGBA, 0, c.indices())
    assert ok == 1 and invalid == 0
    _same(out, c.golden("bc7"), "unplanted")


def test_a_filtered_blocks_neighbour_past_the_palette_contributes_the_centre(ctx):
    """chroma36: the index of a block next to blocks the filter re-encodes is planted at n_endpoints. That block is zero and counted; its neighbours come out as the
    documented rule says -- the bad neighbour counts as the centre's own entry -- which the CPU restatement states; blocks that do not touch it are the golden."""
    c = _Counted(ctx, "chroma36_basis")
    n, nbx = c.nbx * c.nby, c.nbx
    k = 1 * nbx + 4   # an inner block of the saturated half: all eight neighbours exist
    idx = c.indices()
    idx[0][k] = c.ep.shape[0]
    ok, invalid, out = c.run(T.BC7_RGBA, 0, idx)
    assert ok == 1 and invalid == 1 and (out[k] == 0).all()
    neighbour_ok = np.ones((c.nby, nbx), bool)
    neighbour_ok[k // nbx, k % nbx] = False
    routes = {}
    want = X.bc7_blocks(c.dec, c.im, True, routes, neighbour_ok)
    want[k] = 0
    _same(out, want, "the neighbour rule")
    touching = [k + dy * nbx + dx for dy in (-1, 0, 1) for dx in (-1, 0, 1)]
    far = np.setdiff1d(np.arange(n), touching)
    _same(out[far], c.golden("bc7")[far], "blocks away from the planted one")
    assert routes.get("pca", 0) + routes.get("simple", 0) >= 8


def test_resident_bc7_output_goes_through_unpack_blocks(ctx):
    """a byte-order check: the blocks left on the device by the one-launch entry unpack, texel for texel, to what the golden blocks decode to by the format definition"""
    arrays, _ = X.golden()
    data = arrays["file_alpha_ktx2"]
    images = T.read_etc1s_file(data)["images"]
    layout, total = T.etc1s_texture_layout(images, T.BC7_RGBA)
    d_out = ctx.alloc(total)
    try:
        assert T.transcode_etc1s_textures(ctx, data, T.BC7_RGBA, out_device=d_out) == (layout, total)
        im = images[0]
        got = T.unpack_blocks(ctx, d_out + layout[0]["offset"], im["num_blocks_x"], im["num_blocks_y"], T.BC7_RGBA)
    finally:
        ctx.free(d_out)
    texels = X.decode_bc7_mode5(arrays[E.image_key("alpha_ktx2", 0, 0, 0) + "_bc7"])
    nbx, nby = im["num_blocks_x"], im["num_blocks_y"]
    want = texels.reshape(nby, nbx, 4, 4, 4).transpose(0, 2, 1, 3, 4).reshape(nby * 4, nbx * 4, 4)
    assert (got == want).all()
    assert len(np.unique(want[..., 3])) > 8   # the alpha ramp is there


def test_refusals_come_before_any_launch(ctx):
    c = _Counted(ctx, "alpha_basis")
    lib, n = ctx.lib, c.nbx * c.nby
    idx = c.indices()

    def refused(text, **kw):
        args = dict(ep=C.c_void_p(held[0]), n_ep=c.ep.shape[0], sel=C.c_void_p(held[1]), n_sel=c.sel.size, ei=C.c_void_p(held[2]), si=C.c_void_p(held[3]), aei=C.c_void_p(held[4]),
                    asi=C.c_void_p(held[5]), nbx=c.nbx, nby=c.nby, w=c.im["width"], h=c.im["height"], target=T.BC7_RGBA, out=C.c_void_p(d_out), pitch=0, rows=0, flags=0)
        args.update(kw)
        invalid = C.c_uint32(0)
        for fn, tail in ((lib.k_transcode_etc1s_image, ()), (lib.k_transcode_etc1s_image_counted, (C.byref(invalid),))):
            assert fn(ctx.h, *[args[k] for k in ("ep", "n_ep", "sel", "n_sel", "ei", "si", "aei", "asi", "nbx", "nby", "w", "h", "target", "out", "pitch", "rows", "flags")], *tail) == 0
            assert text in lib.last_error(ctx.h), (text, lib.last_error(ctx.h))
        assert (ctx.download(d_out, (n, 16), np.uint8) == 0x5A).all(), text

    held = [ctx.upload(a) for a in [c.ep, c.sel] + [np.ascontiguousarray(a, np.uint16) for a in idx]]
    d_out = ctx.upload(np.full((n, 16), 0x5A, np.uint8))
    try:
        refused("null device pointer", ep=None)
        refused("null device pointer", si=None)
        refused("null device pointer", out=None)
        refused("an alpha slice needs both of its index arrays", asi=None)
        refused("an alpha slice needs both of its index arrays", aei=None)
        refused("palettes of 0 endpoints", n_ep=0)
        refused("transcode_etc1s_image: 32 x 24 pixels do not fit 0 x 6 blocks", nbx=0)
        refused("pixels do not fit 8 x 6 blocks", w=c.nbx * 4 + 1)
        refused("blocks is too many", nby=16385)
        refused("row pitch 8 is less than the width 32", pitch=8)
        refused("bits 0x20 are not supported (supported: 64, cDecodeFlagsNoETC1SChromaFiltering)", flags=32)
        refused("bits 0x1 are not supported", flags=65)
        refused("16-byte aligned", out=C.c_void_p(d_out + 8))
        for target, name in ((3, "BC3_RGBA"), (4, "BC4_R"), (5, "BC5_RG"), (10, "ASTC_4x4_RGBA")):
            refused(f"target {target} ({name}) is not supported (supported: ETC1_RGB (0), ETC2_RGBA (1), BC1_RGB (2), BC7_RGBA (6)", target=target)
            assert lib.etc1s_image_output_bytes(2, 2, 0, 0, target, 0, 0) == 0
        assert lib.etc1s_image_output_bytes(2, 2, 0, 0, T.BC7_RGBA, 0, 0) == 64 and lib.etc1s_image_output_bytes(2, 2, 0, 0, T.ETC1_RGB, 0, 0) == 32
        # the one-launch entry: the same target list and flags, and a pitch is refused for a block target
        rec = (T.TranscodeSlice * 1)(T.TranscodeSlice(0, T.NO_ALPHA_SLICE, 0, c.nbx, c.nby, c.im["width"], c.im["height"], 0, 0))
        counts = (C.c_uint32 * 1)()

        def images(target, flags, records=rec):
            return lib.k_transcode_etc1s_images(ctx.h, C.c_void_p(held[0]), c.ep.shape[0], C.c_void_p(held[1]), c.sel.size, C.c_void_p(held[2]), C.c_void_p(held[3]), n, records, 1,
                                                target, flags, C.c_void_p(d_out), n * 16, counts)
        assert images(3, 0) == 0 and "BC3_RGBA" in lib.last_error(ctx.h)
        assert images(T.BC7_RGBA, 2) == 0 and "bits 0x2 are not supported" in lib.last_error(ctx.h)
        pitched = (T.TranscodeSlice * 1)(T.TranscodeSlice(0, T.NO_ALPHA_SLICE, 0, c.nbx, c.nby, c.im["width"], c.im["height"], 64, 0))
        assert images(T.BC7_RGBA, 0, pitched) == 0 and "block target (BC7_RGBA)" in lib.last_error(ctx.h)
        assert lib.etc1s_image_slice_extent(rec, T.BC7_RGBA) == n * 16 and lib.etc1s_image_slice_extent(rec, 3) == 0 and lib.transcode_slice_extent(rec, T.BC7_RGBA, 1) == 0
        assert (ctx.download(d_out, (n, 16), np.uint8) == 0x5A).all()
        assert images(T.BC7_RGBA, 64) == 1 and counts[0] == 0   # and a good call goes through: the colour slice alone, unfiltered
    finally:
        for p in held + [d_out]:
            ctx.free(p)
