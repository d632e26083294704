"""The device half of reading ETC1S files back: csrc/etc1s_transcode_kernels.hip through bu_hip_k_transcode_etc1s and basis_universal_amd.transcode, against the
reference tool's bytes (tests/golden/etc1s_transcode_vectors.npz)."""
import ctypes as C

import numpy as np
import pytest

import etc1s_transcode_helpers as E
from basis_universal_amd import transcode as T

pytestmark = pytest.mark.gpu

BLOCK_TARGETS = {"etc1": T.ETC1_RGB, "bc1": T.BC1_RGB}
PIXEL_TARGETS = [T.RGBA32, T.RGB565, T.BGR565, T.RGBA4444]


@pytest.fixture(scope="module")
def ctx():
    from basis_universal_amd import capi
    c = capi.Context(0)
    yield c
    c.close()


def _files():
    _, meta = E.golden()
    return [f["name"] for f in meta["files"]]


@pytest.mark.parametrize("name", _files())
def test_every_golden_file_and_target_matches_the_reference_tool(ctx, name):
    """Shapes in here: 1x1 block (mip levels 3, 4), 5x7 pixels = 2x2 ragged blocks (mip level 2), 16x16 blocks (o64), the alpha file, array layers, cubemap faces."""
    arrays, meta = E.golden()
    entry = next(f for f in meta["files"] if f["name"] == name)
    data = arrays["file_" + name]
    decoded = T.decode_etc1s_file(data)
    assert [[im["level"], im["layer"], im["face"], im["width"], im["height"]] for im in decoded["images"]] == entry["images"]
    for im in decoded["images"]:
        key = E.image_key(name, im["level"], im["layer"], im["face"])
        for short, target in BLOCK_TARGETS.items():
            got = T.transcode_etc1s_file(ctx, data, target, level=im["level"], layer=im["layer"], face=im["face"])
            bad = np.flatnonzero((got != arrays[f"{key}_{short}"]).any(1))
            assert bad.size == 0, (key, short, bad[:8], got[bad[:2]], arrays[f"{key}_{short}"][bad[:2]])
        want = E.expected_rgba(arrays, key, im["width"], im["height"], im["num_blocks_x"], im["num_blocks_y"])
        for target in PIXEL_TARGETS:
            got = T.transcode_etc1s_image(ctx, decoded, im, target)
            exp = want if target == T.RGBA32 else E.pack_pixels(want, target)
            assert got.shape == exp.shape and (got == exp).all(), (key, target)


def test_device_built_bc1_tables_equal_the_generator(ctx):
    """The two ETC1S -> BC1 endpoint tables the library computes on the device against tools/gen_etc1s_transcode_tables.py's host computation, entry for entry."""
    import pathlib
    import sys
    sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent.parent / "tools"))
    import gen_etc1s_transcode_tables as G
    t5, t6 = np.zeros(15360, np.uint32), np.zeros(15360, np.uint32)
    ctx.check(ctx.lib.etc1s_bc1_endpoint_tables(ctx.h, t5.ctypes.data_as(C.c_void_p), t6.ctypes.data_as(C.c_void_p)), "etc1s_bc1_endpoint_tables")
    for got, bits in ((t5, 5), (t6, 6)):
        want = G.endpoint_table(bits)
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, (bits, bad[:8], got[bad[:4]], want[bad[:4]])


def test_coverage_member_is_complete_and_bc1_is_exact(ctx):
    arrays, meta = E.golden()
    cov = meta["coverage"]
    # every (intensity table, selector range, mapping) a colour can reach (the generator searches all 32^3 colours per table and range) occurs in the file
    assert cov["table_range_mapping_covered"] == cov["table_range_mapping_reachable"] >= 200 and cov["solid_blocks"] >= 100 and cov["two_colour_blocks"] >= 4, cov
    data = arrays["file_coverage_basis"]
    got = T.transcode_etc1s_file(ctx, data, T.BC1_RGB)
    want = arrays[E.image_key("coverage_basis", 0, 0, 0) + "_bc1"]
    assert got.shape == want.shape == (cov["blocks"], 8)
    bad = np.flatnonzero((got != want).any(1))
    assert bad.size == 0, (bad[:8], got[bad[:2]], want[bad[:2]])


def _synthetic(w, h, seed, alpha):
    """a decoded-file dictionary with one image of random indices over small random palettes"""
    rng = np.random.default_rng(seed)
    nbx, nby = (w + 3) // 4, (h + 3) // 4
    ep = np.stack([rng.integers(0, 32, 40), rng.integers(0, 32, 40), rng.integers(0, 32, 40), rng.integers(0, 8, 40)], 1).astype(np.uint8)
    sel = rng.integers(0, 4, (50, 16)).astype(np.uint8)
    idx = lambda k: rng.integers(0, k, (nby, nbx)).astype(np.uint16)
    im = {"level": 0, "layer": 0, "face": 0, "width": w, "height": h, "num_blocks_x": nbx, "num_blocks_y": nby, "endpoint_indices": idx(40), "selector_indices": idx(50),
          "alpha_endpoint_indices": idx(40) if alpha else None, "alpha_selector_indices": idx(50) if alpha else None}
    return {"endpoint_palette": ep, "selector_palette": E.selector_palette_u32(sel)}, im, ep, sel


def _expected_pixels(ep, sel, im):
    """RGBA by the format definition from palettes and indices (no reference needed: the block-level meaning is pinned by the golden test above)"""
    def plane(ei, si):
        e = ep[ei.reshape(-1)].astype(int)
        base = (e[:, :3] << 3) | (e[:, :3] >> 2)
        px = np.clip(base[:, None, :] + E.INTEN[e[:, 3]][np.arange(e.shape[0])[:, None], sel[si.reshape(-1)]][:, :, None], 0, 255)
        nby, nbx = ei.shape
        return px.reshape(nby, nbx, 4, 4, 3).transpose(0, 2, 1, 3, 4).reshape(nby * 4, nbx * 4, 3).astype(np.uint8)
    rgb = plane(im["endpoint_indices"], im["selector_indices"])
    a = plane(im["alpha_endpoint_indices"], im["alpha_selector_indices"])[..., 1] if im["alpha_endpoint_indices"] is not None else np.full(rgb.shape[:2], 255, np.uint8)
    return np.concatenate([rgb, a[..., None]], 2)[:im["height"], :im["width"]]


@pytest.mark.parametrize("w,h", [(4, 4), (5, 7), (255, 257)])
@pytest.mark.parametrize("alpha", [False, True])
def test_pixel_targets_crop_and_respect_a_padded_pitch(ctx, w, h, alpha):
    decoded, im, ep, sel = _synthetic(w, h, 100 + w, alpha)
    want = _expected_pixels(ep, sel, im)
    for target in PIXEL_TARGETS:
        exp = want if target == T.RGBA32 else E.pack_pixels(want, target)
        got = T.transcode_etc1s_image(ctx, decoded, im, target)
        assert (got == exp).all(), (target, "tight")
        # a caller-owned raster with 3 pixels of padding per row and 2 rows below: the padding keeps its fill
        pitch, rows = w + 3, h + 2
        dtype, shape = (np.uint8, (rows, pitch, 4)) if target == T.RGBA32 else (np.uint16, (rows, pitch))
        fill = np.full(shape, 0xA5 if target == T.RGBA32 else 0xA5A5, dtype)
        d_out = ctx.upload(fill)
        try:
            assert T.transcode_etc1s_image(ctx, decoded, im, target, out_device=d_out, out_row_pitch=pitch, out_rows=rows) is None
            out = ctx.download(d_out, shape, dtype)
        finally:
            ctx.free(d_out)
        assert (out[:h, :w] == exp).all(), (target, "padded")
        assert (out[:h, w:] == fill[:h, w:]).all() and (out[h:] == fill[h:]).all(), (target, "padding touched")


def _call(ctx, fn, ep, sel_u32, ei, si, nbx, nby, target, d_out, extra=()):
    held = [ctx.upload(ep), ctx.upload(sel_u32), ctx.upload(ei), ctx.upload(si)]
    try:
        return fn(ctx.h, C.c_void_p(held[0]), ep.shape[0], C.c_void_p(held[1]), sel_u32.size, C.c_void_p(held[2]), C.c_void_p(held[3]), None, None, nbx, nby, 0, 0, target,
                  C.c_void_p(d_out), 0, 0, *extra)
    finally:
        for p in held:
            ctx.free(p)


def test_an_index_past_the_palette_is_an_error_before_the_launch_and_a_counted_zero_block_on_the_device(ctx):
    decoded, im, ep, sel = _synthetic(32, 16, 5, False)
    sel_u32 = decoded["selector_palette"]
    nbx, nby = 8, 4
    good_e, good_s = im["endpoint_indices"].reshape(-1).copy(), im["selector_indices"].reshape(-1).copy()
    want = T.transcode_etc1s_image(ctx, decoded, im, T.BC1_RGB)
    bad_e, bad_s = good_e.copy(), good_s.copy()
    bad_e[5] = ep.shape[0]          # first index past the endpoint palette
    bad_s[20] = 65535               # far past the selector palette
    fill = np.full((nbx * nby, 8), 0x5A, np.uint8)
    d_out = ctx.upload(fill)
    try:
        # the checked entry point: error return, the output untouched (the transcode was never launched)
        assert _call(ctx, ctx.lib.k_transcode_etc1s, ep, sel_u32, bad_e, bad_s, nbx, nby, T.BC1_RGB, d_out) == 0
        assert "past their palette" in ctx.lib.last_error(ctx.h)
        assert (ctx.download(d_out, fill.shape, np.uint8) == fill).all()
        # the counted entry point: the two blocks are zero-filled and counted, every other block is what it is without them
        invalid = C.c_uint32(0)
        assert _call(ctx, ctx.lib.k_transcode_etc1s_counted, ep, sel_u32, bad_e, bad_s, nbx, nby, T.BC1_RGB, d_out, (C.byref(invalid),)) == 1
        out = ctx.download(d_out, fill.shape, np.uint8)
        assert invalid.value == 2 and (out[[5, 20]] == 0).all()
        keep = np.setdiff1d(np.arange(nbx * nby), [5, 20])
        assert (out[keep] == want[keep]).all()
        # and with good indices the checked entry point gives the same blocks
        assert _call(ctx, ctx.lib.k_transcode_etc1s, ep, sel_u32, good_e, good_s, nbx, nby, T.BC1_RGB, d_out) == 1
        assert (ctx.download(d_out, fill.shape, np.uint8) == want).all()
    finally:
        ctx.free(d_out)


@pytest.mark.parametrize("target,name", [(1, "ETC2_RGBA"), (3, "BC3_RGBA"), (4, "BC4_R"), (5, "BC5_RG"), (6, "BC7_RGBA"), (8, "PVRTC1_4_RGB"), (10, "ASTC_4x4_RGBA"), (11, "ATC_RGB"),
                                         (17, "FXT1_RGB"), (18, "PVRTC2_4_RGB"), (20, "ETC2_EAC_R11"), (99, "unknown")])
def test_unsupported_targets_are_refused_by_name(ctx, target, name):
    arrays, _ = E.golden()
    with pytest.raises(ValueError, match=f"{name}.*not supported"):
        T.transcode_etc1s_file(ctx, arrays["file_o20_q128_basis"], target)
    decoded, im, ep, sel = _synthetic(8, 8, 1, False)
    d_out = ctx.alloc(1024)
    try:
        assert _call(ctx, ctx.lib.k_transcode_etc1s, ep, decoded["selector_palette"], im["endpoint_indices"].reshape(-1), im["selector_indices"].reshape(-1), 2, 2, target, d_out) == 0
        assert "not supported" in ctx.lib.last_error(ctx.h) and name in ctx.lib.last_error(ctx.h)
    finally:
        ctx.free(d_out)
    assert ctx.lib.etc1s_transcode_output_bytes(2, 2, 0, 0, target, 0, 0) == 0


@pytest.mark.parametrize("image", ["k03", "k23"])
def test_end_to_end_compress_then_transcode(ctx, image):
    """compress(uastc=False, quality=128) on two whole Kodak goldens (768x512), then transcode_etc1s_file(RGBA32): bit-identical to the encoder's own final blocks.
    The frontend and backend are driven here exactly as compress() drives them, the file's bytes must equal compress()'s, and the expected pixels are the backend's final
    endpoint and selector of every block (after its RDO moved some) looked up in the frontend's codebooks and decoded by the format definition -- nothing on that side
    goes through the file reader. The RGB PSNR against the source is printed, not asserted."""
    import pathlib
    from basis_universal_amd.backend import Etc1sBackend, default_params
    from basis_universal_amd.compress import compress
    from basis_universal_amd.etc1s import Etc1sFrontend, quality_to_clusters
    import helpers
    rgb = np.load(pathlib.Path(E.GOLDEN).parent / "kodak24.npz")[image]
    img = np.ascontiguousarray(np.concatenate([rgb, np.full(rgb.shape[:2] + (1,), 255, np.uint8)], 2))
    h, w = img.shape[:2]
    nbx, nby = w // 4, h // 4
    data = compress(ctx, img, uastc=False, quality=128)
    max_ep, max_sel = quality_to_clusters(128, nbx * nby)
    fe = Etc1sFrontend(ctx)
    fe.init(helpers.to_pixel_blocks(img), max_ep, max_sel, 1, True)
    fe.compress()
    ept, selt = default_params(128, 1)
    be = Etc1sBackend.from_frontend(fe, [(0, nbx, nby, w, h, 0, 0, 0)], ept, selt, 1)
    be.encode()
    assert bytes(be.basis_file()) == bytes(data), "the frontend and backend driven here do not write compress()'s file"
    final = be.get("encoder_blocks", dtype=np.uint32).reshape(-1, 4)
    ep = fe.get("endpoint_cluster_etc_params").reshape(-1, 16)[:, :4].copy()
    sel = E.selectors_of_etc_blocks(fe.get("optimized_cluster_selectors").reshape(-1, 8))
    moved = int((final[:, 0] != fe.get("block_endpoint_clusters_indices", np.uint32)).sum()), int((final[:, 2] != fe.get("block_selector_cluster_index", np.uint32)).sum())
    be.close()
    fe.close()
    state = {"width": w, "height": h, "endpoint_indices": final[:, 0].reshape(nby, nbx), "selector_indices": final[:, 2].reshape(nby, nbx), "alpha_endpoint_indices": None,
             "alpha_selector_indices": None}
    want = _expected_pixels(ep, sel, state)
    info = T.read_etc1s_file(data)
    assert (info["width"], info["height"], info["has_alpha_slices"]) == (w, h, False)
    got = T.transcode_etc1s_file(ctx, data, T.RGBA32)
    bad = np.argwhere((got != want).any(2))
    assert got.shape == want.shape and bad.size == 0, (len(bad), bad[:4])
    mse = ((got[..., :3].astype(np.float64) - img[..., :3]) ** 2).mean()
    print(f"{image} {w}x{h} q128: {moved[0]} endpoint and {moved[1]} selector indices moved by the backend; RGB PSNR of the file read back {10 * np.log10(255 ** 2 / mse):.2f} dB")
