"""-m gpu: the ETC1S -> BC7 chroma filter and the mode-5 encoder under it at every comparison they branch on, against the reference's bytes
(tests/golden/etc1s_bc7_filter_vectors.npz; the cases are etc1s_bc7_filter_cases.py's). The encoder alone through the diagnostic entry bu_hip_k_bc7_mode5_tiles, the
filter through the three transcoding entries. Shapes: at most 8,192 tiles per call and images of at most 32x32 blocks."""
import ctypes as C

import numpy as np
import pytest

import etc1s_bc7_filter_cases as K
import etc1s_texture_helpers as X
import etc1s_transcode_helpers as E
import helpers
from basis_universal_amd import transcode as T

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from basis_universal_amd import capi
    c = capi.Context(0)
    yield c
    c.close()


def _states():
    return [s["name"] for s in K.golden()[1]["states"]]


def _same_tiles(got, want, tiles, what):
    bad = np.flatnonzero((got != want).any(1))
    routes = K.restate_tiles(tiles[bad[:4]])[1] if bad.size else []
    assert got.shape == want.shape and bad.size == 0, (what, bad.size, bad[:8], "routes of the first", routes, got[bad[:2]], want[bad[:2]])


def _same_blocks(got, want, decoded, im, what):
    """equality of bytes; a failure names the filter's routes (by the CPU restatement) of the first differing blocks"""
    bad = np.flatnonzero((got != want).any(1))
    if bad.size:
        route_of = []
        X.bc7_blocks(decoded, im, True, None, None, route_of)
        raise AssertionError((what, bad.size, bad[:8], "routes", [route_of[k] for k in bad[:8]], got[bad[:2]], want[bad[:2]]))
    assert got.shape == want.shape


# ---------------------------------------------------------------- the encoder alone

@pytest.mark.parametrize("name", K.TILE_CLASSES)
def test_the_device_encodes_every_tile_as_the_reference_does(ctx, name):
    tiles = K.tiles_of(name)
    _same_tiles(T.bc7_mode5_tiles(ctx, tiles), K.golden()[0]["tiles_" + name], tiles, name)


def test_tile_counts_around_a_wave_and_a_workgroup_write_their_blocks_and_nothing_else(ctx):
    tiles, want = K.tile_classes()["random"], K.golden()[0]["tiles_random"]
    d_tiles = ctx.upload(tiles[:257])
    try:
        for n in (1, 63, 64, 65, 257):
            fill = np.full((n + 2, 16), 0xA5, np.uint8)
            d_out = ctx.upload(fill)
            try:
                ctx.check(ctx.lib.k_bc7_mode5_tiles(ctx.h, C.c_void_p(d_tiles), n, C.c_void_p(d_out + 16)), "bc7_mode5_tiles")
                got = ctx.download(d_out, fill.shape, np.uint8)
            finally:
                ctx.free(d_out)
            assert (got[0] == 0xA5).all() and (got[-1] == 0xA5).all(), n
            _same_tiles(got[1:-1], want[:n], tiles[:n], n)
    finally:
        ctx.free(d_tiles)


def test_the_tile_entry_refuses_before_any_launch(ctx):
    lib = ctx.lib
    fill = np.full((8, 16), 0x5A, np.uint8)
    d_tiles, d_out = ctx.upload(K.tile_classes()["random"][:8]), ctx.upload(fill)
    try:
        for text, tiles, n, out in (("null device pointer", None, 4, d_out), ("null device pointer", d_tiles, 4, None), ("16-byte aligned", d_tiles + 8, 4, d_out),
                                    ("16-byte aligned", d_tiles, 4, d_out + 8), ("tiles is too many (at most 2^30)", d_tiles, 2 ** 30 + 1, d_out)):
            assert lib.k_bc7_mode5_tiles(ctx.h, C.c_void_p(tiles), n, C.c_void_p(out)) == 0
            assert "bc7_mode5_tiles" in lib.last_error(ctx.h) and text in lib.last_error(ctx.h), (text, lib.last_error(ctx.h))
            assert (ctx.download(d_out, fill.shape, np.uint8) == 0x5A).all(), text
        assert lib.k_bc7_mode5_tiles(ctx.h, C.c_void_p(d_tiles), 0, C.c_void_p(d_out)) == 1   # nothing to do is no error, and nothing is written
        assert (ctx.download(d_out, fill.shape, np.uint8) == 0x5A).all()
        assert T.bc7_mode5_tiles(ctx, np.zeros((0, 16, 4), np.uint8)).shape == (0, 16)
    finally:
        ctx.free(d_tiles)
        ctx.free(d_out)


# ---------------------------------------------------------------- the filter through the transcoding entries

def _counted(ctx, decoded, im, flags, endpoint_indices=None):
    """bu_hip_k_transcode_etc1s_image_counted on one image's colour slice -> (ok, invalid blocks, the output over a fill of 0x5A)"""
    ep = np.ascontiguousarray(decoded["endpoint_palette"], np.uint8)
    sel = np.ascontiguousarray(decoded["selector_palette"], np.uint32)
    ei = im["endpoint_indices"] if endpoint_indices is None else endpoint_indices
    n = im["num_blocks_x"] * im["num_blocks_y"]
    held = [ctx.upload(a) for a in (ep, sel, np.ascontiguousarray(ei, np.uint16).reshape(-1), np.ascontiguousarray(im["selector_indices"], np.uint16).reshape(-1),
                                    np.full((n, 16), 0x5A, np.uint8))]
    try:
        invalid = C.c_uint32(0xFFFF)
        ok = ctx.lib.k_transcode_etc1s_image_counted(ctx.h, C.c_void_p(held[0]), ep.shape[0], C.c_void_p(held[1]), sel.size, C.c_void_p(held[2]), C.c_void_p(held[3]), None, None,
                                                     im["num_blocks_x"], im["num_blocks_y"], im["width"], im["height"], T.BC7_RGBA, C.c_void_p(held[4]), 0, 0, flags, C.byref(invalid))
        return ok, invalid.value, ctx.download(held[4], (n, 16), np.uint8)
    finally:
        for p in held:
            ctx.free(p)


@pytest.mark.parametrize("name", _states())
def test_every_state_through_the_three_entries_is_the_reference_tools_bytes(ctx, name):
    arrays, _ = K.golden()
    data = arrays["file_" + name]
    decoded = T.decode_etc1s_file(data)
    for suffix, filtering in (("_bc7", True), ("_bc7nf", False)):
        whole = T.transcode_etc1s_textures(ctx, data, T.BC7_RGBA, chroma_filtering=filtering)
        assert len(whole) == len(decoded["images"])
        for im, got_whole in zip(decoded["images"], whole):
            want = arrays[E.image_key(name, im["level"], im["layer"], im["face"]) + suffix]
            what = (name, suffix, im["level"], im["layer"])
            _same_blocks(T.transcode_etc1s_texture_image(ctx, decoded, im, T.BC7_RGBA, chroma_filtering=filtering), want, decoded, im, what + ("one image",))
            ok, invalid, got = _counted(ctx, decoded, im, 0 if filtering else X.NO_CHROMA_FILTERING)
            assert ok == 1 and invalid == 0, what
            _same_blocks(got, want, decoded, im, what + ("counted",))
            _same_blocks(got_whole, want, decoded, im, what + ("one launch",))


def test_one_launch_over_many_images_reads_no_neighbour_from_another_image(ctx):
    """The thin chains and two saturated images behind one slice table (one pair of palettes: the files' palettes end to end, the indices moved up), once in file order
    and once with the records and the index ranges in a seeded other order, which puts other blocks on each side of every image's first and last row. Every image must
    still be its own golden: a neighbour read past an image's edge would meet opposed chroma."""
    arrays, _ = K.golden()
    images, ep_pals, sel_pals = [], [], []
    n_ep = n_sel = 0
    for name in list(K.THIN_CHAINS) + ["saturated"]:
        dec = T.decode_etc1s_file(arrays["file_" + name])
        for im in dec["images"][:2] if name == "saturated" else dec["images"]:
            images.append((dict(im), (im["endpoint_indices"].reshape(-1).astype(np.int64) + n_ep).astype(np.uint16), (im["selector_indices"].reshape(-1).astype(np.int64) + n_sel).astype(np.uint16),
                           arrays[E.image_key(name, im["level"], im["layer"], im["face"]) + "_bc7"], dec))
        ep_pals.append(np.asarray(dec["endpoint_palette"], np.uint8).reshape(-1, 4))
        sel_pals.append(np.asarray(dec["selector_palette"], np.uint32).reshape(-1))
        n_ep, n_sel = n_ep + len(ep_pals[-1]), n_sel + sel_pals[-1].size
    assert len(images) >= 20 and n_ep < 65536 and n_sel < 65536
    for order in (np.arange(len(images)), np.random.default_rng(140).permutation(len(images))):
        picked = [images[k] for k in order]
        firsts = np.concatenate([[0], np.cumsum([len(p[1]) for p in picked])])[:-1]
        merged = {"endpoint_palette": np.concatenate(ep_pals), "selector_palette": np.concatenate(sel_pals), "_endpoint_indices": np.concatenate([p[1] for p in picked]),
                  "_selector_indices": np.concatenate([p[2] for p in picked])}
        got = T._transcode_etc1s_slices(ctx, merged, [p[0] for p in picked], firsts, None, T.BC7_RGBA, None, 0)
        for k, (im, _, _, want, dec), blocks in zip(order, picked, got):
            _same_blocks(blocks, want, dec, im, ("image", int(k), im["num_blocks_x"], im["num_blocks_y"]))


def test_a_planted_neighbour_of_a_gate_cell_leaves_its_centre_unfiltered(ctx):
    """The documented rule -- a neighbour whose index is past the palette contributes the centre's own entry -- on one gate cell per position, each with a difference
    past the threshold: the planted neighbour was the only one that differed, so the centre comes out as without the filter; every block that touches no planted one
    is the golden."""
    arrays, _ = K.golden()
    decoded = T.decode_etc1s_file(arrays["file_gate"])
    im = decoded["images"][0]
    nbx, nby = im["num_blocks_x"], im["num_blocks_y"]
    filtered, plain = arrays[E.image_key("gate", 0, 0, 0) + "_bc7"], arrays[E.image_key("gate", 0, 0, 0) + "_bc7nf"]
    ei = im["endpoint_indices"].copy()
    planted, centres = [], []
    for n, (kind, value, sign, (dx, dy)) in enumerate(K.gate_cells()):
        if (kind, value, sign) == ("cg", 10.25, 1):   # one row of cells: the eight positions
            y, x = 3 * (n // 8) + 1, 3 * (n % 8) + 1
            centres.append(y * nbx + x)
            planted.append((y + dy) * nbx + x + dx)
            ei[y + dy, x + dx] = len(decoded["endpoint_palette"])
    assert len(planted) == 8 and (filtered[centres] != plain[centres]).any(1).sum() >= 4   # re-encoded, all eight; some come out as the bytes they had
    ok, invalid, out = _counted(ctx, decoded, im, 0, ei)
    assert ok == 1 and invalid == 8 and (out[planted] == 0).all()
    _same_blocks(out[centres], plain[centres], decoded, im, "the centres")
    touching = {p + dy * nbx + dx for p in planted for dy in (-1, 0, 1) for dx in (-1, 0, 1)}
    far = np.array(sorted(set(range(nbx * nby)) - touching))
    bad = np.flatnonzero((out[far] != filtered[far]).any(1))
    assert bad.size == 0, far[bad[:8]]


@pytest.mark.ref
@pytest.mark.skipif(helpers.ref_harness_version() < 4, reason="oracle/_ref/libref_harness.so with ref_encode_bc7_mode5 (harness version 4) not present")
@pytest.mark.parametrize("seed", [7001, 7002])
def test_fresh_seeds_against_the_reference(ctx, seed):
    """seeds the golden does not use: 16,384 random tiles against the reference's encoder, one saturated state against the restatement"""
    tiles = K.random_tiles(seed, 16384)
    want = np.zeros((len(tiles), 16), np.uint8)
    u8p = C.POINTER(C.c_uint8)
    assert helpers.ref().ref_encode_bc7_mode5(np.ascontiguousarray(tiles).ctypes.data_as(u8p), len(tiles), want.ctypes.data_as(u8p)) == 1
    _same_tiles(T.bc7_mode5_tiles(ctx, tiles), want, tiles, seed)
    data = K.write_state(K.saturated_state(seed, n_images=1, nb=16))
    decoded = T.decode_etc1s_file(data)
    im = decoded["images"][0]
    _same_blocks(T.transcode_etc1s_texture(ctx, data, T.BC7_RGBA), X.bc7_blocks(decoded, im, True), decoded, im, ("saturated", seed))
