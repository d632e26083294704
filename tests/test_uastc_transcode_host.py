"""CPU tests of the UASTC LDR 4x4 transcode core (basis_universal_amd/csrc/uastc_transcode.h, compiled by g++ into tests/native/libtranscode_host.so) against the
reference's known answers, on encoder output (tests/golden/uastc_transcode_vectors.npz) and on arbitrary valid and invalid blocks no encoder writes
(tests/golden/uastc_transcode_fuzz.npz: the block families of transcode_helpers.fuzz_families; live, 200,000 random-bit blocks per target where oracle/_ref is built).
Both fixtures come from tools/gen_golden_uastc_transcode.py. Also the container reader (transcode.read_uastc_file)."""
import json
import pathlib
import struct

import numpy as np
import pytest

import helpers
import transcode_helpers as T
from basis_universal_amd import transcode
from basis_universal_amd.backend import uastc_basis_file, uastc_ktx2_file

GOLDEN = pathlib.Path(__file__).resolve().parent / "golden"
SETS = ("level3", "level2", "default_l2")
# golden array -> (target, high quality)
CASES = {"rgba32": (T.RGBA32, False), "astc": (T.ASTC, False), "bc7": (T.BC7, False), "bc1": (T.BC1, False), "bc1_hq": (T.BC1, True), "bc3": (T.BC3, False),
         "bc3_hq": (T.BC3, True), "bc4_r": (T.BC4, False), "bc5_ra": (T.BC5, False)}


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN / "uastc_transcode_vectors.npz")


def test_golden_inputs_cover_every_mode_and_bc1_route(golden):
    """The condition the vectors were generated under: all 19 modes occur, and each BC1 route (hint0, hint1, neither) at least 100 times among the non-solid blocks."""
    modes = np.zeros(19, np.int64)
    for s in SETS:
        blocks = golden[f"{s}_blocks"]
        modes += np.bincount(T.block_modes(blocks), minlength=19)[:19]
        r = T.bc1_routes(blocks)
        r = r[r != 0]
        assert ((r & 2) != 0).sum() >= 100 and ((r & 6) == 4).sum() >= 100 and ((r & 6) == 0).sum() >= 100, s
    assert (modes > 0).all(), modes


@pytest.mark.parametrize("name", sorted(CASES))
@pytest.mark.parametrize("which", SETS)
def test_host_core_equals_reference(golden, which, name):
    target, hq = CASES[name]
    blocks = golden[f"{which}_blocks"]
    out, ok = T.host_transcode(blocks, target, hq)
    assert ok.all()
    exp = golden[f"{which}_{name}"]
    bad = np.flatnonzero((out.reshape(exp.shape) != exp).any(axis=1))
    assert bad.size == 0, f"{bad.size} of {exp.shape[0]} blocks differ, first {bad[:8].tolist()}"


def _bc4_numpy(values):
    """encode_bc4 (transcoder/basisu_transcoder.cpp:17737) restated: values (n, 16) -> (n, 8) bytes"""
    v = values.astype(np.int64)
    mn, mx = v.min(axis=1), v.max(axis=1)
    delta = mx - mn
    x = v * 14 + (4 - mn * 14)[:, None]
    k = sum((x >= (delta * m)[:, None]).astype(np.int64) for m in (13, 11, 9, 7, 5, 3, 1))
    code = np.array([1, 7, 6, 5, 4, 3, 2, 0], np.uint64)[k]
    bits = np.zeros(v.shape[0], np.uint64)
    for i in range(16):
        bits |= code[:, i] << np.uint64(3 * i)
    bits[delta == 0] = 0
    word = mx.astype(np.uint64) | (mn.astype(np.uint64) << np.uint64(8)) | (bits << np.uint64(16))
    return word.view(np.uint8).reshape(-1, 8)


def test_channel_plumbing(golden):
    """BC3 = BC4 of alpha + BC1; BC5 = BC4 of its two channels; BC4 of any channel = encode_bc4 of the decoded texels (the reference tool only shows 0 and 0 / 3)."""
    for s in SETS:
        blocks = golden[f"{s}_blocks"]
        texels = golden[f"{s}_rgba32"].reshape(-1, 16, 4)
        bc4 = [T.host_transcode(blocks, T.BC4, channels=(c, 3))[0] for c in range(4)]
        for c in range(4):
            assert (bc4[c] == _bc4_numpy(texels[:, :, c])).all(), (s, c)
        assert (bc4[0] == golden[f"{s}_bc4_r"]).all()
        assert (golden[f"{s}_bc3"][:, :8] == bc4[3]).all() and (golden[f"{s}_bc3"][:, 8:] == golden[f"{s}_bc1"]).all()
        assert (golden[f"{s}_bc3_hq"][:, 8:] == golden[f"{s}_bc1_hq"]).all()
        assert (golden[f"{s}_bc5_ra"][:, :8] == bc4[0]).all() and (golden[f"{s}_bc5_ra"][:, 8:] == bc4[3]).all()
        bc5 = T.host_transcode(blocks, T.BC5, channels=(1, 2))[0]
        assert (bc5[:, :8] == bc4[1]).all() and (bc5[:, 8:] == bc4[2]).all()


# ---------------------------------------------------------------- blocks no encoder writes

needs_harness3 = pytest.mark.skipif(helpers.ref_harness_version() < 3, reason="oracle/_ref/libref_harness.so with ref_transcode_uastc (harness version 3) not present")


@pytest.fixture(scope="module")
def fuzz():
    return np.load(GOLDEN / "uastc_transcode_fuzz.npz")


def test_mode_layout_agrees_with_the_unpacker():
    """The field layout the generator writes through: the weight field is where the RDO pass's table has it, every field lies inside the block, and endpoint values,
    pattern and component selector written through the layout are what unpack_block reads back."""
    first = [65, 69, 73, 89, 89, 68, 66, 89, 0, 97, 65, 66, 81, 94, 92, 62, 98, 61, 49]   # g_uastc_mode_selector_bits' first bit per mode
    rng = T._Bits(5)
    for lay in T.layouts():
        if lay.mode == 8:
            continue
        assert lay.weight_ofs == first[lay.mode] and lay.weight_ofs + lay.weight_len <= 128
        assert lay.ep_ofs + lay.ep_bits * lay.ep_values == lay.weight_ofs
        for _ in range(16):
            values = [rng.below(lay.levels) for _ in range(lay.ep_values)]
            v = T._put_endpoints(T._random_in_mode(rng, lay), lay, values)
            pattern, ccs = T._get(v, lay.pattern_ofs, lay.pattern_bits), T._get(v, lay.ccs_ofs, lay.ccs_bits)
            mode, ep, _w, got_pattern, got_ccs = T.unpacked_fields(T._to_blocks([v])[0])
            assert mode == lay.mode and ep[:lay.ep_values].tolist() == values and got_pattern == pattern
            assert got_ccs == (3 if lay.mode == 17 else ccs)


def test_fuzz_generator_reproduces_the_fixture(fuzz):
    """The committed blocks are what the generator makes today: a change to it cannot silently detach the tests from the fixture."""
    fam, cause, _drawn = T.fuzz_families()
    meta = json.loads(bytes(fuzz["meta"]))
    assert (meta["seed"], meta["quota"], tuple(meta["families"]), tuple(meta["invalid_causes"])) == (T.FUZZ_SEED, T.FUZZ_QUOTA, T.FAMILIES, T.INVALID_CAUSES)
    for i, name in enumerate(T.FAMILIES):
        got, want = fam[name], fuzz["blocks"][fuzz["family"] == i]
        assert got.shape == want.shape and (got == want).all(), f"family {name}: the generator no longer writes the fixture's blocks (rerun tools/gen_golden_uastc_transcode.py fuzz)"
    assert (cause == fuzz["invalid_cause"]).all()
    assert sorted(fuzz.files) == sorted(["blocks", "family", "invalid_cause", "valid", "meta"] + list(T.FUZZ_CASES))


def test_fuzz_fixture_coverage(fuzz):
    """Among the blocks the reference accepts: every mode at least the quota of times, each BC1 route (hint0, hint1 only, neither) at least 100 times among non-solid blocks,
    a trit / quint group at or past its radix in every mode that has such groups; and the invalid family has blocks of each of its four causes, all refused."""
    blocks, family, valid = fuzz["blocks"], fuzz["family"], fuzz["valid"]
    per_mode, routes = T.check_fuzz_coverage(blocks, family, valid, fuzz["invalid_cause"], T.FUZZ_QUOTA)
    meta = json.loads(bytes(fuzz["meta"]))
    assert per_mode.tolist() == meta["valid_per_mode"] and list(routes) == meta["bc1_routes_hint0_hint1_neither"]
    names = np.array(T.FAMILIES)[family]
    assert not valid[(names == "random_invalid") | (names == "invalid")].any()
    assert valid[~((names == "random_invalid") | (names == "invalid"))].all()
    assert all((names == f).any() for f in T.FAMILIES)
    # the families are what their names say
    hints = T.layout_hints(blocks[names == "hints"])
    assert all((hints == h).sum() >= 100 for h in range(4))
    assert T.bise_overflow_mask(blocks[names == "bise_overflow"]).all()
    solid = blocks[names == "solid"]
    assert (T.code_modes(solid) == 8).all() and (solid[:, 5:] != 0).any(axis=1).sum() > solid.shape[0] // 2   # junk after the colour (bits 5..36): in the bytes past it
    # the mode-8 colours include 0 and 255 in every channel
    colours = T.host_transcode(solid, T.RGBA32)[0][:, 0, 0, :]
    assert all((colours[:, c] == 0).any() and (colours[:, c] == 255).any() for c in range(4))


@pytest.mark.parametrize("name", sorted(T.FUZZ_CASES))
def test_host_core_equals_reference_on_fuzz_families(fuzz, name):
    target, hq, ch = T.FUZZ_CASES[name]
    out, ok = T.host_transcode(fuzz["blocks"], target, hq, ch)
    T.assert_equals_reference(fuzz["blocks"], fuzz[name], fuzz["valid"], out, ok, f"host core, {name}", fuzz["family"])


LIVE_BLOCKS, LIVE_BATCH = 200000, 50000


@pytest.mark.ref
@needs_harness3
@pytest.mark.parametrize("name", sorted(T.FUZZ_CASES))
def test_random_blocks_every_target_against_reference(name):
    """200,000 fresh random-bit blocks per target, in batches, through the reference's per-block transcoders: validity and bytes equal, refused blocks zero on both
    sides, no block left out. At least 90 % of the blocks drawn must be valid according to the reference (96.3 % measured with the core)."""
    target, hq, ch = T.FUZZ_CASES[name]
    rng = T._Bits(20261018)
    compared = valid = 0
    while compared < LIVE_BLOCKS:
        blocks = rng.blocks(LIVE_BATCH)
        exp, exp_ok = helpers.ref_transcode_uastc(blocks, target, hq, ch)
        out, ok = T.host_transcode(blocks, target, hq, ch)
        T.assert_equals_reference(blocks, exp, exp_ok, out, ok, f"host core against the live reference, {name}, blocks {compared}..")
        compared += blocks.shape[0]
        valid += int(exp_ok.sum())
    print(f"{name}: {compared} random-bit blocks compared with the reference, none excluded; {valid} ({100.0 * valid / compared:.2f} %) valid, {compared - valid} refused by both")
    assert compared >= 200000 and valid >= 0.9 * compared, (compared, valid)


@pytest.mark.ref
def test_random_blocks_validity_and_bc7_against_reference():
    """20,000 random-bit blocks that unpack as valid: BC7 bytes equal the reference's; and on every random block drawn the core agrees with the reference on validity.
    Runs on any build of the harness: the batched ref_transcode_uastc where it is there (version 3), the per-block entries of the older builds otherwise."""
    L = helpers.ref()
    batched = hasattr(L, "ref_transcode_uastc")
    rng = np.random.default_rng(20261016)
    valid_seen, invalid_seen, tmp, px = 0, 0, np.zeros(64, np.uint8), np.zeros(64, np.uint8)
    while valid_seen < 20000:
        blocks = rng.integers(0, 256, (8192, 16), dtype=np.uint8)
        if batched:
            ref_ok = helpers.ref_transcode_uastc(blocks, T.RGBA32)[1]   # unpack_uastc
        else:
            ref_ok = np.array([L.ref_unpack_uastc(helpers.ptr(blocks[i]), helpers.ptr(tmp)) for i in range(blocks.shape[0])], np.uint8)
        bc7, ok = T.host_transcode(blocks, T.BC7)
        assert (ok == ref_ok).all(), "validity differs from unpack_uastc's"
        for t in (T.RGBA32, T.ASTC, T.BC1, T.BC5):
            assert (T.host_transcode(blocks, t)[1] == ref_ok).all()
        exp = np.zeros((blocks.shape[0], 16), np.uint8)
        for i in np.flatnonzero(ref_ok):
            assert L.ref_uastc_to_bc7_pixels(helpers.ptr(blocks[i]), helpers.ptr(exp[i]), helpers.ptr(px)) in (0, 1)   # the BC7 bytes are written before the unpack
        if batched:   # the batched entry refuses what unpack_uastc refuses and writes what the single-block one does
            out, out_ok = helpers.ref_transcode_uastc(blocks, T.BC7)
            assert (out_ok == ref_ok).all() and (out == exp).all()
        assert (bc7 == exp).all()
        assert (bc7[ref_ok == 0] == 0).all()
        valid_seen += int(ref_ok.sum())
        invalid_seen += int((ref_ok == 0).sum())
    assert invalid_seen > 0


# ---------------------------------------------------------------- containers

def _chain(w, h, levels, layers=1):
    """slices (image-major, then mip) and random blocks for `layers` images of w x h with `levels` mips"""
    slices, first = [], 0
    for image in range(layers):
        for l in range(levels):
            lw, lh = max(w >> l, 1), max(h >> l, 1)
            nbx, nby = (lw + 3) // 4, (lh + 3) // 4
            slices.append((first, nbx, nby, lw, lh, image, l, 0))
            first += nbx * nby
    blocks = np.random.default_rng(7).integers(0, 256, (first, 16), dtype=np.uint8)
    return slices, blocks


@pytest.mark.parametrize("writer", ["basis", "ktx2"])
@pytest.mark.parametrize("w,h,levels,layers", [(64, 64, 7, 1), (61, 35, 3, 1), (32, 20, 2, 3)])
def test_read_uastc_file_round_trip(writer, w, h, levels, layers):
    slices, blocks = _chain(w, h, levels, layers)
    tex_type = 1 if layers > 1 else 0   # cBASISTexType2DArray
    data = (uastc_basis_file(blocks, slices, tex_type=tex_type) if writer == "basis" else uastc_ktx2_file(blocks, slices, tex_type=tex_type, has_alpha=True)).tobytes()
    info = transcode.read_uastc_file(data)
    assert (info["format"], info["width"], info["height"], info["layers"], info["faces"], info["levels"]) == ("UASTC_LDR_4x4", w, h, layers, 1, list(range(levels)))
    assert len(info["images"]) == len(slices)
    for first, nbx, nby, lw, lh, image, l, _a in slices:
        im = [m for m in info["images"] if (m["level"], m["layer"]) == (l, image)]
        assert len(im) == 1
        im = im[0]
        assert (im["width"], im["height"], im["num_blocks_x"], im["num_blocks_y"]) == (lw, lh, nbx, nby)
        assert data[im["offset"]:im["offset"] + im["length"]] == blocks[first:first + nbx * nby].tobytes()


def test_read_uastc_file_refuses_bad_files():
    slices, blocks = _chain(40, 24, 3)
    ktx2 = uastc_ktx2_file(blocks, slices).tobytes()
    basis = uastc_basis_file(blocks, slices).tobytes()
    # truncated at every header boundary (and just short of the end)
    for data, cuts in ((ktx2, (0, 11, 12, 79, 80, 80 + 24 * 3 - 1, 80 + 24 * 3, 80 + 24 * 3 + 43, len(ktx2) - 1)), (basis, (0, 1, 2, 76, 77, 77 + 23 * 3 - 1, 77 + 23 * 3, len(basis) - 1))):
        for cut in cuts:
            with pytest.raises(ValueError):
                transcode.read_uastc_file(data[:cut])
    # a level offset past the end
    bad = bytearray(ktx2)
    struct.pack_into("<Q", bad, 80, len(ktx2) + 16)
    with pytest.raises(ValueError, match="level 0"):
        transcode.read_uastc_file(bytes(bad))
    bad = bytearray(basis)
    struct.pack_into("<I", bad, 77 + 5 + 8, len(basis))
    with pytest.raises(ValueError, match="slice 0"):
        transcode.read_uastc_file(bytes(bad))
    # a supercompression scheme other than none
    for scheme in (1, 2):
        bad = bytearray(ktx2)
        struct.pack_into("<I", bad, 44, scheme)
        with pytest.raises(ValueError, match="supercompression"):
            transcode.read_uastc_file(bytes(bad))
    # an ETC1S file: the .basis header's texture format / flag, the KTX2 descriptor's colour model
    bad = bytearray(basis)
    bad[20] = 0
    with pytest.raises(ValueError, match="ETC1S"):
        transcode.read_uastc_file(bytes(bad))
    bad = bytearray(ktx2)
    bad[struct.unpack_from("<I", ktx2, 48)[0] + 12] = 163
    with pytest.raises(ValueError, match="UASTC"):
        transcode.read_uastc_file(bytes(bad))
    with pytest.raises(ValueError):
        transcode.read_uastc_file(b"not a texture file at all")


def test_unsupported_targets_are_refused():
    for target in (0, 1, 7, 8, 9, 14, 16, 20, 22):   # ETC1, ETC2, BC7 alt, PVRTC1 x2, RGB565, RGBA4444, ETC2 EAC R11, an HDR format
        with pytest.raises(ValueError, match="not supported"):
            transcode.transcode_uastc_blocks(None, np.zeros((1, 16), np.uint8), 1, 1, target)
