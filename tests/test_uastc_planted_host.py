"""CPU-only checks of the planted UASTC tiles (tests/uastc_planted.py, tests/golden/uastc_planted_vectors.npz).

Two kinds. (1) CONDITIONS on the fixture, from the fixture alone: the reference's answers must lie in the cells the tiles were planted in, and its RDO pass must have
modified blocks of most cells -- otherwise the GPU tests built on the file prove less than they say. These are floors on the inputs: a family that falls short is
mended in the generator (seed, tiles per cell), never here. (2) PARITY: the host build of the device core (uastc_core.h, uastc_rdo.h) equals every array of the file,
and where oracle/_ref is present the reference reproduces it. The device build is held to the same file in test_gpu_uastc_planted.py.

This file is also what covers modes 14 and 18, which the image-like vectors of uastc_reference_vectors.npz reach rarely (test_uastc_core_host.py): both are cells of
every family here and win at level 3.
"""
import numpy as np
import pytest

import helpers
import uastc_planted as P

ALL = P.cell_list()
MIN_NOISY_L3 = 165
MIN_SIBLING_MODIFIED = 85
SIBLING_CASE = "sibling_rdo_l3_lam4_jobs3"


def check_conditions(arrays, meta):
    """The floors the fixture is written under (tools/gen_golden_uastc_planted.py asserts them before it writes; test_conditions on the committed file)."""
    n = len(ALL) * P.TILES_PER_CELL
    for fam in P.FAMILIES:
        t = arrays[f"{fam}_tiles"]
        assert t.shape == (n, 4, 4, 4) and t.dtype == np.uint8, fam
    for name, _, _, step in P.encoder_arrays():
        assert arrays[name].shape == (len(range(0, n, step)), 16), name
    for fam in ("exact", "edge"):
        for level in range(5):
            want = P.cells_of_modes(P.LEVEL_MODES[level])
            got = P.reached(arrays[f"{fam}_level{level}"], P.LEVEL4_STEP if level == 4 else 1)
            assert len(want) == {0: 7, 1: 71, 2: 108, 3: 170, 4: 170}[level]
            assert got == want, f"{fam} level {level}: no tile of cells {sorted(set(want) - set(got))} lands in its cell"
    assert len(P.reached(arrays["noisy_level3"])) >= MIN_NOISY_L3
    packed, after = arrays["sibling_level3"], arrays[SIBLING_CASE]
    touched = P.modified_cells(packed, after)
    assert len(touched) >= MIN_SIBLING_MODIFIED, len(touched)
    for mode in P.PATTERN_MODES:
        patterns = len(P.cells_of_modes((mode,)))
        hit = len({c for c in touched if c[0] == mode})
        assert 3 * hit >= patterns, f"RDO modified blocks in {hit} of the {patterns} patterns of mode {mode}"
    assert meta["cells_reached"] == P.meta_counts(arrays)
    assert meta["seeds"] == P.SEEDS and meta["tiles_per_cell"] == P.TILES_PER_CELL and meta["cells"] == 170


@pytest.fixture(scope="module")
def fixture():
    return P.load()


def test_cell_list():
    assert len(ALL) == 170 and len(set(ALL)) == 170 and P.SOLID_CELL not in ALL
    per_mode = {m: sum(1 for c in ALL if c[0] == m) for m in range(19)}
    assert per_mode == {0: 1, 1: 1, 2: 30, 3: 11, 4: 30, 5: 1, 6: 3, 7: 19, 8: 0, 9: 30, 10: 1, 11: 4, 12: 1, 13: 4, 14: 1, 15: 1, 16: 30, 17: 1, 18: 1}
    assert (17, 0, 3) in ALL and [c[2] for c in ALL if c[0] == 6] == [0, 1, 2]
    assert [len(P.cells_of_modes(P.LEVEL_MODES[level])) for level in range(5)] == [7, 71, 108, 170, 170]


def test_conditions(fixture):
    arrays, meta = fixture
    check_conditions(arrays, meta)
    print({k: v for k, v in sorted(meta["cells_reached"].items())})


def test_families_are_what_they_say(fixture):
    """every tile decodes from a block of its cell (the generator asserts it), the fixture holds the generator's tiles, and each family has its property"""
    arrays, _ = fixture
    blocks, tiles = P.families()
    for fam in P.FAMILIES:
        assert (tiles[fam] == arrays[f"{fam}_tiles"]).all(), f"{fam}: the fixture's tiles are not what the generator draws today"
    clean = helpers.host_decode_uastc(blocks["noisy"]).astype(np.int64)
    noisy = arrays["noisy_tiles"].astype(np.int64)
    assert np.abs(noisy - clean).max() == P.NOISE
    opaque = (clean[..., 3] == 255).all(axis=(1, 2))
    grey = (clean[..., 0] == clean[..., 1]).all(axis=(1, 2)) & (clean[..., 0] == clean[..., 2]).all(axis=(1, 2))
    assert opaque.sum() >= 6 * 97 and grey.sum() == 6 * 32       # the 97 cells of the RGB modes; the luminance-alpha modes' 1 + 30 + 1
    assert (noisy[opaque][..., 3] == 255).all() and (noisy[grey][..., 0] == noisy[grey][..., 1]).all() and (noisy[grey][..., 0] == noisy[grey][..., 2]).all()
    e = arrays["edge_tiles"]
    near = ((e <= 8) | (e >= 247))[..., :3].any(axis=(1, 2, 3)) | ((e[..., 3] <= 8).any(axis=(1, 2)))
    print("edge tiles with a channel within 8 of 0 or 255:", int(near.sum()), "of", e.shape[0])
    assert near.sum() >= 0.8 * e.shape[0]
    s = blocks["sibling"].reshape(len(ALL), P.TILES_PER_CELL, 16)
    for c, (cell, group) in enumerate(zip(ALL, s)):
        f0 = P.T.unpacked_fields(group[0])
        for b in group[1:]:
            f = P.T.unpacked_fields(b)
            assert int((f[2] != f0[2]).sum()) <= 1, cell      # weights: at most one differs (a flipped bit changes one weight)


@pytest.mark.parametrize("name,fam,flags,step", P.encoder_arrays(), ids=[a[0] for a in P.encoder_arrays()])
def test_host_core_equals_fixture(fixture, name, fam, flags, step):
    arrays, _ = fixture
    got = helpers.host_encode_uastc(np.ascontiguousarray(arrays[f"{fam}_tiles"][::step]), flags)
    assert (got == arrays[name]).all(), f"{name}: {P.describe_differences(got, arrays[name], P.planted_cells()[::step])}"


@pytest.mark.parametrize("name,src,flags,jobs,kw", P.rdo_arrays(), ids=[a[0] for a in P.rdo_arrays()])
def test_host_rdo_equals_fixture(fixture, name, src, flags, jobs, kw):
    arrays, _ = fixture
    got, counts = helpers.host_uastc_rdo_counted(arrays[src], arrays["sibling_tiles"], flags, jobs, table_trials=True, **kw)
    assert (got == arrays[name]).all(), f"{name}: {P.describe_differences(got, arrays[name])}"
    assert counts["modified"] >= int((arrays[name] != arrays[src]).any(1).sum()) > 0
    plain = helpers.host_uastc_rdo(arrays[src], arrays["sibling_tiles"], flags, jobs, **kw)     # trials decoded, as the reference scores them
    assert (plain == arrays[name]).all(), f"{name}: {P.describe_differences(plain, arrays[name])}"


@pytest.mark.ref
@pytest.mark.skipif(not helpers.have_ref(), reason="oracle/_ref not built")
def test_reference_reproduces_fixture(fixture):
    arrays, _ = fixture
    for name, fam, flags, step in P.encoder_arrays():
        if (flags & 7) == 4 and fam != "exact":
            continue    # level 4 costs the reference the most: once is enough to show the file is its output
        got = helpers.ref_encode_uastc(np.ascontiguousarray(arrays[f"{fam}_tiles"][::step]), flags)
        assert (got == arrays[name]).all(), f"{name}: {P.describe_differences(got, arrays[name])}"
    for name, src, flags, jobs, kw in P.rdo_arrays():
        got = helpers.ref_uastc_rdo(arrays[src], arrays["sibling_tiles"], flags, jobs, **kw)
        assert (got == arrays[name]).all(), f"{name}: {P.describe_differences(got, arrays[name])}"
