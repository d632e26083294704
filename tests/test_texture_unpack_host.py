"""The texture decode core (csrc/texture_unpack.h) built with g++ against the reference's known answers (tests/golden/texture_unpack_vectors.npz, written by
tools/gen_golden_texture_unpack.py from basisu::unpack_block and from the rasters `basisu -unpack` writes): no GPU anywhere in this file."""
import numpy as np
import pytest

import block_unpack_helpers as B
import texture_unpack_helpers as X


@pytest.mark.parametrize("name", sorted(X.BLOCK_MEMBERS))
def test_host_core_equals_the_reference_on_every_golden_block(name):
    """Every block compared, none left out: validity flags equal, every block the reference accepts texel-equal, every block it refuses zero-filled (the
    reference leaves whatever its caller's buffer held)."""
    arrays, meta = X.golden()
    fmt = X.BLOCK_MEMBERS[name]
    assert meta["members"][name]["format"] == fmt
    blocks, want, want_ok = arrays[name + "_blocks"], arrays[name + "_texels"], arrays[name + "_ok"]
    assert blocks.shape == (meta["members"][name]["blocks"], X.BYTES[fmt]) and want.shape == (blocks.shape[0], 16, 4)
    got, got_ok = X.host_unpack(blocks, fmt)
    assert (got_ok == want_ok).all(), (name, np.flatnonzero(got_ok != want_ok)[:8])
    refused = want_ok == 0
    assert int(refused.sum()) == meta["members"][name]["refused"]
    assert (got[refused] == 0).all(), name
    bad = np.flatnonzero((got[~refused] != want[~refused]).any(axis=(1, 2)))
    if bad.size:
        i = np.flatnonzero(~refused)[bad[0]]
        raise AssertionError(f"{name}: {bad.size} of {blocks.shape[0]} blocks differ; first: block {i} {blocks[i].tobytes().hex()} got {got[i].tobytes().hex()} "
                             f"reference {want[i].tobytes().hex()}")


def test_members_are_what_the_issue_of_the_fixture_says():
    arrays, meta = X.golden()
    assert sorted(meta["members"]) == sorted(X.BLOCK_MEMBERS)
    m = meta["members"]
    assert (m["etc1"]["refused"], m["etc1_overflow"]["blocks"], m["etc1_overflow"]["refused"]) == (0, 64, 64)
    assert (m["etc2"]["blocks"], m["etc2"]["refused"]) == (288, 32) and m["r11"]["blocks"] == m["rg11"]["blocks"] == 256
    assert m["astc"]["refused"] == 0 and (m["astc_refused"]["blocks"], m["astc_refused"]["refused"]) == (256, 256)
    for name in X.ENCODER_MADE:
        assert (m[name]["blocks"], m[name]["refused"]) == (X.ENCODER_MADE_BLOCKS, 0)
    assert "restatement" in meta["pvrtc1_modulation_mode_1"] and "not from a run of the reference" in meta["pvrtc1_modulation_mode_1"]


def test_the_fixture_covers_what_it_says_it_covers():
    """Counted from the committed blocks (texture_unpack_helpers.check_coverage, the generator's own assertions): ETC1's modes, flips, tables, delta ends and the
    four ways to overflow; the EAC tables, multipliers, bases and clamps; per ASTC class, endpoint mode, weight range, grid size; void extents; the refusals."""
    arrays, meta = X.golden()
    counts = X.check_coverage(arrays, meta)
    assert counts == meta["counts"]
    assert set(counts["astc_class"]) == {"1_single", "1_dual", "2_single", "2_dual", "3_single", "3_dual", "4_single"}
    assert len(counts["astc_mode"]) == 10 and len(counts["astc_range"]) == 12 and len(counts["astc_grid"]) == 9
    # the refusals are not all of one kind
    assert len(counts["astc_refused"]) >= 5, counts["astc_refused"]


def test_encoder_made_members_are_the_first_blocks_of_the_transcoders_fixtures():
    arrays, _ = X.golden()
    for name, (file, array, fmt) in X.ENCODER_MADE.items():
        z = np.load(X.ROOT / "tests" / "golden" / file)
        assert (arrays[name + "_blocks"] == z[array][:X.ENCODER_MADE_BLOCKS]).all(), name


def test_uastc_made_astc_unpacks_to_the_rgba32_transcode():
    """what the generator recorded about the reference, on the host: the UASTC -> ASTC transcode is exact, so its unpack is the RGBA32 transcode"""
    arrays, meta = X.golden()
    rgba32 = np.load(X.ROOT / "tests" / "golden" / "uastc_transcode_vectors.npz")["level2_rgba32"][:X.ENCODER_MADE_BLOCKS].reshape(-1, 16, 4)
    assert meta["uastc_astc_unpack_equals_rgba32"] == bool((arrays["uastc_astc_texels"] == rgba32).all())
    if meta["uastc_astc_unpack_equals_rgba32"]:
        assert (X.host_unpack(arrays["uastc_astc_blocks"], X.ASTC)[0] == rgba32).all()


@pytest.mark.parametrize("fmt", X.BC_FORMATS, ids=[B.NAMES[f] for f in X.BC_FORMATS])
def test_bc_formats_through_the_new_core_equal_block_unpack_host(fmt):
    blocks, _, _ = B.format_set(fmt)
    old, old_ok = B.host_unpack(blocks, fmt)
    new, new_ok = X.host_unpack(blocks, fmt)
    assert (old_ok == new_ok).all() and (old == new).all()
    assert X.host().th_bytes_per_block(fmt) == B.BYTES[fmt]


def test_bytes_per_block():
    for fmt, unit in X.BYTES.items():
        assert X.host().th_bytes_per_block(fmt) == unit
    for fmt in (7, 11, 12, 13, 14, 19, 22, 99, 2 ** 31):
        assert X.host().th_bytes_per_block(fmt) == 0


def test_etc2_and_rg11_are_their_halves():
    arrays, _ = X.golden()
    blocks = arrays["etc2_blocks"][arrays["etc2_ok"] != 0]
    got, ok = X.host_unpack(blocks, X.ETC2)
    colour, cok = X.host_unpack(blocks[:, 8:], X.ETC1)
    assert ok.all() and cok.all() and (got[..., :3] == colour[..., :3]).all() and (colour[..., 3] == 255).all()
    base, mul, table = blocks[:, 0].astype(int), (blocks[:, 1] >> 4).astype(int), blocks[:, 1] & 15
    sels = np.array([int.from_bytes(b[2:8].tobytes(), "big") for b in blocks], dtype=object)
    tables = np.array(X.EAC_TABLES)
    for t in range(16):
        x, y = t & 3, t >> 2
        s = np.array([(int(v) >> (45 - 3 * (x * 4 + y))) & 7 for v in sels])
        assert (got[:, t, 3] == np.clip(base + tables[table, s] * mul, 0, 255)).all()
    blocks = arrays["rg11_blocks"]
    got, _ = X.host_unpack(blocks, X.RG11)
    assert (got[..., 0] == X.host_unpack(blocks[:, :8], X.R11)[0][..., 0]).all() and (got[..., 1] == X.host_unpack(blocks[:, 8:], X.R11)[0][..., 0]).all()
    assert (got[..., 2] == 0).all() and (got[..., 3] == 255).all()
    vals = np.array([X.eac_values(b) for b in blocks[:, :8]]).clip(0, 2047)   # selector k of eac_values is texel (k // 4, k % 4)
    assert (got[..., 0].reshape(-1, 4, 4).transpose(0, 2, 1).reshape(-1, 16) == (vals * 255 + 1023) // 2047).all()


def test_etc1s_subset_blocks_are_flat_per_block():
    """an ETC1 block whose two halves are equal (differential, delta 0, one table) -- ETC1S -- has four colours in all, the same in both halves whatever the flip"""
    arrays, _ = X.golden()
    blocks = np.array(arrays["etc1_blocks"][:64])
    blocks[:, :3] &= 0xF8
    blocks[:, 3] = (blocks[:, 3] & 0xE0) | ((blocks[:, 3] >> 3) & 0x1C) | 2
    a, ok = X.host_unpack(blocks, X.ETC1)
    blocks[:, 3] |= 1
    b, _ = X.host_unpack(blocks, X.ETC1)
    assert ok.all() and (a == b).all()
    assert max(len({tuple(t) for t in blk}) for blk in a) <= 4


# ---------------------------------------------------------------- BISE groups on their own

def _pack_ise(kind, n, values, rng):
    """a random BISE sequence from the format's packing rule (trit groups m0 T01 m1 T23 m2 T4 m3 T56 m4 T7, quint groups m0 Q012 m1 Q34 m2 Q56) -> (16 bytes, the
    raw T / Q per group, the plain bits per value)"""
    per, tbits = {1: (5, 8), 2: (3, 7)}.get(kind, (1, 0))
    groups = -(-values // per)
    ms = [int(rng.integers(0, 1 << n)) if n else 0 for _ in range(groups * per)]
    packed = [int(rng.integers(0, 1 << tbits)) if tbits else 0 for _ in range(groups)]
    v, at = 0, 0
    cuts = {1: (2, 2, 1, 2, 1), 2: (3, 2, 2)}.get(kind, (0,))
    for g in range(groups):
        t = packed[g]
        for j in range(per):
            v |= ms[g * per + j] << at
            at += n
            v |= (t & ((1 << cuts[j]) - 1)) << at
            t >>= cuts[j]
            at += cuts[j]
    return np.frombuffer((v & ((1 << 128) - 1)).to_bytes(16, "little"), np.uint8), packed, ms


def test_every_trit_and_quint_group_decodes_to_values_in_range_and_is_a_bijection_where_the_format_says_so():
    """All 256 trit groups and all 128 quint groups: every value below 3 / 5; the 243 / 125 canonical encodings (what an encoder writes) decode to distinct
    tuples; plain bits pass through at every width and position of the sequence."""
    for kind, per, size, base in ((1, 5, 256, 3), (2, 3, 128, 5)):
        seen = {}
        for t in range(size):
            bits16 = np.frombuffer(int(t << 0).to_bytes(16, "little"), np.uint8)   # n = 0: the group is its T / Q bits alone
            tup = tuple(X.ise_value(bits16, kind, 0, per, k)[1] for k in range(per))
            assert all(0 <= v < base for v in tup), (kind, t, tup)
            seen.setdefault(tup, []).append(t)
        assert len(seen) == base ** per, (kind, len(seen))
    rng = np.random.default_rng(5)
    for kind, widths in ((0, range(1, 9)), (1, range(0, 7)), (2, range(0, 6))):
        for n in widths:
            values = min(18, 120 // (n + 2))
            bits16, packed, ms = _pack_ise(kind, n, values, rng)
            per = {1: 5, 2: 3}.get(kind, 1)
            for k in range(values):
                m, tq = X.ise_value(bits16, kind, n, values, k)
                assert m == ms[k], (kind, n, k)
                if kind and (k // per + 1) * per <= values:   # a whole group: the same trits / quints as the group alone
                    alone = np.frombuffer(int(packed[k // per]).to_bytes(16, "little"), np.uint8)
                    assert tq == X.ise_value(alone, kind, 0, per, k % per)[1], (kind, n, k)


# ---------------------------------------------------------------- PVRTC1

def _pvrtc1_cases():
    return X.golden()[1]["pvrtc1_images"]


def test_pvrtc1_fixture_lists_the_images_it_should():
    _, meta = X.golden()
    assert sorted({(k, w, h) for k, _, w, h, _ in meta["pvrtc1_images"]}) == sorted(X.pvrtc1_images())
    sizes = {(w, h) for _, _, w, h, _ in meta["pvrtc1_images"]}
    assert {(64, 16), (16, 64), (1, 1), (2, 1), (1, 2), (4, 1), (1, 4), (32, 32), (64, 64)} <= sizes
    assert [tuple(s) for s in meta["pvrtc1_random"]] == list(X.PVRTC1_RANDOM)


@pytest.mark.parametrize("case", _pvrtc1_cases(), ids=[f"{c[0]}_{c[1]}" for c in _pvrtc1_cases()])
def test_pvrtc1_host_core_and_restatement_equal_the_rasters_the_reference_tool_wrote(case):
    key, short, w, h, channels = case
    arrays, _ = X.golden()
    blocks = X.golden_pvrtc1()[0][f"{key}_{short}"]
    want = arrays[f"pvrtc1_{key}_{short}_texels"]
    nbx, nby = (w + 3) // 4, (h + 3) // 4
    assert want.shape == (h, w, channels) and blocks.shape == (nbx * nby, 8)
    assert (blocks[:, 4] & 1 == 0).all(), "every transcoder writes modulation mode 0"
    for what, got in (("host core", X.host_unpack_pvrtc1(blocks, nbx, nby, w, h)), ("restatement", X.pvrtc1_restate(blocks, nbx, nby, w, h))):
        assert (got[..., :channels] == want).all(), (what, key, short)
        if channels == 3:
            assert (got[..., 3] == 255).all(), "opaque endpoints give alpha 255"


@pytest.mark.parametrize("nbx,nby", X.PVRTC1_RANDOM)
def test_pvrtc1_random_images_of_both_modulation_modes(nbx, nby):
    """expected texels from the restatement (the fixture's meta says so): the host core equals the stored raster, and the stored raster is what the restatement gives today"""
    arrays, _ = X.golden()
    blocks, want = arrays[f"pvrtc1_random_{nbx}x{nby}_blocks"], arrays[f"pvrtc1_random_{nbx}x{nby}_texels"]
    assert want.shape == (nby * 4, nbx * 4, 4)
    assert (X.pvrtc1_restate(blocks, nbx, nby) == want).all()
    assert (X.host_unpack_pvrtc1(blocks, nbx, nby) == want).all()


def test_pvrtc1_punch_through_texels_exist_in_the_random_images():
    arrays, _ = X.golden()
    seen = 0
    for nbx, nby in X.PVRTC1_RANDOM:
        blocks, want = arrays[f"pvrtc1_random_{nbx}x{nby}_blocks"], arrays[f"pvrtc1_random_{nbx}x{nby}_texels"]
        for at, b in enumerate(blocks):
            if b[4] & 1:
                mod = int.from_bytes(b[:4].tobytes(), "little")
                bx, by = next((x, y) for y in range(nby) for x in range(nbx) if X.morton_address(x, y, nbx, nby) == at)
                for t in range(16):
                    if (mod >> (2 * t)) & 3 == 2:
                        assert want[by * 4 + (t >> 2), bx * 4 + (t & 3), 3] == 0
                        seen += 1
    assert seen >= 16


def test_morton_address_is_the_kernels():
    """the helper's address rule against pvrtc1.h's through the host core: an image whose block k holds k in its endpoint word decodes block (x, y) from address(x, y)"""
    for nbx, nby in ((1, 1), (2, 1), (1, 2), (8, 2), (2, 8), (4, 4)):
        order = sorted(X.morton_address(x, y, nbx, nby) for y in range(nby) for x in range(nbx))
        assert order == list(range(nbx * nby))
    assert [X.morton_address(x, 0, 8, 2) for x in range(8)] == [0, 2, 4, 6, 8, 10, 12, 14] and X.morton_address(3, 1, 8, 2) == 7
