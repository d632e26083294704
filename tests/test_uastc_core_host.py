"""CPU-only checks of the UASTC path.

The HIP kernels and tests/native/uastc_host.cpp compile the SAME source (basis_universal_amd/csrc/uastc_core.h); here the host build
is held against (1) the committed known-answer vectors produced by the real reference (tests/golden/uastc_reference_vectors.npz,
tools/gen_golden_uastc.py) and (2), where oracle/_ref is present, the reference itself stage by stage. The GPU build is held to the
same vectors in test_gpu_uastc.py. All comparisons are bit-exact.
"""
import pathlib

import numpy as np
import pytest

import helpers
from helpers import ptr

GOLDEN = pathlib.Path(__file__).resolve().parent / "golden" / "uastc_reference_vectors.npz"


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


@pytest.mark.parametrize("name,flags", helpers.uastc_flag_sets())
def test_host_core_matches_reference_vectors(golden, name, flags):
    blocks = golden["blocks"]
    if (flags & 7) == 4:
        blocks = blocks[::4]
    got = helpers.host_encode_uastc(blocks, flags)
    bad = np.nonzero((got != golden[name]).any(1))[0]
    assert bad.size == 0, f"{name}: {bad.size} of {blocks.shape[0]} blocks differ, first {bad[:5]}"


def test_golden_covers_every_mode(golden):
    """The level-2 to level-4 vectors must exercise the UASTC modes image-like tiles end in (mode = prefix code of the first byte, transcoder.cpp:14376-14402).
    Modes 14 and 18 are not asked of THIS file; every mode, partition pattern and dual-plane selector -- 14 and 18 among them -- is asked of the planted tiles at
    level 3 (tests/test_uastc_planted_host.py::test_conditions on tests/golden/uastc_planted_vectors.npz)."""
    codes = {0: (0x1, 4), 1: (0x35, 6), 2: (0x1D, 5), 3: (0x3, 5), 4: (0x13, 5), 5: (0xB, 5), 6: (0x1B, 5), 7: (0x7, 5), 8: (0x17, 5), 9: (0xF, 5),
             10: (0x2, 3), 11: (0x0, 2), 12: (0x6, 3), 13: (0x1F, 5), 14: (0xD, 5), 15: (0x5, 7), 16: (0x15, 6), 17: (0x25, 6), 18: (0x9, 4)}
    seen = set()
    for name in ("level2", "level3", "level4"):
        first = golden[name][:, 0].astype(np.uint32)
        for m, (code, n) in codes.items():
            if ((first & ((1 << n) - 1)) == code).any():
                seen.add(m)
    assert seen >= set(range(19)) - {18, 14}, sorted(seen)


@pytest.mark.ref
@pytest.mark.skipif(not helpers.have_ref(), reason="oracle/_ref not built")
def test_colour_cell_fit_vs_reference():
    """cell_compress / cell_estimate against color_cell_compression / color_cell_compression_est_astc (bc7enc.cpp:1364, 1764) for
    every (weights, endpoint range, alpha) combination a UASTC mode uses, on random, smooth, two-colour, solid and near-solid cells."""
    R, H = helpers.ref(), helpers.uastc_host()
    rng = np.random.default_rng(1)
    combos = [(4, 19, 0), (5, 11, 0), (2, 20, 0), (3, 8, 0), (2, 7, 0), (2, 12, 0), (3, 20, 0), (2, 18, 0), (2, 8, 1), (2, 20, 1), (4, 13, 1), (2, 13, 0),
              (3, 19, 1), (1, 20, 0), (4, 20, 1)]

    def gen(kind, n):
        if kind == 0:
            return rng.integers(0, 256, (n, 4), dtype=np.uint8)
        if kind == 1:
            base, d, t = rng.integers(0, 256, 4), rng.integers(-40, 41, 4), rng.random((n, 1))
            return np.clip(base + d * t + rng.normal(0, 3, (n, 4)), 0, 255).astype(np.uint8)
        if kind == 2:
            return rng.integers(0, 256, (2, 4), dtype=np.uint8)[rng.integers(0, 2, n)]
        if kind == 3:
            return np.tile(rng.integers(0, 256, 4, dtype=np.uint8), (n, 1))
        return np.clip(rng.integers(0, 256, 4) + rng.integers(-2, 3, (n, 4)), 0, 255).astype(np.uint8)

    for _ in range(6000):
        wb, rg, al = combos[rng.integers(len(combos))]
        # the device code fits "the texels of a block selected by a mask"; the reference sees the same texels gathered in order
        mask = int(rng.integers(1, 1 << 16)) if rng.random() < 0.7 else 0xFFFF
        members = [i for i in range(16) if (mask >> i) & 1]
        n, kind = len(members), int(rng.integers(0, 5))
        px16 = np.ascontiguousarray(rng.integers(0, 256, (16, 4), dtype=np.uint8))
        px16[members] = gen(kind, n)
        if not al and rng.random() < 0.7:
            px16[:, 3] = 255
        px = np.ascontiguousarray(px16[members])
        uber, ls = int(rng.choice([0, 1, 1, 3, 6])), int(rng.choice([1, 1, 2]))
        o1, o2 = np.zeros(24, np.uint8), np.zeros(24, np.uint8)
        e1 = R.ref_color_cell_compression(ptr(px), n, wb, rg, al, uber, ls, None, ptr(o1))
        e2 = H.hc_cell_compress(ptr(px16), mask, wb, rg, al, uber, ls, ptr(o2))
        assert e1 == e2 and (o1[:8] == o2[:8]).all() and (o1[8:8 + n] == o2[8:][members]).all(), (wb, rg, al, mask, kind, uber, ls, px.tolist())
        if wb in (2, 3) and not (wb == 3 and al):  # the (weights, channels) combinations the partition estimate is used with
            comps = 4 if al else 3
            assert R.ref_ccell_est(wb, comps, ptr(px), n, 2 ** 64 - 1) == H.hc_cell_estimate(wb, comps, ptr(px16), mask)


def test_weight_formula_matches_tables():
    H = helpers.uastc_host()
    for bits in range(1, 6):
        for s in range(1 << bits):
            assert H.hc_weight_of(bits, s) == H.hc_weight_table(bits, s), (bits, s)


@pytest.mark.ref
@pytest.mark.skipif(not helpers.have_ref(), reason="oracle/_ref not built")
@pytest.mark.parametrize("flags", [0, 1, 2, 3, 2 | 16, 2 | 8 | 512])
def test_host_core_vs_reference_fresh_blocks(flags):
    """Blocks the golden file has never seen (new seeds), including ragged image edges clamped like the reference's block extraction."""
    rng = np.random.default_rng(1000 + flags)
    img = helpers.synth(72, 52, 4321 + flags)  # 72x52: not a multiple of 4 in height -> clamped edge blocks
    img[..., 3] = np.where(rng.random((52, 72)) < 0.3, rng.integers(0, 256, (52, 72)), 255).astype(np.uint8)
    blocks = np.concatenate([helpers.to_pixel_blocks(img), helpers.to_pixel_blocks(helpers.uniform_random(24, 24, 7 + flags))])
    if (flags & 7) == 3:
        blocks = blocks[:120]
    assert (helpers.host_encode_uastc(blocks, flags) == helpers.ref_encode_uastc(blocks, flags)).all()


@pytest.mark.skipif(not helpers.have_ref(), reason="oracle/_ref not present")
def test_host_decoder_matches_reference_unpack(golden):
    """The decoder behind every PSNR this repository prints (helpers.host_decode_uastc = unpack + interpolation of the core) against the reference's
    unpack_uastc, on the blocks of every level of the known answers (all modes incl. solid colour) and on RDO output."""
    for name in ("level0", "level2", "level4"):
        packed = golden[name]
        assert (helpers.host_decode_uastc(packed) == helpers.ref_decode_uastc(packed)).all(), name
    z = np.load(GOLDEN.parent / "uastc_rdo_vectors.npz")
    assert (helpers.host_decode_uastc(z["strong_l2"]) == helpers.ref_decode_uastc(z["strong_l2"])).all()


@pytest.mark.parametrize("flags", [0, 2, 3, 4])
def test_fused_scoring_equals_the_general_decoders(flags):
    """score_candidate's fused decode + error per texel (uastc_errors / bc7_errors: no decoded images, tables picked by select) against decode_uastc / decode_bc7 +
    block_error, for every candidate of every mode: opaque, alpha and luminance-alpha blocks."""
    import ctypes as C
    from helpers import uastc_host, synth, to_pixel_blocks
    rgb = to_pixel_blocks(synth(64, 48, 11))
    rgba = rgb.copy(); rgba[..., 3] = (rgba[..., 0].astype(np.int32) * 3 + rgba[..., 1]) % 256
    la = rgba.copy(); la[..., 1] = la[..., 0]; la[..., 2] = la[..., 0]
    flat = rgb.copy(); flat[:, :, :, :3] = (flat[:, :, :, :3] // 64) * 64 + 7      # few distinct values per block: degenerate cells, two-level planes
    blocks = np.ascontiguousarray(np.concatenate([rgb, rgba, la, flat]))
    L = uastc_host()
    checked = C.c_uint32(0)
    bad = L.hc_score_selfcheck(blocks.ctypes.data_as(C.POINTER(C.c_uint8)), blocks.shape[0], flags, C.byref(checked))
    assert checked.value > 2 * blocks.shape[0] and bad == 0, (bad, checked.value)
