"""CPU (-m "not gpu"): the per-block arithmetic of PSNR-HVS / PSNR-HVS-M that the kernel's lanes share out (csrc/psnr_hvs.h, built for the host) against a numpy
restatement of psnr_hvs_compute_chan, bit for bit; both against every figure `basisu -compare_hvs` printed (tests/golden/psnr_hvs_vectors.npz); the exported
reduction against the restatement's; the committed constant table against its derivation; and, where oracle/_ref/basisu is there, the tool itself on fresh pairs."""
import ctypes as C
import importlib.util
import math
import pathlib

import numpy as np
import pytest

import psnr_hvs_helpers as P
from basis_universal_amd import stats

ROOT = pathlib.Path(__file__).resolve().parent.parent


def same_bits(x, y):
    return np.ascontiguousarray(x, np.float64).tobytes() == np.ascontiguousarray(y, np.float64).tobytes()


def golden_pairs():
    arrays, meta = P.golden()
    out = [(f"block{k}_{kind}", arrays["blocks_a"][k], arrays["blocks_b"][k], arrays["blocks_hvs"][k]) for k, kind in enumerate(meta["block_kinds"])]
    return out + [(f"{w}x{h}", arrays[f"size_{w}x{h}_a"], arrays[f"size_{w}x{h}_b"], arrays[f"size_{w}x{h}_hvs"]) for w, h in meta["sizes"]]


def test_golden_has_the_pairs_the_checks_rest_on():
    _, meta = P.golden()
    kinds = meta["block_kinds"]
    assert len(kinds) >= 40 and {"near", "unrelated", "flat_noise", "flat_flat", "identical", "one_channel", "alpha"} <= set(kinds)
    assert [tuple(s) for s in meta["sizes"]] == [(1, 1), (5, 7), (9, 9), (20, 28), (64, 40), (100, 52)]
    assert meta["entries"] == P.ENTRIES and len(meta["cases"]) == 6


@pytest.mark.parametrize("name,a,b,printed", golden_pairs(), ids=[p[0] for p in golden_pairs()])
def test_golden_pair_bit_for_bit_and_as_printed(name, a, b, printed):
    """Per block and mode the two doubles of the host build equal the restatement's bit for bit, as do the running sums in the reference's order; reduced, both
    reproduce every figure the tool printed within P.PRINT_TOLERANCE (0.00055: half a unit of the third decimal it prints, plus the slack
    image_metrics_helpers argues for its float-to-text rounding)."""
    restated = P.np_all_modes(a, b, key=name)
    hosted = tuple(P.host_blocks(a, b, m) for m in range(6))
    for m in range(6):
        assert hosted[m][0].shape == (P.block_count(a, b), 2)
        assert same_bits(hosted[m][0], restated[m][0]) and same_bits(hosted[m][1], restated[m][1]), (name, P.MODES[m])
    P.assert_close_to_printed(P.printed_from_running(restated), printed, name + " restatement")
    P.assert_close_to_printed(P.printed_from_running(hosted), printed, name + " host build")
    if "identical" in name:
        got = P.printed_from_running(hosted)
        assert all(got[e][f] == 100000.0 for e in P.ENTRIES for f in ("psnr_hvs", "psnr_hvsm"))


def test_random_blocks_bit_for_bit():
    a, b = P.random_blocks(3000, 77)
    for m in range(6):
        (hb, hr), (nb, nr) = P.host_blocks(a, b, m), P.np_blocks(a, b, m)
        assert hb.shape == (3000, 2) and same_bits(hb, nb) and same_bits(hr, nr), P.MODES[m]
        assert (hb >= 0).all() and (hb[:, 1] <= hb[:, 0]).all()     # masking only ever lowers a term


def test_blocks_clamp_to_each_images_own_edge():
    """a 13x10 image against an 11x14 one, pitches padded and poisoned: the region is 11x10 = 2x2 blocks; columns 11-12 of the first image are its own pixels, not
    copies of column 10, and rows 10-13 of the second its own"""
    rng = np.random.default_rng(5)
    a, b = rng.integers(0, 256, (10, 13, 4), dtype=np.uint8), rng.integers(0, 256, (14, 11, 4), dtype=np.uint8)
    cropped_a, cropped_b = np.ascontiguousarray(a[:, :11]), np.ascontiguousarray(b[:10])
    for m in range(6):
        hb, hr = P.host_blocks(a, b, m, 17, 12)
        nb, nr = P.np_blocks(a, b, m)
        assert hb.shape == (4, 2) and same_bits(hb, nb) and same_bits(hr, nr)
        assert not same_bits(hb, P.np_blocks(cropped_a, cropped_b, m)[0])


def reduce_inputs():
    rng = np.random.default_rng(11)
    out = [("random", rng.random(6) * 50, rng.random(6) * 40, 91), ("zero", np.zeros(6), np.zeros(6), 4), ("one_block", rng.random(6), rng.random(6) * 1e-9, 1)]
    mixed = rng.random(6)
    mixed[3] = 0.0                 # one lossless channel among others
    return out + [("mixed", mixed, mixed * 0.5, 12)]


@pytest.mark.parametrize("name,sh,sm,blocks", reduce_inputs(), ids=[r[0] for r in reduce_inputs()])
def test_exported_reduction_is_the_restatements_exactly(name, sh, sm, blocks):
    sums = stats.HvsSums()
    sums.struct_bytes, sums.blocks = C.sizeof(sums), blocks
    for k in range(6):
        sums.sum_hvs[k], sums.sum_hvsm[k] = sh[k], sm[k]
    product, hosted, restated = stats.reduce_hvs_sums(sums), P.host_reduce(sh, sm, blocks), P.np_reduce(sh, sm, blocks)
    for entry in P.ENTRIES:
        for fig in P.FIGURES:
            assert same_bits(product[entry][fig], restated[entry][fig]) and same_bits(hosted[entry][fig], restated[entry][fig]), (entry, fig)
    if name == "zero":
        assert all(product[e]["psnr_hvs"] == 100000.0 and product[e]["psnr_hvsm"] == 100000.0 for e in P.ENTRIES)
    if name == "mixed":
        assert product["g"]["psnr_hvs"] == 100000.0 and product["rgb"]["psnr_hvs"] < 100.0


def test_reduce_refuses_bad_arguments():
    L = stats._reduce_lib()
    sums, m = stats.HvsSums(), stats._HvsMetrics()
    sums.struct_bytes, sums.blocks = C.sizeof(sums), 1
    assert L.bu_psnr_hvs_reduce(None, C.byref(m)) == 0 and L.bu_psnr_hvs_reduce(C.byref(sums), None) == 0
    sums.struct_bytes = C.sizeof(sums) - 8
    assert L.bu_psnr_hvs_reduce(C.byref(sums), C.byref(m)) == 0
    sums.struct_bytes = C.sizeof(sums)
    assert L.bu_psnr_hvs_reduce(C.byref(sums), C.byref(m)) == 1


def _tool(name):
    spec = importlib.util.spec_from_file_location(name, ROOT / "tools" / f"{name}.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_committed_table_is_its_derivation():
    """csf, mask and alpha exactly as tools/gen_psnr_hvs_tables.py derives them (they do not depend on the C library); the cosines within one binary32 step of the
    double-precision cosine of the same binary32 angle (the generator's cosf is the build machine's)."""
    G, t = _tool("gen_psnr_hvs_tables"), P.tables()
    csf, mask = G.hvs_tables()
    assert (t["HVS_CSF"] == csf).all() and (t["HVS_MASK"] == mask).all()
    assert (t["HVS_ALPHA"] == np.array([np.sqrt(np.float32(0.125)), np.float32(0.5)], np.float32)).all()
    assert csf.max() == np.float32(2.573509) and mask.max() == np.float32(1.0)
    f = np.float32      # the angle is the reference's binary32 expression; its cosine is the C library's, within one step of the exact one of that angle
    exact = np.array([math.cos(float(f(f(3.14159265358979323846) * f((2 * x + 1) * u)) / f(f(2.0) * f(8.0)))) for u in range(8) for x in range(8)])
    assert (np.abs(t["HVS_COS"].astype(np.float64) - exact) <= 2.0 ** -23).all() and (t["HVS_COS"][:8] == 1.0).all()


def test_python_keywords_exist_and_default_off():
    import inspect
    from basis_universal_amd.compress import compress
    assert inspect.signature(stats.file_stats).parameters["hvs"].default is False
    assert inspect.signature(compress).parameters["stats_hvs"].default is False
    assert callable(stats.psnr_hvs)


def test_live_compare_hvs_on_fresh_pairs():
    """oracle/_ref/basisu -compare_hvs, run now, on pairs no golden holds: the host build reduced in the reference's order reproduces what it prints"""
    G = _tool("gen_golden_psnr_hvs")
    if not G.BASISU.exists():
        pytest.skip("oracle/_ref/basisu is not built here")
    rng = np.random.default_rng()
    for w, h, spread in [(8, 8, 3), (8, 8, 200), (23, 17, 8), (40, 24, 30)]:
        a = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
        b = np.clip(a.astype(np.int64) + rng.integers(-spread, spread + 1, a.shape), 0, 255).astype(np.uint8)
        printed = G.compare_hvs(a, b, f"{w}x{h}")
        hosted = tuple(P.host_blocks(a, b, m) for m in range(6))
        P.assert_close_to_printed(P.printed_from_running(hosted), printed, f"live {w}x{h} spread {spread}: a = {a.tobytes().hex()} b = {b.tobytes().hex()}")
