"""-m gpu: the image-metrics kernel (csrc/image_metrics_kernels.hip) against numpy -- exact counts --, the C ABI's refusals, stats.file_stats on every golden
file against the numbers the reference tool printed (tests/golden/image_stats_vectors.npz), compress(..., stats=[]) and one Kodak image at size."""
import ctypes as C
import json
import pathlib

import numpy as np
import pytest

import helpers
import image_metrics_helpers as M
from basis_universal_amd import mipmap, stats
from basis_universal_amd.compress import compress

pytestmark = pytest.mark.gpu
HERE = pathlib.Path(__file__).resolve().parent


def check_counts(ctx, a, b):
    hist, sa, sb, w, h = stats.image_counts(ctx, a, b)
    eh, ea, eb = M.np_counts(a, b)
    assert (w, h) == (min(a.shape[1], b.shape[1]), min(a.shape[0], b.shape[0]))
    assert (hist == eh).all() and (sa == ea).all() and (sb == eb).all()


@pytest.mark.parametrize("w,h", [(1, 1), (4, 4), (5, 7), (255, 257), (1024, 1024)])
@pytest.mark.parametrize("near", [True, False], ids=["near", "far"])
def test_counts_are_exact(hip_ctx, w, h, near):
    check_counts(hip_ctx, *M.random_pair(w, h, 1000 + w, near))


def test_region_is_the_minimum_of_each_dimension(hip_ctx):
    a, _ = M.random_pair(40, 30, 1)
    b, _ = M.random_pair(37, 33, 2)
    check_counts(hip_ctx, a, b)
    got = stats.image_metrics(hip_ctx, a, b)
    assert (got["width"], got["height"]) == (37, 30)


def test_unaligned_rows_and_poisoned_padding(hip_ctx):
    """both rasters with 3 pixels of pitch padding (61 of 64), the first starting one pixel into its allocation and the second two: no row of either starts on
    16 bytes, and the padding (0xA5) must not be counted. Then with pitch 63, where the row starts take every 4-byte residue in turn."""
    ctx = hip_ctx
    a, b = M.random_pair(61, 19, 9)
    eh, ea, eb = M.np_counts(a, b)
    for pitch, lead_a, lead_b in [(64, 1, 2), (63, 0, 0)]:
        ra = np.concatenate([np.full((lead_a, 4), 0xA5, np.uint8), M.padded(a, pitch).reshape(-1, 4)])   # poison pixels in front
        rb = np.concatenate([np.full((lead_b, 4), 0xA5, np.uint8), M.padded(b, pitch).reshape(-1, 4)])
        da, db = ctx.upload(ra), ctx.upload(rb)
        try:
            assert da % 16 == 0 and db % 16 == 0
            hist, sa, sb, w, h = stats.image_counts(ctx, (da + 4 * lead_a, 61, 19, pitch), (db + 4 * lead_b, 61, 19, pitch))
        finally:
            ctx.free(da); ctx.free(db)
        assert (w, h) == (61, 19) and (hist == eh).all() and (sa == ea).all() and (sb == eb).all(), pitch


@pytest.mark.parametrize("kind", ["equal", "black_white"])
def test_one_bin_at_full_contention(hip_ctx, kind):
    """2^20 pixels that all land in one bin of every row: the most same-address contention there is, and where a narrow partial counter would wrap. Twice: the
    counts do not depend on the order of accumulation."""
    n = 1024
    if kind == "equal":
        a = np.random.default_rng(3).integers(0, 256, (n, n, 4), dtype=np.uint8)
        b, bin_ = a.copy(), 0
    else:
        a, b, bin_ = np.zeros((n, n, 4), np.uint8), np.full((n, n, 4), 255, np.uint8), 255
    da, db = hip_ctx.upload(a), hip_ctx.upload(b)
    try:
        runs = [stats.image_counts(hip_ctx, (da, n, n, n), (db, n, n, 0)) for _ in range(2)]
    finally:
        hip_ctx.free(da); hip_ctx.free(db)
    hist, sa, sb, _, _ = runs[0]
    expect = np.zeros((6, 256), np.uint32)
    expect[:, bin_] = 1 << 20
    assert (hist == expect).all()
    assert (sa == a.reshape(-1, 4).sum(0, dtype=np.uint64)).all() and (sb == b.reshape(-1, 4).sum(0, dtype=np.uint64)).all()
    assert all((runs[0][k] == runs[1][k]).all() for k in range(3))


def test_empty_region_counts_nothing(hip_ctx):
    d = hip_ctx.upload(np.zeros((4, 4, 4), np.uint8))
    try:
        hist, sa, sb, w, h = stats.image_counts(hip_ctx, (d, 0, 4, 4), (d, 4, 4, 4))
    finally:
        hip_ctx.free(d)
    assert (w, h) == (0, 4) and not hist.any() and not sa.any() and not sb.any()


def test_refusals_leave_the_output_alone(hip_ctx):
    ctx = hip_ctx
    d = ctx.upload(np.zeros((8, 8, 4), np.uint8))
    try:
        def call(da, wa, ha, pa, db, wb, hb, pb, null_out=False):
            c = stats.Counts()
            C.memset(C.byref(c), 0x5A, C.sizeof(c))
            c.struct_bytes = C.sizeof(c)
            before = bytes(c)
            ok = ctx.lib.k_image_metrics(ctx.h, C.c_void_p(da), wa, ha, pa, C.c_void_p(db), wb, hb, pb, None if null_out else C.byref(c))
            return ok, ctx.lib.last_error(ctx.h), bytes(c) == before
        for args, word in [((None, 8, 8, 8, d, 8, 8, 8), "null"), ((d, 8, 8, 8, None, 8, 8, 8), "null"), ((d, 8, 8, 7, d, 8, 8, 8), "pitch"), ((d, 8, 8, 8, d, 8, 8, 5), "pitch"),
                           ((d + 2, 4, 4, 4, d, 8, 8, 8), "aligned")]:
            ok, err, untouched = call(*args)
            assert ok == 0 and word in err and untouched, (args, err)
        ok, err, _ = call(d, 8, 8, 8, d, 8, 8, 8, null_out=True)
        assert ok == 0 and "null" in err
        ok, err, untouched = call(d, 8, 8, 8, d, 8, 8, 0)
        assert ok == 1 and not untouched
    finally:
        ctx.free(d)


def test_a_caller_with_a_shorter_struct_gets_only_its_bytes(hip_ctx):
    ctx = hip_ctx
    a, b = M.random_pair(16, 16, 4)
    da, db = ctx.upload(a), ctx.upload(b)
    try:
        c = stats.Counts()
        C.memset(C.byref(c), 0x5A, C.sizeof(c))
        c.struct_bytes = 16 + 4 * 256 * 4       # a header that ends after the four channel rows
        assert ctx.lib.k_image_metrics(ctx.h, C.c_void_p(da), 16, 16, 0, C.c_void_p(db), 16, 16, 0, C.byref(c)) == 1
    finally:
        ctx.free(da); ctx.free(db)
    hist = np.ctypeslib.as_array(c.hist)
    assert (hist[:4] == M.np_counts(a, b)[0][:4]).all() and (hist[4:] == 0x5A5A5A5A).all() and c.sum_a[0] == 0x5A5A5A5A5A5A5A5A


# ---------------------------------------------------------------- files

def cases():
    return M.golden()[1]["cases"]


@pytest.fixture(scope="module")
def mip_sources(hip_ctx):
    """the source of every level of the 20x28 mip case, made on the device as compress() makes them"""
    src = M.golden()[0]["src_etc1s_mip_basis"]
    return [np.array(src)] + mipmap.generate_mipmaps(hip_ctx, src, has_alpha=False)


def sources_of(case, mip_sources):
    return mip_sources if "-mipmap" in case["args"] else [np.array(M.golden()[0]["src_" + case["name"]])]


@pytest.mark.parametrize("case", cases(), ids=[c["name"] for c in cases()])
def test_file_stats_match_what_the_reference_tool_printed(hip_ctx, case, mip_sources):
    arrays, _ = M.golden()
    printed = arrays["stats_" + case["name"]]
    got = stats.file_stats(hip_ctx, arrays["file_" + case["name"]], sources_of(case, mip_sources))
    assert len(got) == case["slices"] == printed.shape[0]
    for k, s in enumerate(got):
        M.assert_close_to_printed(s, printed[k], f"{case['name']} slice {k}")


def test_file_stats_take_resident_sources(hip_ctx):
    arrays, _ = M.golden()
    src = np.array(arrays["src_etc1s_alpha_basis"])
    d = hip_ctx.upload(M.padded(src, 35))
    try:
        resident = stats.file_stats(hip_ctx, arrays["file_etc1s_alpha_basis"], {(0, 0, 0): (d, 32, 24, 35)})
    finally:
        hip_ctx.free(d)
    assert resident == stats.file_stats(hip_ctx, arrays["file_etc1s_alpha_basis"], [src])


@pytest.mark.parametrize("name,mipmaps", [("etc1s_mip_basis", True), ("etc1s_alpha_basis", False)])
def test_compress_fills_stats(hip_ctx, name, mipmaps, mip_sources):
    arrays, meta = M.golden()
    case = next(c for c in meta["cases"] if c["name"] == name)
    src, printed = np.array(arrays["src_" + name]), arrays["stats_" + name]
    filled, kv = [], helpers.basis_file_key_values(arrays["file_" + name])   # the tool's own key-values (its library version)
    data = compress(hip_ctx, src, quality=128, mipmaps=mipmaps, key_values=kv, stats=filled)
    assert data.tobytes() == arrays["file_" + name].tobytes()
    assert compress(hip_ctx, src, quality=128, mipmaps=mipmaps, key_values=kv).tobytes() == data.tobytes()
    assert filled == stats.file_stats(hip_ctx, data, sources_of(case, mip_sources))
    assert len(filled) == printed.shape[0]
    for k, s in enumerate(filled):
        M.assert_close_to_printed(s, printed[k], f"{name} slice {k}")


def test_kodak_image_at_size(hip_ctx):
    """768x512 through compress(quality=128, stats=[]): the RGBA PSNR the stats stage reports against the committed figure of the reference for the same
    configuration, to the tolerance tests/test_gpu_kodak24.py holds the host-side figure to"""
    golden = json.loads((HERE / "golden" / "kodak24_digests.json").read_text())["images"]["k03"]["etc1s_q128"]
    rgb = np.load(HERE / "golden" / "kodak24.npz")["k03"]
    img = np.concatenate([rgb, np.full(rgb.shape[:2] + (1,), 255, np.uint8)], axis=2)
    filled = []
    compress(hip_ctx, img, quality=128, stats=filled)
    assert len(filled) == 1 and (filled[0]["width"], filled[0]["height"]) == (768, 512)
    assert abs(filled[0]["rgba"]["psnr"] - golden["psnr_rgba"]) < 1e-3, filled[0]["rgba"]["psnr"]
