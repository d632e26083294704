"""-m gpu: the SSIM kernels (csrc/ssim_kernels.hip) against the host restatement of compute_ssim (tests/native/ssim_host.cpp over csrc/ssim.h) -- every smap value and
every figure bit for bit --, stats.ssim / file_stats(ssim=True) / compress(stats_ssim=True) against the text the reference tool printed
(tests/golden/ssim_vectors.npz), and the keyword off. No tolerance anywhere. Nothing from oracle/_ref."""
import ctypes as C

import numpy as np
import pytest

import image_metrics_helpers as M
import ssim_helpers as H
from basis_universal_amd import stats
from basis_universal_amd.compress import compress

pytestmark = pytest.mark.gpu
f32 = np.float32


def pair(w, h, seed, kind="near"):
    a, b = H.make_pair(kind, w, h, seed)
    return a, b


# 100x52 is 7 x 4 tiles with ragged right and bottom tiles; 512x384 is 768 chunks per plane, with binade crossings of the running sum up to 2^17
PARITY = {"5x7": pair(5, 7, 31), "20x28": pair(20, 28, 32), "100x52": pair(100, 52, 33, "unrelated"), "512x384": pair(512, 384, 34)}


def resident(ctx, img, pitch):
    return ctx.upload(M.padded(img, pitch)), img.shape[1], img.shape[0], pitch


@pytest.fixture(scope="module")
def host_maps():
    """the host restatement's smap values of the parity pairs, computed once"""
    return {(name, mode): H.host_map(a, b, mode) for name, (a, b) in PARITY.items() for mode in range(3)}


def assert_same_bits(got, expect, what):
    assert got.shape == expect.shape and got.dtype == expect.dtype == f32, (what, got.shape, expect.shape)
    wrong = np.argwhere(got.view(np.uint32) != expect.view(np.uint32))
    assert wrong.size == 0, (what, len(wrong), wrong[:4].tolist(), [float(got[tuple(i)]) for i in wrong[:4]], [float(expect[tuple(i)]) for i in wrong[:4]])


@pytest.mark.parametrize("name", list(PARITY))
def test_map_equals_the_restatement_bit_for_bit(hip_ctx, host_maps, name):
    a, b = PARITY[name]
    ra, rb = resident(hip_ctx, a, a.shape[1]), resident(hip_ctx, b, b.shape[1])
    try:
        for mode in range(3):
            assert_same_bits(stats.ssim_map(hip_ctx, ra, rb, mode), host_maps[(name, mode)], (name, stats.SSIM_MODES[mode]))
    finally:
        hip_ctx.free(ra[0]); hip_ctx.free(rb[0])


def means_of_maps(maps, name):
    """the seven figures from the restatement's maps by the serial sum"""
    rgba = maps[(name, 0)]
    n = f32(rgba.shape[0] * rgba.shape[1])
    s = [H.serial_sum(rgba[..., c].reshape(-1)) / n for c in range(4)]
    return np.array([s[0], s[1], s[2], (s[0] + s[1] + s[2]) / f32(3.0), s[3], H.serial_sum(maps[(name, 1)].reshape(-1)) / n, H.serial_sum(maps[(name, 2)].reshape(-1)) / n], f32)


@pytest.mark.parametrize("name", list(PARITY))
def test_figures_equal_the_restatement_bit_for_bit(hip_ctx, host_maps, name):
    a, b = PARITY[name]
    got = stats.ssim(hip_ctx, a, b)
    expect = means_of_maps(host_maps, name)
    print(name, H.printed(H.result_values(got)), H.printed(expect))
    assert (got["width"], got["height"]) == (a.shape[1], a.shape[0])
    assert H.result_values(got).tobytes() == expect.tobytes(), (name, H.result_values(got).tolist(), expect.tolist())


def test_the_large_pair_takes_the_shortcut_and_is_repeatable(hip_ctx):
    a, b = PARITY["512x384"]
    runs = [stats.ssim_result(hip_ctx, a, b) for _ in range(2)]
    assert bytes(runs[0]) == bytes(runs[1])
    s = runs[0]
    print("chunks", s.chunks, "walked", s.chunks_walked)
    assert s.chunks == 6 * -(-512 * 384 // H.chunk_length())
    # per plane: the first chunk (the state starts at zero), the second (the state is within a factor of four of an addend) and at most one chunk per binade
    # crossing up to 2^18 may need plain adds; everything else must have been applied as a stretch
    assert s.chunks_walked <= 6 * 20, (s.chunks, s.chunks_walked)


def test_strips_around_the_chunk_length_equal_the_restatement(hip_ctx):
    for name, a, b, texts in H.golden_pairs():
        if not name.startswith("strip_"):
            continue
        got = H.result_values(stats.ssim(hip_ctx, np.array(a), np.array(b)))
        assert got.tobytes() == H.host_ssim_of_golden(name).tobytes(), (name, got.tolist())


def test_ssim_prints_what_the_tool_printed_on_every_golden_pair(hip_ctx):
    for name, a, b, texts in H.golden_pairs():
        got = stats.ssim(hip_ctx, np.array(a), np.array(b))
        assert (got["width"], got["height"]) == (a.shape[1], a.shape[0])
        assert all(isinstance(got[k], float) for k in H.FIGURES)
        assert H.printed(H.result_values(got)) == texts, (name, H.printed(H.result_values(got)), texts)
        if name.startswith("identical_"):
            assert all(got[k] == 1.0 for k in H.FIGURES), name


def test_padded_pitches_and_different_sizes_give_the_cropped_result(hip_ctx):
    ctx = hip_ctx
    rng = np.random.default_rng(41)
    a = rng.integers(0, 256, (37, 53, 4), dtype=np.uint8)
    b = np.clip(rng.integers(-9, 10, (45, 41, 4)) + np.pad(a, ((0, 8), (0, 0), (0, 0)), mode="edge")[:45, :41], 0, 255).astype(np.uint8)
    tight_a, tight_b = np.ascontiguousarray(a[:37, :41]), np.ascontiguousarray(b[:37, :41])
    expect = stats.ssim(ctx, tight_a, tight_b)
    assert (expect["width"], expect["height"]) == (41, 37)
    assert H.result_values(expect).tobytes() == H.host_ssim(tight_a, tight_b).tobytes()
    ra, rb = resident(ctx, a, 64), resident(ctx, b, 47)
    try:
        assert stats.ssim(ctx, ra, rb) == expect
        assert stats.ssim(ctx, (ra[0], 53, 37, 64), (rb[0], 41, 45, 47)) == expect
        for mode in range(3):
            assert_same_bits(stats.ssim_map(ctx, ra, rb, mode), H.host_map(tight_a, tight_b, mode), ("padded", mode))
    finally:
        ctx.free(ra[0]); ctx.free(rb[0])
    assert stats.ssim(ctx, a, b) == expect                       # tight arrays of different sizes: pitch 0 -> the width


def case(name):
    (c,) = [c for c in M.golden()[1]["cases"] if c["name"] == name]
    return c


def pick_cases():
    """one UASTC and one ETC1S case of image_stats_vectors.npz, neither with mipmaps"""
    cases = [c for c in M.golden()[1]["cases"] if "-mipmap" not in c["args"]]
    return [next(c for c in cases if c["uastc"]), next(c for c in cases if not c["uastc"])]


def without_ssim(slices):
    out = []
    for s in slices:
        s = {k: v for k, v in s.items() if k != "ssim"}
        if "bc7" in s:
            s["bc7"] = {k: v for k, v in s["bc7"].items() if k != "ssim"}
        out.append(s)
    return out


def decoded_slices(ctx, data, src, uastc):
    """every slice of the file as (source (h, w, 4) u8, decode (h, w, 4) u8), by the package's own decoders"""
    from basis_universal_amd import transcode
    raw = bytes(np.asarray(data).tobytes())
    out = []
    if uastc:
        info = transcode.read_uastc_file(raw)
        for k in stats._slice_order(info["images"]):
            im = info["images"][k]
            blocks = np.frombuffer(raw, np.uint8, im["length"], im["offset"]).reshape(-1, 16)
            dec = transcode.transcode_uastc_blocks(ctx, blocks, im["num_blocks_x"], im["num_blocks_y"], transcode.RGBA32, width=im["width"], height=im["height"])
            out.append((src, np.asarray(dec).reshape(im["height"], im["width"], 4)))
        return out
    decoded = transcode.decode_etc1s_file(raw)
    for k in stats._slice_order(decoded["images"]):
        im = decoded["images"][k]
        parts, sources = [dict(im, alpha_endpoint_indices=None, alpha_selector_indices=None)], [src]
        if im["has_alpha"]:
            parts.append(dict(im, endpoint_indices=im["alpha_endpoint_indices"], selector_indices=im["alpha_selector_indices"], alpha_endpoint_indices=None,
                              alpha_selector_indices=None))
            sources = list(stats.split_planes(src))
        for part, s in zip(parts, sources):
            dec = transcode.transcode_etc1s_image(ctx, decoded, part, transcode.RGBA32)
            out.append((s, np.asarray(dec).reshape(im["height"], im["width"], 4)))
    return out


@pytest.mark.parametrize("c", pick_cases(), ids=[c["name"] for c in pick_cases()])
def test_file_stats_ssim_is_ssim_of_every_slice(hip_ctx, c):
    arrays, _ = M.golden()
    data, src = arrays["file_" + c["name"]], np.array(arrays["src_" + c["name"]])
    got = stats.file_stats(hip_ctx, data, [src], ssim=True)
    pairs = decoded_slices(hip_ctx, data, src, c["uastc"])
    assert len(got) == c["slices"] == len(pairs)
    for k, (s, (source, decode)) in enumerate(zip(got, pairs)):
        assert s["ssim"] == stats.ssim(hip_ctx, source, decode), (c["name"], k)
        assert (s["ssim"]["width"], s["ssim"]["height"]) == (s["width"], s["height"])
    # the keyword off: today's dicts, with and without naming it
    plain = stats.file_stats(hip_ctx, data, [src])
    assert plain == stats.file_stats(hip_ctx, data, [src], ssim=False) == without_ssim(got) and all("ssim" not in s for s in plain)
    for k, s in enumerate(plain):
        M.assert_close_to_printed(s, arrays["stats_" + c["name"]][k], f"{c['name']} slice {k}")
    if c["uastc"]:
        both = stats.file_stats(hip_ctx, data, [src], ssim=True, bc7=True)
        assert all("ssim" in s["bc7"] and s["bc7"]["ssim"] != s["ssim"] and s["ssim"] == g["ssim"] for s, g in zip(both, got))
        assert without_ssim(both) == stats.file_stats(hip_ctx, data, [src], bc7=True)
    else:
        with pytest.raises(ValueError, match="UASTC files only"):
            stats.file_stats(hip_ctx, data, [src], ssim=True, bc7=True)


def test_compress_with_stats_ssim_writes_the_same_bytes(hip_ctx):
    src = np.array(M.golden()[0]["src_" + pick_cases()[0]["name"]])
    for options in ({"uastc": True, "ktx2": True}, {"quality": 128}):     # the source has alpha: UASTC with alpha is a .ktx2 here
        with_ssim, plain = [], []
        data = compress(hip_ctx, src, stats=with_ssim, stats_ssim=True, **options)
        assert compress(hip_ctx, src, stats=plain, **options).tobytes() == data.tobytes() == compress(hip_ctx, src, **options).tobytes()
        assert compress(hip_ctx, src, stats_ssim=True, **options).tobytes() == data.tobytes()      # without a stats list the keyword does nothing
        assert plain == without_ssim(with_ssim) and all("ssim" not in s for s in plain) and len(with_ssim) >= 1
        assert with_ssim == stats.file_stats(hip_ctx, data, [src], ssim=True)


def test_refusals_leave_the_output_alone(hip_ctx):
    ctx = hip_ctx
    d = ctx.upload(np.zeros((8, 8, 4), np.uint8))
    try:
        def call(da, wa, ha, pa, db, wb, hb, pb):
            s = stats.SsimResult()
            C.memset(C.byref(s), 0x5A, C.sizeof(s))
            s.struct_bytes = C.sizeof(s)
            before = bytes(s)
            ok = ctx.lib.k_ssim(ctx.h, C.c_void_p(da), wa, ha, pa, C.c_void_p(db), wb, hb, pb, C.byref(s))
            return ok, ctx.lib.last_error(ctx.h), bytes(s) == before
        for args, word in [((None, 8, 8, 8, d, 8, 8, 8), "null"), ((d, 8, 8, 8, None, 8, 8, 8), "null"), ((d, 8, 8, 7, d, 8, 8, 8), "pitch"), ((d, 8, 8, 8, d, 8, 8, 5), "pitch"),
                           ((d, 0, 8, 8, d, 8, 8, 8), "empty"), ((d, 8, 8, 8, d, 8, 0, 8), "empty"), ((d + 2, 4, 4, 4, d, 8, 8, 8), "aligned"),
                           ((d, 16385, 1, 16385, d, 16385, 1, 16385), "too large"), ((d, 8192, 8192, 8192, d, 8192, 8192, 8192), "too large")]:
            ok, err, untouched = call(*args)
            assert ok == 0 and word in err and untouched, (args, err)
        assert ctx.lib.k_ssim(ctx.h, C.c_void_p(d), 8, 8, 8, C.c_void_p(d), 8, 8, 8, None) == 0 and "null" in ctx.lib.last_error(ctx.h)
        ok, _, untouched = call(d, 8, 8, 8, d, 8, 8, 0)
        assert ok == 1 and not untouched
        out = np.zeros(64 * 4, f32)
        po = out.ctypes.data_as(C.c_void_p)
        assert ctx.lib.k_ssim_map(ctx.h, C.c_void_p(d), 8, 8, 8, C.c_void_p(d), 8, 8, 8, 3, po, out.size, None) == 0 and "mode" in ctx.lib.last_error(ctx.h)
        assert ctx.lib.k_ssim_map(ctx.h, C.c_void_p(d), 8, 8, 8, C.c_void_p(d), 8, 8, 8, 0, po, 255, None) == 0 and "room" in ctx.lib.last_error(ctx.h)
        assert ctx.lib.k_ssim_map(ctx.h, C.c_void_p(d), 8, 8, 8, C.c_void_p(d), 8, 8, 8, 0, None, 256, None) == 0 and "null" in ctx.lib.last_error(ctx.h)
        assert ctx.lib.k_ssim_map(ctx.h, C.c_void_p(d), 8, 8, 8, C.c_void_p(d), 8, 0, 8, 1, po, 256, None) == 0 and "empty" in ctx.lib.last_error(ctx.h)
        assert ctx.lib.k_ssim_map(ctx.h, C.c_void_p(d), 8, 8, 8, C.c_void_p(d), 8, 8, 8, 0, po, 256, None) == 1 and (out == 1.0).all()
        with pytest.raises(Exception, match="empty"):
            stats.ssim(ctx, np.zeros((0, 4, 4), np.uint8), np.zeros((4, 4, 4), np.uint8))
    finally:
        ctx.free(d)
