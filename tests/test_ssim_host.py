"""The host build of csrc/ssim.h and csrc/ssim_reduce.h (tests/native/ssim_host.cpp) against what the reference tool printed (tests/golden/ssim_vectors.npz), and the
reduction's chunked walk against the serial float sum. No GPU, nothing from oracle/_ref. No tolerance: printed text equals printed text, sums are equal bit for bit."""
import numpy as np
import pytest

import ssim_helpers as H

f32 = np.float32
NAMES = [p[0] for p in H.pair_names()]


def test_golden_file_has_every_pair():
    got = [name for name, _, _, _ in H.golden_pairs()]
    assert got == NAMES and len(got) == len(H.KINDS) * len(H.SIZES) + 6
    assert all(len(texts) == 7 for _, _, _, texts in H.golden_pairs())


@pytest.mark.parametrize("kind", H.KINDS + ["strip"])
def test_restatement_prints_what_the_tool_printed(kind):
    seen = 0
    for name, a, b, texts in H.golden_pairs():
        if not name.startswith(kind + "_"):
            continue
        seen += 1
        got = H.printed(H.host_ssim_of_golden(name))
        assert got == texts, (name, got, texts)
        if kind == "identical":
            assert got == ("1.000000",) * 7
    assert seen >= 6


def test_inverted_pairs_have_negative_figures():
    assert any(t.startswith("-") for name, _, _, texts in H.golden_pairs() if name.startswith("inverted_") for t in texts)


def test_weights_sum_to_one_and_are_symmetric():
    w = H.host_weights().reshape(11, 11)
    assert abs(float(w.astype(np.float64).sum()) - 1.0) < 121 * 2.0 ** -24      # 121 weights, each rounded to binary32 once
    assert (w == w.T).all() and (w == w[::-1]).all() and (w == w[:, ::-1]).all()
    assert w.argmax() == 60 and (w > 0).all() and w[5, 5] > w[5, 4] > w[5, 0]


def test_the_frontend_library_hands_out_the_same_weights():
    import ctypes as C
    from basis_universal_amd.etc1s import load_frontend_library
    out = np.zeros(121, f32)
    assert load_frontend_library().bu_ssim_gaussian_weights(out.ctypes.data_as(C.c_void_p)) == 1
    assert out.tobytes() == H.host_weights().tobytes()
    assert load_frontend_library().bu_ssim_gaussian_weights(None) == 0


def test_map_is_clamped_to_the_region_and_honours_pitches():
    rng = np.random.default_rng(11)
    a = rng.integers(0, 256, (9, 13, 4), dtype=np.uint8)
    b = rng.integers(0, 256, (12, 10, 4), dtype=np.uint8)
    cropped_a, cropped_b = np.ascontiguousarray(a[:9, :10]), np.ascontiguousarray(b[:9, :10])
    for mode in range(3):
        tight = H.host_map(cropped_a, cropped_b, mode)
        assert H.host_map(a, b, mode, 17, 10).tobytes() == tight.tobytes()
    lum = H.host_map(cropped_a, cropped_b, 1)
    assert lum.shape == (9, 10) and H.host_map(cropped_a, cropped_b, 0).shape == (9, 10, 4)


def addend_sets():
    """name -> f32 addends: smap-like values, and the cases the shortcut must leave to plain adds"""
    rng = np.random.default_rng(5)
    n = H.chunk_length()
    near_one = (1.0 - rng.random(40 * n) * 0.1).astype(f32)
    out = {
        "near_one": near_one,
        "ones": np.ones(33 * n + 7, f32),
        "negative": (-near_one[:20 * n]).copy(),
        "mixed_signs": (rng.random(30 * n) * 2.0 - 1.0).astype(f32),
        # up to +40, down through zero to -40, and back: sign crossings and every binade on the way, twice
        "sign_crossing": np.concatenate([np.full(40, 1.0, f32), np.full(90 * n, -0.00390625 * 1.37, f32), (rng.random(50 * n) * 0.9).astype(f32)]),
        "binade_crossing": (rng.random(70 * n) * 0.999).astype(f32),           # 2^0 .. 2^14 on the way up
        "tiny_then_large": np.concatenate([np.full(3 * n, 1e-30, f32), near_one[:5 * n]]),
        "zeros": np.zeros(5 * n + 3, f32),
        "short": near_one[:n - 1].copy(),
        "one_chunk": near_one[:n].copy(),
        "one_over": near_one[:n + 1].copy(),
        "large_addend_among_small": np.concatenate([near_one[:6 * n] * f32(0.001), np.array([3000.0], f32), near_one[:6 * n]]),
    }
    return out


ADDENDS = addend_sets()


@pytest.mark.parametrize("name", list(ADDENDS))
def test_chunked_walk_equals_the_serial_sum(name):
    v = ADDENDS[name]
    expect = H.serial_sum(v)
    for chunk in (H.chunk_length(), 64):
        got, chunks, walked = H.chunked_sum(v, chunk)
        assert got.tobytes() == expect.tobytes(), (name, chunk, float(got), float(expect))
        assert chunks == -(-v.size // chunk) and walked <= chunks


def test_chunked_walk_takes_the_shortcut_where_it_can():
    """a long sum of smap-like values: most chunks are applied as a stretch; the ones added one by one are the first few (the state is still small against the
    addends) and the binade crossings"""
    got, chunks, walked = H.chunked_sum(ADDENDS["near_one"])
    assert got.tobytes() == H.serial_sum(ADDENDS["near_one"]).tobytes()
    assert chunks == 40 and walked <= 16, (chunks, walked)


@pytest.mark.parametrize("scale", [0.0, 0.25, 4.0, -1.0])
def test_a_bad_guess_costs_time_not_bits(scale):
    for name in ("near_one", "sign_crossing", "mixed_signs"):
        v = ADDENDS[name]
        got, chunks, walked = H.chunked_sum(v, prefix_scale=scale)
        assert got.tobytes() == H.serial_sum(v).tobytes(), (name, scale)


def test_random_chunks_of_random_addends():
    rng = np.random.default_rng(77)
    for trial in range(200):
        n = int(rng.integers(1, 3000))
        scale = f32(10.0 ** rng.integers(-3, 3))
        v = ((rng.random(n) - rng.choice([0.0, 0.2, 0.5, 1.0])) * scale).astype(f32)
        chunk = int(rng.choice([16, 64, 256, 512]))
        got, _, _ = H.chunked_sum(v, chunk)
        assert got.tobytes() == H.serial_sum(v).tobytes(), (trial, n, chunk)


def test_mean_of_an_identical_pair_stalls_at_two_to_the_24():
    """what avg_image does from 2^24 pixels on: the running sum of ones stops at 16777216, so the mean of an identical pair falls below 1. The reduction reproduces it."""
    n = (1 << 24) + 4096
    v = np.ones(n, f32)
    got, chunks, walked = H.chunked_sum(v)
    assert float(got) == 16777216.0 and got.tobytes() == H.serial_sum(v).tobytes()
    assert "%f" % float(got / f32(n)) == "0.999756"
