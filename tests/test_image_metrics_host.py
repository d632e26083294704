"""CPU (-m "not gpu"): the arithmetic the image-metrics kernel counts with and the reduction the host library exports (csrc/image_metrics.h), under a serial loop:
exact counts against numpy, the reduced figures bit for bit against a double / float32 restatement of image_metrics::calc, and the numbers the reference tool
printed for the single-level golden files, from host decodes of those files."""
import numpy as np
import pytest

import helpers
import image_metrics_helpers as M
from basis_universal_amd import stats

SHAPES = [(1, 1, 0), (5, 7, 3), (64, 48, 5)]   # width, height, pixels of pitch padding


def degenerate(w=64, h=48):
    rng = np.random.default_rng(5)
    a = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    return {"equal": (a, a.copy()), "black_white": (np.zeros((h, w, 4), np.uint8), np.full((h, w, 4), 255, np.uint8))}


@pytest.mark.parametrize("w,h,pad", SHAPES)
@pytest.mark.parametrize("near", [True, False])
def test_counts_match_numpy(w, h, pad, near):
    a, b = M.random_pair(w, h, 100 + w, near)
    hist, sa, sb = M.host_counts(a, b, w + pad, w + 2 * pad)
    eh, ea, eb = M.np_counts(a, b)
    assert (hist == eh).all() and (sa == ea).all() and (sb == eb).all()
    assert (hist.sum(1) == w * h).all()


def test_counts_crop_to_the_smaller_image():
    a, _ = M.random_pair(40, 30, 1)
    b, _ = M.random_pair(37, 33, 2)
    hist, sa, sb = M.host_counts(a, b, 43, 40)
    eh, ea, eb = M.np_counts(a, b)
    assert (hist == eh).all() and (sa == ea).all() and (sb == eb).all() and hist[0].sum() == 37 * 30


def reduction_inputs():
    out = [(f"{w}x{h}_{'near' if near else 'far'}", *M.random_pair(w, h, 7 + w, near)) for w, h, _ in SHAPES for near in (True, False)]
    return out + [(k, *v) for k, v in degenerate().items()]


@pytest.mark.parametrize("name,a,b", reduction_inputs(), ids=[r[0] for r in reduction_inputs()])
def test_reduction_is_the_reference_expression_bit_for_bit(name, a, b):
    h, w = a.shape[:2]
    hist, _, _ = M.host_counts(a, b)
    product = stats.reduce_counts(hist, w, h)       # libbasisu_frontend.so's exported function
    for line, (first, total, use_601) in M.LINES.items():
        got, exp = M.host_reduce(hist, total, first, w, h, use_601), M.np_reduce(hist, total, first, w, h, use_601)
        for k in ("max", "mean", "mean_squared", "rms", "psnr"):
            assert np.float64(got[k]).tobytes() == np.float64(exp[k]).tobytes(), (line, k, got[k], exp[k])
        for k in M.FIGURES:
            assert np.float64(product[line][k]).tobytes() == np.float64(exp[k]).tobytes(), (line, k)
    assert abs(product["rgba"]["psnr"] - helpers.psnr(a, b)) <= 1e-6
    if name == "equal":
        assert all(product[line]["psnr"] == 100.0 and product[line]["max"] == 0.0 and product[line]["rms"] == 0.0 for line in M.LINES)
    if name == "black_white":
        assert (hist[:, 255] == w * h).all() and hist.sum() == 6 * w * h
        assert all(product[line]["psnr"] == 0.0 and product[line]["max"] == 255.0 and product[line]["mean"] == 255.0 for line in M.LINES)


def test_reduce_refuses_bad_arguments():
    import ctypes as C
    L = stats._reduce_lib()
    hist, m = np.zeros((6, 256), np.uint32), stats._Metrics()
    assert L.bu_image_metrics_reduce(None, 3, 0, 4, 4, 0, C.byref(m)) == 0
    assert L.bu_image_metrics_reduce(hist.ctypes.data, 3, 2, 4, 4, 0, C.byref(m)) == 0     # channels 2..4
    assert L.bu_image_metrics_reduce(hist.ctypes.data, 1, 3, 4, 4, 0, None) == 0
    assert L.bu_image_metrics_reduce(hist.ctypes.data, 1, 3, 4, 4, 0, C.byref(m)) == 1


def single_level_cases():
    return [c for c in M.golden()[1]["cases"] if "-mipmap" not in c["args"]]


@pytest.mark.parametrize("case", single_level_cases(), ids=[c["name"] for c in single_level_cases()])
def test_golden_numbers_from_a_host_decode(case):
    """Every number the reference tool printed for the file, reproduced within M.PRINT_TOLERANCE (0.00055: half a unit of the third decimal the tool prints for all
    four figures, plus slack for its float-to-text rounding) from a decode of the file that needs no GPU."""
    arrays, _ = M.golden()
    printed = arrays["stats_" + case["name"]]
    slices = M.host_slices(case)
    assert len(slices) == case["slices"] == printed.shape[0]
    for k, (src, dec) in enumerate(slices):
        hist, _, _ = M.host_counts(src, dec)
        M.assert_close_to_printed(stats.reduce_counts(hist, src.shape[1], src.shape[0]), printed[k], f"{case['name']} slice {k}")
