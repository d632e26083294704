"""What the image-metrics tests share: the golden file (tests/golden/image_stats_vectors.npz, written by tools/gen_golden_image_stats.py), the host build of
csrc/image_metrics.h (tests/native/image_metrics_host.cpp), a numpy restatement of image_metrics::calc (encoder/basisu_enc.cpp:2155-2226) -- counts in integers,
the reduction in Python doubles narrowed through float32 where the reference narrows -- and host decodes of the golden files."""
import functools
import math
import pathlib

import numpy as np

import native_libs

ROOT = pathlib.Path(__file__).resolve().parent.parent
GOLDEN = ROOT / "tests" / "golden" / "image_stats_vectors.npz"
LINES = {"rgb": (0, 3, 0), "rgba": (0, 4, 0), "r": (0, 1, 0), "g": (1, 1, 0), "b": (2, 1, 0), "a": (3, 1, 0), "luma_709": (0, 0, 0), "luma_601": (0, 0, 1)}
FIGURES = ["max", "mean", "rms", "psnr"]
# The tool prints every figure with three decimals ({3.3} / {2.3}; the generator asserts it): half a unit of the last one, plus slack for its float-to-text rounding.
# From the print precision, not from a measurement.
PRINT_TOLERANCE = 0.00055


def host():
    return native_libs.load("image_metrics_host")


@functools.lru_cache(maxsize=None)
def golden():
    """-> (arrays, meta): loaded once and shared; nobody writes into the arrays"""
    return native_libs.load_npz_golden(GOLDEN)


def padded(img, pitch):
    """(h, w, 4) -> a C-contiguous (h, pitch, 4) raster holding it, the padding poisoned with 0xA5"""
    h, w = img.shape[:2]
    out = np.full((h, pitch, 4), 0xA5, np.uint8)
    out[:, :w] = img
    return out


def host_counts(a, b, pitch_a=None, pitch_b=None):
    """the serial loop of the native unit over two (h, w, 4) u8 images (pitch > w: rows padded with poison) -> (hist (6, 256) u32, sum_a, sum_b (4,) u64)"""
    (ha, wa), (hb, wb) = a.shape[:2], b.shape[:2]
    pa, pb = pitch_a or wa, pitch_b or wb
    ra, rb = padded(a, pa), padded(b, pb)
    hist, sa, sb = np.zeros((6, 256), np.uint32), np.zeros(4, np.uint64), np.zeros(4, np.uint64)
    host().imh_counts(ra.ctypes.data, wa, ha, pa, rb.ctypes.data, wb, hb, pb, hist.ctypes.data, sa.ctypes.data, sb.ctypes.data)
    return hist, sa, sb


def host_reduce(hist, total_chans, first_chan, width, height, use_601):
    out = np.zeros(5, np.float64)
    hist = np.ascontiguousarray(hist, np.uint32)
    host().imh_reduce(hist.ctypes.data, total_chans, first_chan, width, height, use_601, out.ctypes.data)
    return dict(zip(["max", "mean", "mean_squared", "rms", "psnr"], out.tolist()))


def np_luma(img, weights):
    r, g, b = (img[..., k].astype(np.int64) for k in range(3))
    return (weights[0] * r + weights[1] * g + weights[2] * b + 32768) >> 16


def np_counts(a, b):
    """numpy restatement: the region both cover -> (hist (6, 256) u32, sum_a, sum_b (4,) u64)"""
    h, w = min(a.shape[0], b.shape[0]), min(a.shape[1], b.shape[1])
    a, b = a[:h, :w], b[:h, :w]
    rows = [np.abs(a[..., c].astype(np.int64) - b[..., c].astype(np.int64)) for c in range(4)]
    rows.append(np.abs(np_luma(a, (13938, 46869, 4729)) - np_luma(b, (13938, 46869, 4729))))
    rows.append(np.abs(np_luma(a, (19595, 38470, 7471)) - np_luma(b, (19595, 38470, 7471))))
    hist = np.stack([np.bincount(r.reshape(-1), minlength=256) for r in rows]).astype(np.uint32)
    return hist, a.reshape(-1, 4).sum(0, dtype=np.uint64), b.reshape(-1, 4).sum(0, dtype=np.uint64)


def np_reduce(hist, total_chans, first_chan, width, height, use_601):
    """image_metrics::calc from its histogram on: Python floats are doubles, np.float32 narrows where the reference assigns to a float"""
    rows = range(first_chan, first_chan + total_chans) if total_chans else [5 if use_601 else 4]
    h = [float(sum(int(hist[r][i]) for r in rows)) for i in range(256)]
    mx, s, s2 = 0.0, 0.0, 0.0
    for i in range(256):
        if h[i]:
            mx = max(mx, float(i))
            v = i * h[i]
            s += v
            s2 += i * v
    total = float(width) * float(height) * float(min(max(total_chans, 1), 4))
    mean = np.float32(min(max(s / total, 0.0), 255.0))
    mean_squared = np.float32(min(max(s2 / total, 0.0), 255.0 * 255.0))
    rms = np.float32(math.sqrt(float(mean_squared)))
    psnr = np.float32(min(max(math.log10(255.0 / float(rms)) * 20.0, 0.0), 100.0)) if rms else np.float32(100.0)
    return {"max": mx, "mean": float(mean), "mean_squared": float(mean_squared), "rms": float(rms), "psnr": float(psnr)}


def random_pair(w, h, seed, near=True):
    """two random RGBA images; near: b = a + small noise (the differences of a real encode, piled into the low bins), else unrelated (every bin)"""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    if near:
        b = np.clip(a.astype(np.int64) + rng.integers(-6, 7, (h, w, 4)), 0, 255).astype(np.uint8)
    else:
        b = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    return a, b


def assert_close_to_printed(got, printed, what):
    """got: a stats dict (stats.image_metrics / reduce_counts); printed: (8, 4) of the tool's numbers. Every figure within PRINT_TOLERANCE."""
    for li, line in enumerate(LINES):
        for fi, fig in enumerate(FIGURES):
            assert abs(got[line][fig] - printed[li][fi]) <= PRINT_TOLERANCE, (what, line, fig, got[line][fig], float(printed[li][fi]))


def split_planes(img):
    colour = img.copy(); colour[..., 3] = 255
    alpha = np.repeat(img[..., 3:4], 4, axis=2); alpha[..., 3] = 255
    return colour, alpha


def host_slices(case):
    """a single-level golden case decoded without a GPU -> [(source raster, decoded (h, w, 4) raster)] per slice. ETC1S: the file's own palettes and indices
    (decode_etc1s_file, host code) put together as ETC1 blocks and decoded by the format definition; UASTC: helpers.host_decode_uastc."""
    import etc1s_transcode_helpers as E
    import helpers
    from basis_universal_amd import transcode
    arrays, _ = golden()
    src, raw = arrays["src_" + case["name"]], arrays["file_" + case["name"]].tobytes()
    if case["uastc"]:
        info = transcode.read_uastc_file(raw)
        (im,) = info["images"]
        blocks = np.frombuffer(raw, np.uint8, im["length"], im["offset"]).reshape(-1, 16)
        dec = helpers.host_decode_uastc(blocks, im["num_blocks_x"], im["num_blocks_y"])[:im["height"], :im["width"]]
        return [(src, np.ascontiguousarray(dec))]
    dec = transcode.decode_etc1s_file(raw)
    (im,) = dec["images"]
    nbx, nby, w, h = im["num_blocks_x"], im["num_blocks_y"], im["width"], im["height"]
    sel16 = (dec["selector_palette"][:, None] >> (2 * np.arange(16, dtype=np.uint32))[None, :]) & 3

    def decode(ei, si):
        blocks = E.etc1s_output_blocks(dec["endpoint_palette"], sel16, ei.reshape(-1), si.reshape(-1))
        rgb = E.decode_etc1_blocks(blocks, nbx, nby)[:h, :w]
        return blocks, np.ascontiguousarray(np.concatenate([rgb, np.full((h, w, 1), 255, np.uint8)], 2))
    blocks, colour = decode(im["endpoint_indices"], im["selector_indices"])
    if case["same_file_as"]:   # the reference tool's own ETC1 transcode of this file, committed with the transcoder's known answers
        ta, _ = E.golden()
        rgb = E.decode_etc1_blocks(ta[E.image_key(case["same_file_as"], 0, 0, 0) + "_etc1"], nbx, nby)[:h, :w]
        assert (rgb == colour[..., :3]).all(), case["name"]
    if not im["has_alpha"]:
        return [(src, colour)]
    _, alpha = decode(im["alpha_endpoint_indices"], im["alpha_selector_indices"])
    return list(zip(split_planes(src), [colour, alpha]))
