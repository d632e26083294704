"""What the PSNR-HVS tests share: the golden file (tests/golden/psnr_hvs_vectors.npz, written by tools/gen_golden_psnr_hvs.py), the host build of csrc/psnr_hvs.h
(tests/native/psnr_hvs_host.cpp) and a numpy restatement of psnr_hvs_compute_chan / psnr_hvs_compute_metrics (encoder/basisu_enc.cpp:2256-2519).

The restatement is vectorised over blocks only: every array is float32 with the blocks on the first axis, every constant an np.float32, and every summation of the
reference is an explicit loop along its axis in the reference's order (never np.sum, whose pairwise order is numpy's own). It reads the committed constant table
(csrc/psnr_hvs_tables.inc)."""
import functools
import math
import pathlib
import re

import numpy as np

import native_libs
from image_metrics_helpers import PRINT_TOLERANCE, padded  # noqa: F401  (the print tolerance is the one argued there: the tool prints these figures with {1.3} too)

ROOT = pathlib.Path(__file__).resolve().parent.parent
GOLDEN = ROOT / "tests" / "golden" / "psnr_hvs_vectors.npz"
TABLES = ROOT / "basis_universal_amd" / "csrc" / "psnr_hvs_tables.inc"
MODES = ["y_601_8bit", "y_601_float", "r", "g", "b", "a"]                          # the order of bu_psnr_hvs_sums
ENTRIES = ["y_601_float", "y_601_8bit", "rgb", "rgba", "r", "g", "b", "a"]         # the order psnr_hvs_print_metrics prints them
REDUCED = ["y_601_8bit", "y_601_float", "r", "g", "b", "a", "rgb", "rgba"]         # the order of bu_psnr_hvs_metrics
FIGURES = ["mseh_hvs", "mseh_hvsm", "psnr_hvs", "psnr_hvsm"]
f32 = np.float32


def host():
    return native_libs.load("psnr_hvs_host")


@functools.lru_cache(maxsize=None)
def golden():
    """-> (arrays, meta): loaded once and shared; nobody writes into the arrays"""
    return native_libs.load_npz_golden(GOLDEN)


@functools.lru_cache(maxsize=None)
def tables():
    """the committed constants -> {"HVS_COS": (64,) f32, "HVS_ALPHA": (2,), "HVS_CSF": (64,), "HVS_MASK": (64,)}"""
    out = {}
    for name, n, body in re.findall(r"BU_HVS_TAB float (\w+)\[(\d+)\] = \{(.*?)\};", TABLES.read_text(), re.S):
        body = re.sub(r"//[^\n]*", "", body)
        vals = np.array([float.fromhex(t[:-1]) for t in body.replace(",", " ").split()], np.float64)
        assert vals.size == int(n) and (vals.astype(f32).astype(np.float64) == vals).all(), name
        out[name] = vals.astype(f32)
    assert sorted(out) == ["HVS_ALPHA", "HVS_COS", "HVS_CSF", "HVS_MASK"]
    return out


def block_count(a, b):
    h, w = min(a.shape[0], b.shape[0]), min(a.shape[1], b.shape[1])
    return ((w + 7) // 8) * ((h + 7) // 8) if w and h else 0


def host_blocks(a, b, mode, pitch_a=None, pitch_b=None):
    """the native unit over two (h, w, 4) u8 images (pitch > w: rows padded with poison) -> (per-block doubles (blocks, 2), running sums (2,) in the reference's order)"""
    (ha, wa), (hb, wb) = a.shape[:2], b.shape[:2]
    pa, pb = pitch_a or wa, pitch_b or wb
    ra, rb = padded(a, pa), padded(b, pb)
    out, running = np.zeros((max(block_count(a, b), 1), 2), np.float64), np.zeros(2, np.float64)
    n = host().phh_blocks(ra.ctypes.data, wa, ha, pa, rb.ctypes.data, wb, hb, pb, mode, out.ctypes.data, running.ctypes.data)
    assert n == block_count(a, b)
    return out[:n], running


def host_reduce(sum_hvs, sum_hvsm, blocks):
    out = np.zeros(32, np.float64)
    sh, sm = np.ascontiguousarray(sum_hvs, np.float64), np.ascontiguousarray(sum_hvsm, np.float64)
    host().phh_reduce(sh.ctypes.data, sm.ctypes.data, blocks, out.ctypes.data)
    return {name: dict(zip(FIGURES, out[4 * k:4 * k + 4].tolist())) for k, name in enumerate(REDUCED)}


# ---------------------------------------------------------------- the numpy restatement

def extract_blocks(img, w, h):
    """(H, W, 4) u8, the region w x h -> (blocks, 64, 4): 8x8 blocks in raster order, coordinates clamped to the image's own edge (extract_block_clamped)"""
    bxs, bys = (w + 7) // 8, (h + 7) // 8
    ys = np.minimum(np.arange(bys * 8), img.shape[0] - 1)
    xs = np.minimum(np.arange(bxs * 8), img.shape[1] - 1)
    full = img[ys][:, xs]
    return full.reshape(bys, 8, bxs, 8, 4).transpose(0, 2, 1, 3, 4).reshape(bys * bxs, 64, 4)


def np_samples(mode, px):
    """(N, 64, 4) u8 -> (N, 64) f32"""
    inv255 = f32(1.0) / f32(255.0)
    r, g, b = (px[..., k].astype(f32) for k in range(3))
    if mode == 0:
        y = f32(16.0) + f32(65.481) * r * inv255 + f32(128.553) * g * inv255 + f32(24.966) * b * inv255
        y8 = np.floor(y.astype(np.float64) + 0.5).astype(np.uint8)      # std::round of a positive float: exact in double
        return y8.astype(f32) * inv255
    if mode == 1:
        return (f32(16.0) + (f32(65.481) / f32(255.0)) * r + (f32(128.553) / f32(255.0)) * g + (f32(24.966) / f32(255.0)) * b) * inv255
    return px[..., mode - 2].astype(f32) * inv255


def np_dct(block):
    """dct2f::forward: (N, 64) -> (N, 64)"""
    t = tables()
    cos, alpha = t["HVS_COS"].reshape(8, 8), t["HVS_ALPHA"]
    src = block.reshape(-1, 8, 8)
    work = np.zeros_like(src)
    for v in range(8):                      # horizontal: work[row][v] = (sum over y of src[row][y] * cos[v][y]) * alpha
        s = np.zeros(src.shape[:2], f32)
        for y in range(8):
            s = s + src[:, :, y] * cos[v, y]
        work[:, :, v] = s * alpha[int(v != 0)]
    dst = np.zeros_like(src)
    for u in range(8):                      # vertical: dst[u][v] = (sum over x of work[x][v] * cos[u][x]) * alpha
        s = np.zeros(src.shape[:2], f32)
        for x in range(8):
            s = s + work[:, x, :] * cos[u, x]
        dst[:, u, :] = s * alpha[int(u != 0)]
    return dst.reshape(-1, 64)


def np_variance(values):
    """vari_ddof1_times_n along axis 1 of (N, n)"""
    n = values.shape[1]
    mean = np.zeros(values.shape[0], f32)
    for i in range(n):
        mean = mean + values[:, i]
    mean = mean / f32(n)
    sum_sq = np.zeros(values.shape[0], f32)
    for i in range(n):
        d = values[:, i] - mean
        sum_sq = sum_sq + d * d
    return sum_sq * (f32(n) / f32(n - 1))


def np_mask_strength(block, dct):
    g_mask = tables()["HVS_MASK"]
    mask = np.zeros(block.shape[0], f32)
    for i in range(1, 64):
        mask = mask + (dct[:, i] * dct[:, i]) * g_mask[i]
    pop = np_variance(block)
    grid = block.reshape(-1, 8, 8)
    quads = [np_variance(grid[:, y0:y0 + 4, x0:x0 + 4].reshape(-1, 16)) for x0, y0 in ((0, 0), (4, 0), (0, 4), (4, 4))]
    qsum = quads[0] + quads[1] + quads[2] + quads[3]
    with np.errstate(divide="ignore", invalid="ignore"):
        pop = np.where(pop != f32(0.0), qsum / pop, pop).astype(f32)
    return np.sqrt(mask * pop / f32(16.0) / f32(64.0))


def np_terms(mode, pa, pb):
    """(N, 64, 4) u8 blocks of both images -> the float terms (hvs (N, 64) f32, hvsm (N, 64) f32)"""
    t = tables()
    csf, g_mask = t["HVS_CSF"], t["HVS_MASK"]
    a_block, b_block = np_samples(mode, pa), np_samples(mode, pb)
    a_dct, b_dct = np_dct(a_block), np_dct(b_block)
    mask = np.maximum(np_mask_strength(a_block, a_dct), np_mask_strength(b_block, b_dct))
    u = np.abs(a_dct - b_dct)
    w = u * csf[None, :]
    hvs = w * w
    threshold = mask[:, None] / g_mask[None, :]
    um = np.where(u < threshold, f32(0.0), u - threshold).astype(f32)
    um[:, 0] = u[:, 0]
    wm = um * csf[None, :]
    assert hvs.dtype == f32 and wm.dtype == f32 and a_dct.dtype == f32 and mask.dtype == f32
    return hvs, wm * wm


def np_block_sums(terms):
    """(N, 64) f32 -> (N,) f64: the terms of a block added in index order"""
    s = np.zeros(terms.shape[0], np.float64)
    for i in range(64):
        s = s + terms[:, i].astype(np.float64)
    return s


def np_blocks(a, b, mode):
    """-> (per-block doubles (blocks, 2), running sums (2,): every term of every block added to one double in raster order, as the reference does)"""
    h, w = min(a.shape[0], b.shape[0]), min(a.shape[1], b.shape[1])
    hvs, hvsm = np_terms(mode, extract_blocks(a, w, h), extract_blocks(b, w, h))
    running = []
    for t in (hvs, hvsm):
        s = 0.0
        for v in t.astype(np.float64).reshape(-1).tolist():
            s += v
        running.append(s)
    return np.stack([np_block_sums(hvs), np_block_sums(hvsm)], 1), np.array(running, np.float64)


def np_psnr(mseh):
    return 100000.0 if mseh <= 0.0 else 10.0 * math.log10(1.0 / mseh)


def np_reduce(sum_hvs, sum_hvsm, blocks):
    """psnr_hvs_compute_chan's tail and psnr_hvs_compute_metrics' averages in Python doubles -> {entry: {figure: float}}"""
    out, samples = {}, float(blocks * 64)
    for k, name in enumerate(MODES):
        mh, mm = float(sum_hvs[k]) / samples, float(sum_hvsm[k]) / samples
        out[name] = {"mseh_hvs": mh, "mseh_hvsm": mm, "psnr_hvs": np_psnr(mh), "psnr_hvsm": np_psnr(mm)}
    for name, chans in (("rgb", "rgb"), ("rgba", "rgba")):
        mh = mm = 0.0
        for c in chans:
            mh += out[c]["mseh_hvs"]
            mm += out[c]["mseh_hvsm"]
        mh, mm = mh / float(len(chans)), mm / float(len(chans))
        out[name] = {"mseh_hvs": mh, "mseh_hvsm": mm, "psnr_hvs": np_psnr(mh), "psnr_hvsm": np_psnr(mm)}
    return out


def raster_sum(values):
    """doubles added one after the other"""
    s = 0.0
    for v in np.asarray(values, np.float64).tolist():
        s += v
    return s


@functools.lru_cache(maxsize=None)
def _np_all_modes_cached(key):
    a, b = _PAIRS[key]
    return tuple(np_blocks(a, b, m) for m in range(6))


_PAIRS = {}


def np_all_modes(a, b, key=None):
    """np_blocks for the six modes; with a key, computed once per process and shared (nobody writes into the result)"""
    if key is None:
        return tuple(np_blocks(a, b, m) for m in range(6))
    _PAIRS.setdefault(key, (a, b))
    return _np_all_modes_cached(key)


def printed_from_running(per_mode):
    """per_mode: six (blocks (n, 2), running (2,)) -> {entry: figures} from the reference-order running sums"""
    blocks = per_mode[0][0].shape[0]
    return np_reduce([m[1][0] for m in per_mode], [m[1][1] for m in per_mode], blocks)


def assert_close_to_printed(got, printed, what):
    """got: {entry: {"psnr_hvs", "psnr_hvsm"}}; printed: (8, 2) of the tool's numbers in ENTRIES order. Every figure within PRINT_TOLERANCE."""
    for ei, entry in enumerate(ENTRIES):
        for fi, fig in enumerate(("psnr_hvs", "psnr_hvsm")):
            assert abs(got[entry][fig] - printed[ei][fi]) <= PRINT_TOLERANCE, (what, entry, fig, got[entry][fig], float(printed[ei][fi]))


def random_blocks(n, seed):
    """an (8, 8 n, 4) pair = n blocks of mixed kinds: near-noise, unrelated, flat against noise, flat against flat, smooth ramps, single-channel differences"""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 256, (8, 8 * n, 4), dtype=np.uint8)
    b = rng.integers(0, 256, (8, 8 * n, 4), dtype=np.uint8)
    kind = np.repeat(rng.integers(0, 6, n), 8)
    near = np.clip(a.astype(np.int64) + rng.integers(-6, 7, a.shape), 0, 255).astype(np.uint8)
    flat_a = np.repeat(rng.integers(0, 256, (1, n, 4), dtype=np.uint8), 8, axis=1).repeat(8, axis=0)
    flat_b = np.repeat(rng.integers(0, 256, (1, n, 4), dtype=np.uint8), 8, axis=1).repeat(8, axis=0)
    yy, xx = np.mgrid[0:8, 0:8 * n]
    ramp = np.clip(xx[..., None] * rng.integers(1, 5, 4)[None, None] + yy[..., None] * 3, 0, 255).astype(np.uint8)
    b[:, kind == 0] = near[:, kind == 0]
    a[:, kind == 2] = flat_a[:, kind == 2]
    a[:, kind == 3] = flat_a[:, kind == 3]
    b[:, kind == 3] = flat_b[:, kind == 3]
    a[:, kind == 4] = ramp[:, kind == 4]
    b[:, kind == 4] = np.clip(ramp.astype(np.int64) + rng.integers(-2, 3, ramp.shape), 0, 255).astype(np.uint8)[:, kind == 4]
    one = near.copy()
    one[..., 1:] = a[..., 1:]
    b[:, kind == 5] = one[:, kind == 5]
    return a, b
