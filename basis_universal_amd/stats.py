"""How good is the file: the last stage of basis_compressor::process (m_compute_stats, comp.cpp:4195-4253), the per-slice image_stats `basisu -stats` prints --
RGB / RGBA / R / G / B / A / 709-luma / 601-luma Max, Mean, RMS and PSNR of what the file decodes to against the source.

image_metrics::calc (encoder/basisu_enc.cpp:2155-2226) is a 256-bin histogram of absolute differences under a thin layer of doubles. The histograms (and the channel
sums) of all eight lines are counted on the GPU in one pass over two resident RGBA8 rasters (csrc/image_metrics_kernels.hip, bu_hip_k_image_metrics): integer counts,
hence exactly the reference's, whatever the order of accumulation. The doubles are host code in the reference's own expression order (csrc/image_metrics.h,
bu_image_metrics_reduce in libbasisu_frontend.so). The decode that is compared is the device transcoders' RGBA32 (transcode.py), resident, never downloaded.
There is no CPU implementation of the counting: without the HIP library and a GPU `image_metrics` raises. This overload of calc never sets m_ssim; SSIM is `ssim` below.

With hvs=True (file_stats) / stats_hvs=True (compress) every slice also carries what the tool prints under "PSNR-HVS and PSNR-HVS-M metrics:" (m_psnr_hvs_m_stats,
comp.cpp:4265-4276; psnr_hvs_compute_metrics, enc.cpp:2256-2519; `basisu -compare_hvs` for any two images = psnr_hvs below). Per 8x8 block and mode (BT.601 Y rounded
to 8 bits, BT.601 Y in float, R, G, B, A) two float DCTs, two masking strengths and 128 weighted differences, binary32 in the reference's operation order
(csrc/psnr_hvs.h), one wave per block and mode (csrc/psnr_hvs_kernels.hip, bu_hip_k_psnr_hvs); the per-block doubles are the reference's bit for bit, their sum over
the image is added in a fixed order of the kernel's own (deterministic; within 2 (blocks - 1) 2^-53 relative of raster order). mseh and dB are host code
(bu_psnr_hvs_reduce).

With bc7=True (file_stats) / stats_bc7=True (compress) every slice of a UASTC file also carries, under "bc7", the tool's second block, "Quality stats vs. transcoded BC7
texture:" (comp.cpp:3818-3842, 3875-3883, 4278-4337): the same eight lines -- and with hvs its own "hvs", "PSNR-HVS and PSNR-HVS-M metrics (BC7):" -- of the same source
against what the slice's BC7 transcode samples as: the resident blocks through the device's UASTC -> BC7 transcoder and then through the block unpacker
(transcode.unpack_blocks, csrc/block_unpack_kernels.hip), never downloaded. UASTC files only: the ETC1S transcoder here has no BC7 target, and the flag raises for an
ETC1S file.

With ssim=True (file_stats) / stats_ssim=True (compress) every slice dict -- and with bc7 the "bc7" dict too -- also carries "ssim": the seven figures `basisu -compare
-compare_ssim` prints for two images (compute_ssim, encoder/basisu_ssim.cpp = ssim below; the reference's -stats stage does not print them, its compare mode does).
Per pixel and channel five 11x11 Gaussian filterings of float images and the smap formula, binary32 in the reference's operation order (csrc/ssim.h), one lane per
pixel (csrc/ssim_kernels.hip, bu_hip_k_ssim); then the mean as the reference's one running float sum in raster order, evaluated in chunks with csrc/fsum_scan.h
(csrc/ssim_reduce.h): the figures are the reference's bit for bit, and print as the tool prints them. Not here: the best-ETC1S stats."""
import contextlib
import ctypes as C

import numpy as np

from . import transcode
from .etc1s import load_frontend_library

# name -> (first_chan, total_chans, use_601), in the order the reference prints them (comp.cpp:4213-4252)
LINES = {"rgb": (0, 3, 0), "rgba": (0, 4, 0), "r": (0, 1, 0), "g": (1, 1, 0), "b": (2, 1, 0), "a": (3, 1, 0), "luma_709": (0, 0, 0), "luma_601": (0, 0, 1)}


class Counts(C.Structure):      # = bu_image_metrics_counts, include/basisu_hip.h
    _fields_ = [("struct_bytes", C.c_uint32), ("width", C.c_uint32), ("height", C.c_uint32), ("reserved", C.c_uint32), ("hist", C.c_uint32 * 256 * 6),
                ("sum_a", C.c_uint64 * 4), ("sum_b", C.c_uint64 * 4)]


class _Metrics(C.Structure):    # = bu_image_metrics, include/basisu_hip_image_metrics.h
    _fields_ = [("max", C.c_double), ("mean", C.c_float), ("mean_squared", C.c_float), ("rms", C.c_float), ("psnr", C.c_float)]


class HvsSums(C.Structure):     # = bu_psnr_hvs_sums, include/basisu_hip.h
    _fields_ = [("struct_bytes", C.c_uint32), ("width", C.c_uint32), ("height", C.c_uint32), ("blocks", C.c_uint32), ("sum_hvs", C.c_double * 6), ("sum_hvsm", C.c_double * 6)]


class _HvsChan(C.Structure):    # = bu_psnr_hvs_chan, include/basisu_hip_image_metrics.h
    _fields_ = [("mseh_hvs", C.c_double), ("mseh_hvsm", C.c_double), ("psnr_hvs", C.c_double), ("psnr_hvsm", C.c_double)]


class _HvsMetrics(C.Structure):  # = bu_psnr_hvs_metrics
    _fields_ = [("y_601_8bit", _HvsChan), ("y_601_float", _HvsChan), ("chan", _HvsChan * 4), ("rgb", _HvsChan), ("rgba", _HvsChan)]


class SsimResult(C.Structure):  # = bu_ssim_result, include/basisu_hip.h
    _fields_ = [("struct_bytes", C.c_uint32), ("width", C.c_uint32), ("height", C.c_uint32), ("chunks_walked", C.c_uint32), ("r", C.c_float), ("g", C.c_float),
                ("b", C.c_float), ("rgb", C.c_float), ("a", C.c_float), ("luma_709", C.c_float), ("luma_601", C.c_float), ("chunks", C.c_uint32)]


SSIM_FIGURES = ("r", "g", "b", "rgb", "a", "luma_709", "luma_601")   # in the order the reference prints them (basisu_tool.cpp, -compare_ssim)
SSIM_MODES = ("rgba", "luma_709", "luma_601")                        # the mode of bu_hip_k_ssim_map
HVS_MODES = ("y_601_8bit", "y_601_float", "r", "g", "b", "a")   # the index of bu_psnr_hvs_sums::sum_hvs / sum_hvsm
HVS_ENTRIES = ("y_601_float", "y_601_8bit", "rgb", "rgba", "r", "g", "b", "a")   # in the order the reference prints them (psnr_hvs_print_metrics)

_reduce_lib = load_frontend_library   # bu_image_metrics_reduce lives in libbasisu_frontend.so


def reduce_counts(hist, width, height):
    """hist (6, 256) u32 as bu_hip_k_image_metrics counts it -> {line: {"max", "mean", "rms", "psnr"}} for the eight lines of LINES. Host only."""
    hist = np.ascontiguousarray(hist, np.uint32)
    if hist.shape != (6, 256):
        raise ValueError("hist must be (6, 256)")
    L, out = _reduce_lib(), {}
    for name, (first, total, use_601) in LINES.items():
        m = _Metrics()
        if not L.bu_image_metrics_reduce(hist.ctypes.data_as(C.c_void_p), total, first, int(width), int(height), use_601, C.byref(m)):
            raise ValueError(f"bu_image_metrics_reduce refused {name}")
        out[name] = {"max": float(m.max), "mean": float(m.mean), "rms": float(m.rms), "psnr": float(m.psnr)}
    return out


@contextlib.contextmanager
def _resident_pair(ctx, a, b):
    """a, b: a numpy (h, w, 4) u8 image (uploaded, and freed on the way out) or a (device pointer, w, h, pitch in pixels) tuple each -> the two
    (pointer, w, h, pitch) tuples as the kernels' entry points take them"""
    owned, out = [], []
    try:
        for raster in (a, b):
            if isinstance(raster, np.ndarray):
                img = np.ascontiguousarray(raster, np.uint8)
                if img.ndim != 3 or img.shape[2] != 4:
                    raise ValueError("an image must be (h, w, 4) uint8")
                owned.append(ctx.upload(img))
                raster = owned[-1], img.shape[1], img.shape[0], img.shape[1]
            d, w, h, pitch = raster
            out.append((C.c_void_p(int(d)), int(w), int(h), int(pitch)))
        yield out
    finally:
        for d in owned:
            ctx.free(d)


def image_counts(ctx, a, b):
    """bu_hip_k_image_metrics: a, b as for image_metrics -> (hist (6, 256) u32, sum_a (4,) u64, sum_b (4,) u64, width, height) of the region both cover."""
    with _resident_pair(ctx, a, b) as (ra, rb):
        c = Counts()
        c.struct_bytes = C.sizeof(Counts)
        ctx.check(ctx.lib.k_image_metrics(ctx.h, *ra, *rb, C.byref(c)), "image_metrics")
    return np.ctypeslib.as_array(c.hist).copy(), np.array(list(c.sum_a), np.uint64), np.array(list(c.sum_b), np.uint64), int(c.width), int(c.height)


def image_metrics(ctx, a, b):
    """image_metrics::calc of `a` against `b` for every line the reference prints. a, b: (h, w, 4) u8 arrays (uploaded) or (device pointer, width, height, row pitch
    in pixels, 0 = width) tuples of resident RGBA8 rasters; the region is min(widths) x min(heights), as calc crops.
    -> {"rgb", "rgba", "r", "g", "b", "a", "luma_709", "luma_601": {"max", "mean", "rms", "psnr"}, "sum_a", "sum_b": per-channel sums (4 ints each), "width", "height"}.
    avg_comp_error = true throughout, as basis_compressor calls it. An empty region has the reference's 0 / 0 (NaN) means."""
    hist, sum_a, sum_b, w, h = image_counts(ctx, a, b)
    out = reduce_counts(hist, w, h)
    out.update({"sum_a": [int(v) for v in sum_a], "sum_b": [int(v) for v in sum_b], "width": w, "height": h})
    return out


def psnr_hvs_sums(ctx, a, b):
    """bu_hip_k_psnr_hvs: a, b as for image_metrics -> the filled HvsSums (sum_hvs / sum_hvsm per mode of HVS_MODES, blocks, width, height)."""
    with _resident_pair(ctx, a, b) as (ra, rb):
        s = HvsSums()
        s.struct_bytes = C.sizeof(HvsSums)
        ctx.check(ctx.lib.k_psnr_hvs(ctx.h, *ra, *rb, C.byref(s)), "psnr_hvs")
    return s


def psnr_hvs_block_sums(ctx, a, b, mode):
    """bu_hip_k_psnr_hvs_blocks (the test hook): -> (blocks, 2) f64, the HVS and the HVS-M double of every 8x8 block of mode HVS_MODES[mode], raster order."""
    with _resident_pair(ctx, a, b) as (ra, rb):
        w, h = min(ra[1], rb[1]), min(ra[2], rb[2])
        cap = ((w + 7) // 8) * ((h + 7) // 8)
        out, n = np.zeros((max(cap, 1), 2), np.float64), C.c_uint32(0)
        ctx.check(ctx.lib.k_psnr_hvs_blocks(ctx.h, *ra, *rb, int(mode), out.ctypes.data_as(C.c_void_p), cap, C.byref(n)), "psnr_hvs_blocks")
    return out[:n.value]


def reduce_hvs_sums(sums):
    """bu_psnr_hvs_reduce: an HvsSums -> {entry of HVS_ENTRIES: {"mseh_hvs", "mseh_hvsm", "psnr_hvs", "psnr_hvsm"}}. Host only."""
    m = _HvsMetrics()
    if not _reduce_lib().bu_psnr_hvs_reduce(C.byref(sums), C.byref(m)):
        raise ValueError("bu_psnr_hvs_reduce refused the sums")
    chans = {"y_601_float": m.y_601_float, "y_601_8bit": m.y_601_8bit, "rgb": m.rgb, "rgba": m.rgba, "r": m.chan[0], "g": m.chan[1], "b": m.chan[2], "a": m.chan[3]}
    return {name: {f: float(getattr(chans[name], f)) for f, _ in _HvsChan._fields_} for name in HVS_ENTRIES}


def psnr_hvs(ctx, a, b):
    """psnr_hvs_compute_metrics of `a` against `b` (what `basisu -compare_hvs a b` prints after the image metrics). a, b: (h, w, 4) u8 arrays (uploaded) or (device
    pointer, width, height, row pitch in pixels, 0 = width) tuples of resident RGBA8 rasters; the region is min(widths) x min(heights) in 8x8 blocks whose pixel
    coordinates are clamped to each raster's own edge.
    -> {"y_601_float", "y_601_8bit", "rgb", "rgba", "r", "g", "b", "a": {"mseh_hvs", "mseh_hvsm", "psnr_hvs", "psnr_hvsm"}, "width", "height"}; a psnr of 100000.0
    means no difference (PSNR_HVS_LOSSLESS_DB). An empty region has the 0 / 0 (NaN) of the division; the reference refuses it."""
    sums = psnr_hvs_sums(ctx, a, b)
    out = reduce_hvs_sums(sums)
    out.update({"width": int(sums.width), "height": int(sums.height)})
    return out


def ssim_result(ctx, a, b):
    """bu_hip_k_ssim: a, b as for image_metrics -> the filled SsimResult (the seven floats, width, height, and the reduction's chunks / chunks_walked)."""
    with _resident_pair(ctx, a, b) as (ra, rb):
        s = SsimResult()
        s.struct_bytes = C.sizeof(SsimResult)
        ctx.check(ctx.lib.k_ssim(ctx.h, *ra, *rb, C.byref(s)), "ssim")
    return s


def ssim_map(ctx, a, b, mode):
    """bu_hip_k_ssim_map (the test hook): the smap values of one call of compute_ssim in raster order -> (h, w, 4) f32 for mode 0 (the RGBA call), (h, w) f32 for
    mode 1 / 2 (channel 0 of the 709 / 601 luma call)."""
    with _resident_pair(ctx, a, b) as (ra, rb):
        w, h = min(ra[1], rb[1]), min(ra[2], rb[2])
        out, n = np.zeros((h, w, 4) if int(mode) == 0 else (h, w), np.float32), C.c_uint32(0)
        ctx.check(ctx.lib.k_ssim_map(ctx.h, *ra, *rb, int(mode), out.ctypes.data_as(C.c_void_p), out.size, C.byref(n)), "ssim_map")
    if n.value != w * h:
        raise RuntimeError(f"ssim_map: {n.value} pixels for a region of {w} x {h}")
    return out


def ssim(ctx, a, b):
    """compute_ssim of `a` against `b`: the seven figures `basisu -compare -compare_ssim a b` prints. a, b: (h, w, 4) u8 arrays (uploaded) or (device pointer, width,
    height, row pitch in pixels, 0 = width) tuples of resident RGBA8 rasters; the region is min(widths) x min(heights), and the filter's coordinates are clamped to it.
    -> {"r", "g", "b", "rgb", "a", "luma_709", "luma_601": Python floats of the binary32 results ("%f" % value is the tool's text), "width", "height"}.
    An empty region raises (the reference asserts), as does one beyond 2^25 pixels. From 2^24 pixels on the reference's running float sum stops growing for addends
    near 1 (an identical pair then gives less than 1.0); that is reproduced, not repaired."""
    s = ssim_result(ctx, a, b)
    out = {name: float(getattr(s, name)) for name in SSIM_FIGURES}
    out.update({"width": int(s.width), "height": int(s.height)})
    return out


def _slice_stats(ctx, src, decoded, hvs, with_ssim=False):
    """the dict of one slice: image_metrics, and under "hvs" / "ssim" psnr_hvs / ssim of the same two resident rasters when asked for"""
    out = image_metrics(ctx, src, decoded)
    if hvs:
        out["hvs"] = psnr_hvs(ctx, src, decoded)
    if with_ssim:
        out["ssim"] = ssim(ctx, src, decoded)
    return out


def _is_etc1s(raw):
    if len(raw) >= 48 and raw[:12] == transcode._KTX2_MAGIC:
        return int.from_bytes(raw[44:48], "little") == 1     # supercompressionScheme: 1 = BasisLZ (ETC1S), 0 = none (UASTC)
    if len(raw) >= 21 and raw[:2] == b"sB":
        return raw[20] == 0                                   # basis_file_header::m_tex_format: 0 = ETC1S, 1 = UASTC 4x4
    raise ValueError("neither a .basis nor a .ktx2 file")


def split_planes(image):
    """The two source images of an ETC1S image with alpha (comp.cpp:2880-2910): (r, g, b, 255) and (a, a, a, 255)."""
    img = np.ascontiguousarray(image, np.uint8)
    colour = img.copy()
    colour[..., 3] = 255
    alpha = np.repeat(img[..., 3:4], 4, axis=2)
    alpha[..., 3] = 255
    return colour, alpha


def _slice_order(images):
    """the compressor's slice order: source image (layer, face) outermost, then its levels"""
    return sorted(range(len(images)), key=lambda k: (images[k]["layer"], images[k]["face"], images[k]["level"]))


BC7_REFUSAL = "BC7 stats are for UASTC files only: the ETC1S transcoder here has no BC7 target"


def _stats_from_slices(ctx, raw, slice_sources, hvs=False, bc7=False, ssim=False):
    """slice_sources(level, layer, face, n_slices) -> one source raster per slice of that image (array or resident tuple). -> the per-slice dicts, slice order."""
    out = []
    if _is_etc1s(raw):
        if bc7:
            raise ValueError(BC7_REFUSAL)
        # every slice of the file decoded by ONE whole-file call into one allocation. The alpha slice is decoded as a colour image from the alpha indices, as the
        # reference unpacks every slice on its own: a record of its own whose first_block is the alpha range, without an alpha slice
        decoded = transcode._decode_etc1s(raw, False, whole=True)
        order = _slice_order(decoded["images"])
        slices = [(decoded["images"][k], first) for k in order for first in (["_first", "_alpha_first"] if decoded["images"][k]["has_alpha"] else ["_first"])]
        layout, total = transcode.image_layout([im for im, _ in slices], transcode.RGBA32, etc1s=True)
        d_out = ctx.alloc(max(total, 1))
        try:
            transcode._transcode_etc1s_slices(ctx, decoded, [im for im, _ in slices], [im[first] for im, first in slices], None, transcode.RGBA32, d_out)
            at = iter(layout)
            for k in order:
                im = decoded["images"][k]
                for src in slice_sources(im["level"], im["layer"], im["face"], 2 if im["has_alpha"] else 1):
                    out.append(_slice_stats(ctx, src, (d_out + next(at)["offset"], im["width"], im["height"], im["width"]), hvs, ssim))
        finally:
            ctx.free(d_out)
        return out
    info = transcode.read_uastc_file(raw)
    if not bc7:   # the same for UASTC; the bc7 path below stays slice by slice (unpack_blocks has no table form)
        layout, total = transcode.image_layout(info["images"], transcode.RGBA32, etc1s=False)
        d_out = ctx.alloc(max(total, 1))
        try:
            transcode.transcode_file_images(ctx, raw, transcode.RGBA32, out_device=d_out)
            for k in _slice_order(info["images"]):
                im = info["images"][k]
                (src,) = slice_sources(im["level"], im["layer"], im["face"], 1)
                out.append(_slice_stats(ctx, src, (d_out + layout[k]["offset"], im["width"], im["height"], im["width"]), hvs, ssim))
        finally:
            ctx.free(d_out)
        return out
    for k in _slice_order(info["images"]):
        im = info["images"][k]
        w, h = im["width"], im["height"]
        blocks = np.frombuffer(raw, np.uint8, im["length"], im["offset"]).reshape(-1, 16)
        (src,) = slice_sources(im["level"], im["layer"], im["face"], 1)
        d_out = ctx.alloc(w * h * 4)
        try:
            # the blocks go up once; the BC7 texture and both rasters stay on the device
            d_blocks, d_bc7 = ctx.upload(blocks), ctx.alloc(blocks.shape[0] * 16)
            try:
                transcode.transcode_uastc_blocks(ctx, d_blocks, im["num_blocks_x"], im["num_blocks_y"], transcode.RGBA32, width=w, height=h, out_device=d_out)
                one = _slice_stats(ctx, src, (d_out, w, h, w), hvs, ssim)
                transcode.transcode_uastc_blocks(ctx, d_blocks, im["num_blocks_x"], im["num_blocks_y"], transcode.BC7_RGBA, out_device=d_bc7)
                transcode.unpack_blocks(ctx, d_bc7, im["num_blocks_x"], im["num_blocks_y"], transcode.BC7_RGBA, width=w, height=h, out_device=d_out)
                one["bc7"] = _slice_stats(ctx, src, (d_out, w, h, w), hvs, ssim)
                out.append(one)
            finally:
                ctx.free(d_blocks)
                ctx.free(d_bc7)
        finally:
            ctx.free(d_out)
    return out


def file_stats(ctx, data, images, hvs=False, bc7=False, ssim=False):
    """The reference's m_stats for a .basis / .ktx2 file of this package (UASTC LDR 4x4 or ETC1S): one image_metrics dict per slice, in the compressor's slice order
    (source image outermost, then its levels; an ETC1S image with alpha has a colour slice and then an alpha slice, each with its own stats).
    images: the source of every image the file holds -- {(level, layer, face): image} or, for a file of one layer and face, a list by level; an image is an
    (h, w, 4) u8 array or a resident (device pointer, width, height, pitch) tuple. The file is decoded on the device to RGBA32 -- every slice by one whole-file
    transcode call into one allocation (transcode_file_images / the ETC1S slice table; with bc7 slice by slice) --, cropped to each slice's original size, and compared there. A colour slice of an ETC1S file with alpha is compared
    against (r, g, b, 255), its alpha slice -- decoded as a colour image -- against (a, a, a, 255).
    hvs: every slice dict gains "hvs", psnr_hvs of the same source against the same resident decode (m_psnr_hvs_m_stats, which the tool sets with -stats). A source
    that is padded beyond the slice's size (the compressor's level rasters) must be padded with duplicated borders, as the compressor's are: a block's coordinates
    are clamped to each raster's own edge.
    bc7: every slice dict of a UASTC file gains "bc7": the same dict (the eight lines, sums and size, and "hvs" when hvs is set) of the same source against the slice's
    BC7 transcode, unpacked on the device. An ETC1S file raises ValueError before any work.
    ssim: every slice dict (and with bc7 the "bc7" dict) gains "ssim", ssim() of the same source against the same resident decode. The filter is clamped to the
    slice's own size, whatever padding the source raster has beyond it."""
    raw = data.tobytes() if isinstance(data, np.ndarray) else bytes(data)
    if bc7 and _is_etc1s(raw):
        raise ValueError(BC7_REFUSAL)
    by_key = images if isinstance(images, dict) else {(level, 0, 0): im for level, im in enumerate(images)}

    def slice_sources(level, layer, face, n_slices):
        if (level, layer, face) not in by_key:
            raise ValueError(f"no source image for level {level}, layer {layer}, face {face}")
        src = by_key[(level, layer, face)]
        if n_slices == 1:
            return [src]
        if not isinstance(src, np.ndarray):
            d, w, h, pitch = (int(v) for v in src)
            pitch = pitch or w
            rows = np.zeros((h, pitch, 4), np.uint8)      # a raster ends with its last pixel, not with its last row's padding
            if w and h:
                rows.reshape(-1, 4)[:(h - 1) * pitch + w] = ctx.download(d, ((h - 1) * pitch + w, 4), np.uint8)
            src = rows[:, :w]
        return list(split_planes(src))
    return _stats_from_slices(ctx, raw, slice_sources, hvs, bc7, ssim)
