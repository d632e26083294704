#!/usr/bin/env python3
"""Reading one ETC1S file back, timed: the 4096x4096 synthetic image compressed at quality 128 (compress(), .basis), then
  host   decode_etc1s_file: containers, tables, palettes and the slice walk (wall time, best of 3), and
  device the transcode kernel per target: palettes and indices resident in HBM, 5 warm-up + 50 timed launches, measured with the library's HIP events around the launch
         (bu_hip_profile_*), with the algorithmic bytes (4 B of indices in + the target's bytes out per block) over time as a fraction of the 8 TB/s HBM figure,
         and the whole call (launch, stream wait, read-back of the counter) on the host's clock, median of the timed calls. ETC2 RGBA and BC7 go through
         bu_hip_k_transcode_etc1s_image_counted; BC7 is timed with and without the chroma filter. ASTC 4x4, EAC R11 and EAC RG11 go through
         bu_hip_k_transcode_etc1s_block_format_counted (the image has no alpha slice: ASTC takes its opaque routes, RG11 writes the opaque second half). ATC RGB,
         FXT1 (16 bytes per two source blocks, counted as 8 per source block) and PVRTC2 RGB / RGBA go through bu_hip_k_transcode_etc1s_vendor_format_counted. PVRTC2 RGBA
         gets an alpha slice: the image's own indices again, so that alpha is the green channel -- every block is translucent and is re-encoded per pixel.
Also prints the RGB PSNR of the file read back (RGBA32) against the source: the figure README quotes for "the file after the backend's RDO".
Prints one line per figure and one JSON line.   tools/etc1s_transcode_bench.py [steps] [warmup] [size]"""
import ctypes as C
import json
import pathlib
import sys
import time

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
import helpers  # noqa: E402
from basis_universal_amd import capi, transcode  # noqa: E402
from basis_universal_amd.compress import compress  # noqa: E402

HBM_BYTES_PER_S = 8e12
TARGETS = [("rgba32", transcode.RGBA32, 64), ("etc1", transcode.ETC1_RGB, 8), ("bc1", transcode.BC1_RGB, 8), ("rgb565", transcode.RGB565, 32), ("bgr565", transcode.BGR565, 32),
           ("rgba4444", transcode.RGBA4444, 32)]
TEXTURE_TARGETS = [("etc2_rgba", transcode.ETC2_RGBA, 16, 0), ("bc7_filtered", transcode.BC7_RGBA, 16, 0), ("bc7_unfiltered", transcode.BC7_RGBA, 16, transcode.DECODE_FLAGS_NO_ETC1S_CHROMA_FILTERING)]
VENDOR_FORMAT_TARGETS = [("atc_rgb", transcode.ATC_RGB, 8, 0), ("fxt1", transcode.FXT1_RGB, 8, 0), ("pvrtc2_rgb", transcode.PVRTC2_4_RGB, 8, 0),
                         ("pvrtc2_rgba", transcode.PVRTC2_4_RGBA, 8, 0)]   # FXT1: 16 bytes per two source blocks = 8 per source block; PVRTC2 RGBA reads an alpha slice as well
BLOCK_FORMAT_TARGETS = [("astc_4x4", transcode.ASTC_4x4_RGBA, 16, 0), ("eac_r11", transcode.ETC2_EAC_R11, 8, 0), ("eac_rg11", transcode.ETC2_EAC_RG11, 16, 0)]


def main():
    steps = int(sys.argv[1]) if len(sys.argv) > 1 else 50
    warmup = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    size = int(sys.argv[3]) if len(sys.argv) > 3 else 4096
    ctx = capi.Context(0)
    t0 = time.perf_counter()
    source = helpers.synth(size, size, 1234)
    data = compress(ctx, source, uastc=False, quality=128)
    compress_s = time.perf_counter() - t0
    raw = bytes(data)
    host_ms = []
    for _ in range(3):
        t0 = time.perf_counter()
        decoded = transcode.decode_etc1s_file(raw)
        host_ms.append((time.perf_counter() - t0) * 1e3)
    im = decoded["images"][0]
    nbx, nby = im["num_blocks_x"], im["num_blocks_y"]
    n = nbx * nby
    print(f"file {len(raw)} bytes ({compress_s:.1f} s to compress), {decoded['num_endpoints']} endpoints, {decoded['num_selectors']} selectors, {n} blocks", flush=True)
    print(f"host decode {min(host_ms):8.2f} ms (best of 3: {', '.join(f'{v:.2f}' for v in host_ms)})", flush=True)
    back = transcode.transcode_etc1s_image(ctx, decoded, im, transcode.RGBA32)
    psnr = 10 * np.log10(255.0 ** 2 / ((back[..., :3].astype(np.float64) - source[..., :3]) ** 2).mean())
    print(f"RGB PSNR of the file read back against the source {psnr:.2f} dB", flush=True)
    ep, sel = np.ascontiguousarray(decoded["endpoint_palette"]), np.ascontiguousarray(decoded["selector_palette"])
    d = [ctx.upload(ep), ctx.upload(sel), ctx.upload(im["endpoint_indices"]), ctx.upload(im["selector_indices"])]
    d_out = ctx.alloc(n * 64)
    rows = {}
    for name, target, out_bytes, flags, block_format in [t + (None, False) for t in TARGETS] + [t + (False,) for t in TEXTURE_TARGETS] + [t + (True,) for t in BLOCK_FORMAT_TARGETS] + [t + ("vendor",) for t in VENDOR_FORMAT_TARGETS]:
        def launch():
            invalid = C.c_uint32(0)
            alpha = (C.c_void_p(d[2]), C.c_void_p(d[3])) if target == transcode.PVRTC2_4_RGBA else (None, None)
            head = (ctx.h, C.c_void_p(d[0]), ep.shape[0], C.c_void_p(d[1]), sel.size, C.c_void_p(d[2]), C.c_void_p(d[3]), *alpha, nbx, nby, size, size, target, C.c_void_p(d_out), 0, 0)
            if block_format == "vendor":
                ctx.check(ctx.lib.k_transcode_etc1s_vendor_format_counted(*head, flags, C.byref(invalid)), "transcode_etc1s_vendor_format")
            elif block_format:
                ctx.check(ctx.lib.k_transcode_etc1s_block_format_counted(*head, flags, C.byref(invalid)), "transcode_etc1s_block_format")
            elif flags is None:
                ctx.check(ctx.lib.k_transcode_etc1s_counted(*head, C.byref(invalid)), "transcode_etc1s")
            else:
                ctx.check(ctx.lib.k_transcode_etc1s_image_counted(*head, flags, C.byref(invalid)), "transcode_etc1s_image")
            assert invalid.value == 0
        for _ in range(warmup):
            launch()
        ctx.profile_enable(True)
        calls = []
        for _ in range(steps):
            t0 = time.perf_counter()
            launch()
            calls.append((time.perf_counter() - t0) * 1e3)
        ms, launches = ctx.profile_read()["etc1s_transcode"]
        ctx.profile_enable(False)
        assert launches == steps
        ms /= steps
        traffic = n * ((8 if target == transcode.PVRTC2_4_RGBA else 4) + out_bytes)
        rows[name] = {"ms": round(ms, 4), "call_ms": round(float(np.median(calls)), 4), "gblocks_per_s": round(n / ms / 1e6, 2), "algorithmic_mb": round(traffic / 1e6, 1), "fraction_of_8tbps": round(traffic / (ms * 1e-3) / HBM_BYTES_PER_S, 4)}
        print(f"{name:14s} {ms:8.4f} ms  call {np.median(calls):8.4f} ms  {n / ms / 1e6:7.2f} Gblocks/s  {traffic / 1e6:6.1f} MB  {100 * traffic / (ms * 1e-3) / HBM_BYTES_PER_S:6.2f} % of 8 TB/s", flush=True)
    for p in d + [d_out]:
        ctx.free(p)
    ctx.close()
    print(json.dumps({"image": f"synth{size} seed 1234, ETC1S q128 .basis", "file_bytes": len(raw), "steps": steps, "warmup": warmup, "host_decode_ms": round(min(host_ms), 2), "rgb_psnr_db": round(float(psnr), 2), "targets": rows}))


if __name__ == "__main__":
    main()
