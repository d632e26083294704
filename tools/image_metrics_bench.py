#!/usr/bin/env python3
"""The image-metrics kernel (csrc/image_metrics_kernels.hip), timed at 4096x4096 on its two extreme inputs:
  encode   the synthetic image compressed at ETC1S quality 128 (compress(), .basis), read back on the device to RGBA32, against its source: the differences of a
           real encode, piled into the low bins of the six histograms;
  one_bin  the source against itself: every one of the 16.8 M pixels lands in bin 0 of every histogram, the most same-address contention there is.
Both rasters resident in HBM, 5 warm-up + 50 timed calls, measured with the library's HIP events around the launch (bu_hip_profile_*: the clearing of the counts
and the kernel, not the copy of the counts to the host). Beside each time: the floor for reading the two rasters (2 x 64 MiB at the 8 TB/s HBM figure) and the
RGBA32 transcode launch that produced the decode (etc1s_transcode, same events). Prints one line per figure and one JSON line.
tools/image_metrics_bench.py [steps] [warmup] [size]"""
import ctypes as C
import json
import pathlib
import sys

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
import helpers  # noqa: E402
from basis_universal_amd import capi, stats, transcode  # noqa: E402
from basis_universal_amd.compress import compress  # noqa: E402

HBM_BYTES_PER_S = 8e12


def timed(ctx, name, call, steps, warmup):
    for _ in range(warmup):
        call()
    ctx.profile_enable(True)
    for _ in range(steps):
        call()
    ms, launches = ctx.profile_read()[name]
    ctx.profile_enable(False)
    assert launches == steps
    return ms / steps


def main():
    steps = int(sys.argv[1]) if len(sys.argv) > 1 else 50
    warmup = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    size = int(sys.argv[3]) if len(sys.argv) > 3 else 4096
    ctx = capi.Context(0)
    source = helpers.synth(size, size, 1234)
    decoded = transcode.decode_etc1s_file(bytes(compress(ctx, source, uastc=False, quality=128)))
    im = decoded["images"][0]
    d_src, d_dec = ctx.upload(source), ctx.alloc(size * size * 4)
    transcode_ms = timed(ctx, "etc1s_transcode", lambda: transcode.transcode_etc1s_image(ctx, decoded, im, transcode.RGBA32, out_device=d_dec), min(steps, 10), 2)
    counts = stats.Counts()
    counts.struct_bytes = C.sizeof(counts)

    def launch(d_a, d_b):
        ctx.check(ctx.lib.k_image_metrics(ctx.h, C.c_void_p(d_a), size, size, 0, C.c_void_p(d_b), size, size, 0, C.byref(counts)), "image_metrics")
    floor_ms = 2 * size * size * 4 / HBM_BYTES_PER_S * 1e3
    rows = {}
    for name, d_b in (("encode", d_dec), ("one_bin", d_src)):
        ms = timed(ctx, "image_metrics", lambda: launch(d_src, d_b), steps, warmup)
        hist = np.ctypeslib.as_array(counts.hist)
        assert (hist.sum(1) == size * size).all()
        psnr = stats.reduce_counts(hist, size, size)["rgb"]["psnr"]
        rows[name] = {"ms": round(ms, 4), "x_read_floor": round(ms / floor_ms, 2), "x_rgba32_transcode": round(ms / transcode_ms, 2), "bins_used_r": int((hist[0] != 0).sum()),
                      "rgb_psnr_db": round(psnr, 3)}
        print(f"{name:8s} {ms:8.4f} ms  {ms / floor_ms:6.2f} x the {floor_ms:.4f} ms read floor  {ms / transcode_ms:6.2f} x the RGBA32 transcode ({transcode_ms:.4f} ms)  "
              f"{rows[name]['bins_used_r']} R bins used, RGB PSNR {psnr:.3f} dB", flush=True)
    ctx.free(d_src); ctx.free(d_dec)
    ctx.close()
    print(json.dumps({"image": f"synth{size} seed 1234, ETC1S q128 .basis", "steps": steps, "warmup": warmup, "read_floor_ms": round(floor_ms, 4),
                      "rgba32_transcode_ms": round(transcode_ms, 4), "inputs": rows}))


if __name__ == "__main__":
    main()
