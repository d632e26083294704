#!/usr/bin/env python3
"""The PSNR-HVS kernel (csrc/psnr_hvs_kernels.hip), timed at 4096x4096 on the synthetic image compressed at ETC1S quality 128 (compress(), .basis), read back on the
device to RGBA32, against its source -- the pair the stats stage of compress(..., stats=[], stats_hvs=True) sees. Both rasters resident in HBM, 5 warm-up + 50 timed
calls, measured with the library's HIP events around the two launches (bu_hip_profile_*: the clearing of the sums, the block kernel and the sum kernel, not the
copy of the sums to the host). Beside it, the image-metrics kernel on the same pair by the same events, and the flop the block kernel does per pixel (counted from
csrc/psnr_hvs.h: per block and mode 2 x 2 x 64 x 16 for the DCTs, 2 x 5 variances, 2 x 189 for the masking energies, 64 x 8 for the terms, 128 double adds).
Prints one line per figure and one JSON line.
tools/psnr_hvs_bench.py [steps] [warmup] [size]"""
import ctypes as C
import json
import pathlib
import sys

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
import helpers  # noqa: E402
from basis_universal_amd import capi, stats, transcode  # noqa: E402
from basis_universal_amd.compress import compress  # noqa: E402

FLOP_PER_BLOCK_AND_MODE = 2 * 2 * 64 * 16 + 2 * (3 * 64 + 4 * 3 * 16) + 2 * 189 + 64 * 8 + 128


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
    argv = list(sys.argv[1:])
    steps = int(argv[0]) if len(argv) > 0 else 50
    warmup = int(argv[1]) if len(argv) > 1 else 5
    size = int(argv[2]) if len(argv) > 2 else 4096
    ctx = capi.Context(0)
    source = helpers.synth(size, size, 1234)
    decoded = transcode.decode_etc1s_file(bytes(compress(ctx, source, uastc=False, quality=128)))
    d_src, d_dec = ctx.upload(source), ctx.alloc(size * size * 4)
    transcode.transcode_etc1s_image(ctx, decoded, decoded["images"][0], transcode.RGBA32, out_device=d_dec)
    sums, counts = stats.HvsSums(), stats.Counts()
    sums.struct_bytes, counts.struct_bytes = C.sizeof(sums), C.sizeof(counts)
    hvs_ms = timed(ctx, "psnr_hvs", lambda: ctx.check(ctx.lib.k_psnr_hvs(ctx.h, C.c_void_p(d_src), size, size, 0, C.c_void_p(d_dec), size, size, 0, C.byref(sums)),
                                                      "psnr_hvs"), steps, warmup)
    im_ms = timed(ctx, "image_metrics", lambda: ctx.check(ctx.lib.k_image_metrics(ctx.h, C.c_void_p(d_src), size, size, 0, C.c_void_p(d_dec), size, size, 0,
                                                                                   C.byref(counts)), "image_metrics"), steps, warmup)
    ctx.free(d_src); ctx.free(d_dec)
    ctx.close()
    assert sums.blocks == (size // 8) ** 2
    got = stats.reduce_hvs_sums(sums)
    gflops = sums.blocks * 6 * FLOP_PER_BLOCK_AND_MODE / (hvs_ms * 1e-3) / 1e9
    print(f"psnr_hvs      {hvs_ms:8.4f} ms  {sums.blocks} blocks x 6 modes, {gflops:.0f} GFLOP/s of the reference's arithmetic, {hvs_ms / im_ms:.1f} x image_metrics", flush=True)
    print(f"image_metrics {im_ms:8.4f} ms  (same pair, same events)")
    print(f"RGB PSNR-HVS {got['rgb']['psnr_hvs']:.3f} dB, PSNR-HVS-M {got['rgb']['psnr_hvsm']:.3f} dB; 8-bit Y 601 PSNR-HVS-M {got['y_601_8bit']['psnr_hvsm']:.3f} dB")
    print(json.dumps({"image": f"synth{size} seed 1234, ETC1S q128 .basis", "steps": steps, "warmup": warmup, "psnr_hvs_ms": round(hvs_ms, 4),
                      "image_metrics_ms": round(im_ms, 4), "blocks": int(sums.blocks), "gflops": round(gflops, 1),
                      "hvs": {e: {f: round(got[e][f], 3) for f in ("psnr_hvs", "psnr_hvsm")} for e in stats.HVS_ENTRIES}}))


if __name__ == "__main__":
    main()
