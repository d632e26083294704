#!/usr/bin/env python3
"""Time of the UASTC transcode kernel per target on the 4096x4096 synthetic image: level-2 blocks resident in HBM, 5 warm-up + 50 timed launches per target, measured
with the library's HIP events around the launch (bu_hip_profile_*). Prints per target: ms per launch, Gblocks/s, and the algorithmic bytes (16 in + the target's bytes out
per block) over time as a fraction of the 8 TB/s HBM figure the project's roofline uses.   tools/transcode_bench.py [steps] [warmup]"""
import json
import pathlib
import sys

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
import helpers  # noqa: E402
from basis_universal_amd import capi, transcode, uastc  # noqa: E402

HBM_BYTES_PER_S = 8e12
TARGETS = [("rgba32", transcode.RGBA32, False), ("astc", transcode.ASTC_4x4_RGBA, False), ("bc7", transcode.BC7_RGBA, False), ("bc1", transcode.BC1_RGB, False),
           ("bc1_hq", transcode.BC1_RGB, True), ("bc3", transcode.BC3_RGBA, False), ("bc3_hq", transcode.BC3_RGBA, True), ("bc4_r", transcode.BC4_R, False),
           ("bc5_ra", transcode.BC5_RG, False)]


def main():
    steps = int(sys.argv[1]) if len(sys.argv) > 1 else 50
    warmup = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    ctx = capi.Context(0)
    nbx = nby = 1024
    n = nbx * nby
    d_blocks, d_out = ctx.alloc(n * 16), ctx.alloc(n * 64)
    uastc.encode_uastc_blocks(ctx, helpers.to_pixel_blocks(helpers.synth(4096, 4096, 1234)), uastc.LEVEL_DEFAULT, out_device=d_blocks)
    rows = {}
    for name, target, hq in TARGETS:
        for _ in range(warmup):
            transcode.transcode_uastc_blocks(ctx, d_blocks, nbx, nby, target, high_quality=hq, out_device=d_out)
        ctx.profile_enable(True)
        for _ in range(steps):
            transcode.transcode_uastc_blocks(ctx, d_blocks, nbx, nby, target, high_quality=hq, out_device=d_out)
        ms, launches = ctx.profile_read()["uastc_transcode"]
        ctx.profile_enable(False)
        assert launches == steps
        ms /= steps
        traffic = n * (16 + transcode.BYTES_PER_BLOCK[target])
        rows[name] = {"ms": round(ms, 4), "gblocks_per_s": round(n / ms / 1e6, 2), "algorithmic_mb": round(traffic / 1e6, 1),
                      "fraction_of_8tbps": round(traffic / (ms * 1e-3) / HBM_BYTES_PER_S, 4)}
        print(f"{name:8s} {ms:8.4f} ms  {n / ms / 1e6:7.2f} Gblocks/s  {traffic / 1e6:6.1f} MB  {100 * traffic / (ms * 1e-3) / HBM_BYTES_PER_S:6.2f} % of 8 TB/s", flush=True)
    ctx.free(d_blocks)
    ctx.free(d_out)
    ctx.close()
    print(json.dumps({"image": "synth4096 seed 1234, UASTC level 2", "steps": steps, "warmup": warmup, "targets": rows}))


if __name__ == "__main__":
    main()
