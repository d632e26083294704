#!/usr/bin/env python3
"""Time of the block unpack kernel on the 4096x4096 BC7 and BC1 textures that tools/transcode_bench.py's input transcodes to: the synthetic image's level-2 UASTC blocks
resident in HBM, transcoded on the device, then `warmup` + `steps` unpack launches per format, measured with the library's HIP events around the launch
(bu_hip_profile_*). Beside them, from the same process and the same blocks, the UASTC -> RGBA32 transcode: an existing kernel that writes the same 64 MiB raster.
The three are timed in `rounds` alternating passes, so that a drift of the machine shows as a spread and not as a difference. Prints per kernel: ms per launch (mean of the
rounds, and their min .. max), the algorithmic bytes (block bytes in + 64 bytes out per block), bytes per second and their share of the 8 TB/s HBM figure the project's
roofline uses, then one JSON line.   tools/block_unpack_bench.py [steps] [warmup] [rounds]"""
import json
import pathlib
import sys

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
import helpers  # noqa: E402
from basis_universal_amd import capi, transcode, uastc  # noqa: E402

HBM_BYTES_PER_S = 8e12


def main():
    steps = int(sys.argv[1]) if len(sys.argv) > 1 else 50
    warmup = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 3
    ctx = capi.Context(0)
    nbx = nby = 1024
    n = nbx * nby
    d_uastc, d_bc7, d_bc1, d_out = ctx.alloc(n * 16), ctx.alloc(n * 16), ctx.alloc(n * 8), ctx.alloc(n * 64)
    uastc.encode_uastc_blocks(ctx, helpers.to_pixel_blocks(helpers.synth(4096, 4096, 1234)), uastc.LEVEL_DEFAULT, out_device=d_uastc)
    transcode.transcode_uastc_blocks(ctx, d_uastc, nbx, nby, transcode.BC7_RGBA, out_device=d_bc7)
    transcode.transcode_uastc_blocks(ctx, d_uastc, nbx, nby, transcode.BC1_RGB, out_device=d_bc1)
    kernels = [("unpack_bc7", "unpack_blocks", 16, lambda: transcode.unpack_blocks(ctx, d_bc7, nbx, nby, transcode.BC7_RGBA, out_device=d_out)),
               ("unpack_bc1", "unpack_blocks", 8, lambda: transcode.unpack_blocks(ctx, d_bc1, nbx, nby, transcode.BC1_RGB, out_device=d_out)),
               ("uastc_to_rgba32", "uastc_transcode", 16, lambda: transcode.transcode_uastc_blocks(ctx, d_uastc, nbx, nby, transcode.RGBA32, out_device=d_out))]
    times = {name: [] for name, _, _, _ in kernels}
    for _ in range(rounds):
        for name, region, _, run in kernels:
            for _ in range(warmup):
                run()
            ctx.profile_enable(True)
            for _ in range(steps):
                run()
            ms, launches = ctx.profile_read()[region]
            ctx.profile_enable(False)
            assert launches == steps
            times[name].append(ms / steps)
    rows = {}
    for name, _, unit, _ in kernels:
        ms, traffic = sum(times[name]) / rounds, n * (unit + 64)
        rows[name] = {"ms": round(ms, 4), "ms_min": round(min(times[name]), 4), "ms_max": round(max(times[name]), 4), "algorithmic_mb": round(traffic / 1e6, 1),
                      "tb_per_s": round(traffic / (ms * 1e-3) / 1e12, 3), "fraction_of_8tbps": round(traffic / (ms * 1e-3) / HBM_BYTES_PER_S, 4)}
        print(f"{name:16s} {ms:8.4f} ms ({min(times[name]):.4f} .. {max(times[name]):.4f})  {traffic / 1e6:6.1f} MB  {traffic / (ms * 1e-3) / 1e12:6.3f} TB/s  "
              f"{100 * traffic / (ms * 1e-3) / HBM_BYTES_PER_S:6.2f} % of 8 TB/s", flush=True)
    for d in (d_uastc, d_bc7, d_bc1, d_out):
        ctx.free(d)
    ctx.close()
    print(json.dumps({"image": "synth4096 seed 1234, UASTC level 2 -> BC7 / BC1 on the device", "steps": steps, "warmup": warmup, "rounds": rounds, "kernels": rows}))


if __name__ == "__main__":
    main()
