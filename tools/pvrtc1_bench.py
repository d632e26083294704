#!/usr/bin/env python3
"""Time of the four PVRTC1 routes on the two workloads the other transcoder benches use, 1,048,576 resident blocks each (4096x4096, a power of two):
  ETC1S  the synthetic image compressed at quality 128 (compress(), .basis), palettes and indices resident (tools/etc1s_transcode_bench.py's workload). The file has
         no alpha slice, so the RGBA route reads the colour slice's index arrays a second time as its alpha slice: the same traffic and arithmetic as a real one.
  UASTC  the image's level-2 blocks resident (tools/uastc_texture_bench.py's workload).
In the same run, as the yardsticks: ETC1S -> BC1 (first family), UASTC -> RGBA32 and UASTC -> BC1. Per case and round, after `warmup` calls, `steps` calls with the
output resident, each measured twice: launch = the library's HIP events around the call's launches (bu_hip_profile_*: the counter memset plus the kernel, for PVRTC1
both kernels), call = the whole call on the host's clock (launches, stream wait, read-back of the counter); the median over the steps. The cases are run `rounds`
times, interleaved, and the JSON gives every round's median and their spread. Algorithmic bytes: the source block (4 B of indices, 8 B with an alpha slice, or 16 B)
in, the target's bytes out, and for PVRTC1 the workspace word written once and read nine times through the caches (counted once each way: 8 B).
Prints one line per figure and one JSON line.   tools/pvrtc1_bench.py [steps] [warmup] [rounds] [size]"""
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
from basis_universal_amd import capi, transcode as T, uastc  # noqa: E402
from basis_universal_amd.compress import compress  # noqa: E402

HBM_BYTES_PER_S = 8e12


def main():
    steps = int(sys.argv[1]) if len(sys.argv) > 1 else 50
    warmup = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 3
    size = int(sys.argv[4]) if len(sys.argv) > 4 else 4096
    ctx = capi.Context(0)
    source = helpers.synth(size, size, 1234)
    decoded = T.decode_etc1s_file(bytes(compress(ctx, source, uastc=False, quality=128)))
    im = decoded["images"][0]
    nbx, nby = im["num_blocks_x"], im["num_blocks_y"]
    n = nbx * nby
    ep, sel = np.ascontiguousarray(decoded["endpoint_palette"]), np.ascontiguousarray(decoded["selector_palette"])
    d = [ctx.upload(ep), ctx.upload(sel), ctx.upload(im["endpoint_indices"]), ctx.upload(im["selector_indices"])]
    d_blocks, d_out = ctx.alloc(n * 16), ctx.alloc(n * 64)
    uastc.encode_uastc_blocks(ctx, helpers.to_pixel_blocks(source), uastc.LEVEL_DEFAULT, out_device=d_blocks)
    print(f"{n} blocks, {decoded['num_endpoints']} endpoints, {decoded['num_selectors']} selectors", flush=True)

    def etc1s_pvrtc1(target, alpha):
        def call():
            invalid = C.c_uint32(0)
            ctx.check(ctx.lib.k_transcode_etc1s_pvrtc1_counted(ctx.h, C.c_void_p(d[0]), ep.shape[0], C.c_void_p(d[1]), sel.size, C.c_void_p(d[2]), C.c_void_p(d[3]),
                                                               C.c_void_p(d[2]) if alpha else None, C.c_void_p(d[3]) if alpha else None, nbx, nby, size, size, target,
                                                               C.c_void_p(d_out), 0, C.byref(invalid)), "transcode_etc1s_pvrtc1")
            assert invalid.value == 0
        return call

    def etc1s_bc1():
        invalid = C.c_uint32(0)
        ctx.check(ctx.lib.k_transcode_etc1s_counted(ctx.h, C.c_void_p(d[0]), ep.shape[0], C.c_void_p(d[1]), sel.size, C.c_void_p(d[2]), C.c_void_p(d[3]), None, None, nbx, nby, size,
                                                    size, T.BC1_RGB, C.c_void_p(d_out), 0, 0, C.byref(invalid)), "transcode_etc1s")
        assert invalid.value == 0
    # name -> (call, the profile region of its launches, algorithmic bytes per block)
    cases = {"etc1s_bc1": (etc1s_bc1, "etc1s_transcode", 4 + 8),
             "etc1s_pvrtc1_rgb": (etc1s_pvrtc1(T.PVRTC1_4_RGB, False), "transcode_etc1s_pvrtc1", 4 + 8 + 8),
             "etc1s_pvrtc1_rgba": (etc1s_pvrtc1(T.PVRTC1_4_RGBA, True), "transcode_etc1s_pvrtc1", 8 + 8 + 8),
             "uastc_rgba32": (lambda: T.transcode_uastc_blocks(ctx, d_blocks, nbx, nby, T.RGBA32, out_device=d_out), "uastc_transcode", 16 + 64),
             "uastc_bc1": (lambda: T.transcode_uastc_blocks(ctx, d_blocks, nbx, nby, T.BC1_RGB, out_device=d_out), "uastc_transcode", 16 + 8),
             "uastc_pvrtc1_rgb": (lambda: T.transcode_uastc_pvrtc1_blocks(ctx, d_blocks, nbx, nby, T.PVRTC1_4_RGB, out_device=d_out), "transcode_uastc_pvrtc1", 2 * 16 + 8 + 8),
             "uastc_pvrtc1_rgba": (lambda: T.transcode_uastc_pvrtc1_blocks(ctx, d_blocks, nbx, nby, T.PVRTC1_4_RGBA, out_device=d_out), "transcode_uastc_pvrtc1", 2 * 16 + 8 + 8)}
    per_round = {name: {"launch_ms": [], "call_ms": []} for name in cases}
    for r in range(rounds):
        for name, (call, scope, _) in cases.items():
            for _ in range(warmup):
                call()
            launch_ms, call_ms = [], []
            for _ in range(steps):
                ctx.profile_enable(True)
                t0 = time.perf_counter()
                call()
                call_ms.append((time.perf_counter() - t0) * 1e3)
                ms, _launches = ctx.profile_read()[scope]
                ctx.profile_enable(False)
                launch_ms.append(ms)
            per_round[name]["launch_ms"].append(round(float(np.median(launch_ms)), 4))
            per_round[name]["call_ms"].append(round(float(np.median(call_ms)), 4))
            print(f"round {r} {name:18s} launch {np.median(launch_ms):8.4f} ms ({min(launch_ms):.4f}..{max(launch_ms):.4f})  call {np.median(call_ms):8.4f} ms", flush=True)
    rows = {}
    for name, (_, _, bytes_per_block) in cases.items():
        launch, whole = per_round[name]["launch_ms"], per_round[name]["call_ms"]
        ms, traffic = float(np.median(launch)), n * bytes_per_block
        rows[name] = {"launch_ms": round(ms, 4), "launch_ms_per_round": launch, "launch_spread_percent": round(100 * (max(launch) - min(launch)) / ms, 1),
                      "call_ms": round(float(np.median(whole)), 4), "call_ms_per_round": whole, "gblocks_per_s": round(n / ms / 1e6, 2), "algorithmic_mb": round(traffic / 1e6, 1),
                      "fraction_of_8tbps": round(traffic / (ms * 1e-3) / HBM_BYTES_PER_S, 4)}
        print(f"{name:18s} launch {ms:8.4f} ms (rounds {launch})  call {np.median(whole):8.4f} ms  {n / ms / 1e6:7.2f} Gblocks/s  {traffic / 1e6:6.1f} MB  "
              f"{100 * traffic / (ms * 1e-3) / HBM_BYTES_PER_S:6.2f} % of 8 TB/s", flush=True)
    for p in d + [d_blocks, d_out]:
        ctx.free(p)
    ctx.close()
    print(json.dumps({"image": f"synth{size} seed 1234: ETC1S q128 .basis, and UASTC level 2; {n} blocks", "steps": steps, "warmup": warmup, "rounds": rounds, "cases": rows}))


if __name__ == "__main__":
    main()
