#!/usr/bin/env python3
"""bu_hip_k_ssim (csrc/ssim_kernels.hip) timed on seeded pairs (the synthetic image against itself +-7 noise) of 1024x1024 and 4096x4096 pixels, both rasters resident
in HBM. After the warm-up calls, `steps` calls are timed as a whole on the host clock; every call ends with the library's wait for the stream (it copies the seven
floats out), so the device synchronise is inside the timed window. Reported per size: ms per call, Mpix/s, the seven figures, how many of the reduction's chunks were
added one by one, and the map kernels' arithmetic from the shapes -- 121 taps x 5 filtered images x C channels, one multiply and one add each (C = 4 for the RGBA
launch, 2 for the launch that does channel 0 of both luma calls), plus per tap and channel 3 products (a a, b b, a b) and 2 byte-to-float conversions -- against the
VALU issue ceiling those instructions have at the prices of tools/valu_calib.hip (2.2 cycles per wave64 f32 add / mul, 4.1 per conversion; 1024 SIMDs).

  tools/ssim_bench.py [steps] [warmup] [sizes, comma separated]     the timing; one JSON line at the end
  tools/ssim_bench.py --kernels [size]                              3 calls and nothing else: the program to put after `rocprofv3 --kernel-trace --stats --`
  tools/ssim_bench.py --kernel-stats FILE.csv                       sums a rocprofv3 kernel_stats csv into map / reduction time per call
  tools/ssim_bench.py --reference [size]                            build machine only: wall time of oracle/_ref/basisu -compare -compare_ssim minus the same
                                                                    command without -compare_ssim (one CPU thread)"""
import csv
import ctypes as C
import json
import pathlib
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
import helpers  # noqa: E402

PROFILE_CALLS = 3
CHANNELS = 4 + 2                                   # channels filtered per pixel over the two map launches
MUL_ADD_PER_PIXEL = 121 * 5 * CHANNELS * 2         # the issue's count: 121 x 5 x C multiply + add
PRODUCTS_PER_PIXEL = 121 * 3 * CHANNELS
CONVERSIONS_PER_PIXEL = 121 * 2 * CHANNELS
SIMD_CYCLES_PER_WAVE = (MUL_ADD_PER_PIXEL + PRODUCTS_PER_PIXEL) * 2.2 + CONVERSIONS_PER_PIXEL * 4.1    # per 64 pixels


def seeded_pair(size):
    a = helpers.synth(size, size, 1234)
    rng = np.random.default_rng(99)
    a[..., 3] = rng.integers(0, 256, (size, size), dtype=np.uint8)
    b = np.clip(a.astype(np.int16) + rng.integers(-7, 8, a.shape, dtype=np.int16), 0, 255).astype(np.uint8)
    return a, b


def run_calls(size, calls, warmup):
    from basis_universal_amd import capi, stats
    ctx = capi.Context(0)
    a, b = seeded_pair(size)
    d_a, d_b = ctx.upload(a), ctx.upload(b)
    r = stats.SsimResult()
    r.struct_bytes = C.sizeof(r)

    def call():
        ctx.check(ctx.lib.k_ssim(ctx.h, C.c_void_p(d_a), size, size, 0, C.c_void_p(d_b), size, size, 0, C.byref(r)), "ssim")
    for _ in range(warmup):
        call()
    t0 = time.perf_counter()
    for _ in range(calls):
        call()
    ms = (time.perf_counter() - t0) * 1e3 / calls
    ctx.free(d_a); ctx.free(d_b)
    ctx.close()
    return ms, r


def kernel_stats(path):
    """rocprofv3's kernel_stats csv -> (ms in the map kernels, ms in the four reduction kernels) per call of PROFILE_CALLS"""
    groups = {"map": 0.0, "reduction": 0.0}
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            name = row.get("Name") or row.get("KernelName") or ""
            total = float(row.get("TotalDurationNs") or row.get("TotalDuration(ns)") or 0.0)
            if "ssim_map_kernel" in name:
                groups["map"] += total
            elif "ssim_" in name:
                groups["reduction"] += total
            if "ssim_" in name:
                print(f"  {name[:70]:70s} {row.get('Calls')} calls {total / 1e6 / PROFILE_CALLS:9.4f} ms per bu_hip_k_ssim")
    return groups["map"] / 1e6 / PROFILE_CALLS, groups["reduction"] / 1e6 / PROFILE_CALLS


def reference_seconds(size):
    basisu = ROOT / "oracle" / "_ref" / "basisu"
    assert basisu.exists(), "oracle/_ref/basisu is missing: build it on the build machine (make -C oracle ref)"
    a, b = seeded_pair(size)
    with tempfile.TemporaryDirectory() as d:
        helpers.save_png(pathlib.Path(d) / "a.png", a)
        helpers.save_png(pathlib.Path(d) / "b.png", b)
        out = {}
        for name, extra in (("with", ["-compare_ssim"]), ("without", [])):
            best = None
            for _ in range(3):
                t0 = time.perf_counter()
                subprocess.run([str(basisu), "-compare", *extra, "a.png", "b.png"], cwd=d, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, check=True)
                dt = time.perf_counter() - t0
                best = dt if best is None else min(best, dt)
            out[name] = best
    return out["with"] - out["without"], out


def main():
    argv = list(sys.argv[1:])
    if argv and argv[0] == "--kernels":
        size = int(argv[1]) if len(argv) > 1 else 4096
        ms, r = run_calls(size, PROFILE_CALLS, 0)
        print(f"{PROFILE_CALLS} calls at {size}x{size}, {ms:.3f} ms each under the profiler")
        return
    if argv and argv[0] == "--kernel-stats":
        m, r = kernel_stats(argv[1])
        print(json.dumps({"map_ms": round(m, 4), "reduction_ms": round(r, 4), "calls": PROFILE_CALLS}))
        return
    if argv and argv[0] == "--reference":
        size = int(argv[1]) if len(argv) > 1 else 1024
        s, both = reference_seconds(size)
        print(json.dumps({"size": size, "reference_ssim_seconds": round(s, 3), "with": round(both["with"], 3), "without": round(both["without"], 3)}))
        return
    steps = int(argv[0]) if len(argv) > 0 else 20
    warmup = int(argv[1]) if len(argv) > 1 else 3
    sizes = [int(s) for s in argv[2].split(",")] if len(argv) > 2 else [1024, 4096]
    results = []
    for size in sizes:
        ms, r = run_calls(size, steps, warmup)
        pixels = size * size
        ceiling_ms_at_2ghz = pixels / 64 * SIMD_CYCLES_PER_WAVE / 1024 / 2.0e9 * 1e3
        figures = {k: float(getattr(r, k)) for k in ("r", "g", "b", "rgb", "a", "luma_709", "luma_601")}
        print(f"ssim {size}x{size}: {ms:9.3f} ms per call, {pixels / ms / 1e3:8.1f} Mpix/s; {MUL_ADD_PER_PIXEL * pixels / ms / 1e6:8.1f} GFLOP/s of filter multiply-adds; "
              f"chunks {r.chunks}, added one by one {r.chunks_walked}; VALU issue floor of the map kernels at 2.0 GHz {ceiling_ms_at_2ghz:.3f} ms", flush=True)
        print("   " + " ".join(f"{k} {v:.6f}" for k, v in figures.items()))
        results.append({"size": size, "ms": round(ms, 4), "mpix_per_s": round(pixels / ms / 1e3, 1), "chunks": int(r.chunks), "chunks_walked": int(r.chunks_walked),
                        "valu_floor_ms_at_2ghz": round(ceiling_ms_at_2ghz, 4), "figures": {k: round(v, 6) for k, v in figures.items()}})
    print(json.dumps({"pair": "synth seed 1234 with random alpha, +-7 noise", "steps": steps, "warmup": warmup, "results": results}))


if __name__ == "__main__":
    main()
