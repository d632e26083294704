#!/usr/bin/env python3
"""Time of bringing a .dds source's mip chain to the device (basis_universal_amd/source.py: DdsSources.resident, bu_hip_k_prepare_mip_levels) against the same
rasters built from the calls the package had before, on a texture of a size users compress: a 4096x4096 B8G8R8A8 .dds file with its 13 levels (89.5 MB of pixels;
every level an independent synthetic image).

  one_launch : the file's payload uploaded once as it is, ONE launch for the byte order of all 13 levels, one wait for the 13 alpha flags.
  per_level  : per level a byte swap on the host (numpy), then source.prepare_source: an upload, a prepare launch and a wait for its flag, 13 times.
Both start from the file's bytes in host memory and end with 13 resident RGBA rasters and their alpha flags; both are on the host clock and end in a blocking
device-to-host copy. The rasters and flags of the two are compared once, outside the timing. `kernel` is the one launch alone, HIP events around it
(bu_hip_profile_*), in passes of its own with the profiler on. `compress_dds` is the whole call, file bytes to .basis bytes, ETC1S q128 and UASTC level 2.
`warmup` calls, then `steps` timed calls per round, `rounds` rounds that alternate over the two ways so that a drift of the machine shows as a spread. Reported: the
median of all timed calls and their min .. max. No threshold is asserted: these are the first measurements of this path.
Prints one line per figure and writes the JSON.   tools/mip_levels_bench.py [steps] [warmup] [rounds] [out.json]"""
import json
import pathlib
import statistics
import sys
import time

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
import helpers  # noqa: E402
import mip_levels_helpers as L  # noqa: E402
from basis_universal_amd import capi, dds, source  # noqa: E402

SIZE = 4096


def summary(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4), "samples": len(ms)}


def one_launch(ctx, parsed):
    """-> (owned, rasters, flags)"""
    owned = []
    ((rasters, flags),) = source.DdsSources([parsed], True).resident(ctx, owned, None)
    return owned, rasters, flags


def per_level(ctx, parsed):
    owned, rasters, flags = [], [], []
    for lv in parsed["levels"]:
        stored = parsed["payload"][lv["offset"]:lv["offset"] + lv["nbytes"]].reshape(lv["height"], lv["width"], 4)
        rgba = np.ascontiguousarray(stored[..., L.ORDERS[parsed["byte_order"]]])        # the host byte swap
        d, _, has_alpha = source.prepare_source(ctx, rgba)
        owned.append(d)
        rasters.append(d)
        flags.append(has_alpha)
    return owned, rasters, flags


def release(ctx, owned):
    for d in owned:
        ctx.free(d)


def main():
    steps, warmup, rounds = (int(sys.argv[i]) if len(sys.argv) > i else v for i, v in ((1, 10), (2, 2), (3, 3)))
    out_path = pathlib.Path(sys.argv[4]) if len(sys.argv) > 4 else ROOT / "profiles" / "mip_levels_bench.json"
    levels = [helpers.synth(SIZE, SIZE, 1234)] + [L.level_image(max(1, SIZE >> k), max(1, SIZE >> k), 1234 + k) for k in range(1, SIZE.bit_length())]
    levels[5][3, 7, 3] = 200                                        # one level with alpha, so that the flags are not all alike
    data = L.dds_file(levels, order="bgra")
    parsed = dds.read_dds_source(data)
    assert len(parsed["levels"]) == 13 and parsed["byte_order"] == "bgra"
    ctx = capi.Context(0)

    # the two ways give the same rasters and flags
    a, b = one_launch(ctx, parsed), per_level(ctx, parsed)
    for lv, da, db, want in zip(parsed["levels"], a[1], b[1], levels):
        shape = (lv["height"], lv["width"], 4)
        ra, rb = ctx.download(da, shape, np.uint8), ctx.download(db, shape, np.uint8)
        assert (ra == want).all() and (rb == want).all(), lv
    assert a[2] == b[2] == [k == 5 for k in range(13)], (a[2], b[2])
    release(ctx, a[0]); release(ctx, b[0])

    ways = {"one_launch": one_launch, "per_level": per_level}
    times, kernel = {k: [] for k in ways}, []
    for _ in range(rounds):
        for name, fn in ways.items():
            for _ in range(warmup):
                release(ctx, fn(ctx, parsed)[0])
            for _ in range(steps):
                t0 = time.perf_counter()
                owned, _, _ = fn(ctx, parsed)                    # ends in a blocking copy of the flag(s)
                times[name].append((time.perf_counter() - t0) * 1e3)
                release(ctx, owned)
        for _ in range(steps):                                       # the launch alone, profiler on: a pass of its own
            ctx.profile_enable(True)
            owned, _, _ = one_launch(ctx, parsed)
            ms, launches = ctx.profile_read()["prepare_mip_levels"]
            ctx.profile_enable(False)
            release(ctx, owned)
            assert launches == 1
            kernel.append(ms)
    pixels = sum(lv["width"] * lv["height"] for lv in parsed["levels"])
    report = {"file_bytes": int(data.size), "levels": 13, "pixels": pixels, "steps": steps, "warmup": warmup, "rounds": rounds,
              "one_launch_file_bytes_to_resident_rasters": summary(times["one_launch"]), "per_level_byte_swap_and_prepare_source": summary(times["per_level"]),
              "prepare_mip_levels_kernel_device_only": summary(kernel)}
    report["kernel_gbytes_per_s_read_plus_written"] = round(2 * 4 * pixels / (report["prepare_mip_levels_kernel_device_only"]["median_ms"] * 1e-3) / 1e9, 1)
    for key in ("one_launch_file_bytes_to_resident_rasters", "per_level_byte_swap_and_prepare_source", "prepare_mip_levels_kernel_device_only"):
        s = report[key]
        print(f"{key:48s} {s['median_ms']:10.4f} ms ({s['min_ms']:.4f} .. {s['max_ms']:.4f}), {s['samples']} samples", flush=True)

    # the whole call: .dds bytes in host memory -> .basis bytes in host memory
    for name, kw in (("compress_dds_etc1s_q128", dict()), ("compress_dds_uastc_level2", dict(uastc=True))):
        call = []
        for _ in range(warmup):
            dds.compress_dds(ctx, data, **kw)
        for _ in range(steps * rounds):
            t0 = time.perf_counter()
            out = dds.compress_dds(ctx, data, **kw)
            call.append((time.perf_counter() - t0) * 1e3)
        report[name] = dict(summary(call), basis_bytes=int(out.size))
        s = report[name]
        print(f"{name:48s} {s['median_ms']:10.3f} ms ({s['min_ms']:.3f} .. {s['max_ms']:.3f}), {s['samples']} samples, {out.size} bytes", flush=True)
    ctx.close()
    out_path.parent.mkdir(parents=True, exist_ok=True)
    out_path.write_text(json.dumps(report, indent=1, sort_keys=True) + "\n")
    print(json.dumps(report, sort_keys=True))


if __name__ == "__main__":
    main()
