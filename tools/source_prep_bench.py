#!/usr/bin/env python3
"""Time of the source preparation kernels on a 4096x4096 RGBA8 raster resident in HBM (a seeded normal-map-like image with an alpha channel), beside a plain
device-to-device copy of the same raster from the same process as the yardstick:
  prepare_source   every option on: renormalise, swizzle "bgra", alpha check, vertical flip; 64 MiB read + 64 MiB written
  prepare_plain    the same pass without the renormalisation (swizzle, alpha check, flip): its bandwidth half
  split_alpha      64 MiB read + 128 MiB written
  copy_d2d         bu_hip_memcpy_d2d of the raster: 64 MiB read + 64 MiB written
Two clocks. `event_ms`: the library's HIP events around the launch (bu_hip_profile_*), for the kernels. `batch_ms`: a host clock around `steps` calls enqueued back to
back and one synchronise, per call, for split_alpha and the copy -- the copy has no event region, and prepare_source synchronises in every call (it returns the alpha flag),
so its host time per call is printed as `call_ms` and includes that wait. All are timed in `rounds` alternating passes; printed are the mean of the rounds and
their min .. max, the algorithmic bytes, bytes per second, and each kernel's time over the copy's (prepare_*: event_ms / copy batch_ms; split_alpha: batch_ms /
batch_ms), then one JSON line. Nothing is asserted: the ratio is reported.   tools/source_prep_bench.py [steps] [warmup] [rounds]"""
import json
import pathlib
import sys
import time

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from basis_universal_amd import capi, source  # noqa: E402

SIDE = 4096
MIB = SIDE * SIDE * 4


def image(seed=1234):
    rng = np.random.default_rng(seed)
    img = rng.integers(0, 256, (SIDE, SIDE, 4), dtype=np.uint8)
    img[::7, ::5, :3] = 128
    return img


def main():
    steps = int(sys.argv[1]) if len(sys.argv) > 1 else 50
    warmup = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 3
    ctx = capi.Context(0)
    d_src, d_dst, d_alpha = ctx.upload(image()), ctx.alloc(MIB), ctx.alloc(MIB)
    options = dict(renormalize=True, swizzle="bgra", check_for_alpha=True, y_flip=True)
    runs = {"prepare_source": lambda: source.prepare_resident(ctx, d_src, SIDE, SIDE, d_dst, **options),
            "prepare_plain": lambda: source.prepare_resident(ctx, d_src, SIDE, SIDE, d_dst, **dict(options, renormalize=False)),
            "split_alpha": lambda: source.split_alpha_resident(ctx, d_src, SIDE, SIDE, d_dst, d_alpha),
            "copy_d2d": lambda: ctx.check(ctx.lib.memcpy_d2d(ctx.h, d_dst, d_src, MIB), "memcpy_d2d")}
    traffic = {"prepare_source": 2 * MIB, "prepare_plain": 2 * MIB, "split_alpha": 3 * MIB, "copy_d2d": 2 * MIB}
    event, batch = {k: [] for k in runs}, {k: [] for k in runs}
    for _ in range(rounds):
        for name, run in runs.items():
            for _ in range(warmup):
                run()
            ctx.sync()
            t0 = time.perf_counter()
            for _ in range(steps):
                run()
            ctx.sync()
            batch[name].append((time.perf_counter() - t0) * 1e3 / steps)
            if name != "copy_d2d":
                ctx.profile_enable(True)
                for _ in range(steps):
                    run()
                ms, launches = ctx.profile_read()["split_alpha" if name == "split_alpha" else "prepare_source"]
                ctx.profile_enable(False)
                assert launches == steps
                event[name].append(ms / steps)
    mean = lambda v: sum(v) / len(v)
    copy_ms = mean(batch["copy_d2d"])
    rows = {}
    for name in runs:
        own = event[name] if name.startswith("prepare") else batch[name]      # the figure the ratio uses
        ms = mean(own)
        rows[name] = {"ms": round(ms, 4), "ms_min": round(min(own), 4), "ms_max": round(max(own), 4), "clock": "event" if name.startswith("prepare") else "batch",
                      "event_ms": round(mean(event[name]), 4) if event[name] else None,
                      ("call_ms" if name.startswith("prepare") else "batch_ms"): round(mean(batch[name]), 4),
                      "algorithmic_mb": round(traffic[name] / 1e6, 1), "tb_per_s": round(traffic[name] / (ms * 1e-3) / 1e12, 3), "over_copy": round(ms / copy_ms, 3)}
        print(f"{name:15s} {ms:8.4f} ms ({min(own):.4f} .. {max(own):.4f}, {rows[name]['clock']})  {traffic[name] / 1e6:6.1f} MB  {traffic[name] / (ms * 1e-3) / 1e12:6.3f} TB/s  "
              f"{ms / copy_ms:5.2f} x the copy" + (f"   events {mean(event[name]):.4f} ms" if event[name] else "") +
              (f"   per call with its synchronise {mean(batch[name]):.4f} ms" if name.startswith("prepare") else ""), flush=True)
    for d in (d_src, d_dst, d_alpha):
        ctx.free(d)
    ctx.close()
    print(json.dumps({"image": f"{SIDE}x{SIDE} RGBA8, seed 1234", "steps": steps, "warmup": warmup, "rounds": rounds, "kernels": rows}))


if __name__ == "__main__":
    main()
