#!/usr/bin/env python3
"""Reading a whole file back, measured: every image of a .basis / .ktx2 file transcoded (a) by the loop of one-image calls -- the file parsed or decoded once, then
transcode_uastc_blocks / transcode_etc1s_image per image, as stats.py read files back before the whole-file calls existed -- and (b) by ONE whole-file call
(transcode_file_images / transcode_etc1s_file_images), alternating in the same process.

Workloads: `uastc_mips_4096` -- one 4096x4096 UASTC image with its mip chain (13 images, one of them 75 % of the blocks: the case the change is NOT about);
`etc1s_cubemap_1024` -- six 1024x1024 ETC1S faces with mips (66 images); `etc1s_array_alpha_256` -- 64 layers of 256x256 ETC1S with alpha (64 images, 128 slices).
Targets: RGBA32 and BC1. Both sides return host arrays, so both include their downloads; the ETC1S sides both include one host decode of the file, which is
reported on its own (`host_decode`) so that the device part can be told from it.
Times are host clock over windows of at least --window seconds of back-to-back files, each window ending in a stream synchronise, after a warm-up of both sides;
per side the median and the extremes of --windows windows, in ms per file. Launches (profiled regions, bu_hip_profile_*) and host waits (calls that the header
documents as synchronising: blocking copies and the one-image / whole-file entries that read their counters back) per file are counted in a separate pass, not timed.
--stats: compress(..., stats=[]) on the 64-layer case, the whole call by the host clock (run it on two trees to compare). One JSON line per workload and target.
usage: transcode_slices_bench.py [--workload NAME|all] [--windows N] [--window SECONDS] [--stats] [--out FILE]"""
import argparse
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
from basis_universal_amd import capi  # noqa: E402
from basis_universal_amd import transcode as T  # noqa: E402
from basis_universal_amd.compress import compress  # noqa: E402

WAITING_CALLS = ("memcpy_h2d", "memcpy_d2h", "k_transcode_uastc", "k_transcode_etc1s_counted", "k_transcode_uastc_slices", "k_transcode_etc1s_slices")


def with_alpha(img, seed):
    h, w = img.shape[:2]
    yy, xx = np.mgrid[0:h, 0:w]
    out = img.copy()
    out[..., 3] = np.clip(128 + 100 * np.sin((xx + seed) / 17.0) * np.cos(yy / 13.0), 0, 255).astype(np.uint8)
    return out


def workloads():
    return {"uastc_mips_4096": (lambda: np.ascontiguousarray(helpers.synth(4096, 4096, 921)), dict(uastc=True, mipmaps=True), True),
            "etc1s_cubemap_1024": (lambda: [helpers.synth(1024, 1024, 910 + i) for i in range(6)], dict(tex_type="cubemap", mipmaps=True), False),
            "etc1s_array_alpha_256": (lambda: [with_alpha(helpers.synth(256, 256, 930 + i), i) for i in range(64)], dict(tex_type="2darray"), False)}


def per_image(ctx, data, target, uastc):
    """(a): the file parsed / decoded once, then one call per image"""
    if uastc:
        raw = data.tobytes()
        return [T.transcode_uastc_blocks(ctx, np.frombuffer(raw, np.uint8, im["length"], im["offset"]).reshape(-1, 16), im["num_blocks_x"], im["num_blocks_y"], target,
                                         width=im["width"], height=im["height"]) for im in T.read_uastc_file(raw)["images"]]
    decoded = T.decode_etc1s_file(data)
    return [T.transcode_etc1s_image(ctx, decoded, im, target) for im in decoded["images"]]


def whole_file(ctx, data, target, uastc):
    """(b): one call"""
    return T.transcode_file_images(ctx, data, target) if uastc else T.transcode_etc1s_file_images(ctx, data, target)


def window(ctx, fn, seconds):
    """back-to-back files for at least `seconds`, ending in a synchronise -> ms per file"""
    n, t0 = 0, time.perf_counter()
    while True:
        fn()
        n += 1
        if time.perf_counter() - t0 >= seconds:
            break
    ctx.sync()
    return (time.perf_counter() - t0) * 1e3 / n


def summary(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}


def counted(ctx, fn):
    """-> (launches by profiled region, calls that wait for the stream) of one fn()"""
    waits, originals = {}, {name: getattr(ctx.lib, name) for name in WAITING_CALLS}

    def counting(name):
        def call(*args):
            waits[name] = waits.get(name, 0) + 1
            return originals[name](*args)
        return call
    for name in WAITING_CALLS:
        setattr(ctx.lib, name, counting(name))
    ctx.profile_enable(True)
    try:
        fn()
        launches = {k: n for k, (_, n) in ctx.profile_read().items()}
    finally:
        ctx.profile_enable(False)
        for name, f in originals.items():
            setattr(ctx.lib, name, f)
    return launches, waits


def run(ctx, name, data, uastc, target, windows, seconds):
    a = lambda: per_image(ctx, data, target, uastc)   # noqa: E731
    b = lambda: whole_file(ctx, data, target, uastc)  # noqa: E731
    same = all(x.shape == y.shape and bool((x == y).all()) for x, y in zip(a(), b()))   # faster and different is not faster; also the first warm-up of both
    for _ in range(2):
        a()
        b()
    ms_a, ms_b = [], []
    for _ in range(windows):                                # alternating, so that both sides see the same machine
        ms_a.append(window(ctx, a, seconds))
        ms_b.append(window(ctx, b, seconds))
    launches_a, waits_a = counted(ctx, a)
    launches_b, waits_b = counted(ctx, b)
    images = (T.read_uastc_file(data.tobytes()) if uastc else T.read_etc1s_file(data))["images"]
    out = {"workload": name, "target": {T.RGBA32: "RGBA32", T.BC1_RGB: "BC1"}[target], "images": len(images), "slices": len(images) + sum(bool(im.get("has_alpha")) for im in images) * (not uastc),
           "blocks": sum(im["num_blocks_x"] * im["num_blocks_y"] for im in images), "file_bytes": int(data.size), "identical": same,
           "per_image_calls": summary(ms_a), "whole_file_call": summary(ms_b), "launches_per_image_calls": sum(launches_a.values()), "launches_whole_file_call": sum(launches_b.values()),
           "host_waits_per_image_calls": sum(waits_a.values()), "host_waits_whole_file_call": sum(waits_b.values()), "waits_by_call_per_image": waits_a, "waits_by_call_whole_file": waits_b,
           "windows": windows, "window_seconds": seconds}
    if not uastc:
        out["host_decode"] = summary([window(ctx, lambda: T.decode_etc1s_file(data), min(seconds, 0.25)) for _ in range(3)])
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="all", choices=[*workloads(), "all"])
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--stats", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    ctx = capi.Context(0)       # no device, no numbers: this raises
    lines = []
    for name, (make, kw, uastc) in workloads().items():
        if args.workload not in ("all", name):
            continue
        images = make()
        data = compress(ctx, images, **kw)
        for target in (T.RGBA32, T.BC1_RGB):
            lines.append(json.dumps(run(ctx, name, data, uastc, target, args.windows, args.window)))
            print(lines[-1], flush=True)
        if args.stats and name == "etc1s_array_alpha_256":
            compress(ctx, images, stats=[], **kw)
            ms = []
            for _ in range(5):
                t0 = time.perf_counter()
                compress(ctx, images, stats=[], **kw)
                ms.append((time.perf_counter() - t0) * 1e3)
            plain = []
            for _ in range(5):
                t0 = time.perf_counter()
                compress(ctx, images, **kw)
                plain.append((time.perf_counter() - t0) * 1e3)
            lines.append(json.dumps({"workload": name, "compress_with_stats": summary(ms), "compress_without_stats": summary(plain), "slices": 128}))
            print(lines[-1], flush=True)
    ctx.close()
    if args.out:
        pathlib.Path(args.out).write_text("\n".join(lines) + "\n")
