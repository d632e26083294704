#!/usr/bin/env python3
"""Time of the .dds export (basis_universal_amd/dds.py) on textures of a size users export: a 4096x4096 synthetic RGBA image with its full mip chain, and a cubemap
of six 1024x1024 faces with mips, each as bc1, bc3, bc5 and a8r8g8b8.

Two figures per workload and format, both on rasters that are already resident in HBM (the upload of the source is not in either):
  kernel : the pack kernel alone (k_dds_pack_blocks / k_dds_pack_pixels), HIP events around its one launch (bu_hip_profile_*) -- device only.
  call   : dds._export_resident from the resident level-0 rasters to the file's bytes on the host -- mip chain, tiling, the pack launch AND the download of the
           payload -- on the host clock; the call ends in the blocking device-to-host copy.
`warmup` calls, then `steps` timed calls per round, `rounds` rounds that alternate over the formats so that a drift of the machine shows as a spread; the kernel
passes run with the profiler on and the call passes with it off. Reported: the median of all timed calls and their min .. max.
For comparison the reference tool (oracle/_ref/basisu -dds, the binary the oracle Makefile builds) on the same images as PNG files, `tool_runs` runs each with
-no_multithreading and with its default thread pool: wall time of the whole process, which includes reading the PNGs and writing the .dds. No threshold is asserted.
Prints one line per figure, then one JSON line.   tools/dds_export_bench.py [steps] [warmup] [rounds] [tool_runs]"""
import json
import pathlib
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
import helpers  # noqa: E402
from basis_universal_amd import capi, dds, mipmap  # noqa: E402

FORMATS = ("bc1", "bc3", "bc5", "a8r8g8b8")
BASISU = ROOT / "oracle" / "_ref" / "basisu"


def workloads():
    return {"synth4096_mips": dict(images=[helpers.synth(4096, 4096, 1234)], tex_type="2d", tool=["-mipmap"]),
            "cube1024_mips": dict(images=[helpers.synth(1024, 1024, 600 + i) for i in range(6)], tex_type="cubemap", tool=["-tex_type", "cubemap", "-mipmap"])}


def summary(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4), "samples": len(ms)}


def export(ctx, level0, level_sizes, tex_type, fmt):
    owned = []
    try:
        cubemap = tex_type == "cubemap"
        head = dds.dds_header(*level_sizes[0][0], len(level_sizes[0]), len(level0) // (6 if cubemap else 1), cubemap, fmt, True)
        return dds._export_resident(ctx, owned, level0, level_sizes, [False] * len(level0), False, fmt, head, tex_type=tex_type, mip_srgb=True, mip_filter="kaiser",
                                    mip_scale=1.0, mip_wrapping=True, mip_fast=True, mip_renormalize=False)
    finally:
        for d in owned:
            ctx.free(d)


def write_pngs(images, directory):
    names = []
    for i, img in enumerate(images):
        helpers.save_png(pathlib.Path(directory) / f"in{i}.png", img)
        names.append(f"in{i}.png")
    return names


def time_tool(directory, pngs, args, fmt, threads, runs):
    """-> (the wall time of each run in ms, the file of the last)"""
    out = []
    for _ in range(runs):
        t0 = time.perf_counter()
        r = subprocess.run([str(BASISU), *([] if threads else ["-no_multithreading"]), "-dds", "-dds_format", fmt, *args, *pngs, "-output_file", "out.dds"], cwd=directory,
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=900)
        out.append((time.perf_counter() - t0) * 1e3)
        assert r.returncode == 0, r.stdout[-2000:]
    return out, (pathlib.Path(directory) / "out.dds").read_bytes()


def main():
    steps, warmup, rounds, tool_runs = (int(sys.argv[i]) if len(sys.argv) > i else v for i, v in ((1, 10), (2, 2), (3, 3), (4, 2)))
    ctx = capi.Context(0)
    report = {}
    for name, load in workloads().items():
        images = load["images"]
        h, w = images[0].shape[:2]
        level_sizes = [[(w, h)] + mipmap.level_sizes(w, h, 1) for _ in images]
        level0 = [ctx.upload(img) for img in images]
        kernel, call, files = {f: [] for f in FORMATS}, {f: [] for f in FORMATS}, {}
        for _ in range(rounds):
            for fmt in FORMATS:
                region = "dds_pack_blocks" if dds.FORMATS[fmt][1] else "dds_pack_pixels"
                for _ in range(warmup):
                    files[fmt] = export(ctx, level0, level_sizes, load["tex_type"], fmt)
                for _ in range(steps):      # the pack launch alone, one event pair per call
                    ctx.profile_enable(True)
                    export(ctx, level0, level_sizes, load["tex_type"], fmt)
                    ms, launches = ctx.profile_read()[region]
                    ctx.profile_enable(False)
                    assert launches == 1
                    kernel[fmt].append(ms)
                for _ in range(steps):      # the whole call, profiler off; it ends in the blocking download
                    t0 = time.perf_counter()
                    export(ctx, level0, level_sizes, load["tex_type"], fmt)
                    call[fmt].append((time.perf_counter() - t0) * 1e3)
        for d in level0:
            ctx.free(d)
        n_tiles = sum(((lw + 3) // 4) * ((lh + 3) // 4) for lw, lh in level_sizes[0]) * len(images)
        report[name] = {"tiles": n_tiles, "formats": {}}
        with_tool = BASISU.exists() and tool_runs > 0
        scratch = tempfile.TemporaryDirectory()
        pngs = write_pngs(images, scratch.name) if with_tool else []
        for fmt in FORMATS:
            row = {"file_bytes": int(files[fmt].size), "pack_kernel_device_only": summary(kernel[fmt]), "call_resident_raster_to_host_bytes": summary(call[fmt])}
            row["pack_kernel_mtiles_per_s"] = round(n_tiles / (row["pack_kernel_device_only"]["median_ms"] * 1e-3) / 1e6, 1)
            if with_tool:
                for threads, key in ((False, "tool_single_thread_process_wall"), (True, "tool_default_threads_process_wall")):
                    ms, data = time_tool(scratch.name, pngs, load["tool"], fmt, threads, tool_runs)
                    row[key] = summary(ms)
                    row["equals_tool_file"] = bool(data == files[fmt].tobytes())
            report[name]["formats"][fmt] = row
            k, c = row["pack_kernel_device_only"], row["call_resident_raster_to_host_bytes"]
            line = (f"{name:15s} {fmt:9s} kernel {k['median_ms']:8.4f} ms ({k['min_ms']:.4f} .. {k['max_ms']:.4f})  call {c['median_ms']:8.3f} ms "
                    f"({c['min_ms']:.3f} .. {c['max_ms']:.3f})")
            if "tool_single_thread_process_wall" in row:
                s, m = row["tool_single_thread_process_wall"], row["tool_default_threads_process_wall"]
                line += f"  tool 1 thread {s['median_ms']:9.1f} ms, default {m['median_ms']:9.1f} ms  same bytes: {row['equals_tool_file']}"
            print(line, flush=True)
        scratch.cleanup()
    ctx.close()
    print(json.dumps({"steps": steps, "warmup": warmup, "rounds": rounds, "tool_runs": tool_runs, "workloads": report}))


if __name__ == "__main__":
    main()
