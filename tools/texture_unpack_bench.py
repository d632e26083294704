#!/usr/bin/env python3
"""Time of the texture unpack kernels on 1,048,576 resident blocks per format (a 4096x4096 texture): the synthetic image's level-2 UASTC blocks resident in HBM,
transcoded on the device to every block format, then per format `warmup` + `steps` unpack calls. Two figures per format: the LAUNCH alone, from the library's HIP
events around it (bu_hip_profile_*), and the WHOLE CALL, a host clock around transcode.unpack_texture with the raster staying on the device (the call ends in the
stream wait that reads the count of invalid blocks back). BC1 and BC7 also go through the old entry (transcode.unpack_blocks) in the same run, as the yardstick.
ASTC has three inputs, because its cost depends on what the blocks hold: `astc`, what the UASTC transcoder writes (one to three partitions, one or two planes, 4x4
grids); `astc_void`, void-extent blocks only (the header and the store: the floor); `astc_mixed`, the accepted blocks of tests/golden/texture_unpack_vectors.npz
repeated (every grid size, range, partition count and endpoint mode side by side in one wave: the divergent end).
All are timed in `rounds` alternating passes, so that a drift of the machine shows as a spread and not as a difference. Every format writes 64 B per block; the
algorithmic bytes are block bytes in + 64 out. Prints one line per row and writes medians and ranges into profiles/texture_unpack_bench.json.
    tools/texture_unpack_bench.py [steps] [warmup] [rounds] [output json]"""
import json
import pathlib
import statistics
import sys
import time

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
import helpers  # noqa: E402
import numpy as np  # noqa: E402
import texture_unpack_helpers as X  # noqa: E402
from basis_universal_amd import capi, transcode as T, uastc  # noqa: E402

HBM_BYTES_PER_S = 8e12


def main():
    steps = int(sys.argv[1]) if len(sys.argv) > 1 else 50
    warmup = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 5
    out_path = pathlib.Path(sys.argv[4]) if len(sys.argv) > 4 else ROOT / "profiles" / "texture_unpack_bench.json"
    ctx = capi.Context(0)
    nbx = nby = 1024
    n = nbx * nby
    d_uastc, d_out = ctx.alloc(n * 16), ctx.alloc(n * 64)
    uastc.encode_uastc_blocks(ctx, helpers.to_pixel_blocks(helpers.synth(4096, 4096, 1234)), uastc.LEVEL_DEFAULT, out_device=d_uastc)
    resident = {}
    for name, fmt in (("bc1", T.BC1_RGB), ("bc7", T.BC7_RGBA), ("etc1", T.ETC1_RGB), ("etc2", T.ETC2_RGBA), ("r11", T.ETC2_EAC_R11), ("rg11", T.ETC2_EAC_RG11),
                      ("astc", T.ASTC_4x4_RGBA)):
        resident[name] = (fmt, ctx.alloc(n * T.UNPACK_TEXTURE_BYTES_PER_BLOCK[fmt]))
        T.transcode_uastc_texture_blocks(ctx, d_uastc, nbx, nby, fmt, out_device=resident[name][1])
    resident["pvrtc1"] = (T.PVRTC1_4_RGBA, ctx.alloc(n * 8))
    T.transcode_uastc_pvrtc1_blocks(ctx, d_uastc, nbx, nby, T.PVRTC1_4_RGBA, out_device=resident["pvrtc1"][1])
    arrays, _ = X.golden()
    kinds = np.array([X.astc_fields(b)["kind"] for b in arrays["astc_blocks"]])
    for name, blocks in (("astc_void", arrays["astc_blocks"][kinds == "void"]), ("astc_mixed", arrays["astc_blocks"][kinds == "normal"])):
        resident[name] = (T.ASTC_4x4_RGBA, ctx.upload(np.ascontiguousarray(np.concatenate([blocks] * -(-n // blocks.shape[0]))[:n])))
    rows = [(f"old_{name}", "unpack_blocks", resident[name][0], lambda f=resident[name][0], d=resident[name][1]: T.unpack_blocks(ctx, d, nbx, nby, f, out_device=d_out))
            for name in ("bc1", "bc7")]
    rows += [(name, "unpack_texture", fmt, lambda f=fmt, d=d: T.unpack_texture(ctx, d, nbx, nby, f, out_device=d_out)) for name, (fmt, d) in resident.items()]
    launch, call = {name: [] for name, _, _, _ in rows}, {name: [] for name, _, _, _ in rows}
    for _ in range(rounds):
        for name, region, _, run in rows:
            for _ in range(warmup):
                run()
            ctx.profile_enable(True)
            t0 = time.perf_counter()
            for _ in range(steps):
                run()
            wall = time.perf_counter() - t0
            ms, launches = ctx.profile_read()[region]
            ctx.profile_enable(False)
            assert launches == steps
            launch[name].append(ms / steps)
            call[name].append(wall * 1e3 / steps)
    result = {}
    for name, _, fmt, _ in rows:
        ms, traffic = statistics.median(launch[name]), n * (T.UNPACK_TEXTURE_BYTES_PER_BLOCK[fmt] + 64)
        result[name] = {"launch_ms_median": round(ms, 4), "launch_ms_min": round(min(launch[name]), 4), "launch_ms_max": round(max(launch[name]), 4),
                        "call_ms_median": round(statistics.median(call[name]), 4), "call_ms_min": round(min(call[name]), 4), "call_ms_max": round(max(call[name]), 4),
                        "algorithmic_mb": round(traffic / 1e6, 1), "tb_per_s": round(traffic / (ms * 1e-3) / 1e12, 3),
                        "fraction_of_8tbps": round(traffic / (ms * 1e-3) / HBM_BYTES_PER_S, 4)}
        print(f"{name:10s} launch {ms:8.4f} ms ({min(launch[name]):.4f} .. {max(launch[name]):.4f})  call {statistics.median(call[name]):8.4f} ms "
              f"({min(call[name]):.4f} .. {max(call[name]):.4f})  {traffic / 1e6:6.1f} MB  {traffic / (ms * 1e-3) / 1e12:6.3f} TB/s  "
              f"{100 * traffic / (ms * 1e-3) / HBM_BYTES_PER_S:6.2f} % of 8 TB/s", flush=True)
    for d in [d_uastc, d_out] + [d for _, d in resident.values()]:
        ctx.free(d)
    ctx.close()
    doc = {"image": "synth4096 seed 1234, UASTC level 2 -> every block format on the device, 1048576 blocks each", "device": "AMD Instinct MI355X (gfx950)",
           "what": "launch: HIP events around the kernel launch; call: host clock around transcode.unpack_texture / unpack_blocks with out_device, ending in the "
                   "stream wait that reads the invalid count; medians and ranges over the rounds, each round `steps` calls after `warmup`",
           "steps": steps, "warmup": warmup, "rounds": rounds, "rows": result}
    out_path.parent.mkdir(parents=True, exist_ok=True)
    out_path.write_text(json.dumps(doc, indent=1, sort_keys=True) + "\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
