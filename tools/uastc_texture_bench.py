#!/usr/bin/env python3
"""Time of the UASTC texture family's further targets on the 4096x4096 synthetic image: level-2 blocks resident in HBM, the output resident too. Per target, after
`warmup` calls, `steps` calls of transcode_uastc_texture_blocks(out_device=...), each measured twice:
  launch  the library's HIP events around the launch (bu_hip_profile_*: the 4-byte counter memset plus the one kernel), and
  call    the whole call on the host's clock -- launch, stream wait, read-back of the counter,
both given as the median over the steps. In the same run, as the yardstick and the regression check, the first family's nine cases through ITS entry
(transcode_uastc_blocks), to be held against profiles/uastc_transcode.md. Algorithmic bytes are 16 in plus the target's bytes out per block; the fraction is of the
8 TB/s HBM figure the project's roofline uses. Prints one line per figure and one JSON line.   tools/uastc_texture_bench.py [steps] [warmup]"""
import json
import pathlib
import sys
import time

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
import helpers  # noqa: E402
from basis_universal_amd import capi, transcode, uastc  # noqa: E402

HBM_BYTES_PER_S = 8e12
T = transcode
# name -> (target, high quality, bytes out per block)
TEXTURE = [("etc1", T.ETC1_RGB, False, 8), ("etc2_rgba", T.ETC2_RGBA, False, 16), ("eac_r11", T.ETC2_EAC_R11, False, 8), ("eac_r11_hq", T.ETC2_EAC_R11, True, 8),
           ("eac_rg11", T.ETC2_EAC_RG11, False, 16), ("eac_rg11_hq", T.ETC2_EAC_RG11, True, 16), ("rgb565", T.RGB565, False, 32), ("bgr565", T.BGR565, False, 32),
           ("rgba4444", T.RGBA4444, False, 32)]
FIRST = [("rgba32", T.RGBA32, False, 64), ("astc", T.ASTC_4x4_RGBA, False, 16), ("bc7", T.BC7_RGBA, False, 16), ("bc1", T.BC1_RGB, False, 8), ("bc1_hq", T.BC1_RGB, True, 8),
         ("bc3", T.BC3_RGBA, False, 16), ("bc3_hq", T.BC3_RGBA, True, 16), ("bc4_r", T.BC4_R, False, 8), ("bc5_ra", T.BC5_RG, False, 16)]


def main():
    steps = int(sys.argv[1]) if len(sys.argv) > 1 else 30
    warmup = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    ctx = capi.Context(0)
    nbx = nby = 1024
    n = nbx * nby
    d_blocks, d_out = ctx.alloc(n * 16), ctx.alloc(n * 64)
    uastc.encode_uastc_blocks(ctx, helpers.to_pixel_blocks(helpers.synth(4096, 4096, 1234)), uastc.LEVEL_DEFAULT, out_device=d_blocks)
    out = {"texture_family": {}, "first_family": {}}
    for family, cases, scope in (("texture_family", TEXTURE, "uastc_transcode_texture"), ("first_family", FIRST, "uastc_transcode")):
        for name, target, hq, out_bytes in cases:
            def call():
                if family == "texture_family":
                    T.transcode_uastc_texture_blocks(ctx, d_blocks, nbx, nby, target, high_quality=hq, out_device=d_out)
                else:
                    T.transcode_uastc_blocks(ctx, d_blocks, nbx, nby, target, high_quality=hq, out_device=d_out)
            for _ in range(warmup):
                call()
            launch_ms, call_ms = [], []
            for _ in range(steps):
                ctx.profile_enable(True)
                t0 = time.perf_counter()
                call()
                call_ms.append((time.perf_counter() - t0) * 1e3)
                ms, launches = ctx.profile_read()[scope]
                ctx.profile_enable(False)
                assert launches == 1
                launch_ms.append(ms)
            ms, whole = float(np.median(launch_ms)), float(np.median(call_ms))
            traffic = n * (16 + out_bytes)
            out[family][name] = {"launch_ms": round(ms, 4), "launch_ms_min_max": [round(min(launch_ms), 4), round(max(launch_ms), 4)], "call_ms": round(whole, 4),
                                 "gblocks_per_s": round(n / ms / 1e6, 2), "algorithmic_mb": round(traffic / 1e6, 1), "fraction_of_8tbps": round(traffic / (ms * 1e-3) / HBM_BYTES_PER_S, 4)}
            print(f"{family:14s} {name:12s} launch {ms:8.4f} ms ({min(launch_ms):.4f}..{max(launch_ms):.4f})  call {whole:8.4f} ms  {n / ms / 1e6:7.2f} Gblocks/s  "
                  f"{traffic / 1e6:6.1f} MB  {100 * traffic / (ms * 1e-3) / HBM_BYTES_PER_S:6.2f} % of 8 TB/s", flush=True)
    ctx.free(d_blocks)
    ctx.free(d_out)
    ctx.close()
    print(json.dumps(dict(out, image="synth4096 seed 1234, UASTC level 2, 1,048,576 blocks", steps=steps, warmup=warmup)))


if __name__ == "__main__":
    main()
