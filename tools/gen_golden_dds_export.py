#!/usr/bin/env python3
"""Known answers of dds.export_dds from the real reference tool (oracle/_ref/basisu -dds, build machine only) -> tests/golden/dds_export_vectors.npz.

Per case of tests/dds_export_helpers.py -- a 20x28 image with a mip chain down to 1x1 in all five block formats and all seven raw formats, an image with an alpha
ramp, a photographic crop, 256 crafted tiles (solid, two-colour, constant-channel, ramps, min / max one apart, random), a 2-layer array and a cubemap with mips,
`-linear`, `-y_flip`, `-separate_rg_to_color_alpha`, `-normal_map` and `-resample` -- the source pixels and the .dds file the tool writes for them, nothing else.
Every group also has its a8b8g8r8 file: the prepared pixels themselves.
usage: gen_golden_dds_export.py"""
import json
import pathlib
import subprocess
import sys
import tempfile

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests"))
sys.path.insert(0, str(ROOT / "tools"))
sys.path.insert(0, str(ROOT))
import helpers  # noqa: E402
import dds_export_helpers as D  # noqa: E402
from gen_golden_etc1s_transcode import save  # noqa: E402

BASISU = ROOT / "oracle" / "_ref" / "basisu"


def tool(images, fmt, args, directory):
    """-> (exit status, output, the file's bytes or None)"""
    pngs = []
    for i, img in enumerate(images):
        helpers.save_png(pathlib.Path(directory) / f"in{i}.png", img)
        pngs.append(f"in{i}.png")
    r = subprocess.run([str(BASISU), "-no_multithreading", "-dds", "-dds_format", fmt, *args, *pngs, "-output_file", "out.dds"], cwd=directory, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True)
    out = pathlib.Path(directory) / "out.dds"
    return r.returncode, r.stdout, (out.read_bytes() if out.exists() else None)


if __name__ == "__main__":
    assert BASISU.exists(), "oracle/_ref/basisu is missing: build it on the build machine (make -C oracle ref)"
    arrays, meta = {}, {"cases": {}}
    for name, case in D.cases().items():
        for i, img in enumerate(case["images"]):
            arrays[f"image_{D.group_of(name)}_{i}"] = np.ascontiguousarray(img, np.uint8)   # once per group: its formats share the source
        with tempfile.TemporaryDirectory() as d:
            status, text, data = tool(case["images"], case["fmt"], case["tool"], d)
        assert status == 0 and data, text[-2000:]
        arrays[f"file_{name}"] = np.frombuffer(data, np.uint8).copy()
        meta["cases"][name] = {"fmt": case["fmt"], "tool": case["tool"], "images": len(case["images"]), "bytes": len(data)}
        print(name, len(case["images"]), "images,", len(data), "bytes", flush=True)
    arrays["meta"] = np.frombuffer(json.dumps(meta, sort_keys=True).encode(), np.uint8)
    save(D.GOLDEN, arrays)
    assert D.GOLDEN.stat().st_size <= 1 << 20, D.GOLDEN.stat().st_size
    print("wrote", D.GOLDEN, D.GOLDEN.stat().st_size, "bytes,", len(arrays), "members")
