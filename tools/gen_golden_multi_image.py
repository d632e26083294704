#!/usr/bin/env python3
"""Known answers of compress() for several source images per file, from the real reference tool (oracle/_ref/basisu, build machine only)
-> tests/golden/multi_image_vectors.npz.

Per case of tests/multi_image_helpers.py -- texture arrays, cubemaps, video and a volume, ETC1S and UASTC, with mips, alpha on one image, ragged sizes, the RDO
post-pass and compression level 2 -- the source images, the .basis and the .ktx2 file the tool writes for them, and the slice table it prints (its `Slice:` lines).
It also records that the tool refuses an array of two sizes, a cubemap of five images and `-tex_type 2d` with two files for one output file (it compresses those
as separate files): their exit statuses.
usage: gen_golden_multi_image.py"""
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
import multi_image_helpers as M  # noqa: E402
from gen_golden_etc1s_transcode import save  # noqa: E402

BASISU = ROOT / "oracle" / "_ref" / "basisu"


def tool(images, args, ext, directory):
    """-> (exit status, output, the file's bytes or None)"""
    pngs = []
    for i, img in enumerate(images):
        helpers.save_png(pathlib.Path(directory) / f"in{i}.png", img)
        pngs.append(f"in{i}.png")
    r = subprocess.run([str(BASISU), "-no_multithreading", f"-{ext}", *args, *pngs, "-output_file", f"out.{ext}"], cwd=directory, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True)
    out = pathlib.Path(directory) / f"out.{ext}"
    return r.returncode, r.stdout, (out.read_bytes() if out.exists() else None)


def slice_rows(text):
    return np.array([[int(v) for v in m.groups()] for m in M.SLICE_LINE.finditer(text)], np.int64).reshape(-1, len(M.SLICE_FIELDS))


if __name__ == "__main__":
    assert BASISU.exists(), "oracle/_ref/basisu is missing: build it on the build machine (make -C oracle ref)"
    arrays, meta = {}, {"cases": {}, "refusals": {}}
    for name, case in M.cases().items():
        for i, img in enumerate(case["images"]):
            arrays[f"image_{name}_{i}"] = np.ascontiguousarray(img, np.uint8)
        rows = {}
        for ext in ("basis", "ktx2"):
            with tempfile.TemporaryDirectory() as d:
                status, text, data = tool(case["images"], case["tool"], ext, d)
            assert status == 0 and data, text[-2000:]
            arrays[f"file_{name}_{ext}"] = np.frombuffer(data, np.uint8).copy()
            rows[ext] = slice_rows(text)
        assert rows["basis"].shape[0] and (rows["basis"] == rows["ktx2"]).all(), name      # both containers hold the same slices
        arrays[f"slices_{name}"] = rows["basis"]
        meta["cases"][name] = {"tool": case["tool"], "images": len(case["images"]), "slices": int(rows["basis"].shape[0])}
        print(name, len(case["images"]), "images,", rows["basis"].shape[0], "slices,", arrays[f"file_{name}_basis"].size, "+", arrays[f"file_{name}_ktx2"].size, "bytes", flush=True)
    for name, (images, args) in M.refusals().items():
        with tempfile.TemporaryDirectory() as d:
            status, text, data = tool(images, args, "basis", d)
        assert status != 0, f"the tool accepted {name}:\n{text[-2000:]}"
        meta["refusals"][name] = {"tool": args, "images": [[int(v) for v in img.shape[:2]] for img in images], "exit_status": status}
        print("refused:", name, "exit status", status, flush=True)
    arrays["meta"] = np.frombuffer(json.dumps(meta, sort_keys=True).encode(), np.uint8)
    save(M.GOLDEN, arrays)
    assert M.GOLDEN.stat().st_size <= 1 << 20, M.GOLDEN.stat().st_size
    print("wrote", M.GOLDEN, M.GOLDEN.stat().st_size, "bytes,", len(arrays), "members")
