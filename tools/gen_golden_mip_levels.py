#!/usr/bin/env python3
"""Known answers of compress(mip_levels=) and dds.compress_dds from the real reference tool (oracle/_ref/basisu, build machine only)
-> tests/golden/mip_levels_vectors.npz.

Per case of tests/mip_levels_helpers.py the .dds sources are written here -- DX10 and legacy headers, both byte orders, every level an independent synthetic image --
and given to `basisu -no_multithreading`, which uses a .dds file's mip chain as it is. The npz holds the sources (`dds_<case>_<i>`), the files the tool wrote
(`file_<case>_<basis|ktx2>`), its slice table (`slices_<case>`) and, for the cases marked so, the figures of `-stats` (`stats_<case>`, image_stats_vectors.npz's
layout). Asserted for every case: the tool's "Read DDS file" line per source (LDR, size, level count), the slice count, and the alpha flag of every slice --
so the semantics the tests rely on (a chain may stop early; -mipmap is ignored; alpha in a lower level alone gives the file alpha, even with -no_alpha; a UASTC slice
is marked by its own pixels) are the tool's, checked each time this runs.
usage: gen_golden_mip_levels.py"""
import json
import pathlib
import re
import subprocess
import sys
import tempfile

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests"))
sys.path.insert(0, str(ROOT / "tools"))
sys.path.insert(0, str(ROOT))
import mip_levels_helpers as L  # noqa: E402
import multi_image_helpers as M  # noqa: E402
from gen_golden_etc1s_transcode import save  # noqa: E402
from gen_golden_image_stats import parse_stats  # noqa: E402

BASISU = ROOT / "oracle" / "_ref" / "basisu"


def tool(sources, args, ext, directory):
    """-> (output, the file's bytes)"""
    names = []
    for i, data in enumerate(sources):
        (pathlib.Path(directory) / f"in{i}.dds").write_bytes(data.tobytes())
        names.append(f"in{i}.dds")
    r = subprocess.run([str(BASISU), "-no_multithreading", f"-{ext}", *args, *names, "-output_file", f"out.{ext}"], cwd=directory, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-2000:]
    return r.stdout, (pathlib.Path(directory) / f"out.{ext}").read_bytes()


def slice_rows(text):
    return np.array([[int(v) for v in m.groups()] for m in M.SLICE_LINE.finditer(text)], np.int64).reshape(-1, len(M.SLICE_FIELDS))


if __name__ == "__main__":
    assert BASISU.exists(), "oracle/_ref/basisu is missing: build it on the build machine (make -C oracle ref)"
    arrays, meta = {}, {"cases": {}}
    for name, case in L.cases().items():
        sources = [L.dds_file(f["levels"], f["order"], f["srgb"], f["legacy"]) for f in case["files"]]
        for i, data in enumerate(sources):
            arrays[f"dds_{name}_{i}"] = data
        rows = None
        for ext in case["exts"]:
            with tempfile.TemporaryDirectory() as d:
                text, data = tool(sources, case["tool"], ext, d)
                if case.get("stats") and ext == case["exts"][0]:
                    stats_text, stats_data = tool(sources, ["-stats", *case["tool"]], ext, d)
                    assert stats_data == data, f"{name}: -stats changed the file"
                    arrays[f"stats_{name}"] = parse_stats(stats_text)
            read = sorted((int(m.group(1)), int(m.group(2)), int(m.group(3)), int(m.group(4))) for m in re.finditer(L.READ_LINE, text))
            want = [(i, f["levels"][0].shape[1], f["levels"][0].shape[0], len(f["levels"])) for i, f in enumerate(case["files"])]
            assert read == want, (name, read, want)
            got = slice_rows(text)
            assert rows is None or (rows == got).all(), name      # both containers hold the same slices
            rows = got
            arrays[f"file_{name}_{ext}"] = np.frombuffer(data, np.uint8).copy()
        col = M.SLICE_FIELDS.index
        assert rows.shape[0] == case["slices"], (name, rows.shape[0], case["slices"])
        assert rows[:, col("alpha")].tolist() == case["alpha"], (name, rows[:, col("alpha")].tolist())
        n_levels = len(case["files"][0]["levels"])
        assert int(rows[:, col("level")].max()) + 1 == n_levels, name
        if f"stats_{name}" in arrays:
            assert arrays[f"stats_{name}"].shape[0] == case["slices"], name
        arrays[f"slices_{name}"] = rows
        meta["cases"][name] = {"tool": case["tool"], "files": len(sources), "levels": n_levels, "slices": case["slices"], "containers": list(case["exts"]),
                               "stats": bool(case.get("stats"))}
        print(name, len(sources), "files,", n_levels, "levels,", rows.shape[0], "slices, alpha", rows[:, col("alpha")].tolist(), flush=True)
    arrays["meta"] = np.frombuffer(json.dumps(meta, sort_keys=True).encode(), np.uint8)
    save(L.GOLDEN, arrays)
    assert L.GOLDEN.stat().st_size <= 1 << 20, L.GOLDEN.stat().st_size
    print("wrote", L.GOLDEN, L.GOLDEN.stat().st_size, "bytes,", len(arrays), "members")
