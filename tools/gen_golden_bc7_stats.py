#!/usr/bin/env python3
"""Known answers of the "(BC7)" half of the per-slice quality stats from the real reference tool (oracle/_ref/basisu, build machine only)
-> tests/golden/bc7_stats_vectors.npz.

For every UASTC slice `basisu -stats` prints, after the slice's own stats, "Quality stats vs. transcoded BC7 texture:" -- eight `BC7 ... Avg / Luma` lines, Max, Mean,
RMS and PSNR to three decimals -- and "PSNR-HVS and PSNR-HVS-M metrics (BC7):" with the eight PSNR-HVS lines: the slice's source against its BC7 transcode unpacked by
gpu_image::unpack (comp.cpp:3818-3842, 3875-3883, 4278-4337). Three cases: the two UASTC cases of gen_golden_image_stats.py (uastc_alpha_ktx2, uastc_o20_basis; their
files are checked against image_stats_vectors.npz, which holds the sources too) and uastc_mip_basis, the 20x28 image with -uastc -mipmap, five slices down to 1x1,
whose file and level-0 source are stored here (the tests make the other levels' sources with this package's mip generator, as the ETC1S mip stats test does).
Members per case: `stats_<case>` f64 (slices, 8 lines, 4 figures) in image_stats_vectors.npz's layout, `hvs_<case>` f64 (slices, 8 entries, 2 figures) in
psnr_hvs_vectors.npz's; `file_uastc_mip_basis`, `src_uastc_mip_basis`; `meta` names cases, lines, entries and figures.
usage: gen_golden_bc7_stats.py"""
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
import helpers  # noqa: E402
import gen_golden_image_stats as S  # noqa: E402
import gen_golden_psnr_hvs as H  # noqa: E402

GOLDEN = ROOT / "tests" / "golden" / "bc7_stats_vectors.npz"
LABELS = ["BC7 RGB Avg:", "BC7 RGBA Avg:", "BC7 R   Avg:", "BC7 G   Avg:", "BC7 B   Avg:", "BC7 A   Avg:", "BC7 709 Luma:", "BC7 601 Luma:"]   # comp.cpp:4285-4322
MIP_CASE = ("uastc_mip_basis", "basis", ["-uastc", "-mipmap"])


def parse_bc7(text):
    """the tool's output -> ((slices, 8, 4), (slices, 8, 2)): the BC7 block and the "(BC7)" HVS block after every `Slice: N` header of the stats stage"""
    total = int(re.search(r"^Total slices: (\d+)$", text, re.M).group(1))
    lines = text.splitlines()
    headers = [k for k, line in enumerate(lines) if re.fullmatch(r"Slice: \d+", line)]
    stats, hvs = [], []
    for n, at in enumerate(headers):
        assert int(lines[at].split()[1]) == n, "slice blocks out of order"
        end = headers[n + 1] if n + 1 < len(headers) else len(lines)
        (first,) = [k for k in range(at, end) if lines[k] == "Quality stats vs. transcoded BC7 texture:"]
        block = []
        for k, label in enumerate(LABELS):
            row = lines[first + 1 + k]
            assert row.startswith(label), (label, row)
            m = S.NUMBERS.match(row[len(label):])
            assert m, row
            for text_number in m.groups():
                assert re.fullmatch(r"\d+\.\d{3}", text_number), f"{text_number!r}: the tool no longer prints three decimals"
            block.append([float(v) for v in m.groups()])
        stats.append(block)
        (h,) = [k for k in range(first, end) if lines[k] == "PSNR-HVS and PSNR-HVS-M metrics (BC7):"]
        hvs.append(H.parse_block(lines, h + 1, f"slice {n} (BC7)"))
    assert len(stats) == total, f"{len(stats)} BC7 blocks for {total} slices"
    return np.array(stats, np.float64), np.array(hvs, np.float64)


def run_case(img, ext, args):
    with tempfile.TemporaryDirectory() as d:
        helpers.save_png(pathlib.Path(d) / "in0.png", img)
        r = subprocess.run([str(S.BASISU), "-no_multithreading", f"-{ext}", "-stats", *args, "in0.png", "-output_file", f"out.{ext}"], cwd=d, stdout=subprocess.PIPE,
                           stderr=subprocess.STDOUT, text=True)
        assert r.returncode == 0, r.stdout[-2000:]
        return np.frombuffer((pathlib.Path(d) / f"out.{ext}").read_bytes(), np.uint8).copy(), parse_bc7(r.stdout)


if __name__ == "__main__":
    assert S.BASISU.exists(), "oracle/_ref/basisu is missing: build it on the build machine (make -C oracle ref)"
    stats_golden = np.load(S.GOLDEN)
    arrays, meta = {}, {"lines": S.LINES, "figures": S.FIGURES, "hvs_entries": H.ENTRIES, "hvs_figures": ["psnr_hvs", "psnr_hvsm"], "cases": []}
    todo = [(name, img, ext, args, True) for name, img, ext, args, _ in S.cases() if name in ("uastc_alpha_ktx2", "uastc_o20_basis")]
    assert len(todo) == 2
    todo.append((MIP_CASE[0], helpers.synth(20, 28, 12), MIP_CASE[1], MIP_CASE[2], False))
    for name, img, ext, args, shared in todo:
        data, (stats, hvs) = run_case(img, ext, args)
        if shared:
            assert (stats_golden["file_" + name] == data).all() and (stats_golden["src_" + name] == img).all(), f"{name}: not the file image_stats_vectors.npz holds"
        else:
            arrays["file_" + name], arrays["src_" + name] = data, img
        arrays["stats_" + name], arrays["hvs_" + name] = stats, hvs
        meta["cases"].append({"name": name, "container": ext, "args": args, "slices": int(stats.shape[0]), "in_image_stats_vectors": shared})
        print(name, data.size, "bytes,", stats.shape[0], "slices, BC7 rgb psnr", stats[:, 0, 3].tolist(), "BC7 RGB PSNR-HVS-M", hvs[:, 2, 1].tolist(), flush=True)
    arrays["meta"] = np.frombuffer(json.dumps(meta, sort_keys=True).encode(), np.uint8)
    S.save(GOLDEN, arrays)
    assert GOLDEN.stat().st_size <= 1 << 20, GOLDEN.stat().st_size
    print("wrote", GOLDEN, GOLDEN.stat().st_size, "bytes,", len(arrays), "members")
