#!/usr/bin/env python3
"""Known answers of the per-slice quality stats from the real reference tool (oracle/_ref/basisu, build machine only) -> tests/golden/image_stats_vectors.npz.

Each case is a tiny tests/helpers.py synth image compressed by `basisu -no_multithreading -stats`: for every slice the tool prints one block of eight lines
(RGB Avg, RGBA Avg, R Avg, G Avg, B Avg, A Avg, 709 Luma, 601 Luma), each with Max, Mean, RMS and PSNR to three decimals -- image_metrics::calc of the slice's
source against what the file transcodes to (comp.cpp:4195-4253). The npz holds, per case, the source image (`src_<case>`), the file (`file_<case>`) and the printed
numbers (`stats_<case>`: float64 (slices, 8 lines, 4 figures)); `meta` names the cases, their options and the line / figure order.
    ETC1S q128 20x28 (ragged) as .basis and as .ktx2; 32x24 with the alpha ramp of gen_golden_etc1s_transcode.py (two slices, each with its own stats);
    20x28 -mipmap (five slices down to 1x1); UASTC level 2 -ktx2_no_zstandard 32x24 with alpha; UASTC 20x28 opaque.
Where tests/golden/etc1s_transcode_vectors.npz holds the same file, the bytes are checked against it.
usage: gen_golden_image_stats.py"""
import io
import json
import pathlib
import re
import subprocess
import sys
import tempfile
import zipfile

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests"))
import helpers  # noqa: E402

BASISU = ROOT / "oracle" / "_ref" / "basisu"
GOLDEN = ROOT / "tests" / "golden" / "image_stats_vectors.npz"
LINES = ["rgb", "rgba", "r", "g", "b", "a", "luma_709", "luma_601"]
LABELS = ["RGB Avg:", "RGBA Avg:", "R   Avg:", "G   Avg:", "B   Avg:", "A   Avg:", "709 Luma:", "601 Luma:"]   # basis_compressor's prefixes, comp.cpp:4215-4252
FIGURES = ["max", "mean", "rms", "psnr"]
NUMBERS = re.compile(r"\s+Max: ([0-9.]+) Mean: ([0-9.]+) RMS: ([0-9.]+) PSNR: ([0-9.]+) dB\s*$")


def alpha_ramp_image():
    img = helpers.synth(32, 24, 13)
    img[..., 3] = np.clip(np.mgrid[0:24, 0:32][1] * 8 + np.mgrid[0:24, 0:32][0] * 3, 0, 255).astype(np.uint8)
    return img


def cases():
    o20, alpha = helpers.synth(20, 28, 12), alpha_ramp_image()
    return [("etc1s_o20_basis", o20, "basis", ["-q", "128"], "o20_q128_basis"),
            ("etc1s_o20_ktx2", o20, "ktx2", ["-q", "128"], "o20_q128_ktx2"),
            ("etc1s_alpha_basis", alpha, "basis", ["-q", "128"], "alpha_basis"),
            ("etc1s_mip_basis", o20, "basis", ["-q", "128", "-mipmap"], "mip_basis"),
            ("uastc_alpha_ktx2", alpha, "ktx2", ["-uastc", "-uastc_level", "2", "-ktx2_no_zstandard"], None),
            ("uastc_o20_basis", o20, "basis", ["-uastc"], None)]


def parse_stats(text):
    """the tool's output -> (slices, 8, 4): after every `Slice: N` header of the stats stage, the eight lines in order (the `BC7 ...` lines that follow them are
    another decode's: tools/gen_golden_bc7_stats.py reads those); asserts one complete block per slice"""
    total = int(re.search(r"^Total slices: (\d+)$", text, re.M).group(1))
    out, lines = [], text.splitlines()
    for at, line in enumerate(lines):
        if not re.fullmatch(r"Slice: \d+", line):
            continue
        assert int(line.split()[1]) == len(out), "slice blocks out of order"
        assert lines[at + 1].startswith("Quality stats vs. transcoded "), lines[at + 1]
        block = []
        for k, label in enumerate(LABELS):
            row = lines[at + 2 + k]
            assert row.startswith(label), (label, row)
            m = NUMBERS.match(row[len(label):])
            assert m, row
            for text_number in m.groups():
                assert re.fullmatch(r"\d+\.\d{3}", text_number), f"{text_number!r}: the tool no longer prints three decimals"
            block.append([float(v) for v in m.groups()])
        out.append(block)
    assert len(out) == total, f"{len(out)} blocks of eight lines for {total} slices"
    return np.array(out, np.float64)


def run_case(img, ext, args):
    with tempfile.TemporaryDirectory() as d:
        helpers.save_png(pathlib.Path(d) / "in0.png", img)
        r = subprocess.run([str(BASISU), "-no_multithreading", f"-{ext}", "-stats", *args, "in0.png", "-output_file", f"out.{ext}"], cwd=d, stdout=subprocess.PIPE,
                           stderr=subprocess.STDOUT, text=True)
        assert r.returncode == 0, r.stdout[-2000:]
        return np.frombuffer((pathlib.Path(d) / f"out.{ext}").read_bytes(), np.uint8).copy(), parse_stats(r.stdout)


def save(path, arrays):
    """np.savez_compressed with fixed member timestamps, so that a rerun rewrites the file byte for byte"""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for k in sorted(arrays):
            buf = io.BytesIO()
            np.save(buf, arrays[k])
            z.writestr(zipfile.ZipInfo(k + ".npy", (1980, 1, 1, 0, 0, 0)), buf.getvalue(), zipfile.ZIP_DEFLATED, 9)


if __name__ == "__main__":
    assert BASISU.exists(), "oracle/_ref/basisu is missing: build it on the build machine (make -C oracle ref)"
    transcode_golden = np.load(ROOT / "tests" / "golden" / "etc1s_transcode_vectors.npz")
    arrays, meta = {}, {"lines": LINES, "figures": FIGURES, "cases": []}
    for name, img, ext, args, same_as in cases():
        data, stats = run_case(img, ext, args)
        if same_as is not None:
            assert (transcode_golden["file_" + same_as] == data).all(), f"{name}: not the file etc1s_transcode_vectors.npz holds as {same_as}"
        arrays["src_" + name], arrays["file_" + name], arrays["stats_" + name] = img, data, stats
        meta["cases"].append({"name": name, "container": ext, "uastc": "-uastc" in args, "args": args, "slices": int(stats.shape[0]), "same_file_as": same_as})
        print(name, data.size, "bytes,", stats.shape[0], "slices, rgb psnr", stats[:, 0, 3].tolist(), flush=True)
    arrays["meta"] = np.frombuffer(json.dumps(meta, sort_keys=True).encode(), np.uint8)
    save(GOLDEN, arrays)
    assert GOLDEN.stat().st_size <= 1 << 20, GOLDEN.stat().st_size
    print("wrote", GOLDEN, GOLDEN.stat().st_size, "bytes,", len(arrays), "members")
