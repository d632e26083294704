#!/usr/bin/env python3
"""Known answers of SSIM from the real reference tool (oracle/_ref/basisu, build machine only) -> tests/golden/ssim_vectors.npz.

`basisu -compare -compare_ssim a.png b.png` on the seeded pairs of tests/ssim_helpers.py, written with helpers.save_png: the seven lines the tool prints (R, G, B,
RGB Avg, A, Y 709, Y 601 SSIM), kept as the printed TEXT ("%f": six decimals, asserted) -- the tests compare text, not numbers.
  Seven kinds (near: +-7 noise; unrelated; inverted: b = 255 - a, negative SSIM and a descending running sum; identical: all seven print 1.000000; flat against flat;
  different in one channel only; an alpha ramp) at 1x1, 5x7, 11x11, 20x28, 64x40, 100x52 and 256x192, and 1xN / Nx1 strips with N one below, at and one above the
  chunk length of the device's reduction (kSsimChunk, read from csrc/ssim_kernels.h).
Members: a_<name> / b_<name> (h, w, 4) u8 for the pairs of up to 64x40 pixels; a larger pair is its seed, kind and size in `meta` with the crc32 of its pixels, and
the tests regenerate it (ssim_helpers.make_pair). `meta`: {"chunk", "figures", "pairs": [{"name", "kind", "w", "h", "seed", "crc", "printed": [7 texts]}]}.
usage: gen_golden_ssim.py"""
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
import ssim_helpers as H  # noqa: E402
import gen_golden_image_stats as S  # noqa: E402

BASISU = S.BASISU


def compare_ssim(a, b, what):
    """-> the seven printed texts"""
    with tempfile.TemporaryDirectory() as d:
        helpers.save_png(pathlib.Path(d) / "a.png", a)
        helpers.save_png(pathlib.Path(d) / "b.png", b)
        r = subprocess.run([str(BASISU), "-compare", "-compare_ssim", "a.png", "b.png"], cwd=d, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-2000:]
    out = []
    for label in H.LABELS:
        rows = [line for line in r.stdout.splitlines() if line.startswith(label + ": ")]
        assert len(rows) == 1, (what, label, r.stdout[-2000:])
        text_number = rows[0][len(label) + 2:].strip()
        assert re.fullmatch(r"-?\d+\.\d{6}", text_number), f"{text_number!r}: the tool no longer prints six decimals"
        out.append(text_number)
    return out


if __name__ == "__main__":
    assert BASISU.exists(), "oracle/_ref/basisu is missing: build it on the build machine (make -C oracle ref)"
    arrays, meta = {}, {"chunk": H.chunk_length(), "figures": H.FIGURES, "pairs": []}
    for name, kind, w, h, seed in H.pair_names():
        a, b = H.make_pair(kind, w, h, seed)
        texts = compare_ssim(a, b, name)
        if kind == "identical":
            assert texts == ["1.000000"] * 7, (name, texts)
        if w * h <= H.STORED_PIXELS:
            arrays["a_" + name], arrays["b_" + name] = a, b
        meta["pairs"].append({"name": name, "kind": kind, "w": w, "h": h, "seed": seed, "crc": H.crc(a, b), "printed": texts})
        print(name, " ".join(texts), flush=True)
    assert any(t.startswith("-") for p in meta["pairs"] if p["kind"] == "inverted" for t in p["printed"]), "no negative figure among the inverted pairs"
    arrays["meta"] = np.frombuffer(json.dumps(meta, sort_keys=True).encode(), np.uint8)
    S.save(H.GOLDEN, arrays)
    assert H.GOLDEN.stat().st_size <= 1 << 20, H.GOLDEN.stat().st_size
    print("wrote", H.GOLDEN, H.GOLDEN.stat().st_size, "bytes,", len(arrays), "members")
