#!/usr/bin/env python3
"""Known answers of PSNR-HVS / PSNR-HVS-M from the real reference tool (oracle/_ref/basisu, build machine only) -> tests/golden/psnr_hvs_vectors.npz.

(a) `basisu -compare_hvs a.png b.png` on pairs written with helpers.save_png: the eight lines psnr_hvs_print_metrics prints (Float Y 601, 8-Bit Y 601, RGB Avg.,
    RGBA Avg., R, G, B, A), each with PSNR-HVS and PSNR-HVS-M to three decimals.
      44 single 8x8-block pairs, where the printed figure is a per-block check: near-noise, unrelated, flat against noise (the pop == 0 branch of the masking
      strength), flat against a different flat, identical (both figures print 100000.000), different in one channel only, varying alpha.
      Ragged and multi-block pairs: 1x1, 5x7, 9x9, 20x28, 64x40, 100x52.
    Members: blocks_a / blocks_b (44, 8, 8, 4) u8, blocks_hvs (44, 8, 2) f64; size_<w>x<h>_a / _b, size_<w>x<h>_hvs (8, 2).
(b) The six cases of gen_golden_image_stats.py, same sources and options, through `basisu -stats`: the first "PSNR-HVS and PSNR-HVS-M metrics:" block of every slice
    (the one against the slice's own decode, not the "(BC7)" one). The files are checked against those image_stats_vectors.npz holds, which the tests use.
    Members: stats_hvs_<case> (slices, 8, 2) f64.
`meta` names the kinds, sizes, cases and the entry / figure order.
usage: gen_golden_psnr_hvs.py"""
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

BASISU = S.BASISU
GOLDEN = ROOT / "tests" / "golden" / "psnr_hvs_vectors.npz"
ENTRIES = ["y_601_float", "y_601_8bit", "rgb", "rgba", "r", "g", "b", "a"]
LABELS = ["  Float Y 601", "  8-Bit Y 601", "    RGB  Avg.", "    RGBA Avg.", "            R", "            G", "            B", "            A"]
NUMBERS = re.compile(r" PSNR-HVS: ([0-9.]+) dB, PSNR-HVS-M: ([0-9.]+) dB\s*$")
SIZES = [(1, 1), (5, 7), (9, 9), (20, 28), (64, 40), (100, 52)]
KINDS = [("near", 8), ("unrelated", 6), ("flat_noise", 6), ("flat_flat", 6), ("identical", 4), ("one_channel", 8), ("alpha", 6)]


def parse_block(lines, at, what):
    """lines[at : at + 8] = the eight lines of psnr_hvs_print_metrics -> (8, 2)"""
    out = []
    for k, label in enumerate(LABELS):
        row = lines[at + k]
        assert row.startswith(label + " PSNR-HVS:"), (what, label, row)
        m = NUMBERS.match(row[len(label):])
        assert m, (what, row)
        for text_number in m.groups():
            assert re.fullmatch(r"\d+\.\d{3}", text_number), f"{text_number!r}: the tool no longer prints three decimals"
        out.append([float(v) for v in m.groups()])
    return out


def compare_hvs(a, b, what):
    with tempfile.TemporaryDirectory() as d:
        helpers.save_png(pathlib.Path(d) / "a.png", a)
        helpers.save_png(pathlib.Path(d) / "b.png", b)
        r = subprocess.run([str(BASISU), "-compare_hvs", "a.png", "b.png"], cwd=d, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-2000:]
    lines = r.stdout.splitlines()
    at = [k for k, line in enumerate(lines) if line.startswith(LABELS[0])]
    assert len(at) == 1, (what, r.stdout[-2000:])
    return np.array(parse_block(lines, at[0], what), np.float64)


def single_block_pairs():
    rng = np.random.default_rng(20260)
    a_all, b_all, kinds = [], [], []
    for kind, count in KINDS:
        for k in range(count):
            a = rng.integers(0, 256, (8, 8, 4), dtype=np.uint8)
            noise = np.clip(a.astype(np.int64) + rng.integers(-5, 6, a.shape), 0, 255).astype(np.uint8)
            if kind == "near":
                b = noise
            elif kind == "unrelated":
                b = rng.integers(0, 256, (8, 8, 4), dtype=np.uint8)
            elif kind == "flat_noise":
                flat = np.broadcast_to(rng.integers(0, 256, 4, dtype=np.uint8), (8, 8, 4)).copy()
                a, b = (flat, a) if k % 2 else (a, flat)
            elif kind == "flat_flat":
                a = np.broadcast_to(rng.integers(0, 256, 4, dtype=np.uint8), (8, 8, 4)).copy()
                b = np.clip(a.astype(np.int64) + rng.integers(1, 40, 4) * rng.choice([-1, 1], 4), 0, 255).astype(np.uint8)
            elif kind == "identical":
                if k % 2:
                    a = np.broadcast_to(rng.integers(0, 256, 4, dtype=np.uint8), (8, 8, 4)).copy()
                b = a.copy()
            elif kind == "one_channel":
                b = a.copy()
                b[..., k % 4] = noise[..., k % 4]
            else:   # alpha: opaque-ish colour under an alpha ramp or alpha noise, and a decode of it that is off in every channel
                yy, xx = np.mgrid[0:8, 0:8]
                a[..., 3] = np.clip(xx * (9 + 7 * k) + yy * (3 + k), 0, 255).astype(np.uint8) if k % 2 else rng.integers(0, 256, (8, 8), dtype=np.uint8)
                b = np.clip(a.astype(np.int64) + rng.integers(-9, 10, a.shape), 0, 255).astype(np.uint8)
            a_all.append(a); b_all.append(b); kinds.append(kind)
    return np.stack(a_all), np.stack(b_all), kinds


def sized_pair(w, h):
    a = helpers.synth((w + 3) // 4 * 4, (h + 3) // 4 * 4, 300 + w)[:h, :w].copy()   # synth takes multiples of 4
    rng = np.random.default_rng(400 + w)
    a[..., 3] = rng.integers(0, 256, (h, w), dtype=np.uint8)
    b = np.clip(a.astype(np.int64) + rng.integers(-7, 8, a.shape), 0, 255).astype(np.uint8)
    return a, b


def parse_stats_hvs(text):
    """`basisu -stats` output -> (slices, 8, 2): the first HVS block after every `Slice: N` header"""
    total = int(re.search(r"^Total slices: (\d+)$", text, re.M).group(1))
    out, lines = [], text.splitlines()
    headers = [k for k, line in enumerate(lines) if re.fullmatch(r"Slice: \d+", line)]
    for n, at in enumerate(headers):
        assert int(lines[at].split()[1]) == n, "slice blocks out of order"
        end = headers[n + 1] if n + 1 < len(headers) else len(lines)
        first = next(k for k in range(at, end) if lines[k].startswith("PSNR-HVS and PSNR-HVS-M metrics"))
        assert not any("BC7" in lines[k] for k in range(at, first)), "the first HVS block comes after the BC7 stats"
        out.append(parse_block(lines, first + 1, f"slice {n}"))
    assert len(out) == total, f"{len(out)} HVS blocks for {total} slices"
    return np.array(out, np.float64)


def run_stats_case(img, ext, args):
    with tempfile.TemporaryDirectory() as d:
        helpers.save_png(pathlib.Path(d) / "in0.png", img)
        r = subprocess.run([str(BASISU), "-no_multithreading", f"-{ext}", "-stats", *args, "in0.png", "-output_file", f"out.{ext}"], cwd=d, stdout=subprocess.PIPE,
                           stderr=subprocess.STDOUT, text=True)
        assert r.returncode == 0, r.stdout[-2000:]
        return np.frombuffer((pathlib.Path(d) / f"out.{ext}").read_bytes(), np.uint8).copy(), parse_stats_hvs(r.stdout)


if __name__ == "__main__":
    assert BASISU.exists(), "oracle/_ref/basisu is missing: build it on the build machine (make -C oracle ref)"
    arrays, meta = {}, {"entries": ENTRIES, "figures": ["psnr_hvs", "psnr_hvsm"], "sizes": [list(s) for s in SIZES], "cases": []}
    a, b, kinds = single_block_pairs()
    assert len(kinds) >= 40
    arrays["blocks_a"], arrays["blocks_b"], meta["block_kinds"] = a, b, kinds
    arrays["blocks_hvs"] = np.stack([compare_hvs(a[k], b[k], f"block {k} ({kinds[k]})") for k in range(len(kinds))])
    for k, kind in enumerate(kinds):
        if kind == "identical":
            assert (arrays["blocks_hvs"][k] == 100000.0).all(), k
    print(len(kinds), "single-block pairs; R PSNR-HVS-M", arrays["blocks_hvs"][:, 4, 1].tolist(), flush=True)
    for w, h in SIZES:
        a, b = sized_pair(w, h)
        arrays[f"size_{w}x{h}_a"], arrays[f"size_{w}x{h}_b"], arrays[f"size_{w}x{h}_hvs"] = a, b, compare_hvs(a, b, f"{w}x{h}")
        print(f"{w}x{h}", arrays[f"size_{w}x{h}_hvs"][:, 1].tolist(), flush=True)
    stats_golden = np.load(S.GOLDEN)
    for name, img, ext, args, _ in S.cases():
        data, hvs = run_stats_case(img, ext, args)
        assert (stats_golden["file_" + name] == data).all() and (stats_golden["src_" + name] == img).all(), f"{name}: not the file image_stats_vectors.npz holds"
        assert hvs.shape[0] == stats_golden["stats_" + name].shape[0]
        arrays["stats_hvs_" + name] = hvs
        meta["cases"].append({"name": name, "slices": int(hvs.shape[0])})
        print(name, hvs.shape[0], "slices, RGB PSNR-HVS-M", hvs[:, 2, 1].tolist(), flush=True)
    arrays["meta"] = np.frombuffer(json.dumps(meta, sort_keys=True).encode(), np.uint8)
    S.save(GOLDEN, arrays)
    assert GOLDEN.stat().st_size <= 1 << 20, GOLDEN.stat().st_size
    print("wrote", GOLDEN, GOLDEN.stat().st_size, "bytes,", len(arrays), "members")
