#!/usr/bin/env python3
"""Known answers of the compressor's source-image options from the real reference tool (oracle/_ref/basisu, build machine only)
-> tests/golden/source_prep_vectors.npz and tests/golden/source_prep_digests.json.

Every case of tests/source_prep_helpers.py (a seeded tiny image, a codec and the tool's flags) is compressed by `basisu -no_multithreading -debug -debug_images`:
  slice<k>_<case>   what the tool saved as basis_debug_source_image_0_slice_<k>.png: the slice's source image after ALL preparation and mip generation, padded to
                    whole blocks as the tool pads it, ETC1S alpha slices as their own (a, a, a, 255) images
  file_<case>       the .basis / .ktx2 it wrote (the same bytes with and without the two debug flags: asserted)
and `meta` holds per case its flags, the number of slices, every slice's unpadded size, and has_alpha as the tool's debug output states it ("has alpha: N").
The digests: a 4096x4096 image holding every RGB value once (alpha a fixed pattern) through `-renorm -uastc -uastc_level 0 -debug_images`; of the tool's prepared
raster only the SHA-256 of every band of 64 rows is kept (64 digests), after asserting that alpha came through unchanged.
usage: gen_golden_source_prep.py"""
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
import source_prep_helpers as H  # noqa: E402
import gen_golden_image_stats as S  # noqa: E402

BASISU = S.BASISU


def load_png(path):
    from PIL import Image
    im = Image.open(path)
    assert im.mode in ("RGB", "RGBA"), (path, im.mode)   # the tool's save_png writes three channels exactly when image::has_alpha says every alpha is 255
    return np.ascontiguousarray(np.array(im.convert("RGBA"), dtype=np.uint8))


def codec_flags(case):
    if case["uastc"]:
        return ["-uastc", "-uastc_level", "2"] + (["-ktx2_no_zstandard"] if case["ext"] == "ktx2" else [])
    return ["-q", "128"]


def run_tool(img, ext, args, cwd, threads=False):
    helpers.save_png(pathlib.Path(cwd) / "in0.png", img)
    r = subprocess.run([str(BASISU), *([] if threads else ["-no_multithreading"]), f"-{ext}", *args, "in0.png", "-output_file", f"out.{ext}"], cwd=cwd,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-3000:]
    return np.frombuffer((pathlib.Path(cwd) / f"out.{ext}").read_bytes(), np.uint8).copy(), r.stdout


def run_case(case):
    """-> (file bytes, [slice rasters], [(orig_w, orig_h)], has_alpha)"""
    img, args = H.source_image(case), codec_flags(case) + case["flags"]
    with tempfile.TemporaryDirectory() as d:
        plain, _ = run_tool(img, case["ext"], args, d)
    with tempfile.TemporaryDirectory() as d:
        data, text = run_tool(img, case["ext"], args + ["-debug", "-debug_images"], d)
        assert (data.shape == plain.shape) and (data == plain).all(), f"{case['name']}: the debug flags changed the file"
        (has_alpha,) = re.findall(r"Source image index 0 filename .* has alpha: (\d)", text)
        described = re.findall(r"\*+ Slice (\d+): mip (\d+), alpha_slice: (\d), filename: .*, original: (\d+)x(\d+) actual: (\d+)x(\d+)", text)
        rasters, sizes = [], []
        for k, (index, _, _, ow, oh, aw, ah) in enumerate(described):
            assert int(index) == k
            raster = load_png(pathlib.Path(d) / f"basis_debug_source_image_0_slice_{k}.png")
            assert raster.shape == (int(ah), int(aw), 4), (case["name"], k, raster.shape)
            rasters.append(raster)
            sizes.append((int(ow), int(oh)))
        assert rasters and not (pathlib.Path(d) / f"basis_debug_source_image_0_slice_{len(rasters)}.png").exists()
    return data, rasters, sizes, bool(int(has_alpha))


def all_colours_digests():
    img = H.all_colours_image()
    with tempfile.TemporaryDirectory() as d:
        run_tool(img, "basis", ["-renorm", "-uastc", "-uastc_level", "0", "-debug_images"], d, threads=True)   # the prepared raster does not depend on the threads
        raster = load_png(pathlib.Path(d) / "basis_debug_source_image_0_slice_0.png")
    assert raster.shape == img.shape and (raster[..., 3] == img[..., 3]).all(), "alpha did not come through unchanged"
    changed = int((raster[..., :3] != img[..., :3]).any(axis=2).sum())
    assert 0 < changed < H.ALL_SIDE ** 2
    return H.band_digests(raster), changed


if __name__ == "__main__":
    assert BASISU.exists(), "oracle/_ref/basisu is missing: build it on the build machine (make -C oracle ref)"
    arrays, meta = {}, {"cases": []}
    for kind in ("normal",):
        for w, h in ((21, 13), (20, 28)):
            _, counts = H.normal_map_image(w, h, 1)
            assert all(v >= w * h // 10 for v in counts.values()), counts     # the known shares: off unit length, exactly grey, near zero
    for case in H.case_list():
        data, rasters, sizes, has_alpha = run_case(case)
        arrays["file_" + case["name"]] = data
        for k, raster in enumerate(rasters):
            arrays[f"slice{k}_{case['name']}"] = raster
        meta["cases"].append(dict(case, slices=len(rasters), sizes=sizes, has_alpha=has_alpha))
        print(case["name"], data.size, "bytes,", len(rasters), "slices", sizes, "has alpha", has_alpha, flush=True)
    arrays["meta"] = np.frombuffer(json.dumps(meta, sort_keys=True).encode(), np.uint8)
    if H.GOLDEN.exists():   # cases are only ever added: what the committed file holds comes out as it is, before anything is overwritten
        committed, committed_meta = H.native_libs.load_npz_golden(H.GOLDEN)
        for key, value in committed.items():
            assert key == "meta" or (key in arrays and arrays[key].shape == value.shape and (arrays[key] == value).all()), f"{key}: not what the committed fixture holds"
        assert json.loads(json.dumps(meta["cases"]))[:len(committed_meta["cases"])] == committed_meta["cases"], "a committed case's description changed"
        print("all", len(committed) - 1, "committed members and", len(committed_meta["cases"]), "committed cases unchanged")
    S.save(H.GOLDEN, arrays)
    assert H.GOLDEN.stat().st_size <= 1 << 20, H.GOLDEN.stat().st_size
    print("wrote", H.GOLDEN, H.GOLDEN.stat().st_size, "bytes,", len(arrays), "members")
    bands, changed = all_colours_digests()
    H.DIGESTS.write_text(json.dumps({"image": "source_prep_helpers.all_colours_image", "flags": ["-renorm", "-uastc", "-uastc_level", "0", "-debug_images"],
                                     "band_rows": H.BAND_ROWS, "pixels_changed": changed, "sha256": bands}, indent=1, sort_keys=True) + "\n")
    print("wrote", H.DIGESTS, len(bands), "digests,", changed, "pixels changed")
