#!/usr/bin/env python3
"""Known answers of one resampling step from the real image_resample (oracle/_ref/libref_harness.so: ref_image_resample, build machine only)
-> tests/golden/resample_vectors.npz.

Every case of tests/test_mipmap_host.py::WIDE_AND_MAGNIFY (source size, destination size, sRGB, filter, filter scale, wrapping, components) with both seeds of SEEDS and the case's EXTRA_SEEDS:
  out<k>_seed<s>    the (dst_h, dst_w, 4) bytes the reference wrote for case k from rgba(src_w, src_h, s, noise)
and `meta` holds the case table, every case's seeds and the pass order each case is there for. The inputs are not stored: rgba() makes them again.
usage: gen_golden_resample.py"""
import json
import pathlib
import sys

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests"))
sys.path.insert(0, str(ROOT / "tools"))
import helpers  # noqa: E402
import test_mipmap_host as T  # noqa: E402
import gen_golden_image_stats as S  # noqa: E402


if __name__ == "__main__":
    assert helpers.have_ref(), "oracle/_ref/libref_harness.so is missing: build it on the build machine (make -C oracle ref)"
    arrays, raw = {}, 0
    for k, case in enumerate(T.WIDE_AND_MAGNIFY):
        sw, sh, dw, dh, srgb, flt, scale, wrap, comps = case
        for seed, noise in T.seeds_of(case):
            out = T.reference(T.rgba(sw, sh, seed, noise), dw, dh, srgb, flt, scale, wrap, comps)
            arrays[f"out{k}_seed{seed}"] = out
            raw += out.nbytes
        print(T.case_id(case), T.PASS_ORDER[case], out.shape, flush=True)
    meta = {"cases": [list(c) for c in T.WIDE_AND_MAGNIFY], "seeds": [[list(s) for s in T.seeds_of(c)] for c in T.WIDE_AND_MAGNIFY], "pass_order": [T.PASS_ORDER[c] for c in T.WIDE_AND_MAGNIFY],
            "layout": "out<case index>_seed<seed>: (dst_h, dst_w, 4) u8 of ref_image_resample on test_mipmap_host.rgba(src_w, src_h, seed, noise)"}
    arrays["meta"] = np.frombuffer(json.dumps(meta, sort_keys=True).encode(), np.uint8)
    S.save(T.GOLDEN, arrays)
    assert T.GOLDEN.stat().st_size <= 1 << 20, T.GOLDEN.stat().st_size
    print("wrote", T.GOLDEN, T.GOLDEN.stat().st_size, "bytes,", len(arrays), "members,", raw, "bytes of outputs")
