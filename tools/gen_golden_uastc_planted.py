#!/usr/bin/env python3
"""Generate tests/golden/uastc_planted_vectors.npz: the four planted tile families of tests/uastc_planted.py (tiles of every UASTC mode, partition pattern and
dual-plane selector) with the answers of the REAL reference (oracle/_ref/libref_harness.so; build machine only):
  <family>_tiles                     (1020, 4, 4, 4) u8
  <family>_level0 .. _level3         encode_uastc of every tile; <family>_level4 of every third tile
  exact_<option flag set>            the eight option-flag sets of helpers.uastc_flag_sets() on `exact`
  sibling_rdo_l<2|3>_<case>          uastc_rdo (uastc_planted.RDO_CASES) on sibling_level2 / sibling_level3
  meta                               seeds, and per array the number of cells the reference reached (encoder: tiles that land in the cell they were planted in;
                                     RDO: cells holding a block it modified)
The conditions tests/test_uastc_planted_host.py holds the committed file to are checked here before it is written."""
import pathlib
import sys

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests"))
sys.path.insert(0, str(ROOT))
import helpers  # noqa: E402
import uastc_planted as P  # noqa: E402
from gen_golden_uastc_transcode import helpers_save  # noqa: E402


def main():
    assert helpers.have_ref(), "oracle/_ref/libref_harness.so is not built (make -C oracle ref)"
    _, tiles = P.families()
    arrays = {f"{fam}_tiles": np.ascontiguousarray(tiles[fam]) for fam in P.FAMILIES}
    for name, fam, flags, step in P.encoder_arrays():
        arrays[name] = helpers.ref_encode_uastc(np.ascontiguousarray(tiles[fam][::step]), flags)
        print(name, "cells reached", len(P.reached(arrays[name], step)), flush=True)
    for name, src, flags, jobs, kw in P.rdo_arrays():
        arrays[name] = helpers.ref_uastc_rdo(arrays[src], tiles["sibling"], flags, jobs, **kw)
        print(name, "blocks modified", int((arrays[name] != arrays[src]).any(1).sum()), "in cells", len(P.modified_cells(arrays[src], arrays[name])), flush=True)
    meta = P.make_meta(arrays)
    arrays["meta"] = P.meta_bytes(meta)
    import test_uastc_planted_host as H
    H.check_conditions(arrays, meta)
    helpers_save(P.GOLDEN, arrays)
    size = P.GOLDEN.stat().st_size
    assert size < 1000000, size
    print("wrote", P.GOLDEN, size, "bytes")


if __name__ == "__main__":
    main()
