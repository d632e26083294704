#!/usr/bin/env python3
"""Known answers for the ETC1S -> BC7 chroma filter and the mode-5 encoder under it, at every comparison they branch on, from the real reference (oracle/_ref,
build machine only; `make -C oracle ref`) -> tests/golden/etc1s_bc7_filter_vectors.npz. The cases are tests/etc1s_bc7_filter_cases.py's.

Tiles: per tile class the 16-byte answers of bc7_mode_5_encoder::encode_bc7_mode_5_block (ref_encode_bc7_mode5 of the harness), key tiles_<class>; the tiles
themselves come from their seeds, except the searched class alt_sums, whose tiles are stored too (alt_sums_tiles).
States: per state the .basis file this package's backend writer makes of it (key file_<state>) and, per image, the raw BC7 blocks of `basisu -unpack -ktx_only`
(_bc7) and of a second run with -no_etc1s_chroma_filtering (_bc7nf), keyed as tools/gen_golden_etc1s_texture.py keys them.
`meta` holds the route counts, the reports of the two searches (the variance gate's and the doubtful routes') and the table of mutation against blocks changed.
The file is accepted only after the CPU restatement (tests/etc1s_texture_helpers.py) has reproduced every block in it.
usage: gen_golden_etc1s_bc7_filter.py [--no-mutations | --mutations-only]"""
import ctypes as C
import json
import pathlib
import sys

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests"))
sys.path.insert(0, str(ROOT / "tools"))
sys.path.insert(0, str(ROOT))
import helpers  # noqa: E402
import etc1s_transcode_helpers as E  # noqa: E402
import etc1s_texture_helpers as X  # noqa: E402
import etc1s_bc7_filter_cases as K  # noqa: E402
import gen_golden_etc1s_transcode as GG  # noqa: E402
import gen_golden_etc1s_texture as GT  # noqa: E402

MAX_BYTES = 621589   # tests/golden/uastc_texture_vectors.npz


def ref_encode(tiles):
    tiles = np.ascontiguousarray(tiles, np.uint8)
    out = np.zeros((len(tiles), 16), np.uint8)
    u8p = C.POINTER(C.c_uint8)
    assert helpers.ref().ref_encode_bc7_mode5(tiles.ctypes.data_as(u8p), len(tiles), out.ctypes.data_as(u8p)) == 1
    return out


def tile_member(arrays, meta):
    meta["alt_sums_search"], arrays["alt_sums_tiles"] = K.alt_sums_search()
    print("alt sums search", meta["alt_sums_search"], flush=True)
    for name in K.TILE_CLASSES:
        tiles = K.tiles_of(name, arrays)
        want = ref_encode(tiles)
        got, routes = K.restate_tiles(tiles)
        bad = np.flatnonzero((got != want).any(1))
        assert bad.size == 0, (name, bad[:8], got[bad[:2]], want[bad[:2]], tiles[bad[:1], :, :3])
        arrays["tiles_" + name] = want
        meta["tile_routes"][name] = {r: routes.count(r) for r in sorted(set(routes))}
        print("tiles", name, len(tiles), meta["tile_routes"][name], flush=True)


def state_member(name, state, arrays, meta):
    data = K.write_state(state)
    arrays["file_" + name] = data
    tool = {}
    dec = GT.unpack_with_tool(name, bytes(data), "basis", tool)
    routes = {}
    for im in dec["images"]:
        key = E.image_key(name, im["level"], im["layer"], im["face"])
        for suffix, got in (("_bc7nf", X.bc7_blocks(dec, im, False)), ("_bc7", X.bc7_blocks(dec, im, True, routes))):
            bad = np.flatnonzero((got != tool[key + suffix]).any(1))
            assert bad.size == 0, (key, suffix, bad[:8], got[bad[:2]], tool[key + suffix][bad[:2]])
            arrays[key + suffix] = tool[key + suffix]
    meta["states"].append({"name": name, "images": [[im["level"], im["layer"], im["face"], im["width"], im["height"]] for im in dec["images"]]})
    meta["state_routes"][name] = {str(k): v for k, v in routes.items()}
    print("state", name, len(data), "bytes", meta["state_routes"][name], flush=True)


def mutation_table(arrays):
    """every mutation of the restatement against every golden block: how many blocks it changes, per tile class and per state"""
    table = {}
    for mutation in K.MUTATIONS:
        table[mutation] = K.blocks_changed(mutation, arrays, everything=True)
        print("mutation", mutation, table[mutation], flush=True)
        assert (sum(table[mutation].values()) > 0) != (mutation in K.EQUIVALENT), mutation   # grow the cases until every other mutation shows
    return table


if __name__ == "__main__":
    if "--mutations-only" in sys.argv:   # the table alone, over the file as it stands
        arrays, meta = K.golden()
        arrays = dict(arrays)
        meta["mutations"] = mutation_table(arrays)
        arrays["meta"] = np.frombuffer(json.dumps(meta, sort_keys=True).encode(), np.uint8)
        GG.save(K.GOLDEN, arrays)
        print("wrote", K.GOLDEN, K.GOLDEN.stat().st_size, "bytes")
        sys.exit(0)
    assert GG.BASISU.exists() and helpers.ref_harness_version() >= 4, "oracle/_ref is missing or older than harness version 4: build it on the build machine (make -C oracle ref)"
    arrays, meta = {}, {"tile_routes": {}, "state_routes": {}, "states": [], "tile_seeds": K.TILE_SEEDS}
    tile_member(arrays, meta)
    meta["variance_search"], kept = K.variance_search()
    meta["variance_kept"] = {kind: sum(1 for k in kept if k[2] == kind) for kind in ("below", "above", "at3", "exact", "fused")}
    print("variance search", meta["variance_search"], meta["variance_kept"], flush=True)
    meta["doubtful_search"], cells = K.doubtful_search()
    print("doubtful search", meta["doubtful_search"], flush=True)
    states = {"gate": K.gate_state(), "variance": K.variance_state(kept), "saturated": K.saturated_state(K.SATURATED_SEED), "quiet": K.quiet_state(),
              **{n: K.thin_state(n) for n in K.THIN_CHAINS}}
    if cells:
        states["doubtful"] = K.doubtful_state(cells)
        meta["doubtful_cells"] = [x[7] for x in cells]
    for name, state in states.items():
        state_member(name, state, arrays, meta)
    total = {}
    for r in meta["state_routes"].values():
        for k, v in r.items():
            total[k] = total.get(k, 0) + v
    meta["routes"] = total
    print("routes over the states", total, flush=True)
    if "--no-mutations" not in sys.argv:
        meta["mutations"] = mutation_table(arrays)
    arrays["meta"] = np.frombuffer(json.dumps(meta, sort_keys=True).encode(), np.uint8)
    GG.save(K.GOLDEN, arrays)
    assert K.GOLDEN.stat().st_size <= MAX_BYTES, K.GOLDEN.stat().st_size
    print("wrote", K.GOLDEN, K.GOLDEN.stat().st_size, "bytes,", len(arrays), "members")
