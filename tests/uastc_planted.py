"""Tiles planted in every UASTC cell, and the fixture that holds them (tests/golden/uastc_planted_vectors.npz, written by tools/gen_golden_uastc_planted.py).

A CELL is (mode, partition pattern, dual-plane component selector). UASTC LDR 4x4 has 171 of them: modes 2, 4, 9 and 16 with 30 patterns each, mode 3 with 11,
mode 7 with 19, mode 6 with selectors 0-2, modes 11 and 13 with selectors 0-3, the nine other non-solid modes with one cell each (mode 17 has no selector field and
unpacks as selector 3), and the solid mode 8. A planted tile is the DECODED form of a valid block of a chosen cell whose endpoints and weights are random: the encoder,
given that tile, has a candidate of that cell with (nearly) no error, so at the levels that try the mode it lands there -- on partition table rows, anchor indices and
selector rotations the image-like vectors of uastc_reference_vectors.npz never reach.

Four families, TILES_PER_CELL tiles per non-solid cell each, tile i belonging to cell CELLS[i // TILES_PER_CELL]:
  exact    the decoded block as it is
  noisy    a fresh draw plus uniform noise of -2 .. 2 per texel and channel that keeps the tile's class: alpha stays 255 in opaque tiles, grey tiles get one value for r, g, b
  edge     endpoints in the outer eighths of the range (unquantised value below 32 or above 223): most tiles have a channel within 8 of 0 or 255, where the ETC1 hint
           search clamps
  sibling  the six tiles of a cell share one block up to one flipped weight bit each, every endpoint moved by at most one quantisation level: neighbours the RDO pass
           can take selectors from, so that it modifies blocks of most cells. The two ends of a component lie within a quarter of the range of each other: RDO
           accepts a trial whose error is at most ten times the block's own, and with ends drawn over the whole range one step of a 2-bit weight is more than
           that in mode 4 (whose BC7 transcode is nearly lossless, so that its own error is small): a third of its patterns was out of reach
Blocks are built field by field through transcode_helpers.Layout from the raw PCG64 stream (_Bits), and decoded by helpers.host_decode_uastc. The tests read the tiles
from the fixture, never from here: only the generator and the one test that compares the two call families()."""
import json
import pathlib

import numpy as np

import helpers
import transcode_helpers as T

GOLDEN = pathlib.Path(__file__).resolve().parent / "golden" / "uastc_planted_vectors.npz"
FAMILIES = ("exact", "noisy", "edge", "sibling")
SEEDS = {"exact": 20261101, "noisy": 20261102, "edge": 20261103, "sibling": 20261104}
TILES_PER_CELL = 6
NOISE = 2
SIBLING_SPAN = 4    # sibling: the high end of a component within levels / 4 of its low end
LEVEL4_STEP = 3     # level 4 answers are kept for every third tile: two tiles of every cell
# the modes encode_uastc tries per level (the level's mode mask; levels 3 and 4 try all)
LEVEL_MODES = {0: (0, 8, 11, 12, 15), 1: (0, 4, 6, 8, 9, 11, 12, 15, 17), 2: (0, 1, 4, 5, 6, 8, 9, 10, 11, 12, 13, 15, 16, 17), 3: tuple(range(19)), 4: tuple(range(19))}
PATTERN_MODES = (2, 3, 4, 7, 9, 16)
# (name, total_jobs, uastc_rdo_params overrides) of the RDO answers kept for `sibling`, each on the blocks packed at every level of RDO_LEVELS
RDO_CASES = [("lam1", 0, dict(lam=1.0)), ("lam4_jobs3", 3, dict(lam=4.0)), ("lam20_norefine", 0, dict(lam=20.0, refine=0))]
RDO_LEVELS = (2, 3)
OPTION_FLAG_SETS = helpers.uastc_flag_sets()[5:]   # the eight sets behind the five plain levels


def _cell_list():
    out = []
    for lay in T.layouts():
        if lay.mode == 8:
            continue
        patterns = range(lay.pattern_limit) if lay.pattern_bits else (0,)
        selectors = (3,) if lay.mode == 17 else (range(3) if lay.mode == 6 else (range(4) if lay.ccs_bits else (0,)))
        out += [(lay.mode, p, s) for p in patterns for s in selectors]
    return out


_cells = None


def cell_list():
    """the 170 non-solid cells, ordered by mode, then pattern, then selector"""
    global _cells
    if _cells is None:
        _cells = _cell_list()
        assert len(_cells) == 170
    return _cells


SOLID_CELL = (8, 0, 0)


def cells_of_modes(modes):
    return [c for c in cell_list() if c[0] in modes]


def cells(packed):
    """(n, 16) UASTC blocks -> [(mode, pattern, selector)] as the core's unpacker reads them"""
    out = []
    for b in np.ascontiguousarray(packed, np.uint8).reshape(-1, 16):
        mode, _, _, pattern, ccs = T.unpacked_fields(b)
        assert mode != 255, b.tobytes().hex()
        out.append((mode, pattern, ccs))
    return out


def planted_cells():
    """the cell every tile of a family was planted in"""
    return [c for c in cell_list() for _ in range(TILES_PER_CELL)]


def reached(packed, step=1):
    """the cells in which the block of tile i * step lies in the cell the tile was planted in"""
    got = cells(packed)
    want = planted_cells()[::step]
    assert len(got) == len(want)
    return sorted({g for g, w in zip(got, want) if g == w})


def modified_cells(before, after):
    """the cells (of the blocks as they went in) of the blocks a pass changed"""
    changed = np.flatnonzero((np.asarray(before) != np.asarray(after)).any(axis=1))
    return sorted(set(cells(np.asarray(before)[changed])))


def describe_differences(got, want, tiles_cells=None, limit=8):
    """for an assertion message: how many blocks differ, and the cells (of the expected blocks) they lie in"""
    bad = np.flatnonzero((np.asarray(got) != np.asarray(want)).any(axis=1))
    if not bad.size:
        return ""
    where = cells(np.asarray(want)[bad])
    text = f"{bad.size} of {len(want)} blocks differ, in cells (mode, pattern, selector) {sorted(set(where))[:40]}; first"
    for i, c in list(zip(bad, where))[:limit]:
        planted = f", planted in {tiles_cells[i]}" if tiles_cells is not None else ""
        text += f"\n  block {i} cell {c}{planted}: got {np.asarray(got)[i].tobytes().hex()} want {np.asarray(want)[i].tobytes().hex()}"
    return text


# ---------------------------------------------------------------- the generator

_unquant = {}


def unquant(lay):
    """the unquantised value (0 .. 255) of every endpoint index of the mode's range, read off the decoder: a block whose endpoints all hold index i decodes to that value"""
    if lay.mode not in _unquant:
        blocks = []
        for i in range(lay.levels):
            v = T._put(0, 0, lay.code_len, lay.code)
            blocks.append(T._put_endpoints(v, lay, [i] * lay.ep_values))
        _unquant[lay.mode] = helpers.host_decode_uastc(T._to_blocks(blocks))[:, 0, 0, 0].astype(np.int64)
    return _unquant[lay.mode]


def _block(rng, lay, cell, values, weights=None):
    """a valid block of the cell: random bits under the mode's code (hints, and the weights unless given), the pattern, the selector and the endpoint values written over them"""
    _, pattern, sel = cell
    v = T._put(rng.bits128(), 0, lay.code_len, lay.code)
    if lay.pattern_bits:
        v = T._put(v, lay.pattern_ofs, lay.pattern_bits, pattern)
    if lay.ccs_bits:
        v = T._put(v, lay.ccs_ofs, lay.ccs_bits, sel)
    v = T._put_endpoints(v, lay, values)
    if weights is not None:
        v = T._put(v, lay.weight_ofs, lay.weight_len, weights)
    return v


def _family_exact(rng):
    out = []
    for cell in cell_list():
        lay = T.layouts()[cell[0]]
        for _ in range(TILES_PER_CELL):
            out.append(_block(rng, lay, cell, [rng.below(lay.levels) for _ in range(lay.ep_values)]))
    return T._to_blocks(out)


def _family_edge(rng):
    out = []
    for cell in cell_list():
        lay = T.layouts()[cell[0]]
        uq = unquant(lay)
        outer = [int(i) for i in np.flatnonzero((uq < 32) | (uq > 223))]
        for _ in range(TILES_PER_CELL):
            out.append(_block(rng, lay, cell, [outer[rng.below(len(outer))] for _ in range(lay.ep_values)]))
    return T._to_blocks(out)


def _family_sibling(rng):
    out = []
    for cell in cell_list():
        lay = T.layouts()[cell[0]]
        by_value = np.argsort(unquant(lay), kind="stable")      # endpoint indices in the order of their values
        rank = np.argsort(by_value, kind="stable")
        base, reach = [], max(2, lay.levels // SIBLING_SPAN)
        for _ in range(lay.ep_values // 2):     # per subset and component {low, high}: the two ends within a quarter of the range of each other
            lo = rng.below(lay.levels)
            hi = min(max(lo + rng.below(2 * reach + 1) - reach, 0), lay.levels - 1)
            base += [int(by_value[lo]), int(by_value[hi])]
        weights = rng.bits128() & ((1 << lay.weight_len) - 1)
        for k in range(TILES_PER_CELL):
            values = [int(by_value[min(max(int(rank[x]) + rng.below(3) - 1, 0), lay.levels - 1)]) for x in base]
            flipped = weights ^ (1 << rng.below(lay.weight_len)) if k else weights
            out.append(_block(rng, lay, cell, values, flipped))
    return T._to_blocks(out)


def _add_noise(rng, tiles):
    out = tiles.astype(np.int64)
    for t in out:
        opaque, grey = bool((t[..., 3] == 255).all()), bool((t[..., 0] == t[..., 1]).all() and (t[..., 0] == t[..., 2]).all())
        for y in range(4):
            for x in range(4):
                d = [rng.below(2 * NOISE + 1) - NOISE for _ in range(4)]
                if grey:
                    d[1] = d[2] = d[0]
                if opaque:
                    d[3] = 0
                t[y, x] += d
    out = np.clip(out, 0, 255)
    grey = (tiles[..., 0] == tiles[..., 1]).all(axis=(1, 2)) & (tiles[..., 0] == tiles[..., 2]).all(axis=(1, 2))
    assert ((out[..., 3] == 255).all(axis=(1, 2)) >= (tiles[..., 3] == 255).all(axis=(1, 2))).all()
    assert ((out[grey][..., 0] == out[grey][..., 1]) & (out[grey][..., 0] == out[grey][..., 2])).all()
    return out.astype(np.uint8)


def families():
    """-> ({family: the planted blocks (n, 16)}, {family: the tiles (n, 4, 4, 4) u8}); `noisy` has the blocks its tiles were before the noise"""
    blocks = {"exact": _family_exact(T._Bits(SEEDS["exact"])), "noisy": _family_exact(T._Bits(SEEDS["noisy"])),
              "edge": _family_edge(T._Bits(SEEDS["edge"])), "sibling": _family_sibling(T._Bits(SEEDS["sibling"]))}
    tiles = {k: helpers.host_decode_uastc(v) for k, v in blocks.items()}
    tiles["noisy"] = _add_noise(T._Bits(SEEDS["noisy"] + 1000), tiles["noisy"])
    for k in FAMILIES:
        assert cells(blocks[k]) == planted_cells(), k
    return blocks, tiles


# ---------------------------------------------------------------- the fixture

def encoder_arrays():
    """[(array name, family, pack flags, tile step)] of the encoder answers the fixture holds"""
    out = []
    for fam in FAMILIES:
        out += [(f"{fam}_level{level}", fam, level, LEVEL4_STEP if level == 4 else 1) for level in range(5)]
    out += [(f"exact_{name}", "exact", flags, 1) for name, flags in OPTION_FLAG_SETS]
    return out


def rdo_arrays():
    """[(array name, the packed array it starts from, pack flags, total_jobs, parameter overrides)] of the RDO answers the fixture holds"""
    return [(f"sibling_rdo_l{level}_{name}", f"sibling_level{level}", level, jobs, kw) for level in RDO_LEVELS for name, jobs, kw in RDO_CASES]


_loaded = None


def load():
    """-> (arrays of the fixture, read-only and shared; its meta)"""
    global _loaded
    if _loaded is None:
        import native_libs
        _loaded = native_libs.load_npz_golden(GOLDEN)
    return _loaded


def meta_counts(arrays):
    """what `meta` records per array: how many cells the encoder answers reach (tiles that land in the cell they were planted in), how many cells hold blocks the
    RDO answers modified"""
    counts = {name: len(reached(arrays[name], step)) for name, _, _, step in encoder_arrays()}
    counts.update({name: len(modified_cells(arrays[src], arrays[name])) for name, src, _, _, _ in rdo_arrays()})
    return counts


def make_meta(arrays):
    return {"seeds": SEEDS, "tiles_per_cell": TILES_PER_CELL, "noise": NOISE, "level4_step": LEVEL4_STEP, "sibling_span": SIBLING_SPAN, "cells": len(cell_list()), "cells_reached": meta_counts(arrays)}


def meta_bytes(meta):
    return np.frombuffer(json.dumps(meta, sort_keys=True).encode(), np.uint8)
