#!/usr/bin/env python3
"""The look-up tables of the ETC1S -> BC1 block conversion (etc1s_transcode_kernels.hip), computed from the two formats' definitions. The small ones are generated into
basis_universal_amd/csrc/etc1s_transcode_tables.inc. The two endpoint tables (15,360 entries each) are NOT committed as numbers: the library computes them on the device
the first time a context transcodes to BC1 (etc1s_build_bc1_tables_kernel, the same search as endpoint_table() below, which the golden generator and the tests use as the
host-side statement of it).

ETC1S side: a block has one 5-bit base colour per channel, expanded to 8 bits as (c << 3) | (c >> 2), and one of eight intensity tables whose four modifiers are
added to every channel and clamped to 0..255; a selector 0..3 per texel picks the modifier (ascending order).
BC1 side: two endpoints, 5 bits for red / blue and 6 bits for green, expanded as (c << 3) | (c >> 2) and (c << 2) | (c >> 4); the four colours of a block are
c0 = lo, c3 = hi, c1 = (2 c0 + c3) / 3, c2 = (2 c3 + c0) / 3 (integer division), in that linear order.

Because an ETC1S block moves all channels by the same modifiers, the conversion is separable: per channel, for
    intensity table (8) x 5-bit base value (32) x selector range in use (6: lo..hi of the block's selectors) x selector mapping (10: which of the four BC1 colours
    each ETC1S selector is sent to)
the table holds the BC1 endpoint pair (lo, hi) with the least squared error over the selectors of the range, and that error. The block conversion sums the three
channels' errors per mapping and takes the best mapping. Search order: hi outermost, lo innermost, first minimum wins -- the tie rule the reference tool's BC1 output
shows (tests/golden/etc1s_transcode_vectors.npz, whose coverage member hits every range x mapping pair, decides that).

Also: for solid blocks the endpoint pair whose colour 1 (2/3 hi + 1/3 lo) is nearest a value, with a small penalty on the endpoints' distance; and for two-colour
blocks of the widest table the endpoint nearest a value.

usage: gen_etc1s_transcode_tables.py [--check]     (--check: regenerate in memory and compare with the committed file)"""
import pathlib
import sys

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parent.parent
OUT = ROOT / "basis_universal_amd" / "csrc" / "etc1s_transcode_tables.inc"

INTEN = np.array([[-8, -2, 2, 8], [-17, -5, 5, 17], [-29, -9, 9, 29], [-42, -13, 13, 42], [-60, -18, 18, 60], [-80, -24, 24, 80], [-106, -33, 33, 106], [-183, -47, 47, 183]])
RANGES = [(0, 3), (1, 3), (0, 2), (1, 2), (2, 3), (0, 1)]
MAPPINGS = [(0, 0, 1, 1), (0, 0, 1, 2), (0, 0, 1, 3), (0, 0, 2, 3), (0, 1, 1, 1), (0, 1, 2, 2), (0, 1, 2, 3), (0, 2, 3, 3), (1, 2, 2, 2), (1, 2, 3, 3)]


def expand(bits):
    v = np.arange(1 << bits)
    return (v << (8 - bits)) | (v >> (2 * bits - 8))


def endpoint_table(bits):
    """[inten][base5][range][mapping] -> lo | hi << 8 | err << 16"""
    e = expand(bits)
    n = e.size
    hi, lo = np.meshgrid(e, e, indexing="ij")   # axis 0 = hi (outer), axis 1 = lo (inner)
    colors = np.stack([lo, (lo * 2 + hi) // 3, (hi * 2 + lo) // 3, hi], -1).reshape(n * n, 4)
    base = expand(5)
    out = np.zeros((8, 32, len(RANGES), len(MAPPINGS)), np.uint32)
    for t in range(8):
        block = np.clip(base[:, None] + INTEN[t][None, :], 0, 255)   # (32, 4)
        for r, (s0, s1) in enumerate(RANGES):
            for m, mapping in enumerate(MAPPINGS):
                err = np.zeros((32, n * n), np.int64)
                for s in range(s0, s1 + 1):
                    d = block[:, s][:, None] - colors[:, mapping[s]][None, :]
                    err += d * d
                best = err.argmin(1)   # first minimum
                best_err = err[np.arange(32), best]
                assert best_err.max() <= 0xFFFF
                out[t, :, r, m] = (best % n) | ((best // n) << 8) | (best_err << 16)
    return out.reshape(-1)


def solid_table(bits, sel):
    """[value] -> (hi, lo): sel 1: colour 1 of the pair nearest the value; sel 0: the endpoint nearest the value (lo = 0)"""
    e = expand(bits)
    n = e.size
    out = np.zeros((256, 2), np.uint8)
    lo, hi = np.meshgrid(e if sel == 1 else e[:1], e, indexing="ij")   # lo outer, hi inner
    for i in range(256):
        if sel == 1:
            err = np.abs((hi * 2 + lo) // 3 - i) + (np.abs(hi - lo) * 3) // 100
        else:
            err = np.abs(hi - i)
        k = int(err.reshape(-1).argmin())
        out[i] = (k % n, k // n)
    return out.reshape(-1)


def emit(name, ctype, values, per_line, comment, fmt):
    lines = [f"// {comment}", f"BU_TAB {ctype} {name}[{values.size}] = {{"]
    for i in range(0, values.size, per_line):
        lines.append("  " + " ".join(fmt % int(v) + "," for v in values[i:i + per_line]))
    lines.append("};")
    return "\n".join(lines)


def generate():
    range_index = np.full((4, 4), 255, np.uint8)
    for i, (a, b) in enumerate(RANGES):
        range_index[a, b] = i
    linear_to_bc1 = [0, 2, 3, 1]    # the four colours in linear order -> BC1's selector codes (0 = c0, 1 = c3, 2 and 3 between)
    inverted = [1, 0, 3, 2]         # the same colour when the two endpoints are swapped
    xlat = np.zeros((len(MAPPINGS), 2, 4), np.uint8)
    for m, mapping in enumerate(MAPPINGS):
        for s in range(4):
            xlat[m, 0, s] = linear_to_bc1[mapping[s]]
            xlat[m, 1, s] = inverted[linear_to_bc1[mapping[s]]]
    parts = [
        "// GENERATED by tools/gen_etc1s_transcode_tables.py from the ETC1S and BC1 format definitions -- do not edit. Tables of the ETC1S -> BC1 block conversion.",
        "// BU_TAB is defined by the includer: `static const` on the host, `static __device__ const` under hipcc.",
        emit("ke_bc1_range_index", "unsigned char", range_index.reshape(-1), 16, "[lowest selector][highest selector] of a block -> selector range (255: cannot occur, lo > hi or lo == hi)", "%3u"),
        emit("ke_bc1_selector_xlat", "unsigned char", xlat.reshape(-1), 8, "[mapping][endpoints swapped][ETC1S selector] -> BC1 selector code", "%u"),
        emit("ke_bc1_ranges", "unsigned char", np.array(RANGES, np.uint8).reshape(-1), 12, "[range] {lowest, highest selector}", "%u"),
        emit("ke_bc1_mappings", "unsigned char", np.array(MAPPINGS, np.uint8).reshape(-1), 4, "[mapping][ETC1S selector] -> which of BC1's four colours in linear order (c0, 2/3 c0, 2/3 c3, c3)", "%u"),
        emit("ke_bc1_solid5", "unsigned char", solid_table(5, 1), 32, "[value] {hi, lo}: 5-bit endpoints whose colour 1 is nearest the value", "%2u"),
        emit("ke_bc1_solid6", "unsigned char", solid_table(6, 1), 32, "the same, 6-bit", "%2u"),
        emit("ke_bc1_end5", "unsigned char", solid_table(5, 0)[0::2], 32, "[value]: the 5-bit endpoint nearest the value", "%2u"),
        emit("ke_bc1_end6", "unsigned char", solid_table(6, 0)[0::2], 32, "the same, 6-bit", "%2u"),
    ]
    return "\n".join(parts) + "\n"


if __name__ == "__main__":
    text = generate()
    if "--check" in sys.argv[1:]:
        assert OUT.read_text() == text, f"{OUT} is not what this script generates"
        print("ok:", OUT)
    else:
        OUT.write_text(text)
        print("wrote", OUT, len(text), "bytes")
