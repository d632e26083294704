#!/usr/bin/env python3
"""The look-up tables of the ETC1S -> BC1, -> EAC A8 and -> BC7 mode 5 block conversions (etc1s_transcode_kernels.hip), computed from the formats' definitions. The small ones are generated into
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

EAC A8 (the alpha half of ETC2 RGBA) and BC7 mode 5: eac_a8_table(), bc7_color_table(), bc7_alpha_table() and bc7_solid_table() below state their searches. The EAC,
BC7 alpha and BC7 solid tables go into the .inc; the BC7 colour table (15,360 entries) is built on the device like BC1's. tests/golden/etc1s_texture_vectors.npz,
whose coverage member reaches every entry a block can reach, decides the tie rules.

EAC R11 / RG11 and ASTC 4x4 (the third entry family): eac_r11_table(), astc_table_0_47(), astc_table_0_255() with astc_scaled_errors(), astc_best_grey_mapping(),
astc_unquant48(), astc_solid_table() and astc_nearest_table() state their searches. EAC R11 and the two small ASTC tables go into the .inc; the two ASTC endpoint
look-ups (15,360 entries each) are built on the device (etc1s_build_astc_tables_kernel). tests/golden/etc1s_block_format_vectors.npz decides the rules.

ATC RGB, PVRTC2 4bpp RGB and FXT1 (the fourth entry family): atc_endpoint_table() for the three look-ups 55 / 56 / 45 (built on the device by
etc1s_build_atc_tables_kernel; the reference carries this generator, and every entry agrees with what it ships), atc_solid_table() and atc_nearest_table() for the six
256-entry tables, which go into the .inc. FXT1 reads BC1's tables. PVRTC2 4bpp RGBA: pvrtc2_match_table() and atc_nearest_table() over the translucent mode's
endpoint expansions, five 256-entry tables for its constant blocks. tests/golden/etc1s_vendor_format_vectors.npz decides the rules.

usage: gen_etc1s_transcode_tables.py [--check]     (--check: regenerate in memory and compare with the committed file)"""
import functools
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


ALPHA_RANGES = [(0, 3), (1, 3), (0, 2), (1, 2)]   # the selector ranges of the EAC A8 look-up; a block of one selector never gets there, any other range reads entry 0
EAC_MODIFIERS = np.array([[-3, -6, -9, -15, 2, 5, 8, 14], [-3, -7, -10, -13, 2, 6, 9, 12], [-2, -5, -8, -13, 1, 4, 7, 12], [-2, -4, -6, -13, 1, 3, 5, 12],
                          [-3, -6, -8, -12, 2, 5, 7, 11], [-3, -7, -9, -11, 2, 6, 8, 10], [-4, -7, -8, -11, 3, 6, 7, 10], [-3, -5, -8, -11, 2, 4, 7, 10],
                          [-2, -6, -8, -10, 1, 5, 7, 9], [-2, -5, -8, -10, 1, 4, 7, 9], [-2, -4, -8, -10, 1, 3, 7, 9], [-2, -5, -7, -10, 1, 4, 6, 9],
                          [-3, -4, -7, -10, 2, 3, 6, 9], [-1, -2, -3, -10, 0, 1, 2, 9], [-4, -6, -8, -9, 3, 5, 7, 8], [-3, -5, -7, -9, 2, 4, 6, 8]])   # ETC2 EAC, table 3.17.2 of the Khronos data format spec


def eac_a8_values():
    """(256 * 15 * 16, 8): the eight values of an EAC A8 block, row (base * 15 + multiplier - 1) * 16 + table: clamp(base + multiplier * modifier). Multiplier 0 is
    left out of the search."""
    base, mul, table = np.meshgrid(np.arange(256), np.arange(1, 16), np.arange(16), indexing="ij")
    return np.clip(base.reshape(-1, 1) + mul.reshape(-1, 1) * EAC_MODIFIERS[table.reshape(-1)], 0, 255)


def nearest_value_table(values, ranges, code_bits, ends_weighted, target_of=lambda c: c):
    """[inten][base5][range] -> (row of `values`, trans): the candidate row whose values are nearest the ETC1S block's in-range colours, each colour on its nearest
    value (first minimum in code order), the squared differences summed; first minimum over the rows in their order. trans holds the code chosen for ETC1S selector
    s at bits code_bits * s, zero for a selector outside the range. ends_weighted: the widest intensity table over the whole selector range counts the errors of
    selectors 0 and 3 five times (there the two clamp to 0 or 255 and the block is about those). target_of: the value an 8-bit colour stands for on the scale of
    `values` (EAC R11 compares on 11 bits)."""
    v = values.astype(np.int16)
    near_err = np.zeros((256, v.shape[0]), np.int32)
    near_code = np.zeros((256, v.shape[0]), np.uint8)
    base = expand(5)
    blocks = np.clip(base[None, :, None] + INTEN[:, None, :], 0, 255)   # (8, 32, 4)
    for c in np.unique(blocks):
        d = np.abs(v - np.int16(target_of(int(c))))
        near_code[c] = d.argmin(1)
        near_err[c] = d.min(1)
    near_err *= near_err
    rows = np.zeros((8, 32, len(ranges)), np.uint32)
    trans = np.zeros_like(rows)
    for t in range(8):
        for g in range(32):
            for r, (s0, s1) in enumerate(ranges):
                five = ends_weighted and t == 7 and (s0, s1) == (0, 3)
                err = sum(near_err[blocks[t, g, s]] * (5 if five and s in (0, 3) else 1) for s in range(s0, s1 + 1))
                k = int(err.argmin())
                rows[t, g, r] = k
                trans[t, g, r] = sum(int(near_code[blocks[t, g, s], k]) << (code_bits * s) for s in range(s0, s1 + 1))
    return rows, trans


@functools.lru_cache(maxsize=None)
def eac_a8_table():
    """[inten][base5][range] -> base | (table | multiplier << 4) << 8 | trans << 16, the ETC1S -> EAC A8 look-up: the block's first two bytes, then the 3-bit code of
    each ETC1S selector. Search order: base outermost, then multiplier 1..15, table innermost, first minimum -- the loop order of the reference's generator, which the
    tool's output on the coverage file confirms."""
    rows, trans = nearest_value_table(eac_a8_values(), ALPHA_RANGES, 3, False)
    base, mul, table = rows // 240, (rows // 16) % 15 + 1, rows % 16
    return (base | ((table | mul << 4) << 8) | (trans << 16)).astype(np.uint32).reshape(-1)


def bc7_values(e):
    """(n * n, 4): the four colours of a BC7 2-bit index between endpoints hi (outer) and lo (inner) of the expanded values e: weights 0, 21, 43, 64 of 64, rounded"""
    hi, lo = np.meshgrid(e, e, indexing="ij")
    hi, lo = hi.reshape(-1), lo.reshape(-1)
    return np.stack([lo, (lo * 43 + hi * 21 + 32) // 64, (lo * 21 + hi * 43 + 32) // 64, hi], -1)


@functools.lru_cache(maxsize=None)
def bc7_color_table():
    """[inten][base5][range][mapping] -> lo | hi << 8 | min(err, 65535) << 16, the ETC1S -> BC7 mode 5 colour look-up: 7-bit endpoints, expanded (c << 1) | (c >> 6).
    As endpoint_table() (hi outermost, lo innermost, first minimum), except that the widest intensity table over the whole selector range counts the errors of
    selectors 0 and 3 five times: there the two clamp to 0 or 255 and the block is about those."""
    v = np.arange(128)
    colors = bc7_values((v << 1) | (v >> 6)).astype(np.int32)
    base = expand(5)
    out = np.zeros((8, 32, len(RANGES), len(MAPPINGS)), np.uint32)
    for t in range(8):
        block = np.clip(base[:, None] + INTEN[t][None, :], 0, 255).astype(np.int32)
        sq = {(s, k): (block[:, s][:, None] - colors[:, k][None, :]) ** 2 for s in range(4) for k in range(4)}   # (32, 16384) each
        for r, (s0, s1) in enumerate(RANGES):
            five = t == 7 and (s0, s1) == (0, 3)
            for m, mapping in enumerate(MAPPINGS):
                err = sum(sq[s, mapping[s]] * (5 if five and s in (0, 3) else 1) for s in range(s0, s1 + 1))
                best = err.argmin(1)
                out[t, :, r, m] = (best % 128) | ((best // 128) << 8) | (np.minimum(err[np.arange(32), best], 0xFFFF) << 16)
    return out.reshape(-1)


@functools.lru_cache(maxsize=None)
def bc7_alpha_table():
    """[inten][base5][range] -> lo | hi << 8 | trans << 16, the ETC1S -> BC7 mode 5 alpha look-up: 8-bit endpoints, hi outermost, lo innermost, first minimum; each
    in-range selector goes to its nearest of the four values (first minimum), its 2-bit index at bits 2 s of trans; same five-fold weight as the colour table."""
    rows, trans = nearest_value_table(bc7_values(np.arange(256)), RANGES, 2, True)
    return ((rows % 256) | ((rows // 256) << 8) | (trans << 16)).astype(np.uint32).reshape(-1)


@functools.lru_cache(maxsize=None)
def bc7_solid_table():
    """[value] {hi, lo}: the 7-bit endpoints whose index-1 colour (21/64 of the way from lo to hi) is nearest the value: lo outermost, hi innermost, first minimum"""
    v = np.arange(128)
    e = (v << 1) | (v >> 6)
    lo, hi = np.meshgrid(e, e, indexing="ij")
    c1 = ((lo * 43 + hi * 21 + 32) >> 6).reshape(-1)
    out = np.zeros((256, 2), np.uint8)
    for i in range(256):
        k = int(np.abs(c1 - i).argmin())
        out[i] = (k % 128, k // 128)
    return out.reshape(-1)


# ---------------------------------------------------------------- EAC R11 and ASTC 4x4 (the third entry family, etc1s_block_format_targets.h)

def eac_r11_values():
    """(256 * 16 * 16, 8): the eight 11-bit values of an EAC R11 block, row (base * 16 + multiplier) * 16 + table: clamp(base * 8 + 4 + modifier * multiplier * 8, 0,
    2047); multiplier 0 acts as 1/8 (the modifier itself is added)."""
    base, mul, table = np.meshgrid(np.arange(256), np.arange(16), np.arange(16), indexing="ij")
    step = np.where(mul == 0, 1, mul * 8).reshape(-1, 1)
    return np.clip(base.reshape(-1, 1) * 8 + 4 + step * EAC_MODIFIERS[table.reshape(-1)], 0, 2047)


@functools.lru_cache(maxsize=None)
def eac_r11_table():
    """[inten][base5][range] -> base | (table | multiplier << 4) << 8 | trans << 16, the ETC1S -> EAC R11 look-up, laid out as eac_a8_table(). An 8-bit colour p stands
    for the 11-bit value (p * 2047 + 128) / 255. Search order: base 0..255 outermost, multiplier 0..15, table innermost; each in-range selector on its nearest of the
    eight values (first minimum), squared 11-bit differences summed, first minimum overall -- the loop order of the reference's generator. The ranges are EAC A8's."""
    rows, trans = nearest_value_table(eac_r11_values(), ALPHA_RANGES, 3, False, lambda c: (c * 2047 + 128) // 255)
    base, mul, table = rows // 256, (rows // 16) % 16, rows % 16
    return (base | ((table | mul << 4) << 8) | (trans << 16)).astype(np.uint32).reshape(-1)


def astc_unquant48():
    """[BISE code of range 0..47: four bits, then a trit] -> the 8-bit endpoint value, by the format's unquantisation formula for one trit and four bits
    (A = the lowest bit replicated nine times, B = the other three bits b at b | b << 6, C = 22: ((trit * C + B) ^ A) >> 2, bit 7 from A)"""
    out = np.zeros(48, np.int64)
    for trit in range(3):
        for bit in range(16):
            a = 511 if bit & 1 else 0
            b = (bit >> 1) | ((bit >> 1) << 6)
            out[bit | (trit << 4)] = (a & 0x80) | (((trit * 22 + b) ^ a) >> 2)
    return out


def astc_values(e):
    """(n * n, 4): the four values of an ASTC 2-bit weight between endpoints hi (outer) and lo (inner) of the unquantised 8-bit values e: both replicated to 16 bits,
    ((c0 * (64 - w) + c1 * w + 32) / 64) >> 8 for the weights 0, 21, 43, 64"""
    hi, lo = np.meshgrid(e, e, indexing="ij")
    c1, c0 = (hi | (hi << 8)).reshape(-1), (lo | (lo << 8)).reshape(-1)
    return np.stack([((c0 * (64 - w) + c1 * w + 32) // 64) >> 8 for w in (0, 21, 43, 64)], -1)


def astc_scaled_errors(raw):
    """(..., 10) raw errors of an entry's ten mappings -> what the table holds: as they are while the largest of the ten fits 16 bits, else each times 65535 over
    that largest, rounded to nearest (halves up) -- so the largest becomes 65535 and the order among the ten is kept where a plain clamp would lose it"""
    raw = np.asarray(raw, np.int64)
    top = raw.max(-1, keepdims=True)
    return np.where(top > 0xFFFF, (2 * raw * 0xFFFF + top) // (2 * np.maximum(top, 1)), raw)


def astc_endpoint_table(e, scaled=True):
    """[inten][base5][range][mapping] -> lo | hi << 8 | err << 16 over the endpoint values e, lo and hi being indices into e (BISE codes for the 0..47 table, the
    values themselves for 0..255). The selector ranges (RANGES) and the ten mappings (MAPPINGS) are BC1's, in that order. hi outermost, lo innermost, first minimum;
    squared error over the range's selectors, those of selectors 0 and 3 counted eight times for the widest intensity table over the range (0, 3); the ten errors
    of an entry are stored through astc_scaled_errors() (scaled=False: each clamped to 65535 instead -- NOT what the reference's tables hold; the golden generator
    uses it to find the blocks that tell the two rules apart)."""
    n = e.size
    colors = astc_values(e).astype(np.int32)
    base = expand(5)
    out = np.zeros((8, 32, len(RANGES), len(MAPPINGS)), np.uint32)
    pairs = sorted({(s, mapping[s]) for mapping in MAPPINGS for s in range(4)})
    for t in range(8):
        block = np.clip(base[:, None] + INTEN[t][None, :], 0, 255).astype(np.int32)
        sq = {(s, k): (block[:, s][:, None] - colors[:, k][None, :]) ** 2 for s, k in pairs}   # (32, n * n) each
        for r, (s0, s1) in enumerate(RANGES):
            eight = t == 7 and (s0, s1) == (0, 3)
            raw = np.zeros((32, len(MAPPINGS)), np.int64)
            for m, mapping in enumerate(MAPPINGS):
                err = sum(sq[s, mapping[s]] * (8 if eight and s in (0, 3) else 1) for s in range(s0, s1 + 1))
                best = err.argmin(1)
                raw[:, m] = err[np.arange(32), best]
                out[t, :, r, m] = (best % n) | ((best // n) << 8)
            stored = astc_scaled_errors(raw) if scaled else np.minimum(raw, 0xFFFF)
            assert stored.max() <= 0xFFFF
            out[t, :, r, :] |= (stored << 16).astype(np.uint32)
    return out.reshape(-1)


@functools.lru_cache(maxsize=None)
def astc_table_0_47():
    """the ETC1S -> ASTC look-up over the 48 BISE codes of endpoint range 0..47, searched in code order"""
    return astc_endpoint_table(astc_unquant48())


@functools.lru_cache(maxsize=None)
def astc_table_0_255():
    """the same over 8-bit endpoints (the higher-quality opaque and grey routes); 256 x 256 pairs per entry, a few seconds"""
    return astc_endpoint_table(np.arange(256))


def astc_table_0_255_entries(t, base5, r):
    """the ten entries [inten t][base5][range r][mapping] of astc_table_0_255() by the same search, for checks that cannot afford the whole table"""
    colors = astc_values(np.arange(256)).astype(np.int64)
    block = np.clip(int(expand(5)[base5]) + INTEN[t], 0, 255)
    s0, s1 = RANGES[r]
    eight = t == 7 and (s0, s1) == (0, 3)
    best, raw = [], []
    for mapping in MAPPINGS:
        err = sum((int(block[s]) - colors[:, mapping[s]]) ** 2 * (8 if eight and s in (0, 3) else 1) for s in range(s0, s1 + 1))
        best.append(int(err.argmin()))
        raw.append(int(err[best[-1]]))
    return np.array([(b % 256) | ((b // 256) << 8) | (int(v) << 16) for b, v in zip(best, astc_scaled_errors(raw))], np.uint32)


def astc_best_grey_mapping(table):
    """[inten][base5][range] -> the mapping of the ten with the least error in an endpoint table, first on ties: what a one-channel (grey or alpha) conversion uses"""
    return (table.reshape(8, 32, len(RANGES), len(MAPPINGS)) >> 16).argmin(3).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def astc_solid_table():
    """[value] {lo, hi}: the BISE codes of range 0..47 whose weight-21 value is nearest the value: lo outermost, hi innermost over the codes in order, first minimum"""
    u = astc_unquant48()
    lo, hi = np.meshgrid(u, u, indexing="ij")
    l16, h16 = (lo | (lo << 8)).reshape(-1), (hi | (hi << 8)).reshape(-1)
    v = ((l16 * 43 + h16 * 21 + 32) // 64) >> 8
    out = np.zeros((256, 2), np.uint8)
    for i in range(256):
        k = int(np.abs(v - i).argmin())
        out[i] = (k // 48, k % 48)
    return out.reshape(-1)


@functools.lru_cache(maxsize=None)
def astc_nearest_table():
    """[value] -> the BISE code of range 0..47 whose unquantised value is nearest, first on ties in code order"""
    u = astc_unquant48()
    return np.array([int(np.abs(u - i).argmin()) for i in range(256)], np.uint8)


# ---------------------------------------------------------------- ATC RGB, PVRTC2 4bpp and FXT1 (the fourth entry family, etc1s_vendor_format_targets.h)

def expand4_via5():
    """PVRTC2's 4-bit blue of the low colour: to 5 bits by (c << 1) | (c >> 3), then to 8 like any 5-bit value"""
    v = np.arange(16)
    v = (v << 1) | (v >> 3)
    return (v << 3) | (v >> 2)


ATC_EXPANSIONS = {"55": (expand(5), expand(5)), "56": (expand(5), expand(6)), "45": (expand4_via5(), expand(5))}   # (low endpoint, high endpoint) of the three look-ups


@functools.lru_cache(maxsize=None)
def atc_endpoint_table(which):
    """[inten][base5][range][mapping] -> lo | hi << 8 | min(err, 65535) << 16, the ETC1S -> ATC / PVRTC2 look-ups "55", "56" and "45": the low and the high endpoint
    have their own widths (ATC_EXPANSIONS). The four values are c0 = lo, c3 = hi, c1 = (5 c0 + 3 c3) / 8, c2 = (5 c3 + 3 c0) / 8 by integer division. The search is
    endpoint_table()'s -- hi outermost, lo innermost, first minimum over the range's selectors -- with the errors of selectors 0 and 3 counted five times for the
    widest intensity table over the range (0, 3), as in bc7_color_table()."""
    e_lo, e_hi = ATC_EXPANSIONS[which]
    hi, lo = np.meshgrid(e_hi, e_lo, indexing="ij")   # axis 0 = hi (outer), axis 1 = lo (inner)
    hi, lo = hi.reshape(-1), lo.reshape(-1)
    colors = np.stack([lo, (lo * 5 + hi * 3) // 8, (hi * 5 + lo * 3) // 8, hi], -1).astype(np.int64)
    n_lo = e_lo.size
    base = expand(5)
    out = np.zeros((8, 32, len(RANGES), len(MAPPINGS)), np.uint32)
    for t in range(8):
        block = np.clip(base[:, None] + INTEN[t][None, :], 0, 255).astype(np.int64)
        for r, (s0, s1) in enumerate(RANGES):
            five = t == 7 and (s0, s1) == (0, 3)
            for m, mapping in enumerate(MAPPINGS):
                err = sum((block[:, s][:, None] - colors[:, mapping[s]][None, :]) ** 2 * (5 if five and s in (0, 3) else 1) for s in range(s0, s1 + 1))
                best = err.argmin(1)
                out[t, :, r, m] = (best % n_lo) | ((best // n_lo) << 8) | (np.minimum(err[np.arange(32), best], 0xFFFF) << 16)
    return out.reshape(-1)


def atc_solid_table(which):
    """[value] {lo, hi}: the endpoints of look-up `which` whose value 1, (5 lo + 3 hi) / 8, is nearest the value: lo outermost, hi innermost, first minimum"""
    e_lo, e_hi = ATC_EXPANSIONS[which]
    lo, hi = np.meshgrid(e_lo, e_hi, indexing="ij")
    c1 = ((lo * 5 + hi * 3) // 8).reshape(-1)
    out = np.zeros((256, 2), np.uint8)
    for i in range(256):
        k = int(np.abs(c1 - i).argmin())
        out[i] = (k // e_hi.size, k % e_hi.size)
    return out.reshape(-1)


def atc_nearest_table(e):
    """[value] -> the endpoint of the expanded values e nearest the value, first on ties"""
    return np.array([int(np.abs(e - i).argmin()) for i in range(256)], np.uint8)


# PVRTC2 4bpp RGBA (translucent mode: colour a 4433 with alpha (a << 1) expanded 4 -> 8 bits by replication, colour b 4443 with alpha (a << 1) | 1)

def pvrtc2_alpha_a():
    v = np.arange(8) << 1
    return (v << 4) | v


def pvrtc2_alpha_b():
    v = (np.arange(8) << 1) | 1
    return (v << 4) | v


def expand3_via5():
    """the 3-bit blue of translucent colour a: to 5 bits by (c << 2) | (c >> 1), then to 8"""
    v = np.arange(8)
    v = (v << 2) | (v >> 1)
    return (v << 3) | (v >> 2)


def pvrtc2_match_table(e_lo, e_hi):
    """[value] {l, h}: the endpoints whose value 1, (5 l + 3 h) / 8, is nearest the value: l outermost, h innermost, first minimum (transcoder_init_pvrtc2)"""
    lo, hi = np.meshgrid(e_lo, e_hi, indexing="ij")
    m = ((lo * 5 + hi * 3) // 8).reshape(-1)
    out = np.zeros((256, 2), np.uint8)
    for i in range(256):
        k = int(np.abs(m - i).argmin())
        out[i] = (k // e_hi.size, k % e_hi.size)
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
    alpha_range_index = np.zeros((4, 4), np.uint8)
    for i, (a, b) in enumerate(ALPHA_RANGES):
        alpha_range_index[a, b] = i
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
        "// Tables of the ETC1S -> EAC A8 and ETC1S -> BC7 mode 5 block conversions. The selector ranges and mappings of BC7 are BC1's above. The BC7 colour look-up",
        "// (15,360 entries) is not here: etc1s_build_bc7_tables_kernel computes it on the device, bc7_color_table() of the tool is the same search on the host.",
        emit("ke_alpha_range_index", "unsigned char", alpha_range_index.reshape(-1), 16, "[lowest selector][highest selector] -> selector range of the EAC A8 look-up; a range it does not have reads entry 0", "%u"),
        emit("ke_eac_a8", "unsigned int", eac_a8_table(), 8, "[inten][base5][range] -> base | (table | multiplier << 4) << 8 | 3-bit code of selector s << (16 + 3 s)", "0x%07x"),
        emit("ke_bc7_alpha", "unsigned int", bc7_alpha_table(), 8, "[inten][base5][range] -> lo | hi << 8 | 2-bit index of selector s << (16 + 2 s)", "0x%06x"),
        emit("ke_bc7_solid", "unsigned char", bc7_solid_table(), 32, "[value] {hi, lo}: 7-bit endpoints whose index-1 colour is nearest the value", "%3u"),
        "// Tables of the ETC1S -> EAC R11 and ETC1S -> ASTC 4x4 block conversions. EAC R11 uses EAC A8's selector ranges, ASTC the ranges and mappings of BC1. The two ASTC",
        "// endpoint look-ups (15,360 entries each) are not here: etc1s_build_astc_tables_kernel computes them on the device, astc_table_0_47() and astc_table_0_255() of the",
        "// tool are the same searches on the host.",
        emit("ke_eac_r11", "unsigned int", eac_r11_table(), 8, "[inten][base5][range] -> base | (table | multiplier << 4) << 8 | 3-bit code of selector s << (16 + 3 s)", "0x%07x"),
        emit("ke_astc_solid", "unsigned char", astc_solid_table(), 32, "[value] {lo, hi}: BISE codes of range 0..47 whose weight-21 value is nearest the value", "%2u"),
        emit("ke_astc_nearest", "unsigned char", astc_nearest_table(), 32, "[value]: the BISE code of range 0..47 nearest the value", "%2u"),
        "// Tables of the ETC1S -> ATC RGB and ETC1S -> PVRTC2 4bpp RGB block conversions (FXT1 goes through BC1's above). The ranges and mappings are BC1's. The three",
        "// endpoint look-ups 55 / 56 / 45 (15,360 entries each) are not here: etc1s_build_atc_tables_kernel computes them on the device, atc_endpoint_table() of the tool is",
        "// the same search on the host.",
        emit("ke_atc_solid55", "unsigned char", atc_solid_table("55"), 32, "[value] {lo, hi}: 5-bit endpoints whose value 1, (5 lo + 3 hi) / 8, is nearest the value", "%2u"),
        emit("ke_atc_solid56", "unsigned char", atc_solid_table("56"), 32, "the same, 5-bit low and 6-bit high endpoint", "%2u"),
        emit("ke_atc_solid45", "unsigned char", atc_solid_table("45"), 32, "the same, PVRTC2's 4-bit low and 5-bit high endpoint", "%2u"),
        emit("ke_atc_end4", "unsigned char", atc_nearest_table(expand4_via5()), 32, "[value]: PVRTC2's 4-bit endpoint nearest the value", "%2u"),
        emit("ke_atc_end5", "unsigned char", atc_nearest_table(expand(5)), 32, "the same, 5-bit", "%2u"),
        emit("ke_atc_end6", "unsigned char", atc_nearest_table(expand(6)), 32, "the same, 6-bit", "%2u"),
        "// Tables of the constant blocks of ETC1S -> PVRTC2 4bpp RGBA: colour a is 4433 with alpha (a << 1), colour b 4443 with alpha (a << 1) | 1, alpha to 8 bits by replication.",
        emit("ke_pvrtc2_alpha33", "unsigned char", pvrtc2_match_table(pvrtc2_alpha_a(), pvrtc2_alpha_b()), 32, "[value] {l, h}: the 3-bit alphas whose value 1, (5 l + 3 h) / 8, is nearest the value", "%u"),
        emit("ke_pvrtc2_alpha33_0", "unsigned char", atc_nearest_table(pvrtc2_alpha_a()), 32, "[value]: the 3-bit alpha of colour a nearest the value", "%u"),
        emit("ke_pvrtc2_alpha33_3", "unsigned char", atc_nearest_table(pvrtc2_alpha_b()), 32, "[value]: the 3-bit alpha of colour b nearest the value", "%u"),
        emit("ke_pvrtc2_trans34", "unsigned char", pvrtc2_match_table(expand3_via5(), expand4_via5()), 32, "[value] {l, h}: blue of 3 and 4 bits whose value 1 is nearest the value", "%2u"),
        emit("ke_pvrtc2_trans44", "unsigned char", pvrtc2_match_table(expand4_via5(), expand4_via5()), 32, "[value] {l, h}: red / green of 4 and 4 bits whose value 1 is nearest the value", "%2u"),
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
