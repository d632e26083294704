"""What the ETC1S block-format tests share: the golden file (tests/golden/etc1s_block_format_vectors.npz, written by tools/gen_golden_etc1s_block_format.py) and a
plain restatement on the CPU of the three conversions the third entry family adds -- ASTC 4x4, EAC R11, EAC RG11 -- over the look-ups that
tools/gen_etc1s_transcode_tables.py computes. A block is built as a Python int of 128 bits, field by field at the bit positions the format gives, so nothing here
shares the device code's two-halves-and-bit-tricks structure. The generator accepts its npz only after this restatement has reproduced every block in it; the host
tests repeat that, and the GPU tests compare the kernels with the goldens and with this."""
import functools
import pathlib
import sys

import numpy as np

import etc1s_texture_helpers as X
import native_libs

GOLDEN = pathlib.Path(__file__).resolve().parent / "golden" / "etc1s_block_format_vectors.npz"
ASTC_4x4_RGBA, ETC2_EAC_R11, ETC2_EAC_RG11 = 10, 20, 21
TAGS = {"astc": "ASTC_LDR_4X4_RGBA", "r11": "ETC2_EAC_R11", "rg11": "ETC2_EAC_RG11"}   # npz key suffix -> the reference tool's file tag
TARGETS = {"astc": ASTC_4x4_RGBA, "r11": ETC2_EAC_R11, "rg11": ETC2_EAC_RG11}
RANGES, ALPHA_RANGES, MAPPINGS = X.RANGES, X.ALPHA_RANGES, X.MAPPINGS
WEIGHTS = (0, 21, 43, 64)
ROUTES = ("void", "btc", "grey", "rgb", "rgba")   # the five routes of the ASTC conversion, in the order they are tried


@functools.lru_cache(maxsize=None)
def golden():
    return native_libs.load_npz_golden(GOLDEN)


def _tool():
    sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent.parent / "tools"))
    import gen_etc1s_transcode_tables as G
    return G


class Tables:
    """the host statements of the look-ups (tools/gen_etc1s_transcode_tables.py), computed once; the 0..255 ASTC table takes a few seconds. reached255 collects which
    (intensity table, base, range) rows of it the restatement has read."""

    def __init__(self):
        G = self.G = _tool()
        self.unquant = [int(v) for v in G.astc_unquant48()]
        self.table47 = G.astc_table_0_47().reshape(8, 32, 6, 10)
        self.whole255 = G.astc_table_0_255().reshape(8, 32, 6, 10)
        self.solid = G.astc_solid_table().reshape(256, 2)
        self.nearest = G.astc_nearest_table()
        self.r11 = G.eac_r11_table().reshape(8, 32, 4)
        self.trits = trit_encode_table()
        self.reached255 = set()

    def table255(self, t, base5, r):
        self.reached255.add((t, base5, r))
        return self.whole255[t, base5, r]


@functools.lru_cache(maxsize=None)
def tables():
    return Tables()


@functools.lru_cache(maxsize=None)
def trit_encode_table():
    """[t0 + 3 t1 + 9 t2 + 27 t3 + 81 t4] -> the 8 bits T that the format's trit decoding takes apart into those five trits; the lowest T where two decode alike"""
    out = {}
    for T in range(256):
        b = [(T >> k) & 1 for k in range(8)]
        if (b[2], b[3], b[4]) == (1, 1, 1):
            C = (b[7] << 4) | (b[6] << 3) | (b[5] << 2) | (b[1] << 1) | b[0]
            t4 = t3 = 2
        else:
            C = T & 31
            if (b[5], b[6]) == (1, 1):
                t4, t3 = 2, b[7]
            else:
                t4, t3 = b[7], (b[6] << 1) | b[5]
        c = [(C >> k) & 1 for k in range(5)]
        if (c[0], c[1]) == (1, 1):
            t2, t1, t0 = 2, c[4], (c[3] << 1) | (c[2] & ~c[3] & 1)
        elif (c[2], c[3]) == (1, 1):
            t2, t1, t0 = 2, 2, (c[1] << 1) | c[0]
        else:
            t2, t1, t0 = c[4], (c[3] << 1) | c[2], (c[1] << 1) | (c[0] & ~c[1] & 1)
        if max(t0, t1, t2, t3, t4) <= 2:
            out.setdefault(t0 + 3 * t1 + 9 * t2 + 27 * t3 + 81 * t4, T)
    assert sorted(out) == list(range(243))
    return [out[k] for k in range(243)]


# ---------------------------------------------------------------- EAC R11 / RG11

OPAQUE_EAC = X.OPAQUE_EAC_A8   # base 255, table 13, multiplier 1, every code 4


def eac_r11_block(t, e, sel):
    """8 bytes: EAC A8's layout over the R11 look-up, on the first channel"""
    lo, hi = int(sel.min()), int(sel.max())
    if lo == hi:
        base, table, mul, code = int(X.block_colors(e)[lo, 0]), 13, 1, [4, 4, 4, 4]
    else:
        v = int(t.r11[int(e[3]), int(e[0]), ALPHA_RANGES.index((lo, hi)) if (lo, hi) in ALPHA_RANGES else 0])
        base, table, mul, code = v & 255, (v >> 8) & 15, (v >> 12) & 15, [(v >> (16 + 3 * s)) & 7 for s in range(4)]
    bits = 0
    for y in range(4):
        for x in range(4):
            bits |= code[int(sel[y * 4 + x])] << (45 - 3 * (x * 4 + y))
    return [base, table | (mul << 4)] + [(bits >> (8 * (5 - k))) & 255 for k in range(6)]


# ---------------------------------------------------------------- ASTC 4x4

def _rev2(w):
    return ((w & 1) << 1) | (w >> 1)


def _put_weights(block, weights, bits):
    """weights from the top of the block down, each with its bits reversed"""
    at = 128
    for w in weights:
        at -= bits
        block |= (_rev2(w) if bits == 2 else w) << at
    return block


def _header(block_bytes):
    return int.from_bytes(bytes(block_bytes), "little")


def _plane(t, e, sel, table_of):
    """one channel's endpoints and weights through a look-up: the ten entries of (table, green base, range), the first least error of them"""
    lo, hi = int(sel.min()), int(sel.max())
    rows = table_of(int(e[3]), int(e[1]), RANGES.index((lo, hi)))
    m = int((rows >> 16).argmin())
    return int(rows[m]) & 255, (int(rows[m]) >> 8) & 255, [MAPPINGS[m][int(s)] for s in sel]


def astc_block(t, e, sel, ae=None, asel=None):
    """-> (the 16 bytes as an int, route, detail). e / ae: (r5, g5, b5, table) of the colour / alpha slice's block, sel / asel their 16 selectors; ae None = no alpha
    slice. detail says which sub-routes and table entries the block took (the coverage counts are made of it)."""
    e = [int(v) for v in e]
    sel = [int(s) for s in sel]
    used = sorted(set(sel))
    low, high, n = used[0], used[-1], len(used)
    colors = X.block_colors(e)
    has_alpha = ae is not None
    a_n, constant_alpha = 1, 255
    if has_alpha:
        ae, asel = [int(v) for v in ae], [int(s) for s in asel]
        a_used = sorted(set(asel))
        a_low, a_high, a_n = a_used[0], a_used[-1], len(a_used)
        a_values = [int(v) for v in X.block_colors(ae)[:, 1]]
        if a_n == 1:
            constant_alpha = a_values[a_low]
    if n == 1 and a_n == 1:
        block = _header([0xFC, 0xFD, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF])
        for k, v in enumerate([int(c) for c in colors[low]] + [constant_alpha]):
            block |= (v | (v << 8)) << (64 + 16 * k)
        return block, "void", {"color": tuple(int(c) for c in colors[low]), "alpha": constant_alpha}
    if n <= 2 and a_n <= 2:
        c0, c1 = [int(v) for v in colors[low]], [int(v) for v in colors[high]]
        invert = sum(c1) < sum(c0)
        if invert:
            c0, c1 = c1, c0
        a0, a1 = (a_values[a_low], a_values[a_high]) if has_alpha else (255, 255)
        block = _header([0x41, 0x84, 0x01, 0x00, 0, 0, 0, 0, 0, 0, 0, 0xC0])
        for k, v in enumerate([c0[0], c1[0], c0[1], c1[1], c0[2], c1[2], a0, a1]):
            block |= v << (17 + 8 * k)
        weights = []
        for p in range(16):
            weights += [int(sel[p] == high) ^ int(invert), int(asel[p] == a_high) if has_alpha else 0]
        return _put_weights(block, weights, 1), "btc", {"pair": (low, high), "swapped": invert, "alpha_pair": (a_low, a_high) if has_alpha else None}
    detail = {}
    if e[0] == e[1] == e[2]:
        def grey_plane(pe, psel, what):
            u = sorted(set(psel))
            values = [int(v) for v in X.block_colors(pe)[:, 1]]
            if len(u) <= 2:
                return values[u[0]], values[u[-1]], [3 if s == u[-1] else 0 for s in psel]
            detail[what] = (pe[3], pe[1], RANGES.index((u[0], u[-1])))
            return _plane(t, pe, np.array(psel), t.table255)
        l, h, wc = grey_plane(e, sel, "grey255")
        al, ah, wa = grey_plane(ae, asel, "alpha255") if has_alpha else (255, 255, [0] * 16)
        block = _header([0x42, 0x84, 0x00, 0x00, 0, 0, 0, 0xC0])
        for k, v in enumerate([l, h, al, ah]):
            block |= v << (17 + 8 * k)
        return _put_weights(block, [w for p in range(16) for w in (wc[p], wa[p])], 2), "grey", detail

    def color_lookup(table_of):
        r = RANGES.index((low, high))
        rows = [table_of(e[3], e[c], r) for c in range(3)]
        m = int(sum((row >> 16).astype(np.int64) for row in rows).argmin())
        return [int(row[m]) & 255 for row in rows], [(int(row[m]) >> 8) & 255 for row in rows], m, r
    if a_n == 1 and constant_alpha == 255:
        l, h, m, r = color_lookup(t.table255)
        invert = sum(h) < sum(l)
        if invert:
            l, h = h, l
        block = _header([0x42, 0x00, 0x01, 0x00])
        for k, v in enumerate([l[0], h[0], l[1], h[1], l[2], h[2]]):
            block |= v << (17 + 8 * k)
        weights = [MAPPINGS[m][s] ^ (3 if invert else 0) for s in sel]
        return _put_weights(block, weights, 2), "rgb", {"color": (e[3], r, m), "swapped": invert}
    # RGBA over BISE codes of range 0..47
    if not has_alpha:
        al, ah, wa = 1, 1, [0] * 16
        detail["alpha"] = "none"
    elif a_n == 1:
        (al, ah), wa = (int(v) for v in t.solid[constant_alpha]), [1] * 16
        detail["alpha"] = "solid"
    elif ae[3] == 7 and a_n == 2 and (a_low, a_high) == (0, 3):
        al, ah, wa = int(t.nearest[a_values[0]]), int(t.nearest[a_values[3]]), [3 if s == 3 else 0 for s in asel]
        detail["alpha"] = "outlier"
    else:
        al, ah, wa = _plane(t, ae, np.array(asel), lambda a, b, c: t.table47[a, b, c])
        detail["alpha"] = "lookup"
        detail["alpha47"] = (ae[3], ae[1], RANGES.index((a_low, a_high)))
    if n == 1:
        c = [int(v) for v in colors[low]]
        l, h, wc = [int(t.solid[v, 0]) for v in c], [int(t.solid[v, 1]) for v in c], [1] * 16
        detail["color"] = "solid"
        detail["solid_values"] = tuple(c)
    elif e[3] == 7 and n == 2 and (low, high) == (0, 3):
        l, h = [int(t.nearest[int(v)]) for v in colors[0]], [int(t.nearest[int(v)]) for v in colors[3]]
        wc = [3 if s == 3 else 0 for s in sel]
        detail["color"] = "outlier"
    else:
        l, h, m, r = color_lookup(lambda a, b, c: t.table47[a, b, c])
        wc = [MAPPINGS[m][s] for s in sel]
        detail["color"] = "lookup"
        detail["color47"] = (e[3], r, m)
    invert = sum(t.unquant[v] for v in h) < sum(t.unquant[v] for v in l)
    if invert:
        l, h, wc = h, l, [3 - w for w in wc]
    detail["swapped"] = invert
    block = _header([0x42, 0x84, 0x01, 0x00, 0, 0, 0, 0xC0])
    at = 17
    values = [l[0], h[0], l[1], h[1], l[2], h[2], al, ah, 0, 0]
    for g in range(2):   # two groups of five values: four bits each, and the five trits as one 8-bit block T, interleaved m0 T0-1 m1 T2-3 m2 T4 m3 T5-6 m4 T7
        v = values[5 * g:5 * g + 5]
        T = t.trits[sum((v[i] >> 4) * 3 ** i for i in range(5))]
        for field, width in ((v[0] & 15, 4), (T & 3, 2), (v[1] & 15, 4), ((T >> 2) & 3, 2), (v[2] & 15, 4), ((T >> 4) & 1, 1), (v[3] & 15, 4), ((T >> 5) & 3, 2), (v[4] & 15, 4),
                             (T >> 7, 1)):
            block |= field << at
            at += width
    return _put_weights(block, [w for p in range(16) for w in (wc[p], wa[p])], 2), "rgba", detail


def blocks(decoded, image, target, routes=None, details=None, t=None):
    """(n, 8 | 16) u8: what the transcoder writes for ASTC_4x4_RGBA, ETC2_EAC_R11 or ETC2_EAC_RG11. routes: a dict that receives how many ASTC blocks took each
    route; details: a list that receives (route, detail) per ASTC block."""
    t = t or tables()
    ep, sel = np.asarray(decoded["endpoint_palette"]), X.selectors16(decoded["selector_palette"])
    ei, si = image["endpoint_indices"].reshape(-1), image["selector_indices"].reshape(-1)
    alpha = image["alpha_endpoint_indices"] is not None
    aei, asi = (image["alpha_endpoint_indices"].reshape(-1), image["alpha_selector_indices"].reshape(-1)) if alpha else (None, None)
    out = np.zeros((ei.size, 8 if target == ETC2_EAC_R11 else 16), np.uint8)
    cache = {}
    for k in range(ei.size):
        key = (int(ei[k]), int(si[k])) + ((int(aei[k]), int(asi[k])) if alpha and target != ETC2_EAC_R11 else ())
        if key not in cache:
            if target == ASTC_4x4_RGBA:
                block, route, detail = astc_block(t, ep[key[0]], sel[key[1]], ep[key[2]] if alpha else None, sel[key[3]] if alpha else None)
                cache[key] = (list(block.to_bytes(16, "little")), route, detail)
            else:
                red = eac_r11_block(t, ep[key[0]], sel[key[1]])
                if target == ETC2_EAC_RG11:
                    red = red + (eac_r11_block(t, ep[key[2]], sel[key[3]]) if alpha else OPAQUE_EAC)
                cache[key] = (red, None, None)
        out[k], route, detail = cache[key]
        if route is not None:
            if routes is not None:
                routes[route] = routes.get(route, 0) + 1
            if details is not None:
                details.append((route, detail))
    return out


# ---------------------------------------------------------------- a decoder of the two lossless layouts, from the format

def decode_astc_lossless(block16):
    """16 bytes -> (16, 4) texels for exactly two layouts: a void-extent block (the 16-bit constants' top bytes) and the one-partition, two-plane block of CEM 12 with
    8-bit endpoints and 1-bit weights (a weight of 1 bit selects an endpoint outright). None for anything else."""
    v = int.from_bytes(bytes(block16), "little")
    if v & 0x1FF == 0x1FC:   # void extent: bits 0-8 all but bit 1, bit 9 clear = LDR; four 16-bit constants from bit 64
        if (v >> 9) & 1 or (v >> 10) & ((1 << 54) - 1) != (1 << 54) - 1:   # LDR; the two reserved bits and the four 13-bit extent coordinates all ones
            return None
        return np.array([[(v >> (64 + 16 * k + 8)) & 255 for k in range(4)]] * 16, np.uint8)
    mode = v & 0x7FF
    # block mode 0x441: bits 0-1 = 01 and bits 2-3 = 00 -> the layout "width B + 4, height A + 2" with A = bits 5-6 = 2, B = bits 7-8 = 0: a 4x4 grid; weight range
    # bits R0 = bit 4 = 0, R1 R2 = bits 0-1 = 1 0 -> R = 2 with H = bit 9 = 0: two levels, one bit; D = bit 10 = 1: two planes
    if mode != 0x441 or (v >> 11) & 3 != 0 or (v >> 13) & 15 != 12:   # one partition, CEM 12
        return None
    if (v >> 94) & 3 != 3:   # the second plane's channel, just under the 32 weight bits: alpha
        return None
    ends = [(v >> (17 + 8 * k)) & 255 for k in range(8)]
    r0, r1, g0, g1, b0, b1, a0, a1 = ends
    if r1 + g1 + b1 < r0 + g0 + b0:   # CEM 12 swaps the endpoints (blue contraction) when the second sum is smaller: the transcoder never writes that
        return None
    out = np.zeros((16, 4), np.uint8)
    for p in range(16):
        wc, wa = (v >> (127 - 2 * p)) & 1, (v >> (126 - 2 * p)) & 1
        out[p] = [r1 if wc else r0, g1 if wc else g0, b1 if wc else b0, a1 if wa else a0]
    return out
