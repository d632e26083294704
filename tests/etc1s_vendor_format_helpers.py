"""What the ETC1S vendor-format tests share: the golden file (tests/golden/etc1s_vendor_format_vectors.npz, written by tools/gen_golden_etc1s_vendor_format.py) and a
plain restatement on the CPU of the four conversions the fourth entry family adds -- ATC RGB, FXT1, PVRTC2 4bpp RGB and RGBA -- over the look-ups that
tools/gen_etc1s_transcode_tables.py computes. A block is built as a Python int, field by field at the bit positions the format gives, over lists of sixteen
selectors, so nothing here shares the device code's packed words. The generator accepts its npz only after this restatement has reproduced every block in it; the
host tests repeat that, and the GPU tests compare the kernels with the goldens and with this."""
import functools
import hashlib
import pathlib
import sys

import numpy as np

import etc1s_texture_helpers as X
import native_libs

GOLDEN = pathlib.Path(__file__).resolve().parent / "golden" / "etc1s_vendor_format_vectors.npz"
ATC_RGB, FXT1_RGB, PVRTC2_4_RGB, PVRTC2_4_RGBA = 11, 17, 18, 19
TAGS = {"atc": "ATC_RGB", "fxt1": "FXT1_RGB", "pvrtc2": "PVRTC2_4_RGB", "pvrtc2a": "PVRTC2_4_RGBA"}   # npz key suffix -> the reference tool's file tag
TARGETS = {"atc": ATC_RGB, "fxt1": FXT1_RGB, "pvrtc2": PVRTC2_4_RGB, "pvrtc2a": PVRTC2_4_RGBA}
UNIT = {"atc": 8, "fxt1": 16, "pvrtc2": 8, "pvrtc2a": 8}
RANGES, MAPPINGS = X.RANGES, X.MAPPINGS
ROUTES = ("solid", "outlier", "lookup")   # the three routes of every conversion here, in the order they are tried
# the gates that no file can reach, and why: what DESIGN 4t states. The one is in PVRTC2 RGBA; every branch of the integer targets is reached.
UNREACHABLE = {"pvrtc2a_err0_equals_err3": "the tie of the constant-block choice does not occur over every grey block colour against every alpha value below 250; which side wins it rests on the restatement alone"}


@functools.lru_cache(maxsize=None)
def golden():
    return native_libs.load_npz_golden(GOLDEN)


def _tool():
    sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent.parent / "tools"))
    import gen_etc1s_transcode_tables as G
    return G


class Tables:
    """the host statements of the look-ups (tools/gen_etc1s_transcode_tables.py), computed once"""

    def __init__(self):
        G = self.G = _tool()
        self.atc = {w: G.atc_endpoint_table(w).reshape(8, 32, 6, 10) for w in ("55", "56", "45")}
        self.solid = {w: G.atc_solid_table(w).reshape(256, 2) for w in ("55", "56", "45")}
        self.end = {4: G.atc_nearest_table(G.expand4_via5()), 5: G.atc_nearest_table(G.expand(5)), 6: G.atc_nearest_table(G.expand(6))}
        self.bc1 = {5: G.endpoint_table(5).reshape(8, 32, 6, 10), 6: G.endpoint_table(6).reshape(8, 32, 6, 10)}
        self.bc1_solid = {5: G.solid_table(5, 1).reshape(256, 2), 6: G.solid_table(6, 1).reshape(256, 2)}   # {hi, lo}
        self.bc1_end = {5: G.solid_table(5, 0)[0::2], 6: G.solid_table(6, 0)[0::2]}
        self.alpha33 = G.pvrtc2_match_table(G.pvrtc2_alpha_a(), G.pvrtc2_alpha_b()).reshape(256, 2)
        self.alpha33_0, self.alpha33_3 = G.atc_nearest_table(G.pvrtc2_alpha_a()), G.atc_nearest_table(G.pvrtc2_alpha_b())
        self.trans34 = G.pvrtc2_match_table(G.expand3_via5(), G.expand4_via5()).reshape(256, 2)
        self.trans44 = G.pvrtc2_match_table(G.expand4_via5(), G.expand4_via5()).reshape(256, 2)

    def digest(self):
        """of the three endpoint look-ups, 55 then 56 then 45, as little-endian words"""
        return hashlib.sha256(b"".join(np.ascontiguousarray(self.atc[w], "<u4").tobytes() for w in ("55", "56", "45"))).hexdigest()


@functools.lru_cache(maxsize=None)
def tables():
    return Tables()


def _use(sel):
    used = sorted(set(int(s) for s in sel))
    return used[0], used[-1], len(used)


def _best_mapping(rows):
    """the mapping with the least summed error over the three channels' rows of ten, first on ties"""
    total = [sum(int(row[m]) >> 16 for row in rows) for m in range(10)]
    return total.index(min(total))


# ---------------------------------------------------------------- ATC RGB and PVRTC2 4bpp RGB

def atc_solve(t, e, sel, widths):
    """-> (low [r, g, b], high [r, g, b], sixteen selectors, route, detail). widths: per channel which look-up it reads ("55", "56" or "45"), e.g. ATC ("55", "56",
    "55"). The low endpoint of "45" has four bits, the high endpoint of "56" six, every other five."""
    e, sel = [int(v) for v in e], [int(s) for s in sel]
    low, high, n = _use(sel)
    colors = X.block_colors(e)
    if n == 1:
        c = [int(v) for v in colors[low]]
        pairs = [t.solid[w][c[k]] for k, w in enumerate(widths)]
        return [int(p[0]) for p in pairs], [int(p[1]) for p in pairs], [1] * 16, "solid", {"values": tuple(c)}
    if e[3] == 7 and n == 2 and (low, high) == (0, 3):
        lo_bits = [4 if w == "45" else 5 for w in widths]
        hi_bits = [6 if w == "56" else 5 for w in widths]
        return ([int(t.end[lo_bits[k]][int(colors[0][k])]) for k in range(3)], [int(t.end[hi_bits[k]][int(colors[3][k])]) for k in range(3)], sel, "outlier", {})
    r = RANGES.index((low, high))
    rows = [t.atc[w][e[3], e[k], r] for k, w in enumerate(widths)]
    m = _best_mapping(rows)
    return ([int(row[m]) & 255 for row in rows], [(int(row[m]) >> 8) & 255 for row in rows], [MAPPINGS[m][s] for s in sel], "lookup", {"entry": (e[3], r, m)})


def _selector_bytes(sel):
    """sixteen 2-bit selectors -> four bytes, a byte per row, texel x of the row at bits 2 x"""
    return [sum(sel[y * 4 + x] << (2 * x) for x in range(4)) for y in range(4)]


def atc_block(t, e, sel):
    lo, hi, s, route, detail = atc_solve(t, e, sel, ("55", "56", "55"))
    low16, high16 = (lo[0] << 10) | (lo[1] << 5) | lo[2], (hi[0] << 11) | (hi[1] << 5) | hi[2]
    return [low16 & 255, low16 >> 8, high16 & 255, high16 >> 8] + _selector_bytes(s), route, detail


def pvrtc2_rgb_block(t, e, sel):
    """the modulation bytes, then the colour word: modulation flag 0, blue a (4 bits) from bit 1, green a 5, red a 10, hard flag 15, blue b 16, green b 21, red b 26,
    opaque flag 31"""
    lo, hi, s, route, detail = atc_solve(t, e, sel, ("55", "55", "45"))
    word = (lo[2] << 1) | (lo[1] << 5) | (lo[0] << 10) | (1 << 15) | (hi[2] << 16) | (hi[1] << 21) | (hi[0] << 26) | (1 << 31)
    return _selector_bytes(s) + list(word.to_bytes(4, "little")), route, detail


# ---------------------------------------------------------------- PVRTC2 4bpp RGBA

F = np.float32


def _x4(c):
    c = (c << 1) | (c >> 3)
    return (c << 3) | (c >> 2)


def _x3(c):
    c = (c << 2) | (c >> 1)
    return (c << 3) | (c >> 2)


def _trans_word(a, b):
    """colour a (r4, g4, b3, a3), colour b (r4, g4, b4, a3) -> the colour word of a hard translucent block"""
    return (a[2] << 1) | (a[1] << 4) | (a[0] << 8) | (a[3] << 12) | (1 << 15) | (b[2] << 16) | (b[1] << 20) | (b[0] << 24) | (b[3] << 28)


def _dot(a, b):
    return F(F(F(a[0] * b[0]) + F(a[1] * b[1])) + F(a[2] * b[2])) + F(a[3] * b[3])


def _normalized(v):
    s = _dot(v, v)
    if s != F(0):
        s = F(1) / np.sqrt(s)
        return [F(c * s) for c in v]
    return list(v)


def _sat(v):
    return [F(0) if c < F(0) else (F(1) if c > F(1) else c) for c in v]


def pvrtc2_rgba_block(t, e, sel, ae, asel):
    """-> (8 bytes, route, detail): the reference's per-pixel re-encoding in binary32, every product and sum rounded on its own, sums left to right. detail["gate"] names
    the way the block went; the coverage counts are made of it."""
    e, sel, ae, asel = [int(v) for v in e], [int(s) for s in sel], [int(v) for v in ae], [int(s) for s in asel]
    low, high, _ = _use(sel)
    a_low, a_high, _ = _use(asel)
    colors = [[int(v) for v in c] for c in X.block_colors(e)]
    av = [int(v) for v in X.block_colors(ae)[:, 1]]
    constant = av[a_low] if all(av[s] == av[a_low] for s in range(a_low, a_high + 1)) else -1
    if constant >= 250:
        block, route, detail = pvrtc2_rgb_block(t, e, sel)
        return block, "rgb", {"gate": "opaque", "alpha": constant, "rgb_route": route}
    solid = all(colors[s] == colors[low] for s in range(low, high + 1))
    if solid and constant >= 0:
        r, g, b = colors[low]
        a0 = [(r * 15 + 128) // 255, (g * 15 + 128) // 255, (b * 7 + 128) // 255, int(t.alpha33_0[constant])]
        err0 = (_x4(a0[0]) - r) ** 2 + (_x4(a0[1]) - g) ** 2 + (_x3(a0[2]) - b) ** 2 + ((a0[3] << 1) * 17 - constant) ** 2 * 2
        if err0 == 0 or constant < 3:
            return [0, 0, 0, 0] + list(_trans_word(a0, [0, 0, 0, 0]).to_bytes(4, "little")), "constant", {"gate": "early_err0" if err0 == 0 else "early_alpha", "alpha": constant}
        b3 = [a0[0], a0[1], (b * 15 + 128) // 255, int(t.alpha33_3[constant])]
        err3 = (_x4(b3[0]) - r) ** 2 + (_x4(b3[1]) - g) ** 2 + (_x4(b3[2]) - b) ** 2 + ((((b3[3] << 1) | 1) * 17) - constant) ** 2 * 2
        l1 = [int(t.trans44[r, 0]), int(t.trans44[g, 0]), int(t.trans34[b, 0]), int(t.alpha33[constant, 0])]
        h1 = [int(t.trans44[r, 1]), int(t.trans44[g, 1]), int(t.trans34[b, 1]), int(t.alpha33[constant, 1])]
        lo8, hi8 = [_x4(l1[0]), _x4(l1[1]), _x3(l1[2]), (l1[3] << 1) * 17], [_x4(h1[0]), _x4(h1[1]), _x4(h1[2]), ((h1[3] << 1) | 1) * 17]
        mid = [(p * 5 + q * 3) // 8 for p, q in zip(lo8, hi8)]
        err1 = (mid[0] - r) ** 2 + (mid[1] - g) ** 2 + (mid[2] - b) ** 2 + (mid[3] - constant) ** 2 * 2
        detail = {"alpha": constant, "tie03": err0 == err3}
        if err1 < err0 and err1 < err3:
            return [0x55] * 4 + list(_trans_word(l1, h1).to_bytes(4, "little")), "constant", dict(detail, gate="mode1")
        if err0 < err3:
            return [0] * 4 + list(_trans_word(a0, [0, 0, 0, 0]).to_bytes(4, "little")), "constant", dict(detail, gate="mode0")
        return [0xFF] * 4 + list(_trans_word([0, 0, 0, 0], b3).to_bytes(4, "little")), "constant", dict(detail, gate="mode3")
    S = F(1) / F(255)
    detail = {}
    clamped = any(colors[low][k] == 0 or colors[high][k] == 255 for k in range(3)) or av[a_low] == 0 or av[a_high] == 255
    if solid:
        lo, hi = [F(F(c) * S) for c in colors[low] + [av[a_low]]], [F(F(c) * S) for c in colors[low] + [av[a_high]]]
        detail["gate"] = "solid_colour"
    elif constant >= 0:
        lo, hi = [F(F(c) * S) for c in colors[low] + [constant]], [F(F(c) * S) for c in colors[high] + [constant]]
        detail["gate"], detail["alpha"] = "constant_alpha", constant
    elif clamped:
        px = [colors[sel[p]] + [av[asel[p]]] for p in range(16)]
        total = [F(sum(q[k] for q in px)) for k in range(4)]
        mean16 = [F(c * F(1.0 / 16.0)) for c in total]
        mean = _sat([F(c * (F(1) / F(16.0 * 255.0))) for c in total])
        axis = [F(0)] * 4
        for p in range(16):
            q = [F(F(c) - m) for c, m in zip(px[p], mean16)]
            n = _normalized(axis if p else q)
            axis = [F(axis[k] + _dot([F(c * q[k]) for c in q], n)) for k in range(4)]
        axis = _normalized(axis)
        detail["axis_fallback"] = bool(_dot(axis, axis) < F(.5))
        if detail["axis_fallback"]:
            axis = [F(.5)] * 4
        l, h = F(1e9), F(-1e9)
        for p in range(16):
            d = _dot([F(F(c) - m) for c, m in zip(px[p], mean16)], axis)
            l, h = (l if l < d else d), (h if h > d else d)
        l, h = F(l * S), F(h * S)
        lo, hi = _sat([F(m + F(c * l)) for m, c in zip(mean, axis)]), _sat([F(m + F(c * h)) for m, c in zip(mean, axis)])
        detail["swapped"] = bool(lo[3] > hi[3])
        if detail["swapped"]:
            lo, hi = hi, lo
        detail["gate"] = "pca4d_swapped" if detail["swapped"] else "pca4d"
    else:
        lum, alp = [sum(c) for c in colors], [a * 3 for a in av]
        p0 = [lum[sel[p]] + alp[asel[p]] for p in range(16)]
        p1 = [lum[sel[p]] - alp[asel[p]] for p in range(16)]
        lo, hi = [F(F(c) * S) for c in colors[low] + [av[a_low]]], [F(F(c) * S) for c in colors[high] + [av[a_high]]]
        flip = max(p1) - min(p1) > max(p0) - min(p0)
        if flip:
            lo[:3], hi[:3] = hi[:3], lo[:3]
        detail["gate"] = "pca2d_flipped" if flip else "pca2d"
    qa = [int(F(F(lo[0] * F(15)) + F(.5))), int(F(F(lo[1] * F(15)) + F(.5))), int(F(F(lo[2] * F(7)) + F(.5))), int(F(F(lo[3] * F(7)) + F(.5)))]
    qb = [int(F(F(hi[0] * F(15)) + F(.5))), int(F(F(hi[1] * F(15)) + F(.5))), int(F(F(hi[2] * F(15)) + F(.5))), int(F(F(hi[3] * F(7)) + F(.5)))]
    c0 = [_x4(qa[0]), _x4(qa[1]), _x3(qa[2]), (qa[3] << 1) * 17]
    c3 = [_x4(qb[0]), _x4(qb[1]), _x4(qb[2]), ((qb[3] << 1) | 1) * 17]
    axis = [q - p for p, q in zip(c0, c3)]
    length = sum(c * c for c in axis)
    t01, t12, t23 = (length * 3) // 16, length >> 1, (length * 13) // 16
    detail["alpha_only"] = axis[:3] == [0, 0, 0]
    mod = []
    for p in range(16):
        d = sum((colors[sel[p]][k] - c0[k]) * axis[k] for k in range(3)) + (av[asel[p]] - c0[3]) * axis[3]
        mod.append((d >= t23) + (d >= t12) + (d >= t01))
    return _selector_bytes(mod) + list(_trans_word(qa, qb).to_bytes(4, "little")), "pixels", detail


# ---------------------------------------------------------------- FXT1 by way of BC1 without three-colour blocks

BC1_CODE = [0, 2, 3, 1]   # the four colours in linear order -> BC1's selector codes


def bc1_four_colour(t, e, sel):
    """-> (colour 0 as 565, colour 1 as 565, sixteen BC1 selector codes, route, detail): the reference's ETC1S -> BC1 with three-colour blocks forbidden, so that the
    first colour always ends up greater than the second. detail["guard"]: None, or which of the two punch-through guards fired and on what: ("solid" | "lookup",
    "zero" | "positive")."""
    e, sel = [int(v) for v in e], [int(s) for s in sel]
    low, high, n = _use(sel)
    colors = X.block_colors(e)
    if n == 1:
        r, g, b = (int(v) for v in colors[low])
        max16 = (int(t.bc1_solid[5][r, 0]) << 11) | (int(t.bc1_solid[6][g, 0]) << 5) | int(t.bc1_solid[5][b, 0])
        min16 = (int(t.bc1_solid[5][r, 1]) << 11) | (int(t.bc1_solid[6][g, 1]) << 5) | int(t.bc1_solid[5][b, 1])
        code, guard = 2, None
        if min16 == max16:
            if min16 > 0:
                min16, code, guard = min16 - 1, 0, ("solid", "positive")
            else:
                max16, min16, code, guard = 1, 0, 1, ("solid", "zero")
        if max16 < min16:
            max16, min16, code = min16, max16, code ^ 1
        return max16, min16, [code] * 16, "solid", {"guard": guard, "values": (r, g, b)}
    if e[3] == 7 and n == 2 and (low, high) == (0, 3):
        c0, c3 = [int(v) for v in colors[0]], [int(v) for v in colors[3]]
        max16 = (int(t.bc1_end[5][c0[0]]) << 11) | (int(t.bc1_end[6][c0[1]]) << 5) | int(t.bc1_end[5][c0[2]])
        min16 = (int(t.bc1_end[5][c3[0]]) << 11) | (int(t.bc1_end[6][c3[1]]) << 5) | int(t.bc1_end[5][c3[2]])
        l, h = 0, 1
        if min16 == max16:
            if min16 > 0:
                min16, l, h = min16 - 1, 0, 0
            else:
                max16, min16, l, h = 1, 0, 1, 1
        if max16 < min16:
            max16, min16, l, h = min16, max16, 1, 0
        return max16, min16, [h if s == 3 else l for s in sel], "outlier", {"guard": None}
    r = RANGES.index((low, high))
    rows = [t.bc1[5][e[3], e[0], r], t.bc1[6][e[3], e[1], r], t.bc1[5][e[3], e[2], r]]
    m = _best_mapping(rows)
    l = ((int(rows[0][m]) & 255) << 11) | ((int(rows[1][m]) & 255) << 5) | (int(rows[2][m]) & 255)
    h = (((int(rows[0][m]) >> 8) & 255) << 11) | (((int(rows[1][m]) >> 8) & 255) << 5) | ((int(rows[2][m]) >> 8) & 255)
    swapped = l < h
    if swapped:
        l, h = h, l
    if l == h:
        if h > 0:
            return l, h - 1, [0] * 16, "lookup", {"guard": ("lookup", "positive"), "entry": (e[3], r, m)}
        return 1, 0, [1] * 16, "lookup", {"guard": ("lookup", "zero"), "entry": (e[3], r, m)}
    codes = [BC1_CODE[3 - MAPPINGS[m][s]] if swapped else BC1_CODE[MAPPINGS[m][s]] for s in sel]
    return l, h, codes, "lookup", {"guard": None, "entry": (e[3], r, m)}


def fxt1_half(t, e, sel):
    """-> (colour 0 as [r5, g5, b5], colour 1, the lsb of colour 1's green, sixteen selectors in linear order, route, detail). FXT1 keeps five bits of green per colour
    and one lsb per half, colour 1's; colour 0's lsb is that bit XOR the top bit of the half's first selector. Where the BC1 block says otherwise the colours trade
    places and the selectors are inverted (detail["swapped"])."""
    l, h, codes, route, detail = bc1_four_colour(t, e, sel)
    linear = [BC1_CODE.index(c) for c in codes]
    c0, c1 = [(l >> 11) & 31, (l >> 5) & 63, l & 31], [(h >> 11) & 31, (h >> 5) & 63, h & 31]
    g0, g1 = c0[1] & 1, c1[1] & 1
    c0[1] >>= 1
    c1[1] >>= 1
    detail["swapped"] = (linear[0] >> 1) != (g0 ^ g1)
    if detail["swapped"]:
        c0, c1, g0, g1, linear = c1, c0, g1, g0, [3 - s for s in linear]
    return c0, c1, g1, linear, route, detail


def fxt1_block(left, right):
    """two fxt1_half() results (right None: the lone left half of an odd row) -> 16 bytes: the selectors of the left half, of the right half, then 64 bits: four
    colours of b, g, r (5 bits each, in that order from bit 0), alpha (bit 60), the two green lsbs (61, 62), mode (63)"""
    if right is None:
        dup = [left[3][y * 4 + 3] for y in range(4) for _ in range(4)]   # the left half's right column across the other half
        right = (left[0], left[1], left[2], dup)
    word = 0
    for k, c in enumerate((left[0], left[1], right[0], right[1])):
        word |= (c[2] | (c[1] << 5) | (c[0] << 10)) << (15 * k)
    word |= (left[2] | (right[2] << 1)) << 61
    word |= 1 << 63
    return _selector_bytes(left[3]) + _selector_bytes(right[3]) + list(word.to_bytes(8, "little"))


def blocks(decoded, image, target, details=None, t=None):
    """(n, 8 | 16) u8: what the transcoder writes for ATC_RGB, FXT1_RGB or PVRTC2_4_RGB. details: a list that receives (route, detail) per SOURCE block."""
    t = t or tables()
    ep, sel = np.asarray(decoded["endpoint_palette"]), X.selectors16(decoded["selector_palette"])
    ei, si = image["endpoint_indices"], image["selector_indices"]
    nby, nbx = ei.shape
    cache = {}

    def one(y, x):
        key = (int(ei[y, x]), int(si[y, x]))
        if key not in cache:
            cache[key] = (fxt1_half if target == FXT1_RGB else atc_block if target == ATC_RGB else pvrtc2_rgb_block)(t, ep[key[0]], sel[key[1]])
        if details is not None:
            details.append(cache[key][-2:])
        return cache[key]
    if target == PVRTC2_4_RGBA:
        if image["alpha_endpoint_indices"] is None:
            return blocks(decoded, image, PVRTC2_4_RGB, None, t)
        aei, asi = image["alpha_endpoint_indices"], image["alpha_selector_indices"]
        out = []
        for y in range(nby):
            for x in range(nbx):
                key = (int(ei[y, x]), int(si[y, x]), int(aei[y, x]), int(asi[y, x]))
                if key not in cache:
                    cache[key] = pvrtc2_rgba_block(t, ep[key[0]], sel[key[1]], ep[key[2]], sel[key[3]])
                out.append(cache[key][0])
                if details is not None:
                    details.append(cache[key][1:])
        return np.array(out, np.uint8).reshape(-1, 8)
    if target != FXT1_RGB:
        return np.array([one(y, x)[0] for y in range(nby) for x in range(nbx)], np.uint8).reshape(-1, 8)
    return np.array([fxt1_block(one(y, x), one(y, x + 1) if x + 1 < nbx else None) for y in range(nby) for x in range(0, nbx, 2)], np.uint8).reshape(-1, 16)
