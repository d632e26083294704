"""What the ETC1S texture-target tests share: the golden file (tests/golden/etc1s_texture_vectors.npz, written by tools/gen_golden_etc1s_texture.py) and a plain
restatement on the CPU of what the device does for the two-half and BC7 targets: the per-block conversions over the look-up tables that
tools/gen_etc1s_transcode_tables.py computes, the BC7 chroma filter and the small mode-5 encoder under it. The filter and the encoder are binary32 arithmetic: every
operand below is an np.float32 and every expression keeps the operation order of the device code, so the result is the same bits. The generator accepts its npz only
after this restatement has reproduced every block in it; the host tests repeat that, and the GPU tests compare the kernels with the same goldens."""
import functools
import pathlib
import sys

import numpy as np

import etc1s_transcode_helpers as E
import native_libs

GOLDEN = pathlib.Path(__file__).resolve().parent / "golden" / "etc1s_texture_vectors.npz"
ETC2_RGBA, BC7_RGBA = 1, 6
TAGS = {"etc2": "ETC2_RGBA", "bc7": "BC7_RGBA"}           # npz key suffix -> the reference tool's file tag; "bc7nf" is BC7 with the chroma filter off
NO_CHROMA_FILTERING = 64                                  # cDecodeFlagsNoETC1SChromaFiltering
F = np.float32
RANGES = E.BC1_RANGES                                     # the six selector ranges of the BC7 look-ups
ALPHA_RANGES = [(0, 3), (1, 3), (0, 2), (1, 2)]           # the four of the EAC A8 look-up; any other range reads entry 0
MAPPINGS = [(0, 0, 1, 1), (0, 0, 1, 2), (0, 0, 1, 3), (0, 0, 2, 3), (0, 1, 1, 1), (0, 1, 2, 2), (0, 1, 2, 3), (0, 2, 3, 3), (1, 2, 2, 2), (1, 2, 3, 3)]


@functools.lru_cache(maxsize=None)
def golden():
    return native_libs.load_npz_golden(GOLDEN)


@functools.lru_cache(maxsize=None)
def tables():
    """the host statements of every look-up (tools/gen_etc1s_transcode_tables.py), computed once"""
    sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent.parent / "tools"))
    import gen_etc1s_transcode_tables as G
    return {"bc7_color": G.bc7_color_table().reshape(8, 32, 6, 10), "bc7_alpha": G.bc7_alpha_table().reshape(8, 32, 6), "bc7_solid": G.bc7_solid_table().reshape(256, 2),
            "eac_a8": G.eac_a8_table().reshape(8, 32, 4)}


def block_colors(e):
    """(4, 3) ints: the four colours of an endpoint-palette entry (r5, g5, b5, intensity table)"""
    base = np.array([(int(c) << 3) | (int(c) >> 2) for c in e[:3]])
    return np.clip(base[None, :] + E.INTEN[int(e[3])][:, None], 0, 255)


def selectors16(selector_palette):
    """(n,) u32 -> (n, 16): selector of texel y * 4 + x"""
    return ((np.asarray(selector_palette, np.uint32)[:, None] >> (2 * np.arange(16, dtype=np.uint32))[None, :]) & 3).astype(np.int64)


# ---------------------------------------------------------------- ETC2 RGBA: EAC A8 of the alpha slice, ETC1 of the colour slice

def eac_a8_block(t, e, sel):
    """8 bytes: base, table | multiplier << 4, then 48 selector bits big endian, texel (x, y) at bit 45 - 3 * (x * 4 + y)"""
    lo, hi = int(sel.min()), int(sel.max())
    if lo == hi:   # constant: table 13, multiplier 1, every selector 4 (modifier 0)
        base, table, mul, code = int(block_colors(e)[lo, 0]), 13, 1, [4, 4, 4, 4]
    else:
        v = int(t["eac_a8"][int(e[3]), int(e[0]), ALPHA_RANGES.index((lo, hi)) if (lo, hi) in ALPHA_RANGES else 0])
        base, table, mul, code = v & 255, (v >> 8) & 15, (v >> 12) & 15, [(v >> (16 + 3 * s)) & 7 for s in range(4)]
    bits = 0
    for y in range(4):
        for x in range(4):
            bits |= code[int(sel[y * 4 + x])] << (45 - 3 * (x * 4 + y))
    return [base, table | (mul << 4)] + [(bits >> (8 * (5 - k))) & 255 for k in range(6)]


OPAQUE_EAC_A8 = [255, 13 | (1 << 4), 0x92, 0x49, 0x24, 0x92, 0x49, 0x24]


def etc2_rgba_blocks(decoded, image):
    """(n, 16) u8: what the transcoder writes for ETC2_RGBA"""
    t, ep, sel = tables(), np.asarray(decoded["endpoint_palette"]), selectors16(decoded["selector_palette"])
    ei, si = image["endpoint_indices"].reshape(-1), image["selector_indices"].reshape(-1)
    out = np.zeros((ei.size, 16), np.uint8)
    etc1 = E.etc1s_output_blocks(ep, sel, ei, si)
    etc1[:, 3] &= 0xFE   # the transcoder leaves the flip bit clear
    out[:, 8:] = etc1
    if image["alpha_endpoint_indices"] is None:
        out[:, :8] = OPAQUE_EAC_A8
    else:
        for k, (a, s) in enumerate(zip(image["alpha_endpoint_indices"].reshape(-1), image["alpha_selector_indices"].reshape(-1))):
            out[k, :8] = eac_a8_block(t, ep[a], sel[s])
    return out


# ---------------------------------------------------------------- BC7 mode 5
# A block as two Python ints (low and high 64 bits). Low: mode (bit 5 set) in bits 0-5, rotation 6-7, then r0 r1 g0 g1 b0 b1 of 7 bits each from bit 8, a0 (8 bits)
# at bit 50, the low six bits of a1 at bit 58. High: the top two bits of a1, 31 bits of colour indices from bit 2 (texel 0 has one bit: its top bit is implied 0),
# 31 bits of alpha indices from bit 33.

def _pack_lo(l, h, a0=255, a1=255):
    return 32 | (l[0] << 8) | (h[0] << 15) | (l[1] << 22) | (h[1] << 29) | (l[2] << 36) | (h[2] << 43) | (a0 << 50) | ((a1 & 63) << 58)


def _index_bits(idx):
    """16 two-bit indices, texel 0 first, its top bit dropped -> 31 bits"""
    bits, at = 0, 0
    for i, v in enumerate(idx):
        bits |= int(v) << at
        at += 2 if i else 1
    return bits


def bc7_color(t, e, sel):
    """the opaque mode-5 block of one colour-slice block -> (lo, hi)"""
    e = [int(v) for v in e]
    used = sorted(set(int(s) for s in sel))
    low, high = used[0], used[-1]
    colors = block_colors(e)
    if len(used) == 1:   # solid: the endpoints whose index-1 colour is nearest, every index 1
        c = colors[low]
        l, h = [int(t["bc7_solid"][v, 1]) for v in c], [int(t["bc7_solid"][v, 0]) for v in c]
        return _pack_lo(l, h), 3 | (_index_bits([1] * 16) << 2)
    if len(used) == 2:   # block truncation: the two colours are the endpoints; texel 0 must get an index below 2
        l, h = [int(v) >> 1 for v in colors[low]], [int(v) >> 1 for v in colors[high]]
        low_index = 0
        if int(sel[0]) != low:
            l, h, low_index = h, l, 3
        return _pack_lo(l, h), 3 | (_index_bits([low_index if int(s) == low else 3 ^ low_index for s in sel]) << 2)
    r = RANGES.index((low, high))
    rows = [t["bc7_color"][e[3], e[c], r] for c in range(3)]
    err = sum((row >> 16).astype(np.int64) for row in rows)
    m = int(err.argmin())   # first minimum
    l, h = [int(row[m]) & 127 for row in rows], [(int(row[m]) >> 8) & 127 for row in rows]
    inv = 0
    if MAPPINGS[m][int(sel[0])] & 2:
        l, h, inv = h, l, 3
    return _pack_lo(l, h), 3 | (_index_bits([MAPPINGS[m][int(s)] ^ inv for s in sel]) << 2)


def bc7_alpha(t, lo, hi, e, sel):
    """writes the alpha fields of a block from one alpha-slice block -> (lo, hi)"""
    e = [int(v) for v in e]
    used = sorted(set(int(s) for s in sel))
    low, high = used[0], used[-1]
    values = block_colors(e)[:, 0]

    def with_endpoints(a0, a1):
        return (lo & ~((0xFF << 50) | (0x3F << 58))) | (a0 << 50) | ((a1 & 63) << 58), (hi & ~3) | (a1 >> 6)
    if len(used) == 1:   # the index bits stay as they are: zero
        return with_endpoints(int(values[low]), int(values[low]))
    if len(used) == 2:
        a0, a1, low_index = int(values[low]), int(values[high]), 0
        if int(sel[0]) != low:
            a0, a1, low_index = a1, a0, 3
        idx = [low_index if int(s) == low else 3 ^ low_index for s in sel]
    else:
        v = int(t["bc7_alpha"][e[3], e[0], RANGES.index((low, high))])
        a0, a1, trans = v & 255, (v >> 8) & 255, v >> 16
        if (trans >> (2 * int(sel[0]))) & 2:
            a0, a1, trans = a1, a0, trans ^ 0xFF
        idx = [(trans >> (2 * int(s))) & 3 for s in sel]
    lo, hi = with_endpoints(a0, a1)
    return lo, (hi & ((1 << 33) - 1)) | (_index_bits(idx) << 33)


def _midpoints():
    out = []
    for i in range(128):
        vl = i << 1
        vl |= vl >> 7
        vh = min(127, i + 1) << 1
        vh |= vh >> 7
        out.append(F(1e15) if i == 127 else (F(vl) / F(255.0) + F(vh) / F(255.0)) / F(2.0))
    return out


MIDPOINTS = _midpoints()

# Deliberate errors in the restatement below, each behind its name in MUTATIONS (empty: the restatement as it is). tests/test_etc1s_bc7_filter_host.py switches them on
# one at a time to show that the golden cases tell each of them from the real thing; nothing else may.
#   chroma_ge   >= for > at the chroma gate                  var_le      <= for < at the variance gate
#   var_fused   the variance gate's mean * mean unrounded: product and difference in binary64, rounded once (what a fused multiply-subtract computes)
#   alt_fused   the same in the three sums of the power iteration            ls_fused    the same in the two least-squares results per channel
#   recip       x * (1 / d) for the two divisions 2048 / k and (3 / 255) / det              axis_round  rounding for truncation in (int)(alt * m)
#   to7_ge      >= for > in to_7                              skip_corner the gate never looks at the neighbour at (+1, +1)
#   clamp_off   a neighbour past an edge is clamped one block short of that edge             tie_other   ties on the axis go to the other pixel
#   thresh_161  161 for 160 as the low-variance threshold
MUTATIONS = set()
D = np.float64


def to_7(c):
    """a float in 0..1 -> the 7-bit endpoint nearest it"""
    v = int(c * F(127.0))
    return min(max(v + int(c >= MIDPOINTS[v] if "to7_ge" in MUTATIONS else c > MIDPOINTS[v]), 0), 127)


def to_7_from_8(c8):
    return to_7(F(c8) * (F(1.0) / F(255.0)))


def from_7(v):
    return (v << 1) | (v >> 6)


def interp2(l, h, w):
    return (l * (64 - (0, 21, 43, 64)[w]) + h * (0, 21, 43, 64)[w] + 32) >> 6


def eval_weights(px, l, h):
    l8, h8 = [from_7(v) for v in l], [from_7(v) for v in h]
    c = [[interp2(l8[k], h8[k], i) & 255 for k in range(3)] for i in range(4)]
    a = [c[3][k] - c[0][k] for k in range(3)]
    dots = [sum(c[i][k] * a[k] for k in range(3)) for i in range(4)]
    t0, t1, t2 = dots[0] + dots[1], dots[1] + dots[2], dots[2] + dots[3]
    out = []
    for p in px:
        d = sum(int(p[k]) * a[k] * 2 for k in range(3))
        out.append(int(d > t0) + int(d >= t1) + int(d >= t2))
    return out


def pack_mode5_rgb(l, h, w):
    inv = 0
    if w[0] & 2:
        l, h, inv = h, l, 3
    return _pack_lo(l, h), 3 | (_index_bits([v ^ inv for v in w]) << 2)


def encode_mode5(t, px, trace=None):
    """the filter's mode-5 encoder over 16 RGB pixels ((16, 3) ints) -> ((lo, hi), route): "equal" all pixels the same, "simple" low variance: endpoints at 16/255 and
    239/255 of the channel ranges, "pca" principal axis + one least-squares pass, "pca_det" the same when the least-squares system is singular. trace: a dict that
    receives max_var and, on the two pca routes, default_axis (the power iteration gave nothing), the dots' tie classes (ties) and the two end pixels' numbers."""
    px = [[int(v) for v in p] for p in px]
    total = [sum(p[k] for p in px) for k in range(3)]
    mn, mx = [min(p[k] for p in px) for k in range(3)], [max(p[k] for p in px) for k in range(3)]
    if mn == mx:
        l, h = [int(t["bc7_solid"][v, 1]) for v in mn], [int(t["bc7_solid"][v, 0]) for v in mn]
        return pack_mode5_rgb(l, h, [1] * 16), "equal"
    mean = [(v + 8) >> 4 for v in total]
    icov = [0] * 6
    for p in px:
        r, g, b = (p[k] - mean[k] for k in range(3))
        for j, v in enumerate((r * r, r * g, r * b, g * g, g * b, b * b)):
            icov[j] += v
    max_var = max(icov[0], icov[3], icov[5])
    if trace is not None:
        trace["max_var"] = max_var
    if max_var < (161 if "thresh_161" in MUTATIONS else 160):
        def lerp8(a, b, s):
            v = (b - a) * s + 128
            return a + ((v + (v >> 8)) >> 8)
        l, h = [to_7_from_8(lerp8(mn[k], mx[k], 16)) for k in range(3)], [to_7_from_8(lerp8(mn[k], mx[k], 239)) for k in range(3)]
        return pack_mode5_rgb(l, h, eval_weights(px, l, h)), "simple"
    cov = [F(v) for v in icov]
    sc = F(1.0) / F(max_var)
    wx, wy, wz = sc * cov[0], sc * cov[3], sc * cov[5]
    alt = [cov[0] * wx + cov[1] * wy + cov[2] * wz, cov[1] * wx + cov[3] * wy + cov[4] * wz, cov[2] * wx + cov[4] * wy + cov[5] * wz]
    if "alt_fused" in MUTATIONS:
        alt = [F(D(cov[a]) * D(wx) + D(cov[b]) * D(wy) + D(cov[c]) * D(wz)) for a, b, c in ((0, 1, 2), (1, 3, 4), (2, 4, 5))]
    axis = [306, 601, 117]
    k = max(abs(alt[0]), abs(alt[1]), abs(alt[2]))
    if k >= F(.0000125):
        m = F(2048.0) * (F(1.0) / k) if "recip" in MUTATIONS else F(2048.0) / k
        axis = [int(np.rint(v * m)) if "axis_round" in MUTATIONS else int(v * m) for v in alt]
    elif trace is not None:
        trace["default_axis"] = True
    axis = [v * 16 for v in axis]
    low_dot, high_dot, other = 2 ** 31 - 1, -2 ** 31, 15 if "tie_other" in MUTATIONS else 0
    dots = [(p[0] * axis[0] + p[1] * axis[1] + p[2] * axis[2]) & ~0xF for p in px]
    for i, d in enumerate(dots):
        low_dot, high_dot = min(low_dot, d + (i ^ other)), max(high_dot, d + (i ^ other))
    pl, ph = px[(low_dot & 15) ^ other], px[(high_dot & 15) ^ other]
    if trace is not None:   # a tie that matters: pixels of different colours share the lowest or the highest dot
        trace["ends"] = ((low_dot & 15) ^ other, (high_dot & 15) ^ other)
        trace["ties"] = [len({tuple(p) for p, d in zip(px, dots) if d == e}) for e in (min(dots), max(dots))]
    l, h = [to_7_from_8(v) for v in pl], [to_7_from_8(v) for v in ph]
    w = eval_weights(px, l, h)
    # least squares for the endpoints under these weights
    accum = sum((0x000009, 0x010204, 0x040201, 0x090000)[v] for v in w)
    uq = [sum(w[i] * px[i][c] for i in range(16)) for c in range(3)]
    q10 = [total[c] * 3 - uq[c] for c in range(3)]
    z00, z10, z11 = F((accum >> 16) & 255), F((accum >> 8) & 255), F(accum & 255)
    det = z00 * z11 - z10 * z10
    if abs(det) < F(1e-8):
        return pack_mode5_rgb(l, h, w), "pca_det"
    det = (F(3.0) / F(255.0)) * (F(1.0) / det) if "recip" in MUTATIONS else (F(3.0) / F(255.0)) / det
    iz00, iz01, iz10, iz11 = z11 * det, -z10 * det, -z10 * det, z00 * det

    def clamp01(v):
        return F(0.0) if v < F(0.0) else (F(1.0) if v > F(1.0) else v)
    def pair(a, b, c):
        return F(D(a) * D(F(uq[c])) + D(b) * D(F(q10[c]))) if "ls_fused" in MUTATIONS else a * F(uq[c]) + b * F(q10[c])
    h = [to_7(clamp01(pair(iz00, iz01, c))) for c in range(3)]
    l = [to_7(clamp01(pair(iz10, iz11, c))) for c in range(3)]
    return pack_mode5_rgb(l, h, eval_weights(px, l, h)), "pca"


def cocg(e):
    r, g, b = (F((int(c) << 3) | (int(c) >> 2)) for c in e[:3])
    return (r * F(0.5) + g * F(0.0)) + b * F(-0.5), (r * F(-0.25) + g * F(0.5)) + b * F(-0.25)


def chroma_filter_block(t, lo, hi, ep, ei, bx, by, neighbour_ok=None, trace=None):
    """The chroma filter on block (bx, by) of an image whose colour-slice endpoint indices are ei (nby, nbx): -> ((lo, hi), route). route: None no neighbour differs
    in chroma, "smooth" left alone by the variance gate, else encode_mode5's. neighbour_ok (same shape, bool): False marks an index past the palette, which
    contributes the centre's own entry (the device's documented rule)."""
    nby, nbx = ei.shape

    def clamp(v, n):
        if "clamp_off" in MUTATIONS:
            return min(1, n - 1) if v < 0 else (max(n - 2, 0) if v >= n else v)
        return min(max(v, 0), n - 1)

    def entry(x, y):
        x, y = clamp(x, nbx), clamp(y, nby)
        return ep[int(ei[by, bx])] if neighbour_ok is not None and not neighbour_ok[y, x] else ep[int(ei[y, x])]
    cco, ccg = cocg(entry(bx, by))
    differs = False
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            if (dx or dy) and 0 <= bx + dx < nbx and 0 <= by + dy < nby and not ("skip_corner" in MUTATIONS and dx == 1 and dy == 1):
                co, cg = cocg(entry(bx + dx, by + dy))
                dco, dcg = abs(co - cco), abs(cg - ccg)
                differs = differs or ((dco >= F(10) or dcg >= F(10)) if "chroma_ge" in MUTATIONS else (dco > F(10) or dcg > F(10)))
    if not differs:
        return (lo, hi), None
    l8 = [from_7((lo >> s) & 127) for s in (8, 22, 36)]
    h8 = [from_7((lo >> s) & 127) for s in (15, 29, 43)]
    y_vals = []
    for i in range(4):
        c = [interp2(l8[k], h8[k], i) for k in range(3)]
        y_vals.append(F(c[0]) * F(.25) + F(c[1]) * F(.5) + F(c[2]) * F(.25))
    bits, ys, y_sum, y_sq = hi >> 2, [], F(0.0), F(0.0)
    for i in range(16):
        y = y_vals[bits & (3 if i else 1)]
        bits >>= 2 if i else 1
        ys.append(y)
        y_sum = y_sum + y
        y_sq = y_sq + y * y
    S = F(1.0) / F(16.0)
    mean = y_sum * S
    var = F(D(y_sq * S) - D(mean) * D(mean)) if "var_fused" in MUTATIONS else (y_sq * S) - mean * mean
    if var <= F(3.0) if "var_le" in MUTATIONS else var < F(3.0):
        return (lo, hi), "smooth"
    px = []
    for py in range(4):
        uy = by + ((py - 2) >> 2)
        fy = (F((py + 2) & 3) + F(.5)) * F(.25)
        for pxx in range(4):
            ux = bx + ((pxx - 2) >> 2)
            fx = (F((pxx + 2) & 3) + F(.5)) * F(.25)
            a, b, c, d = cocg(entry(ux, uy)), cocg(entry(ux + 1, uy)), cocg(entry(ux, uy + 1)), cocg(entry(ux + 1, uy + 1))
            f = []
            for k in range(2):
                ab, cd = a[k] + (b[k] - a[k]) * fx, c[k] + (d[k] - c[k]) * fx
                f.append(ab + (cd - ab) * fy)
            y = ys[py * 4 + pxx]
            rgb = [(y * F(1.0) + f[0] * F(1.0)) + f[1] * F(-1.0), (y * F(1.0) + f[0] * F(0.0)) + f[1] * F(1.0), (y * F(1.0) + f[0] * F(-1.0)) + f[1] * F(-1.0)]
            px.append([int(F(.5) + min(max(v, F(0.0)), F(255.0))) for v in rgb])
    if trace is not None:
        trace["px"] = px
    return encode_mode5(t, px, trace)


def bc7_blocks(decoded, image, chroma_filtering=True, routes=None, neighbour_ok=None, route_of=None):
    """(n, 16) u8: what the transcoder writes for BC7_RGBA. routes: a dict that receives how many blocks took each of chroma_filter_block's routes; route_of: a list
    that receives every block's route, in raster order, the two pca routes with "+axis" behind them where the encoder fell back to its default axis."""
    t, ep, sel = tables(), np.asarray(decoded["endpoint_palette"]), selectors16(decoded["selector_palette"])
    ei, si = image["endpoint_indices"], image["selector_indices"]
    nby, nbx = ei.shape
    out = np.zeros((nby * nbx, 16), np.uint8)
    for by in range(nby):
        for bx in range(nbx):
            lo, hi = bc7_color(t, ep[int(ei[by, bx])], sel[int(si[by, bx])])
            if chroma_filtering:
                trace = {}
                (lo, hi), route = chroma_filter_block(t, lo, hi, ep, ei, bx, by, neighbour_ok, trace)
                if routes is not None:
                    routes[route] = routes.get(route, 0) + 1
                if route_of is not None:
                    route_of.append(route + "+axis" if trace.get("default_axis") else route)
            if image["alpha_endpoint_indices"] is not None:
                lo, hi = bc7_alpha(t, lo, hi, ep[int(image["alpha_endpoint_indices"][by, bx])], sel[int(image["alpha_selector_indices"][by, bx])])
            out[by * nbx + bx] = np.frombuffer(int(lo).to_bytes(8, "little") + int(hi).to_bytes(8, "little"), np.uint8)
    return out


def decode_bc7_mode5(blocks):
    """(n, 16) u8 mode-5 blocks, rotation 0 -> (n, 16, 4) u8 texels by the format definition (the byte-order check of the unpack test)"""
    out = np.zeros((len(blocks), 16, 4), np.uint8)
    for n, blk in enumerate(np.asarray(blocks, np.uint8)):
        lo, hi = int.from_bytes(blk[:8].tobytes(), "little"), int.from_bytes(blk[8:].tobytes(), "little")
        assert lo & 255 == 32, "not a mode-5 block with rotation 0"
        l8, h8 = [from_7((lo >> s) & 127) for s in (8, 22, 36)], [from_7((lo >> s) & 127) for s in (15, 29, 43)]
        a0, a1 = (lo >> 50) & 255, ((lo >> 58) & 63) | ((hi & 3) << 6)
        cb, ab = hi >> 2, hi >> 33
        for i in range(16):
            ci, ai = cb & (3 if i else 1), ab & (3 if i else 1)
            cb >>= 2 if i else 1
            ab >>= 2 if i else 1
            out[n, i] = [interp2(l8[k], h8[k], ci) for k in range(3)] + [interp2(a0, a1, ai)]
    return out
