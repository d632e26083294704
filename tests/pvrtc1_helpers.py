"""What the PVRTC1 tests share: the golden file (tests/golden/pvrtc1_vectors.npz, written by tools/gen_golden_pvrtc1.py) and a CPU restatement of the four routes
(ETC1S / UASTC to PVRTC1 4bpp RGB / RGBA) in vectorised numpy, written from the rules of the format and of the reference's transcoder, none of its tables copied:

  expansions    5 bits to 8 by bit replication; 4 and 3 bits to 5 by bit replication, then on; the 3-bit alpha code a is the 4-bit code 2a replicated (34a), code 8
                is the opaque 255
  floor / ceil  BY DEFINITION here: the largest code whose expansion is <= v, the smallest whose expansion is >= v (a search; the kernels use a closed form)
  endpoints     low | high << 16; opaque 1 RRRRR GGGGG BBBB 0 / 1 RRRRR GGGGG BBBBB; translucent 0 AAA RRRR GGGG BBB 0 / 0 AAA RRRR GGGG BBBB. RGB routes: always
                opaque. RGBA routes: each endpoint on its own is opaque where its alpha floors (low) / ceils (high) to code 8
  pass 1        ETC1S: the block colour of the lowest / highest selector the block uses (alpha: the alpha slice's green); UASTC: component-wise min / max of the pixels
  pass 2        per texel cl = ETC1S RGB: 16 (r8 + g8 + b8) + 48 intensity, not clamped; ETC1S RGBA: that clamped to 0..48*255 plus 16 g8 + 16 intensity of the alpha
                slice clamped to 0..16*255; UASTC: 16 (r + g + b [+ a]). Against ca / cb, the low / high lumas of the 3x3 neighbours (wrapped) under the bilinear
                weights: p = 16 (cl - ca), dl = cb - ca, both negated when ca > cb; modulation 1 / 2 / 3 where p > 3 dl, p > 8 dl, p > 13 dl (strict)
  address       Morton, y in the even bits, over the low min(log2 nbx, log2 nby) bits of both; the longer axis' other bits above
  invalid block its endpoint word is 0 (neighbours read both lumas as 0), its eight output bytes are 0
"""
import functools
import pathlib

import numpy as np

import native_libs

GOLDEN = pathlib.Path(__file__).resolve().parent / "golden" / "pvrtc1_vectors.npz"
RGB, RGBA = 8, 9   # cTFPVRTC1_4_RGB, cTFPVRTC1_4_RGBA
TAGS = {"rgb": "PVRTC1_4_RGB", "rgba": "PVRTC1_4_RGBA"}
TARGETS = {"rgb": RGB, "rgba": RGBA}
INTEN = np.array([[-8, -2, 2, 8], [-17, -5, 5, 17], [-29, -9, 9, 29], [-42, -13, 13, 42], [-60, -18, 18, 60], [-80, -24, 24, 80], [-106, -33, 33, 106], [-183, -47, 47, 183]])


@functools.lru_cache(maxsize=None)
def golden():
    """-> (arrays, meta): loaded once and shared; nobody writes into the arrays"""
    return native_libs.load_npz_golden(GOLDEN)


def image_key(name, level, layer, face):
    return f"{name}_L{level}_A{layer}_F{face}"


# ---------------------------------------------------------------- codes

def _replicate(c, bits, to):
    """a `bits`-bit code widened to `to` bits by repeating its top bits"""
    c = np.asarray(c, np.int64)
    out, have = c.copy(), bits
    while have < to:
        take = min(bits, to - have)
        out = (out << take) | (c >> (bits - take))
        have += take
    return out


EXPAND = {5: _replicate(np.arange(32), 5, 8), 4: _replicate(_replicate(np.arange(16), 4, 5), 5, 8), 3: _replicate(_replicate(np.arange(8), 3, 5), 5, 8),
          "alpha": np.concatenate([_replicate(2 * np.arange(8), 4, 8), [255]])}


def floor_codes(kind):
    """(256,): for every v the largest code whose expansion is <= v"""
    e = EXPAND[kind]
    return np.array([max(c for c in range(e.size) if e[c] <= v) for v in range(256)])


def ceil_codes(kind):
    """(256,): for every v the smallest code whose expansion is >= v"""
    e = EXPAND[kind]
    return np.array([min(c for c in range(e.size) if e[c] >= v) for v in range(256)])


FLOOR = {k: floor_codes(k) for k in EXPAND}
CEIL = {k: ceil_codes(k) for k in EXPAND}


def endpoint_words(low, high, alpha):
    """low / high: (n, 4) bounds r, g, b, a -> (n,) u32"""
    low, high = np.asarray(low, np.int64), np.asarray(high, np.int64)
    lo = 0x8000 | (FLOOR[5][low[:, 0]] << 10) | (FLOOR[5][low[:, 1]] << 5) | (FLOOR[4][low[:, 2]] << 1)
    hi = 0x8000 | (CEIL[5][high[:, 0]] << 10) | (CEIL[5][high[:, 1]] << 5) | CEIL[5][high[:, 2]]
    if alpha:
        la, ha = FLOOR["alpha"][low[:, 3]], CEIL["alpha"][high[:, 3]]
        lo = np.where(la == 8, lo, (la << 12) | (FLOOR[4][low[:, 0]] << 8) | (FLOOR[4][low[:, 1]] << 4) | (FLOOR[3][low[:, 2]] << 1))
        hi = np.where(ha == 8, hi, (ha << 12) | (CEIL[4][high[:, 0]] << 8) | (CEIL[4][high[:, 1]] << 4) | CEIL[4][high[:, 2]])
    return (lo | (hi << 16)).astype(np.uint32)


def endpoint_lumas(words, alpha):
    """what the modulation pass reads back from the words -> (low luma, high luma), int64, the words' shape"""
    w = np.asarray(words, np.uint32).astype(np.int64)
    lo, hi = w & 0xFFFE, w >> 16
    if not alpha:
        b = lo & 30
        return (((lo >> 10) & 31) + ((lo >> 5) & 31) + (b | (b >> 4))) * 255 // 31, (((hi >> 10) & 31) + ((hi >> 5) & 31) + (hi & 31)) * 255 // 31
    l0 = np.where(lo & 0x8000, EXPAND[5][(lo >> 10) & 31] + EXPAND[5][(lo >> 5) & 31] + EXPAND[4][(lo & 31) >> 1] + 255,
                  EXPAND[4][(lo >> 8) & 15] + EXPAND[4][(lo >> 4) & 15] + EXPAND[3][(lo & 15) >> 1] + EXPAND["alpha"][(lo >> 12) & 7])
    l1 = np.where(hi & 0x8000, EXPAND[5][(hi >> 10) & 31] + EXPAND[5][(hi >> 5) & 31] + EXPAND[5][hi & 31] + 255,
                  EXPAND[4][(hi >> 8) & 15] + EXPAND[4][(hi >> 4) & 15] + EXPAND[4][hi & 15] + EXPAND["alpha"][(hi >> 12) & 7])
    return l0, l1


# ---------------------------------------------------------------- the address

def interleave_bit_by_bit(x, y, nbx, nby):
    """the Morton address of block (x, y), one bit at a time (plain ints)"""
    xb, yb = nbx.bit_length() - 1, nby.bit_length() - 1
    low, at = min(xb, yb), 0
    for k in range(low):
        at |= ((y >> k) & 1) << (2 * k)
        at |= ((x >> k) & 1) << (2 * k + 1)
    return at | (((x if nbx > nby else y) >> low) << (2 * low))


def morton_addresses(nbx, nby):
    """(nby, nbx) int64: where each block of the raster is stored"""
    assert nbx & (nbx - 1) == 0 and nby & (nby - 1) == 0 and nbx and nby
    y, x = np.mgrid[0:nby, 0:nbx].astype(np.int64)
    low, at = min(nbx.bit_length(), nby.bit_length()) - 1, np.zeros((nby, nbx), np.int64)
    for k in range(low):
        at |= (((y >> k) & 1) << (2 * k)) | (((x >> k) & 1) << (2 * k + 1))
    return at | (((x if nbx > nby else y) >> low) << (2 * low))


# ---------------------------------------------------------------- the second pass, and the whole image

def new_stats():
    return {"modulation": [0, 0, 0, 0], "endpoint_formats": {"opaque_opaque": 0, "opaque_translucent": 0, "translucent_opaque": 0, "translucent_translucent": 0},
            "wrapped": {k: 0 for k in ("left", "right", "top", "bottom", "top_left", "top_right", "bottom_left", "bottom_right")},
            "dl_zero_p_positive": 0, "dl_zero_p_not_positive": 0, "p_equals_3dl": 0, "p_equals_8dl": 0, "p_equals_13dl": 0, "ca_above_cb": 0, "blocks": 0}


def assemble(words, cl, alpha, valid=None, stats=None):
    """words: (nby, nbx) u32 of pass 1 (0 where invalid); cl: (nby, nbx, 16) texel values, texel y * 4 + x -> the image's (nby * nbx, 8) u8 blocks in storage order"""
    words = np.asarray(words, np.uint32)
    nby, nbx = words.shape
    cl = np.asarray(cl, np.int64).reshape(nby, nbx, 16)
    valid = np.ones((nby, nbx), bool) if valid is None else np.asarray(valid, bool).reshape(nby, nbx)
    l0, l1 = endpoint_lumas(words, alpha)

    def at(a, dy, dx):   # a[(y + dy) mod nby, (x + dx) mod nbx]
        return np.roll(a, (-dy, -dx), (0, 1))
    mod = np.zeros((nby, nbx), np.int64)
    for y in range(4):
        for x in range(4):
            dx, dy, u, v = (x >> 1) - 1, (y >> 1) - 1, (x + 2) & 3, (y + 2) & 3
            w = ((4 - u) * (4 - v), u * (4 - v), (4 - u) * v, u * v)
            ca = w[0] * at(l0, dy, dx) + w[1] * at(l0, dy, dx + 1) + w[2] * at(l0, dy + 1, dx) + w[3] * at(l0, dy + 1, dx + 1)
            cb = w[0] * at(l1, dy, dx) + w[1] * at(l1, dy, dx + 1) + w[2] * at(l1, dy + 1, dx) + w[3] * at(l1, dy + 1, dx + 1)
            swap = ca > cb
            dl, p = np.where(swap, ca - cb, cb - ca), np.where(swap, -1, 1) * (cl[:, :, y * 4 + x] - ca) * 16
            m = (p > 3 * dl).astype(np.int64) + (p > 8 * dl) + (p > 13 * dl)
            mod |= m << (y * 8 + x * 2)
            if stats is not None:
                for k in range(4):
                    stats["modulation"][k] += int(((m == k) & valid).sum())
                stats["dl_zero_p_positive"] += int(((dl == 0) & (p > 0) & valid).sum())
                stats["dl_zero_p_not_positive"] += int(((dl == 0) & (p <= 0) & valid).sum())
                for k in (3, 8, 13):
                    stats[f"p_equals_{k}dl"] += int(((dl > 0) & (p == k * dl) & valid).sum())
                stats["ca_above_cb"] += int((swap & valid).sum())
    if stats is not None:
        lo_opaque, hi_opaque = (words & 0x8000) != 0, (words & 0x80000000) != 0
        for name, sel in (("opaque_opaque", lo_opaque & hi_opaque), ("opaque_translucent", lo_opaque & ~hi_opaque), ("translucent_opaque", ~lo_opaque & hi_opaque),
                          ("translucent_translucent", ~lo_opaque & ~hi_opaque)):
            stats["endpoint_formats"][name] += int((sel & valid).sum())
        stats["blocks"] += nbx * nby
        for name, n in (("left", nby), ("right", nby), ("top", nbx), ("bottom", nbx), ("top_left", 1), ("top_right", 1), ("bottom_left", 1), ("bottom_right", 1)):
            stats["wrapped"][name] += n
    out = np.zeros((nby * nbx, 2), np.uint32)
    where = morton_addresses(nbx, nby)
    out[where.reshape(-1), 0] = np.where(valid, mod, 0).reshape(-1).astype(np.uint32)
    out[where.reshape(-1), 1] = np.where(valid, words, 0).reshape(-1)
    return out.view(np.uint8).reshape(-1, 8)


# ---------------------------------------------------------------- ETC1S

def _selectors16(words):
    return ((np.asarray(words, np.uint32)[:, None] >> (2 * np.arange(16, dtype=np.uint32))[None, :]) & 3).astype(np.int64)


def etc1s_state_blocks(endpoint_palette, selector_palette, endpoint_idx, selector_idx, alpha_endpoint_idx, alpha_selector_idx, nbx, nby, target, stats=None):
    """One image of an ETC1S state: endpoint_palette (n, 4) u8 -- r5, g5, b5, intensity table --, selector_palette (n,) u32, the image's indices (the alpha slice's
    None = no alpha slice; RGBA then takes the RGB route). An index past its palette makes the block invalid -> ((nby * nbx, 8) u8, invalid count)"""
    ep, sp = np.asarray(endpoint_palette, np.int64).reshape(-1, 4), np.asarray(selector_palette, np.uint32).reshape(-1)
    alpha = int(target) == RGBA and alpha_endpoint_idx is not None
    idx = [np.asarray(a, np.int64).reshape(-1) for a in ([endpoint_idx, selector_idx] + ([alpha_endpoint_idx, alpha_selector_idx] if alpha else []))]
    n = nbx * nby
    assert all(a.size == n for a in idx)
    valid = (idx[0] < ep.shape[0]) & (idx[1] < sp.size)
    if alpha:
        valid &= (idx[2] < ep.shape[0]) & (idx[3] < sp.size)
    safe = [np.where(valid, a, 0) for a in idx]
    rows = np.arange(n)
    e, sel = ep[safe[0]], _selectors16(sp[safe[1]])
    base = (e[:, :3] << 3) | (e[:, :3] >> 2)
    inten = INTEN[e[:, 3]]                                           # (n, 4)
    low = np.full((n, 4), 255, np.int64)
    high = low.copy()
    low[:, :3] = np.clip(base + inten[rows, sel.min(1)][:, None], 0, 255)
    high[:, :3] = np.clip(base + inten[rows, sel.max(1)][:, None], 0, 255)
    cl = 16 * base.sum(1)[:, None] + 48 * inten[rows[:, None], sel]
    if alpha:
        ae, asel = ep[safe[2]], _selectors16(sp[safe[3]])
        ag, ainten = (ae[:, 1] << 3) | (ae[:, 1] >> 2), INTEN[ae[:, 3]]
        low[:, 3] = np.clip(ag + ainten[rows, asel.min(1)], 0, 255)
        high[:, 3] = np.clip(ag + ainten[rows, asel.max(1)], 0, 255)
        cl = np.clip(cl, 0, 48 * 255) + np.clip(16 * ag[:, None] + 16 * ainten[rows[:, None], asel], 0, 16 * 255)
    words = np.where(valid, endpoint_words(low, high, alpha), 0).astype(np.uint32)
    return assemble(words.reshape(nby, nbx), cl, alpha, valid, stats), int((~valid).sum())


def etc1s_image_blocks(dec, im, target, stats=None):
    """one image of decode_etc1s_file's result"""
    return etc1s_state_blocks(dec["endpoint_palette"], dec["selector_palette"], im["endpoint_indices"], im["selector_indices"], im["alpha_endpoint_indices"],
                              im["alpha_selector_indices"], im["num_blocks_x"], im["num_blocks_y"], target, stats)[0]


# ---------------------------------------------------------------- UASTC

def uastc_pixels(blocks):
    """(n, 16) u8 UASTC blocks -> ((n, 16, 4) the unpacked pixels, pixel y * 4 + x; (n,) bool: the block unpacks), by the host build of the unpacker"""
    import uastc_texture_helpers as U
    px, ok = U.host_texture(blocks, 13)
    return px.reshape(-1, 16, 4).astype(np.int64), ok != 0


def pixels_blocks(px, valid, nbx, nby, target, stats=None):
    """the UASTC routes behind the unpacker: px (n, 16, 4) -> ((nby * nbx, 8) u8, invalid count)"""
    alpha = int(target) == RGBA
    px, valid = np.asarray(px, np.int64).reshape(nbx * nby, 16, 4), np.asarray(valid, bool).reshape(-1)
    words = np.where(valid, endpoint_words(px.min(1), px.max(1), alpha), 0).astype(np.uint32)
    cl = 16 * (px.sum(2) if alpha else px[:, :, :3].sum(2))
    return assemble(words.reshape(nby, nbx), cl, alpha, valid, stats), int((~valid).sum())


def uastc_blocks(blocks, nbx, nby, target, stats=None):
    px, ok = uastc_pixels(blocks)
    return pixels_blocks(px, ok, nbx, nby, target, stats)


def reserved_mode_byte():
    """a first byte that matches none of UASTC's 19 mode codes: a block that begins with it does not unpack"""
    import transcode_helpers as T
    first = np.zeros((256, 16), np.uint8)
    first[:, 0] = np.arange(256)
    return int(np.flatnonzero(T.code_modes(first) == 255)[0])
