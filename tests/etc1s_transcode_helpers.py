"""What the ETC1S transcoder tests share: the golden file (tests/golden/etc1s_transcode_vectors.npz, written by tools/gen_golden_etc1s_transcode.py), an ETC1 decoder
written from the format definition (the expected value of the pixel targets is the reference tool's ETC1 output decoded by it), the 16-bit packings, and the builders
of synthetic ETC1S states that the backend here wraps into files without a GPU."""
import functools
import pathlib

import numpy as np

import native_libs

GOLDEN = pathlib.Path(__file__).resolve().parent / "golden" / "etc1s_transcode_vectors.npz"
INTEN = np.array([[-8, -2, 2, 8], [-17, -5, 5, 17], [-29, -9, 9, 29], [-42, -13, 13, 42], [-60, -18, 18, 60], [-80, -24, 24, 80], [-106, -33, 33, 106], [-183, -47, 47, 183]])
BC1_RANGES = [(0, 3), (1, 3), (0, 2), (1, 2), (2, 3), (0, 1)]   # selector ranges of the ETC1S -> BC1 tables (tools/gen_etc1s_transcode_tables.py)
BC1_MAPPINGS = 10


@functools.lru_cache(maxsize=None)
def golden():
    """-> (arrays, meta): loaded once and shared; nobody writes into the arrays"""
    return native_libs.load_npz_golden(GOLDEN)


def image_key(name, level, layer, face):
    return f"{name}_L{level}_A{layer}_F{face}"


def decode_etc1_blocks(blocks, nbx, nby):
    """ETC1 (individual and differential mode, both flip settings) by the format definition: (nby * nbx, 8) u8 -> (nby * 4, nbx * 4, 3) u8.
    Bytes 0-2: the two base colours (4+4 bits each, or 5 bits + 3-bit signed delta when the diff bit is set), byte 3: table of sub-block 0 (bits 7-5), of sub-block 1
    (bits 4-2), diff bit (1), flip bit (0); bytes 4-5: the selectors' MSBs, bytes 6-7 their LSBs, texel (x, y) at bit x * 4 + y, big endian. A texel's pixel index
    (MSB, LSB) picks the modifier: 00 -> +small, 01 -> +large, 10 -> -small, 11 -> -large."""
    b = np.ascontiguousarray(blocks, np.uint8).reshape(-1, 8).astype(np.int64)
    n = b.shape[0]
    assert n == nbx * nby
    diff, flip = (b[:, 3] >> 1) & 1, b[:, 3] & 1
    base = np.zeros((n, 2, 3), np.int64)
    for c in range(3):
        hi5, d3 = b[:, c] >> 3, b[:, c] & 7
        d3 = np.where(d3 >= 4, d3 - 8, d3)
        c0d, c1d = hi5, hi5 + d3
        assert ((c1d >= 0) & (c1d <= 31))[diff == 1].all(), "differential colour out of range"
        c0i, c1i = b[:, c] >> 4, b[:, c] & 15
        base[:, 0, c] = np.where(diff == 1, (c0d << 3) | (c0d >> 2), (c0i << 4) | c0i)
        base[:, 1, c] = np.where(diff == 1, (c1d << 3) | (c1d >> 2), (c1i << 4) | c1i)
    table = np.stack([(b[:, 3] >> 5) & 7, (b[:, 3] >> 2) & 7], 1)
    msb, lsb = (b[:, 4] << 8) | b[:, 5], (b[:, 6] << 8) | b[:, 7]
    modifier_of_pixel_index = np.array([2, 3, 1, 0])   # (msb << 1 | lsb) -> column of INTEN's ascending rows
    out = np.zeros((n, 4, 4, 3), np.uint8)
    for x in range(4):
        for y in range(4):
            bit = x * 4 + y
            sel = modifier_of_pixel_index[(((msb >> bit) & 1) << 1) | ((lsb >> bit) & 1)]
            sub = np.where(flip == 1, y >> 1, x >> 1)
            rows = np.arange(n)
            out[:, y, x] = np.clip(base[rows, sub] + INTEN[table[rows, sub], sel][:, None], 0, 255)
    return out.reshape(nby, nbx, 4, 4, 3).transpose(0, 2, 1, 3, 4).reshape(nby * 4, nbx * 4, 3)


def mul_8(v, q):
    """the reference's 8-bit -> q scaling (transcoder.cpp:269)"""
    v = v.astype(np.uint32) * q + 128
    return ((v + (v >> 8)) >> 8) & 255


def pack_pixels(rgba, target):
    """(h, w, 4) u8 -> the 16-bit pixel targets' (h, w) u16: RGB565 (14), BGR565 (15), RGBA4444 (16)"""
    r, g, b, a = (rgba[..., k] for k in range(4))
    if target == 14:
        return ((mul_8(r, 31) << 11) | (mul_8(g, 63) << 5) | mul_8(b, 31)).astype(np.uint16)
    if target == 15:
        return ((mul_8(b, 31) << 11) | (mul_8(g, 63) << 5) | mul_8(r, 31)).astype(np.uint16)
    assert target == 16
    return ((mul_8(r, 15) << 12) | (mul_8(g, 15) << 8) | (mul_8(b, 15) << 4) | mul_8(a, 15)).astype(np.uint16)


def expected_rgba(arrays, key, width, height, nbx, nby):
    """the RGBA32 a golden image must transcode to: its ETC1 golden decoded, alpha from the golden's alpha plane (the reference's RGBA32 of the alpha file) or 255"""
    rgb = decode_etc1_blocks(arrays[key + "_etc1"], nbx, nby)[:height, :width]
    alpha = arrays[key + "_alpha"] if key + "_alpha" in arrays else np.full((height, width), 255, np.uint8)
    return np.concatenate([rgb, alpha[:height, :width, None]], 2)


def etc1s_output_blocks(endpoint_palette, selector_palette, endpoint_idx, selector_idx):
    """the ETC1S blocks a frontend would hold for this state, as the backend reads them (differential, both halves equal, flip set): (n, 8) u8"""
    ep = np.asarray(endpoint_palette, np.int64)[np.asarray(endpoint_idx)]
    sel = np.asarray(selector_palette, np.int64)[np.asarray(selector_idx)]   # (n, 16): selector of texel y * 4 + x
    n = ep.shape[0]
    out = np.zeros((n, 8), np.uint8)
    out[:, 0], out[:, 1], out[:, 2] = ep[:, 0] << 3, ep[:, 1] << 3, ep[:, 2] << 3
    out[:, 3] = (ep[:, 3] << 5) | (ep[:, 3] << 2) | 3
    raw = np.array([3, 2, 0, 1])[sel]   # ascending selector -> ETC1 pixel index
    lo = np.zeros(n, np.int64)
    for x in range(4):
        for y in range(4):
            r = raw[:, y * 4 + x]
            lo |= ((r & 1) << (x * 4 + y)) | ((r >> 1) << (16 + x * 4 + y))
    for k in range(4):
        out[:, 4 + k] = (lo >> (8 * (3 - k))) & 255
    return out


def selectors_of_etc_blocks(blocks):
    """the inverse of etc1s_output_blocks' selector half: (k, 8) u8 ETC1 blocks -> (k, 16) ascending selectors, texel y * 4 + x"""
    b = np.ascontiguousarray(blocks, np.uint8).reshape(-1, 8).astype(np.int64)
    lo = (b[:, 4] << 24) | (b[:, 5] << 16) | (b[:, 6] << 8) | b[:, 7]
    out = np.zeros((b.shape[0], 16), np.uint8)
    for x in range(4):
        for y in range(4):
            raw = ((lo >> (x * 4 + y)) & 1) | (((lo >> (16 + x * 4 + y)) & 1) << 1)
            out[:, y * 4 + x] = np.array([2, 3, 1, 0])[raw]
    return out


def selector_palette_u32(selector_palette):
    """(k, 16) selectors -> the packed form decode_etc1s_file returns"""
    s = np.asarray(selector_palette, np.uint32)
    return (s << (2 * np.arange(16, dtype=np.uint32))[None, :]).sum(1).astype(np.uint32)


def backend_from_state(endpoint_palette, selector_palette, endpoint_idx, selector_idx, slices, **kw):
    """An Etc1sBackend (host only) over a synthetic state whose source pixels are exactly what the blocks decode to, with the RDO thresholds off: nothing gives the backend
    a reason to move a block to another palette entry, so the file codes the state as given (up to the palette renumbering the backend reports)."""
    from basis_universal_amd.backend import Etc1sBackend
    ep, sel = np.asarray(endpoint_palette, np.uint8), np.asarray(selector_palette, np.uint8)
    ei, si = np.asarray(endpoint_idx, np.uint32), np.asarray(selector_idx, np.uint32)
    base = (ep[ei, :3].astype(int) << 3) | (ep[ei, :3].astype(int) >> 2)
    px = np.clip(base[:, None, :] + INTEN[ep[ei, 3]][np.arange(ei.size)[:, None], sel[si]][:, :, None], 0, 255)
    src = np.concatenate([px, np.full((ei.size, 16, 1), 255)], 2).astype(np.uint8).reshape(-1, 4, 4, 4)
    sel_blocks = etc1s_output_blocks(np.zeros((1, 4), np.uint8), sel, np.zeros(sel.shape[0], np.int64), np.arange(sel.shape[0]))
    return Etc1sBackend.from_arrays(src, etc1s_output_blocks(ep, sel, ei, si), ei, si, ep, sel_blocks, slices, endpoint_rdo_thresh=0.0, selector_rdo_thresh=0.0, **kw)
