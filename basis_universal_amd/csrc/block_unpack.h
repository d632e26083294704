// block_unpack.h -- BC1 / BC3 / BC4 / BC5 / BC7 block decode core: one 8- or 16-byte block in, 16 RGBA8 texels out. What gpu_image::unpack shows of a texture
// this package transcoded (encoder/basisu_gpu_texture.cpp:984-1023 -> transcoder/basisu_dds_transcoder.inl:23-196, transcoder/basisu_transcoder.cpp:29790-30149),
// written from the formats' definitions.
//
// The unit is ONE TEXEL: unpack_texel_*(block bits, texel index) -> r | g << 8 | b << 16 | a << 24. The kernel gives a lane a texel, the unpack_block_* functions
// below call it sixteen times. A texel function indexes no array of its own by a run-time value (its one array, four channels, is walked by an unrolled loop) and reads tables only
// through a field that was masked to the table's size where it was extracted (a 6-bit partition field into 64 entries, a 2..4-bit index into a weight set).
//
//   BC1   565 endpoints with replicated high bits; low > high: four colours, thirds; else three colours, the mean, and index 3 = (0, 0, 0, 0) (set_alpha = true).
//   BC4   low > high: eight values, sevenths; else six values, fifths, then 0 and 255. R only: G = B = 0, A = 255 (gpu_image::unpack starts a texel at (0, 0, 0, 255)).
//   BC5   two BC4 blocks into R and G; B = 0, A = 255.
//   BC3   alpha from the BC4 half (bytes 0-7), colour from the BC1 half (bytes 8-15) in four-colour mode whatever the order of its endpoints.
//   BC7   all eight modes; the mode is the lowest set bit of byte 0. Byte 0 == 0 is the reserved mode and the only invalid block: the texel is 0 and *ok false.
//         (The reference returns false there and leaves whatever the caller's buffer held -- in gpu_image::unpack, the previous block's pixels. Not imitated.)
// Same convention as uastc_core.h: hipcc compiles it for block_unpack_kernels.hip, g++ for the test-only host library (tests/native).
#pragma once
#include "uastc_transcode.h"   // BU_FN / BU_TAB, ku_bc7_part2 / part3 / anchor2 / anchor3a / anchor3b, ku_weights, ku_bc7_weights4

namespace bu_unpack {

// the reference's transcoder_texture_format values of the formats that unpack here: a transcoder's target can be handed straight over
enum : uint32_t { UF_BC1 = 2, UF_BC3 = 3, UF_BC4 = 4, UF_BC5 = 5, UF_BC7 = 6 };

BU_FN_HD uint32_t unpack_bytes_per_block(uint32_t format) {   // 0: not a format that unpacks here
    return (format == UF_BC1 || format == UF_BC4) ? 8u : ((format == UF_BC3 || format == UF_BC5 || format == UF_BC7) ? 16u : 0u);
}

BU_FN uint32_t rgba(uint32_t r, uint32_t g, uint32_t b, uint32_t a) { return r | (g << 8) | (b << 16) | (a << 24); }

// ---- BC1: bytes 0-1 the low colour, 2-3 the high colour, 4-7 two selector bits per texel
BU_FN uint32_t unpack_texel_bc1(uint64_t blk, uint32_t i, bool force_four) {
    const uint32_t l = (uint32_t)blk & 0xFFFFu, h = (uint32_t)(blk >> 16) & 0xFFFFu, s = (uint32_t)(blk >> (32u + 2u * i)) & 3u;
    const bool four = force_four || l > h;
    if (!four && s == 3u) return 0u;
    uint32_t out = 0xFF000000u;
    BU_UNROLL
    for (uint32_t c = 0; c < 3; c++) {   // c = 0 red (bits 11-15), 1 green (5-10), 2 blue (0-4)
        const uint32_t sh = c == 0 ? 11u : (c == 1 ? 5u : 0u), bits = c == 1 ? 6u : 5u, mask = (1u << bits) - 1u;
        uint32_t a = (l >> sh) & mask, b = (h >> sh) & mask;
        a = (a << (8u - bits)) | (a >> (2u * bits - 8u));
        b = (b << (8u - bits)) | (b >> (2u * bits - 8u));
        const uint32_t v = s == 0u ? a : (s == 1u ? b : (four ? (s == 2u ? (2u * a + b) / 3u : (2u * b + a) / 3u) : (a + b) / 2u));
        out |= v << (8u * c);
    }
    return out;
}

// ---- BC4: byte 0 the low value, byte 1 the high value, 48 bits of three per texel
BU_FN uint32_t unpack_value_bc4(uint64_t blk, uint32_t i) {
    const uint32_t l = (uint32_t)blk & 255u, h = (uint32_t)(blk >> 8) & 255u, s = (uint32_t)(blk >> (16u + 3u * i)) & 7u;
    if (s == 0u) return l;
    if (s == 1u) return h;
    if (l > h) return ((8u - s) * l + (s - 1u) * h) / 7u;
    if (s >= 6u) return s == 6u ? 0u : 255u;
    return ((6u - s) * l + (s - 1u) * h) / 5u;
}

// ---- BC7
// 128 bits as two words; `n` (0..8) bits from bit `pos` (0..127; bits past 127 read as 0)
BU_FN uint32_t bits_at(uint64_t lo, uint64_t hi, uint32_t pos, uint32_t n) {
    uint64_t v;
    if (pos >= 64u) v = hi >> (pos - 64u);
    else v = pos ? ((lo >> pos) | (hi << (64u - pos))) : lo;
    return (uint32_t)v & ((1u << n) - 1u);
}
// `bits` raw bits (plus a p-bit under them when has_p) widened to 8 by replicating the high bits
BU_FN uint32_t bc7_widen(uint32_t v, uint32_t bits, bool has_p, uint32_t p) {
    if (has_p) { v = (v << 1) | p; bits++; }
    v <<= 8u - bits;
    return v | (v >> bits);
}
BU_FN uint32_t bc7_weight(uint32_t bits, uint32_t idx) {   // idx < 1 << bits by how it was read
    return bits == 4u ? ku_bc7_weights4[idx & 15u] : ku_weights[((1u << bits) - 2u) + (idx & ((1u << bits) - 1u))];
}
BU_FN uint32_t bc7_lerp8(uint32_t a, uint32_t b, uint32_t w) { return (a * (64u - w) + b * w + 32u) >> 6; }

// The fields of a mode as one word: subsets | partition bits << 2 | colour bits << 5 | alpha bits << 9 | p-bits (0 none, 1 per endpoint, 2 per subset) << 13 |
// index bits << 15 | second index bits << 18 | rotation (modes 4, 5) << 20 | index selection bit (mode 4) << 21
#define BU_BC7_MODE(ns, pb, cb, ab, pt, ib, ib2, rot, isb) ((ns) | ((pb) << 2) | ((cb) << 5) | ((ab) << 9) | ((pt) << 13) | ((ib) << 15) | ((ib2) << 18) | ((rot) << 20) | ((isb) << 21))
BU_FN uint32_t bc7_mode_fields(uint32_t mode) {
    switch (mode) {
    case 0: return BU_BC7_MODE(3u, 4u, 4u, 0u, 1u, 3u, 0u, 0u, 0u);
    case 1: return BU_BC7_MODE(2u, 6u, 6u, 0u, 2u, 3u, 0u, 0u, 0u);
    case 2: return BU_BC7_MODE(3u, 6u, 5u, 0u, 0u, 2u, 0u, 0u, 0u);
    case 3: return BU_BC7_MODE(2u, 6u, 7u, 0u, 1u, 2u, 0u, 0u, 0u);
    case 4: return BU_BC7_MODE(1u, 0u, 5u, 6u, 0u, 2u, 3u, 1u, 1u);
    case 5: return BU_BC7_MODE(1u, 0u, 7u, 8u, 0u, 2u, 2u, 1u, 0u);
    case 6: return BU_BC7_MODE(1u, 0u, 7u, 7u, 1u, 4u, 0u, 0u, 0u);
    default: return BU_BC7_MODE(2u, 6u, 5u, 5u, 1u, 2u, 0u, 0u, 0u);
    }
}
#undef BU_BC7_MODE

BU_FN uint32_t unpack_texel_bc7(uint64_t lo, uint64_t hi, uint32_t i, bool* ok) {
    const uint32_t first = (uint32_t)lo & 255u;
    *ok = first != 0u;
    if (!first) return 0u;
    const uint32_t mode = (uint32_t)__builtin_ctz(first);   // 0..7: the byte is not 0
    const uint32_t f = bc7_mode_fields(mode);
    const uint32_t ns = f & 3u, pb = (f >> 2) & 7u, cb = (f >> 5) & 15u, ab = (f >> 9) & 15u, pt = (f >> 13) & 3u, ib = (f >> 15) & 7u, ib2 = (f >> 18) & 3u;
    uint32_t pos = mode + 1u;
    const uint32_t rot = ((f >> 20) & 1u) ? bits_at(lo, hi, pos, 2) : 0u;
    pos += ((f >> 20) & 1u) * 2u;
    const uint32_t isel = ((f >> 21) & 1u) ? bits_at(lo, hi, pos, 1) : 0u;
    pos += (f >> 21) & 1u;
    const uint32_t part = bits_at(lo, hi, pos, pb);   // < 64 (16 in mode 0) by the mask
    pos += pb;
    // subset of this texel and the anchor texels of the partition (texel 0 always is one)
    uint32_t s = 0, a1 = 16u, a2 = 16u;
    if (ns == 2u) { s = (ku_bc7_part2[part] >> (2u * i)) & 3u; a1 = ku_bc7_anchor2[part]; }
    else if (ns == 3u) { s = (ku_bc7_part3[part] >> (2u * i)) & 3u; a1 = ku_bc7_anchor3a[part]; a2 = ku_bc7_anchor3b[part]; }
    // endpoints: per channel, every endpoint's value in turn (endpoint 2s is the subset's low end, 2s + 1 its high end); then the p-bits
    const uint32_t ne = 2u * ns, alpha_at = pos + 3u * ne * cb, p_at = alpha_at + ne * ab;
    const uint32_t np = pt == 1u ? ne : (pt == 2u ? ns : 0u);
    const uint32_t p_lo = pt ? bits_at(lo, hi, p_at + (pt == 1u ? 2u * s : s), 1) : 0u, p_hi = pt == 1u ? bits_at(lo, hi, p_at + 2u * s + 1u, 1) : p_lo;
    // indices: texel i's sits i * bits past the first, less one bit per anchor before it, and is a bit short when it is an anchor itself
    const uint32_t i_at = p_at + np;
    const uint32_t before = (i > 0u ? 1u : 0u) + (i > a1 ? 1u : 0u) + (i > a2 ? 1u : 0u), anchor = (i == 0u || i == a1 || i == a2) ? 1u : 0u;
    const uint32_t idx0 = bits_at(lo, hi, i_at + i * ib - before, ib - anchor);
    uint32_t cbits = ib, cidx = idx0, abits = ib, aidx = idx0;
    if (ib2) {   // modes 4, 5: a second index set after the 31 bits of the first; mode 4's selection bit gives the colour the wider one
        const uint32_t idx1 = bits_at(lo, hi, i_at + 16u * ib - 1u + i * ib2 - (i > 0u ? 1u : 0u), ib2 - (i == 0u ? 1u : 0u));
        if (isel) { cbits = ib2; cidx = idx1; abits = ib; aidx = idx0; }
        else { abits = ib2; aidx = idx1; }
    }
    const uint32_t cw = bc7_weight(cbits, cidx), aw = bc7_weight(abits, aidx);
    uint32_t v[4];
    BU_UNROLL
    for (uint32_t c = 0; c < 3; c++) {
        const uint32_t at = pos + (c * ne + 2u * s) * cb;
        v[c] = bc7_lerp8(bc7_widen(bits_at(lo, hi, at, cb), cb, pt != 0u, p_lo), bc7_widen(bits_at(lo, hi, at + cb, cb), cb, pt != 0u, p_hi), cw);
    }
    v[3] = 255u;
    if (ab) {
        const uint32_t at = alpha_at + 2u * s * ab;
        v[3] = bc7_lerp8(bc7_widen(bits_at(lo, hi, at, ab), ab, pt != 0u, p_lo), bc7_widen(bits_at(lo, hi, at + ab, ab), ab, pt != 0u, p_hi), aw);
    }
    // rotation: alpha trades places with red, green or blue
    const uint32_t r = rot == 1u ? v[3] : v[0], g = rot == 2u ? v[3] : v[1], b = rot == 3u ? v[3] : v[2], a = rot == 1u ? v[0] : (rot == 2u ? v[1] : (rot == 3u ? v[2] : v[3]));
    return rgba(r, g, b, a);
}

// ---- one texel of any of the five formats. lo = bytes 0-7, hi = bytes 8-15 (unused by BC1, BC4)
template <uint32_t FORMAT>
BU_FN uint32_t unpack_texel(uint64_t lo, uint64_t hi, uint32_t i, bool* ok) {
    *ok = true;
    if (FORMAT == UF_BC1) return unpack_texel_bc1(lo, i, false);
    if (FORMAT == UF_BC4) return rgba(unpack_value_bc4(lo, i), 0u, 0u, 255u);
    if (FORMAT == UF_BC5) return rgba(unpack_value_bc4(lo, i), unpack_value_bc4(hi, i), 0u, 255u);
    if (FORMAT == UF_BC3) return (unpack_texel_bc1(hi, i, true) & 0x00FFFFFFu) | (unpack_value_bc4(lo, i) << 24);
    return unpack_texel_bc7(lo, hi, i, ok);
}

BU_FN uint64_t load64(const uint8_t* p) {
    uint64_t v = 0;
    for (uint32_t k = 0; k < 8; k++) v |= (uint64_t)p[k] << (8u * k);
    return v;
}

// ---- one block: 16 texels in raster order, 4 bytes each (R, G, B, A). False (and zeros) only for a BC7 block whose first byte is 0.
template <uint32_t FORMAT>
BU_FN bool unpack_block(const uint8_t* blk, uint8_t* out64) {
    const uint64_t lo = load64(blk), hi = unpack_bytes_per_block(FORMAT) == 16u ? load64(blk + 8) : 0ull;
    bool all = true;
    for (uint32_t i = 0; i < 16; i++) {
        bool ok;
        const uint32_t px = unpack_texel<FORMAT>(lo, hi, i, &ok);
        all = all && ok;
        for (uint32_t k = 0; k < 4; k++) out64[i * 4 + k] = (uint8_t)(px >> (8u * k));
    }
    return all;
}
BU_FN bool unpack_block_bc1(const uint8_t* blk, uint8_t* out64) { return unpack_block<UF_BC1>(blk, out64); }
BU_FN bool unpack_block_bc3(const uint8_t* blk, uint8_t* out64) { return unpack_block<UF_BC3>(blk, out64); }
BU_FN bool unpack_block_bc4(const uint8_t* blk, uint8_t* out64) { return unpack_block<UF_BC4>(blk, out64); }
BU_FN bool unpack_block_bc5(const uint8_t* blk, uint8_t* out64) { return unpack_block<UF_BC5>(blk, out64); }
BU_FN bool unpack_block_bc7(const uint8_t* blk, uint8_t* out64) { return unpack_block<UF_BC7>(blk, out64); }

}  // namespace bu_unpack
