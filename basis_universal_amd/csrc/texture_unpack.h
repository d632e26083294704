// texture_unpack.h -- the block decode core of the texture unpacker: every block format this package's transcoders write, back to RGBA8. The five BC formats are
// block_unpack.h's, included and not restated; this file adds ETC1, ETC2 RGBA, EAC R11 / RG11, ASTC 4x4 (LDR, L8 decode profile) and PVRTC1 4bpp. What a texel is
// is pinned by the reference's gpu_image::unpack (encoder/basisu_gpu_texture.cpp:984-1240 -> encoder/basisu_etc.cpp:604, basisu_gpu_texture.cpp:121 / :936,
// encoder/3rdparty/android_astc_decomp.cpp decompress_ldr, encoder/basisu_pvrtc1_4.cpp:238-379); everything here is written from the formats' definitions.
//
// The unit is ONE TEXEL, as in block_unpack.h: unpack_texel_*(block bits, texel index) -> r | g << 8 | b << 16 | a << 24. No array is indexed by a run-time value:
// the few arrays (four channels, eight endpoint values) are walked by unrolled loops, and the one table (ku_eac_tables) is read through masked fields.
//
//   ETC1    bytes 0-2 the colours (individual: two 4-bit bases per channel; differential: a 5-bit base and a signed 3-bit delta), byte 3 the two intensity tables,
//           the diff and the flip bit, bytes 4-7 the selector planes, texel (x, y) at bit x * 4 + y. A differential base that leaves 0..31 in any channel is one of
//           ETC2's T / H / planar encodings, which the reference does not decode: the whole block is invalid (texels 0, *ok false). A = 255.
//   ETC2    bytes 0-7 an EAC A8 block (base, multiplier | table, 48 selector bits, texel (x, y) at bit 45 - 3 (x * 4 + y) of the big-endian field):
//           clamp255(base + table[s] * multiplier); bytes 8-15 ETC1. An invalid colour half zeroes alpha too.
//   R11     the same block read at 11 bits: clamp(base * 8 + 4 + table[s] * (multiplier ? multiplier * 8 : 1), 0, 2047), to 8 bits as (v * 255 + 1023) / 2047;
//           G = B = 0, A = 255. RG11: two of them into R and G. Never invalid.
//   ASTC    see the section below: void extent, every block mode a 4x4 footprint admits, BISE bits / trits / quints, 1-4 partitions, dual plane, the ten LDR
//           endpoint modes. A lane decodes only the BISE groups that hold its own weights and its own partition's endpoint values. A channel is the top 8 bits
//           of the UNORM16 interpolation (endpoints widened as c * 257). Invalid where the reference's decoder refuses the block.
//   PVRTC1  texel (x, y) lies between the 5554 endpoints of the 2x2 blocks around it (the caller wraps them at the edges and resolves Morton order):
//           bilinear weights u = (x + 2) & 3, v = (y + 2) & 3, then the block's own 2-bit modulation value under its mode bit M. Never invalid.
// Same convention as block_unpack.h: hipcc compiles it for texture_unpack_kernels.hip, g++ for the test-only host library and tools/texture_unpack_sanitize.cpp.
#pragma once
#include "block_unpack.h"
#include "pvrtc1.h"   // morton_address

namespace bu_unpack {

// the reference's transcoder_texture_format values of the formats this file adds
enum : uint32_t { UF_ETC1 = 0, UF_ETC2_RGBA = 1, UF_PVRTC1_RGB = 8, UF_PVRTC1_RGBA = 9, UF_ASTC_4x4 = 10, UF_EAC_R11 = 20, UF_EAC_RG11 = 21 };

BU_FN_HD bool texture_format_is_pvrtc1(uint32_t format) { return format == UF_PVRTC1_RGB || format == UF_PVRTC1_RGBA; }
BU_FN_HD uint32_t texture_bytes_per_block(uint32_t format) {   // 0: not a format that unpacks here
    if (format == UF_ETC1 || format == UF_EAC_R11 || texture_format_is_pvrtc1(format)) return 8u;
    if (format == UF_ETC2_RGBA || format == UF_EAC_RG11 || format == UF_ASTC_4x4) return 16u;
    return unpack_bytes_per_block(format);
}

BU_FN uint32_t clamp255(int v) { return v < 0 ? 0u : (v > 255 ? 255u : (uint32_t)v); }

// ---- ETC1
BU_FN int etc1_modifier(uint32_t table, uint32_t msb, uint32_t lsb) {   // the eight tables' small and large step as bytes of two words; msb = the sign
    const int small = (int)((0x2F2118120D090502ull >> (8u * table)) & 255u), large = (int)((0xB76A503C2A1D1108ull >> (8u * table)) & 255u);
    const int step = lsb ? large : small;
    return msb ? -step : step;
}
BU_FN uint32_t unpack_texel_etc1(uint64_t blk, uint32_t i, bool* ok) {
    const uint32_t x = i & 3u, y = i >> 2, flags = (uint32_t)(blk >> 24) & 255u;
    const bool flip = (flags & 1u) != 0u, diff = (flags & 2u) != 0u;
    const bool second = ((flip ? y : x) >> 1) != 0u;
    const uint32_t table = (flags >> (second ? 2u : 5u)) & 7u;
    const uint32_t n = x * 4u + y, plane = 8u * (1u - (n >> 3)) + (n & 7u);   // bit n of a 16-bit big-endian plane: bytes 5 | 4 the high bits, 7 | 6 the low ones
    const int mod = etc1_modifier(table, (uint32_t)(blk >> (32u + plane)) & 1u, (uint32_t)(blk >> (48u + plane)) & 1u);
    uint32_t out = 0xFF000000u;
    bool valid = true;
    BU_UNROLL
    for (uint32_t c = 0; c < 3; c++) {
        const uint32_t byte = (uint32_t)(blk >> (8u * c)) & 255u;
        uint32_t base;
        if (diff) {
            const int b5 = (int)(byte >> 3), d = (int)(byte & 7u) - (int)((byte & 4u) << 1), s5 = b5 + d;
            valid = valid && s5 >= 0 && s5 <= 31;
            const uint32_t v5 = second ? (uint32_t)(s5 & 31) : (uint32_t)b5;
            base = (v5 << 3) | (v5 >> 2);
        } else {
            base = (second ? (byte & 15u) : (byte >> 4)) * 17u;
        }
        out |= clamp255((int)base + mod) << (8u * c);
    }
    *ok = valid;
    return valid ? out : 0u;
}

// ---- EAC: byte 0 the base, byte 1 multiplier << 4 | table, bytes 2-7 sixteen 3-bit selectors, big-endian, texel (x, y) at bit 45 - 3 (x * 4 + y)
BU_FN int eac_step(uint64_t blk, uint32_t i) {
    const uint32_t table = (uint32_t)(blk >> 8) & 15u, n = (i & 3u) * 4u + (i >> 2);
    const uint32_t s = (uint32_t)((__builtin_bswap64(blk) & 0xFFFFFFFFFFFFull) >> (45u - 3u * n)) & 7u;
    return (int)ku_eac_tables[table * 8u + s];
}
BU_FN uint32_t unpack_value_eac_a8(uint64_t blk, uint32_t i) {
    return clamp255((int)((uint32_t)blk & 255u) + eac_step(blk, i) * (int)((uint32_t)(blk >> 12) & 15u));
}
BU_FN uint32_t unpack_value_eac_r11(uint64_t blk, uint32_t i) {
    const int mul = (int)((uint32_t)(blk >> 12) & 15u);
    int v = (int)((uint32_t)blk & 255u) * 8 + 4 + eac_step(blk, i) * (mul ? mul * 8 : 1);
    v = v < 0 ? 0 : (v > 2047 ? 2047 : v);
    return ((uint32_t)v * 255u + 1023u) / 2047u;
}

// ---- ASTC 4x4, LDR, the L8 (non-sRGB) decode profile.
// Layout of a block (128 bits, bit 0 first): 11 bits of block mode, 2 of partition count - 1, then for one partition the 4-bit endpoint mode (CEM) at 13 and the
// endpoint values from 17; for more a 10-bit partition seed at 13, a 6-bit CEM field at 23 (selector 0: one CEM for all at 25; else a class bit per partition and
// two low bits per partition, which spill into the bits under the weights) and the endpoint values from 29. The weights are read from bit 127 downwards; under
// them sit the spilled CEM bits and under those the two bits of the dual plane's channel. The endpoint values use the widest BISE range that fits what is left.
// A BISE sequence is `n` plain bits per value, plus per five values 8 bits of packed trits, or per three values 7 bits of packed quints, interleaved with them.

// `n` (0..8) bits from bit `pos` of lo | hi << 64; bits past 127 read as 0
BU_FN uint32_t astc_bits(uint64_t lo, uint64_t hi, uint32_t pos, uint32_t n) { return pos >= 128u ? 0u : bits_at(lo, hi, pos, n); }
BU_FN uint64_t reverse64(uint64_t v) {
    v = ((v >> 1) & 0x5555555555555555ull) | ((v & 0x5555555555555555ull) << 1);
    v = ((v >> 2) & 0x3333333333333333ull) | ((v & 0x3333333333333333ull) << 2);
    v = ((v >> 4) & 0x0F0F0F0F0F0F0F0Full) | ((v & 0x0F0F0F0F0F0F0F0Full) << 4);
    return __builtin_bswap64(v);
}
// the low `n` (0..128) bits of (lo | hi << 64) >> by (by < 64)
BU_FN void astc_window(uint64_t& lo, uint64_t& hi, uint32_t by, uint32_t n) {
    if (by) { lo = (lo >> by) | (hi << (64u - by)); hi >>= by; }
    if (n < 64u) { lo &= (1ull << n) - 1ull; hi = 0; }
    else if (n < 128u) hi &= (1ull << (n - 64u)) - 1ull;
}

enum : uint32_t { ISE_BITS = 0, ISE_TRITS = 1, ISE_QUINTS = 2 };
BU_FN uint32_t ise_sequence_bits(uint32_t kind, uint32_t n, uint32_t values) {
    return values * n + (kind == ISE_TRITS ? (values * 8u + 4u) / 5u : (kind == ISE_QUINTS ? (values * 7u + 2u) / 3u : 0u));
}
// value k of a BISE sequence that starts at bit 0 of lo | hi << 64 and was cut to its length (bits past it are 0, which is also how a short last group reads):
// -> its plain bits; *tq its trit or quint
BU_FN uint32_t ise_value(uint64_t lo, uint64_t hi, uint32_t kind, uint32_t n, uint32_t k, uint32_t* tq) {
    if (kind == ISE_TRITS) {   // m0 T01 m1 T23 m2 T4 m3 T56 m4 T7
        const uint32_t g = k / 5u, j = k - g * 5u, at = g * (5u * n + 8u);
        const uint32_t T = astc_bits(lo, hi, at + n, 2) | (astc_bits(lo, hi, at + 2u * n + 2u, 2) << 2) | (astc_bits(lo, hi, at + 3u * n + 4u, 1) << 4) |
                           (astc_bits(lo, hi, at + 4u * n + 5u, 2) << 5) | (astc_bits(lo, hi, at + 5u * n + 7u, 1) << 7);
        uint32_t C, t0, t1, t2, t3, t4;
        if (((T >> 2) & 7u) == 7u) { C = (((T >> 5) & 7u) << 2) | (T & 3u); t4 = t3 = 2u; }
        else {
            C = T & 31u;
            if (((T >> 5) & 3u) == 3u) { t4 = 2u; t3 = (T >> 7) & 1u; }
            else { t4 = (T >> 7) & 1u; t3 = (T >> 5) & 3u; }
        }
        if ((C & 3u) == 3u) { t2 = 2u; t1 = (C >> 4) & 1u; t0 = (((C >> 3) & 1u) << 1) | (((C >> 2) & 1u) & ~((C >> 3) & 1u)); }
        else if (((C >> 2) & 3u) == 3u) { t2 = 2u; t1 = 2u; t0 = C & 3u; }
        else { t2 = (C >> 4) & 1u; t1 = (C >> 2) & 3u; t0 = (((C >> 1) & 1u) << 1) | ((C & 1u) & ~((C >> 1) & 1u)); }
        *tq = j == 0u ? t0 : (j == 1u ? t1 : (j == 2u ? t2 : (j == 3u ? t3 : t4)));
        return astc_bits(lo, hi, at + j * n + (j == 0u ? 0u : (j == 1u ? 2u : (j == 2u ? 4u : (j == 3u ? 5u : 7u)))), n);
    }
    if (kind == ISE_QUINTS) {   // m0 Q012 m1 Q34 m2 Q56
        const uint32_t g = k / 3u, j = k - g * 3u, at = g * (3u * n + 7u);
        const uint32_t Q = astc_bits(lo, hi, at + n, 3) | (astc_bits(lo, hi, at + 2u * n + 3u, 2) << 3) | (astc_bits(lo, hi, at + 3u * n + 5u, 2) << 5);
        uint32_t q0, q1, q2;
        if (((Q >> 1) & 3u) == 3u && ((Q >> 5) & 3u) == 0u) {
            const uint32_t not0 = ~Q & 1u;
            q2 = ((Q & 1u) << 2) | ((((Q >> 4) & 1u) & not0) << 1) | (((Q >> 3) & 1u) & not0);
            q1 = q0 = 4u;
        } else {
            uint32_t C;
            if (((Q >> 1) & 3u) == 3u) { q2 = 4u; C = (((Q >> 3) & 3u) << 3) | ((~(Q >> 5) & 3u) << 1) | (Q & 1u); }
            else { q2 = (Q >> 5) & 3u; C = Q & 31u; }
            if ((C & 7u) == 5u) { q1 = 4u; q0 = (C >> 3) & 3u; }
            else { q1 = (C >> 3) & 3u; q0 = C & 7u; }
        }
        *tq = j == 0u ? q0 : (j == 1u ? q1 : q2);
        return astc_bits(lo, hi, at + j * n + (j == 0u ? 0u : (j == 1u ? 3u : 5u)), n);
    }
    *tq = 0u;
    return astc_bits(lo, hi, k * n, n);
}

BU_FN uint32_t replicate_bits(uint32_t v, uint32_t from, uint32_t to) {   // 1 <= from <= to <= 8
    uint32_t out = 0;
    for (int s = (int)to - (int)from; s > -(int)from; s -= (int)from) out |= s >= 0 ? v << s : v >> -s;
    return out;
}

// an endpoint value to 0..255
BU_FN uint32_t astc_unquant_endpoint(uint32_t kind, uint32_t n, uint32_t m, uint32_t tq) {
    if (kind == ISE_BITS) return replicate_bits(m, n, 8);
    const uint32_t b = (m >> 1) & 1u, c = (m >> 2) & 1u, d = (m >> 3) & 1u, e = (m >> 4) & 1u, f = (m >> 5) & 1u, A = (m & 1u) ? 511u : 0u;
    uint32_t B = 0, C = 0;
    switch (n * 2u - (kind == ISE_TRITS ? 2u : 1u)) {   // trits with 1..6 bits: 0, 2, .., 10; quints with 1..5: 1, 3, .., 9
    case 0: C = 204u; break;
    case 1: C = 113u; break;
    case 2: C = 93u; B = (b << 8) | (b << 4) | (b << 2) | (b << 1); break;
    case 3: C = 54u; B = (b << 8) | (b << 3) | (b << 2); break;
    case 4: C = 44u; B = (c << 8) | (b << 7) | (c << 3) | (b << 2) | (c << 1) | b; break;
    case 5: C = 26u; B = (c << 8) | (b << 7) | (c << 2) | (b << 1) | c; break;
    case 6: C = 22u; B = (d << 8) | (c << 7) | (b << 6) | (d << 2) | (c << 1) | b; break;
    case 7: C = 13u; B = (d << 8) | (c << 7) | (b << 6) | (d << 1) | c; break;
    case 8: C = 11u; B = (e << 8) | (d << 7) | (c << 6) | (b << 5) | (e << 1) | d; break;
    case 9: C = 6u; B = (e << 8) | (d << 7) | (c << 6) | (b << 5) | e; break;
    default: C = 5u; B = (f << 8) | (e << 7) | (d << 6) | (c << 5) | (b << 4) | f; break;
    }
    return (((tq * C + B) ^ A) >> 2) | (A & 0x80u);
}
// a weight to 0..64
BU_FN uint32_t astc_unquant_weight(uint32_t kind, uint32_t n, uint32_t m, uint32_t tq) {
    uint32_t w;
    if (kind == ISE_BITS) w = replicate_bits(m, n, 6);
    else if (n == 0u) w = kind == ISE_TRITS ? (tq == 0u ? 0u : (tq == 1u ? 32u : 63u)) : (tq == 0u ? 0u : (tq == 1u ? 16u : (tq == 2u ? 32u : (tq == 3u ? 47u : 63u))));
    else {
        const uint32_t b = (m >> 1) & 1u, c = (m >> 2) & 1u, A = (m & 1u) ? 127u : 0u;
        uint32_t B = 0, C;
        switch (n * 2u + (kind == ISE_QUINTS ? 1u : 0u)) {   // trits with 1..3 bits: 2, 4, 6; quints with 1, 2: 3, 5
        case 2: C = 50u; break;
        case 3: C = 28u; break;
        case 4: C = 23u; B = (b << 6) | (b << 2) | b; break;
        case 5: C = 13u; B = (b << 6) | (b << 1); break;
        default: C = 11u; B = (c << 6) | (b << 5) | (c << 1) | b; break;
        }
        w = (((tq * C + B) ^ A) >> 2) | (A & 0x20u);
    }
    return w + (w > 32u ? 1u : 0u);
}

// The partition function's per-block half: the squared, shifted seeds as eight nibble-wide fields of one word each way (x: s1 s3 s5 s7, y: s2 s4 s6 s8) and the
// hash. A 4x4 block is a "small block": coordinates are doubled.
struct astc_partition_seeds { uint32_t sx, sy, rnum; };
BU_FN astc_partition_seeds astc_seeds(uint32_t seed10, uint32_t parts) {
    const uint32_t seed = seed10 + 1024u * (parts - 1u);
    uint32_t p = seed;
    p ^= p >> 15; p -= p << 17; p += p << 7; p += p << 4;
    p ^= p >> 5; p += p << 16; p ^= p >> 7; p ^= p >> 3;
    p ^= p << 6; p ^= p >> 17;
    const uint32_t shA = (seed & 2u) ? 4u : 5u, shB = parts == 3u ? 6u : 5u, sh1 = (seed & 1u) ? shA : shB, sh2 = (seed & 1u) ? shB : shA;
    astc_partition_seeds s = { 0u, 0u, p };
    BU_UNROLL
    for (uint32_t k = 0; k < 4; k++) {   // seeds 2k + 1 (x) and 2k + 2 (y): a nibble squared, as a byte, shifted down
        const uint32_t a = (p >> (8u * k)) & 15u, b = (p >> (8u * k + 4u)) & 15u;
        s.sx |= (((a * a) & 255u) >> sh1) << (8u * k);
        s.sy |= (((b * b) & 255u) >> sh2) << (8u * k);
    }
    return s;
}
BU_FN uint32_t astc_partition_of(const astc_partition_seeds& s, uint32_t parts, uint32_t x, uint32_t y) {
    x <<= 1; y <<= 1;
    const uint32_t a = 63u & ((s.sx & 255u) * x + (s.sy & 255u) * y + (s.rnum >> 14));
    const uint32_t b = 63u & (((s.sx >> 8) & 255u) * x + ((s.sy >> 8) & 255u) * y + (s.rnum >> 10));
    const uint32_t c = parts >= 3u ? 63u & (((s.sx >> 16) & 255u) * x + ((s.sy >> 16) & 255u) * y + (s.rnum >> 6)) : 0u;
    const uint32_t d = parts >= 4u ? 63u & ((s.sx >> 24) * x + (s.sy >> 24) * y + (s.rnum >> 2)) : 0u;
    return (a >= b && a >= c && a >= d) ? 0u : ((b >= c && b >= d) ? 1u : (c >= d ? 2u : 3u));
}

BU_FN void astc_bit_transfer(int& a, int& b) {   // bit 7 of a moves to the top of b; a becomes a signed 6-bit delta
    b = (b >> 1) | (a & 0x80);
    a = (a >> 1) & 0x3F;
    if (a & 0x20) a -= 0x40;
}
BU_FN int astc_clamp8(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

// The two endpoints of one partition from its unquantised values v[0 .. 2 * (mode / 4 + 1)), LDR modes only. lo[c] / hi[c]: c = 0 red .. 3 alpha.
BU_FN void astc_endpoints(uint32_t mode, const uint32_t v[8], int lo[4], int hi[4]) {
    int a0 = (int)v[0], a1 = (int)v[1], a2 = (int)v[2], a3 = (int)v[3], a4 = (int)v[4], a5 = (int)v[5], a6 = (int)v[6], a7 = (int)v[7];
    bool contract = false;   // blue contraction: the endpoints trade places and red, green move half way to blue
    lo[3] = hi[3] = 255;
    switch (mode) {
    case 0: lo[0] = lo[1] = lo[2] = a0; hi[0] = hi[1] = hi[2] = a1; break;
    case 1: {
        const int l0 = (a0 >> 2) | (a1 & 0xC0), l1 = l0 + (a1 & 0x3F);
        lo[0] = lo[1] = lo[2] = l0; hi[0] = hi[1] = hi[2] = l1 > 255 ? 255 : l1;
        break;
    }
    case 4: lo[0] = lo[1] = lo[2] = a0; hi[0] = hi[1] = hi[2] = a1; lo[3] = a2; hi[3] = a3; break;
    case 5:
        astc_bit_transfer(a1, a0); astc_bit_transfer(a3, a2);
        lo[0] = lo[1] = lo[2] = astc_clamp8(a0); hi[0] = hi[1] = hi[2] = astc_clamp8(a0 + a1); lo[3] = astc_clamp8(a2); hi[3] = astc_clamp8(a2 + a3);
        break;
    case 6: case 10:
        lo[0] = (a0 * a3) >> 8; lo[1] = (a1 * a3) >> 8; lo[2] = (a2 * a3) >> 8; hi[0] = a0; hi[1] = a1; hi[2] = a2;
        if (mode == 10u) { lo[3] = a4; hi[3] = a5; }
        break;
    case 8: case 12:
        contract = a1 + a3 + a5 < a0 + a2 + a4;
        lo[0] = a0; lo[1] = a2; lo[2] = a4; hi[0] = a1; hi[1] = a3; hi[2] = a5;
        if (mode == 12u) { lo[3] = a6; hi[3] = a7; }
        break;
    default:   // 9, 13
        astc_bit_transfer(a1, a0); astc_bit_transfer(a3, a2); astc_bit_transfer(a5, a4);
        contract = a1 + a3 + a5 < 0;
        lo[0] = a0; lo[1] = a2; lo[2] = a4; hi[0] = a0 + a1; hi[1] = a2 + a3; hi[2] = a4 + a5;
        if (mode == 13u) { astc_bit_transfer(a7, a6); lo[3] = a6; hi[3] = a6 + a7; }
        break;
    }
    if (contract) {
        BU_UNROLL
        for (uint32_t c = 0; c < 4; c++) {
            int t = lo[c]; lo[c] = hi[c]; hi[c] = t;
        }
        lo[0] = (lo[0] + lo[2]) >> 1; lo[1] = (lo[1] + lo[2]) >> 1;
        hi[0] = (hi[0] + hi[2]) >> 1; hi[1] = (hi[1] + hi[2]) >> 1;
    }
    BU_UNROLL
    for (uint32_t c = 0; c < 4; c++) { lo[c] = astc_clamp8(lo[c]); hi[c] = astc_clamp8(hi[c]); }
}

BU_FN uint32_t astc_values_of_mode(uint32_t mode) { return ((mode >> 2) + 1u) * 2u; }
BU_FN bool astc_mode_is_hdr(uint32_t mode) { return ((0xC88Cu >> mode) & 1u) != 0u; }   // 2, 3, 7, 11, 14, 15

BU_FN uint32_t unpack_texel_astc(uint64_t lo, uint64_t hi, uint32_t i, bool* ok) {
    *ok = false;
    const uint32_t bm = (uint32_t)lo & 0x7FFu;
    if ((bm & 0x1FFu) == 0x1FCu) {   // void extent: bit 9 is the HDR flag, bits 10, 11 are 1, four 13-bit extents (all ones, or low < high both ways), four UNORM16 channels
        const uint32_t s0 = (uint32_t)(lo >> 12) & 0x1FFFu, s1 = (uint32_t)(lo >> 25) & 0x1FFFu, t0 = (uint32_t)(lo >> 38) & 0x1FFFu, t1 = (uint32_t)(lo >> 51) & 0x1FFFu;
        const bool all_ones = (s0 & s1 & t0 & t1) == 0x1FFFu;
        if (((bm >> 10) & 1u) == 0u || ((uint32_t)(lo >> 11) & 1u) == 0u || ((bm >> 9) & 1u) || (!all_ones && (s0 >= s1 || t0 >= t1))) return 0u;
        *ok = true;
        return rgba((uint32_t)(hi >> 8) & 255u, (uint32_t)(hi >> 24) & 255u, (uint32_t)(hi >> 40) & 255u, (uint32_t)(hi >> 56) & 255u);
    }
    // block mode: of the layouts, a 4x4 footprint admits only the two whose grid can be 4 wide and 4 high or less (bits 0-1 != 0, bits 2-3 == 0 or 3)
    if ((bm & 3u) == 0u) return 0u;   // reserved, or a grid at least 6 one way
    const uint32_t layout = (bm >> 2) & 3u, fa = (bm >> 5) & 3u, fb = (bm >> 7) & 3u;
    uint32_t gw, gh;
    if (layout == 0u) { gw = fb + 4u; gh = fa + 2u; }
    else if (layout == 3u && (fb & 2u)) { gw = (fb & 1u) + 2u; gh = fa + 2u; }
    else return 0u;   // 8 or more wide or high, or 6 or 7 high
    if (gw > 4u || gh > 4u) return 0u;
    const uint32_t r = ((bm >> 4) & 1u) | ((bm & 3u) << 1), high = (bm >> 9) & 1u, dual = (bm >> 10) & 1u;   // r = 2..7
    // weight range: r = 2, 3, 4 are 1 bit / trits / 2 bits, r = 5, 6, 7 quints / trits + 1 bit / 3 bits; the high-precision bit adds what makes 2..5 bits, 1..3 on trits, 1..2 on quints
    const uint32_t wkind = (r == 3u || r == 6u) ? ISE_TRITS : ((r == 2u && high) || r == 5u ? ISE_QUINTS : ISE_BITS);
    uint32_t wn;
    if (wkind == ISE_BITS) wn = (r == 2u ? 1u : (r == 4u ? 2u : 3u)) + (high ? 2u : 0u);
    else if (wkind == ISE_TRITS) wn = (r == 6u ? 1u : 0u) + (high ? 2u : 0u);
    else wn = r == 2u ? 1u : (high ? 2u : 0u);
    const uint32_t planes = dual + 1u, weights = gw * gh * planes, wbits = ise_sequence_bits(wkind, wn, weights);
    const uint32_t parts = ((uint32_t)(lo >> 11) & 3u) + 1u;
    if (wbits > 96u || wbits < 24u || (parts == 4u && dual)) return 0u;
    // endpoint modes
    const uint32_t selector = parts == 1u ? 0u : (uint32_t)(lo >> 23) & 3u;
    const bool one_cem = selector == 0u;
    const uint32_t config = (parts == 1u ? 17u : (one_cem ? 29u : 25u + 3u * parts)) + 2u * dual;
    const uint32_t under = 128u - wbits - (one_cem ? 0u : 3u * parts - 4u);   // where the spilled CEM bits start; the dual plane's channel is the two bits below
    uint32_t cems = 0, values = 0;   // four 4-bit modes in one word
    BU_UNROLL
    for (uint32_t p = 0; p < 4; p++) {
        if (p >= parts) continue;
        uint32_t mode;
        if (parts == 1u) mode = (uint32_t)(lo >> 13) & 15u;
        else if (one_cem) mode = (uint32_t)(lo >> 25) & 15u;
        else {
            const uint32_t cls = selector - (((uint32_t)(lo >> (25u + p)) & 1u) ? 0u : 1u), q0 = parts + 2u * p, q1 = q0 + 1u;
            const uint32_t l0 = astc_bits(lo, hi, q0 < 4u ? 25u + q0 : under + q0 - 4u, 1), l1 = astc_bits(lo, hi, q1 < 4u ? 25u + q1 : under + q1 - 4u, 1);
            mode = (cls << 2) | (l1 << 1) | l0;
        }
        cems |= mode << (4u * p);
        values += astc_values_of_mode(mode);
    }
    const int colour_bits = 128 - (int)wbits - (int)config;
    if (values > 18u || colour_bits < (int)((13u * values + 4u) / 5u)) return 0u;
    // this texel's partition; an HDR endpoint mode refuses the block if any texel is in such a partition
    const uint32_t x = i & 3u, y = i >> 2;
    astc_partition_seeds seeds = { 0u, 0u, 0u };
    uint32_t part = 0;
    if (parts > 1u) {
        seeds = astc_seeds((uint32_t)(lo >> 13) & 1023u, parts);
        part = astc_partition_of(seeds, parts, x, y);
    }
    const uint32_t hdr = (astc_mode_is_hdr(cems & 15u) ? 1u : 0u) | (astc_mode_is_hdr((cems >> 4) & 15u) && parts > 1u ? 2u : 0u) |
                         (astc_mode_is_hdr((cems >> 8) & 15u) && parts > 2u ? 4u : 0u) | (astc_mode_is_hdr((cems >> 12) & 15u) && parts > 3u ? 8u : 0u);
    if (hdr) {
        if (parts == 1u) return 0u;
        for (uint32_t t = 0; t < 16; t++)
            if ((hdr >> astc_partition_of(seeds, parts, t & 3u, t >> 2)) & 1u) return 0u;
    }
    const uint32_t mode = (cems >> (4u * part)) & 15u;
    uint32_t first = 0;   // where this partition's values start
    BU_UNROLL
    for (uint32_t p = 0; p < 3; p++)
        if (p < part) first += astc_values_of_mode((cems >> (4u * p)) & 15u);
    // the endpoint range: the widest of 8 bits, trits + 6, quints + 5, 7 bits, ... , trits + 1 whose sequence fits (candidate c: 8 - c / 3 bits, less 2 / 3 under trits / quints)
    uint32_t ekind = ISE_TRITS, en = 1u;
    for (int c = 15; c >= 0; c--) {
        const uint32_t kind = (uint32_t)c % 3u, n = 8u - (uint32_t)c / 3u - (kind == 0u ? 0u : kind + 1u);
        if ((int)ise_sequence_bits(kind, n, values) <= colour_bits) { ekind = kind; en = n; }
    }
    uint64_t clo = lo, chi = hi;
    astc_window(clo, chi, parts == 1u ? 17u : 29u, ise_sequence_bits(ekind, en, values));
    uint32_t v[8];
    const uint32_t count = astc_values_of_mode(mode);
    BU_UNROLL
    for (uint32_t j = 0; j < 8; j++) {
        v[j] = 0u;
        if (j < count) {
            uint32_t tq;
            const uint32_t m = ise_value(clo, chi, ekind, en, first + j, &tq);
            v[j] = astc_unquant_endpoint(ekind, en, m, tq);
        }
    }
    int e0[4], e1[4];
    astc_endpoints(mode, v, e0, e1);
    // weights: the stream runs from bit 127 downwards; this texel's place in the grid and the up to four grid weights around it, per plane
    uint64_t wlo = reverse64(hi), whi = reverse64(lo);
    astc_window(wlo, whi, 0u, wbits);
    const uint32_t gx = (342u * x * (gw - 1u) + 32u) >> 6, gy = (342u * y * (gh - 1u) + 32u) >> 6, jx = gx >> 4, jy = gy >> 4, fx = gx & 15u, fy = gy & 15u;
    const uint32_t w11 = (fx * fy + 8u) >> 4, w10 = fy - w11, w01 = fx - w11, w00 = 16u - fx - fy + w11, at = jy * gw + jx;
    uint32_t w[2] = { 0u, 0u };
    BU_UNROLL
    for (uint32_t pl = 0; pl < 2; pl++) {
        if (pl >= planes) continue;
        uint32_t sum = 8u;
        BU_UNROLL
        for (uint32_t k = 0; k < 4; k++) {
            const uint32_t f = k == 0u ? w00 : (k == 1u ? w01 : (k == 2u ? w10 : w11));
            if (!f) continue;   // a grid point past the edge always has factor 0
            uint32_t tq;
            const uint32_t m = ise_value(wlo, whi, wkind, wn, (at + (k & 1u) + (k >> 1) * gw) * planes + pl, &tq);
            sum += f * astc_unquant_weight(wkind, wn, m, tq);
        }
        w[pl] = sum >> 4;
    }
    const uint32_t ccs = dual ? astc_bits(lo, hi, under - 2u, 2) : 4u;
    uint32_t out = 0;
    BU_UNROLL
    for (uint32_t c = 0; c < 4; c++) {
        const uint32_t wt = c == ccs ? w[1] : w[0];
        out |= ((((uint32_t)e0[c] * 257u * (64u - wt) + (uint32_t)e1[c] * 257u * wt + 32u) >> 6) >> 8) << (8u * c);
    }
    *ok = true;
    return out;
}

// ---- PVRTC1 4bpp: a block is its 32 modulation bits (texel (x, y) at bits 2 (y * 4 + x)) and its endpoint word (low | high << 16, bit 0 the modulation mode)
BU_FN void pvrtc1_endpoint_5554(uint32_t word, uint32_t high, uint32_t c[4]) {
    const uint32_t p = high ? word >> 16 : word & 0xFFFFu;
    if (p & 0x8000u) {   // opaque: 554 (low) or 555
        c[0] = (p >> 10) & 31u; c[1] = (p >> 5) & 31u; c[3] = 15u;
        if (high) c[2] = p & 31u;
        else { const uint32_t b = (p >> 1) & 15u; c[2] = (b << 1) | (b >> 3); }
    } else {             // translucent: 3443 (low) or 3444
        const uint32_t r = (p >> 8) & 15u, g = (p >> 4) & 15u;
        c[0] = (r << 1) | (r >> 3); c[1] = (g << 1) | (g >> 3); c[3] = ((p >> 12) & 7u) << 1;
        if (high) { const uint32_t b = p & 15u; c[2] = (b << 1) | (b >> 3); }
        else { const uint32_t b = (p >> 1) & 7u; c[2] = (b << 2) | (b >> 1); }
    }
}
// p, q, r, s: the endpoint words of the blocks at (left, top), (right, top), (left, bottom), (right, bottom) of the 2x2 blocks around texel i of a block; the
// block itself is the right one of them for x < 2 and the bottom one for y < 2. modulation: the block's own 32 bits.
BU_FN uint32_t unpack_texel_pvrtc1(uint32_t p, uint32_t q, uint32_t r, uint32_t s, uint32_t modulation, uint32_t i) {
    const uint32_t x = i & 3u, y = i >> 2;
    const int u = (int)((x + 2u) & 3u), v = (int)((y + 2u) & 3u);
    const uint32_t own = y < 2u ? (x < 2u ? s : r) : (x < 2u ? q : p);
    const uint32_t m = (modulation >> (2u * i)) & 3u;
    uint32_t ends[2][4];
    BU_UNROLL
    for (uint32_t h = 0; h < 2; h++) {
        uint32_t cp[4], cq[4], cr[4], cs[4];
        pvrtc1_endpoint_5554(p, h, cp); pvrtc1_endpoint_5554(q, h, cq); pvrtc1_endpoint_5554(r, h, cr); pvrtc1_endpoint_5554(s, h, cs);
        BU_UNROLL
        for (uint32_t c = 0; c < 4; c++) {
            const int t = (int)cp[c] * 4 + u * ((int)cq[c] - (int)cp[c]), b = (int)cr[c] * 4 + u * ((int)cs[c] - (int)cr[c]);
            int val = t * 4 + v * (b - t);
            if (c < 3u) { val >>= 1; val += val >> 5; }
            else val += val >> 4;
            ends[h][c] = (uint32_t)val;
        }
    }
    uint32_t out = 0;
    BU_UNROLL
    for (uint32_t c = 0; c < 4; c++) {
        const uint32_t l = ends[0][c], h = ends[1][c];
        uint32_t val;
        if (m == 0u) val = l;
        else if (m == 3u) val = h;
        else if (own & 1u) val = (c == 3u && m == 2u) ? 0u : (l + h) / 2u;   // punch-through mode: the mean, and value 2 is transparent
        else val = m == 1u ? (l * 5u + h * 3u) / 8u : (l * 3u + h * 5u) / 8u;
        out |= val << (8u * c);
    }
    return out;
}

// ---- one texel of any format that is decoded from its own block alone. lo = bytes 0-7, hi = bytes 8-15 (unused by the 8-byte formats)
template <uint32_t FORMAT>
BU_FN uint32_t unpack_texture_texel(uint64_t lo, uint64_t hi, uint32_t i, bool* ok) {
    *ok = true;
    if (FORMAT == UF_ETC1) return unpack_texel_etc1(lo, i, ok);
    if (FORMAT == UF_ETC2_RGBA) {
        const uint32_t colour = unpack_texel_etc1(hi, i, ok);
        return *ok ? (colour & 0x00FFFFFFu) | (unpack_value_eac_a8(lo, i) << 24) : 0u;
    }
    if (FORMAT == UF_EAC_R11) return rgba(unpack_value_eac_r11(lo, i), 0u, 0u, 255u);
    if (FORMAT == UF_EAC_RG11) return rgba(unpack_value_eac_r11(lo, i), unpack_value_eac_r11(hi, i), 0u, 255u);
    if (FORMAT == UF_ASTC_4x4) return unpack_texel_astc(lo, hi, i, ok);
    return unpack_texel<FORMAT>(lo, hi, i, ok);   // the five BC formats
}

// ---- one block: 16 texels in raster order, 4 bytes each (R, G, B, A). False (and zeros) for an invalid block.
template <uint32_t FORMAT>
BU_FN bool unpack_texture_block(const uint8_t* blk, uint8_t* out64) {
    const uint64_t lo = load64(blk), hi = texture_bytes_per_block(FORMAT) == 16u ? load64(blk + 8) : 0ull;
    bool all = true;
    for (uint32_t i = 0; i < 16; i++) {
        bool ok;
        const uint32_t px = unpack_texture_texel<FORMAT>(lo, hi, i, &ok);
        all = all && ok;
        for (uint32_t k = 0; k < 4; k++) out64[i * 4 + k] = (uint8_t)(px >> (8u * k));
    }
    return all;
}

// ---- PVRTC1: block (bx, by) of an nbx x nby image (both powers of two) whose blocks lie in Morton order; neighbours wrap at the edges
BU_FN void unpack_pvrtc1_block(const uint8_t* blocks, uint32_t nbx, uint32_t nby, uint32_t bx, uint32_t by, uint8_t* out64) {
    const uint64_t own = load64(blocks + (size_t)bu_pvrtc1::morton_address(bx, by, nbx, nby) * 8u);
    for (uint32_t i = 0; i < 16; i++) {
        const uint32_t x0 = ((i & 3u) < 2u ? bx + nbx - 1u : bx) & (nbx - 1u), x1 = (x0 + 1u) & (nbx - 1u);
        const uint32_t y0 = ((i >> 2) < 2u ? by + nby - 1u : by) & (nby - 1u), y1 = (y0 + 1u) & (nby - 1u);
        const uint32_t p = (uint32_t)(load64(blocks + (size_t)bu_pvrtc1::morton_address(x0, y0, nbx, nby) * 8u) >> 32);
        const uint32_t q = (uint32_t)(load64(blocks + (size_t)bu_pvrtc1::morton_address(x1, y0, nbx, nby) * 8u) >> 32);
        const uint32_t r = (uint32_t)(load64(blocks + (size_t)bu_pvrtc1::morton_address(x0, y1, nbx, nby) * 8u) >> 32);
        const uint32_t s = (uint32_t)(load64(blocks + (size_t)bu_pvrtc1::morton_address(x1, y1, nbx, nby) * 8u) >> 32);
        const uint32_t px = unpack_texel_pvrtc1(p, q, r, s, (uint32_t)own, i);
        for (uint32_t k = 0; k < 4; k++) out64[i * 4 + k] = (uint8_t)(px >> (8u * k));
    }
}

}  // namespace bu_unpack
