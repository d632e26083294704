// pvrtc1.h -- PVRTC1 4bpp RGB / RGBA from ETC1S palette entries and from unpacked UASTC pixels: the per-block halves of the two passes of
// pvrtc1_kernels.hip. Integer arithmetic only; hipcc compiles it for the kernels, g++ for tools/pvrtc1_sanitize.cpp.
//
// What it computes is pinned, byte for byte, by the reference transcoder (transcoder/basisu_transcoder.cpp): the endpoint pass of transcode_slice's two
// PVRTC1 cases (:8901-8987) and of transcode_uastc_to_pvrtc1_4_rgb / _rgba (:19541-19643), and the four modulation passes fixup_pvrtc1_4_modulation_rgb /
// _rgba (:3621-3977, :19217-19539). Nothing here is a copied table: every look-up of the reference is restated as the rule it follows.
//   expansions   a 5-bit code to 8 bits by bit replication; a 4-bit and a 3-bit code to 5 bits the same way, then on; a 3-bit alpha code a to the 4-bit
//                code 2a, replicated to 8 bits (34a); alpha code 8 is the opaque 255
//   floor / ceil the largest code whose expansion is <= v / the smallest whose expansion is >= v
//   endpoints    low | high << 16. Opaque: 1 RRRRR GGGGG BBBB M (low, M = modulation mode = 0) and 1 RRRRR GGGGG BBBBB (high). Translucent: 0 AAA RRRR GGGG
//                BBB M and 0 AAA RRRR GGGG BBBB. The RGB routes write opaque words; the RGBA routes choose per endpoint: opaque where its alpha code is 8
//   modulation   texel (x, y) of a block lies between the endpoint pairs of four blocks of the 3x3 around it: the pair of columns (x < 2: left and own, else
//                own and right), the pair of rows likewise, with weights u = (x + 2) & 3 towards the later column and v = (y + 2) & 3 towards the later row,
//                (4 - u | u) x (4 - v | v) of 16. With ca / cb the interpolated low / high lumas and cl the texel's value: p = 16 (cl - ca), dl = cb - ca,
//                both negated when ca > cb; the modulation is 1 / 2 / 3 where p > 3 dl, p > 8 dl, p > 13 dl, all strict
//   lumas        RGB routes: (r5 + g5 + b5) * 255 / 31 of the packed word, the low endpoint's blue as (b & 30) | (b >> 4). RGBA routes: r + g + b + a of the
//                endpoint expanded to 8 bits. The word 0 (what the endpoint pass writes for an invalid block) reads as 0 / 0 either way
//   address      Morton order, y in the even bits and x in the odd ones, over the low min(log2 nbx, log2 nby) bits of both; the longer axis' other bits above
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#define BU_PV_FN __host__ __device__ __forceinline__
#define BU_PV_UNROLL _Pragma("unroll")
#else
#define BU_PV_FN static inline
#define BU_PV_UNROLL
#endif

namespace bu_pvrtc1 {

enum : uint32_t { TF_PVRTC1_4_RGB = 8, TF_PVRTC1_4_RGBA = 9 };   // the reference's transcoder_texture_format values
enum : uint32_t { kBytesPerBlock = 8 };

template <uint32_t BITS>
BU_PV_FN uint32_t expand(uint32_t c) {
    static_assert(BITS >= 3 && BITS <= 5, "3, 4 or 5 bits");
    if (BITS == 3) c = (c << 2) | (c >> 1);
    if (BITS == 4) c = (c << 1) | (c >> 3);
    return (c << 3) | (c >> 2);
}
// An expansion is at least c << (8 - BITS) and less than (c + 1) << (8 - BITS), so the floor is v >> (8 - BITS) or one below it
template <uint32_t BITS>
BU_PV_FN uint32_t floor_code(uint32_t v) {
    const uint32_t c = v >> (8u - BITS);
    return expand<BITS>(c) > v ? c - 1u : c;
}
template <uint32_t BITS>
BU_PV_FN uint32_t ceil_code(uint32_t v) {
    const uint32_t c = floor_code<BITS>(v);
    return expand<BITS>(c) < v ? c + 1u : c;
}
BU_PV_FN uint32_t expand_alpha(uint32_t a) { return a >= 8u ? 255u : a * 34u; }
BU_PV_FN uint32_t floor_alpha(uint32_t v) { return v == 255u ? 8u : v / 34u; }
BU_PV_FN uint32_t ceil_alpha(uint32_t v) { return v > 238u ? 8u : (v + 33u) / 34u; }

// ---- the endpoint word of a block from its bounds, c[0..3] = r, g, b, a
BU_PV_FN uint32_t opaque_low(const uint32_t c[4]) { return 0x8000u | (floor_code<5>(c[0]) << 10) | (floor_code<5>(c[1]) << 5) | (floor_code<4>(c[2]) << 1); }
BU_PV_FN uint32_t opaque_high(const uint32_t c[4]) { return 0x8000u | (ceil_code<5>(c[0]) << 10) | (ceil_code<5>(c[1]) << 5) | ceil_code<5>(c[2]); }
template <bool ALPHA>
BU_PV_FN uint32_t endpoint_word(const uint32_t low[4], const uint32_t high[4]) {
    uint32_t lo = opaque_low(low), hi = opaque_high(high);
    if (ALPHA) {
        const uint32_t la = floor_alpha(low[3]), ha = ceil_alpha(high[3]);
        if (la != 8u) lo = (la << 12) | (floor_code<4>(low[0]) << 8) | (floor_code<4>(low[1]) << 4) | (floor_code<3>(low[2]) << 1);
        if (ha != 8u) hi = (ha << 12) | (ceil_code<4>(high[0]) << 8) | (ceil_code<4>(high[1]) << 4) | ceil_code<4>(high[2]);
    }
    return lo | (hi << 16);
}

// ---- what the modulation pass reads back from a word: the luma of each endpoint
template <bool ALPHA>
BU_PV_FN void endpoint_lumas(uint32_t word, int& l0, int& l1) {
    const uint32_t lo = word & 0xFFFEu, hi = word >> 16;
    if (!ALPHA) {
        const uint32_t b = lo & 30u;
        l0 = (int)((((lo >> 10) & 31u) + ((lo >> 5) & 31u) + (b | (b >> 4))) * 255u / 31u);
        l1 = (int)((((hi >> 10) & 31u) + ((hi >> 5) & 31u) + (hi & 31u)) * 255u / 31u);
        return;
    }
    l0 = (lo & 0x8000u) ? (int)(expand<5>((lo >> 10) & 31u) + expand<5>((lo >> 5) & 31u) + expand<4>((lo & 31u) >> 1) + 255u)
                        : (int)(expand<4>((lo >> 8) & 15u) + expand<4>((lo >> 4) & 15u) + expand<3>((lo & 15u) >> 1) + expand_alpha((lo >> 12) & 7u));
    l1 = (hi & 0x8000u) ? (int)(expand<5>((hi >> 10) & 31u) + expand<5>((hi >> 5) & 31u) + expand<5>(hi & 31u) + 255u)
                        : (int)(expand<4>((hi >> 8) & 15u) + expand<4>((hi >> 4) & 15u) + expand<4>(hi & 15u) + expand_alpha((hi >> 12) & 7u));
}

// The 32 modulation bits of a block: words[ey * 3 + ex] are the endpoint words of the 3x3 blocks around it (own = words[4], wrapped by the caller), cl[y * 4 + x]
// the value of its texel (x, y) on the scale of 16 x luma.
template <bool ALPHA>
BU_PV_FN uint32_t modulation(const uint32_t words[9], const int cl[16]) {
    int e0[9], e1[9];
    BU_PV_UNROLL
    for (int k = 0; k < 9; k++) endpoint_lumas<ALPHA>(words[k], e0[k], e1[k]);
    uint32_t mod = 0;
    BU_PV_UNROLL
    for (int y = 0; y < 4; y++) {
        BU_PV_UNROLL
        for (int x = 0; x < 4; x++) {
            const int at = (y >> 1) * 3 + (x >> 1), u = (x + 2) & 3, v = (y + 2) & 3;
            const int w0 = (4 - u) * (4 - v), w1 = u * (4 - v), w2 = (4 - u) * v, w3 = u * v;
            const int ca = e0[at] * w0 + e0[at + 1] * w1 + e0[at + 3] * w2 + e0[at + 4] * w3;
            const int cb = e1[at] * w0 + e1[at + 1] * w1 + e1[at + 3] * w2 + e1[at + 4] * w3;
            int dl = cb - ca, p = (cl[y * 4 + x] - ca) * 16;
            if (ca > cb) { p = -p; dl = -dl; }
            uint32_t m = 0;
            if (p > 3 * dl) m = 1;
            if (p > 8 * dl) m = 2;
            if (p > 13 * dl) m = 3;
            mod |= m << (y * 8 + x * 2);
        }
    }
    return mod;
}

// ---- where block (x, y) of an nbx x nby image (both powers of two) is stored, in blocks
BU_PV_FN uint32_t spread_bits(uint32_t v) {   // bit i of the low 16 to bit 2 i
    v &= 0xFFFFu;
    v = (v | (v << 8)) & 0x00FF00FFu;
    v = (v | (v << 4)) & 0x0F0F0F0Fu;
    v = (v | (v << 2)) & 0x33333333u;
    return (v | (v << 1)) & 0x55555555u;
}
BU_PV_FN uint32_t log2_pow2(uint32_t v) { return 31u - (uint32_t)__builtin_clz(v); }
BU_PV_FN uint32_t morton_address(uint32_t x, uint32_t y, uint32_t nbx, uint32_t nby) {
    uint32_t at = spread_bits(y) | (spread_bits(x) << 1);
    if (nbx != nby) {
        const uint32_t xb = log2_pow2(nbx), yb = log2_pow2(nby), low = xb < yb ? xb : yb;
        at = (at & ((1u << (2u * low)) - 1u)) | (((nbx > nby ? x : y) >> low) << (2u * low));
    }
    return at;
}

// ---- ETC1S: a palette entry r5 | g5 << 8 | b5 << 16 | intensity table << 24, and a selector word with texel (x, y) at bits 2 * (y * 4 + x)
BU_PV_FN int clamp_to(int v, int top) { return v < 0 ? 0 : (v > top ? top : v); }
BU_PV_FN int intensity(uint32_t table, uint32_t s) {   // the ETC1 modifier tables, rows -b, -a, a, b: a and b of the eight tables as bytes of two words
    const int a = (int)((0x2F2118120D090502ull >> (8u * table)) & 255u), b = (int)((0xB76A503C2A1D1108ull >> (8u * table)) & 255u);
    const int v = (s == 0u || s == 3u) ? b : a;
    return s < 2u ? -v : v;
}
BU_PV_FN void selector_range(uint32_t sel, uint32_t& low, uint32_t& high) {
    uint32_t used = 0;
    BU_PV_UNROLL
    for (uint32_t p = 0; p < 16; p++) used |= 1u << ((sel >> (2u * p)) & 3u);
    low = (used & 1u) ? 0u : ((used & 2u) ? 1u : ((used & 4u) ? 2u : 3u));
    high = (used & 8u) ? 3u : ((used & 4u) ? 2u : ((used & 2u) ? 1u : 0u));
}
// pass 1: the block colour of the lowest and of the highest selector in use, alpha from the alpha slice's green
template <bool ALPHA>
BU_PV_FN uint32_t etc1s_endpoint_word(uint32_t entry, uint32_t sel, uint32_t alpha_entry, uint32_t alpha_sel) {
    const uint32_t table = (entry >> 24) & 7u;
    uint32_t l, h, low[4], high[4];
    selector_range(sel, l, h);
    const int dl = intensity(table, l), dh = intensity(table, h);
    BU_PV_UNROLL
    for (uint32_t k = 0; k < 3; k++) {
        const int c = (int)expand<5>((entry >> (8u * k)) & 31u);
        low[k] = (uint32_t)clamp_to(c + dl, 255);
        high[k] = (uint32_t)clamp_to(c + dh, 255);
    }
    low[3] = high[3] = 255u;
    if (ALPHA) {
        const uint32_t alpha_table = (alpha_entry >> 24) & 7u;
        const int g = (int)expand<5>((alpha_entry >> 8) & 31u);
        selector_range(alpha_sel, l, h);
        low[3] = (uint32_t)clamp_to(g + intensity(alpha_table, l), 255);
        high[3] = (uint32_t)clamp_to(g + intensity(alpha_table, h), 255);
    }
    return endpoint_word<ALPHA>(low, high);
}
// pass 2: 16 x (r8 + g8 + b8) + 48 x intensity, NOT clamped in the RGB route; in the RGBA route clamped to 0..48 * 255, plus the alpha slice's
// 16 x g8 + 16 x intensity clamped to 0..16 * 255
template <bool ALPHA>
BU_PV_FN void etc1s_texel_values(uint32_t entry, uint32_t sel, uint32_t alpha_entry, uint32_t alpha_sel, int cl[16]) {
    const uint32_t table = (entry >> 24) & 7u, alpha_table = (alpha_entry >> 24) & 7u;
    const int base = 16 * (int)(expand<5>(entry & 31u) + expand<5>((entry >> 8) & 31u) + expand<5>((entry >> 16) & 31u));
    const int alpha_base = 16 * (int)expand<5>((alpha_entry >> 8) & 31u);
    BU_PV_UNROLL
    for (uint32_t p = 0; p < 16; p++) {
        int c = base + 48 * intensity(table, (sel >> (2u * p)) & 3u);
        if (ALPHA) c = clamp_to(c, 48 * 255) + clamp_to(alpha_base + 16 * intensity(alpha_table, (alpha_sel >> (2u * p)) & 3u), 16 * 255);
        cl[p] = c;
    }
}

// ---- UASTC: the 16 unpacked pixels, r | g << 8 | b << 16 | a << 24, pixel y * 4 + x
template <bool ALPHA>
BU_PV_FN uint32_t pixels_endpoint_word(const uint32_t px[16]) {
    uint32_t low[4] = { 255u, 255u, 255u, 255u }, high[4] = { 0u, 0u, 0u, 0u };
    BU_PV_UNROLL
    for (uint32_t p = 0; p < 16; p++) {
        BU_PV_UNROLL
        for (uint32_t k = 0; k < 4; k++) {
            const uint32_t c = (px[p] >> (8u * k)) & 255u;
            low[k] = c < low[k] ? c : low[k];
            high[k] = c > high[k] ? c : high[k];
        }
    }
    return endpoint_word<ALPHA>(low, high);
}
template <bool ALPHA>
BU_PV_FN void pixels_texel_values(const uint32_t px[16], int cl[16]) {
    BU_PV_UNROLL
    for (uint32_t p = 0; p < 16; p++)
        cl[p] = 16 * (int)((px[p] & 255u) + ((px[p] >> 8) & 255u) + ((px[p] >> 16) & 255u) + (ALPHA ? px[p] >> 24 : 0u));
}

}  // namespace bu_pvrtc1
