// etc1s_block_format_targets.h -- the per-block conversions of the third ETC1S entry family's targets, included by etc1s_transcode_kernels.hip after
// etc1s_texture_targets.h: EAC R11 / RG11 (transcoder/basisu_transcoder.cpp: convert_etc1s_to_etc2_eac_r11 5104) and ASTC 4x4 (convert_etc1s_to_astc_4x4 5747 as the
// native build compiles it, with the 8-bit-endpoint routes, and the four astc_pack_block_cem_* layouts 5496-5604). One lane per block, everything in registers: a
// block is two 64-bit halves, the weights of a plane one 32-bit word (texel p at bits 2 p), and no array is indexed by a run-time value.
#pragma once

namespace bu {

enum : uint32_t { kAstcEntries = 8 * 32 * 6 * 10, kAstcTableWords = 2 * kAstcEntries + 48 };   // the 0..47 look-up, the 0..255 look-up, the 48 unquantised values

// ---- EAC R11: EAC A8's layout and route over its own look-up, on the first channel of the slice. RG11 is the colour slice's block, then the alpha slice's.
__device__ __forceinline__ uint2 to_eac_r11(const etc1s_entry& e, uint32_t sel) { return eac_from_lookup(e, sel, ke_eac_r11); }

// ---- ASTC 4x4
struct astc_block { uint64_t lo, hi; };

// the 8-bit value of a BISE code of endpoint range 0..47 (four bits, then a trit): the format's unquantisation, A = the lowest bit nine times, B = the other three bits
// b as b | b << 6, C = 22
__device__ __forceinline__ uint32_t astc_unquant48(uint32_t code) {
    const uint32_t bit = code & 15u, A = (bit & 1u) ? 511u : 0u, B = (bit >> 1) | ((bit >> 1) << 6);
    return (A & 0x80u) | ((((code >> 4) * 22u + B) ^ A) >> 2);
}
// the four values of a 2-bit weight between two 8-bit endpoints: both replicated to 16 bits, weights 0, 21, 43, 64 of 64, rounded, the top byte
__device__ __forceinline__ uint32_t astc_interp2(uint32_t l, uint32_t h, uint32_t k) { return (((l * 257u) * (64u - k) + (h * 257u) * k + 32u) >> 6) >> 8; }

__device__ __forceinline__ uint32_t green_of(const etc1s_entry& e, uint32_t s) { return (uint32_t)clamp255(scale5((int)e.g5) + inten_delta((int)e.table, (int)s)); }
__device__ __forceinline__ uint32_t rgb_sum(uint32_t c) { return (c & 255u) + ((c >> 8) & 255u) + (c >> 16); }
// the word map_selectors() wants from one of the ten mappings
__device__ __forceinline__ uint32_t mapping_word(uint32_t m) {
    const unsigned char* mp = &ke_bc1_mappings[m * 4u];
    return (uint32_t)mp[0] | ((uint32_t)mp[1] << 2) | ((uint32_t)mp[2] << 4) | ((uint32_t)mp[3] << 6);
}
// every pair of bits of a 32-bit word moved to twice its place: pair j (bits 2 j) -> bits 4 j
__device__ __forceinline__ uint64_t spread_pairs(uint32_t v) {
    uint64_t x = v;
    x = (x | (x << 16)) & 0x0000FFFF0000FFFFull;
    x = (x | (x << 8)) & 0x00FF00FF00FF00FFull;
    x = (x | (x << 4)) & 0x0F0F0F0F0F0F0F0Full;
    x = (x | (x << 2)) & 0x3333333333333333ull;
    return x;
}
// Weights lie from the top of the block down, each with its bits reversed: reversing the whole word does both. Two planes of 2-bit weights (colour, then alpha, per
// texel) fill the high 64 bits; one plane, or two planes of 1-bit weights (w1: texel p's colour bit at 2 p, alpha bit at 2 p + 1), the top 32.
__device__ __forceinline__ uint64_t astc_weights_two_planes(uint32_t wc, uint32_t wa) { return (spread_pairs(__brev(wc)) << 2) | spread_pairs(__brev(wa)); }
__device__ __forceinline__ uint64_t astc_weights_top32(uint32_t w) { return (uint64_t)__brev(w) << 32; }
// 8-bit endpoints, endpoint i at bits 8 i of `ends`, from bit 17 of the block
__device__ __forceinline__ astc_block astc_with_endpoints8(uint64_t lo, uint64_t hi, uint64_t ends) { return astc_block{ lo | (ends << 17), hi | (ends >> 47) }; }
// five BISE values of range 0..47 -> their 28 bits: four bits each, the five trits as one 8-bit block interleaved with them
__device__ __forceinline__ uint64_t astc_trit_group(uint32_t e0, uint32_t e1, uint32_t e2, uint32_t e3, uint32_t e4) {
    const uint32_t T = ku_trit_encode[(e0 >> 4) + 3u * (e1 >> 4) + 9u * (e2 >> 4) + 27u * (e3 >> 4) + 81u * (e4 >> 4)];
    const uint32_t first = (e0 & 15u) | ((T & 3u) << 4) | ((e1 & 15u) << 6);
    const uint32_t second = ((T >> 2) & 3u) | ((e2 & 15u) << 2) | (((T >> 4) & 1u) << 6) | ((e3 & 15u) << 7) | (((T >> 5) & 3u) << 11) | ((e4 & 15u) << 13) | ((T >> 7) << 17);
    return (uint64_t)first | ((uint64_t)second << 10);
}

// the first least error of the ten mappings of one entry (a grey or alpha plane), and of three entries summed (colour)
__device__ __forceinline__ uint32_t astc_best_mapping(const uint32_t* t) {
    uint32_t best_err = 0xFFFFFFFFu, best = 0;
#pragma unroll
    for (uint32_t m = 0; m < 10; m++) {
        const uint32_t err = t[m] >> 16;
        if (err < best_err) { best_err = err; best = m; }
    }
    return best;
}
__device__ __forceinline__ uint32_t astc_best_mapping(const uint32_t* tr, const uint32_t* tg, const uint32_t* tb) {
    uint32_t best_err = 0xFFFFFFFFu, best = 0;
#pragma unroll
    for (uint32_t m = 0; m < 10; m++) {
        const uint32_t err = (tr[m] >> 16) + (tg[m] >> 16) + (tb[m] >> 16);
        if (err < best_err) { best_err = err; best = m; }
    }
    return best;
}
__device__ __forceinline__ const uint32_t* astc_entry(const uint32_t* table, uint32_t inten, uint32_t base5, uint32_t range) { return &table[((inten * 32u + base5) * 6u + range) * 10u]; }

// what a block's selectors say
struct selector_use { uint32_t low, high, n; };
__device__ __forceinline__ selector_use selector_use_of(uint32_t sel) {
    selector_use u;
    u.n = (uint32_t)__popc(selectors_used(sel, u.low, u.high));
    return u;
}
__device__ __forceinline__ bool is_outlier(uint32_t table, const selector_use& u) { return table >= 7u && u.n == 2u && u.low == 0u && u.high == 3u; }

// one plane of the luminance + alpha mode (8-bit endpoints, 2-bit weights) from the green channel: at most two selectors -> the two values, weights 0 / 3; else the
// 0..255 look-up under its best mapping
__device__ __forceinline__ void astc_grey_plane(const etc1s_entry& e, uint32_t sel, const selector_use& u, const uint32_t* table255, uint32_t& l, uint32_t& h, uint32_t& w) {
    if (u.n <= 2u) {
        l = green_of(e, u.low); h = green_of(e, u.high);
        w = map_selectors(sel, 3u << (2u * u.high));
        return;
    }
    const uint32_t* t = astc_entry(table255, e.table, e.g5, ke_bc1_range_index[u.low * 4u + u.high]);
    const uint32_t m = astc_best_mapping(t), v = t[m];
    l = v & 255u; h = (v >> 8) & 255u;
    w = map_selectors(sel, mapping_word(m));
}

// The ASTC block of a colour-slice block (e, sel) and, with has_alpha, an alpha-slice block (ae, asel). tables: launch_etc1s_build_astc_tables' words. The routes in
// the reference's order: void extent, block truncation (1-bit weights), grey base colour (luminance + alpha), opaque (RGB, one plane), and the general one: RGBA over
// endpoints of range 0..47, two planes. Wherever colour endpoints are ordered, the pair trades places and the colour weights are inverted when the high endpoint's
// r + g + b is the smaller.
__device__ __forceinline__ astc_block to_astc(const etc1s_entry& e, uint32_t sel, bool has_alpha, const etc1s_entry& ae, uint32_t asel, const uint32_t* tables) {
    const selector_use u = selector_use_of(sel);
    selector_use au = { 0u, 0u, 1u };
    uint32_t constant_alpha = 255u;
    if (has_alpha) {
        au = selector_use_of(asel);
        if (au.n == 1u) constant_alpha = green_of(ae, au.low);
    }
    uint32_t colors[4];
    block_colors(e, colors);
    if (u.n == 1u && au.n == 1u) {   // void extent: every channel as 16 bits
        const uint32_t c = pick4(colors, u.low);
        return astc_block{ 0xFFFFFFFFFFFFFDFCull, (uint64_t)((c & 255u) * 257u) | ((uint64_t)(((c >> 8) & 255u) * 257u) << 16) | ((uint64_t)((c >> 16) * 257u) << 32) |
                                                  ((uint64_t)(constant_alpha * 257u) << 48) };
    }
    if (u.n <= 2u && au.n <= 2u) {   // block truncation: the two colours and the two alphas are the endpoints
        uint32_t c0 = pick4(colors, u.low), c1 = pick4(colors, u.high), cmap = 1u << (2u * u.high);
        if (rgb_sum(c1) < rgb_sum(c0)) { const uint32_t t = c0; c0 = c1; c1 = t; cmap ^= 0x55u; }
        uint32_t a0 = 255u, a1 = 255u, w1 = map_selectors(sel, cmap);
        if (has_alpha) {
            a0 = green_of(ae, au.low); a1 = green_of(ae, au.high);
            w1 |= map_selectors(asel, 1u << (2u * au.high)) << 1;
        }
        const uint64_t ends = (uint64_t)((c0 & 255u) | ((c1 & 255u) << 8) | (((c0 >> 8) & 255u) << 16) | (((c1 >> 8) & 255u) << 24)) |
                              ((uint64_t)((c0 >> 16) | ((c1 >> 16) << 8) | (a0 << 16) | (a1 << 24)) << 32);
        return astc_with_endpoints8(0x0000000000018441ull, 0xC0000000ull | astc_weights_top32(w1), ends);
    }
    const uint32_t* table255 = tables + kAstcEntries;
    if (e.r5 == e.g5 && e.r5 == e.b5) {   // grey: luminance + alpha, each plane on its own
        uint32_t l, h, wc, al = 255u, ah = 255u, wa = 0u;
        astc_grey_plane(e, sel, u, table255, l, h, wc);
        if (has_alpha) astc_grey_plane(ae, asel, au, table255, al, ah, wa);
        return astc_with_endpoints8(0xC000000000008442ull, astc_weights_two_planes(wc, wa), (uint64_t)(l | (h << 8) | (al << 16) | (ah << 24)));
    }
    if (au.n == 1u && constant_alpha == 255u) {   // opaque: RGB over 8-bit endpoints, one plane (three or four selectors in use here)
        const uint32_t range = ke_bc1_range_index[u.low * 4u + u.high];
        const uint32_t *tr = astc_entry(table255, e.table, e.r5, range), *tg = astc_entry(table255, e.table, e.g5, range), *tb = astc_entry(table255, e.table, e.b5, range);
        const uint32_t m = astc_best_mapping(tr, tg, tb), r = tr[m], g = tg[m], b = tb[m];
        uint32_t c0 = (r & 255u) | ((g & 255u) << 8) | ((b & 255u) << 16), c1 = ((r >> 8) & 255u) | (((g >> 8) & 255u) << 8) | (((b >> 8) & 255u) << 16);
        uint32_t w = map_selectors(sel, mapping_word(m));
        if (rgb_sum(c1) < rgb_sum(c0)) { const uint32_t t = c0; c0 = c1; c1 = t; w = ~w; }
        const uint64_t ends = (uint64_t)((c0 & 255u) | ((c1 & 255u) << 8) | (((c0 >> 8) & 255u) << 16) | (((c1 >> 8) & 255u) << 24)) | ((uint64_t)((c0 >> 16) | ((c1 >> 16) << 8)) << 32);
        return astc_with_endpoints8(0x0000000000010042ull, astc_weights_top32(w), ends);
    }
    // RGBA over BISE codes of range 0..47. Alpha first: none -> code 1 (255) twice; one selector -> the pair whose weight-1 value is nearest; the widest table's two
    // extremes -> the nearest code each, weights 0 / 3; else the look-up under its best mapping.
    uint32_t al = 1u, ah = 1u, wa = 0u;
    if (has_alpha) {
        if (au.n == 1u) {
            al = ke_astc_solid[constant_alpha * 2u]; ah = ke_astc_solid[constant_alpha * 2u + 1u];
            wa = 0x55555555u;
        } else if (is_outlier(ae.table, au)) {
            al = ke_astc_nearest[green_of(ae, 0u)]; ah = ke_astc_nearest[green_of(ae, 3u)];
            wa = map_selectors(asel, 3u << 6);
        } else {
            const uint32_t* t = astc_entry(tables, ae.table, ae.g5, ke_bc1_range_index[au.low * 4u + au.high]);
            const uint32_t m = astc_best_mapping(t), v = t[m];
            al = v & 255u; ah = (v >> 8) & 255u;
            wa = map_selectors(asel, mapping_word(m));
        }
    }
    // colour the same three ways per channel; l and h hold the three codes r | g << 8 | b << 16
    uint32_t l, h, wc;
    if (u.n == 1u) {
        const uint32_t c = pick4(colors, u.low), r = c & 255u, g = (c >> 8) & 255u, b = c >> 16;
        l = (uint32_t)ke_astc_solid[r * 2u] | ((uint32_t)ke_astc_solid[g * 2u] << 8) | ((uint32_t)ke_astc_solid[b * 2u] << 16);
        h = (uint32_t)ke_astc_solid[r * 2u + 1u] | ((uint32_t)ke_astc_solid[g * 2u + 1u] << 8) | ((uint32_t)ke_astc_solid[b * 2u + 1u] << 16);
        wc = 0x55555555u;
    } else if (is_outlier(e.table, u)) {
        const uint32_t c0 = colors[0], c3 = colors[3];
        l = (uint32_t)ke_astc_nearest[c0 & 255u] | ((uint32_t)ke_astc_nearest[(c0 >> 8) & 255u] << 8) | ((uint32_t)ke_astc_nearest[c0 >> 16] << 16);
        h = (uint32_t)ke_astc_nearest[c3 & 255u] | ((uint32_t)ke_astc_nearest[(c3 >> 8) & 255u] << 8) | ((uint32_t)ke_astc_nearest[c3 >> 16] << 16);
        wc = map_selectors(sel, 3u << 6);
    } else {
        const uint32_t range = ke_bc1_range_index[u.low * 4u + u.high];
        const uint32_t *tr = astc_entry(tables, e.table, e.r5, range), *tg = astc_entry(tables, e.table, e.g5, range), *tb = astc_entry(tables, e.table, e.b5, range);
        const uint32_t m = astc_best_mapping(tr, tg, tb), r = tr[m], g = tg[m], b = tb[m];
        l = (r & 255u) | ((g & 255u) << 8) | ((b & 255u) << 16);
        h = ((r >> 8) & 255u) | (((g >> 8) & 255u) << 8) | (((b >> 8) & 255u) << 16);
        wc = map_selectors(sel, mapping_word(m));
    }
    const uint32_t s0 = astc_unquant48(l & 255u) + astc_unquant48((l >> 8) & 255u) + astc_unquant48(l >> 16);
    const uint32_t s1 = astc_unquant48(h & 255u) + astc_unquant48((h >> 8) & 255u) + astc_unquant48(h >> 16);
    if (s1 < s0) { const uint32_t t = l; l = h; h = t; wc = ~wc; }
    const uint64_t g1 = astc_trit_group(l & 255u, h & 255u, (l >> 8) & 255u, (h >> 8) & 255u, l >> 16), g2 = astc_trit_group(h >> 16, al, ah, 0u, 0u);
    return astc_block{ 0xC000000000018442ull | (g1 << 17) | (g2 << 45), astc_weights_two_planes(wc, wa) };
}

}  // namespace bu
