// uastc_transcode.h -- UASTC LDR 4x4 transcode core: one 16-byte block in, one block of a GPU texture format (or 16 RGBA texels) out.
//
// What it computes is pinned, bit for bit, by the reference's per-block transcoders (transcoder/basisu_transcoder.cpp): unpack_uastc (:15886),
// transcode_uastc_to_astc (:16014) + pack_astc_block (:15028), transcode_uastc_to_bc7 (:16034-16537) + encode_bc7_block (:14657),
// transcode_uastc_to_bc1 / _bc3 / _bc4 / _bc5 (:18730-18864) with encode_bc1 (:18047) and encode_bc4 (:17737). Every function returns false exactly
// where the reference's does: a mode code that matches nothing, a pattern index out of range. The unpacker, the two decoders and the BC1 encoder are
// those of uastc_core.h / uastc_rdo.h; the output packers below are written from the formats' definitions (ASTC: BISE integer sequences, bit-reversed
// weights, the void-extent block; BC7: mode / partition / endpoint / p-bit / index fields with the anchor convention; BC4: the 8-value ramp).
// Same convention as uastc_core.h: hipcc compiles it for uastc_transcode_kernels.hip, g++ for the test-only host library (tests/native).
//
//
// The second half of the file is the texture family's further targets, the consumers of the encoder's ETC hints: transcode_uastc_to_etc1 (:16720) with
// etc1_determine_selectors (:16616) and apply_etc1_bias, transcode_uastc_to_etc2_eac_a8 (:17629), transcode_uastc_to_etc2_rgba (:17706), pack_eac_solid_block /
// pack_eac / pack_eac_high_quality (:18868-19155), transcode_uastc_to_etc2_eac_r11 / _rg11 (:19157-19214) and the three 16-bit cases of transcode_slice
// (:10246-10302). The first family's callers (transcode_bytes_per_block) do not reach them.
//
// PVRTC1 is not a per-block target (a block's modulation depends on the blocks around it, and images must be powers of two): it is pvrtc1.h's, in two passes over
// transcode_rgba32 (pvrtc1_kernels.hip). The callers of this file keep refusing it.
// Out of scope: ETC1 from the alpha channel (cDecodeFlagsTranscodeAlphaDataToOpaqueFormats: the single-channel packer at :16925), ATC / FXT1 / PVRTC2 (the reference
// refuses them for UASTC too), ETC1S slices, UASTC HDR / ASTC LDR / XUASTC blocks, Zstandard-supercompressed KTX2 levels. Callers refuse those; nothing is silently
// mapped to another target.
#pragma once
#include <math.h>
#include "uastc_rdo.h"
#include "uastc_transcode_tables.inc"
#include "tile_raster.h"

namespace bu_uastc {

// the reference's transcoder_texture_format values of the supported targets (basisu_transcoder.h)
enum { TF_BC1_RGB = 2, TF_BC3_RGBA = 3, TF_BC4_R = 4, TF_BC5_RG = 5, TF_BC7_RGBA = 6, TF_ASTC_4x4_RGBA = 10, TF_RGBA32 = 13 };
enum { DECODE_FLAGS_HIGH_QUALITY = 32 };   // cDecodeFlagsHighQuality

// An output block under construction: 128 bits in two registers, fields OR-ed in at any bit position (bits past 127 fall off, as they do in the
// reference's 20-byte staging buffer for the last partial BISE group).
struct bits128 { uint64_t lo, hi; };
BU_FN void put128(bits128& w, uint32_t pos, uint64_t v, uint32_t n) {
    if (!n || pos >= 128) return;
    if (n < 64) v &= (1ull << n) - 1;
    if (pos < 64) {
        w.lo |= v << pos;
        if (pos && pos + n > 64) w.hi |= v >> (64 - pos);
    } else {
        w.hi |= v << (pos - 64);
    }
}
BU_FN void store128(const bits128& w, uint8_t* out16) {
    for (uint32_t i = 0; i < 8; i++) { out16[i] = (uint8_t)(w.lo >> (8 * i)); out16[8 + i] = (uint8_t)(w.hi >> (8 * i)); }
}
BU_FN uint64_t reverse64(uint64_t v) {
    v = ((v >> 1) & 0x5555555555555555ull) | ((v & 0x5555555555555555ull) << 1);
    v = ((v >> 2) & 0x3333333333333333ull) | ((v & 0x3333333333333333ull) << 2);
    v = ((v >> 4) & 0x0F0F0F0F0F0F0F0Full) | ((v & 0x0F0F0F0F0F0F0F0Full) << 4);
    v = ((v >> 8) & 0x00FF00FF00FF00FFull) | ((v & 0x00FF00FF00FF00FFull) << 8);
    v = ((v >> 16) & 0x0000FFFF0000FFFFull) | ((v & 0x0000FFFF0000FFFFull) << 16);
    return (v >> 32) | (v << 32);
}

// ---- RGBA32: unpack_uastc(blk, pixels, srgb = false)
BU_FN bool transcode_rgba32(const uint8_t* blk, rgba8* out) {
    cand c;
    if (!unpack_block(blk, c)) return false;
    if (c.mode == 8) {
        for (uint32_t i = 0; i < 16; i++)
            for (uint32_t k = 0; k < 4; k++) out[i].c[k] = c.endpoints[k];
        return true;
    }
    decode_uastc(c, out);
    return true;
}

// ---- ASTC 4x4
// The 11-bit block mode of a 4x4 weight grid (ASTC block mode layout "B+4 x A+2" with B = 0, A = 2): D = dual plane (bit 10), H = high precision
// weight range (bit 9), the range code R in bits 4 (R0), 0 (R1), 1 (R2).
BU_FN uint32_t astc_block_mode(uint32_t wbits, bool dual) {
    const uint32_t h = wbits >= 4 ? 1u : 0u;
    const uint32_t r = wbits == 1 ? 2u : ((wbits == 2 || wbits == 4) ? 4u : 7u);   // 2 / 4 / 8 levels at low precision, 16 / 32 at high
    return (dual ? 1u << 10 : 0u) | (h << 9) | (2u << 5) | ((r & 1u) << 4) | (((r >> 2) & 1u) << 1) | ((r >> 1) & 1u);
}

// astc_pack_bise: `n` endpoint values of `range` as a bounded integer sequence starting at bit `pos`
BU_FN void astc_put_endpoints(bits128& w, uint32_t pos, const uint8_t* v, uint32_t n, uint32_t range) {
    const uint32_t bits = ku_bise[range * 3], mask = (1u << bits) - 1;
    if (ku_bise[range * 3 + 1]) {           // trits: 5 values -> 8 + 5 bits
        for (uint32_t g = 0; g < n; g += 5) {
            uint32_t m[5], t = 0, mul = 1;
            for (uint32_t i = 0; i < 5; i++) {
                const uint32_t x = g + i < n ? v[g + i] : 0u;
                m[i] = x & mask; t += (x >> bits) * mul; mul *= 3;
            }
            const uint32_t T = ku_trit_encode[t];
            put128(w, pos, m[0] | ((T & 3u) << bits) | (m[1] << (2 + bits)), bits * 2 + 2);
            pos += bits * 2 + 2;
            put128(w, pos, ((T >> 2) & 3u) | (m[2] << 2) | (((T >> 4) & 1u) << (2 + bits)) | (m[3] << (3 + bits)) | (((T >> 5) & 3u) << (3 + bits * 2)) |
                           (m[4] << (5 + bits * 2)) | (((T >> 7) & 1u) << (5 + bits * 3)), bits * 3 + 6);
            pos += bits * 3 + 6;
        }
    } else if (ku_bise[range * 3 + 2]) {    // quints: 3 values -> 7 + 3 bits
        for (uint32_t g = 0; g < n; g += 3) {
            uint32_t m[3], q = 0, mul = 1;
            for (uint32_t i = 0; i < 3; i++) {
                const uint32_t x = g + i < n ? v[g + i] : 0u;
                m[i] = x & mask; q += (x >> bits) * mul; mul *= 5;
            }
            const uint32_t Q = ku_quint_encode[q];
            put128(w, pos, m[0] | ((Q & 7u) << bits) | (m[1] << (3 + bits)) | (((Q >> 3) & 3u) << (3 + bits * 2)) | (m[2] << (5 + bits * 2)) |
                           (((Q >> 5) & 3u) << (5 + bits * 3)), 7 + bits * 3);
            pos += 7 + bits * 3;
        }
    } else {
        for (uint32_t i = 0; i < n; i++) { put128(w, pos, v[i], bits); pos += bits; }
    }
}

BU_FN bool transcode_astc(const uint8_t* blk, uint8_t* out16) {
    cand c;
    if (!unpack_block(blk, c)) return false;
    bits128 w = { 0, 0 };
    if (c.mode == 8) {   // void-extent block: 0x1FC, the "no extent" coordinates all ones, four UNORM16 channels
        w.lo = 0xFFFFFFFFFFFFFDFCull;
        for (uint32_t k = 0; k < 4; k++) w.hi |= (uint64_t)(c.endpoints[k] * 257u) << (16 * k);
        store128(w, out16);
        return true;
    }
    const uint32_t mode = c.mode, subsets = ku_mode_subsets[mode], planes = ku_mode_planes[mode], comps = ku_mode_comps[mode];
    const uint32_t wbits = ku_mode_weight_bits[mode], range = ku_mode_endpoint_ranges[mode], top = (1u << wbits) - 1;
    // ASTC decodes RGB(A) endpoints whose second colour sums lower than the first with blue contraction; UASTC never means that, so such a
    // subset is stored the other way round with its weights mirrored (unpack_uastc's blue_contract_check, :15693-15736)
    if (comps >= 3) {
        const uint32_t pat = astc_pattern_bits(mode, c.pattern);
        for (uint32_t s = 0; s < subsets; s++) {
            if (!order_endpoints(c.endpoints + s * comps * 2, comps, range)) continue;
            for (uint32_t i = 0; i < 16; i++)
                if (((pat >> (2 * i)) & 3) == s)
                    for (uint32_t p = 0; p < planes; p++) c.weights[i * planes + p] = (uint8_t)(top - c.weights[i * planes + p]);
        }
    }
    const uint32_t cem = comps == 2 ? 4u : (comps == 3 ? 8u : 12u);   // LA direct, RGB direct, RGBA direct
    put128(w, 0, astc_block_mode(wbits, planes == 2), 11);
    put128(w, 11, subsets - 1, 2);
    uint32_t pos = 13;
    if (subsets == 1) { put128(w, pos, cem, 4); pos += 4; }
    else {
        const uint32_t seed = subsets == 3 ? ku_cp3_astc[c.pattern] : (mode == 7 ? ku_cp7_astc[c.pattern] : ku_cp2_astc[c.pattern]);
        put128(w, pos, seed, 10); pos += 10;
        put128(w, pos, (cem << 2) & 63u, 6); pos += 6;   // "all subsets share one endpoint mode": two zero bits, then the mode
    }
    const uint32_t total_weights = 16 * planes;
    if (planes == 2) put128(w, 128 - total_weights * wbits - 2, c.ccs, 2);
    astc_put_endpoints(w, pos, c.endpoints, comps * 2 * subsets, range);
    // weights fill the block from the top bit downwards, each bit-reversed: the forward stream (weight i at bit i * wbits) reversed as a whole
    bits128 f = { 0, 0 };
    for (uint32_t i = 0; i < total_weights; i++) put128(f, i * wbits, c.weights[i], wbits);
    w.hi |= reverse64(f.lo);
    w.lo |= reverse64(f.hi);
    store128(w, out16);
    return true;
}

// ---- BC7
struct bc7_fields {          // bc7_optimization_results, index selector always 0
    uint8_t mode, partition, rotation;
    uint8_t sel[16], asel[16];
    uint8_t low[3][4], high[3][4];
    uint32_t pbits[3][2];
};

// float endpoints of the subset whose ASTC endpoint indices start at `e` (LA modes replicate luminance), then determine_unique_pbits /
// determine_shared_pbits into subset `d` of the result
BU_FN void bc7_quantise_subset(const cand& c, const uint8_t* e, bool shared, uint32_t ncomp, uint32_t bits, bc7_fields& o, uint32_t d) {
    const uint32_t comps = ku_mode_comps[c.mode];
    const uint8_t* UQ = ku_unquant + ku_mode_endpoint_ranges[c.mode] * 256;
    float xl[4], xh[4];
    if (comps == 2) {
        xl[0] = xl[1] = xl[2] = (float)UQ[e[0]] / 255.0f; xh[0] = xh[1] = xh[2] = (float)UQ[e[1]] / 255.0f;
        xl[3] = (float)UQ[e[2]] / 255.0f; xh[3] = (float)UQ[e[3]] / 255.0f;
    } else {
        for (uint32_t k = 0; k < 4; k++) {
            xl[k] = k < comps ? (float)UQ[e[k * 2]] / 255.0f : 1.0f;
            xh[k] = k < comps ? (float)UQ[e[k * 2 + 1]] / 255.0f : 1.0f;
        }
    }
    uint8_t lo[4] = { 0, 0, 0, 0 }, hi[4] = { 0, 0, 0, 0 };
    uint32_t pb[2] = { 0, 0 };
    bc7_pbit_quantise(shared, ncomp, bits, xl, xh, lo, hi, pb);
    for (uint32_t k = 0; k < 4; k++) { o.low[d][k] = lo[k]; o.high[d][k] = hi[k]; }
    o.pbits[d][0] = pb[0]; o.pbits[d][1] = pb[1];
}

// transcode_uastc_to_bc7(unpacked, results), :16034-16526
BU_FN void bc7_from_uastc(const cand& c, bc7_fields& o) {
    const uint32_t mode = c.mode, comps = ku_mode_comps[mode];
    const uint8_t* UQ = ku_unquant + ku_mode_endpoint_ranges[mode] * 256;
    const uint8_t* ep = c.endpoints;
    o.mode = 0; o.partition = 0; o.rotation = 0;
    for (uint32_t i = 0; i < 16; i++) { o.sel[i] = c.weights[i]; o.asel[i] = 0; }
    for (uint32_t s = 0; s < 3; s++) {
        for (uint32_t k = 0; k < 4; k++) { o.low[s][k] = 0; o.high[s][k] = 0; }
        o.pbits[s][0] = o.pbits[s][1] = 0;
    }
    switch (mode) {
    case 8: {  // solid: mode 6 where some p-bit reproduces the colour exactly, mode 5 otherwise
        uint32_t e0 = 0, e1 = 0;
        for (uint32_t k = 0; k < 4; k++) { e0 += ku_bc7_m6_solid[ep[k] * 6]; e1 += ku_bc7_m6_solid[ep[k] * 6 + 3]; }
        if (e0 > 0 && e1 > 0) {
            o.mode = 5;
            for (uint32_t k = 0; k < 3; k++) { o.low[0][k] = ku_bc7_m5_solid[ep[k] * 2]; o.high[0][k] = ku_bc7_m5_solid[ep[k] * 2 + 1]; }
            o.low[0][3] = o.high[0][3] = ep[3];
            for (uint32_t i = 0; i < 16; i++) o.sel[i] = 1;
        } else {
            o.mode = 6;
            const uint32_t p = e1 < e0 ? 1u : 0u;
            for (uint32_t k = 0; k < 4; k++) { o.low[0][k] = ku_bc7_m6_solid[ep[k] * 6 + p * 3 + 1]; o.high[0][k] = ku_bc7_m6_solid[ep[k] * 6 + p * 3 + 2]; }
            o.pbits[0][0] = o.pbits[0][1] = p;
            for (uint32_t i = 0; i < 16; i++) o.sel[i] = 5;
        }
        break;
    }
    case 0: case 5: case 10: case 12: case 14: case 15: case 18: {  // -> BC7 mode 6
        o.mode = 6;
        bc7_quantise_subset(c, ep, false, comps == 2 ? 4 : comps, 7, o, 0);
        if (comps == 3) { o.low[0][3] = 127; o.high[0][3] = 127; }
        const uint8_t five_to_four[32] = { 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 6, 7, 8, 9, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13, 14, 14, 15, 15 };
        const uint8_t three_to_four[8] = { 0, 2, 4, 6, 9, 11, 13, 15 };
        for (uint32_t i = 0; i < 16; i++) {
            const uint32_t wv = c.weights[i];
            o.sel[i] = (uint8_t)(mode == 18 ? five_to_four[wv] : (mode == 14 ? wv * 5 : ((mode == 5 || mode == 12) ? three_to_four[wv] : wv)));
        }
        break;
    }
    case 1: {  // one subset -> BC7 mode 3, partition 0, both subsets alike
        o.mode = 3;
        bc7_quantise_subset(c, ep, false, 3, 7, o, 0);
        for (uint32_t k = 0; k < 4; k++) { o.low[0][k] = k < 3 ? o.low[0][k] : 0; o.high[0][k] = k < 3 ? o.high[0][k] : 0; o.low[1][k] = o.low[0][k]; o.high[1][k] = o.high[0][k]; }
        o.pbits[1][0] = o.pbits[0][0]; o.pbits[1][1] = o.pbits[0][1];
        break;
    }
    case 2: case 4: case 9: case 16: {  // two subsets -> BC7 mode 1 (2), 3 (4), 7 (9, 16)
        o.mode = (uint8_t)(mode == 2 ? 1 : (mode == 4 ? 3 : 7));
        o.partition = ku_cp2_bc7[c.pattern];
        const bool invert = ku_cp2_invert[c.pattern] != 0;
        const uint32_t ncomp = mode >= 9 ? 4 : 3, bits = mode == 2 ? 6 : (ncomp == 4 ? 5 : 7);
        for (uint32_t s = 0; s < 2; s++) {
            const uint32_t d = invert ? 1 - s : s;
            bc7_quantise_subset(c, ep + s * comps * 2, mode == 2, ncomp, bits, o, d);
            if (ncomp == 3) { o.low[d][3] = o.high[d][3] = (uint8_t)(mode == 4 ? 127 : 0); }
            if (mode == 2) o.pbits[d][1] = 0;
        }
        break;
    }
    case 3: case 7: {  // -> BC7 mode 2: three subsets of 5-bit endpoints
        o.mode = 2;
        o.partition = mode == 3 ? ku_cp3_bc7[c.pattern] : ku_cp7_bc7[c.pattern];
        for (uint32_t d = 0; d < 3; d++) {
            uint32_t s = 0;   // the ASTC subset that BC7 subset d takes its endpoints from
            if (mode == 7) s = bc7_3_to_2(d, ku_cp7_k[c.pattern]);
            else for (uint32_t a = 0; a < 3; a++) if (ku_astc_to_bc7_perm[ku_cp3_perm[c.pattern] * 3 + a] == d) s = a;
            for (uint32_t k = 0; k < 3; k++) {
                o.low[d][k] = (uint8_t)((UQ[ep[k * 2 + s * 6]] * 31 + 127) / 255);
                o.high[d][k] = (uint8_t)((UQ[ep[k * 2 + 1 + s * 6]] * 31 + 127) / 255);
            }
        }
        break;
    }
    default: {  // 6, 11, 13, 17 -> BC7 mode 5: the second plane's channel rotated into alpha
        o.mode = 5;
        o.rotation = (uint8_t)((c.ccs + 1u) & 3u);
        if (comps == 2) {
            o.low[0][0] = o.low[0][1] = o.low[0][2] = (uint8_t)((UQ[ep[0]] * 127 + 127) / 255);
            o.high[0][0] = o.high[0][1] = o.high[0][2] = (uint8_t)((UQ[ep[1]] * 127 + 127) / 255);
            o.low[0][3] = UQ[ep[2]]; o.high[0][3] = UQ[ep[3]];
        } else {
            for (uint32_t ac = 0; ac < 4; ac++) {
                const uint32_t bc = ac == c.ccs ? 3 : (ac == 3 ? c.ccs : ac);
                uint32_t l = 255, h = 255;
                if (ac < comps) { l = UQ[ep[ac * 2]]; h = UQ[ep[ac * 2 + 1]]; }
                if (bc < 3) { l = (l * 127 + 127) / 255; h = (h * 127 + 127) / 255; }
                o.low[0][bc] = (uint8_t)l; o.high[0][bc] = (uint8_t)h;
            }
        }
        for (uint32_t i = 0; i < 16; i++) {
            uint32_t cs = c.weights[i * 2], as = c.weights[i * 2 + 1];
            if (mode == 13) { cs = cs ? 3 : 0; as = as ? 3 : 0; }
            o.sel[i] = (uint8_t)cs; o.asel[i] = (uint8_t)as;
        }
        break;
    }
    }
}

// encode_bc7_block (:14657-14824) for the modes the transcoder produces (1, 2, 3, 5, 6, 7): an index whose top bit is set at a subset's anchor texel
// flips that subset (indices mirrored, endpoints and unique p-bits swapped), then the fields in the format's order
BU_FN void bc7_pack(bc7_fields& r, uint8_t* out16) {
    const uint32_t m = r.mode;
    const uint32_t subsets = (m == 2) ? 3u : ((m == 1 || m == 3 || m == 7) ? 2u : 1u);
    const uint32_t cbits = m == 1 ? 6u : ((m == 2 || m == 7) ? 5u : 7u), abits = m == 5 ? 8u : (m == 6 ? 7u : (m == 7 ? 5u : 0u));
    const uint32_t ibits = m == 1 ? 3u : (m == 6 ? 4u : 2u);
    const bool has_p = m == 1 || m == 3 || m == 6 || m == 7, shared_p = m == 1, sep_alpha = m == 5;
    const uint32_t part = subsets == 1 ? 0u : (subsets == 2 ? ku_bc7_part2[r.partition] : ku_bc7_part3[r.partition]);
    uint32_t anchor[3] = { 0, 99, 99 };
    if (subsets == 2) anchor[1] = ku_bc7_anchor2[r.partition];
    if (subsets == 3) { anchor[1] = ku_bc7_anchor3a[r.partition]; anchor[2] = ku_bc7_anchor3b[r.partition]; }
    for (uint32_t k = 0; k < subsets; k++) {
        if (r.sel[anchor[k]] & (1u << (ibits - 1))) {
            for (uint32_t i = 0; i < 16; i++)
                if (((part >> (2 * i)) & 3) == k) r.sel[i] = (uint8_t)(((1u << ibits) - 1) - r.sel[i]);
            for (uint32_t q = 0; q < (sep_alpha ? 3u : 4u); q++) { const uint8_t t = r.low[k][q]; r.low[k][q] = r.high[k][q]; r.high[k][q] = t; }
            if (!shared_p) { const uint32_t t = r.pbits[k][0]; r.pbits[k][0] = r.pbits[k][1]; r.pbits[k][1] = t; }
        }
        if (sep_alpha && (r.asel[anchor[k]] & 2u)) {
            for (uint32_t i = 0; i < 16; i++) r.asel[i] = (uint8_t)(3u - r.asel[i]);
            const uint8_t t = r.low[k][3]; r.low[k][3] = r.high[k][3]; r.high[k][3] = t;
        }
    }
    bits128 w = { 0, 0 };
    uint32_t pos = 0;
    put128(w, pos, 1u << m, m + 1); pos += m + 1;
    if (m == 5) { put128(w, pos, r.rotation, 2); pos += 2; }
    if (subsets > 1) { put128(w, pos, r.partition, 6); pos += 6; }
    const uint32_t total_comps = m >= 4 ? 4 : 3;
    for (uint32_t comp = 0; comp < total_comps; comp++)
        for (uint32_t s = 0; s < subsets; s++) {
            const uint32_t nb = comp == 3 ? abits : cbits;
            put128(w, pos, r.low[s][comp], nb); pos += nb;
            put128(w, pos, r.high[s][comp], nb); pos += nb;
        }
    if (has_p)
        for (uint32_t s = 0; s < subsets; s++) {
            put128(w, pos, r.pbits[s][0], 1); pos++;
            if (!shared_p) { put128(w, pos, r.pbits[s][1], 1); pos++; }
        }
    for (uint32_t i = 0; i < 16; i++) {
        const uint32_t nb = ibits - ((i == anchor[0] || i == anchor[1] || i == anchor[2]) ? 1u : 0u);
        put128(w, pos, r.sel[i], nb); pos += nb;
    }
    if (sep_alpha)
        for (uint32_t i = 0; i < 16; i++) {
            const uint32_t nb = 2u - (i == 0 ? 1u : 0u);
            put128(w, pos, r.asel[i], nb); pos += nb;
        }
    store128(w, out16);
}

BU_FN bool transcode_bc7(const uint8_t* blk, uint8_t* out16) {
    cand c;
    if (!unpack_block(blk, c)) return false;
    bc7_fields f;
    bc7_from_uastc(c, f);
    bc7_pack(f, out16);
    return true;
}

// ---- BC4: encode_bc4 (:17737-17855) of channel `chan` of 16 packed texels. The ramp is max, min and six values between them; a texel's code comes from
// counting the midpoints (scaled by 14) it reaches.
BU_FN uint64_t bc4_encode(const uint32_t* px, uint32_t chan) {
    uint32_t mn = 255, mx = 0;
    BU_UNROLL
    for (int i = 0; i < 16; i++) { const uint32_t v = (uint32_t)px_comp(px[i], (int)chan); mn = v < mn ? v : mn; mx = v > mx ? v : mx; }
    uint64_t out = (uint64_t)mx | ((uint64_t)mn << 8);
    if (mx == mn) return out;
    const int delta = (int)(mx - mn), bias = 4 - (int)mn * 14;
    BU_UNROLL
    for (int i = 0; i < 16; i++) {
        const int v = px_comp(px[i], (int)chan) * 14 + bias;
        const uint32_t k = (uint32_t)((v >= delta * 13) + (v >= delta * 11) + (v >= delta * 9) + (v >= delta * 7) + (v >= delta * 5) + (v >= delta * 3) + (v >= delta));
        const uint64_t code = (0x02345671u >> (4 * k)) & 7u;   // {1, 7, 6, 5, 4, 3, 2, 0}[k], one nibble each
        out |= code << (16 + 3 * i);
    }
    return out;
}
BU_FN uint64_t bc4_solid(uint32_t v) { return (uint64_t)v | ((uint64_t)v << 8); }   // write_bc4_solid_block

// ---- BC1 of a non-solid block: the hint0 shortcut, the hint1 selectors, or the full encoder (transcode_uastc_to_bc1, :18744-18757)
BU_FN bc1_blk bc1_from_uastc(const uint8_t* blk, const cand& c, const uint32_t* decoded, bool high_quality) {
    bool hint0, hint1;
    read_bc1_hints(blk, c.mode, hint0, hint1);
    const uint32_t passes = high_quality ? 2u : 1u;
    if (!high_quality && hint0) return bc1_hint0_block(c, bc1_translated_weights(c));
    if (hint1) return bc1_encode(decoded, true, bc1_hint1_selectors(bc1_translated_weights(c)), passes);
    return bc1_encode(decoded, false, 0, passes);
}
BU_FN uint64_t bc1_bits(const bc1_blk& b) { return (uint64_t)b.c0 | ((uint64_t)b.c1 << 16) | ((uint64_t)b.sel << 32); }

// The four BCn targets that go through the decoded texels. out[0] is the first 8 bytes, out[1] the second 8 (BC3, BC5). chan0 / chan1: BC4's channel, BC5's two.
BU_FN bool transcode_bcn(const uint8_t* blk, uint32_t target, bool high_quality, uint32_t chan0, uint32_t chan1, uint64_t* out) {
    cand c;
    if (!unpack_block(blk, c)) return false;
    if (c.mode == 8) {
        const uint64_t colour = bc1_bits(bc1_solid(c.endpoints[0], c.endpoints[1], c.endpoints[2]));
        if (target == TF_BC1_RGB) out[0] = colour;
        else if (target == TF_BC3_RGBA) { out[0] = bc4_solid(c.endpoints[3]); out[1] = colour; }
        else if (target == TF_BC4_R) out[0] = bc4_solid(c.endpoints[chan0]);
        else { out[0] = bc4_solid(c.endpoints[chan0]); out[1] = bc4_solid(c.endpoints[chan1]); }
        return true;
    }
    rgba8 dec[16];
    decode_uastc(c, dec);
    uint32_t px[16];
    BU_UNROLL
    for (int i = 0; i < 16; i++) px[i] = pack_px(dec[i].c);
    if (target == TF_BC1_RGB) out[0] = bc1_bits(bc1_from_uastc(blk, c, px, high_quality));
    else if (target == TF_BC3_RGBA) { out[0] = bc4_encode(px, 3); out[1] = bc1_bits(bc1_from_uastc(blk, c, px, high_quality)); }
    else if (target == TF_BC4_R) out[0] = bc4_encode(px, chan0);
    else { out[0] = bc4_encode(px, chan0); out[1] = bc4_encode(px, chan1); }
    return true;
}

BU_FN_HD uint32_t transcode_bytes_per_block(uint32_t target) {   // 0: not a supported target
    switch (target) {
    case TF_BC1_RGB: case TF_BC4_R: return 8;
    case TF_BC3_RGBA: case TF_BC5_RG: case TF_BC7_RGBA: case TF_ASTC_4x4_RGBA: return 16;
    case TF_RGBA32: return 64;
    default: return 0;
    }
}

// ------------------------------------------------------------------------------------------------------------------
// The texture family's further targets: ETC1, ETC2 RGBA, EAC R11 / RG11 and the 16-bit pixel formats. They are the consumers of the hints the encoder packs behind
// the mode code (uastc_core.h computes them): ETC1 flip / diff / intensity tables / bias, the EAC table and multiplier, and a solid block's ETC1 colour and selector.
// Everything is integer arithmetic but the one binary32 expression that places an EAC base value. The texels are the 16 packed dwords of transcode_bcn, every loop
// over them is unrolled, and nothing is indexed at run time but the two constant tables (ku_eac_tables by table, the intensity values as immediates).
// ------------------------------------------------------------------------------------------------------------------
enum { TF_ETC1_RGB = 0, TF_ETC2_RGBA = 1, TF_RGB565 = 14, TF_BGR565 = 15, TF_RGBA4444 = 16, TF_ETC2_EAC_R11 = 20, TF_ETC2_EAC_RG11 = 21 };

#if defined(__HIPCC__)
#define BU_NOUNROLL _Pragma("nounroll")
#else
#define BU_NOUNROLL
#endif

// the hint fields of unpack_uastc with read_hints (transcoder.cpp:15325-15371) that the BC1 route does not read. A solid block: diff, inten0, selector and r / g / b
// behind its colour; any other: flip, diff, the two intensity tables, the bias (modes that carry one) and the EAC byte (modes with alpha) behind the BC1 bits.
struct etc_hints { uint32_t flip, diff, inten0, inten1, bias, etc2, selector, r, g, b; };
BU_FN etc_hints read_etc_hints(const uint8_t* blk, uint32_t mode) {
    etc_hints h = { 0, 0, 0, 0, 0, 0, 0, 0, 0, 0 };
    uint32_t ofs = ku_mode_code_len[mode];
    if (mode == 8) {
        const uint32_t v = (uint32_t)block_bits(blk, ofs + 32, 21);
        h.diff = v & 1u; h.inten0 = (v >> 1) & 7u; h.selector = (v >> 4) & 3u; h.r = (v >> 6) & 31u; h.g = (v >> 11) & 31u; h.b = (v >> 16) & 31u;
        return h;
    }
    ofs += (ku_mode_has_bc1_hint0[mode] ? 1u : 0u) + (ku_mode_has_bc1_hint1[mode] ? 1u : 0u);
    const uint32_t v = (uint32_t)block_bits(blk, ofs, 21);
    h.flip = v & 1u; h.diff = (v >> 1) & 1u; h.inten0 = (v >> 2) & 7u; h.inten1 = (v >> 5) & 7u;
    uint32_t pos = 8;
    if (ku_mode_has_etc1_bias[mode]) { h.bias = (v >> pos) & 31u; pos += 5; }
    if (ku_mode_has_alpha[mode]) h.etc2 = (v >> pos) & 255u;
    return h;
}

// ---- ETC1: transcode_uastc_to_etc1 (:16720-16807) with etc1_determine_selectors (:16616-16686). The block's eight bytes, byte k at bits 8 k.
BU_FN uint32_t etc1_luma(uint32_t r, uint32_t g, uint32_t b) { return r * 54u + g * 183u + b * 19u; }
// the three luma midpoints (sums of neighbouring block colours' luma) of a sub-block whose base colour is r, g, b (8 bits each)
BU_FN void etc1_midpoints(int r, int g, int b, uint32_t table, uint32_t* mid) {
    const int small = etc1_inten_small(table), large = etc1_inten_large(table);
    const uint32_t y0 = etc1_luma((uint32_t)clampi(r - large, 0, 255), (uint32_t)clampi(g - large, 0, 255), (uint32_t)clampi(b - large, 0, 255));
    const uint32_t y1 = etc1_luma((uint32_t)clampi(r - small, 0, 255), (uint32_t)clampi(g - small, 0, 255), (uint32_t)clampi(b - small, 0, 255));
    const uint32_t y2 = etc1_luma((uint32_t)clampi(r + small, 0, 255), (uint32_t)clampi(g + small, 0, 255), (uint32_t)clampi(b + small, 0, 255));
    const uint32_t y3 = etc1_luma((uint32_t)clampi(r + large, 0, 255), (uint32_t)clampi(g + large, 0, 255), (uint32_t)clampi(b + large, 0, 255));
    mid[0] = y0 + y1; mid[1] = y1 + y2; mid[2] = y2 + y3;
}
BU_FN uint64_t etc1_solid(const etc_hints& h) {
    const uint32_t b3 = (h.diff << 1) | (h.inten0 << 5) | (h.inten0 << 2);
    const uint32_t r = h.diff ? h.r << 3 : (h.r | (h.r << 4)), g = h.diff ? h.g << 3 : (h.g | (h.g << 4)), b = h.diff ? h.b << 3 : (h.b | (h.b << 4));
    const uint32_t sel = h.selector == 0 ? 0xFFFFFFFFu : (h.selector == 1 ? 0x0000FFFFu : (h.selector == 2 ? 0u : 0xFFFF0000u));   // s_etc1_solid_selectors
    return (uint64_t)((r & 255u) | ((g & 255u) << 8) | ((b & 255u) << 16) | (b3 << 24)) | ((uint64_t)sel << 32);
}
BU_FN uint64_t etc1_from_hints(uint32_t mode, const etc_hints& h, const uint32_t* px) {
    const bool flip = h.flip != 0, diff = h.diff != 0;
    const uint32_t limit = diff ? 31u : 15u;
    // sums over the four 2x2 quadrants, q[2 * (y >> 1) + (x >> 1)]: a sub-block is two of them, which two the flip bit says
    uint32_t q[4][3] = { { 0, 0, 0 }, { 0, 0, 0 }, { 0, 0, 0 }, { 0, 0, 0 } };
    BU_UNROLL
    for (int i = 0; i < 16; i++) {
        BU_UNROLL
        for (int c = 0; c < 3; c++) q[2 * (i >> 3) + ((i >> 1) & 1)][c] += (uint32_t)px_comp(px[i], c);
    }
    uint32_t col[2][3];
    BU_UNROLL
    for (int c = 0; c < 3; c++) {
        const uint32_t s0 = q[0][c] + (flip ? q[1][c] : q[2][c]), s1 = q[3][c] + (flip ? q[2][c] : q[1][c]);
        col[0][c] = (s0 * limit + 1020u) / 2040u;
        col[1][c] = (s1 * limit + 1020u) / 2040u;
        if (ku_mode_has_etc1_bias[mode]) {
            col[0][c] = etc1_bias_apply(col[0][c], (uint32_t)c, h.bias, limit, 0);
            col[1][c] = etc1_bias_apply(col[1][c], (uint32_t)c, h.bias, limit, 1);
        }
    }
    uint32_t bytes = ((uint32_t)flip | ((uint32_t)diff << 1) | (h.inten0 << 5) | (h.inten1 << 2)) << 24;
    int base[2][3];   // the two sub-blocks' base colours as the written block decodes them (decoder_etc_block::get_block_colors)
    BU_UNROLL
    for (int c = 0; c < 3; c++) {
        if (diff) {
            const int d = clampi((int)col[1][c] - (int)col[0][c], -4, 3);
            bytes |= (((col[0][c] << 3) | (uint32_t)(d < 0 ? d + 8 : d)) & 255u) << (8 * c);
            const int c1 = clampi((int)col[0][c] + d, 0, 31);
            base[0][c] = (int)((col[0][c] << 3) | (col[0][c] >> 2));
            base[1][c] = (c1 << 3) | (c1 >> 2);
        } else {
            bytes |= ((col[1][c] | (col[0][c] << 4)) & 255u) << (8 * c);
            base[0][c] = (int)((col[0][c] << 4) | col[0][c]);
            base[1][c] = (int)((col[1][c] << 4) | col[1][c]);
        }
    }
    uint32_t mid0[3], mid1[3];
    etc1_midpoints(base[0][0], base[0][1], base[0][2], h.inten0, mid0);
    etc1_midpoints(base[1][0], base[1][1], base[1][2], h.inten1, mid1);
    // texel (x, y) sits at bit x * 4 + y of both masks, whichever way the block is split; its luma is weighted twice the block colours'
    uint32_t lmask = 0, hmask = 0;
    BU_UNROLL
    for (int i = 0; i < 16; i++) {
        const int x = i & 3, y = i >> 2;
        const bool second = flip ? y >= 2 : x >= 2;
        const uint32_t l = (uint32_t)px_comp(px[i], 0) * 108u + (uint32_t)px_comp(px[i], 1) * 366u + (uint32_t)px_comp(px[i], 2) * 38u;
        const uint32_t below = (l < (second ? mid1[0] : mid0[0]) ? 1u : 0u) + (l < (second ? mid1[1] : mid0[1]) ? 1u : 0u) + (l < (second ? mid1[2] : mid0[2]) ? 1u : 0u);
        const uint32_t t = (0x3201u >> (4 * below)) & 3u;   // s_tran = { 1, 0, 2, 3 }
        lmask |= (t & 1u) << (x * 4 + y);
        hmask |= (t >> 1) << (x * 4 + y);
    }
    const uint32_t sel = (hmask >> 8) | ((hmask & 255u) << 8) | ((lmask >> 8) << 16) | ((lmask & 255u) << 24);   // bytes 4..7: h high, h low, l high, l low
    return (uint64_t)bytes | ((uint64_t)sel << 32);
}

// ---- EAC: an eac_block (:1447-1497) as its eight bytes -- base, table | multiplier << 4, then the 48 selector bits most significant byte first. Texel (x, y) has its
// three bits at 45 - 3 (x * 4 + y): s_etc2_eac_bit_ofs of pack_eac's raster order, and the a8 route's block_pixels[i & 3][i >> 2] at 45 - 3 i.
BU_FN uint64_t eac_block(uint32_t base, uint32_t table, uint32_t mul, uint64_t sels48) {
    return (uint64_t)(base & 255u) | ((uint64_t)((table & 15u) | ((mul & 15u) << 4)) << 8) | __builtin_bswap64(sels48);
}
BU_FN uint32_t eac_selector_shift(int i) { return 45u - 3u * (uint32_t)((i & 3) * 4 + (i >> 2)); }   // i: raster index
enum : uint64_t { EAC_ALL_FOUR = 0x924924924924ull };   // g_etc2_eac_a8_sel4: every selector 4, the table's smallest positive step
BU_FN void eac_table_values(uint32_t table, int* tv) {
    const signed char* T = ku_eac_tables + (table & 15u) * 8;
    BU_UNROLL
    for (int s = 0; s < 8; s++) tv[s] = T[s];
}
// the base value that puts the table's span over [mn, mx]: (int)roundf(lerp(mn, mx, -table[3] / range)), binary32, every operation rounded on its own
BU_FN int eac_center(const int* tv, uint32_t mn, uint32_t mx) {
    const float range = (float)(tv[7] - tv[3]);
    const float t = (float)(0 - tv[3]) / range;
    const float a = (float)mn, b = (float)mx;
    return (int)roundf(a + (b - a) * t);
}
// min over the eight selectors of |value - a| << 3 | selector: the nearest value, the lowest selector on a tie. clamped: the table's values clamp to 0..255 first.
BU_FN uint32_t eac_nearest(const int* tv, int mul, int base, int a, bool clamped) {
    uint32_t l = 0xFFFFFFFFu;
    BU_UNROLL
    for (int s = 0; s < 8; s++) {
        int v = mul * tv[s] + base;
        if (clamped) v = clampi(v, 0, 255);
        v -= a;
        const uint32_t e = ((uint32_t)(v < 0 ? -v : v) << 3) | (uint32_t)s;
        l = e < l ? e : l;
    }
    return l;
}

// transcode_uastc_to_etc2_eac_a8 (:17629-17704) of a block that is not solid: the hint's table and multiplier (0 is computed through, as the release build does)
BU_FN uint64_t eac_a8_from_hint(uint32_t mode, const etc_hints& h, const uint32_t* px) {
    if (!ku_mode_has_alpha[mode]) return eac_block(255, 13, 1, EAC_ALL_FOUR);
    uint32_t mn = 255, mx = 0;
    BU_UNROLL
    for (int i = 0; i < 16; i++) { const uint32_t a = px[i] >> 24; mn = a < mn ? a : mn; mx = a > mx ? a : mx; }
    if (mn == mx) return eac_block(mn, 13, 1, EAC_ALL_FOUR);
    const uint32_t table = h.etc2 & 15u;
    const int mul = (int)(h.etc2 >> 4);
    int tv[8];
    eac_table_values(table, tv);
    const int center = eac_center(tv, mn, mx);
    uint64_t sels = 0;
    BU_UNROLL
    for (int i = 0; i < 16; i++) sels |= (uint64_t)(eac_nearest(tv, mul, center, (int)(px[i] >> 24), true) & 7u) << eac_selector_shift(i);
    return eac_block((uint32_t)center, table, (uint32_t)mul, sels);
}

// pack_eac (:18880-19034: tables 2, 8, 11, 13; values clamp only for a texel below 7 or above 248) and pack_eac_high_quality (:19037-19155: all 16, always clamped)
// of 16 values. Each table's squared error is accumulated first and the winner's selectors derived again, so no selector array is kept; the first table wins a tie.
template <bool HQ>
BU_FN uint64_t eac_pack(const int* a) {
    int mn = 255, mx = 0;
    BU_UNROLL
    for (int i = 0; i < 16; i++) { mn = a[i] < mn ? a[i] : mn; mx = a[i] > mx ? a[i] : mx; }
    if (mn == mx) return eac_block((uint32_t)mn, 13, 0, EAC_ALL_FOUR);   // pack_eac_solid_block: multiplier 0
    if (mx - mn <= 5) {   // table 13 with multiplier 1 reaches -3..2 around its base: lossless
        const int base = clampi(mx - 2, 0, 255);
        uint64_t sels = 0;
        BU_UNROLL
        for (int i = 0; i < 16; i++) sels |= (uint64_t)((0x654012u >> (4 * (a[i] - (base - 3)))) & 7u) << eac_selector_shift(i);   // { 2, 1, 0, 4, 5, 6 }[a - (base - 3)]
        return eac_block((uint32_t)base, 13, 1, sels);
    }
    uint32_t best_err = 0xFFFFFFFFu, best_table = 0;
    int best_base = 0, best_mul = 1;
    BU_NOUNROLL
    for (uint32_t k = 0; k < (HQ ? 16u : 4u); k++) {
        const uint32_t table = HQ ? k : ((0xDB82u >> (4 * k)) & 15u);
        int tv[8];
        eac_table_values(table, tv);
        const int base = clampi(eac_center(tv, (uint32_t)mn, (uint32_t)mx), 0, 255);
        const int mul = clampi((int)roundf((float)(uint32_t)(mx - mn) / (float)(tv[7] - tv[3])), 1, 15);
        uint32_t err = 0;
        BU_UNROLL
        for (int i = 0; i < 16; i++) {
            const uint32_t d = eac_nearest(tv, mul, base, a[i], HQ || a[i] < 7 || a[i] > 248) >> 3;
            err += d * d;
        }
        if (err < best_err) { best_err = err; best_table = table; best_base = base; best_mul = mul; }
    }
    int tv[8];
    eac_table_values(best_table, tv);
    uint64_t sels = 0;
    BU_UNROLL
    for (int i = 0; i < 16; i++) sels |= (uint64_t)(eac_nearest(tv, best_mul, best_base, a[i], HQ || a[i] < 7 || a[i] > 248) & 7u) << eac_selector_shift(i);
    return eac_block((uint32_t)best_base, best_table, (uint32_t)best_mul, sels);
}
template <bool HQ>
BU_FN uint64_t eac_pack_channel(const uint32_t* px, uint32_t chan) {
    int a[16];
    BU_UNROLL
    for (int i = 0; i < 16; i++) a[i] = px_comp(px[i], (int)chan);
    return eac_pack<HQ>(a);
}

// The block targets of the texture family that the first family does not have. out[0] is the first 8 bytes, out[1] the second 8 (ETC2 RGBA: the EAC A8 block, then
// the ETC1 block; RG11: chan0's block, then chan1's). chan0 / chan1: R11's channel, RG11's two; channel 3 of a block that is not solid goes the hint's way.
template <uint32_t TARGET, bool HQ>
BU_FN bool transcode_etc(const uint8_t* blk, uint32_t chan0, uint32_t chan1, uint64_t* out) {
    cand c;
    if (!unpack_block(blk, c)) return false;
    const etc_hints h = read_etc_hints(blk, c.mode);
    if (c.mode == 8) {
        if (TARGET == TF_ETC1_RGB) out[0] = etc1_solid(h);
        else if (TARGET == TF_ETC2_RGBA) { out[0] = eac_block(c.endpoints[3], 13, 1, EAC_ALL_FOUR); out[1] = etc1_solid(h); }
        else {
            out[0] = eac_block(c.endpoints[chan0], 13, 0, EAC_ALL_FOUR);
            if (TARGET == TF_ETC2_EAC_RG11) out[1] = eac_block(c.endpoints[chan1], 13, 0, EAC_ALL_FOUR);
        }
        return true;
    }
    rgba8 dec[16];
    decode_uastc(c, dec);
    uint32_t px[16];
    BU_UNROLL
    for (int i = 0; i < 16; i++) px[i] = pack_px(dec[i].c);
    if (TARGET == TF_ETC1_RGB) out[0] = etc1_from_hints(c.mode, h, px);
    else if (TARGET == TF_ETC2_RGBA) { out[0] = eac_a8_from_hint(c.mode, h, px); out[1] = etc1_from_hints(c.mode, h, px); }
    else {
        out[0] = chan0 == 3 ? eac_a8_from_hint(c.mode, h, px) : eac_pack_channel<HQ>(px, chan0);
        if (TARGET == TF_ETC2_EAC_RG11) out[1] = chan1 == 3 ? eac_a8_from_hint(c.mode, h, px) : eac_pack_channel<HQ>(px, chan1);
    }
    return true;
}

// one texel of a 16-bit pixel target (transcode_slice, :10246-10302)
template <uint32_t TARGET>
BU_FN uint32_t pack_pixel16(const rgba8& p) {
    if (TARGET == TF_RGB565) return bu::pack_rgb565(p.c[0], p.c[1], p.c[2]);
    if (TARGET == TF_BGR565) return bu::pack_rgb565(p.c[2], p.c[1], p.c[0]);
    return bu::pack_rgba4444(p.c[0], p.c[1], p.c[2], p.c[3]);
}

// the texture family's unit: bytes per block of a block target, per pixel of a pixel target; 0: not a target of the family
BU_FN_HD bool texture_is_pixel_target(uint32_t target) { return target == TF_RGBA32 || target == TF_RGB565 || target == TF_BGR565 || target == TF_RGBA4444; }
BU_FN_HD uint32_t texture_unit_bytes(uint32_t target) {
    switch (target) {
    case TF_ETC1_RGB: case TF_ETC2_EAC_R11: return 8;
    case TF_ETC2_RGBA: case TF_ETC2_EAC_RG11: return 16;
    case TF_RGB565: case TF_BGR565: case TF_RGBA4444: return 2;
    case TF_RGBA32: return 4;
    default: return transcode_bytes_per_block(target);
    }
}

}  // namespace bu_uastc
