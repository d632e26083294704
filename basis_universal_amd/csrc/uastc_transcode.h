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
// Out of scope: ETC1 / ETC2 / EAC / PVRTC1 targets (mobile formats a CDNA GPU does not sample), the 16-bit pixel formats, ETC1S slices, UASTC HDR /
// ASTC LDR / XUASTC blocks, Zstandard-supercompressed KTX2 levels. Callers refuse those; nothing is silently mapped to another target.
#pragma once
#include "uastc_rdo.h"
#include "uastc_transcode_tables.inc"

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

}  // namespace bu_uastc
