// etc1s_vendor_format_targets.h -- the per-block conversions of the fourth ETC1S entry family's targets, included by etc1s_transcode_kernels.hip after
// etc1s_block_format_targets.h: ATC RGB (transcoder/basisu_transcoder.cpp: convert_etc1s_to_atc 6476), PVRTC2 4bpp RGB (convert_etc1s_to_pvrtc2_rgb 7153) and RGBA
// (convert_etc1s_to_pvrtc2_rgba 7285), and FXT1 (convert_etc1s_to_fxt1 2573 over etc1s_bc1.h's to_bc1<false>). A block is built in registers and written with one
// store, and no array is indexed by a run-time value: selectors are translated through packed words (map_selectors), the four block colours picked by selects (pick4).
#pragma once

namespace bu {

enum : uint32_t { kAtcEntries = 8 * 32 * 6 * 10, kAtcTableWords = 3 * kAtcEntries };   // the look-ups 55, 56 and 45, in that order

// ---- ATC RGB and PVRTC2 4bpp RGB: one conversion over different endpoint widths. Both formats have four values per block in linear order, lo, (5 lo + 3 hi) / 8,
// (3 lo + 5 hi) / 8, hi, so the selectors of a mapping go in as they are. ATC: low colour 555, high colour 565. PVRTC2 (hard, non-interpolated, opaque): low 554, high 555.
struct atc_solution { uint32_t lo, hi, sels; };   // lo, hi: the endpoint codes r | g << 8 | b << 16
__device__ __forceinline__ uint32_t code3(const unsigned char* tr, const unsigned char* tg, const unsigned char* tb, uint32_t c, uint32_t stride, uint32_t at) {
    return (uint32_t)tr[(c & 255u) * stride + at] | ((uint32_t)tg[((c >> 8) & 255u) * stride + at] << 8) | ((uint32_t)tb[(c >> 16) * stride + at] << 16);
}
// tables: launch_etc1s_build_atc_tables' words. The three routes, in the reference's order: one selector -> the pair whose value 1 is nearest, every selector 1; the
// widest table's two extremes alone -> the nearest endpoint each, selectors as they are; else the look-ups under the mapping of least summed error, first on ties.
template <bool PVRTC2>
__device__ __forceinline__ atc_solution atc_solve(const etc1s_entry& e, uint32_t sel, const uint32_t* tables) {
    const selector_use u = selector_use_of(sel);
    uint32_t colors[4];
    block_colors(e, colors);
    if (u.n == 1u) {
        const uint32_t c = pick4(colors, u.low);
        const unsigned char *sg = PVRTC2 ? ke_atc_solid55 : ke_atc_solid56, *sb = PVRTC2 ? ke_atc_solid45 : ke_atc_solid55;
        return atc_solution{ code3(ke_atc_solid55, sg, sb, c, 2u, 0u), code3(ke_atc_solid55, sg, sb, c, 2u, 1u), 0x55555555u };
    }
    if (is_outlier(e.table, u))
        return atc_solution{ code3(ke_atc_end5, ke_atc_end5, PVRTC2 ? ke_atc_end4 : ke_atc_end5, colors[0], 1u, 0u),
                             code3(ke_atc_end5, PVRTC2 ? ke_atc_end5 : ke_atc_end6, ke_atc_end5, colors[3], 1u, 0u), sel };
    const uint32_t range = ke_bc1_range_index[u.low * 4u + u.high];
    const uint32_t *t55 = tables, *t56 = tables + kAtcEntries, *t45 = tables + 2u * kAtcEntries;
    const uint32_t *tr = astc_entry(t55, e.table, e.r5, range), *tg = astc_entry(PVRTC2 ? t55 : t56, e.table, e.g5, range), *tb = astc_entry(PVRTC2 ? t45 : t55, e.table, e.b5, range);
    const uint32_t m = astc_best_mapping(tr, tg, tb), r = tr[m], g = tg[m], b = tb[m];
    return atc_solution{ (r & 255u) | ((g & 255u) << 8) | ((b & 255u) << 16), ((r >> 8) & 255u) | (((g >> 8) & 255u) << 8) | (((b >> 8) & 255u) << 16),
                         map_selectors(sel, mapping_word(m)) };   // the identity mapping (6) leaves them as they are
}
__device__ __forceinline__ uint2 to_atc(const etc1s_entry& e, uint32_t sel, const uint32_t* tables) {
    const atc_solution s = atc_solve<false>(e, sel, tables);
    const uint32_t lo = ((s.lo & 255u) << 10) | (((s.lo >> 8) & 255u) << 5) | (s.lo >> 16), hi = ((s.hi & 255u) << 11) | (((s.hi >> 8) & 255u) << 5) | (s.hi >> 16);
    return make_uint2(lo | (hi << 16), s.sels);
}
// the colour word: bit 0 the modulation flag (0), blue a from bit 1 (4 bits), green a 5, red a 10, the hard flag 15, blue b 16, green b 21, red b 26, opaque 31
__device__ __forceinline__ uint2 to_pvrtc2_rgb(const etc1s_entry& e, uint32_t sel, const uint32_t* tables) {
    const atc_solution s = atc_solve<true>(e, sel, tables);
    return make_uint2(s.sels, ((s.lo >> 16) << 1) | (((s.lo >> 8) & 255u) << 5) | ((s.lo & 255u) << 10) | (1u << 15) | ((s.hi >> 16) << 16) | (((s.hi >> 8) & 255u) << 21) |
                                  ((s.hi & 255u) << 26) | (1u << 31));
}

// ---- PVRTC2 4bpp RGBA (convert_etc1s_to_pvrtc2_rgba 7285): hard, translucent blocks, re-encoded per pixel from the colour block (e, sel) and the alpha block (ae,
// asel: alpha is the green channel of its block colours). Colour a is 4433, colour b 4443; a's alpha expands as a << 1, b's as (a << 1) | 1, both to 8 bits by
// replication, so b's alpha is never 0. A constant alpha >= 250 takes the RGB route. A constant colour with constant alpha chooses between modulation 0, 1 and 3
// everywhere. Any other block gets its two bounds one of four ways (constant colour; constant alpha; the 4D incremental PCA where a colour or alpha clamped; the integer
// 2D test), quantises them, and places each texel by three integer thresholds along the axis. The float work is binary32 in the reference's operation order: sums of
// products are left to right, and nothing may be contracted into a fused multiply-add (the library is built with -ffp-contract=off).
struct vec4f { float x, y, z, w; };
__device__ __forceinline__ float dot4(const vec4f& a, const vec4f& b) { return a.x * b.x + a.y * b.y + a.z * b.z + a.w * b.w; }
__device__ __forceinline__ vec4f normalized4(vec4f v) {
    float s = v.x * v.x + v.y * v.y + v.z * v.z + v.w * v.w;
    if (s != 0.0f) { s = 1.0f / sqrtf(s); v.x *= s; v.y *= s; v.z *= s; v.w *= s; }
    return v;
}
__device__ __forceinline__ float saturate1(float v) { if (v < 0.0f) v = 0.0f; else if (v > 1.0f) v = 1.0f; return v; }
__device__ __forceinline__ vec4f saturate4(const vec4f& v) { return vec4f{ saturate1(v.x), saturate1(v.y), saturate1(v.z), saturate1(v.w) }; }
__device__ __forceinline__ vec4f rgba_over_255(uint32_t c, uint32_t a) {
    const float S = 1.0f / 255.0f;
    return vec4f{ (float)(c & 255u) * S, (float)((c >> 8) & 255u) * S, (float)(c >> 16) * S, (float)a * S };
}
// colour a (r4 g4 b3 a3) and colour b (r4 g4 b4 a3) -> the colour word: modulation flag 0 at bit 0, blue a from bit 1, green a 4, red a 8, alpha a 12, hard flag 15, blue b
// 16, green b 20, red b 24, alpha b 28, opaque flag (0) 31
__device__ __forceinline__ uint32_t pvrtc2_trans_word(uint32_t ra, uint32_t ga, uint32_t ba, uint32_t aa, uint32_t rb, uint32_t gb, uint32_t bb, uint32_t ab) {
    return (ba << 1) | (ga << 4) | (ra << 8) | (aa << 12) | (1u << 15) | (bb << 16) | (gb << 20) | (rb << 24) | (ab << 28);
}
__device__ __forceinline__ uint32_t x4to8(uint32_t c) { c = (c << 1) | (c >> 3); return (c << 3) | (c >> 2); }   // 4 bits to 5, then to 8
__device__ __forceinline__ uint32_t x3to8(uint32_t c) { c = (c << 2) | (c >> 1); return (c << 3) | (c >> 2); }
__device__ __forceinline__ uint32_t sq_diff(uint32_t a, uint32_t b) { const int d = (int)a - (int)b; return (uint32_t)(d * d); }
__device__ __forceinline__ uint32_t threshold_code(int d, int t01, int t12, int t23) { return (uint32_t)(d >= t23) + (uint32_t)(d >= t12) + (uint32_t)(d >= t01); }

// four values picked by a selector, as selects over scalars
struct quad { uint32_t v0, v1, v2, v3; };
__device__ __forceinline__ uint32_t pickq(const quad& q, uint32_t s) { const uint32_t lo = (s & 1u) ? q.v1 : q.v0, hi = (s & 1u) ? q.v3 : q.v2; return (s & 2u) ? hi : lo; }

__device__ __forceinline__ uint2 to_pvrtc2_rgba(const etc1s_entry& e, uint32_t sel, const etc1s_entry& ae, uint32_t asel, const uint32_t* tables) {
    const selector_use u = selector_use_of(sel), au = selector_use_of(asel);
    uint32_t colors_of[4];
    block_colors(e, colors_of);
    const quad colors = { colors_of[0], colors_of[1], colors_of[2], colors_of[3] }, av = { green_of(ae, 0u), green_of(ae, 1u), green_of(ae, 2u), green_of(ae, 3u) };
    const uint32_t c_low = pickq(colors, u.low), c_high = pickq(colors, u.high), a_low = pickq(av, au.low), a_high = pickq(av, au.high);
    bool constant_alpha = true, solid = true;   // over the selectors of the range, used or not
#pragma unroll
    for (uint32_t s = 1; s < 4; s++) {
        if (s > au.low && s <= au.high && pickq(av, s) != a_low) constant_alpha = false;
        if (s > u.low && s <= u.high && pickq(colors, s) != c_low) solid = false;
    }
    if (constant_alpha && a_low >= 250u) return to_pvrtc2_rgb(e, sel, tables);
    if (solid && constant_alpha) {
        const uint32_t r = c_low & 255u, g = (c_low >> 8) & 255u, b = c_low >> 16, a = a_low;
        const uint32_t lr0 = (r * 15u + 128u) / 255u, lg0 = (g * 15u + 128u) / 255u, lb0 = (b * 7u + 128u) / 255u, la0 = ke_pvrtc2_alpha33_0[a];
        const uint32_t err0 = sq_diff(x4to8(lr0), r) + sq_diff(x4to8(lg0), g) + sq_diff(x3to8(lb0), b) + sq_diff((la0 << 1) * 17u, a) * 2u;
        if (err0 == 0u || a < 3u) return make_uint2(0u, pvrtc2_trans_word(lr0, lg0, lb0, la0, 0u, 0u, 0u, 0u));
        const uint32_t lb3 = (b * 15u + 128u) / 255u, la3 = ke_pvrtc2_alpha33_3[a];
        const uint32_t err3 = sq_diff(x4to8(lr0), r) + sq_diff(x4to8(lg0), g) + sq_diff(x4to8(lb3), b) + sq_diff(((la3 << 1) | 1u) * 17u, a) * 2u;
        const uint32_t lr1 = ke_pvrtc2_trans44[r * 2u], hr1 = ke_pvrtc2_trans44[r * 2u + 1u], lg1 = ke_pvrtc2_trans44[g * 2u], hg1 = ke_pvrtc2_trans44[g * 2u + 1u];
        const uint32_t lb1 = ke_pvrtc2_trans34[b * 2u], hb1 = ke_pvrtc2_trans34[b * 2u + 1u], la1 = ke_pvrtc2_alpha33[a * 2u], ha1 = ke_pvrtc2_alpha33[a * 2u + 1u];
        const uint32_t r1 = (x4to8(lr1) * 5u + x4to8(hr1) * 3u) / 8u, g1 = (x4to8(lg1) * 5u + x4to8(hg1) * 3u) / 8u, b1 = (x3to8(lb1) * 5u + x4to8(hb1) * 3u) / 8u;
        const uint32_t a1 = ((la1 << 1) * 17u * 5u + ((ha1 << 1) | 1u) * 17u * 3u) / 8u;
        const uint32_t err1 = sq_diff(r1, r) + sq_diff(g1, g) + sq_diff(b1, b) + sq_diff(a1, a) * 2u;
        if (err1 < err0 && err1 < err3) return make_uint2(0x55555555u, pvrtc2_trans_word(lr1, lg1, lb1, la1, hr1, hg1, hb1, ha1));
        if (err0 < err3) return make_uint2(0u, pvrtc2_trans_word(lr0, lg0, lb0, la0, 0u, 0u, 0u, 0u));
        return make_uint2(0xFFFFFFFFu, pvrtc2_trans_word(0u, 0u, 0u, 0u, lr0, lg0, lb3, la3));
    }
    vec4f lo, hi;
    const bool clamped = (c_low & 255u) == 0u || (c_high & 255u) == 255u || ((c_low >> 8) & 255u) == 0u || ((c_high >> 8) & 255u) == 255u || (c_low >> 16) == 0u ||
                         (c_high >> 16) == 255u || a_low == 0u || a_high == 255u;
    if (solid) {
        lo = rgba_over_255(c_low, a_low); hi = rgba_over_255(c_low, a_high);
    } else if (constant_alpha) {
        lo = rgba_over_255(c_low, a_low); hi = rgba_over_255(c_high, a_low);
    } else if (clamped) {   // the principal axis of the sixteen RGBA pixels, by an incremental estimate
        uint32_t sr = 0, sg = 0, sb = 0, sa = 0;
#pragma unroll
        for (uint32_t p = 0; p < 16; p++) {
            const uint32_t c = pickq(colors, (sel >> (2u * p)) & 3u);
            sr += c & 255u; sg += (c >> 8) & 255u; sb += c >> 16; sa += pickq(av, (asel >> (2u * p)) & 3u);
        }
        const vec4f sum = { (float)sr, (float)sg, (float)sb, (float)sa };
        const float k16 = 1.0f / 16.0f, k4080 = 1.0f / (float)(16.0f * 255.0f);
        const vec4f mean16 = { sum.x * k16, sum.y * k16, sum.z * k16, sum.w * k16 };
        const vec4f mean = saturate4(vec4f{ sum.x * k4080, sum.y * k4080, sum.z * k4080, sum.w * k4080 });
        vec4f axis = { 0.0f, 0.0f, 0.0f, 0.0f };
#pragma unroll
        for (uint32_t p = 0; p < 16; p++) {
            const uint32_t c = pickq(colors, (sel >> (2u * p)) & 3u);
            const vec4f q = { (float)(c & 255u) - mean16.x, (float)((c >> 8) & 255u) - mean16.y, (float)(c >> 16) - mean16.z, (float)pickq(av, (asel >> (2u * p)) & 3u) - mean16.w };
            const vec4f qa = { q.x * q.x, q.y * q.x, q.z * q.x, q.w * q.x }, qb = { q.x * q.y, q.y * q.y, q.z * q.y, q.w * q.y };
            const vec4f qc = { q.x * q.z, q.y * q.z, q.z * q.z, q.w * q.z }, qd = { q.x * q.w, q.y * q.w, q.z * q.w, q.w * q.w };
            const vec4f n = normalized4(p ? axis : q);
            axis.x += dot4(qa, n); axis.y += dot4(qb, n); axis.z += dot4(qc, n); axis.w += dot4(qd, n);
        }
        axis = normalized4(axis);
        if (dot4(axis, axis) < .5f) axis = vec4f{ .5f, .5f, .5f, .5f };
        float l = 1e+9f, h = -1e+9f;
#pragma unroll
        for (uint32_t p = 0; p < 16; p++) {
            const uint32_t c = pickq(colors, (sel >> (2u * p)) & 3u);
            const vec4f q = { (float)(c & 255u) - mean16.x, (float)((c >> 8) & 255u) - mean16.y, (float)(c >> 16) - mean16.z, (float)pickq(av, (asel >> (2u * p)) & 3u) - mean16.w };
            const float d = dot4(q, axis);
            l = l < d ? l : d;
            h = h > d ? h : d;
        }
        l *= 1.0f / 255.0f;
        h *= 1.0f / 255.0f;
        lo = saturate4(vec4f{ mean.x + axis.x * l, mean.y + axis.y * l, mean.z + axis.z * l, mean.w + axis.w * l });
        hi = saturate4(vec4f{ mean.x + axis.x * h, mean.y + axis.y * h, mean.z + axis.z * h, mean.w + axis.w * h });
        if (lo.w > hi.w) { const vec4f t = lo; lo = hi; hi = t; }
    } else {   // nothing clamped: colour moves along luma alone, and only whether alpha rises or falls with it is open
        const quad L = { rgb_sum(colors.v0), rgb_sum(colors.v1), rgb_sum(colors.v2), rgb_sum(colors.v3) }, A = { av.v0 * 3u, av.v1 * 3u, av.v2 * 3u, av.v3 * 3u };
        int p0_min = 0x7FFFFFFF, p0_max = -0x7FFFFFFF - 1, p1_min = 0x7FFFFFFF, p1_max = -0x7FFFFFFF - 1;
#pragma unroll
        for (uint32_t p = 0; p < 16; p++) {
            const int lum = (int)pickq(L, (sel >> (2u * p)) & 3u), alp = (int)pickq(A, (asel >> (2u * p)) & 3u), p0 = lum + alp, p1 = lum - alp;
            p0_min = p0 < p0_min ? p0 : p0_min; p0_max = p0 > p0_max ? p0 : p0_max;
            p1_min = p1 < p1_min ? p1 : p1_min; p1_max = p1 > p1_max ? p1 : p1_max;
        }
        lo = rgba_over_255(c_low, a_low); hi = rgba_over_255(c_high, a_high);
        if (p1_max - p1_min > p0_max - p0_min) { const vec4f t = lo; lo.x = hi.x; lo.y = hi.y; lo.z = hi.z; hi.x = t.x; hi.y = t.y; hi.z = t.z; }
    }
    const uint32_t ra = (uint32_t)(int)(lo.x * 15.0f + .5f), ga = (uint32_t)(int)(lo.y * 15.0f + .5f), ba = (uint32_t)(int)(lo.z * 7.0f + .5f), aa = (uint32_t)(int)(lo.w * 7.0f + .5f);
    const uint32_t rb = (uint32_t)(int)(hi.x * 15.0f + .5f), gb = (uint32_t)(int)(hi.y * 15.0f + .5f), bb = (uint32_t)(int)(hi.z * 15.0f + .5f), ab = (uint32_t)(int)(hi.w * 7.0f + .5f);
    const int lr = (int)x4to8(ra), lg = (int)x4to8(ga), lb = (int)x3to8(ba), la = (int)((aa << 1) * 17u);
    const int axis_r = (int)x4to8(rb) - lr, axis_g = (int)x4to8(gb) - lg, axis_b = (int)x4to8(bb) - lb, axis_a = (int)(((ab << 1) | 1u) * 17u) - la;
    const int len = axis_r * axis_r + axis_g * axis_g + axis_b * axis_b + axis_a * axis_a, t01 = (len * 3) / 16, t12 = len >> 1, t23 = (len * 13) / 16;
    // each selector's place along the axis, as two's complement words for pickq
    const auto along = [&](uint32_t c) { return (uint32_t)(((int)(c & 255u) - lr) * axis_r + ((int)((c >> 8) & 255u) - lg) * axis_g + ((int)(c >> 16) - lb) * axis_b); };
    const auto along_alpha = [&](uint32_t a) { return (uint32_t)(((int)a - la) * axis_a); };
    const quad cy = { along(colors.v0), along(colors.v1), along(colors.v2), along(colors.v3) }, ca = { along_alpha(av.v0), along_alpha(av.v1), along_alpha(av.v2), along_alpha(av.v3) };
    const bool alpha_only = (axis_r | axis_g | axis_b) == 0;
    uint32_t mod = 0;
#pragma unroll
    for (uint32_t p = 0; p < 16; p++) {
        const int d = (alpha_only ? 0 : (int)pickq(cy, (sel >> (2u * p)) & 3u)) + (int)pickq(ca, (asel >> (2u * p)) & 3u);
        mod |= threshold_code(d, t01, t12, t23) << (2u * p);
    }
    return make_uint2(mod, pvrtc2_trans_word(ra, ga, ba, aa, rb, gb, bb, ab));
}

// ---- FXT1, CC_MIXED without alpha: an 8x4 block is two BC1-like halves. Bytes 0-7 the 2-bit selectors (left half, then right half, a byte per row each); then 64
// bits: four 15-bit colours b | g << 5 | r << 10 from bit 0 (colours 0 and 1 the left half's pair, 2 and 3 the right's), alpha at bit 60, the green lsb of each half
// at bits 61 and 62, mode at bit 63. A half's green has 6 bits: 5 in the colour, the lsb of colour 1 in the glsb field, and the lsb of colour 0 is implied as
// glsb ^ the top bit of the half's first selector -- so where that does not hold the two colours trade places and the selectors are inverted.
struct fxt1_half { uint32_t c0, c1, g1, sels; };
__device__ __forceinline__ uint32_t fxt1_color15(uint32_t c565) { return (c565 & 31u) | (((c565 >> 6) & 31u) << 5) | ((c565 >> 11) << 10); }
__device__ __forceinline__ fxt1_half fxt1_half_of(const uint2 bc1) {
    const uint32_t l = bc1.x & 0xFFFFu, h = bc1.x >> 16;
    fxt1_half f = { fxt1_color15(l), fxt1_color15(h), (h >> 5) & 1u, map_selectors(bc1.y, 0x9Cu) };   // BC1's codes 0, 1, 2, 3 -> the linear order 0, 3, 1, 2
    const uint32_t g0 = (l >> 5) & 1u;
    if (((f.sels >> 1) & 1u) != (g0 ^ f.g1)) {
        const uint32_t t = f.c0;
        f.c0 = f.c1; f.c1 = t; f.g1 = g0; f.sels = ~f.sels;
    }
    return f;
}
// has_right false: the lone left half of an odd row fills both colour pairs and repeats its right column across the other half's selectors
__device__ __forceinline__ uint4 to_fxt1(const uint2 left, const uint2 right, bool has_right) {
    const fxt1_half a = fxt1_half_of(left);
    fxt1_half b = fxt1_half_of(right);
    if (!has_right) {
        b = a;
        b.sels = ((a.sels >> 6) & 0x03030303u) * 0x55u;
    }
    const uint64_t hi = (uint64_t)a.c0 | ((uint64_t)a.c1 << 15) | ((uint64_t)b.c0 << 30) | ((uint64_t)b.c1 << 45) | ((uint64_t)(a.g1 | (b.g1 << 1)) << 61) | (1ull << 63);
    return make_uint4(a.sels, b.sels, (uint32_t)hi, (uint32_t)(hi >> 32));
}

// ---- one block of a launch: the range check, the gathers, the conversion, the store. The index pointers are the image's, `out` is where the image's output begins, `i`
// the source block's place in the image's raster order, nbx the image's width in source blocks. The alpha pointers (both null: no alpha slice) are read by PVRTC2 RGBA
// alone, and there a bad alpha index is the block's failure too. ATC RGB / PVRTC2 RGB / RGBA: one uint2 at out[i]. FXT1: the lane of an even
// block column builds the 16-byte block of its own source block and its right neighbour's (none at the end of an odd row) and stores one uint4 at row-major place
// (bx / 2, by) of rows that hold (nbx + 1) / 2 blocks; an odd column's lane does nothing. -> how many source blocks had an index past its palette: such an index
// never reaches a gather, and the output block it belongs to is zero bytes.
enum : uint32_t { VF_ATC_RGB = 11, VF_FXT1_RGB = 17, VF_PVRTC2_4_RGB = 18, VF_PVRTC2_4_RGBA = 19 };   // the reference's transcoder_texture_format values
struct vendor_format_inputs {
    const uint32_t *endpoint_palette, *selector_palette, *bc1_endpoints5, *bc1_endpoints6, *atc_tables;   // the BC1 tables: FXT1 only; atc_tables: the other two
    uint32_t n_endpoints, n_selectors;
};
template <uint32_t TARGET>
__device__ __forceinline__ uint32_t vendor_format_block(const vendor_format_inputs& a, const uint16_t* endpoint_idx, const uint16_t* selector_idx, const uint16_t* alpha_endpoint_idx,
                                                        const uint16_t* alpha_selector_idx, void* out, uint32_t i, uint32_t nbx) {
    if (TARGET == VF_FXT1_RGB) {
        const uint32_t bx = i % nbx, by = i / nbx;
        if (bx & 1u) return 0u;
        const bool has_right = bx + 1u < nbx;
        const uint32_t ei = endpoint_idx[i], si = selector_idx[i], ej = has_right ? endpoint_idx[i + 1u] : 0u, sj = has_right ? selector_idx[i + 1u] : 0u;
        const bool ok_left = ei < a.n_endpoints && si < a.n_selectors, ok_right = ej < a.n_endpoints && sj < a.n_selectors;
        uint4 o = make_uint4(0u, 0u, 0u, 0u);
        if (ok_left && ok_right) {
            const uint2 left = to_bc1<false>(unpack_entry(a.endpoint_palette[ei]), a.selector_palette[si], a.bc1_endpoints5, a.bc1_endpoints6);
            const uint2 right = has_right ? to_bc1<false>(unpack_entry(a.endpoint_palette[ej]), a.selector_palette[sj], a.bc1_endpoints5, a.bc1_endpoints6) : make_uint2(0u, 0u);
            o = to_fxt1(left, right, has_right);
        }
        ((uint4*)out)[(size_t)by * ((nbx + 1u) / 2u) + bx / 2u] = o;
        return (ok_left ? 0u : 1u) + (ok_right ? 0u : 1u);
    }
    const uint32_t ei = endpoint_idx[i], si = selector_idx[i];
    bool ok = ei < a.n_endpoints && si < a.n_selectors;
    const bool has_alpha = TARGET == VF_PVRTC2_4_RGBA && alpha_endpoint_idx != nullptr;   // PVRTC2 RGBA of an image without an alpha slice is PVRTC2 RGB
    uint32_t aei = 0, asi = 0;
    if (has_alpha) {
        aei = alpha_endpoint_idx[i]; asi = alpha_selector_idx[i];
        ok = ok && aei < a.n_endpoints && asi < a.n_selectors;
    }
    uint2 o = make_uint2(0u, 0u);
    if (ok) {
        const etc1s_entry e = unpack_entry(a.endpoint_palette[ei]);
        const uint32_t sel = a.selector_palette[si];
        if (has_alpha) o = to_pvrtc2_rgba(e, sel, unpack_entry(a.endpoint_palette[aei]), a.selector_palette[asi], a.atc_tables);
        else o = TARGET == VF_ATC_RGB ? to_atc(e, sel, a.atc_tables) : to_pvrtc2_rgb(e, sel, a.atc_tables);
    }
    ((uint2*)out)[i] = o;
    return ok ? 0u : 1u;
}

}  // namespace bu
