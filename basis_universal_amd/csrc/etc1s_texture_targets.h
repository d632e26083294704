// etc1s_texture_targets.h -- the per-block conversions of the 16-byte targets of etc1s_transcode_kernels.hip, which includes this after its own helpers and tables:
// EAC A8 (the alpha half of ETC2 RGBA) and BC7 mode 5 with the reference's chroma filter and the small mode-5 encoder under it (transcoder/basisu_transcoder.cpp:
// convert_etc1s_to_etc2_eac_a8 4786, convert_etc1s_to_bc7_m5_color 4310, convert_etc1s_to_bc7_m5_alpha 4472, chroma_filter_bc7_mode5 4641, encode_bc7_mode_5_block
// 8102). One lane per block, everything in registers: the 16 pixels of a filtered block are 16 packed words, their 16 weights one 32-bit word, and every loop is
// unrolled so that no array is indexed by a run-time value.
// The filter and the encoder are binary32 in the reference's operation order. The whole library is built with -ffp-contract=off (no fused multiply-add is formed)
// and without any fast-math flag, and hipcc rounds `/` on float correctly unless told otherwise (-fhip-fp32-correctly-rounded-divide-sqrt, which the Makefile states);
// nothing here calls fmaf.
#pragma once

namespace bu {

enum : uint32_t { kBc7ColorEntries = 8 * 32 * 6 * 10, kBc7TableWords = kBc7ColorEntries + 128 };   // the colour look-up, then the encoder's 128 midpoints as float bits

// which selectors a block uses: bit s set; low / high the lowest and highest of them
__device__ __forceinline__ uint32_t selectors_used(uint32_t sel, uint32_t& low, uint32_t& high) {
    uint32_t used = 0;
#pragma unroll
    for (uint32_t p = 0; p < 16; p++) used |= 1u << ((sel >> (2u * p)) & 3u);
    low = (uint32_t)__ffs((int)used) - 1u;
    high = 31u - (uint32_t)__clz((int)used);
    return used;
}
// the red value of an entry under selector s (the alpha look-ups read the first channel)
__device__ __forceinline__ uint32_t red_of(const etc1s_entry& e, uint32_t s) { return (uint32_t)clamp255(scale5((int)e.r5) + inten_delta((int)e.table, (int)s)); }

// EAC A8: byte 0 base, byte 1 table | multiplier << 4, then 48 bits big endian, the 3-bit code of texel (x, y) at bit 45 - 3 (x * 4 + y). A block of one selector
// is base = its value under table 13, multiplier 1, every code 4 (modifier 0); any other block reads base, table, multiplier and the four codes from the look-up.
// `lookup` is EAC A8's table or, for EAC R11 (etc1s_block_format_targets.h), the one searched on 11 bits: the two formats share the layout and the route.
__device__ __forceinline__ uint2 eac_from_lookup(const etc1s_entry& e, uint32_t sel, const unsigned int* lookup) {
    uint32_t low, high;
    selectors_used(sel, low, high);
    uint32_t v = red_of(e, low) | ((13u | (1u << 4)) << 8) | (04444u << 16);
    if (low != high) v = lookup[(e.table * 32u + e.r5) * 4u + ke_alpha_range_index[low * 4u + high]];
    uint64_t bits = 0;
#pragma unroll
    for (uint32_t y = 0; y < 4; y++)
#pragma unroll
        for (uint32_t x = 0; x < 4; x++) bits |= (uint64_t)((v >> (16u + 3u * texel_selector(sel, x, y))) & 7u) << (45u - 3u * (x * 4u + y));
    return make_uint2((v & 0xFFFFu) | ((uint32_t)((bits >> 40) & 255u) << 16) | ((uint32_t)((bits >> 32) & 255u) << 24), __builtin_bswap32((uint32_t)bits));
}
__device__ __forceinline__ uint2 to_eac_a8(const etc1s_entry& e, uint32_t sel) { return eac_from_lookup(e, sel, ke_eac_a8); }
__device__ __forceinline__ uint2 opaque_eac_a8() { return make_uint2(255u | ((13u | (1u << 4)) << 8) | (0x92u << 16) | (0x49u << 24), 0x24499224u); }

// ---- BC7 mode 5. The block as two 64-bit halves. Low: mode bit 5, rotation 0, r0 r1 g0 g1 b0 b1 (7 bits each) from bit 8, a0 at bit 50, the low 6 bits of a1 at 58.
// High: the top 2 bits of a1, 31 bits of colour indices from bit 2, 31 bits of alpha indices from bit 33; texel 0 has one bit in each, its top bit is implied 0.
struct bc7_m5 { uint64_t lo, hi; };

// 16 two-bit indices (texel p at bits 2 p, texel 0 below 2) -> the 31 bits of the block
__device__ __forceinline__ uint64_t m5_index_bits(uint32_t idx2) { return (uint64_t)((idx2 & 1u) | ((idx2 >> 2) << 1)); }
// endpoints r | g << 8 | b << 16 of 7 bits each; when texel 0's index has its top bit set the endpoints trade places and every index is inverted
__device__ __forceinline__ bc7_m5 pack_m5_rgb(uint32_t l, uint32_t h, uint32_t idx2) {
    if (idx2 & 2u) { const uint32_t t = l; l = h; h = t; idx2 = ~idx2; }
    bc7_m5 b;
    b.lo = 32u | ((uint64_t)(l & 127u) << 8) | ((uint64_t)(h & 127u) << 15) | ((uint64_t)((l >> 8) & 127u) << 22) | ((uint64_t)((h >> 8) & 127u) << 29) |
           ((uint64_t)((l >> 16) & 127u) << 36) | ((uint64_t)((h >> 16) & 127u) << 43) | (255ull << 50) | (63ull << 58);
    b.hi = 3u | (m5_index_bits(idx2) << 2);
    return b;
}
// the 2-bit index of every texel from a word that holds the index of ETC1S selector s at bits 2 s
__device__ __forceinline__ uint32_t map_selectors(uint32_t sel, uint32_t map) {
    uint32_t idx2 = 0;
#pragma unroll
    for (uint32_t p = 0; p < 16; p++) idx2 |= ((map >> (2u * ((sel >> (2u * p)) & 3u))) & 3u) << (2u * p);
    return idx2;
}
// a block of two selectors: `low` -> index 0, the other -> index 3
__device__ __forceinline__ uint32_t two_selector_map(uint32_t low) { return 0xFFu & ~(3u << (2u * low)); }
__device__ __forceinline__ uint32_t solid7(uint32_t c, uint32_t which) {   // which: 0 hi, 1 lo
    return (uint32_t)ke_bc7_solid[(c & 255u) * 2u + which] | ((uint32_t)ke_bc7_solid[((c >> 8) & 255u) * 2u + which] << 8) | ((uint32_t)ke_bc7_solid[(c >> 16) * 2u + which] << 16);
}

// the opaque block of a colour-slice block: one selector -> the endpoints whose index-1 colour is nearest, every index 1; two -> block truncation, the two colours are
// the endpoints; else per channel the look-up's endpoints of the mapping with the least summed error, first on ties (as to_bc1)
__device__ __forceinline__ bc7_m5 to_bc7_m5_color(const etc1s_entry& e, uint32_t sel, const uint32_t* table) {
    uint32_t low, high;
    const uint32_t used = selectors_used(sel, low, high), n = (uint32_t)__popc(used);
    uint32_t colors[4];
    block_colors(e, colors);
    if (n == 1) {
        const uint32_t c = pick4(colors, low);
        return pack_m5_rgb(solid7(c, 1), solid7(c, 0), 0x55555555u);
    }
    if (n == 2) return pack_m5_rgb((pick4(colors, low) >> 1) & 0x7F7F7Fu, (pick4(colors, high) >> 1) & 0x7F7F7Fu, map_selectors(sel, two_selector_map(low)));
    const uint32_t range = ke_bc1_range_index[low * 4 + high];
    const uint32_t* tr = &table[((e.table * 32u + e.r5) * 6u + range) * 10u];
    const uint32_t* tg = &table[((e.table * 32u + e.g5) * 6u + range) * 10u];
    const uint32_t* tb = &table[((e.table * 32u + e.b5) * 6u + range) * 10u];
    uint32_t best_err = 0xFFFFFFFFu, best = 0, br = 0, bg = 0, bb = 0;
#pragma unroll
    for (uint32_t m = 0; m < 10; m++) {
        const uint32_t r = tr[m], g = tg[m], b = tb[m], err = (r >> 16) + (g >> 16) + (b >> 16);
        if (err < best_err) { best_err = err; best = m; br = r; bg = g; bb = b; }
    }
    const unsigned char* mp = &ke_bc1_mappings[best * 4u];
    const uint32_t map = (uint32_t)mp[0] | ((uint32_t)mp[1] << 2) | ((uint32_t)mp[2] << 4) | ((uint32_t)mp[3] << 6);
    return pack_m5_rgb((br & 127u) | ((bg & 127u) << 8) | ((bb & 127u) << 16), ((br >> 8) & 127u) | (((bg >> 8) & 127u) << 8) | (((bb >> 8) & 127u) << 16),
                       map_selectors(sel, map));
}

// the alpha fields of a block from an alpha-slice block; a block of one selector leaves the index bits as they are (zero)
__device__ __forceinline__ void bc7_m5_alpha(bc7_m5& b, const etc1s_entry& e, uint32_t sel) {
    uint32_t low, high;
    const uint32_t used = selectors_used(sel, low, high), n = (uint32_t)__popc(used);
    uint32_t a0 = red_of(e, low), a1 = a0;
    if (n > 1) {
        uint32_t map = two_selector_map(low);
        a1 = red_of(e, high);
        if (n > 2) {
            const uint32_t v = ke_bc7_alpha[(e.table * 32u + e.r5) * 6u + ke_bc1_range_index[low * 4 + high]];
            a0 = v & 255u; a1 = (v >> 8) & 255u; map = v >> 16;
        }
        uint32_t idx2 = map_selectors(sel, map);
        if (idx2 & 2u) { const uint32_t t = a0; a0 = a1; a1 = t; idx2 = ~idx2; }
        b.hi = (b.hi & 0x1FFFFFFFFull) | (m5_index_bits(idx2) << 33);
    }
    b.lo = (b.lo & ((1ull << 50) - 1ull)) | ((uint64_t)a0 << 50) | ((uint64_t)(a1 & 63u) << 58);
    b.hi = (b.hi & ~3ull) | (a1 >> 6);
}

// ---- the mode-5 encoder under the chroma filter
__device__ __forceinline__ uint32_t from_7(uint32_t v) { return (v << 1) | (v >> 6); }
__device__ __forceinline__ uint32_t bc7_interp2(uint32_t l, uint32_t h, uint32_t w) {   // weights 0, 21, 43, 64 of 64
    const uint32_t k = w == 0 ? 0u : (w == 1 ? 21u : (w == 2 ? 43u : 64u));
    return (l * (64u - k) + h * k + 32u) >> 6;
}
// The midpoint between 7-bit endpoint i and i + 1 on the 0..1 scale, in the float operations of the reference's init; etc1s_build_bc7_tables_kernel stores the 128
// of them behind the colour look-up.
__device__ __forceinline__ float mode5_midpoint(uint32_t i) {
    uint32_t vl = i << 1; vl |= vl >> 7;
    uint32_t vh = (i + 1u < 127u ? i + 1u : 127u) << 1; vh |= vh >> 7;
    const float lo = (float)vl / 255.0f, hi = (float)vh / 255.0f;
    return i == 127u ? 1e+15f : (lo + hi) / 2.0f;
}
__device__ __forceinline__ int to_7(float c, const float* mid) {
    int vl = (int)(c * 127.0f);
    vl += (c > mid[vl]);
    return vl < 0 ? 0 : (vl > 127 ? 127 : vl);
}
__device__ __forceinline__ uint32_t to_7_rgb(uint32_t c, const float* mid) {   // an 8-bit colour r | g << 8 | b << 16
    return (uint32_t)to_7((float)(c & 255u) * (1.0f / 255.0f), mid) | ((uint32_t)to_7((float)((c >> 8) & 255u) * (1.0f / 255.0f), mid) << 8) |
           ((uint32_t)to_7((float)(c >> 16) * (1.0f / 255.0f), mid) << 16);
}
// every pixel's index between the endpoints l, h (7 bits per channel): its place along the endpoint axis against the three midpoints of the four colours
__device__ __forceinline__ uint32_t eval_weights(const uint32_t px[16], uint32_t l, uint32_t h) {
    int c[4][3];
#pragma unroll
    for (uint32_t k = 0; k < 3; k++) {
        const uint32_t l8 = from_7((l >> (8u * k)) & 127u), h8 = from_7((h >> (8u * k)) & 127u);
#pragma unroll
        for (uint32_t i = 0; i < 4; i++) c[i][k] = (int)(bc7_interp2(l8, h8, i) & 255u);
    }
    int ar = c[3][0] - c[0][0], ag = c[3][1] - c[0][1], ab = c[3][2] - c[0][2];
    int dots[4];
#pragma unroll
    for (uint32_t i = 0; i < 4; i++) dots[i] = c[i][0] * ar + c[i][1] * ag + c[i][2] * ab;
    const int t0 = dots[0] + dots[1], t1 = dots[1] + dots[2], t2 = dots[2] + dots[3];
    ar *= 2; ag *= 2; ab *= 2;
    uint32_t w = 0;
#pragma unroll
    for (uint32_t i = 0; i < 16; i++) {
        const int d = (int)(px[i] & 255u) * ar + (int)((px[i] >> 8) & 255u) * ag + (int)(px[i] >> 16) * ab;
        w |= (uint32_t)((d > t0) + (d >= t1) + (d >= t2)) << (2u * i);
    }
    return w;
}
__device__ __forceinline__ int lerp_8bit(int a, int b, int s) { const int t = (b - a) * s + 128; return a + ((t + (t >> 8)) >> 8); }
__device__ __forceinline__ float clamp01(float v) { return v < 0.0f ? 0.0f : (v > 1.0f ? 1.0f : v); }

// 16 opaque pixels (r | g << 8 | b << 16) -> the block. All equal: the solid endpoints. Little variance (the largest channel variance, times 16, under 160): the
// endpoints at 16/255 and 239/255 of each channel's range. Else the two pixels at the ends of the principal axis (one power iteration from the covariance, the pixel's
// number in the low four bits of its dot so that ties go to the lower pixel for the minimum and the higher for the maximum), then one least-squares pass over the
// weights those give, unless its 2x2 system is singular.
__device__ __forceinline__ bc7_m5 encode_bc7_mode5(const uint32_t px[16], const float* mid) {
    int total[3] = { 0, 0, 0 }, mn[3] = { 255, 255, 255 }, mx[3] = { 0, 0, 0 };
#pragma unroll
    for (uint32_t i = 0; i < 16; i++)
#pragma unroll
        for (uint32_t k = 0; k < 3; k++) {
            const int v = (int)((px[i] >> (8u * k)) & 255u);
            total[k] += v; mn[k] = v < mn[k] ? v : mn[k]; mx[k] = v > mx[k] ? v : mx[k];
        }
    if (mn[0] == mx[0] && mn[1] == mx[1] && mn[2] == mx[2]) {
        const uint32_t c = (uint32_t)mn[0] | ((uint32_t)mn[1] << 8) | ((uint32_t)mn[2] << 16);
        return pack_m5_rgb(solid7(c, 1), solid7(c, 0), 0x55555555u);
    }
    const int mean[3] = { (total[0] + 8) >> 4, (total[1] + 8) >> 4, (total[2] + 8) >> 4 };
    int icov[6] = { 0, 0, 0, 0, 0, 0 };   // rr rg rb gg gb bb
#pragma unroll
    for (uint32_t i = 0; i < 16; i++) {
        const int r = (int)(px[i] & 255u) - mean[0], g = (int)((px[i] >> 8) & 255u) - mean[1], b = (int)(px[i] >> 16) - mean[2];
        icov[0] += r * r; icov[1] += r * g; icov[2] += r * b; icov[3] += g * g; icov[4] += g * b; icov[5] += b * b;
    }
    int max_var = icov[0] > icov[3] ? icov[0] : icov[3];
    max_var = max_var > icov[5] ? max_var : icov[5];
    if (max_var < 160) {
        uint32_t l = 0, h = 0;
#pragma unroll
        for (uint32_t k = 0; k < 3; k++) {
            l |= (uint32_t)to_7((float)lerp_8bit(mn[k], mx[k], 16) * (1.0f / 255.0f), mid) << (8u * k);
            h |= (uint32_t)to_7((float)lerp_8bit(mn[k], mx[k], 239) * (1.0f / 255.0f), mid) << (8u * k);
        }
        return pack_m5_rgb(l, h, eval_weights(px, l, h));
    }
    float cov[6];
#pragma unroll
    for (uint32_t i = 0; i < 6; i++) cov[i] = (float)icov[i];
    const float sc = 1.0f / (float)max_var;
    const float wx = sc * cov[0], wy = sc * cov[3], wz = sc * cov[5];
    const float alt_r = cov[0] * wx + cov[1] * wy + cov[2] * wz;
    const float alt_g = cov[1] * wx + cov[3] * wy + cov[4] * wz;
    const float alt_b = cov[2] * wx + cov[4] * wy + cov[5] * wz;
    int axis_r = 306, axis_g = 601, axis_b = 117;
    float k = fabsf(alt_r) > fabsf(alt_g) ? fabsf(alt_r) : fabsf(alt_g);
    k = k > fabsf(alt_b) ? k : fabsf(alt_b);
    if (k >= .0000125f) {
        const float m = 2048.0f / k;
        axis_r = (int)(alt_r * m); axis_g = (int)(alt_g * m); axis_b = (int)(alt_b * m);
    }
    axis_r = (int)((uint32_t)axis_r << 4); axis_g = (int)((uint32_t)axis_g << 4); axis_b = (int)((uint32_t)axis_b << 4);
    int low_dot = 0x7FFFFFFF, high_dot = (int)0x80000000;
    uint32_t low_px = 0, high_px = 0;   // the colour travels with its dot
#pragma unroll
    for (uint32_t i = 0; i < 16; i++) {
        const int d = (((int)(px[i] & 255u) * axis_r + (int)((px[i] >> 8) & 255u) * axis_g + (int)(px[i] >> 16) * axis_b) & ~0xF) + (int)i;
        if (d < low_dot) { low_dot = d; low_px = px[i]; }
        if (d > high_dot) { high_dot = d; high_px = px[i]; }
    }
    uint32_t l = to_7_rgb(low_px, mid), h = to_7_rgb(high_px, mid);
    uint32_t w = eval_weights(px, l, h);
    // least squares for both endpoints under these weights: accum holds 9 w^2, 9 w (1 - w), 9 (1 - w)^2 summed, a byte each
    uint32_t accum = 0, uq[3] = { 0, 0, 0 };
#pragma unroll
    for (uint32_t i = 0; i < 16; i++) {
        const uint32_t s = (w >> (2u * i)) & 3u;
        accum += s == 0 ? 0x000009u : (s == 1 ? 0x010204u : (s == 2 ? 0x040201u : 0x090000u));
        uq[0] += s * (px[i] & 255u); uq[1] += s * ((px[i] >> 8) & 255u); uq[2] += s * (px[i] >> 16);
    }
    const float z00 = (float)((accum >> 16) & 0xFFu), z10 = (float)((accum >> 8) & 0xFFu), z11 = (float)(accum & 0xFFu), z01 = z10;
    float det = z00 * z11 - z01 * z10;
    if (!(fabsf(det) < 1e-8f)) {
        det = (3.0f / 255.0f) / det;
        const float iz00 = z11 * det, iz01 = -z01 * det, iz10 = -z10 * det, iz11 = z00 * det;
        l = 0; h = 0;
#pragma unroll
        for (uint32_t c = 0; c < 3; c++) {
            const int q10 = total[c] * 3 - (int)uq[c];
            h |= (uint32_t)to_7(clamp01(iz00 * (float)uq[c] + iz01 * (float)q10), mid) << (8u * c);
            l |= (uint32_t)to_7(clamp01(iz10 * (float)uq[c] + iz11 * (float)q10), mid) << (8u * c);
        }
        w = eval_weights(px, l, h);
    }
    return pack_m5_rgb(l, h, w);
}

// Co and Cg of an endpoint-palette entry's base colour
__device__ __forceinline__ float2 entry_cocg(uint32_t entry) {
    const float r = (float)scale5((int)(entry & 31u)), g = (float)scale5((int)((entry >> 8) & 31u)), b = (float)scale5((int)((entry >> 16) & 31u));
    return make_float2((r * 0.5f + g * 0.0f) + b * -0.5f, (r * -0.25f + g * 0.5f) + b * -0.25f);
}

// The chroma filter on block (bx, by), whose opaque block `b` the colour conversion has just made. It reads the endpoint indices of the 3x3 blocks around it, clamped
// to the image -- never a neighbour's output, so one lane does all of it. If none of them differs from the centre by more than 10 in Co or Cg, or the 16 luma values
// of `b` have a variance under 3, `b` stays. Else every pixel becomes its luma plus the chroma interpolated bilinearly between the four blocks nearest it (taps at the
// block centres), and the block is encoded again. A neighbour whose index is past the palette contributes the centre's own entry: it cannot trigger the filter, and it
// pulls the interpolation towards the centre. (The reference would have failed the file; here that neighbour is itself zero-filled and counted.)
// The clamped 3x3 holds every in-image neighbour, and a clamped duplicate is the centre or one of them, so testing all nine is the reference's test.
__device__ __forceinline__ bc7_m5 bc7_chroma_filter(bc7_m5 b, const uint32_t* endpoint_palette, uint32_t n_endpoints, const uint16_t* endpoint_idx, uint32_t centre_entry,
                                                    uint32_t bx, uint32_t by, uint32_t nbx, uint32_t nby, const float* mid) {
    float2 cc[3][3];
    bool differs = false;
    const float2 centre = entry_cocg(centre_entry);
#pragma unroll
    for (int dy = 0; dy < 3; dy++)
#pragma unroll
        for (int dx = 0; dx < 3; dx++) {
            const uint32_t x = dx == 0 ? (bx ? bx - 1u : 0u) : (dx == 1 ? bx : (bx + 1u < nbx ? bx + 1u : nbx - 1u));
            const uint32_t y = dy == 0 ? (by ? by - 1u : 0u) : (dy == 1 ? by : (by + 1u < nby ? by + 1u : nby - 1u));
            const uint32_t ni = endpoint_idx[y * nbx + x];
            cc[dy][dx] = (dx == 1 && dy == 1) || ni >= n_endpoints ? centre : entry_cocg(endpoint_palette[ni]);
            differs = differs || fabsf(cc[dy][dx].x - centre.x) > 10.0f || fabsf(cc[dy][dx].y - centre.y) > 10.0f;
        }
    if (!differs) return b;
    float y_vals[4];
#pragma unroll
    for (uint32_t i = 0; i < 4; i++) {
        const uint32_t cr = bc7_interp2(from_7((uint32_t)(b.lo >> 8) & 127u), from_7((uint32_t)(b.lo >> 15) & 127u), i);
        const uint32_t cg = bc7_interp2(from_7((uint32_t)(b.lo >> 22) & 127u), from_7((uint32_t)(b.lo >> 29) & 127u), i);
        const uint32_t cb = bc7_interp2(from_7((uint32_t)(b.lo >> 36) & 127u), from_7((uint32_t)(b.lo >> 43) & 127u), i);
        y_vals[i] = (float)cr * .25f + (float)cg * .5f + (float)cb * .25f;
    }
    const uint32_t idx2 = (uint32_t)(((b.hi >> 2) & 1u) | (((b.hi >> 3) & 0x3FFFFFFFu) << 2));   // texel p's index at bits 2 p again
    float ys[16], y_sum = 0.0f, y_sum_sq = 0.0f;
#pragma unroll
    for (uint32_t i = 0; i < 16; i++) {
        const uint32_t s = (idx2 >> (2u * i)) & 3u;
        const float y = (s & 2u) ? ((s & 1u) ? y_vals[3] : y_vals[2]) : ((s & 1u) ? y_vals[1] : y_vals[0]);
        ys[i] = y;
        y_sum += y;
        y_sum_sq += y * y;
    }
    const float S = 1.0f / 16.0f, y_mean = y_sum * S;
    if ((y_sum_sq * S) - y_mean * y_mean < 3.0f) return b;
    uint32_t px[16];
#pragma unroll
    for (int py = 0; py < 4; py++) {
        const int uy = py < 2 ? 0 : 1;
        const float fy = ((float)((py + 2) & 3) + .5f) * (1.0f / 4.0f);
#pragma unroll
        for (int pxx = 0; pxx < 4; pxx++) {
            const int ux = pxx < 2 ? 0 : 1;
            const float fx = ((float)((pxx + 2) & 3) + .5f) * (1.0f / 4.0f);
            const float2 a = cc[uy][ux], bb = cc[uy][ux + 1], c = cc[uy + 1][ux], d = cc[uy + 1][ux + 1];
            const float ab_x = a.x + (bb.x - a.x) * fx, cd_x = c.x + (d.x - c.x) * fx, co = ab_x + (cd_x - ab_x) * fy;
            const float ab_y = a.y + (bb.y - a.y) * fx, cd_y = c.y + (d.y - c.y) * fx, cg = ab_y + (cd_y - ab_y) * fy;
            const float y = ys[py * 4 + pxx];
            float r = (y * 1.0f + co * 1.0f) + cg * -1.0f, g = (y * 1.0f + co * 0.0f) + cg * 1.0f, bl = (y * 1.0f + co * -1.0f) + cg * -1.0f;
            r = r < 0.0f ? 0.0f : (r > 255.0f ? 255.0f : r);
            g = g < 0.0f ? 0.0f : (g > 255.0f ? 255.0f : g);
            bl = bl < 0.0f ? 0.0f : (bl > 255.0f ? 255.0f : bl);
            px[py * 4 + pxx] = (uint32_t)(int)(.5f + r) | ((uint32_t)(int)(.5f + g) << 8) | ((uint32_t)(int)(.5f + bl) << 16);
        }
    }
    return encode_bc7_mode5(px, mid);
}

}  // namespace bu
